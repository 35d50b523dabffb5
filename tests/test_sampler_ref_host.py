"""The yardsticks of tests/test_gpu_sampler_edges.py, checked without a GPU: the Philox of oracle/sampler.py against the Random123
known answers, its MT19937 against NumPy's own generator (values and state), and every case of tests/helpers/sampler_cases.py
against the property it is named for -- from the restatements alone."""
import numpy as np
import pytest

from oracle import sampler as osampler
from tests.helpers import sampler_cases as sc


# ----------------------------------------------------------------------------------------------------------- the generators
@pytest.mark.parametrize("ctr,key,exp", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, exp):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert osampler.philox4x32_10(*ctr, *key) == exp


def test_philox_stream_words_are_the_blocks_in_order():
    """Sample n's stream: counter (n_lo, n_hi, block, stream id), key (seed_lo, seed_hi), a block's four words in order."""
    n, seed = 2 ** 40 + 7, 2 ** 32 + 5
    for stream in (0, 1):
        ps = osampler._PhiloxStream(n, seed, stream=stream)
        got = [ps.next() for _ in range(12)]
        exp = [w for block in range(3) for w in osampler.philox4x32_10(7, 2 ** 8, block, stream, 5, 1)]
        assert got == exp and ps.words == 12
    assert osampler._PhiloxStream(n, seed).stream == 0                     # the BPR sampler's id is the default


@pytest.mark.parametrize("seed", [1, 42, 2 ** 32 - 1])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_mt19937_equals_numpy_values_and_state(seed, n):
    """MT19937(seed).randint(n) against np.random.RandomState(seed).randint(n) over more than two twists, then the state:
    NumPy is the yardstick of the device generator's state in the GPU test.  n = 1 draws no word on either side."""
    mine, theirs = osampler.MT19937(seed), np.random.RandomState(seed)
    twists, twist = [0], mine._twist

    def counting_twist():
        twists[0] += 1
        twist()
    mine._twist = counting_twist
    draws = 1500                                                           # a word or more each: the third block is reached
    got = [mine.randint(n) for _ in range(draws)]
    exp = [int(theirs.randint(n)) for _ in range(draws)]
    assert got == exp
    key, pos = theirs.get_state()[1:3]
    assert mine.pos == pos and np.array_equal(mine.mt, key)
    if n == 1:
        assert pos == 624 and twists[0] == 0                               # not one word taken
    else:
        assert twists[0] >= 3


def test_mt19937_randint_refuses_an_empty_range_like_numpy():
    with pytest.raises(ValueError):
        np.random.RandomState(1).randint(0)
    with pytest.raises(ValueError):
        osampler.MT19937(1).randint(0)


# ------------------------------------------------------------------------------------------------------------- Philox cases
def test_case_builders_refuse_a_data_set_nobody_can_finish_on():
    with pytest.raises(ValueError):
        sc.philox_case("empty_and_full", [[], [0, 1, 2]], 3, 10)
    with pytest.raises(ValueError):
        sc.philox_case("shard_all_positive", [[1, 4, 5], [2, 4, 5]], 8, 10, shard=(4, 6))
    with pytest.raises(ValueError):
        sc.mt_case("empty_list", [[1], []], 4, (5,))


@pytest.mark.parametrize("name", sc.PHILOX_NAMES)
def test_every_philox_case_has_a_user_to_finish_on(name):
    c = sc.philox_cases()[name]
    rows = sc.rows_of(c)
    assert all(r == sorted(set(r)) for r in rows)                          # CSR rows ascending, no duplicates
    assert sc.finishing_users(rows, c.n_items, c.shard)
    assert c.n <= 4000 and c.n_users <= 400
    if c.shard is not None:
        assert c.n <= 1500


def _check_triplets(c, u, i, j, lo, hi):
    rows = [set(r) for r in sc.rows_of(c)]
    for uu, ii, jj in zip(u.tolist(), i.tolist(), j.tolist()):
        assert ii in rows[uu] and jj not in rows[uu] and lo <= jj < hi


@pytest.mark.parametrize("name", sc.PHILOX_NAMES)
def test_restated_bpr_samples_are_valid(name):
    c = sc.philox_cases()[name]
    u, i, j, draws = sc.bpr_expected(name)
    lo, hi = c.shard if c.shard else (0, c.n_items)
    _check_triplets(c, u, i, j, lo, hi)
    assert draws.shape == (c.n,) and draws.min() >= 3


@pytest.mark.parametrize("ratio", [None] + list(sc.RATIOS))
@pytest.mark.parametrize("name", sc.UNSHARDED_NAMES)
def test_restated_pointwise_samples_are_valid(name, ratio):
    c = sc.philox_cases()[name]
    u, i, y, draws = sc.pw_expected(name, ratio)
    rows = [set(r) for r in sc.rows_of(c)]
    assert set(np.unique(y).tolist()) <= {0.0, 1.0}
    for uu, ii, yy in zip(u.tolist(), i.tolist(), y.tolist()):
        assert (ii in rows[uu]) == (yy == 1.0) and 0 <= ii < c.n_items
    if c.n >= 255 and ratio != 255:
        assert 0 < y.sum() < c.n                                           # both sides of the coin occur


def test_launch_and_user_count_cases():
    cs = sc.philox_cases()
    assert [cs["launch_n%d" % n].n for n in (1, 255, 256, 257)] == [1, 255, 256, 257]
    assert [cs["users_%d" % n].n_users for n in (1, 2, 64, 65)] == [1, 2, 64, 65]
    # bounded(1) takes a word: with U = 1 a BPR sample still makes its three draws or more
    assert sc.bpr_expected("users_1")[3].min() >= 3


def test_row_length_case_has_rows_of_0_1_Im1_and_I_and_passes_over_the_unusable():
    c = sc.philox_cases()["row_lengths"]
    lens = [len(r) for r in sc.rows_of(c)]
    assert c.n_items == 33 and {0, 1, c.n_items - 1, c.n_items} <= set(lens) and any(1 < k < c.n_items - 1 for k in lens)
    usable = {u for u, k in enumerate(lens) if 0 < k < c.n_items}
    for exp in (sc.bpr_expected(c.name), sc.pw_expected(c.name), sc.pw_expected(c.name, 4)):
        assert set(exp[0].tolist()) == usable                              # every usable user occurs, no other
    u, i, j, draws = sc.bpr_expected(c.name)
    assert (draws > 3).any()                                               # a user was drawn again in some stream
    full_minus_one = lens.index(c.n_items - 1)
    only_negative = (set(range(c.n_items)) - set(sc.rows_of(c)[full_minus_one])).pop()
    assert (u == full_minus_one).any() and set(j[u == full_minus_one].tolist()) == {only_negative}


def test_signature_cases():
    c = sc.philox_cases()["sig_full"]
    row0 = sc.rows_of(c)[0]
    assert len(row0) > sc.SIG_BITS and {sc.sig_bit(x) for x in row0} == set(range(sc.SIG_BITS))
    assert (sc.bpr_expected(c.name)[0] == 0).any() and (sc.pw_expected(c.name)[0] == 0).any()
    c = sc.philox_cases()["sig_one_bit"]
    rows = sc.rows_of(c)
    bits = [{sc.sig_bit(x) for x in r} for r in rows]
    assert all(len(b) == 1 for b in bits)
    # a negative that hits the row's one signature bit and is no positive comes out of both samplers
    u, _, j, _ = sc.bpr_expected(c.name)
    assert any(sc.sig_bit(jj) in bits[uu] for uu, jj in zip(u.tolist(), j.tolist()))
    u, i, y, _ = sc.pw_expected(c.name)
    assert any(yy == 0.0 and sc.sig_bit(ii) in bits[uu] for uu, ii, yy in zip(u.tolist(), i.tolist(), y.tolist()))


def test_catalogue_size_cases():
    cs = sc.philox_cases()
    assert cs["items_64"].n_items == 64 and cs["items_65"].n_items == 65 and cs["items_2p31m2"].n_items == 2 ** 31 - 2
    c = cs["items_2p31m2"]
    assert c.indices.min() == 0 and c.indices.max() == 2 ** 31 - 3 and c.indices.dtype == np.int32
    j = sc.bpr_expected(c.name)[2]
    assert j.min() >= 0 and j.max() > 2 ** 30                              # negatives from the top half of the int32 range


def test_counter_and_seed_cases():
    cs = sc.philox_cases()
    c = cs["counter_carry"]
    assert (c.first, c.n) == (2 ** 32 - 100, 300) and c.first < 2 ** 32 <= c.first + c.n - 1
    assert cs["counter_2p40"].first == 2 ** 40 + 7
    assert cs["seed_high_word"].seed == 2 ** 32 + 5 and cs["seed_all_ones"].seed == 2 ** 64 - 1
    # same data, same n: the high counter word and the high seed word each change the samples
    base = [tuple(a.tolist()) for a in sc.bpr_expected("counter_carry")[:3]]
    for other in ("counter_2p40", "seed_high_word", "seed_all_ones"):
        assert [tuple(a.tolist()) for a in sc.bpr_expected(other)[:3]] != base


@pytest.mark.parametrize("name", sc.SHARDED_NAMES)
def test_sharded_cases_exhaust_their_attempts_and_draw_the_user_again(name):
    """No row of a sharded case is empty or full, so a stream without an exhausted user makes at most 2 + 4096 draws, and one
    that exhausts a user at least 2 + 4096 + 3."""
    c = sc.philox_cases()[name]
    rows = sc.rows_of(c)
    lo, hi = c.shard
    assert all(0 < len(r) < c.n_items for r in rows)
    covered = [u for u, r in enumerate(rows) if set(range(lo, hi)) <= set(r)]
    assert len(covered) >= 2 and len(covered) < c.n_users
    if name == "shard_width1":
        assert hi - lo == 1
    u, i, j, draws = sc.bpr_expected(name)
    exhausted = draws > 2 + sc.ATTEMPTS
    assert exhausted.any() and (~exhausted).any()
    assert (draws[exhausted] >= 2 + sc.ATTEMPTS + 3).all()
    assert not set(u.tolist()) & set(covered)


@pytest.mark.parametrize("what", ["stream_id", "n_hi", "k1"])
def test_cases_tell_a_wrong_counter_or_key_apart(monkeypatch, what):
    """A restatement whose Philox takes the other stream id, forgets the counter's high word or the seed's: the cases notice."""
    class Wrong(osampler._PhiloxStream):
        def __init__(self, n, seed, stream=0):
            super().__init__(n, seed, stream)
            if what == "stream_id":
                self.stream = 1 - stream
            elif what == "n_hi":
                self.n_hi = 0
            else:
                self.k1 = 0

    name = {"stream_id": "launch_n257", "n_hi": "counter_carry", "k1": "seed_high_word"}[what]
    c = sc.philox_cases()[name]
    good_bpr, good_pw = sc.bpr_expected(name)[:3], sc.pw_expected(name)[:3]
    monkeypatch.setattr(osampler, "_PhiloxStream", Wrong)
    bad_bpr = osampler.philox_sample(c.indptr, c.indices, c.n_users, c.n_items, c.seed, c.first, c.n)
    bad_pw = osampler.philox_pointwise_sample(c.indptr, c.indices, c.n_users, c.n_items, c.seed, c.first, c.n)
    assert not all(np.array_equal(a, b) for a, b in zip(good_bpr, bad_bpr))
    assert not all(np.array_equal(a, b) for a, b in zip(good_pw, bad_pw))
    if what == "n_hi":                                                     # the first 100 samples lie below the carry
        assert all(np.array_equal(a[:100], b[:100]) for a, b in zip(good_bpr, bad_bpr))
        assert not np.array_equal(good_bpr[0][100:], bad_bpr[0][100:])


def test_coin_is_one_draw_at_its_documented_place():
    """The fair coin is the top bit of the word after the user's; the ratio coin is bounded(neg_ratio + 1) == 0 there."""
    c = sc.philox_cases()["users_64"]                                      # U = 64: the user draw is exactly one word
    for ratio in (None,) + sc.RATIOS:
        y = sc.pw_expected(c.name, ratio)[2]
        for t in range(c.n):
            ps = osampler._PhiloxStream(c.first + t, c.seed, stream=1)
            ps.next()
            exp = ps.next() >> 31 if ratio is None else int(ps.bounded(ratio + 1) == 0)
            assert y[t] == exp
    fair, ratio1 = sc.pw_expected(c.name)[2], sc.pw_expected(c.name, 1)[2]
    assert not np.array_equal(fair, ratio1)                                # top bit against low bit of the same word
    frac = [sc.pw_expected("sig_one_bit", r)[2].mean() for r in sc.RATIOS]
    assert abs(frac[0] - 1 / 2) < 0.05 and abs(frac[1] - 1 / 5) < 0.04 and 0 < frac[2] < 1 / 256 + 0.01


# ------------------------------------------------------------------------------------------------------------ MT19937 cases
@pytest.mark.parametrize("name", sc.MT_NAMES)
def test_mt_cases_restatement_equals_numpy_triplets_and_state(name):
    c = sc.mt_cases()[name]
    ref = sc.counted_ref_sampler(c)
    for n, (trip, state) in zip(c.calls, sc.mt_numpy(name)):
        got = np.array([ref.sample() for _ in range(n)], dtype=np.int32)
        assert np.array_equal(got, trip)
        assert ref.rng.pos == int(state[624]) and np.array_equal(ref.rng.mt, state[:624])
    exp = sc.mt_expected(name)
    assert len(exp) == len(c.calls) and exp[-1][3] == ref.words()
    assert np.array_equal(exp[-1][0], trip[:, 0]) and np.array_equal(exp[-1][2], trip[:, 2])


def test_mt_block_boundary_case_ends_on_word_624_twice():
    c = sc.mt_cases()["block_boundary"]
    assert c.lists == [[0]] and c.n_items == 2 and c.calls == (299, 309, 1)
    words = [e[3] for e in sc.mt_expected(c.name)]
    assert words[:2] == [624, 1248] and words[2] > 1248
    states = [s for _, s in sc.mt_numpy(c.name)]
    assert int(states[0][624]) == 624 and int(states[1][624]) == 624 and 0 < int(states[2][624]) < 624
    assert not np.array_equal(states[0][:624], states[1][:624])


def test_mt_case_properties():
    exp = sc.mt_expected("many_twists")
    assert exp[0][3] >= 5 * 624
    c = sc.mt_cases()["single_calls"]
    assert c.calls == (1,) * 700 and sc.mt_expected(c.name)[-1][3] > 624
    assert sc.mt_cases()["items_64"].n_items == 64 and sc.mt_cases()["items_65"].n_items == 65
    c = sc.mt_cases()["one_item_list"]
    assert len(c.lists) > 1 and min(len(l) for l in c.lists) == 1
    assert any(l != sorted(l) for l in c.lists)                            # list order is not the CSR's


def test_mt_out_of_words_case_needs_more_words_than_are_provisioned():
    c = sc.mt_out_of_words_case()
    assert all(len(l) == c.n_items - 1 for l in c.lists) and c.n_items == 64 and c.calls == (2000,)
    ref = sc.counted_ref_sampler(c)
    for _ in range(10):
        ref.sample()
    assert ref.words() < 16 * 5 + 8 * 624                                  # the GPU test's two calls of 5 samples have their words
    ref = sc.counted_ref_sampler(c)
    for _ in range(c.calls[0]):
        ref.sample()
    assert ref.words() > 16 * c.calls[0] + 8 * 624


def test_mt_empty_list_case_raises_in_the_reference_restatement():
    c = sc.mt_empty_list_case()
    assert [] in c.lists
    ref = osampler.RefSampler(c.lists, c.n_items, seed=c.seed)
    with pytest.raises(ValueError):
        for _ in range(c.calls[0]):
            ref.sample()
