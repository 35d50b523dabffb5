"""The four device samplers, bit for bit against their CPU restatements at their stream and row edges.

k_bpr_sample (ops.bpr_sample, plain and through the sampler records) against oracle.sampler.philox_sample; k_pw_sample
(ops.pointwise_sample plain and through the records, ops.pointwise_sample_ratio) against oracle.sampler.philox_pointwise_sample;
el_bpr_sample_mt19937 (ops.MtReplaySampler) against oracle.sampler.RefSampler for the triplets and against
np.random.RandomState itself for the 625 words of generator state after every call.  The cases and what they are for:
tests/helpers/sampler_cases.py; that they have those properties: tests/test_sampler_ref_host.py.  Every comparison is
np.array_equal.

Measured on an MI355X: the 140 tests of this file take 3.6 s (pytest's own figure, the restatements included); the slowest are
the two sharded cases whose restatement walks through exhausted users (0.7 s and 0.4 s), the 700 single-sample calls take 0.2 s.
"""
import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from oracle import sampler as osampler
from tests.gpu_util import cpu, dump
from tests.helpers import sampler_cases as sc

pytestmark = pytest.mark.gpu


def _pos(ctx, c):
    return ops.DeviceCSR(c.indptr, c.indices, c.n_items, ctx.device)


def _same(name, got, exp, labels):
    got = [cpu(t) for t in got]
    bad = [l for l, g, e in zip(labels, got, exp) if not (g.dtype == e.dtype and np.array_equal(g, e))]
    if bad:
        first = int(np.argmax(np.any([g != e for g, e in zip(got, exp)], axis=0)))
        dump("sampler_edges_" + name, **{"got_" + l: g for l, g in zip(labels, got)}, **{"exp_" + l: e for l, e in zip(labels, exp)})
        raise AssertionError("%s: %s differ from the restatement, first at sample %d: got %s, expected %s"
                             % (name, bad, first, [g[first] for g in got], [e[first] for e in exp]))


# ---------------------------------------------------------------------------------------------------------- Philox samplers
@pytest.mark.parametrize("use_meta", [False, True], ids=["plain", "records"])
@pytest.mark.parametrize("name", sc.PHILOX_NAMES)
def test_bpr_sample_equals_restatement(ctx, name, use_meta):
    c = sc.philox_cases()[name]
    lo, hi = c.shard if c.shard else (0, None)
    got = ops.bpr_sample(ctx, _pos(ctx, c), c.n, seed=c.seed, first_sample=c.first, item_lo=lo, item_hi=hi, use_meta=use_meta)
    _same("bpr_%s_%d" % (name, use_meta), got, sc.bpr_expected(name)[:3], "uij")


@pytest.mark.parametrize("use_meta", [False, True], ids=["plain", "records"])
@pytest.mark.parametrize("name", sc.UNSHARDED_NAMES)
def test_pointwise_sample_equals_restatement(ctx, name, use_meta):
    """The label array is the restatement's coin: a stream whose coin sits one word off fails on "y" by itself."""
    c = sc.philox_cases()[name]
    u, i, y = ops.pointwise_sample(ctx, _pos(ctx, c), c.n, seed=c.seed, first_sample=c.first, use_meta=use_meta)
    eu, ei, ey, _ = sc.pw_expected(name)
    assert np.array_equal(cpu(y), ey), "coin"
    _same("pw_%s_%d" % (name, use_meta), (u, i, y), (eu, ei, ey), "uiy")


@pytest.mark.parametrize("neg_ratio", sc.RATIOS)
@pytest.mark.parametrize("name", sc.UNSHARDED_NAMES)
def test_pointwise_sample_ratio_equals_restatement(ctx, name, neg_ratio):
    c = sc.philox_cases()[name]
    u, i, y = ops.pointwise_sample_ratio(ctx, _pos(ctx, c), c.n, neg_ratio, seed=c.seed, first_sample=c.first)
    eu, ei, ey, _ = sc.pw_expected(name, neg_ratio)
    assert np.array_equal(cpu(y), ey), "coin"
    _same("pwr_%s_%d" % (name, neg_ratio), (u, i, y), (eu, ei, ey), "uiy")


def test_sampler_records_hold_row_bounds_and_signatures(ctx):
    """The 64-byte record of every user of the two signature cases: row start, length, and exactly the bits of its items."""
    for name in ("sig_full", "sig_one_bit", "row_lengths"):
        c = sc.philox_cases()[name]
        rec = cpu(ops.sampler_meta(ctx, _pos(ctx, c))).view(np.uint32).reshape(c.n_users, 16)
        for u, row in enumerate(sc.rows_of(c)):
            sig = np.zeros(12, dtype=np.uint32)
            for item in row:
                b = sc.sig_bit(item)
                sig[b >> 5] |= np.uint32(1 << (b & 31))
            assert int(rec[u, 0]) | int(rec[u, 1]) << 32 == int(c.indptr[u]) and int(rec[u, 2]) == len(row), (name, u)
            assert np.array_equal(rec[u, 4:], sig), (name, u)


# ---------------------------------------------------------------------------------------------------------- MT19937 replay
def _state(s):
    return cpu(s.state).view(np.uint32).copy()


def _replay(ctx, c):
    return ops.MtReplaySampler(ctx, c.lists, _pos(ctx, c), seed=c.seed)


@pytest.mark.parametrize("name", sc.MT_NAMES)
def test_mt_replay_equals_reference_and_numpy_state_after_every_call(ctx, name):
    """single_calls: 700 calls of one sample each, every one ending in the state-only pass of k_mt_generate."""
    c = sc.mt_cases()[name]
    s = _replay(ctx, c)
    assert np.array_equal(_state(s), ops.mt19937_init_state(c.seed))
    for k, (n, exp, (trip, state)) in enumerate(zip(c.calls, sc.mt_expected(name), sc.mt_numpy(name))):
        got = s.sample(n)
        _same("mt_%s_call%d" % (name, k), got, exp[:3], "uij")
        assert np.array_equal(np.stack([cpu(t) for t in got], axis=1), trip), (name, k)
        st = _state(s)
        assert int(st[624]) == int(state[624]), (name, k, "position")
        assert np.array_equal(st, state), (name, k, "state words")


def test_mt_replay_saves_and_starts_on_the_block_boundary(ctx):
    c = sc.mt_cases()["block_boundary"]
    s = _replay(ctx, c)
    states = [state for _, state in sc.mt_numpy(c.name)]
    s.sample(299)
    assert int(_state(s)[624]) == 624 and np.array_equal(_state(s), states[0])
    s.sample(309)
    assert int(_state(s)[624]) == 624 and np.array_equal(_state(s), states[1])
    s.sample(1)
    assert np.array_equal(_state(s), states[2])


def test_mt_replay_out_of_words_raises_and_keeps_the_state(ctx):
    c = sc.mt_out_of_words_case()
    s = _replay(ctx, c)
    s.sample(5)                                                            # a state that is not the seeded one
    before = _state(s)
    with pytest.raises(_lib.ElliotHipError, match="ran out of generated words"):
        s.sample(c.calls[0])
    torch.cuda.synchronize()
    assert _state(s).tobytes() == before.tobytes()
    ref = osampler.RefSampler(c.lists, c.n_items, seed=c.seed)             # and the sampler goes on where it was
    exp = np.array([ref.sample() for _ in range(10)], dtype=np.int32)[5:]
    got = s.sample(5)
    assert np.array_equal(np.stack([cpu(t) for t in got], axis=1), exp)


def test_mt_replay_empty_list_returns_an_error(ctx):
    c = sc.mt_empty_list_case()
    s = _replay(ctx, c)
    before = _state(s)
    with pytest.raises(_lib.ElliotHipError):
        s.sample(c.calls[0])
    torch.cuda.synchronize()
    assert _state(s).tobytes() == before.tobytes()
