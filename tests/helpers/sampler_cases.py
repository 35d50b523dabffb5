"""The small data sets that hold the four device samplers to their stream and row edges (tests/test_gpu_sampler_edges.py), and what
the CPU restatements (oracle/sampler.py) and NumPy's own generator give on them.  tests/test_sampler_ref_host.py checks, without a
GPU, that every case has the property it is named for; the GPU test only reads the tables.

Every case is built through philox_case() / mt_case(), which refuse a data set without a user the samplers can finish on: a user
with 0 < len(row) < I and, for a sharded case, a free item inside [item_lo, item_hi).  Without one the kernels never return.
"""
import collections
import functools
import os

import numpy as np

from oracle import sampler as osampler

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
ATTEMPTS = 4096                     # negative candidates per user draw
SIG_BITS = 384                      # bits of a sampler record's membership signature
RATIOS = (1, 4, 255)

PhiloxCase = collections.namedtuple("PhiloxCase", "name indptr indices n_users n_items seed first n shard")
MtCase = collections.namedtuple("MtCase", "name lists indptr indices n_items seed calls")


def sig_bit(item):
    """The signature bit of an item in a sampler record (el_sig_bit)."""
    return ((int(item) * 0x9E3779B1) & 0xFFFFFFFF) % SIG_BITS


def csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate([np.asarray(sorted(r), dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return indptr, indices


def random_rows(n_users, n_items, seed, lo=1, hi=20):
    """Rows of lo..hi distinct items each."""
    rs = np.random.RandomState(seed)
    return [sorted(rs.choice(n_items, rs.randint(lo, hi + 1), replace=False).tolist()) for _ in range(n_users)]


def rows_of(case):
    return [case.indices[case.indptr[u]:case.indptr[u + 1]].tolist() for u in range(len(case.indptr) - 1)]


def finishing_users(rows, n_items, shard=None):
    """The users a sample can end on: 0 < len(row) < I and, with a shard, an item of the shard that is not in the row."""
    lo, hi = shard if shard else (0, 0)
    return [u for u, r in enumerate(rows)
            if 0 < len(r) < n_items and (shard is None or any(c not in set(r) for c in range(lo, hi)))]


def philox_case(name, rows, n_items, n, seed=42, first=0, shard=None):
    if not finishing_users(rows, n_items, shard):
        raise ValueError("case %s: no user a sample can end on -- the device samplers would never return" % name)
    assert shard is None or 0 <= shard[0] < shard[1] <= n_items
    indptr, indices = csr(rows)
    return PhiloxCase(name, indptr, indices, len(rows), int(n_items), int(seed), int(first), int(n), shard)


# ------------------------------------------------------------------------------------------------------------- Philox cases
BASE_U, BASE_I = 50, 100


def _base():
    return random_rows(BASE_U, BASE_I, seed=1)


def _row_lengths():
    """I = 33: rows of 0, 1, I - 1 (one negative left) and I (full: passed over) items among ordinary ones."""
    n_items = 33
    rs = np.random.RandomState(7)
    lens = [0, 1, n_items - 1, n_items, 5, 10, 0, n_items, 7]
    return [sorted(rs.choice(n_items, k, replace=False).tolist()) for k in lens], n_items


def _sig_full():
    """Row 0 holds, for every signature bit, the smallest item with that bit, and 16 more: 400 items, all 384 bits set."""
    n_items = 2000
    first = {}
    for item in range(n_items):
        first.setdefault(sig_bit(item), item)
    assert len(first) == SIG_BITS
    row = set(first.values())
    row |= set([c for c in range(n_items) if c not in row][:16])
    return [sorted(row)] + random_rows(2, n_items, seed=3), n_items


def _sig_one_bit():
    """I = 512, four users of one item each; another item of the catalogue has the same signature bit and is no positive."""
    n_items = 512
    by_bit = collections.defaultdict(list)
    for item in range(n_items):
        by_bit[sig_bit(item)].append(item)
    shared = [items for _, items in sorted(by_bit.items()) if len(items) >= 2]
    return [[items[0]] for items in shared[:4]], n_items


def _huge():
    """I = 2^31 - 2: column ids at both ends of the int32 range."""
    n_items = 2 ** 31 - 2
    top = n_items - 1
    return [[0, 1, 5], [top], [7, 2 ** 30, top], [top - 1, top], [0], [3, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, top - 2]], n_items


def _shard_width1():
    """I = 40, negatives only from [17, 18): users 0 and 1 hold item 17, the other six do not.  No empty and no full row."""
    rows = random_rows(8, 40, seed=11, lo=2, hi=12)
    rows = [sorted(set(r) | {17}) if u < 2 else sorted(set(r) - {17}) or [0] for u, r in enumerate(rows)]
    return rows, 40, (17, 18)


def _shard_covered():
    """I = 64, negatives only from [16, 24): users 0..2 hold all eight, the other seven at most seven of them.  No empty and no
    full row."""
    rows = random_rows(10, 64, seed=12, lo=3, hi=25)
    out = []
    for u, r in enumerate(rows):
        s = set(r) | set(range(16, 24)) if u < 3 else set(r) - {16 + u % 8}
        out.append(sorted(s))
    return out, 64, (16, 24)


@functools.lru_cache(maxsize=None)
def philox_cases():
    cases = []
    for n in (1, 255, 256, 257):                                           # launch sizes: one lane, a block +- 1
        cases.append(philox_case("launch_n%d" % n, _base(), BASE_I, n))
    for n_users in (1, 2, 64, 65):                                         # bounded(U): U = 1 still takes a word
        cases.append(philox_case("users_%d" % n_users, random_rows(n_users, BASE_I, seed=100 + n_users), BASE_I, 300))
    rows, n_items = _row_lengths()
    cases.append(philox_case("row_lengths", rows, n_items, 1000))
    rows, n_items = _sig_full()
    cases.append(philox_case("sig_full", rows, n_items, 1000))
    rows, n_items = _sig_one_bit()
    cases.append(philox_case("sig_one_bit", rows, n_items, 3000))
    cases.append(philox_case("items_64", random_rows(20, 64, seed=5, hi=30), 64, 500))
    cases.append(philox_case("items_65", random_rows(20, 65, seed=6, hi=30), 65, 500))
    rows, n_items = _huge()
    cases.append(philox_case("items_2p31m2", rows, n_items, 500))
    cases.append(philox_case("counter_carry", _base(), BASE_I, 300, first=2 ** 32 - 100))
    cases.append(philox_case("counter_2p40", _base(), BASE_I, 300, first=2 ** 40 + 7))
    cases.append(philox_case("seed_high_word", _base(), BASE_I, 300, seed=2 ** 32 + 5))
    cases.append(philox_case("seed_all_ones", _base(), BASE_I, 300, seed=2 ** 64 - 1))
    rows, n_items, shard = _shard_width1()
    cases.append(philox_case("shard_width1", rows, n_items, 300, shard=shard))
    rows, n_items, shard = _shard_covered()
    cases.append(philox_case("shard_covered", rows, n_items, 400, shard=shard))
    return collections.OrderedDict((c.name, c) for c in cases)


PHILOX_NAMES = tuple(philox_cases())
UNSHARDED_NAMES = tuple(n for n, c in philox_cases().items() if c.shard is None)
SHARDED_NAMES = tuple(n for n, c in philox_cases().items() if c.shard is not None)


def _traced(fn, *args, **kw):
    """fn's result and, per sample, how many bounded() draws its Philox stream made."""
    osampler.TRACE = []
    try:
        out = fn(*args, **kw)
        draws = np.array([ps.draws for ps in osampler.TRACE], dtype=np.int64)
    finally:
        osampler.TRACE = None
    return out, draws


@functools.lru_cache(maxsize=None)
def bpr_expected(name):
    """(u, i, j, draws) of oracle.sampler.philox_sample on the case."""
    c = philox_cases()[name]
    lo, hi = c.shard if c.shard else (0, None)
    (u, i, j), draws = _traced(osampler.philox_sample, c.indptr, c.indices, c.n_users, c.n_items, c.seed, c.first, c.n,
                               item_lo=lo, item_hi=hi)
    return u, i, j, draws


@functools.lru_cache(maxsize=None)
def pw_expected(name, neg_ratio=None):
    """(u, item, label, draws) of oracle.sampler.philox_pointwise_sample on the case (neg_ratio None: the fair coin)."""
    c = philox_cases()[name]
    (u, i, y), draws = _traced(osampler.philox_pointwise_sample, c.indptr, c.indices, c.n_users, c.n_items, c.seed, c.first, c.n,
                               neg_ratio=neg_ratio)
    return u, i, y, draws


# ------------------------------------------------------------------------------------------------------------ MT19937 cases
def mt_case(name, lists, n_items, calls, seed=42, allow_unfinished=False):
    """lists: the users' positives in the order the reference's sampler holds them (any order); the CSR has them ascending."""
    if not allow_unfinished and len(finishing_users(lists, n_items)) != len(lists):
        raise ValueError("case %s: a user the replay cannot finish on" % name)
    indptr, indices = csr(lists)
    return MtCase(name, [list(l) for l in lists], indptr, indices, int(n_items), int(seed), tuple(calls))


def _golden_lists():
    g = np.load(os.path.join(GOLDEN, "sampler_ref.npz"), allow_pickle=False)
    lp, li = g["lists_indptr"], g["lists_items"]
    return [li[lp[u]:lp[u + 1]].tolist() for u in range(int(g["n_users"]))], int(g["n_items"])


def _descending(rows):
    return [sorted(r, reverse=True) for r in rows]


@functools.lru_cache(maxsize=None)
def mt_cases():
    cases = []
    # U = 1 and a one-item list: randint(1) takes no word, a sample is the words of j alone.  299 samples end on word 624 of the
    # first block, 608 on word 624 of the second: a state saved on the boundary, a call that starts there, a call of one sample
    cases.append(mt_case("block_boundary", [[0]], 2, (299, 309, 1), seed=1))
    lists, n_items = _golden_lists()
    cases.append(mt_case("many_twists", lists, n_items, (3000,)))
    cases.append(mt_case("single_calls", _descending(random_rows(20, 30, seed=21, hi=10)), 30, (1,) * 700))
    cases.append(mt_case("items_64", _descending(random_rows(10, 64, seed=22, hi=30)), 64, (500, 500)))
    cases.append(mt_case("items_65", _descending(random_rows(10, 65, seed=23, hi=30)), 65, (500, 500)))
    cases.append(mt_case("one_item_list", [[5], [3, 1, 2], [7], [9, 0, 4, 8]], 10, (400, 7)))
    return collections.OrderedDict((c.name, c) for c in cases)


MT_NAMES = tuple(mt_cases())


def mt_out_of_words_case():
    """Every user holds I - 1 = 63 of 64 items: a negative takes 64 words on average, 16 a sample are provisioned."""
    return mt_case("out_of_words", [[c for c in range(64) if c != 7 * u] for u in range(4)], 64, (2000,))


def mt_empty_list_case():
    """User 1 has no positive: the reference's randint(0) raises as soon as that user is drawn."""
    return mt_case("empty_list", [[1, 2], [], [3]], 8, (50,), allow_unfinished=True)


@functools.lru_cache(maxsize=None)
def mt_expected(name):
    """Per call of the case: (u, i, j) of oracle.sampler.RefSampler and the words its generator has handed out so far."""
    c = mt_cases()[name]
    out = []
    ref = counted_ref_sampler(c)
    for n in c.calls:
        t = np.array([ref.sample() for _ in range(n)], dtype=np.int32)
        out.append((t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), ref.words()))
    return out


def counted_ref_sampler(c):
    """RefSampler of an MT case with .words(): how many words its generator has handed out (624 a twist)."""
    ref = osampler.RefSampler(c.lists, c.n_items, seed=c.seed)
    twists, twist = [0], ref.rng._twist

    def counting_twist():
        twists[0] += 1
        twist()
    ref.rng._twist = counting_twist
    ref.words = lambda: 624 * (twists[0] - 1) + ref.rng.pos if twists[0] else 0
    return ref


@functools.lru_cache(maxsize=None)
def mt_numpy(name):
    """Per call of the case: the triplets of custom_sampler's three lines run on np.random.RandomState(seed) itself, and that
    generator's state afterwards as the device keeps it: 624 words and the position, uint32[625]."""
    c = mt_cases()[name]
    rs = np.random.RandomState(c.seed)
    sets = [set(l) for l in c.lists]
    n_users = len(c.lists)
    out = []
    for n in c.calls:
        t = np.empty((n, 3), dtype=np.int32)
        for k in range(n):
            u = rs.randint(n_users)
            i = c.lists[u][rs.randint(len(c.lists[u]))]
            j = rs.randint(c.n_items)
            while j in sets[u]:
                j = rs.randint(c.n_items)
            t[k] = (u, i, j)
        st = rs.get_state()
        out.append((t, np.concatenate([st[1].astype(np.uint32), np.array([st[2]], dtype=np.uint32)])))
    return out
