"""Device-side beyond-accuracy metrics (el_beyond_metrics / el_beyond_hist_finish / el_beyond_entropy) against the
reference Evaluator's golden values (tests/golden/metrics_beyond_ref.npz) and the host route of the stand-alone evaluator (itself
pinned to the reference, tests/test_metrics_beyond_host.py)."""
import math

import numpy as np
import pytest
import torch

from elliot_amd import ops
from elliot_amd.evaluation import beyond
from elliot_amd.evaluation.evaluator import Evaluator
from elliot_amd.recommender.masks import device_masks
from tests.helpers import beyond_ref

pytestmark = pytest.mark.gpu
NAMES = list(ops.BEYOND_METRIC_NAMES)
Z = beyond_ref.load()
CASES = [str(t) for t in Z["cases"]]


@pytest.fixture(scope="module")
def ctx():
    return ops.get_context(0)


def blocks_of(ctx, lists, block=None):
    U = lists.shape[0]
    block = block or U
    for first in range(0, U, block):
        idx = torch.from_numpy(np.ascontiguousarray(lists[first:first + block], dtype=np.int32)).to(ctx.device)
        yield first, idx, idx


def raw_passes(ctx, data, lists, thr, cutoff, block=None, direct=False):
    """The three passes through ops: (sums, hist, stats, nov, entropy sum) as host arrays."""
    ev = Evaluator(data, None)
    sets = ev.device_sets(data, ctx.device)
    train = device_masks(data, ctx).train
    tables = ops.DeviceItemTables(ev.item_tables(data), ctx.device)
    sums = torch.zeros(ops.BEYOND_SUMS, dtype=torch.float64, device=ctx.device)
    hist = torch.zeros(data.num_items, dtype=torch.int32, device=ctx.device)
    kept = []
    for first, idx, _ in blocks_of(ctx, lists, block):
        ops.beyond_metrics(ctx, idx, sets["test"], train, tables, thr, cutoff, u_start=first, sums=sums, hist=hist, direct=direct)
        kept.append((first, idx))
    stats, nov = ops.beyond_hist_finish(ctx, hist)
    ent = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    for first, idx in kept:
        ops.beyond_entropy(ctx, idx, sets["test"], nov, cutoff, u_start=first, total=ent)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (sums, hist, stats, nov, ent))


def close(a, b, tol):
    if isinstance(b, int):
        return isinstance(a, int) and a == b
    if math.isnan(b):
        return math.isnan(a)
    return abs(a - b) <= tol * abs(b)


# ---- 1. golden -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_device_matches_the_reference_golden(ctx, tag):
    data, lists = beyond_ref.golden_case(Z, tag, NAMES)
    res = Evaluator(data, None).eval_device(ctx, data, blocks_of(ctx, lists))
    thr = float(Z[f"{tag}_threshold"])
    for r, c in enumerate(Z[f"{tag}_cutoffs"].tolist()):
        assert list(res[c]["test_results"]) == NAMES
        beyond_ref.check_against(res[c]["test_results"], NAMES, Z[f"{tag}_values"][r], 1e-11, f"{tag}@{c}")
        _, _, stats, _, _ = raw_passes(ctx, data, lists, thr, c)
        assert int(stats[2]) == int(Z[f"{tag}_G"][r]) and int(stats[0]) == int(Z[f"{tag}_values"][r][0])


# ---- 2. random vs the host evaluator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff,thr", [(10, 0.0), (50, 3.0), (100, 2.5), (7, 1.0)])
def test_device_matches_the_host_route_random(ctx, cutoff, thr):
    U, I, k = 700, 4000, max(cutoff, 20)
    train, test, lists = beyond_ref.random_case(U, I, k, seed=cutoff, big_user=5, empty_user=6)
    assert (lists[:, :cutoff] < 0).any() and np.diff(test[0])[5] == 1500 and np.diff(test[0])[6] == 0
    data = beyond_ref.Data(U, I, train, test, k, [cutoff], thr, NAMES)
    ev = Evaluator(data, None)
    recs = beyond_ref.recs_of(lists)
    host = ev.eval((recs, recs))[cutoff]["test_results"]
    dev = ev.eval_device(ctx, data, blocks_of(ctx, lists))[cutoff]["test_results"]
    assert list(dev) == NAMES
    for m in NAMES:
        print(f"{m}: device {dev[m]!r} host {host[m]!r}")
        assert close(dev[m], host[m], 1e-10), (m, dev[m], host[m])          # <= 7e4 terms per sum
    # the same input gives the same bytes, in both histogram forms; and the two forms agree exactly
    a = raw_passes(ctx, data, lists, thr, cutoff)
    b = raw_passes(ctx, data, lists, thr, cutoff)
    d = raw_passes(ctx, data, lists, thr, cutoff, direct=True)
    for x, y, z in zip(a, b, d):
        assert x.tobytes() == y.tobytes() == z.tobytes()


# ---- 3. block accumulation ---------------------------------------------------------------------------------------------------------
def test_blocks_accumulate_into_the_same_sums(ctx):
    U, I, k, cutoff, thr = 300, 500, 20, 20, 3.0
    train, test, lists = beyond_ref.random_case(U, I, k, seed=3)
    data = beyond_ref.Data(U, I, train, test, k, [cutoff], thr, NAMES)
    one = raw_passes(ctx, data, lists, thr, cutoff)
    blk = raw_passes(ctx, data, lists, thr, cutoff, block=128)
    assert np.array_equal(one[1], blk[1]) and np.array_equal(one[2], blk[2])           # histogram, n / free / G
    ints = [0, 1, 2, 3, 6, 7, 10, 11, 12, 13, 14, 15, 16, 17]
    assert np.array_equal(one[0][ints], blk[0][ints])
    assert one[3].tobytes() == blk[3].tobytes()
    for x, y in list(zip(one[0], blk[0])) + [(one[4][0], blk[4][0])]:
        assert abs(x - y) <= 1e-13 * abs(x), (x, y)


# ---- 4. contention and edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True])
def test_everyone_recommends_the_same_ten_items(ctx, direct):
    U, I, k = 65573, 50, 10                                 # U: no multiple of 4, 64 or 256
    rs = np.random.RandomState(0)
    items = np.sort(rs.choice(I, size=k, replace=False))
    lists = np.tile(items.astype(np.int32), (U, 1))
    others = np.setdiff1d(np.arange(I), items)
    qc = others[rs.randint(0, len(others), size=U)].astype(np.int32)                  # one train item per user, outside the list
    tc = np.where(others[0] == qc, others[1], others[0]).astype(np.int32)             # one held-out item per user
    ptr = np.arange(U + 1, dtype=np.int64)
    data = beyond_ref.Data(U, I, (ptr, qc), (ptr, tc, np.full(U, 4.0, np.float32)), k, [k], 1.0, NAMES)
    sums, hist, stats, nov, ent = raw_passes(ctx, data, lists, 1.0, k, direct=direct)
    expect = np.zeros(I, dtype=np.int64)
    expect[items] = U
    assert np.array_equal(hist, expect)
    assert stats[:3].tolist() == [k, k * U, 400 * U]        # G = U sum_{j < 10} (2 (j + 41) - 51)
    out = beyond.finish(NAMES, sums, int(stats[0]), int(stats[1]), int(stats[2]), float(ent[0]), I)
    assert out["ItemCoverage"] == k and out["UserCoverage"] == U
    assert abs(out["Gini"] - (1 - 40 / 49)) <= 1e-15
    assert abs(out["SEntropy"] - math.log(10) / math.log(2)) <= 1e-12        # every list: (1 / 10) 10 log2(10)


def test_one_item_catalogue(ctx):
    U = 9
    ptr = np.arange(U + 1, dtype=np.int64)
    none = np.zeros(U + 1, dtype=np.int64)
    # nobody holds the item in train; users 0..7 hold it in the held-out split, user 8 has an item the model has no row for
    tc = np.array([0] * 8 + [1], dtype=np.int32)
    data = beyond_ref.Data(U, 1, (none, np.zeros(0, np.int32)), (ptr, tc, np.full(U, 5.0, np.float32)), 1, [1], 1.0, NAMES, transactions=0)
    lists = np.zeros((U, 1), dtype=np.int32)
    lists[3, 0] = -1
    sums, hist, stats, nov, ent = raw_passes(ctx, data, lists, 1.0, 1)
    assert hist.tolist() == [8] and stats[:3].tolist() == [1, 8, 0] and nov.tolist() == [0.0]
    assert sums[[0, 1, 2, 3]].tolist() == [9.0, 9.0, 8.0, 8.0]
    ev = Evaluator(data, None)
    recs = beyond_ref.recs_of(lists)
    host = ev.eval((recs, recs))[1]["test_results"]
    dev = ev.eval_device(ctx, data, blocks_of(ctx, lists))[1]["test_results"]
    for m in NAMES:
        assert close(dev[m], host[m], 1e-12), (m, dev[m], host[m])
    assert dev["Gini"] == 0.0 and dev["ItemCoverage"] == 1 and dev["UserCoverage"] == 8


@pytest.mark.parametrize("U,I,k,cutoff", [(130, 4097, 16, 16), (50, 2000, 512, 512), (130, 4097, 16, 3)])
def test_edge_shapes_match_the_host_route(ctx, U, I, k, cutoff):
    train, test, lists = beyond_ref.random_case(U, I, k, seed=I + cutoff)
    data = beyond_ref.Data(U, I, train, test, k, [cutoff], 2.0, NAMES)
    ev = Evaluator(data, None)
    recs = beyond_ref.recs_of(lists)
    host = ev.eval((recs, recs))[cutoff]["test_results"]
    dev = ev.eval_device(ctx, data, blocks_of(ctx, lists))[cutoff]["test_results"]
    for m in NAMES:
        assert close(dev[m], host[m], 1e-10), (m, dev[m], host[m])


def test_cutoff_limits_are_refused(ctx):
    train, test, lists = beyond_ref.random_case(20, 100, 8, seed=1)
    data = beyond_ref.Data(20, 100, train, test, 8, [8], 0.0, NAMES)
    with pytest.raises(Exception, match="cutoff"):
        raw_passes(ctx, data, lists, 0.0, 9)                # cutoff > ld
    with pytest.raises(Exception, match="cutoff"):
        raw_passes(ctx, data, np.zeros((20, 600), np.int32), 0.0, 513)


# ---- 5. the histogram finish alone ----------------------------------------------------------------------------------------------------
def crafted_counts():
    rs = np.random.RandomState(7)
    ties = np.concatenate([np.full(5000, 255), np.full(5000, 256), np.full(3000, 65535), np.full(3000, 65536), np.full(700, 0),
                           np.full(2000, (1 << 24) - 1), np.full(2000, 1 << 24), rs.randint(0, 1 << 20, size=1234)])
    rs.shuffle(ties)
    one = np.zeros(4097, dtype=np.int64)
    one[1234] = 77
    return {"all_equal": np.full(1000, 13), "one_nonzero": one, "tie_runs_across_digit_boundaries": ties, "single_item": np.array([5])}


@pytest.mark.parametrize("name", list(crafted_counts()))
def test_hist_finish_on_crafted_counts(ctx, name):
    counts = crafted_counts()[name].astype(np.int64)
    I = counts.shape[0]
    stats, nov = ops.beyond_hist_finish(ctx, torch.from_numpy(counts.astype(np.int32)).to(ctx.device))
    torch.cuda.synchronize()
    stats, nov = stats.cpu().numpy(), nov.cpu().numpy()
    nz = sorted(int(c) for c in counts if c > 0)
    n, free = len(nz), sum(nz)
    G = sum((2 * (j + I - n + 1) - I - 1) * c for j, c in enumerate(nz))            # Python integers
    assert stats.tolist() == [n, free, G, 0]
    assert beyond.gini_numerator(counts, I) == (n, free, G)
    ref = np.array([-math.log(c / free) / math.log(2) if c > 0 else 0.0 for c in counts.tolist()])
    assert np.abs(nov - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
