"""GPU: the SlopeOne kernels -- el_slope_build, el_slope_table, el_slope_scores, el_dense_topk_f64 + el_topk_pad_f64 -- against
the restatement of tests/helpers/slopeone_ref.py, which scripts/gen_golden_slopeone.py proved equal to the reference's own
SlopeOneModel bit for bit.  Integer and half-step ratings make every sum exact: there are no tolerances here, only equalities."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd import ops
from tests.helpers import slopeone_ref

pytestmark = pytest.mark.gpu

CASES = ["int", "half", "cold_item", "one_rating", "split"]
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def matrix(indptr, indices, ratings, U, I):
    """The scipy train matrix of dict-order rows, on copies: the builders sort the matrix they are given in place."""
    return sp.csr_matrix((np.array(ratings, np.float64), np.array(indices), np.array(indptr)), shape=(U, I))


def reference(g, tag):
    """(indptr, indices, ratings, U, I, freq, dev, mean) of a golden case: computed once, shared, never written to."""
    if tag not in _cache:
        c = slopeone_ref.case(g, tag)
        _cache[tag] = c + slopeone_ref.build(*c)
    return _cache[tag]


@pytest.mark.parametrize("tag", CASES)
def test_build_equals_reference(ctx, golden, tag):
    indptr, indices, ratings, U, I, freq, dev, _ = reference(golden("slopeone_ref.npz"), tag)
    R = matrix(indptr, indices, ratings, U, I)
    f1, d1, t1 = (host(x) for x in ops.slope_build(ctx, R))
    assert f1.dtype == np.int32 and np.array_equal(f1, freq)
    assert np.array_equal(bits(d1), bits(dev))                              # as uint64: pins the -0.0 pattern
    assert np.array_equal(bits(t1), bits(slopeone_ref.table(freq, dev)))
    f2, d2, t2 = (host(x) for x in ops.slope_build(ctx, R))
    assert f1.tobytes() == f2.tobytes() and d1.tobytes() == d2.tobytes() and t1.tobytes() == t2.tobytes()


def random_rows(rs, U, I, per_user, levels):
    lens = np.minimum(rs.poisson(per_user, U) + 1, I)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([rs.choice(I, n, replace=False) for n in lens]).astype(np.int32)
    return indptr, indices, levels[rs.randint(0, len(levels), indptr[-1])].astype(np.float64)


def check_sampled_rows(ctx, indptr, indices, ratings, U, I, rows):
    freq, dev, _ = ops.slope_build(ctx, matrix(indptr, indices, ratings, U, I), table=False)
    f, d = host(freq[torch.as_tensor(rows, device=ctx.device)]), host(dev[torch.as_tensor(rows, device=ctx.device)])
    rf, rd = slopeone_ref.build_rows(indptr, indices, ratings, U, I, rows)
    assert np.array_equal(f, rf)
    assert np.array_equal(bits(d), bits(rd))
    return rf


def test_build_counts_a_row_in_two_passes(ctx):
    """One LDS tile of k_slope_build + 917 items: every row is counted in two passes over the catalogue."""
    U, I = 2500, ops.SLOPE_TILE + 917
    rs = np.random.RandomState(7)
    indptr, indices, ratings = random_rows(rs, U, I, 40, np.arange(1, 11) * 0.5)
    rows = np.unique(np.concatenate([[0, ops.SLOPE_TILE - 1, ops.SLOPE_TILE, I - 1], rs.choice(I, 44, replace=False)]))
    rf = check_sampled_rows(ctx, indptr, indices, ratings, U, I, rows)
    off = rf.copy()
    off[np.arange(len(rows)), rows] = 0
    assert off[:, :ops.SLOPE_TILE].any() and off[:, ops.SLOPE_TILE:].any()   # co-rated pairs on both sides of the tile edge


@pytest.mark.parametrize("top", [20_000, 20_000_000])
def test_build_with_large_ratings(ctx, top):
    """Ratings up to 20 000 on 300 x 120; and up to 20 000 000, where |S| passes 2^31 and the 64-bit cells are needed
    (2 * max_deg * max_abs >= 2^31)."""
    U, I = 300, 120
    rs = np.random.RandomState(8)
    indptr, indices, ratings = random_rows(rs, U, I, 50, np.array([1, 2, top // 2, top - 1, top]))
    if top > 20_000:
        deg = np.bincount(indices, minlength=I).max()
        assert 2 * deg * top >= 2 ** 31
    check_sampled_rows(ctx, indptr, indices, ratings, U, I, np.arange(I))


@pytest.mark.parametrize("tag", ["int", "half"])
def test_scores_equal_reference(ctx, golden, tag):
    g = golden("slopeone_ref.npz")
    indptr, indices, ratings, U, I, freq, dev, mean = reference(g, tag)
    _, _, T = ops.slope_build(ctx, matrix(indptr, indices, ratings, U, I))
    rows = ops.DeviceCSR(indptr, indices, I, ctx.device)
    P = ops.slope_scores(ctx, rows, torch.from_numpy(mean).to(ctx.device), T, 0, U)
    assert np.array_equal(bits(host(P)), bits(g[f"{tag}_pred"]))
    part = ops.slope_scores(ctx, rows, torch.from_numpy(mean).to(ctx.device), T, 17, 101)
    assert np.array_equal(bits(host(part)), bits(g[f"{tag}_pred"][17:101]))


def test_scoring_chain(ctx):
    """I = 1037 (no multiple of any tile); rows of 1, 63, 64, 65 and 3 000 entries in non-ascending order (the long one
    repeats items: the kernel sums what the row stores) and an empty row.  The chain of rounded quotients is order-sensitive."""
    U0, I = 200, 1037
    rs = np.random.RandomState(9)
    indptr, indices, ratings = random_rows(rs, U0, I, 100, np.arange(1, 11) * 0.5)
    freq, dev, T = ops.slope_build(ctx, matrix(indptr, indices, ratings, U0, I))
    rf, rd = host(freq).astype(np.float64), host(dev)
    assert (rf == 0).any() and (rf > 0).mean() > 0.5
    lens = [1, 63, 0, 64, 65, 3000]
    s_indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    s_indices = np.concatenate([rs.randint(0, I, n) for n in lens]).astype(np.int32)
    assert all(np.any(np.diff(s_indices[a:b]) < 0) for a, b in zip(s_indptr[:-1], s_indptr[1:]) if b - a > 1)
    mean = np.array([3.5, 2.25, 4.0, 1.0 / 3.0, 2.75, 3.125])
    want = slopeone_ref.predictions(s_indptr, s_indices, rf, rd, mean)
    rows = ops.DeviceCSR(s_indptr, s_indices, I, ctx.device)
    P = host(ops.slope_scores(ctx, rows, torch.from_numpy(mean).to(ctx.device), T, 0, len(lens)))
    assert np.array_equal(bits(P), bits(want))
    assert np.array_equal(bits(P[2]), bits(np.full(I, 4.0)))                # the empty row: mean_u for every item
    long_row = s_indices[s_indptr[5]:]                                      # (that row in reverse order gives other bits)
    flipped = slopeone_ref.predictions(np.array([0, 3000]), long_row[::-1].copy(), rf, rd, mean[5:])
    assert not np.array_equal(bits(flipped[0]), bits(want[5]))


@pytest.mark.parametrize("tag", ["half", "split"])
def test_table_from_restored_pair_equals_build(ctx, golden, tag):
    indptr, indices, ratings, U, I, freq, dev, _ = reference(golden("slopeone_ref.npz"), tag)
    _, _, T = ops.slope_build(ctx, matrix(indptr, indices, ratings, U, I))
    again = ops.slope_table(ctx, torch.from_numpy(freq.astype(np.int32)).to(ctx.device), torch.from_numpy(dev).to(ctx.device))
    assert host(T).tobytes() == host(again).tobytes()


def test_table_beyond_one_transpose_tile(ctx):
    U, I = 120, 203
    rs = np.random.RandomState(10)
    indptr, indices, ratings = random_rows(rs, U, I, 20, np.arange(1, 6).astype(float))
    freq, dev, T = ops.slope_build(ctx, matrix(indptr, indices, ratings, U, I))
    assert host(T).tobytes() == host(ops.slope_table(ctx, freq, dev)).tobytes()
    assert np.array_equal(bits(host(T)), bits(slopeone_ref.table(host(freq), host(dev))))


def topk_case(rs, n, I, levels):
    """A block with many equal values, an exclusion CSR and a candidate CSR whose first rows hold fewer than k items."""
    preds = rs.randint(0, levels, (n, I)).astype(np.float64) / 8.0 - 3.0
    excl = rs.rand(n, I) < 0.3
    cand = rs.rand(n, I) < 0.2
    cand[0] = False
    cand[1] = False
    cand[1, [5, 200, 17]] = True
    cand[2, :] = False
    cand[2, rs.choice(I, 9, replace=False)] = True
    return preds, excl, cand


def csr_of(mask, ctx, U, first):
    """The rows of `mask` as rows first, first + 1, ... of a DeviceCSR over U users."""
    full = np.zeros((U, mask.shape[1]), dtype=bool)
    full[first:first + mask.shape[0]] = mask
    m = sp.csr_matrix(full)
    m.sort_indices()
    return ops.DeviceCSR(m.indptr, m.indices, mask.shape[1], ctx.device)


@pytest.mark.parametrize("kind", ["none", "excl", "cand"])
def test_dense_topk_f64(ctx, kind):
    n, I, k, first, U = 37, 301, 10, 5, 50
    preds, excl, cand = topk_case(np.random.RandomState(11), n, I, 12)
    allowed = {"none": np.ones((n, I), bool), "excl": ~excl, "cand": cand}[kind]
    kw = {"none": {}, "excl": {"excl": csr_of(excl, ctx, U, first)}, "cand": {"cand": csr_of(cand, ctx, U, first)}}[kind]
    idx, val = ops.dense_topk_f64(ctx, torch.from_numpy(preds).to(ctx.device), first, first + n, k, pad=True, **kw)
    idx, val = host(idx), host(val)
    assert idx.dtype == np.int32 and val.dtype == np.float64
    for r in range(n):
        wi, wv = slopeone_ref.topk(preds[r], allowed[r], k)                 # (value desc, index asc), (-1, -inf) padding
        assert np.array_equal(idx[r], wi) and np.array_equal(bits(val[r]), bits(wv)), r
    if kind == "cand":
        assert (idx[0] == -1).all() and (idx[1, 3:] == -1).all() and idx[2, 9] == -1 and (idx[2, :9] >= 0).all()


def test_dense_topk_f64_unpadded_short_list_and_values(ctx):
    """Without the padding step a short list is filled with masked items at -inf (el_dense_topk's contract); values that fp32
    cannot tell apart are ordered as fp64."""
    n, I, k = 3, 70, 8
    preds = np.full((n, I), 1.0)
    preds[:, 40] = 1.0 + 2.0 ** -40
    preds[:, 3] = 1.0 - 2.0 ** -41
    cand = np.zeros((n, I), bool)
    cand[:, [3, 40, 50]] = True
    idx, val = ops.dense_topk_f64(ctx, torch.from_numpy(preds).to(ctx.device), 0, n, k, cand=csr_of(cand, ctx, n, 0))
    idx, val = host(idx), host(val)
    assert idx[0, :3].tolist() == [40, 50, 3] and np.array_equal(bits(val[0, :3]), bits(preds[0, [40, 50, 3]]))
    assert idx[0, 3:].tolist() == [0, 1, 2, 4, 5] and np.isneginf(val[0, 3:]).all()
