"""el_csr_row_l1 / el_rp3_rows / el_rp3_cut (csrc/el_rp3.hip) against the restatement (tests/helpers/rp3_ref.py) and the
reference's own W and lists (tests/golden/rp3beta_ref.npz)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.helpers import knn_ref, rp3_ref
from tests.helpers.rp3_ref import assert_w_equal, bits, case_matrix, golden_operands, host_w, load_golden as load, reference_w, to_device

pytestmark = pytest.mark.gpu

GOLDEN_CASES = 7
TILE = 4096                      # RP3_TILE of csrc/el_rp3.hip: columns of one slice


def golden_case(golden, n):
    z, R = load(golden)
    tag, p = str(z["cases"][n]), z["tag_params"][n]
    return z, R, tag, int(p[0]), float(p[1]), float(p[2]), bool(p[3])


def float_ratings(indptr, indices, shape, seed):
    rs = np.random.RandomState(seed)
    return sp.csr_matrix((rs.uniform(0.5, 5.0, indices.shape[0]).astype(np.float32), indices, indptr), shape=shape)


def test_row_l1_matches_the_sequential_loop(ctx):
    """Non-integer ratings, empty rows, a row whose sum is 0, a long row: bit for bit the loop that test_oracle_rp3beta pins
    to sklearn's normalize."""
    from elliot_amd import ops
    rs = np.random.RandomState(11)
    X = sp.random(3000, 900, density=0.03, random_state=rs, format="csr", dtype=np.float32)
    X.data[:] = rs.uniform(-1.0, 5.0, X.nnz).astype(np.float32)
    X = sp.vstack([X, sp.csr_matrix(np.full((1, 900), 0.3, np.float32)), sp.csr_matrix((2, 900), dtype=np.float32)]).tocsr()
    X.data[X.indptr[5]:X.indptr[6]] = 0.0
    assert (np.diff(X.indptr) == 0).any() and np.diff(X.indptr).max() == 900
    got = ops.csr_row_l1(ctx, torch.from_numpy(X.indptr.astype(np.int64)).to(ctx.device), ops.device_values(X.data, ctx.device))
    assert np.array_equal(bits(got.cpu().numpy()), bits(rp3_ref.row_l1(X.indptr, X.data)))


@pytest.mark.parametrize("n", range(GOLDEN_CASES))
def test_build_on_reference_operands_equals_reference_w(ctx, golden, n):
    from elliot_amd import ops
    z, R, tag, N, alpha, beta, norm = golden_case(golden, n)
    W, Wv = ops.rp3_build(ctx, *to_device(ops, ctx, *golden_operands(z, R, tag)), N, norm)
    assert_w_equal(host_w(W, Wv), reference_w(z, tag, R.shape[1]))


@pytest.mark.parametrize("n", range(GOLDEN_CASES))
def test_device_operands_equal_restatement(ctx, golden, n):
    """rp3_operands (device row-l1, host powers) == the restated operands computed in the same process."""
    from elliot_amd import ops
    z, R, tag, N, alpha, beta, norm = golden_case(golden, n)
    Rc = case_matrix(R, tag)
    Piu, pv, Pui, qv, deg = ops.rp3_operands(ctx, Rc, alpha, beta)
    ePiu, ePui, edeg = rp3_ref.operands(Rc, alpha, beta)
    assert np.array_equal(Piu.indptr.cpu().numpy(), ePiu.indptr) and np.array_equal(Piu.indices.cpu().numpy(), ePiu.indices)
    assert np.array_equal(Pui.indptr.cpu().numpy(), ePui.indptr) and np.array_equal(Pui.indices.cpu().numpy(), ePui.indices)
    assert np.array_equal(bits(pv.cpu().numpy()), bits(ePiu.data)) and np.array_equal(bits(qv.cpu().numpy()), bits(ePui.data))
    assert np.array_equal(deg.cpu().numpy(), edeg)


def test_tie_rules_and_neighborhood_beyond_the_catalogue(ctx):
    """Binary input with many tied cuts pins (value desc, index asc) in both cuts; N > I keeps every non-zero."""
    from elliot_amd import ops
    from elliot_amd.synthetic import small_dataset
    indptr, indices, _ = small_dataset(200, 150, seed=0)
    I = int(indices.max()) + 1
    R = sp.csr_matrix((np.ones(indices.shape[0], np.float32), indices, indptr), shape=(200, I))
    Piu, Pui, degree = rp3_ref.operands(R, 1.0, 0.0)
    W_ref, row_ties, col_ties = rp3_ref.build_w(Piu, Pui, degree, 20, False)
    print("tied row cuts", row_ties, "tied column cuts", col_ties)
    assert row_ties >= 10
    dev = to_device(ops, ctx, Piu, Pui, degree)
    assert_w_equal(host_w(*ops.rp3_build(ctx, *dev, 20, False)), W_ref)
    for N in (1000, -1):
        assert_w_equal(host_w(*ops.rp3_build(ctx, *dev, N, True)), rp3_ref.build_w(Piu, Pui, degree, N, True)[0])


@pytest.mark.parametrize("normalize", [False, True])
def test_ml1m_shape_full_w(ctx, normalize):
    """6040 x 3706, float ratings, N = 50: several column slices per row, the whole W against the restatement."""
    from elliot_amd import ops
    from elliot_amd.synthetic import zipf_csr
    U, I = 6040, 3706
    indptr, indices = zipf_csr(U, I, mean_log=4.6, sigma_log=0.9, dmin=20, dmax=2000, zipf_a=0.9, seed=1)
    R = float_ratings(indptr, indices, (U, I), seed=1)
    Piu, pv, Pui, qv, deg = ops.rp3_operands(ctx, R, 1.0, 0.6)
    ePiu, ePui, edeg = rp3_ref.operands(R, 1.0, 0.6)
    assert np.array_equal(bits(qv.cpu().numpy()), bits(ePui.data)) and np.array_equal(deg.cpu().numpy(), edeg)
    W, Wv = ops.rp3_build(ctx, Piu, pv, Pui, qv, deg, 50, normalize)
    assert_w_equal(host_w(W, Wv), rp3_ref.build_w(ePiu, ePui, edeg, 50, normalize)[0])


def test_wide_catalogue_slices(ctx):
    """40 000 items = 10 column slices of one LDS tile each: the lists of 64 sampled rows that include the 8 longest, one row
    asked for alone, and the cut of the device's own full lists against the CPU cut of those lists."""
    from elliot_amd import ops
    from elliot_amd.synthetic import zipf_csr
    U, I, N = 20000, 40000, 50
    assert I > 2 * TILE
    indptr, indices = zipf_csr(U, I, mean_log=3.0, sigma_log=0.8, dmin=2, dmax=400, zipf_a=0.9, seed=7)
    R = float_ratings(indptr, indices, (U, I), seed=7)
    Piu, Pui, degree = rp3_ref.operands(R, 1.0, 0.6)
    dev = to_device(ops, ctx, Piu, Pui, degree)
    idx, val, cnt = (t.cpu().numpy() for t in ops.rp3_rows(ctx, *dev, N))
    rs = np.random.RandomState(7)
    lens = np.diff(Piu.indptr)
    rows = np.sort(rs.choice(np.flatnonzero(lens), size=64, replace=False))
    rows[:8] = np.argsort(-lens, kind="stable")[:8]
    lists, _ = rp3_ref.row_lists(Piu, Pui, degree, rows, N)
    for i, (j, v) in zip(rows, lists):
        assert cnt[i] == len(j), i
        assert np.array_equal(idx[i, :cnt[i]], j), i
        assert np.array_equal(bits(val[i, :cnt[i]]), bits(v)), i
    i = int(rows[0])                                                     # the longest row on its own: the row-range form
    one = [t.cpu().numpy() for t in ops.rp3_rows(ctx, *dev, N, i, i + 1)]
    assert one[2][0] == cnt[i] and np.array_equal(one[0][0, :cnt[i]], idx[i, :cnt[i]])
    assert np.array_equal(bits(one[1][0, :cnt[i]]), bits(val[i, :cnt[i]]))
    for normalize in (False, True):
        W, Wv = ops.rp3_cut(ctx, *(torch.from_numpy(a).to(ctx.device) for a in (idx, val, cnt)), N, normalize)
        assert_w_equal(host_w(W, Wv), rp3_ref.cut(idx, val, cnt, I, N, normalize)[0])


@pytest.mark.parametrize("n", range(GOLDEN_CASES))
def test_scoring_on_reference_w_matches_reference_lists(ctx, golden, n):
    from elliot_amd import ops
    z, R, tag, *_ = golden_case(golden, n)
    Rc = case_matrix(R, tag)
    Wr = reference_w(z, tag, R.shape[1])
    Rd, Rv = ops.DeviceCSR(Rc.indptr, Rc.indices, Rc.shape[1], ctx.device), ops.device_values(Rc.data, ctx.device)
    Wd, Wv = ops.DeviceCSR(Wr.indptr, Wr.indices, Wr.shape[1], ctx.device), ops.device_values(Wr.data, ctx.device)
    idx, val = ops.knn_score_topk(ctx, Rd, Rv, Wd, Wv, 0, R.shape[0], int(z["k"]), excl=Rd)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    ri, rv = z[f"{tag}_rec_idx"], z[f"{tag}_rec_val"]
    assert np.array_equal(bits(val), bits(rv))
    assert knn_ref.cut_ties_equal(idx, val, ri, rv)


def test_deterministic_bytes(ctx, golden):
    from elliot_amd import ops
    z, R, tag, N, alpha, beta, norm = golden_case(golden, 1)
    outs = []
    for _ in range(2):
        operands = ops.rp3_operands(ctx, case_matrix(R, tag), alpha, beta)
        lists = ops.rp3_rows(ctx, *operands, N)
        W, Wv = ops.rp3_cut(ctx, *lists, N, norm)
        cnt = lists[2].cpu().numpy()
        used = np.arange(lists[0].shape[1])[None, :] < cnt[:, None]
        outs.append([lists[0].cpu().numpy()[used].tobytes(), lists[1].cpu().numpy()[used].tobytes(), cnt.tobytes()] +
                    [t.cpu().numpy().tobytes() for t in (W.indptr, W.indices, Wv)])
    assert outs[0] == outs[1]


def test_neighborhood_beyond_the_limit_is_an_error(ctx):
    from elliot_amd import _lib, ops
    rs = np.random.RandomState(0)
    R = sp.random(400, 2100, density=0.01, random_state=rs, format="csr", dtype=np.float32)
    operands = ops.rp3_operands(ctx, R, 1.0, 0.6)
    with pytest.raises(_lib.ElliotHipError, match="2048"):
        ops.rp3_build(ctx, *operands, 2049, False)
    with pytest.raises(_lib.ElliotHipError, match="2048"):
        ops.rp3_build(ctx, *operands, -1, False)
    W, _ = ops.rp3_build(ctx, *operands, 2048, False)                     # the limit itself is served
    assert W.n_rows == 2100
