"""GPU: the EASE^R kernels -- el_ease_gram, el_inv_f64, el_ease_weights, el_csr_dense_scores + el_dense_topk -- against exact
integer products, NumPy / SciPy in float64 and the reference's own B (tests/golden/ease_ref.npz)."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import torch

from elliot_amd import ops
from tests.helpers import ease_ref

pytestmark = pytest.mark.gpu


def dev(a, ctx, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def ratings(U, I, density, seed, half=False):
    rs = np.random.RandomState(seed)
    M = sp.random(U, I, density=density, format="csr", random_state=rs, dtype=np.float64)
    M.data = rs.randint(1, 11 if half else 6, M.nnz) * (0.5 if half else 1.0)
    M = sp.csr_matrix(M, dtype=np.float32)
    M.sort_indices()
    return M


def exact_gram_rows(R, rows, l2):
    R64 = sp.csr_matrix(R, dtype=np.float64)
    G = (R64.T[rows] @ R64).toarray()
    n = np.diff(sp.csc_matrix(R).indptr)
    G[np.arange(len(rows)), rows] = (n[rows] + l2).astype(np.float32).astype(np.float64)
    return G


# ---- Gram -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
def test_gram_exact_symmetric_repeatable(ctx, half):
    R = ratings(700, 1037, 0.05, 3, half)
    G1 = ops.ease_gram(ctx, R, 13.7).cpu().numpy()
    G2 = ops.ease_gram(ctx, R, 13.7).cpu().numpy()
    assert np.array_equal(G1, exact_gram_rows(R, np.arange(R.shape[1]), 13.7))
    assert np.array_equal(G1, G1.T)
    assert G1.tobytes() == G2.tobytes()
    assert np.array_equal(G1, ease_ref.gram(R, 13.7))


def count_bound(R):
    """The largest magnitude a Gram count can reach: the longest column times the largest rating squared."""
    return float(np.diff(sp.csc_matrix(R).indptr).max()) * float(np.abs(R.data).max()) ** 2


def test_gram_wide_counts_use_the_int64_counters(ctx):
    """max degree x max |r|^2 beyond int32 (and below 2^53, so the fp64 products of the check are exact): 64-bit LDS counters."""
    rs = np.random.RandomState(5)
    R = sp.random(300, 120, density=0.3, random_state=rs, format="csr", dtype=np.float32)
    R.data[:] = rs.randint(1, 20001, size=R.nnz)
    R.data[:5] = 20000
    assert 2 ** 31 - 1 < count_bound(R) < 2 ** 53
    G1 = ops.ease_gram(ctx, R, 13.7).cpu().numpy()
    G2 = ops.ease_gram(ctx, R, 13.7).cpu().numpy()
    assert np.array_equal(G1, exact_gram_rows(R, np.arange(R.shape[1]), 13.7))
    assert np.array_equal(G1, G1.T)
    assert G1.tobytes() == G2.tobytes()


@pytest.mark.parametrize("wide", [False, True])
def test_gram_more_than_one_lds_tile(ctx, wide):
    """I > 16 384: every row of G is counted in two passes over the columns.  wide: ratings of 40 000 to 60 000, so the 64-bit
    counters take the two passes and most sampled cells exceed int32."""
    R = ratings(2500, 16384 + 917, 0.002, 5)
    rows = np.array([0, 1, 4097, 16383, 16384, 16385, R.shape[1] - 1])
    if wide:
        R.data[:] = np.random.RandomState(6).randint(40000, 60001, size=R.nnz)
        assert 2 ** 31 - 1 < count_bound(R) < 2 ** 53
        assert (exact_gram_rows(R, rows, 1000.0) > 2 ** 31).sum() > 500
    G = ops.ease_gram(ctx, R, 1000.0)
    got = G[torch.from_numpy(rows).to(ctx.device)].cpu().numpy()
    assert np.array_equal(got, exact_gram_rows(R, rows, 1000.0))
    again = ops.ease_gram(ctx, R, 1000.0)[torch.from_numpy(rows).to(ctx.device)].cpu().numpy()
    assert got.tobytes() == again.tobytes()


def test_gram_refuses_other_ratings(ctx):
    R = ratings(50, 40, 0.2, 1)
    R.data[0] = 1.3
    with pytest.raises(ValueError, match="half-step"):
        ops.ease_gram(ctx, R, 1.0)


# ---- inverse --------------------------------------------------------------------------------------------------------------------
def matrix(kind, n, seed):
    rs = np.random.RandomState(seed)
    A = rs.normal(size=(n, n))
    if kind == "spd":
        return A @ A.T / n + np.eye(n)
    if kind == "sym_indef":
        S = (A + A.T) / 2
        return S + np.diag(rs.choice([-1.0, 1.0], n) * 3.0)
    if kind == "zero_diag":                                   # every step must swap
        A[np.diag_indices(n)] = 0.0
        return A
    return A


def check_inverse(ctx, A):
    n = A.shape[0]
    Ad = dev(A, ctx, np.float64)
    ipiv = ops.inv_f64(ctx, Ad)
    X = Ad.cpu().numpy()
    Xn = np.linalg.inv(A)
    cond = np.abs(A).sum(axis=0).max() * np.abs(Xn).sum(axis=0).max()          # the 1-norm condition number
    tol = max(cond, 1.0) * 1e-14
    resid = np.abs(A @ X - np.eye(n)).max()
    assert resid <= tol * max(1.0, np.abs(A).max() * np.abs(X).max() * n ** 0.5), (resid, cond)
    assert np.abs(X - Xn).max() <= tol * np.abs(Xn).max(), (np.abs(X - Xn).max() / np.abs(Xn).max(), cond)
    return ipiv.cpu().numpy(), X


@pytest.mark.parametrize("n", [1, 17, 1000, 2053, 4097, 8192 + 5])
def test_inverse_general(ctx, n):
    check_inverse(ctx, matrix("general", n, n))


@pytest.mark.parametrize("kind", ["spd", "sym_indef", "zero_diag"])
@pytest.mark.parametrize("n", [17, 1000, 2053])
def test_inverse_kinds(ctx, kind, n):
    ipiv, _ = check_inverse(ctx, matrix(kind, n, n + 1))
    if kind == "zero_diag":
        assert ipiv[0] != 0                                   # a zero diagonal: the first step cannot keep its row


@pytest.mark.parametrize("n", [300, 2053])
def test_pivots_equal_lapack(ctx, n):
    """A permuted, strongly diagonal matrix: every pivot is far ahead of the rest of its column, so getrf's choice is unique."""
    rs = np.random.RandomState(n)
    M = rs.uniform(-0.1, 0.1, size=(n, n)) + np.diag(10.0 + rs.rand(n))
    A = M[rs.permutation(n)]
    ipiv, _ = check_inverse(ctx, A)
    lu, piv = scipy.linalg.lu_factor(A)
    assert np.array_equal(ipiv, piv.astype(np.int32))
    Ad = dev(A, ctx, np.float64)
    ipiv2 = ops.lu_f64(ctx, Ad).cpu().numpy()                  # the factorisation alone (getrf)
    assert np.array_equal(ipiv2, ipiv)
    assert np.abs(Ad.cpu().numpy() - lu).max() <= 1e-12 * np.abs(lu).max()


def test_inverse_repeatable_bits(ctx):
    A = matrix("sym_indef", 2053, 7)
    outs = []
    for _ in range(2):
        Ad = dev(A, ctx, np.float64)
        ipiv = ops.inv_f64(ctx, Ad)
        outs.append((Ad.cpu().numpy().tobytes(), ipiv.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("how,col", [("zero_column", 5), ("duplicate_rows", 99)])
def test_singular_raises_and_device_stays_healthy(ctx, how, col):
    A = matrix("general", 100, 3)
    if how == "zero_column":
        A[:, 5] = 0.0
    else:
        A[40] = A[12]
    with pytest.raises(np.linalg.LinAlgError, match=f"column {col}\\b"):
        ops.inv_f64(ctx, dev(A, ctx, np.float64))
    check_inverse(ctx, matrix("general", 64, 4))


# ---- weights --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["rat_l5", "rat_l1320", "bin_l50"])
def test_weights(ctx, golden, tag):
    g = golden("ease_ref.npz")
    R = sp.csr_matrix((g[f"{tag}_R_data"], g[f"{tag}_R_indices"], g[f"{tag}_R_indptr"]), shape=tuple(g[f"{tag}_shape"]))
    l2 = float(g[f"{tag}_l2"])
    G = ops.ease_gram(ctx, R, l2)
    ops.inv_f64(ctx, G)
    P = G.cpu().numpy()
    B = ops.ease_weights(ctx, G).cpu().numpy()
    assert np.array_equal(B.view(np.int32), ease_ref.weights(P).view(np.int32))      # the rule, bit for bit, on the device's P
    G64 = ease_ref.gram(R, l2)
    B64 = -np.linalg.inv(G64) / np.diag(np.linalg.inv(G64))[None, :]
    B64[np.diag_indices(B64.shape[0])] = 0.0
    cond = np.linalg.cond(G64, 1)
    ulp = np.spacing(np.abs(B64).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(B - B64) <= ulp + cond * 1e-15 * np.abs(B64).max())
    Bref = g[f"{tag}_B"]
    assert np.abs(B.astype(np.float64) - Bref).max() <= 1e-6 * np.abs(Bref).max()


# ---- scoring --------------------------------------------------------------------------------------------------------------------
def lists(ctx, R, B, start, stop, k, excl=None, cand=None):
    st = ops.EaseDeviceState.__new__(ops.EaseDeviceState)
    st.ctx, st.U, st.I = ctx, R.shape[0], R.shape[1]
    st.R = ops.DeviceCSR(R.indptr, R.indices, R.shape[1], ctx.device)
    st.R_vals = ops.device_values(R.data, ctx.device)
    st.B, st._S, st.block_rows = dev(B, ctx, np.float32), None, 97                 # several blocks per call
    mask = ("excl", excl) if excl is not None else (("cand", cand) if cand is not None else None)
    idx, val = st.recommend(mask, k, start, stop)
    return idx.cpu().numpy(), val.cpu().numpy()


@pytest.mark.parametrize("tag", ["rat_l5", "rat_l1320", "bin_l50"])
def test_scores_bit_equal_scipy_with_reference_B(ctx, golden, tag):
    g = golden("ease_ref.npz")
    R = sp.csr_matrix((g[f"{tag}_R_data"], g[f"{tag}_R_indices"], g[f"{tag}_R_indptr"]), shape=tuple(g[f"{tag}_shape"]))
    Bref = g[f"{tag}_B"]
    U, I = R.shape
    Rd = ops.DeviceCSR(R.indptr, R.indices, I, ctx.device)
    S = ops.csr_dense_scores(ctx, Rd, ops.device_values(R.data, ctx.device), dev(Bref, ctx, np.float32), 0, U).cpu().numpy()
    assert np.array_equal(S.view(np.int32), R.dot(Bref).view(np.int32))
    idx, val = lists(ctx, R, Bref, 0, U, 10, excl=Rd)
    eidx, evals = ease_ref.topk(R.dot(Bref), (R.indptr, R.indices), 10)
    assert np.array_equal(idx, eidx) and np.array_equal(val.view(np.int32), evals.view(np.int32))
    ok = ease_ref.same_lists(g[f"{tag}_rec_idx"], idx, R.dot(Bref))
    assert ok.all(), np.flatnonzero(~ok)


def test_scores_masks_and_ranges(ctx):
    rs = np.random.RandomState(11)
    U, I = 400, 2500                                          # I not a multiple of the 1 024-column slab
    R = ratings(U, I, 0.01, 12)
    R.data = R.data[rs.permutation(R.nnz)]                    # values in no particular order; the stored order is what counts
    B = rs.normal(size=(I, I)).astype(np.float32)
    S = R.dot(B)
    Rd = ops.DeviceCSR(R.indptr, R.indices, I, ctx.device)
    got = ops.csr_dense_scores(ctx, Rd, ops.device_values(R.data, ctx.device), dev(B, ctx, np.float32), 37, 351).cpu().numpy()
    assert np.array_equal(got.view(np.int32), S[37:351].view(np.int32))
    # excl mask, a user range not starting at 0
    idx, val = lists(ctx, R, B, 37, 351, 10, excl=Rd)
    eidx, evals = ease_ref.topk(S, (R.indptr, R.indices), 10)
    assert np.array_equal(idx, eidx[37:351]) and np.array_equal(val.view(np.int32), evals[37:351].view(np.int32))
    # candidate lists, some shorter than k: padded with (-1, -inf)
    cl = [np.sort(rs.choice(I, rs.randint(0, 30), replace=False)) for _ in range(U)]
    cp = np.zeros(U + 1, np.int64)
    cp[1:] = np.cumsum([len(c) for c in cl])
    ci = np.concatenate(cl).astype(np.int32)
    cand = ops.DeviceCSR(cp, ci, I, ctx.device)
    idx, val = lists(ctx, R, B, 5, 400, 20, cand=cand)
    eidx, evals = ease_ref.topk(S, None, 20, cand=(cp, ci))
    assert np.array_equal(idx, eidx[5:]) and np.array_equal(val.view(np.int32), evals[5:].view(np.int32))
    assert (idx == -1).any()
