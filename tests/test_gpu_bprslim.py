"""GPU: the BPRSlim kernels at their edges (el_bprslim_apply, el_bprslim_apply_levels, el_bprslim_table, el_bprslim_scores) against
exact sums, the NumPy expressions of the reference and the reference's own prediction matrix (tests/golden/bprslim_ref.npz).

Bounds of the sum, with u = 2^-53 and gamma_m = m u / (1 - m u): a row of n seen items costs one rounding per difference and at
most n roundings of additions on any path of the kernel's fixed tree (ceil(n / 64) in a lane, 6 shuffle steps, of which those
that add +0 are exact), so |x_gpu - x_exact| <= gamma_{n+1} sum_s (|S_is| + |S_js|).  g = 1 / (1 + exp(x)) has slope <= 1/4; exp,
the addition and the division cost a few ulp of g: |g_gpu - g_exact| <= bound_x / 4 + 4 ulp(g_exact).  Everything after g is
rounded operation by operation in the reference's order, so every cell is compared for equality."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.helpers import bprslim_ref as br

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
I_BIG, PAD_C, PAD_R = 1100, 3, 1
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025]
LR, LI_REG, LJ_REG = 0.05, 0.1, 0.001
_edge = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def gamma(m):
    return m * U53 / (1 - m * U53)


def edge_case():
    """300 conflict-free triplets over 1 100 items, computed once and never written to: users 0..9 hold rows of LENGTHS, user
    10 has seen nothing but the i of triplet 0, user 11 has seen both the i and the j of triplet 1."""
    if _edge:
        return _edge
    rs = np.random.RandomState(11)
    perm = rs.permutation(I_BIG)
    n = 300
    i, j = perm[0:2 * n:2].astype(np.int32), perm[1:2 * n:2].astype(np.int32)
    rows = [np.sort(rs.choice(I_BIG, L, replace=False)) for L in LENGTHS]
    rows.append(np.array([i[0]]))
    rows.append(np.sort(np.concatenate([[i[1], j[1]], rs.choice(np.setdiff1d(np.arange(I_BIG), [i[1], j[1]]), 63, replace=False)])))
    u = np.array([10, 11, 9] + [(t - 3) % len(LENGTHS) for t in range(3, n)], dtype=np.int32)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    S = np.full((I_BIG + PAD_R, I_BIG + PAD_C), np.nan)
    S[:I_BIG, :I_BIG] = rs.normal(scale=0.1, size=(I_BIG, I_BIG))
    S[:I_BIG, I_BIG:] = rs.normal(size=(I_BIG, PAD_C))                       # guard columns
    S[I_BIG:, :] = rs.normal(size=(PAD_R, I_BIG + PAD_C))                    # guard row
    assert len(np.unique(np.concatenate([i, j]))) == 2 * n
    assert set(np.diff(indptr).tolist()) >= set(LENGTHS) and j[1] in rows[11] and any(i[t] in rows[u[t]] for t in range(3, n))
    _edge.update(u=u, i=i, j=j, indptr=indptr, indices=indices, S=S)
    return _edge


def run_apply(ctx, c, n):
    from elliot_amd import ops
    d = ctx.device
    rows = ops.DeviceCSR(c["indptr"], c["indices"], I_BIG, d)
    S = torch.from_numpy(c["S"]).to(d)
    x = torch.full((n,), 7.0, dtype=torch.float64, device=d)
    g = torch.full((n,), 7.0, dtype=torch.float64, device=d)
    t = [torch.from_numpy(c[k][:n].copy()).to(d) for k in "uij"]
    ops.bprslim_apply(ctx, t[0], t[1], t[2], rows, S, LR, LI_REG, LJ_REG, I=I_BIG, x_out=x, g_out=g)
    torch.cuda.synchronize()
    return S.cpu().numpy(), x.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 300])
def test_one_conflict_free_launch(ctx, n):
    c = edge_case()
    S0 = c["S"]
    S1, x, g = run_apply(ctx, c, n)
    want = S0.copy()
    for t in range(n):
        u, i, j = int(c["u"][t]), int(c["i"][t]), int(c["j"][t])
        row = c["indices"][c["indptr"][u]:c["indptr"][u + 1]]
        si, sj = S0[i, row], S0[j, row]
        x_exact = math.fsum(si.tolist() + (-sj).tolist())
        bound_x = gamma(len(row) + 1) * float(np.abs(si).sum() + np.abs(sj).sum())
        g_exact = 1 / (1 + np.exp(x_exact))
        print(f"n={n} t={t} len={len(row)}: |x - x_exact| {abs(x[t] - x_exact):.3e} (bound {bound_x:.3e}), "
              f"|g - g_exact| {abs(g[t] - g_exact):.3e} (bound {bound_x / 4 + 4 * np.spacing(g_exact):.3e})")
        assert abs(x[t] - x_exact) <= bound_x, (t, len(row))
        assert abs(g[t] - g_exact) <= bound_x / 4 + 4 * np.spacing(g_exact), (t, len(row))
        if len(row) == 0:
            assert x[t] == 0.0 and not np.signbit(x[t]) and g[t] == 0.5
        gt = np.float64(g[t])
        keep_i, keep_j = row != i, row != j
        want[i, row[keep_i]] = si[keep_i] + LR * (gt - LI_REG * si[keep_i])                  # bprslim_model.py:62
        want[j, row[keep_j]] = sj[keep_j] - LR * (gt - LJ_REG * sj[keep_j])                  # :65
    assert np.array_equal(bits(S1), bits(want))                              # every other cell, guards included, keeps its bytes
    moved = bits(S1) != bits(S0)
    assert moved[:I_BIG, :I_BIG].any() and not moved[I_BIG:].any() and not moved[:, I_BIG:].any()
    if n >= 1:                                                               # seen = {i}: row i's only seen cell is skipped
        i0, j0 = int(c["i"][0]), int(c["j"][0])
        assert not moved[i0].any() and moved[j0].sum() == 1 and moved[j0, i0]
    if n >= 2:                                                               # a seen j: S[j, j] stays, S[i, j] moves
        i1, j1 = int(c["i"][1]), int(c["j"][1])
        assert not moved[j1, j1] and moved[i1, j1] and not moved[i1, i1] and moved[j1, i1]


def test_same_input_same_bytes(ctx):
    c = edge_case()
    a, b = run_apply(ctx, c, 300), run_apply(ctx, c, 300)
    for p, q in zip(a, b):
        assert np.array_equal(bits(p), bits(q))


def test_first_offsets_the_triplets_and_their_outputs(ctx):
    from elliot_amd import ops
    c = edge_case()
    d = ctx.device
    rows = ops.DeviceCSR(c["indptr"], c["indices"], I_BIG, d)
    S = torch.from_numpy(c["S"]).to(d)
    x = torch.full((300,), 7.0, dtype=torch.float64, device=d)
    t = [torch.from_numpy(c[k]).to(d) for k in "uij"]
    ops.bprslim_apply(ctx, t[0], t[1], t[2], rows, S, LR, LI_REG, LJ_REG, first=5, n=6, I=I_BIG, x_out=x)
    ops.bprslim_apply(ctx, t[0], t[1], t[2], rows, S, LR, LI_REG, LJ_REG, first=0, n=5, I=I_BIG, x_out=x)
    ops.bprslim_apply(ctx, t[0], t[1], t[2], rows, S, LR, LI_REG, LJ_REG, first=11, I=I_BIG, x_out=x)
    torch.cuda.synchronize()
    S_all, x_all, _ = run_apply(ctx, c, 300)
    assert np.array_equal(bits(S.cpu().numpy()), bits(S_all)) and np.array_equal(bits(x.cpu().numpy()), bits(x_all))


def test_equal_i_and_j_follow_the_reference_s_two_statements(ctx):
    """i == j (the sampler never draws it): x = +0 and g = 0.5 exactly, and the second statement reads the cell the first one
    stored, so the restatement's bytes are the kernel's -- on a row that lies partly in the lanes' registers (300 > 256)."""
    from elliot_amd import ops
    rs = np.random.RandomState(21)
    I = 400
    row = np.sort(rs.choice(I, 300, replace=False)).astype(np.int32)
    i = int(row[17])
    S0 = rs.normal(scale=0.3, size=(I, I))
    want = S0.copy()
    assert br.step(want, row, i, i, LR, LI_REG, LJ_REG) == 0.0
    d = ctx.device
    S = torch.from_numpy(S0).to(d)
    x, g = (torch.full((1,), 7.0, dtype=torch.float64, device=d) for _ in range(2))
    t = [torch.tensor([v], dtype=torch.int32, device=d) for v in (0, i, i)]
    ops.bprslim_apply(ctx, t[0], t[1], t[2], ops.DeviceCSR(np.array([0, 300]), row, I, d), S, LR, LI_REG, LJ_REG, x_out=x, g_out=g)
    assert x.item() == 0.0 and g.item() == 0.5
    got = S.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and (bits(got) != bits(S0)).sum() == 299


def test_levels_follow_the_sequential_restatement(ctx):
    from elliot_amd import ops
    rs = np.random.RandomState(3)
    U, I, n = 20, 30, 2000
    M = rs.rand(U, I) < 0.3
    M[4, :] = False                                                          # a user who has seen nothing
    M[5, :] = False
    M[5, 12] = True
    R = sp.csr_matrix(M.astype(np.float64))
    u = rs.randint(0, U, n)
    i = rs.randint(0, I, n)
    j = (i + 1 + rs.randint(0, I - 1, n)) % I
    trip = np.stack([u, i, j]).astype(np.int32)
    S_left, S_fsum = np.zeros((I, I)), np.zeros((I, I))
    x_left = br.train(S_left, R.indptr, R.indices, trip, LR, LI_REG, LJ_REG)
    br.train(S_fsum, R.indptr, R.indices, trip, LR, LI_REG, LJ_REG, chain="fsum")
    own = float(np.abs(S_left - S_fsum).max())
    bound = max(4 * own, 1e-12)
    st = ops.BprSlimDeviceState(ctx, R, LR, LI_REG, LJ_REG)
    n_levels, x = st.apply_sequential_equivalent(u, i, j)
    S = st.S.cpu().numpy()
    err = float(np.abs(S - S_left).max())
    print(f"levels {n_levels}; max |S - sequential| {err:.3e} (the restatement's own chain against fsum {own:.3e}, bound {bound:.3e})")
    assert n_levels == len(br.levels(i, j, I)[2]) - 1
    assert err <= bound
    assert not np.diag(S).any()
    # x_t sums at most L differences of cells that are each within `bound`; the chain and the tree are each within
    # gamma_{L+1} sum |S| of the exact sum of their cells
    L = int(np.diff(R.indptr).max())
    bound_x = 2 * L * bound + 2 * gamma(L + 1) * 2 * L * float(np.abs(S_left).max())
    assert float(np.abs(x - x_left).max()) <= bound_x
    assert st.St is None


@pytest.mark.parametrize("I", [1, 31, 33, 84])
def test_table_is_the_transpose(ctx, I):
    from elliot_amd import ops
    rs = np.random.RandomState(I)
    S = rs.normal(size=(I + 1, I + 5))
    out = np.full((I + 2, I + 3), -7.25)
    St = torch.from_numpy(out.copy()).to(ctx.device)
    ops.bprslim_table(ctx, torch.from_numpy(S).to(ctx.device), out=St, I=I)
    got = St.cpu().numpy()
    assert np.array_equal(bits(got[:I, :I]), bits(S[:I, :I].T.copy()))
    got[:I, :I] = -7.25
    assert np.array_equal(bits(got), bits(out))                              # the padding keeps its bytes
    fresh = ops.bprslim_table(ctx, torch.from_numpy(np.ascontiguousarray(S[:I, :I])).to(ctx.device))
    assert fresh.shape == (I, I) and np.array_equal(bits(fresh.cpu().numpy()), bits(S[:I, :I].T.copy()))


def test_scores_equal_the_reference_s_predictions(ctx, golden):
    from elliot_amd import ops
    g = golden("bprslim_ref.npz")
    indptr, indices, U, I = br.case(g, "plain")
    indptr, indices = br.sorted_rows(indptr, indices)
    S, pred = g["plain_S"][-1], g["plain_pred"]
    # an empty row in the middle: every later user moves up by one
    E = 5
    indptr2 = np.concatenate([indptr[:E + 1], indptr[E:]])
    want = np.concatenate([pred[:E], np.zeros((1, I)), pred[E:]])
    rows = ops.DeviceCSR(indptr2, indices, I, ctx.device)
    St = ops.bprslim_table(ctx, torch.from_numpy(S).to(ctx.device))
    got = ops.bprslim_scores(ctx, rows, St, 0, U + 1).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert not got[E].any() and not np.signbit(got[E]).any()                 # +0.0, the sign bit included
    # u_start > 0, into a wider block whose other cells keep their bytes
    P = torch.full((U, I + 2), -7.25, dtype=torch.float64, device=ctx.device)
    ops.bprslim_scores(ctx, rows, St, 3, U + 1, out=P)
    P = P.cpu().numpy()
    assert np.array_equal(bits(P[:U - 2, :I]), bits(want[3:]))
    assert (P[U - 2:] == -7.25).all() and (P[:, I:] == -7.25).all()


def test_scores_of_a_long_row_keep_the_stored_order(ctx):
    """More items than one slab of targets and a row whose stored order is not ascending: the chain runs in stored order."""
    from elliot_amd import ops
    rs = np.random.RandomState(9)
    I = 1100
    S = rs.normal(size=(I, I)) * 10.0 ** rs.randint(-8, 8, size=(I, I))
    row = rs.permutation(I)[:300].astype(np.int32)
    indptr = np.array([0, 300], dtype=np.int64)
    want = br.predictions(indptr, row, S)
    St = ops.bprslim_table(ctx, torch.from_numpy(S).to(ctx.device))
    got = ops.bprslim_scores(ctx, ops.DeviceCSR(indptr, row, I, ctx.device), St, 0, 1).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(br.predictions(indptr, np.sort(row), S)), bits(want))     # the order does matter here
