"""GPU kernels of KaHFM: el_kahfm_init against the reference's start tables, el_bprsgd_apply / el_bprsgd_apply_levels on rows too
wide for k_bprsgd_apply (k_bprsgd_apply_wide).  Every table has a guard row of sentinels behind it.

The parity bound of the wide kernel is derived, not tuned.  With the exact dot products (every product split into two doubles by
Dekker's algorithm, all of them added by math.fsum) any summation order satisfies |x - x_exact| <= gamma_F sum|p_f q_f| with
gamma_F = F u / (1 - F u), u = 2^-53; z = 1 / (1 + exp(x_ui - x_uj)) has |dz/dx| <= 1/4, so
|z_gpu - z_exact| <= 1/4 gamma_F (sum|p q_i| + sum|p q_j|) + 4 ulp(z) (exp, the add, the divide).  z_gpu is read back from the
updated biases (b = 0, reg_bias = 0, lr = 1/2: b_i' = z / 2 exactly).  The new rows must equal the NumPy update computed from the
GPU's own z to within 2 ulp per element."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from elliot_amd import ops
from elliot_amd._lib import BprsgdState
from elliot_amd.recommender import attribute_profiles as ap
from oracle import sgd as osgd
from tests.helpers import kahfm_ref as kr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
HP = dict(lr=0.5, reg_bias=0.0, reg_user=0.0025, reg_pos=0.0025, reg_neg=0.00025)


def cpu(t):
    return t.detach().cpu().numpy()


class GuardedState(ops.BprSgdDeviceState):
    """BprSgdDeviceState on tables with one more row (b: one more cell) of sentinels behind them, in the same allocation;
    `shift`: the tables start 8 bytes into their buffers (not 16-byte aligned)."""

    def __init__(self, ctx, P, Q, b, hp, shift=False):
        self.ctx = ctx
        dev = ctx.device
        (self.U, self.F), self.I = P.shape, Q.shape[0]
        off = 1 if shift else 0

        def guarded(x, cells):
            buf = torch.full((off + x.size + cells,), SENTINEL, dtype=torch.float64, device=dev)
            buf[off:off + x.size] = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev)
            return buf
        self._buf = [guarded(P, self.F), guarded(Q, self.F), guarded(b, 1)]
        self.P = self._buf[0][off:off + P.size].view(self.U, self.F)
        self.Q = self._buf[1][off:off + Q.size].view(self.I, self.F)
        self.b = self._buf[2][off:off + b.size]
        assert (self.P.data_ptr() % 16 == 8) == shift
        self._c = BprsgdState(P=self.P.data_ptr(), Q=self.Q.data_ptr(), b=self.b.data_ptr(), U=self.U, I=self.I, F=self.F,
                              **{k: float(v) for k, v in hp.items()})
        self._off = off

    def guards_intact(self):
        torch.cuda.synchronize()
        sizes = (self.U * self.F, self.I * self.F, self.I)
        return all(bool((buf[:self._off] == SENTINEL).all()) and bool((buf[self._off + n:] == SENTINEL).all()) and buf[self._off + n:].numel() > 0
                   for buf, n in zip(self._buf, sizes))


def two_product(a, b):
    """(hi, lo) with hi + lo = a * b exactly (Dekker; no overflow or underflow at these magnitudes)."""
    split = 134217729.0                                          # 2^27 + 1
    hi = a * b
    ca, cb = split * a, split * b
    a1, b1 = ca - (ca - a), cb - (cb - b)
    a2, b2 = a - a1, b - b1
    return hi, a2 * b2 - (((hi - a1 * b1) - a2 * b1) - a1 * b2)


def exact_z(p, qi, qj):
    """(z from the correctly rounded x_ui - x_uj, sum|p q_i| + sum|p q_j|) for one triplet with zero biases."""
    hi_i, lo_i = two_product(p, qi)
    hi_j, lo_j = two_product(p, qj)
    x = math.fsum(np.concatenate([hi_i, lo_i, -hi_j, -lo_j]).tolist())
    return 1.0 / (1.0 + math.exp(x)), float(np.abs(hi_i).sum() + np.abs(hi_j).sum())


def numpy_update(P, Q, u, i, j, z, hp):
    """update_factors (kahfm_model.py:133-164) for conflict-free triplets with the given z per triplet, vectorised."""
    z = z[:, None]
    pu, qi, qj = P[u], Q[i], Q[j]
    nu = pu + hp["lr"] * ((qi - qj) * z - hp["reg_user"] * pu)
    ni = qi + hp["lr"] * (nu * z - hp["reg_pos"] * qi)
    nj = qj + hp["lr"] * (-nu * z - hp["reg_neg"] * qj)
    return nu, ni, nj


def within_ulps(got, exp, n):
    return bool(np.all(np.abs(got - exp) <= n * np.spacing(np.abs(exp))))


# ---- el_kahfm_init --------------------------------------------------------------------------------------------------------------
def guarded_tables(dev, U, I, nF):
    bp = torch.full((U + 1, nF), SENTINEL, dtype=torch.float64, device=dev)
    bq = torch.full((I + 1, nF), SENTINEL, dtype=torch.float64, device=dev)
    return bp, bq


@pytest.mark.parametrize("tag", kr.CASES)
def test_kahfm_init_equals_the_reference_start_tables(ctx, golden, tmp_path, tag):
    fx = kr.load(golden("kahfm_ref.npz"), tag, tmp_path)
    side = fx.data.side_information.ChainedKG
    F, w = ap.item_features(fx.data, side, ap.item_tfidf(side.feature_map))
    indptr, indices = ap.train_rows_in_dict_order(fx.data)
    U, (I, nF) = fx.data.num_users, F.shape
    runs = []
    for _ in range(2):
        bp, bq = guarded_tables(ctx.device, U, I, nF)
        P0, Q0 = ops.kahfm_init(ctx, indptr, indices, F, w, P0=bp[:U], Q0=bq[:I])
        assert bool((bp[U] == SENTINEL).all()) and bool((bq[I] == SENTINEL).all())
        runs.append((cpu(P0), cpu(Q0)))
    assert kr.same_bits(runs[0][0], fx.z[f"{tag}_P0"]) and kr.same_bits(runs[0][1], fx.z[f"{tag}_Q0"])
    assert kr.same_bits(runs[0][0], runs[1][0]) and kr.same_bits(runs[0][1], runs[1][1])


def test_kahfm_init_empty_rows_last_writer_and_more_than_one_tile(ctx):
    """nF spans two LDS tiles; user 1 has no item, item 2 no feature; users 0 and 2 meet feature 5 and the last feature twice with
    different weights (the later item wins); a weight of zero stays +0.0 / len."""
    nF, I = 8192 + 37, 4
    rows = [[5, 8191, 8192, nF - 1], [5, 7, nF - 1], [], [0, 5, 8200]]
    F = sp.csr_matrix((np.ones(10, np.float32), np.concatenate(rows).astype(np.int32), np.cumsum([0] + [len(r) for r in rows])), shape=(I, nF))
    w = np.array([0.5, 0.25, 0.125, 0.75, 0.3, 0.0, 0.9, 0.1, 0.7, 0.6])
    indptr, indices = np.array([0, 3, 3, 6], np.int64), np.array([0, 2, 1, 3, 1, 0], np.int32)
    bp, bq = guarded_tables(ctx.device, 3, I, nF)
    P0, Q0 = ops.kahfm_init(ctx, indptr, indices, F, w, P0=bp[:3], Q0=bq[:I])
    assert bool((bp[3] == SENTINEL).all()) and bool((bq[I] == SENTINEL).all())
    eQ = np.zeros((I, nF))
    eQ[np.repeat(np.arange(I), np.diff(F.indptr)), F.indices] = w
    eP = np.zeros((3, nF))
    for u in (0, 2):
        row = indices[indptr[u]:indptr[u + 1]]
        last = {}
        for i in row:
            last.update({int(f): w[a] for a, f in zip(range(F.indptr[i], F.indptr[i + 1]), F.indices[F.indptr[i]:F.indptr[i + 1]])})
        for f, v in last.items():
            eP[u, f] = v / len(row)
    assert kr.same_bits(cpu(Q0), eQ) and kr.same_bits(cpu(P0), eP)
    assert eP[0, 5] == 0.3 / 3 and eP[2, 5] == 0.5 / 3 and eP[0, 7] == 0.0 and not np.signbit(cpu(P0)[1]).any()


# ---- el_bprsgd_apply on wide rows ---------------------------------------------------------------------------------------------
N_MAX = 300


def wide_case(F, seed):
    """Random tables of 300 users x 600 items and 300 conflict-free triplets whose first is (last user, first item, last item) and
    whose second holds the first user."""
    rs = np.random.RandomState(seed)
    U, I = N_MAX, 2 * N_MAX
    P, Q = rs.normal(scale=0.1, size=(U, F)), rs.normal(scale=0.1, size=(I, F))
    u = np.concatenate([[U - 1, 0], 1 + rs.permutation(U - 2)]).astype(np.int32)
    items = np.concatenate([[0], 1 + rs.permutation(I - 2), [I - 1]])
    i, j = items[:N_MAX].astype(np.int32), items[N_MAX:][::-1].astype(np.int32).copy()
    assert (u[0], i[0], j[0]) == (U - 1, 0, I - 1) and len(set(u)) == N_MAX and len(set(i) | set(j)) == 2 * N_MAX
    return P, Q, np.zeros(I), u, i, j


def apply_once(ctx, P, Q, b, u, i, j, n, shift=False):
    st = GuardedState(ctx, P, Q, b, HP, shift=shift)
    d = ctx.device
    st.apply(torch.from_numpy(u).to(d), torch.from_numpy(i).to(d), torch.from_numpy(j).to(d), 0, n)
    assert st.guards_intact()
    return cpu(st.P), cpu(st.Q), cpu(st.b)


def check_wide(ctx, F, shift=False):
    P, Q, b, u, i, j = wide_case(F, seed=F)
    exact = [exact_z(P[u[t]], Q[i[t]], Q[j[t]]) for t in range(N_MAX)]
    z_exact, mass = np.array([e[0] for e in exact]), np.array([e[1] for e in exact])
    gamma = F * 2.0 ** -53 / (1.0 - F * 2.0 ** -53)
    bound = 0.25 * gamma * mass + 4 * np.spacing(z_exact)
    for n in (1, 3, N_MAX):
        gP, gQ, gb = apply_once(ctx, P, Q, b, u, i, j, n, shift)
        uu, ii, jj = u[:n], i[:n], j[:n]
        z = 2.0 * gb[ii]                                         # b_i' = 0 + 1/2 (z - 0 * 0)
        assert np.array_equal(gb[jj], -gb[ii])
        err = np.abs(z - z_exact[:n])
        print(f"F={F} n={n} shift={shift}: max |z_gpu - z_exact| {err.max():.3e}, smallest bound {bound[:n].min():.3e}")
        assert np.all(err <= bound[:n]), (F, n, err.max())
        nu, ni, nj = numpy_update(P, Q, uu, ii, jj, z, HP)
        assert within_ulps(gP[uu], nu, 2) and within_ulps(gQ[ii], ni, 2) and within_ulps(gQ[jj], nj, 2)
        rest_u, rest_i = np.setdiff1d(np.arange(P.shape[0]), uu), np.setdiff1d(np.arange(Q.shape[0]), np.concatenate([ii, jj]))
        assert kr.same_bits(gP[rest_u], P[rest_u]) and kr.same_bits(gQ[rest_i], Q[rest_i]) and not gb[rest_i].any()
    again = apply_once(ctx, P, Q, b, u, i, j, N_MAX, shift)
    assert all(kr.same_bits(a, g) for a, g in zip(again, (gP, gQ, gb)))         # the same call from the same start: the same bytes


@pytest.mark.parametrize("F", [301, 513, 514, 1023, 4096, 4097, 8191])
def test_bprsgd_apply_wide_rows(ctx, F):
    """301: odd, above the scalar limit of k_bprsgd_apply (256); 513 / 514: just above its limit of 512, scalar and 16-byte pieces;
    1023: scalar, four pieces per lane; 4096: the widest register-held shape; 4097 / 8191: the two-pass loop."""
    check_wide(ctx, F)


@pytest.mark.parametrize("F", [514, 4100])
def test_bprsgd_apply_wide_rows_in_unaligned_tables(ctx, F):
    """An even F in tables that are not 16-byte aligned takes the scalar pieces (514: registers; 4100: the loop)."""
    check_wide(ctx, F, shift=True)


def test_narrow_rows_keep_their_kernel(ctx):
    """The shapes k_bprsgd_apply accepts never reach the wide kernel: F = 512 (its widest) and F = 35."""
    for F, wide in ((35, False), (512, False), (514, True)):
        P, Q, b, u, i, j = wide_case(F, seed=1)
        st = ops.BprSgdDeviceState(ctx, P, Q, b, **HP)
        d = ctx.device
        ctx.timing(True)
        try:
            st.apply(torch.from_numpy(u).to(d), torch.from_numpy(i).to(d), torch.from_numpy(j).to(d))
            names = set(ctx.timing_report())
        finally:
            ctx.timing(False)
        assert names == ({"k_bprsgd_apply_wide"} if wide else {"k_bprsgd_apply"}), (F, names)


# ---- el_bprsgd_apply_levels ---------------------------------------------------------------------------------------------------
def update_factors_fsum(P, Q, b, u, i, j, lr, reg_bias, reg_user, reg_pos, reg_neg):
    """oracle.sgd.update_factors with both dot products summed by math.fsum."""
    pu, qi, qj = P[u].copy(), Q[i].copy(), Q[j].copy()
    bi, bj = b[i], b[j]
    z = 1 / (1 + np.exp((0 + bi + math.fsum(pu * qi)) - (0 + bj + math.fsum(pu * qj))))
    b[i] = bi + lr * (z - reg_bias * bi)
    b[j] = bj + lr * (-z - reg_bias * bj)
    pu_new = pu + lr * ((qi - qj) * z - reg_user * pu)
    P[u] = pu_new
    Q[i] = qi + lr * (pu_new * z - reg_pos * qi)
    Q[j] = qj + lr * (-pu_new * z - reg_neg * qj)


def test_bprsgd_levels_on_wide_rows_equal_the_sequential_oracle(ctx):
    """2000 triplets over 20 users x 30 items (every row is shared by many triplets), F = 600.  The bound is the oracle's own
    sensitivity to the summation order measured on these inputs (`@` against math.fsum), times 4, floor 1e-12."""
    rs = np.random.RandomState(21)
    U, I, F, n = 20, 30, 600, 2000
    hp = dict(lr=0.05, reg_bias=0.01, reg_user=0.0025, reg_pos=0.0025, reg_neg=0.00025)
    P0, Q0, b0 = rs.normal(scale=0.1, size=(U, F)), rs.normal(scale=0.1, size=(I, F)), rs.normal(scale=0.1, size=I)
    u, i = rs.randint(0, U, n).astype(np.int32), rs.randint(0, I, n).astype(np.int32)
    j = ((i + 1 + rs.randint(0, I - 1, n)) % I).astype(np.int32)
    assert (i != j).all() and {0, U - 1} <= set(u) and {0, I - 1} <= set(i) | set(j)
    P, Q, b = P0.copy(), Q0.copy(), b0.copy()
    osgd.train_sequential(P, Q, b, u, i, j, **hp)
    Pf, Qf, bf = P0.copy(), Q0.copy(), b0.copy()
    for t in range(n):
        update_factors_fsum(Pf, Qf, bf, int(u[t]), int(i[t]), int(j[t]), **hp)
    d_reorder = max(np.abs(P - Pf).max(), np.abs(Q - Qf).max(), np.abs(b - bf).max())
    bound = max(4 * d_reorder, 1e-12)
    runs = []
    for _ in range(2):
        st = GuardedState(ctx, P0, Q0, b0, hp)
        levels = st.apply_sequential_equivalent(u, i, j)
        assert st.guards_intact() and levels > n // 15
        runs.append((cpu(st.P), cpu(st.Q), cpu(st.b)))
    err = max(np.abs(runs[0][0] - P).max(), np.abs(runs[0][1] - Q).max(), np.abs(runs[0][2] - b).max())
    print(f"levels {levels}, d_reorder {d_reorder:.3e}, bound {bound:.3e}, max |gpu - oracle| {err:.3e}")
    assert err <= bound
    assert all(kr.same_bits(a, g) for a, g in zip(*runs))
