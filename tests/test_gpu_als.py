"""GPU: el_als_gram / el_als_solve against the NumPy restatement (tests/helpers/als_ref.py), and three ALS iterations through
ops.AlsDeviceState against the reference's own X, Y and lists (tests/golden/als_*_ref.npz)."""
import numpy as np
import pytest
import torch

from elliot_amd import ops
from elliot_amd.recommender.latent_factor_models.als_model import ials_weights, wrmf_weights
from elliot_amd.synthetic import zipf_csr
from tests.helpers import als_ref

pytestmark = pytest.mark.gpu


def dev64(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.device)


@pytest.mark.parametrize("F", [8, 20, 64, 128])
def test_gram_matches_numpy_symmetric_and_repeatable(ctx, F):
    Y = np.random.RandomState(F).normal(size=(70001, F))
    Yd = dev64(Y, ctx)
    G1 = ops.als_gram(ctx, Yd).cpu().numpy()
    G2 = ops.als_gram(ctx, Yd).cpu().numpy()
    ref = Y.T.dot(Y)
    assert np.abs(G1 - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(G1, G1.T)
    assert G1.tobytes() == G2.tobytes()


def solve_case(ctx, F, indptr, indices, I, seed, skip_empty=False, piece_len=ops.ALS_PIECE_LEN):
    rs = np.random.RandomState(seed)
    U = indptr.shape[0] - 1
    Y = rs.normal(scale=0.1, size=(I, F))
    X0 = rs.normal(size=(U, F))
    Yd = dev64(Y, ctx)
    G = ops.als_gram(ctx, Yd)
    pat = ops.AlsCSR(indptr, indices, I, ctx.device, piece_len)
    out = []
    for _ in range(2):
        Xd = dev64(X0, ctx)
        ops.als_solve(ctx, pat, Yd, G, 1.5, 2.5, 0.1, Xd, skip_empty=skip_empty)
        out.append(Xd.cpu().numpy())
    ref = als_ref.half(G.cpu().numpy(), indptr, indices, Y, 1.5, 2.5, 0.1, X0.copy(), skip_empty=skip_empty)
    return out, ref, X0, pat


@pytest.mark.parametrize("F", [8, 20, 64, 128])
def test_solve_matches_restatement(ctx, F):
    indptr, indices = zipf_csr(700, 900, mean_log=3.0, sigma_log=1.0, dmin=1, dmax=400, seed=F)
    (x1, x2), ref, _, _ = solve_case(ctx, F, indptr, indices, 900, seed=F)
    assert np.abs(x1 - ref).max() <= 1e-12 * np.abs(ref).max()
    assert x1.tobytes() == x2.tobytes()


@pytest.mark.parametrize("F", [8, 128])
def test_solve_long_row_split_path(ctx, F):
    """Row 1 holds 100 000 + 17 entries: summed in 13 pieces of 8192 and combined in piece order."""
    rs = np.random.RandomState(5)
    I = 120000
    rows = [np.sort(rs.choice(I, 30, replace=False)), np.sort(rs.choice(I, 100017, replace=False))]
    rows += [np.sort(rs.choice(I, rs.randint(1, 50), replace=False)) for _ in range(300)]
    indptr = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    (x1, x2), ref, _, pat = solve_case(ctx, F, indptr, indices, I, seed=F)
    assert pat.n_long == 1 and pat.n_pieces == 13
    assert np.abs(x1 - ref).max() <= 1e-12 * np.abs(ref).max()
    assert x1.tobytes() == x2.tobytes()


@pytest.mark.parametrize("F", [10, 40, 100])
def test_empty_rows_skipped_or_zero(ctx, F):
    indptr, indices = zipf_csr(200, 300, mean_log=2.5, sigma_log=0.8, dmin=1, dmax=80, seed=2)
    lens = np.diff(indptr)
    lens[::7] = 0                                        # every 7th row empty
    keep = np.concatenate([np.arange(indptr[r], indptr[r] + lens[r]) for r in range(200)]).astype(np.int64)
    indices = indices[keep]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    (xs, _), ref_s, X0, _ = solve_case(ctx, F, indptr, indices, 300, seed=3, skip_empty=True)
    (xz, _), ref_z, _, _ = solve_case(ctx, F, indptr, indices, 300, seed=3, skip_empty=False)
    empty = lens == 0
    assert np.array_equal(xs[empty], X0[empty])
    assert np.all(xz[empty] == 0.0)
    assert np.abs(xs - ref_s).max() <= 1e-12 * np.abs(ref_s).max()
    assert np.abs(xz - ref_z).max() <= 1e-12 * np.abs(ref_z).max()


def test_non_positive_pivot_raises(ctx):
    indptr = np.array([0, 2, 3], np.int64)
    indices = np.array([0, 1, 1], np.int32)
    Y = torch.zeros((2, 8), dtype=torch.float64, device=ctx.device)
    G = ops.als_gram(ctx, Y)
    X = torch.ones((2, 8), dtype=torch.float64, device=ctx.device)
    pat = ops.AlsCSR(indptr, indices, 2, ctx.device)
    with pytest.raises(np.linalg.LinAlgError, match="row 0"):
        ops.als_solve(ctx, pat, Y, G, 1.0, 2.0, 0.0, X)


def test_refuses_too_many_factors(ctx):
    Y = torch.zeros((4, 129), dtype=torch.float64, device=ctx.device)
    with pytest.raises(ops._lib.ElliotHipError, match="factors=129"):
        ops.als_gram(ctx, Y)


IALS = {"lin_a1": "ials", "lin_a40": "ials", "log_a2_e05": "ials", "lin_a1_f20": "ials", "a1": "wrmf", "a0": "wrmf", "a1_f20": "wrmf"}


@pytest.mark.parametrize("tag", list(IALS))
def test_three_iterations_match_reference(ctx, golden, tag):
    model = IALS[tag]
    z = golden(f"als_{model}_ref.npz")
    U, I = (int(x) for x in z["shape"])
    p = z[f"{tag}_params"]
    F = int(p[0])
    if model == "ials":
        _, w_A, w_b = ials_weights(p[1], p[2], "linear" if p[4] == 0 else "log")
        reg = p[3]
    else:
        _, w_A, w_b = wrmf_weights(int(p[1]))
        reg = p[2]
    X, Y = als_ref.init_tables(int(z["seed"]), U, I, F)
    st = ops.AlsDeviceState(ctx, X, Y, z["R_indptr"], z["R_indices"], w_A, w_b, reg, gram="fresh" if model == "ials" else "stale")
    for it in range(1, 4):
        st.step()
        if f"{tag}_X_it{it}" in z.files:
            for name, t in (("X", st.X), ("Y", st.Y)):
                ref = z[f"{tag}_{name}_it{it}"]
                got = t.cpu().numpy()
                assert np.abs(got - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-300), (tag, name, it)
    excl = ops.DeviceCSR(z["R_indptr"], z["R_indices"], I, ctx.device)
    k = int(z["k"])
    idx, val = st.recommend(("excl", excl), k, 0, U)
    idx = idx.cpu().numpy()
    _, _, S = als_ref.topk(st.X.cpu().numpy(), st.Y.cpu().numpy(), (z["R_indptr"], z["R_indices"]), k)
    fragile = als_ref.fragile_users(S, (z["R_indptr"], z["R_indices"]), k)
    ref_idx = z[f"{tag}_rec_idx"]
    bad = [u for u in range(U) if not fragile[u] and not np.array_equal(idx[u], ref_idx[u])]
    assert not bad, (tag, bad[:5])
