"""The rank kernels (csrc/el_rank.hip) at their edges: el_dense_rank / el_dense_rank_f64 against the host restatement
(evaluation/ranks.positions, a stable sort), all four entry points against the lists the selection kernels produce at k = I, the
fused MFMA route against the wave route byte for byte, repeatability, el_rank_metrics against ranks.finish and the golden cases
of the reference's own Evaluator through Evaluator.eval_device, and the argument checks.

Positions are integers: every comparison of positions is exact.  The metric sums are fp64 sums of at most a few hundred
non-negative terms taken in two orders, bound 1e-11 max(1, |ref|) (rank_ref.TOL); their integer slots are exact."""
import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from elliot_amd.evaluation import ranks
from elliot_amd.evaluation.evaluator import Evaluator
from tests.gpu_util import cpu
from tests.helpers import rank_ref

pytestmark = pytest.mark.gpu

U0 = 3                                        # u_start of every case: rows of every CSR are absolute user ids
KINDS = ["equal", "distinct", "ties", "zeros"]
PATTERNS = ["ends", "none", "all", "odd", "rand"]
Z = rank_ref.load()
CASES = [str(t) for t in Z["cases"]]


def content(kind, I, rs):
    j = np.arange(I, dtype=np.float64)
    if kind == "equal":
        return np.full(I, 1.25)
    if kind == "distinct":
        return rs.permutation(I) * 0.5 - I / 4.0
    if kind == "ties":
        return np.round(rs.normal(size=I) * 4.0) / 2.0
    v = np.where(j % 2 == 0, -0.0, 0.0)
    v[3::7] = 1.0
    v[5::11] = -1.0
    return v


def mask_rows(n, I, kind, rs):
    """U0 + n ascending rows (the first U0 belong to other users): empty, full and random ones."""
    rows = [np.sort(rs.choice(I, rs.randint(0, I + 1), replace=False)) for _ in range(U0)]
    for u in range(n):
        if u % 7 == 0:
            rows.append(np.zeros(0, np.int64))
        elif u % 7 == 1:
            rows.append(np.arange(I))
        else:
            rows.append(np.flatnonzero(rs.rand(I) < (0.3 if kind == "excl" else 0.6)))
    return rows


def target_row(pattern, s, adm, I, rs):
    ok = np.flatnonzero(adm)
    if pattern == "none":
        return np.zeros(0, np.int64)
    if pattern == "all":
        return ok
    if pattern == "ends":
        t = [0, I - 1]
        if ok.shape[0]:
            order = ok[np.argsort(-(s[ok] + 0.0), kind="stable")]
            t += [order[0], order[-1]]
        return np.unique(t)
    if pattern == "odd":                      # ids the model has no row for, a masked item, a few others
        t = [I, I + 3]
        bad = np.flatnonzero(~adm)
        if bad.shape[0]:
            t.append(bad[rs.randint(bad.shape[0])])
        return np.unique(np.concatenate([t, rs.choice(I, min(3, I), replace=False)]))
    return np.unique(rs.choice(I, rs.randint(1, min(I, 40) + 1), replace=False))


def dense_case(I, mask, dtype, seed):
    """20 users (every content x every target pattern) behind U0 foreign rows: scores, mask rows, target rows, admissible."""
    rs = np.random.RandomState(seed)
    n = len(KINDS) * len(PATTERNS)
    S = np.stack([content(KINDS[u % len(KINDS)], I, rs) for u in range(n)]).astype(dtype)
    mrows = mask_rows(n, I, mask, rs) if mask else None
    adm = np.ones((n, I), dtype=bool)
    if mask:
        mp, mi = rank_ref.csr_of(mrows)
        adm = rank_ref.mask_of(mp[U0:], mi, n, I, mask)
    trows = [np.array([0], np.int64)] * U0 + [target_row(PATTERNS[u // len(KINDS)], S[u], adm[u], I, rs) for u in range(n)]
    return S, mrows, trows, adm


def device_case(ctx, S, mrows, trows, mask, I):
    preds = torch.from_numpy(S).to(ctx.device)
    csr = ops.DeviceCSR(*rank_ref.csr_of(mrows), I, ctx.device) if mask else None
    tp, ti = rank_ref.csr_of(trows)
    targets = ops.DeviceTestSet(tp, ti, None, ctx.device)
    return preds, {"excl": csr if mask == "excl" else None, "cand": csr if mask == "cand" else None}, targets, (tp, ti)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask", [None, "excl", "cand"])
@pytest.mark.parametrize("I", [1, 63, 64, 65, 129, 1025])
def test_dense_rank_equals_the_stable_sort(ctx, I, mask, dtype):
    S, mrows, trows, adm = dense_case(I, mask, dtype, 100 + I)
    preds, mk, targets, (tp, ti) = device_case(ctx, S, mrows, trows, mask, I)
    n = S.shape[0]
    fn = ops.dense_rank if dtype == np.float32 else ops.dense_rank_f64
    got = cpu(fn(ctx, preds, U0, U0 + n, targets, **mk))
    exp = ranks.positions(S, adm if mask else None, (tp[U0:], ti))
    assert got.dtype == np.int32 and got.shape == exp.shape
    bad = np.flatnonzero(got != exp)
    assert bad.shape[0] == 0, (I, mask, bad[:8], got[bad[:8]], exp[bad[:8]])
    assert (exp == -1).any() and (exp == 0).any()                      # ids >= I or masked targets; a best item


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_around_the_slice_capacity(ctx, dtype):
    """Rows of RANK_WAVE_CAP - 1, RANK_WAVE_CAP, RANK_WAVE_CAP + 1 and more than two slices of targets: one, one, two and three
    passes over the catalogue."""
    I, C = 1025, ops.RANK_WAVE_CAP
    rs = np.random.RandomState(7)
    lens = [C - 1, C, C + 1, 2 * C + 76]
    S = np.stack([content("ties", I, rs) for _ in lens]).astype(dtype)
    mrows = [np.zeros(0, np.int64)] * U0 + [np.flatnonzero(rs.rand(I) < 0.2) for _ in lens]
    trows = [np.array([1], np.int64)] * U0 + [np.sort(rs.choice(I + 300, L, replace=False)) for L in lens]
    preds, mk, targets, (tp, ti) = device_case(ctx, S, mrows, trows, "excl", I)
    mp, mi = rank_ref.csr_of(mrows)
    fn = ops.dense_rank if dtype == np.float32 else ops.dense_rank_f64
    got = cpu(fn(ctx, preds, U0, U0 + len(lens), targets, **mk))
    exp = ranks.positions(S, rank_ref.mask_of(mp[U0:], mi, len(lens), I, "excl"), (tp[U0:], ti))
    assert np.array_equal(got, exp)
    assert (exp >= 0).sum() > 2 * C


# ---- agreement with the selection kernels -------------------------------------------------------------------------------------
def quantised_tables(n, I, F, rs, dtype):
    """Half of the users and items on a grid of quarters (sums exact in fp32: exact ties), half normal."""
    Gu = (rs.randint(-2, 3, size=(U0 + n, F)) * 0.5).astype(dtype)
    Gi = (rs.randint(-2, 3, size=(I, F)) * 0.5).astype(dtype)
    Gu[U0 + n // 2:] = rs.normal(size=(n - n // 2, F)).astype(dtype)
    Gi[I // 2:] = rs.normal(size=(I - I // 2, F)).astype(dtype)
    Bi = (rs.randint(-1, 2, size=I) * 0.25).astype(dtype)
    return Gu, Gi, Bi


def assert_positions_index_the_lists(pos, idx, tp, ti, adm, I, what):
    """pos[e] is where the list holds target e; -1 exactly for ids >= I and masked targets."""
    n = idx.shape[0]
    for u in range(n):
        for e in range(tp[U0 + u], tp[U0 + u + 1]):
            t, q = int(ti[e]), int(pos[e - tp[U0]])
            if t >= I or not adm[u, t]:
                assert q == -1, (what, u, t, q)
            else:
                assert 0 <= q < I and int(idx[u, q]) == t, (what, u, t, q, idx[u, max(q - 2, 0):q + 3])


@pytest.mark.parametrize("mask", ["excl", "cand"])
@pytest.mark.parametrize("F", [1, 5, 64, 200])
def test_positions_index_the_lists_of_the_selection_kernels(ctx, F, mask):
    I, n = 513, 10
    rs = np.random.RandomState(50 + F)
    mrows = mask_rows(n, I, mask, rs)
    mp, mi = rank_ref.csr_of(mrows)
    adm = rank_ref.mask_of(mp[U0:], mi, n, I, mask)
    csr = ops.DeviceCSR(mp, mi, I, ctx.device)
    mk = {"excl": csr if mask == "excl" else None, "cand": csr if mask == "cand" else None}
    trows = [np.array([2], np.int64)] * U0 + [np.arange(I + 2) if u == 2 else np.unique(rs.choice(I + 5, 30)) for u in range(n)]
    tp, ti = rank_ref.csr_of(trows)
    targets = ops.DeviceTestSet(tp, ti, None, ctx.device)
    dev = lambda a: torch.from_numpy(a).to(ctx.device)
    # fp32 tables (wave route) and fp64 tables
    Gu, Gi, Bi = quantised_tables(n, I, F, rs, np.float32)
    pos = cpu(ops.score_rank(ctx, dev(Gu), dev(Gi), dev(Bi), U0, U0 + n, targets, algo="simple", **mk))
    idx, val = ops.score_topk(ctx, dev(Gu), dev(Gi), dev(Bi), U0, U0 + n, I, algo="simple", **mk)
    assert_positions_index_the_lists(pos, cpu(idx), tp, ti, adm, I, "el_score_topk")
    P, Q, b = quantised_tables(n, I, F, rs, np.float64)
    pos64 = cpu(ops.score_rank_f64(ctx, dev(P), dev(Q), dev(b), U0, U0 + n, targets, **mk))
    idx64, _ = ops.score_topk_f64(ctx, dev(P), dev(Q), dev(b), U0, U0 + n, I, **mk)
    assert_positions_index_the_lists(pos64, cpu(idx64), tp, ti, adm, I, "el_score_topk_f64")
    if F == 1:                                     # the dense pair once: the scores above as materialised blocks
        S32 = np.stack([content(KINDS[u % 4], I, rs) for u in range(n)]).astype(np.float32)
        posd = cpu(ops.dense_rank(ctx, dev(S32), U0, U0 + n, targets, **mk))
        idxd, _ = ops.dense_topk(ctx, dev(S32), U0, U0 + n, I, **mk)
        assert_positions_index_the_lists(posd, cpu(idxd), tp, ti, adm, I, "el_dense_topk")
        S64 = S32.astype(np.float64) + np.where(np.arange(I) % 3 == 0, 2.0 ** -40, 0.0)      # distinct only in fp64
        posd = cpu(ops.dense_rank_f64(ctx, dev(S64), U0, U0 + n, targets, **mk))
        idxd, _ = ops.dense_topk_f64(ctx, dev(S64), U0, U0 + n, I, **mk)
        assert_positions_index_the_lists(posd, cpu(idxd), tp, ti, adm, I, "el_dense_topk_f64")


# ---- the fused route ------------------------------------------------------------------------------------------------------------
def mfma_case(ctx, n, I, F, seed, with_excl=True):
    rs = np.random.RandomState(seed)
    Gu, Gi, Bi = quantised_tables(n, I, F, rs, np.float32)
    C = ops.RANK_MFMA_CAP
    erows = [np.flatnonzero(rs.rand(I) < 0.5) for _ in range(U0)]
    trows = [np.array([0], np.int64)] * U0
    for u in range(n):
        L = {5: C, 6: C + 1, 7: min(100, I), 40: C - 1}.get(u, rs.randint(0, 21))
        trows.append(np.sort(rs.choice(I + 4, L, replace=False)))
        erows.append(np.zeros(0, np.int64) if u % 5 == 3 else (np.arange(3, I) if u % 11 == 9 else np.flatnonzero(rs.rand(I) < 0.25)))
    tp, ti = rank_ref.csr_of(trows)
    dev = lambda a: torch.from_numpy(a).to(ctx.device)
    excl = ops.DeviceCSR(*rank_ref.csr_of(erows), I, ctx.device) if with_excl else None
    return dev(Gu), dev(Gi), dev(Bi), ops.DeviceTestSet(tp, ti, None, ctx.device), excl


# (30: a row width the float4 staging cannot take, once)
MFMA_SHAPES = [(F, I, n) for F in (32, 64, 128, 256) for I in (127, 128, 129, 513) for n in (129, 300)] + [(30, 129, 129)]


@pytest.mark.parametrize("F,I,n", MFMA_SHAPES)
def test_mfma_route_equals_the_wave_route(ctx, F, I, n):
    Gu, Gi, Bi, targets, excl = mfma_case(ctx, n, I, F, 1000 * F + I + n)
    ctx.timing(True)
    try:
        a = ops.score_rank(ctx, Gu, Gi, Bi, U0, U0 + n, targets, excl=excl, algo="mfma")
        kernels = set(ctx.timing_report())
    finally:
        ctx.timing(False)
    assert {"k_score_rank_mfma", "k_rank_wave"} <= kernels
    b = ops.score_rank(ctx, Gu, Gi, Bi, U0, U0 + n, targets, excl=excl, algo="simple")
    a, b = cpu(a), cpu(b)
    assert a.tobytes() == b.tobytes(), (F, I, n, np.flatnonzero(a != b)[:8])
    assert (a >= 0).sum() > n and (a == -1).any()
    if (F, I) == (64, 513):                       # no mask at all, and the bias left out
        a = ops.score_rank(ctx, Gu, Gi, None, U0, U0 + n, targets, algo="mfma")
        b = ops.score_rank(ctx, Gu, Gi, None, U0, U0 + n, targets, algo="simple")
        assert cpu(a).tobytes() == cpu(b).tobytes()


def test_auto_takes_a_listed_route_and_the_mfma_route_refuses_what_it_cannot_do(ctx):
    Gu, Gi, Bi, targets, excl = mfma_case(ctx, 129, 129, 64, 3)
    auto = cpu(ops.score_rank(ctx, Gu, Gi, Bi, U0, U0 + 129, targets, excl=excl))
    assert np.array_equal(auto, cpu(ops.score_rank(ctx, Gu, Gi, Bi, U0, U0 + 129, targets, excl=excl, algo="simple")))
    with pytest.raises(_lib.ElliotHipError, match="MFMA route needs"):
        ops.score_rank(ctx, Gu, Gi, Bi, U0, U0 + 129, targets, cand=excl, algo="mfma")


def test_two_runs_give_the_same_bytes(ctx):
    Gu, Gi, Bi, targets, excl = mfma_case(ctx, 300, 513, 64, 9)
    for algo in ("mfma", "simple"):
        a = cpu(ops.score_rank(ctx, Gu, Gi, Bi, U0, U0 + 300, targets, excl=excl, algo=algo)).tobytes()
        assert a == cpu(ops.score_rank(ctx, Gu, Gi, Bi, U0, U0 + 300, targets, excl=excl, algo=algo)).tobytes()


# ---- el_rank_metrics ------------------------------------------------------------------------------------------------------------
def golden_device(ctx, tag, name):
    tp, tc, tr = rank_ref.split_of(Z, tag, name)
    U, I = (int(v) for v in Z[f"{tag}_shape"])
    test = ops.DeviceTestSet(tp, tc, tr, ctx.device)
    train = ops.DeviceCSR(Z[f"{tag}_train_indptr"], Z[f"{tag}_train_indices"], I, ctx.device)
    return tp, tr, test, train, U, I


def assert_sums(got, ref, what):
    for slot in (1, 4, 5):
        assert got[slot] == ref[slot], (what, slot, got, ref)
    for slot in (0, 2, 3):
        err = abs(got[slot] - ref[slot])
        print(f"{what} slot {slot}: {got[slot]!r} vs {ref[slot]!r}, |diff| {err:.3g}")
        assert err <= rank_ref.TOL * max(1.0, abs(ref[slot])), (what, slot, got[slot], ref[slot])


@pytest.mark.parametrize("tag", CASES)
def test_rank_metrics_equal_the_host_sums(ctx, tag):
    tp, tr, test, train, U, I = golden_device(ctx, tag, "test")
    thr = float(Z[f"{tag}_threshold"])
    pos_h = Z[f"{tag}_test_pos"]
    pos = torch.from_numpy(pos_h).to(ctx.device)
    train_len = np.diff(Z[f"{tag}_train_indptr"])
    for c in Z[f"{tag}_cutoffs"].tolist():
        rows_h = ranks.user_rows(pos_h, tp, tr, thr, train_len, I, c)
        sums, rows = ops.rank_metrics(ctx, pos, test, thr, train, I, c, per_user=True)
        assert_sums(cpu(sums), rows_h.sum(axis=0), f"{tag}@{c}")
        # a row is two exact integers and IEEE divisions of them on either side
        assert np.array_equal(cpu(rows), rows_h[:, :4])
        # block after block into one accumulator, positions sliced as the kernels lay them out
        acc = torch.zeros(ops.RANK_SUMS, dtype=torch.float64, device=ctx.device)
        for s, e in ((0, 37), (37, 38), (38, U)):
            ops.rank_metrics(ctx, pos[int(tp[s]):int(tp[e])].contiguous(), test, thr, train, I, c, u_start=s, u_stop=e, sums=acc)
        assert_sums(cpu(acc), cpu(sums), f"{tag}@{c} blocks")


def test_rank_metrics_count_a_user_without_negatives(ctx):
    # 3 items; user 0: 2 in train, 2 relevant held out (one without a model row): neg = 0; user 1 is ordinary
    test = ops.DeviceTestSet(np.array([0, 2, 3]), np.array([0, 7, 1], np.int32), np.array([1, 1, 1], np.float32), ctx.device)
    train = ops.DeviceCSR(np.array([0, 2, 3]), np.array([1, 2, 0], np.int32), 3, ctx.device)
    pos = torch.tensor([0, -1, 1], dtype=torch.int32, device=ctx.device)
    got = cpu(ops.rank_metrics(ctx, pos, test, 0.0, train, 3, 5))
    ref = ranks.user_rows(np.array([0, -1, 1], np.int32), np.array([0, 2, 3]), np.ones(3, np.float32), 0.0, np.array([2, 1]), 3, 5).sum(axis=0)
    assert got.tolist() == ref.tolist() and got[5] == 1.0 and got[4] == 1.0


@pytest.mark.parametrize("tag", CASES)
def test_golden_cases_through_eval_device(ctx, tag):
    data = rank_ref.golden_case(Z, tag, ["nDCG", "AUC", "GAUC", "LAUC"])
    ev = Evaluator(data, None)
    U, I = data.num_users, data.num_items
    sets = ev.device_sets(data, ctx.device)
    from elliot_amd.recommender.masks import device_masks
    excl = device_masks(data, ctx).train
    S = torch.from_numpy(Z[f"{tag}_scores"]).to(ctx.device)

    def blocks():
        for s, e in ((0, 50), (50, U)):
            idx, _ = ops.dense_topk(ctx, S[s:e].contiguous(), s, e, 10, excl=excl)
            pv = ops.dense_rank(ctx, S[s:e].contiguous(), s, e, sets["val"], excl=excl) if sets["val"] is not None else None
            yield s, idx, idx, pv, ops.dense_rank(ctx, S[s:e].contiguous(), s, e, sets["test"], excl=excl)
    res = ev.eval_device(ctx, data, blocks())
    for r, c in enumerate(Z[f"{tag}_cutoffs"].tolist()):
        assert list(res[c]["test_results"]) == ["nDCG", "AUC", "GAUC", "LAUC"]
        rank_ref.check_values(res[c]["test_results"], Z[f"{tag}_values"][r], f"{tag}@{c}")
        if sets["val"] is not None:
            rank_ref.check_values(res[c]["val_results"], Z[f"{tag}_val_values"][r], f"{tag}/val@{c}")
    with pytest.raises(Exception, match="need the positions"):
        ev.eval_device(ctx, data, ((s, i, j) for s, i, j, _, _ in blocks()))


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_half_given_csrs_and_a_null_pos_are_refused_before_any_launch(ctx):
    I, n = 65, 4
    S = torch.zeros((n, I), dtype=torch.float32, device=ctx.device)
    G = torch.zeros((n, 8), dtype=torch.float32, device=ctx.device)
    Q = torch.zeros((I, 8), dtype=torch.float32, device=ctx.device)
    tp = torch.arange(n + 1, dtype=torch.int64, device=ctx.device)
    ti = torch.zeros(n, dtype=torch.int32, device=ctx.device)
    pos = torch.full((n,), 77, dtype=torch.int32, device=ctx.device)
    p = lambda t: t.data_ptr()
    lib, h, st = ctx.lib, ctx.handle, ctx.stream()
    calls = {
        "excl_indptr alone": lambda: lib.el_dense_rank(h, st, p(S), I, 0, n, I, p(tp), None, None, None, p(tp), p(ti), p(pos)),
        "excl_indices alone": lambda: lib.el_dense_rank(h, st, p(S), I, 0, n, I, None, p(ti), None, None, p(tp), p(ti), p(pos)),
        "cand_indptr alone": lambda: lib.el_score_rank(h, st, p(G), p(Q), None, 0, n, I, 8, None, None, p(tp), None, p(tp), p(ti), p(pos),
                                                       _lib.EL_TOPK_SIMPLE, None, 0),
        "target indices missing": lambda: lib.el_dense_rank(h, st, p(S), I, 0, n, I, None, None, None, None, p(tp), None, p(pos)),
        "null pos": lambda: lib.el_dense_rank(h, st, p(S), I, 0, n, I, None, None, None, None, p(tp), p(ti), None),
        "null pos, MFMA": lambda: lib.el_score_rank(h, st, p(G), p(Q), None, 0, n, I, 8, None, None, None, None, p(tp), p(ti), None,
                                                    _lib.EL_TOPK_MFMA, p(pos), 4096),
    }
    ctx.timing(True)
    try:
        for what, call in calls.items():
            assert call() == 2, what                                   # the library's argument error
            assert lib.el_last_error(), what
        assert not ctx.timing_report()                                 # nothing was launched
    finally:
        ctx.timing(False)
    torch.cuda.synchronize()
    assert (cpu(pos) == 77).all()
