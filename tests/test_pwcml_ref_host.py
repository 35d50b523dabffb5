"""CPU: tests/helpers/pwcml_ref.py (what tests/test_gpu_pointwise_edges.py and tests/test_gpu_cml_edges.py hold the kernels to) against the
originals in oracle/, the layouts against their docstrings, every exact case against its 2^24 budget and every bounded case against an fp32
NumPy emulation: a bound that plain fp32 cannot meet against fp64, or that a dropped sample fits under, would say nothing about the kernels."""
import numpy as np
import pytest

from oracle import cml as oc
from oracle import pointwise_mf as pw
from tests.helpers import pwcml_ref as R

f32, f64 = np.float32, np.float64


def test_restated_pick_lpt_gives_the_lane_classes():
    for (F, vw), want in R.LPT_TABLE.items():
        assert R.pick_lpt(F, vw) == want, (F, vw)
        assert R.lanes(F)[0] == vw
    assert {R.lanes(F)[2] for F in R.PW_CLASS_F} == {1, 2, 4} and {R.lanes(F)[2] for F in R.CML_FORWARD_F} == {1, 2, 4}
    assert all(R.lanes(F)[1] is None for F in R.PW_REFUSED_F)
    assert R.lanes(8)[1:] == R.lanes(7)[1:] == (8, 1)


@pytest.mark.parametrize("kind,bias,alpha,l_w", [("mse", False, 0.0, 0.0), ("mse", True, 0.0, 0.0), ("mse_sigmoid", False, 0.0, 0.0),
                                                 ("logistic", True, 0.5, 0.03)])
def test_pointwise_reference_equals_the_oracle_in_fp64(kind, bias, alpha, l_w):
    rs = np.random.RandomState(5)
    U, I, F, n = 40, 30, 9, 500
    w = {"Gu": rs.normal(size=(U, F)) * 0.4, "Gi": rs.normal(size=(I, F)) * 0.4}
    if bias:
        w["Bu"], w["Bi"] = rs.normal(size=U) * 0.1, rs.normal(size=I) * 0.1
    u, i, y = rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n).astype(f64)
    want_loss, want = pw.loss_and_grads(w, kind, u, i, y, alpha, l_w, dtype=f64)
    loss, g = R.pw_ref(w, kind, u, i, y, alpha=alpha, l_w=l_w)
    assert abs(loss - want_loss) <= 1e-13 * abs(want_loss)
    for k in want:
        assert np.abs(g[k] - want[k]).max() <= 1e-13 * np.abs(want[k]).max(), k
    # n_global: the mean-squared kinds scale by n / n_global, the logistic sum does not; side: the other accumulators stay zero
    loss2, g2 = R.pw_ref(w, kind, u, i, y, n_global=4 * n, side="items", alpha=alpha, l_w=l_w)
    s = 1.0 if kind == "logistic" else 0.25
    assert abs(loss2 - s * want_loss) <= 1e-13 * abs(want_loss) and not g2["Gu"].any()
    assert np.abs(g2["Gi"] - s * want["Gi"]).max() <= 1e-13 * np.abs(want["Gi"]).max()
    # the mutations are what they say: the batch without the sample / with it twice, the mean still over n_global
    keep = np.arange(n) != 7
    _, g3 = R.pw_ref(w, kind, u, i, y, n_global=n, alpha=alpha, l_w=l_w, skip=7)
    _, g4 = R.pw_ref(w, kind, u[keep], i[keep], y[keep], n_global=n, alpha=alpha, l_w=l_w)
    _, g5 = R.pw_ref(w, kind, u, i, y, n_global=n, alpha=alpha, l_w=l_w, twice=7)
    for k in g3:
        assert np.abs(g3[k] - g4[k]).max() <= 1e-13 and np.abs((g5[k] - g[k]) - (g[k] - g3[k])).max() <= 1e-13, k
    _, g6 = R.pw_ref(w, kind, u, i, y, n_global=n, alpha=alpha, l_w=l_w, move=(7, (u[7] + 1) % U))
    assert np.abs(g6["Gu"][u[7]] - g3["Gu"][u[7]]).max() <= 1e-13 and np.abs(g6["Gi"] - g["Gi"]).max() <= 1e-13


def test_cml_reference_equals_the_oracle_in_fp64():
    rs = np.random.RandomState(8)
    U, I, F, B, l_w, l_b, margin = 30, 25, 6, 200, 0.01, 0.02, 0.5
    Gu, Gi, Bi = rs.normal(size=(U, F)) * 2.5, rs.normal(size=(I, F)) * 2.5, rs.normal(size=I)      # some pairs below the -80 clip
    u, i, j = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B)
    want_loss, wGu, wGi, wBi = oc.loss_and_grads(Gu, Gi, Bi, u, i, j, l_w, l_b, margin, dtype=f64)
    D, E, reg = R.cml_forward_ref(Gu, Gi, Bi, u, i, j, l_w, l_b)
    hinge, dGu, dGi, dBi, (n_a, m_b, low_a) = R.cml_grads_ref(Gu, Gi, Bi, u, i, j, D, E, D, E, l_w, l_b, margin)
    assert low_a.sum() > 0 and 0 < n_a.sum() < B * B
    assert abs(reg + hinge - want_loss) <= 1e-12 * want_loss and abs(hinge - R.cml_hinge_full(D, E, margin)) <= 1e-12 * hinge
    for got, want in ((dGu, wGu), (dGi, wGi), (dBi, wBi)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("B,B_all,lo,kind", [(300, None, 0, "ties"), (300, 700, 250, "ties"), (1, None, 0, "ties"), (3, 8, 2, "ties"),
                                             (64, None, 0, "clipped"), (64, None, 0, "inactive")])
def test_brute_force_counts_equal_the_sorted_searches_on_planted_ties(B, B_all, lo, kind):
    D, E, D_all, E_all = R.cml_de(11, B, B_all, lo, kind)
    n_a, m_b, low_a = R.cml_counts(D, E, D_all, E_all, R.CML_MARGIN)
    cD, cE, hinge = oc.coefficients(D, E, D_all, E_all, R.CML_MARGIN)
    assert np.array_equal(-cD, n_a) and np.array_equal(-cE, m_b)
    assert hinge == R.cml_hinge_share(D, E, D_all, E_all, R.CML_MARGIN)
    if B_all is None:
        assert hinge == R.cml_hinge_full(D, E, R.CML_MARGIN)
    if kind == "ties":                                              # every planted sum is there, on the grid
        s = D_all[:, None] + E_all[None, :]
        for v in (0.5, 0.375, 0.625, -80.0, -80.125, -79.875)[:max(1, min(6, len(D_all)))]:
            assert (s == v).any(), v
        if B >= 300:
            assert (np.bincount(((E_all + 2000) * 8).astype(int)).max() >= 30) and (D_all == 3.0).sum() >= 30     # the runs
    elif kind == "clipped":
        assert not n_a.any() and not m_b.any() and hinge == B * len(D_all) * (R.CML_MARGIN + 80.0)
    else:
        assert not n_a.any() and not m_b.any() and hinge == 0.0


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.LAYOUTS)
def test_layouts_are_what_their_docstrings_say(name):
    L = 8
    pu, pi = R.layout_plans(name, L)
    u, i = R.make_batch(np.random.RandomState(1), pu, pi)
    assert len(u) == pu.pos == pi.pos
    for ids, p in ((u, pu), (i, pi)):
        conts = R.assert_layout(ids, p)
        rows, start, end, _ = R.layout_of(ids, p.c)
        c, nm = p.c, p.names
        at = lambda k: (int(start[nm[k]]), int(end[nm[k]]), int(conts[nm[k]]))
        if name == "small":
            assert at("first_cut") == (0, c + 1, 1)
            s, e, k = at("ends_on_border")
            assert e % c == 0 and k == 0 and at("starts_on_border") == (e, e + 2, 0)
            s, e, k = at("two_positions")
            assert (s % c, e - s, k) == (c - 1, 2, 1)
            s, e, k = at("three_chunks")
            assert (s % c, e - s, k) == (0, 3 * c, 2)
            (s1, e1, k1), (s2, e2, k2) = at("adjacent_a"), at("adjacent_b")
            assert e1 == s2 and s1 // c + 1 == s2 // c == e1 // c and k1 == k2 == 1          # tail of a and head of b in one chunk
            assert [at("conts_%d" % k)[2] for k in (L - 2, L - 1, L, L + 1)] == [L - 2, L - 1, L, L + 1]
            assert (conts >= L).sum() >= 4 and at("long_b")[1] % c == 0
        if name.startswith("long") and p is pi:
            k = {"long_a": 255, "long_b": 256, "long_c": 257, "long_d": 513}[name]
            assert at("conts_%d" % k)[2] == k == conts.max()
        if name == "long_a" and p is pu:
            assert sorted(conts[conts > 200].tolist()) == [255, 256, 257, 513]
        if "last_cut" in nm:
            s, e, k = at("last_cut")
            assert e == len(ids) and len(ids) % c != 0 and s % c == c - 1 and k == 1
        else:
            assert len(ids) < c
    # a batch that is not the plan's is refused
    if len(u) > 3:
        bad = u.copy()
        bad[0] = (u[0] + 1) % len(pu.counts)                       # one sample credited to the neighbouring row
        with pytest.raises(AssertionError):
            R.assert_layout(bad, pu)


# ---- exact cases --------------------------------------------------------------------------------------------------------------------------
def _pw_exact_ids():
    out = [(name, F, b) for name in R.LAYOUTS for F in R.PW_LAYOUT_F for b in (False, True) if not (name.startswith("long") and F != 8)]
    return out + [("class", F, True) for F in R.PW_CLASS_F]


def test_every_exact_pointwise_case_is_inside_the_budget():
    for layout, F, bias in _pw_exact_ids():
        c = R.pw_exact_case(layout, F, bias)                       # (asserts layout and budget)
        assert 0 < c.budget < R.BUDGET and c.n_global >= len(c.y)
    # the budget check does refuse: a hot row long enough, or an input off the grid
    c = R.pw_exact_case("small", 8, True)
    w = dict(c.w, Gu=c.w["Gu"] * 4096)
    with pytest.raises(AssertionError):
        R.pw_budget(w, c.u, c.i, c.y, c.n_global)
    with pytest.raises(AssertionError):
        R.pw_budget(dict(c.w, Gi=c.w["Gi"] + 0.1), c.u, c.i, c.y, c.n_global)
    with pytest.raises(AssertionError):
        R.pw_budget(c.w, c.u, c.i, c.y, len(c.y))


@pytest.mark.parametrize("layout,F,bias", [("small", 8, True), ("small", 7, False), ("class", 4, True), ("class", 1, True)])
def test_fp32_emulation_of_an_exact_pointwise_case_has_the_fp64_bits_in_both_orders(layout, F, bias):
    c = R.pw_exact_case(layout, F, bias)
    for side in ("both", "items"):
        want_loss, want = R.pw_ref(c.w, "mse", c.u, c.i, c.y, c.n_global, side=side)
        for reverse in (False, True):
            loss, g = R.pw_emulate_f32(c.w, "mse", c.u, c.i, c.y, c.n_global, side=side, reverse=reverse)
            assert loss == want_loss
            for k in want:
                assert np.array_equal(g[k].astype(f64), want[k]), (k, side, reverse)


def test_every_exact_cml_case_is_inside_the_budget_and_fp32_has_the_fp64_bits():
    for F in R.CML_FORWARD_F:
        assert 0 < R.cml_forward_case(F).budget < R.BUDGET
    for case in R.CML_GRADS_CASES:
        c = R.cml_grads_case(*case)
        assert 0 < c.budget < R.BUDGET
        n_a, m_b, low_a = c.counts
        cD, cE, hinge = oc.coefficients(c.D, c.E, c.D_all, c.E_all, R.CML_MARGIN)
        assert np.array_equal(-cD, n_a) and np.array_equal(-cE, m_b) and hinge == c.hinge
    c = R.cml_grads_case(8, 300)
    for sl in (slice(None), slice(None, None, -1)):
        g = oc.row_gradients(c.Gu, c.Gi, c.Bi, c.u[sl], c.i[sl], c.j[sl], -c.counts[0][sl].astype(f64), -c.counts[1][sl].astype(f64), R.CML_L_W, 0.0,
                             dtype=f32)
        for got, want in zip(g, (c.dGu, c.dGi, c.dBi)):
            assert got.dtype == f32 and np.array_equal(got.astype(f64), want)
    f = R.cml_forward_case(4)
    D32, E32 = oc.distances(f.Gu, f.Gi, f.Bi, f.u, f.i, f.j, dtype=f32)
    D, E, _ = R.cml_forward_ref(f.Gu, f.Gi, f.Bi, f.u, f.i, f.j, R.CML_L_W, 0.0)
    assert np.array_equal(D32.astype(f64), D) and np.array_equal(E32.astype(f64), E)
    with pytest.raises(AssertionError):                            # counts too large for the grid: refused
        R.cml_budget(c.Gu * 1024, c.Gi * 1024, c.Bi, c.u, c.i, c.j, c.D, c.E, c.D_all, c.E_all - 1000.0, R.CML_L_W, R.CML_MARGIN)


# ---- bounded cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(R.PW_BOUNDED_KINDS))
@pytest.mark.parametrize("layout,F", R.pw_bounded_cases())
def test_bounded_cases_hold_fp32_in_both_orders_and_hide_no_sample(layout, F, model):
    c = R.pw_bounded_case(layout, F, model)
    for side in c.sides:
        want_loss, want = R.pw_ref(c.w, c.kind, c.u, c.i, c.y, c.n_global, side=side, alpha=c.alpha, l_w=c.l_w)
        loss_bound, bound = R.pw_bound(c.w, c.kind, c.u, c.i, c.y, c.n_global, side=side, alpha=c.alpha, l_w=c.l_w)
        for reverse in (False, True):
            loss, g = R.pw_emulate_f32(c.w, c.kind, c.u, c.i, c.y, c.n_global, side=side, alpha=c.alpha, l_w=c.l_w, reverse=reverse)
            assert abs(loss - want_loss) <= loss_bound
            for k in want:
                assert R.bound_ratio(g[k], want[k], bound[k]) <= 1.0, (k, side, reverse)
        # a bound is no licence: it stays below a hundredth of the typical entry it guards ...
        for k in ("Gu", "Gi"):
            big = np.abs(want[k]) > 0
            assert not big.any() or np.median(bound[k][big] / np.abs(want[k][big])) < 1e-2
        # ... and no covered row can lose, double or hand over a sample unseen
        hidden = R.pw_hidden_rows(c.w, c.kind, c.u, c.i, c.y, c.n_global, side, c.alpha, c.l_w, bound)
        assert all(len(v) == 0 for v in hidden.values()), hidden
        covered = {"Gu": np.bincount(c.u), "Gi": np.bincount(c.i)}
        assert all(((covered[k] > 0) & (covered[k] <= R.COVERED_LEN)).sum() >= 5 for k in hidden)
        # the same said with the references themselves, on one cut row per side
        pu, pi = c.plans
        for tab, plan, ids in (("Gu", pu, c.u), ("Gi", pi, c.i)):
            if tab not in hidden:
                continue
            row = next(plan.names[k] for k in ("two_positions", "short_cut", "last_cut") if k in plan.names)
            b = int(np.nonzero(ids == row)[0][0])
            muts = [dict(skip=b), dict(twice=b)] + ([dict(move=(b, row - 1))] if tab == "Gu" else [])
            for mut in muts:
                _, gm = R.pw_ref(c.w, c.kind, c.u, c.i, c.y, c.n_global, side=side, alpha=c.alpha, l_w=c.l_w, **mut)
                assert (np.abs(gm[tab][row] - want[tab][row]) > 2 * bound[tab][row]).any(), (tab, mut)


def test_cml_bounds_hold_fp32():
    rs = np.random.RandomState(3)
    for F in (1, 63, 64, 65, 200, 1024):
        Gu, Gi, Bi = rs.normal(size=(6, F)).astype(f32), rs.normal(size=(9, F)).astype(f32), rs.normal(size=9).astype(f32)
        s = np.zeros(9, f32)
        for f in range(F):
            s = s + Gi[:, f] * Gi[:, f]
        ref = Bi.astype(f64) - np.sum(Gi.astype(f64) ** 2, -1)
        assert (np.abs((Bi - s).astype(f64) - ref) <= R.item_side_bound(Gi.astype(f64), Bi.astype(f64))).all()
        d = Gu[:, None, :] - Gi[None, :, :]
        acc = np.zeros((6, 9), f32)
        for f in range(F):
            acc = acc + d[:, :, f] * d[:, :, f]
        d64 = Gu.astype(f64)[:, None, :] - Gi.astype(f64)[None, :, :]
        ref = Bi.astype(f64)[None, :] - np.sum(d64 * d64, -1)
        bnd = R.rescore_bound(Gu.astype(f64)[:, None, :], Gi.astype(f64)[None, :, :], Bi.astype(f64)[None, :], F)
        assert (np.abs((Bi[None, :] - acc).astype(f64) - ref) <= bnd).all() and (bnd < 1e-3 * (1 + np.abs(ref))).all()
    f = R.cml_forward_case(36)
    l_b = 0.02
    per = (f32(0.5) * f32(R.CML_L_W) * np.sum(f.Gu[f.u] ** 2 + f.Gi[f.i] ** 2 + f.Gi[f.j] ** 2, -1).astype(f32) + f32(0.5) * f32(l_b) * f.Bi[f.i].astype(f32) ** 2
           + (f32(0.5) * f32(l_b) * f.Bi[f.j].astype(f32) ** 2) / f32(10))
    assert per.dtype == f32
    _, _, reg = R.cml_forward_ref(f.Gu, f.Gi, f.Bi, f.u, f.i, f.j, R.CML_L_W, float(f32(l_b)))
    assert abs(float(per.astype(f64).sum()) - reg) <= R.cml_reg_bound(f.Gu, f.Gi, f.Bi, f.u, f.i, f.j, R.CML_L_W, l_b) < 1e-5 * reg
