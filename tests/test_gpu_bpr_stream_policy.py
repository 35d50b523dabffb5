"""The deferred BPR kernels load and store the rows they stream once (a user's theta gather, m and v; an item's m and v) with the
non-temporal hint, and the rows that are re-used (the theta they hand to the item side, Gi, the partial rows of cut segments) with the
default policy.  A hint can go wrong only in which bytes it touches and in the ordering between launches, so every instantiation on
that path is run at its row widths and compared bit for bit with the forms that do not take it (tests/test_gpu_bpr.py and
tests/test_gpu_bpr_trailing.py pin the arithmetic)."""
import numpy as np
import pytest
import torch

from elliot_amd import ops

pytestmark = pytest.mark.gpu

NINE = ("Gu", "mGu", "vGu", "Gi", "mGi", "vGi", "Bi", "mBi", "vBi")
ITEM = ("Gi", "mGi", "vGi", "Bi", "mBi", "vBi")
LR, L_W, L_B = 0.01, 0.1, 0.001


def _tables(rs, U, I, F):
    Gu = rs.normal(scale=0.1, size=(U, F)).astype(np.float32)
    Gi = rs.normal(scale=0.1, size=(I, F)).astype(np.float32)
    Bi = rs.normal(scale=0.01, size=I).astype(np.float32)
    return Gu, Gi, Bi


def _batch(rs, dev, users, I):
    """Triplets for the given user column: i and j uniform over the catalogue, j != i."""
    users = np.asarray(users, dtype=np.int32)
    i = rs.randint(0, I, size=users.size).astype(np.int32)
    j = ((i + 1 + rs.randint(0, I - 1, size=users.size)) % I).astype(np.int32)
    return tuple(torch.from_numpy(x).to(dev) for x in (users, i, j))


def _mk(ctx, tabs, **kw):
    return ops.BprmfDeviceState(ctx, *tabs, optimizer="adam_tf_dense", compact_user_grads=True, **kw)


def _same(a, b, names, tag):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (tag, name, int((x != y).sum()), float((x - y).abs().max()))


@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("F", [4, 12, 128, 256, 512])
def test_row_widths(ctx, F, B, lib_option):
    """U = 64, I = 37, exact replay, 6 steps, syncs after steps 1, 2, 4 and 6; the deferred form against the every-row form, all nine
    tables.  F = 4 and 12: one and three live lanes per row (the e < F guard), 128: the headline instantiation, 256 and 512: the wide
    rows, up to two element groups per lane, and at 512 the flush walks a row in several passes.  B = 300 brings every user back in consecutive steps: m and v
    stored non-temporally by step t are loaded non-temporally by step t + 1, theta stored with the default policy is gathered by the
    item segments of the same step; B = 1: a single position."""
    lib_option("ichunk", 1 << 20)
    U, I = 64, 37
    rs = np.random.RandomState(1000 * F + B)
    tabs = _tables(rs, U, I, F)
    a, b = _mk(ctx, tabs, deferred=False), _mk(ctx, tabs, deferred=True)
    assert a.fused and not a.deferred and b.deferred and b.item_fused
    for s in range(1, 7):
        if B == 300:
            users = np.concatenate([np.arange(U), np.full(10, s % U), rs.randint(0, U, size=B - U - 10)])
            rs.shuffle(users)
        else:
            users = np.array([11 + (s // 3)])
        t = _batch(rs, ctx.device, users, I)
        for st in (a, b):
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        if s in (1, 2, 4, 6):
            b.sync()
            assert int(b.Gu_last.min()) == b.step == int(b.Gu_last.max())
            _same(a, b, NINE, (s, F, B))


@pytest.mark.parametrize("F", [128, 256])
def test_deferred_item_rows(ctx, F, lib_option):
    """U = 300, I = 1000, B = 64: 2 B <= I turns the item deferral on, an item that comes back after a gap is caught up by
    k_bpr_catchup_items before its segment takes the step.  5 steps, sync(), against the two-pass form (grads() + apply())."""
    lib_option("ichunk", 1 << 20)
    U, I, B = 300, 1000, 64
    rs = np.random.RandomState(F)
    tabs = _tables(rs, U, I, F)
    a = _mk(ctx, tabs, deferred=False, fused_item_step=False)
    b = _mk(ctx, tabs, deferred=True)
    first = None
    for s in range(1, 6):
        users = rs.randint(0, U, size=B)
        t = _batch(rs, ctx.device, users, I)
        if s == 1:
            first = t
        elif s == 4:                                            # the items of step 1 again: every one of them waited for steps 2 and 3
            t = (t[0], first[1], first[2])
        a.grads(t[0], t[1], t[2], L_W, L_B)
        a.apply(LR)
        b.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        assert b.item_fused and b.item_deferred
    assert int(b.Gi_last.min()) < b.step                        # rows are waiting
    b.sync()
    assert int(b.Gi_last.min()) == b.step == int(b.Gi_last.max())
    _same(a, b, ITEM, F)


def test_cut_item_segments_beside_whole_ones(ctx, lib_option):
    """16-position item chunks, U = 300, I = 37, F = 128, B = 2048, 3 steps without a sync of the user table: the partial rows of cut
    segments (default policy, read back by the combine kernel) and the m, v of whole segments (non-temporal) in the same launch."""
    lib_option("ichunk", 16)
    U, I, F, B = 300, 37, 128, 2048
    rs = np.random.RandomState(5)
    tabs = _tables(rs, U, I, F)
    a, b = _mk(ctx, tabs, deferred=False), _mk(ctx, tabs, deferred=True)
    for s in range(1, 4):
        t = _batch(rs, ctx.device, rs.randint(0, U, size=B), I)
        for st in (a, b):
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        if s in (1, 3):
            _same(a, b, ITEM, s)
    _same(a, b, NINE, "end")


def test_series_replay(ctx, lib_option):
    """U = 4099, I = 1000, F = 128, 8 steps from a sixteenth of the users, then sync().  Two runs from the same tables: the same bytes in
    all nine tables.  Against the step-by-step replay on the same batches: the bound of
    tests/test_gpu_bpr.py::test_series_replay_matches_the_step_by_step_replay (restated: it is a closure there)."""
    lib_option("ichunk", 1 << 20)
    U, I, F, B = 4099, 1000, 128, 600
    tabs = _tables(np.random.RandomState(8), U, I, F)

    def run(mode):
        rs = np.random.RandomState(88)
        st = _mk(ctx, tabs, deferred=True, replay=mode)
        for s in range(1, 9):
            t = _batch(rs, ctx.device, rs.randint(0, U // 16, size=B), I)
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        st.sync()
        assert int(st.Gu_last.min()) == st.step == int(st.Gu_last.max())
        return st

    s1, s2, ex = run("series"), run("series"), run("exact")
    assert s1._c.replay_series == 1 and ex._c.replay_series == 0
    _same(s1, s2, NINE, "run to run")
    for name in ("Gu", "Gi", "Bi"):
        x, y = getattr(ex, name), getattr(s1, name)
        err = (x - y).abs()
        assert float((err > 1e-6 * (1 + x.abs())).float().mean()) < 1e-4 and float(err.max()) < 5 * LR, (name, float(err.max()))
    for name in ("mGu", "vGu", "mGi", "vGi", "mBi", "vBi"):
        x, y = getattr(ex, name), getattr(s1, name)
        rel = (x - y).abs() / (x.abs() + float(x.abs().mean()) + 1e-30)
        assert float((rel > 1e-4).float().mean()) < 1e-4 and float(rel.median()) < 1e-6, (name, float(rel.max()))
