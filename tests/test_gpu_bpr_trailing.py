"""The deferred decay with user rows that trail one Adam move (el_bprmf_state.Gu_last < 0: m, v current at s = ~Gu_last, theta as it
stood before the move of step s, that move owed), the item side reading the pre-update rows from Gu in place, and the item flush
that replays the biases inside the row kernel.  Everything here is bit for bit against the every-row forms on the same batches."""
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


def _stamps_current(st):
    assert int(st.Gu_last.min()) == st.step == int(st.Gu_last.max())


@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("F", [8, 128, 256])
def test_every_row_touched_every_step(ctx, F, B, lib_option):
    """U = 64, I = 37, exact replay, 6 steps.  B = 300 holds every user in every step (a sync right after a step that touched all rows:
    the flush has 64 theta-only visits and nothing else), one user owns a segment longer than the four positions of a user chunk, and
    the same users come back in consecutive steps, so a segment head meets an owed move with no step to replay (steps 3 and 5 are not
    synced: their moves are taken by the segments of steps 4 and 6).  B = 7: one user six times, one once; B = 1: a single position."""
    lib_option("ichunk", 1 << 20)
    U, I = 64, 37
    rs = np.random.RandomState(1000 * F + B)
    tabs = _tables(rs, U, I, F)
    a, b = _mk(ctx, tabs, deferred=False), _mk(ctx, tabs, deferred=True)
    assert a.fused and not a.deferred and b.deferred
    for s in range(1, 7):
        if B == 300:
            users = np.concatenate([np.arange(U), np.full(10, s % U), rs.randint(0, U, size=B - U - 10)])
            rs.shuffle(users)
        elif B == 7:
            users = np.array([3, 3, 3, 3, 3, 3, 5 + (s % 2)])
        else:
            users = np.array([11 + (s // 3)])
        t = _batch(rs, ctx.device, users, I)
        for st in (a, b):
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        if s in (1, 2, 4, 6):
            assert int((b.Gu_last < 0).sum()) >= len(set(users.tolist()))
            b.sync()
            _stamps_current(b)
            _same(a, b, NINE, (s, F, B))


@pytest.mark.parametrize("B", [7, 600])
@pytest.mark.parametrize("hist", [4, 8])
def test_owed_moves_meet_the_lr_ring(ctx, hist, B, monkeypatch, lib_option):
    """U = 4099, I = 1000, F = 128, a 4- and an 8-entry lr ring, 12 steps: batches from a sixteenth of the users, step 7 from all of
    them.  Before a sync the rows with a negative stamp are exactly the distinct users of the batches since the table was last brought
    up to date -- by a sync, or by the flush the library runs in front of every step k * hist / 2 + 1 -- each stamped ~(its last step);
    at steps 1 and 5 (a flush ran in front of step 5 with either ring) that is the last batch alone.  After the sync none is left, a
    second sync -- the call, and the kernel run again with nothing pending -- changes nothing.  All nine tables equal the every-row
    form's at steps 1, 5 and 12."""
    lib_option("ichunk", 1 << 20)
    monkeypatch.setattr(ops.BprmfDeviceState, "_LR_HIST", hist)
    U, I, F = 4099, 1000, 128
    rs = np.random.RandomState(hist * 1000 + B)
    tabs = _tables(rs, U, I, F)
    a, b = _mk(ctx, tabs, deferred=False), _mk(ctx, tabs, deferred=True)
    assert b.deferred and b._c.lr_hist_cap == hist
    owed = {}                                                   # user -> the step whose move it owes
    for s in range(1, 13):
        users = rs.randint(0, U if s == 7 else U // 16, size=B)
        t = _batch(rs, ctx.device, users, I)
        for st in (a, b):
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        if s > 1 and (s - 1) % (hist // 2) == 0:
            owed = {}                                           # the half-ring flush in front of this step
        owed.update({int(u): s for u in users})
        if s in (1, 5, 12):
            assert b._pending
            last = b.Gu_last.cpu().numpy()
            neg = np.nonzero(last < 0)[0]
            assert sorted(neg.tolist()) == sorted(owed), (s, len(neg), len(owed))
            assert all(int(~last[u]) == st_ for u, st_ in owed.items())
            if s in (1, 5):
                assert len(neg) == len(set(users.tolist()))
            b.sync()
            assert not b._pending and int((b.Gu_last < 0).sum()) == 0
            _stamps_current(b)
            snap = {n: getattr(b, n).clone() for n in NINE}
            b.sync()
            b._pending = True                                   # the flush kernel itself, with no row pending
            b.sync()
            assert not b._pending
            _stamps_current(b)
            for n in NINE:
                assert torch.equal(snap[n].view(torch.int32), getattr(b, n).view(torch.int32)), (s, n)
            _same(a, b, NINE, (s, hist, B))
            owed = {}


def test_item_side_reads_the_trailing_rows_in_place_with_cut_rows(ctx, lib_option):
    """U = 300, I = 37, F = 128, B = 2048, 16-position item chunks: every item's segment is cut into partial rows, gamma_u comes from
    Gu itself.  The item side after 1 and after 3 steps (no sync of the user table in between: steps 2 and 3 gather rows whose owed
    move the user segments of the same step have just taken)."""
    lib_option("ichunk", 16)
    U, I, F, B = 300, 37, 128, 2048
    rs = np.random.RandomState(3)
    tabs = _tables(rs, U, I, F)
    a, b = _mk(ctx, tabs, deferred=False), _mk(ctx, tabs, deferred=True)
    for s in range(1, 4):
        t = _batch(rs, ctx.device, rs.randint(0, U, size=B), I)
        for st in (a, b):
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        if s in (1, 3):
            _same(a, b, ITEM, s)
    _same(a, b, NINE, "end")


@pytest.mark.parametrize("I", [37, 65, 1000])
def test_waiting_item_rows_with_the_bias_replay_inside_the_flush(ctx, I, lib_option):
    """B = 7, item rows replayed at the end of every step (set_item_deferred(False)): the flush kernel's lanes replay their rows' biases
    before the rows are walked and stamped.  I = 37: part of one wave's 64 rows; 65: a second wave with one row; 1000: several
    workgroups.  Against a state run through the two-pass form, grads() + apply(), 5 steps."""
    lib_option("ichunk", 1 << 20)
    U, F, B = 64, 128, 7
    rs = np.random.RandomState(I)
    tabs = _tables(rs, U, I, F)
    a = _mk(ctx, tabs, deferred=False, fused_item_step=False)
    b = _mk(ctx, tabs, deferred=True, fused_item_step=True)
    b.set_item_deferred(False)
    assert b.item_fused and not b.item_deferred
    for s in range(1, 6):
        t = _batch(rs, ctx.device, rs.randint(0, U, size=B), I)
        a.grads(t[0], t[1], t[2], L_W, L_B)
        a.apply(LR)
        b.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        assert int(b.Gi_last.min()) == s == int(b.Gi_last.max())
        _same(a, b, ITEM, (s, I))


@pytest.mark.parametrize("how", ["set_deferred", "step", "two_pass"])
def test_leaving_the_mode_with_moves_owed(ctx, how, lib_option):
    """Three steps on the deferred state leave moves owed; then the mode is left -- set_deferred(False), the step counter set from
    outside, a grads() + apply() pair -- and one more step follows.  The every-row state goes through the same calls."""
    lib_option("ichunk", 1 << 20)
    U, I, F, B = 257, 37, 128, 100
    rs = np.random.RandomState(17)
    tabs = _tables(rs, U, I, F)
    a, b = _mk(ctx, tabs, deferred=False), _mk(ctx, tabs, deferred=True)
    for s in range(3):
        t = _batch(rs, ctx.device, rs.randint(0, U // (1 + s), size=B), I)
        for st in (a, b):
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
    assert b._pending and int((b.Gu_last < 0).sum()) > 0
    t = _batch(rs, ctx.device, rs.randint(0, U, size=B), I)
    for st in (a, b):
        if how == "set_deferred":
            st.set_deferred(False)
        elif how == "step":
            st.step = 10
        else:
            st.grads(t[0], t[1], t[2], L_W, L_B)
            st.apply(LR)
    if how != "set_deferred":
        assert int((b.Gu_last < 0).sum()) == 0
        _stamps_current(b)
    _same(a, b, NINE, how)
    for st in (a, b):
        st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
    _same(a, b, NINE, (how, "next step"))


def test_series_replay_with_trailing_rows(ctx, lib_option):
    """The closed-form replay: the owed move is Keras' own (exact), the gap behind it in closed form.  The same run twice gives the same
    bits; against the step-by-step replay it stays inside what tests/test_gpu_bpr.py asks of that pair (theta 4e-6 on all but 1e-4 of
    the elements, v 1e-7)."""
    lib_option("ichunk", 1 << 20)
    U, I, F, B = 4099, 1000, 128, 600
    tabs = _tables(np.random.RandomState(6), U, I, F)

    def run(mode):
        rs = np.random.RandomState(66)
        st = _mk(ctx, tabs, deferred=True, replay=mode)
        for s in range(1, 13):
            t = _batch(rs, ctx.device, rs.randint(0, U if s == 7 else U // 16, size=B), I)
            st.train_step(t[0], t[1], t[2], LR, L_W, L_B)
        st.sync()
        _stamps_current(st)
        return st

    s1, s2, ex = run("series"), run("series"), run("exact")
    assert s1._c.replay_series == 1 and ex._c.replay_series == 0
    _same(s1, s2, NINE, "run to run")
    assert float(((s1.Gu - ex.Gu).abs() > 4e-6).float().mean()) < 1e-4
    assert float((s1.vGu - ex.vGu).abs().max()) <= 1e-7
