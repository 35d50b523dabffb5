"""GPU: the ItemAutoRec / UserAutoRec step (elliot_amd/csrc/el_autorec.hip) at the edges of its kernels, against the dense fp64
restatement of the reference's lines (tests/helpers/autorec_ref.py; tests/test_autorec_ref_host.py checks the helper, the cases and the
bounds without a GPU).  Every case runs for both heads (linear: UserAutoRec, sigmoid: ItemAutoRec).
  k_ar_item_light / k_ar_item_heavy   items in exactly 16 and 17 batch rows (the hand-over between the two), in every row, in none (exact
                                      zeros), in the last row alone; rows without entries; one row id at two batch positions; the batch
                                      mean over 2 B rows; a second step on the same state
  chunks per lane                     H = 4, 260, 516, 772, 1024 -> CPL 1, 2, 3, 4, 4; H = 1024 asks for 64 KiB + (k_ar_dec, k_ar_item_heavy)
  presence bits                       B = 1100, 2048 (the 17-row item at positions >= 1024 only), 2049 and 5000 on the same sparse path
  k_ar_adam                           scalar tails of lengths 203 and 7 against an fp32 restatement, m and v bit for bit; zero gradients move
  repeatability                       the same step twice: the same bytes in every gradient and variable
  prediction                          the user block and the transposed item block (row bias + sigmoid) within 1e-4 of fp64
Every gradient call starts from gradient buffers full of NaN and must leave none.
"""
import numpy as np
import pytest
import torch

from elliot_amd import ops
from tests.gpu_util import cpu
from tests.helpers import autorec_ref as ar

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float("nan")
ACT = {"linear": None, "sigmoid": "sigmoid"}


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _state(ctx, c, head, max_batch=None, nnz_max=None, w=None):
    """Device state and train matrix of a case, after the prescribed in-batch counts were checked on the host."""
    b = c.batch
    cnt = ar.batch_counts(b.indptr, b.indices, b.rows, c.N)
    for item, n in c.want_counts.items():
        assert cnt[item] == n, (c.name, item, int(cnt[item]), n)
    st = ops.AutoRecDeviceState(ctx, c.w if w is None else w, ACT[head], max_batch=c.B if max_batch is None else max_batch,
                                nnz_max=c.nnz if nnz_max is None else nnz_max)
    return st, ops.DeviceCSR(b.indptr, b.indices, c.N, ctx.device)


def _grads(ctx, st, csr, c, n_global=None):
    for g in st.g:
        g.fill_(NAN)
    st.pop_loss()
    st.grads(csr, _dev(ctx, c.batch.rows), n_global=n_global)
    loss = st.pop_loss()
    return loss, {k: cpu(t) for k, t in zip(st.ORDER, st.g)}


def _check(c, head, loss, got, want_loss, want, n_global, tag=""):
    """Loss within 1e-4 relative of fp64; each gradient tensor within 2e-5 of its reference's largest |entry|; the rows of gW1 of the
    16-, 17-, one- and no-row items each within 2e-5 of THAT row's largest |entry|; every row of gW2T and entry of gb2 within
    2e-5 (2 / B_global) n_j; the rows of the item in no batch row exactly zero; no NaN left."""
    v = ar.grad_violations(got, want, c.counts, n_global or c.B, c.special)
    print(c.name, head, tag, "loss %.9g want %.9g (%.3g of the bound);" % (loss, want_loss, abs(loss - want_loss) / (ar.LOSS_RTOL * abs(want_loss))),
          " ".join("%s %.3g" % (k, m) for k, _, _, m in v))
    for k in ar.ORDER:
        assert not np.isnan(got[k]).any(), (k, "left unwritten")
    assert abs(loss - want_loss) <= ar.LOSS_RTOL * abs(want_loss), (loss, want_loss)
    for what, err, bound, _ in v:
        assert err <= bound, (c.name, head, tag, what, err, bound)
    none = c.items.none
    assert (got["W1"][none] == 0).all() and (got["W2T"][none] == 0).all() and got["b2"][none] == 0


def _run_case(ctx, name, head, n_global=None):
    c = ar.case_inputs(name)
    st, csr = _state(ctx, c, head)
    loss, got = _grads(ctx, st, csr, c, n_global)
    want_loss, want = ar.run_reference(name, head, n_global)
    _check(c, head, loss, got, want_loss, want, n_global)
    return c, st, csr


# ---- 1. the edge case ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ar.HEADS)
def test_step_with_16_and_17_row_items_empty_rows_and_a_repeated_row(ctx, head):
    """N = 203, B = 150: item 1 in 16 batch rows (k_ar_item_light's last), item 2 in 17 (k_ar_item_heavy's first), item 0 in every row,
    item 3 in none, item 202 in the last row alone; three rows without entries (h = sigmoid(b1), nothing added to the loss); one row id
    at two batch positions.  Then the same with the batch mean over 2 B rows, then -- after one Adam step -- a second step on the same
    state, against fp64 on the variables the device now holds."""
    c, st, csr = _run_case(ctx, "edge", head)
    h = cpu(st.h)[list(c.empty)]
    want_h = 1.0 / (1.0 + np.exp(-c.w["b1"].astype(np.float64)))
    assert np.abs(h - want_h[None, :]).max() < 1e-6
    assert (cpu(st.dh)[list(c.empty)] == 0).all()
    loss, got = _grads(ctx, st, csr, c, 2 * c.B)
    _check(c, head, loss, got, *ar.run_reference("edge", head, 2 * c.B), 2 * c.B, tag="B_global = 2B")
    loss, got = _grads(ctx, st, csr, c)                              # (the gradients of the step that follows)
    st.apply(0.01)
    w2 = st.weights()
    want_loss, want = ar.ref_grads(w2, c.Xb, head)
    loss, got = _grads(ctx, st, csr, c)
    _check(c, head, loss, got, float(want_loss), want, None, tag="second step")


# ---- 2. chunks per lane; the LDS requests at H = 1024 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ar.HEADS)
@pytest.mark.parametrize("H", [4, 260, 516, 772, 1024])
def test_step_at_every_chunks_per_lane(ctx, H, head):
    _run_case(ctx, f"cpl-H{H}", head)


# ---- 3. large batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ar.HEADS)
@pytest.mark.parametrize("name", ["big-B1100", "big-B2048", "big-B2049", "big-B5000"])
def test_step_with_large_batches_on_the_sparse_path(ctx, name, head):
    """Item 2 is in 17 rows, all at batch positions >= 1024 (>= 4096 at B = 5000); item 1 in the 16 rows around that position; item 0
    in every row.  B = 2049 and 5000 are beyond the VAE's presence flags: the same kernels."""
    _run_case(ctx, name, head)


def test_a_batch_with_more_entries_than_nnz_max_is_refused_loudly(ctx):
    c = ar.case_inputs("edge")
    st, csr = _state(ctx, c, "linear", nnz_max=c.nnz - 1)
    st.grads(csr, _dev(ctx, c.batch.rows))
    with pytest.raises(ops._lib.ElliotHipError):
        st.pop_loss()
    with pytest.raises(ops._lib.ElliotHipError):
        ops.AutoRecDeviceState(ctx, c.w, None, max_batch=262145, nnz_max=10).grads(csr, _dev(ctx, c.batch.rows))


# ---- 4. Adam in isolation ------------------------------------------------------------------------------------------------------------------
def test_adam_tails_match_the_fp32_restatement(ctx):
    """k_ar_adam on known slots: b2 of 203 entries (N = 203: 16-byte lanes and a scalar tail of 3) and of 7 entries (N = 7, H = 4).
    g and v hold zeros (also together: the update is m alpha / eps, the element still moves).  Two steps against vae_ref.adam_f32:
      m, v   only IEEE fp32 add and multiply, compiled without contraction: bit-equal
      th     update = (m alpha) / (sqrt(v) + eps): the multiply, the square root, the add and the divide may each be off by one rounding
             (2^-24 relative) on the device, so the update differs by at most 4 x 2^-24 |update|; the final th - update rounds once more
             on each side: ulp(th).  The bound is this derivation, not what a device gives."""
    for N, H in ((203, 64), (7, 4)):
        st = ops.AutoRecDeviceState(ctx, ar.init_weights(N, H, 5), None, max_batch=8, nnz_max=64)
        assert st.w[3].numel() == N
        rs = np.random.RandomState(77)
        host = {"g": [], "m": [], "v": []}
        for k in range(4):
            shape = tuple(st.w[k].shape)
            g = (rs.normal(size=shape) * 1e-3).astype(f32)
            m = (rs.normal(size=shape) * 1e-3).astype(f32)
            v = (rs.uniform(0, 1e-3, size=shape) ** 2).astype(f32)
            g[rs.rand(*shape) < 0.2] = 0
            v[rs.rand(*shape) < 0.2] = 0
            g.reshape(-1)[-1], v.reshape(-1)[-1] = 0, 0                  # the last entry (in the scalar tail): g = 0 and v = 0
            if g.ndim == 2:
                g[1] = 0                                                 # a row with zero gradient still moves
            for slot, a in (("g", g), ("m", m), ("v", v)):
                host[slot].append(a)
            st.g[k].copy_(_dev(ctx, g)), st.m[k].copy_(_dev(ctx, m)), st.v[k].copy_(_dev(ctx, v))
        th = [cpu(t).copy() for t in st.w]
        m, v = host["m"], host["v"]
        lr = 0.001
        for step in (1, 2):
            st.apply(lr)
            for k, nm in enumerate(st.ORDER):
                want_th, want_m, want_v, upd = ar.adam_f32(th[k], host["g"][k], m[k], v[k], ops.adam_lr_t(lr, step))
                got_th, got_m, got_v = cpu(st.w[k]), cpu(st.m[k]), cpu(st.v[k])
                assert np.array_equal(got_m.view(np.uint32), want_m.view(np.uint32)), (N, step, nm)
                assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), (N, step, nm)
                bound = 4 * 2.0 ** -24 * np.abs(upd.astype(np.float64)) + np.spacing(np.maximum(np.abs(th[k]), np.abs(want_th))).astype(np.float64)
                err = np.abs(got_th.astype(np.float64) - want_th.astype(np.float64))
                assert np.isfinite(got_th).all() and (err <= bound).all(), (N, step, nm, float((err / bound).max()))
                if got_th.ndim == 2:
                    assert (got_th[1] != th[k][1]).any(), "a row with zero gradient did not move"
                th[k], m[k], v[k] = got_th.copy(), got_m.copy(), got_v.copy()


# ---- 5. repeatability ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ar.HEADS)
def test_the_same_step_twice_gives_the_same_bytes(ctx, head):
    c = ar.case_inputs("big-B1100")
    runs = []
    for _ in range(2):
        st, csr = _state(ctx, c, head)
        st.train_step(csr, _dev(ctx, c.batch.rows), 0.01)
        runs.append([cpu(t).copy() for t in st.g + st.w])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 6. prediction -------------------------------------------------------------------------------------------------------------------------
def test_user_block_prediction_matches_fp64(ctx):
    """N = 203: the encoder on a block of rows (three without entries) + one product against W2T with the bias b2."""
    c = ar.case_inputs("edge")
    st, csr = _state(ctx, c, "linear")
    got = cpu(st.predict_rows(csr, _dev(ctx, c.batch.rows)))
    want = ar.predict(c.w, c.Xb, "linear")
    assert got.shape == want.shape == (c.B, c.N)
    print("user block: max |r - fp64| %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() < 1e-4
    assert np.abs(got[list(c.empty)] - want[list(c.empty)]).max() < 1e-4


def test_item_block_prediction_is_the_transposed_output_with_row_bias_and_sigmoid(ctx):
    """The item variant at layer width 203: every row of the matrix is encoded once, a block of columns u of the output is
    sigmoid(W2T[u] . h[i] + b2[u]) -- the transpose the reference takes on the host.  Rows and columns without entries included."""
    c = ar.case_inputs("edge")
    st, csr = _state(ctx, c, "sigmoid")
    R = c.batch.X.shape[0]
    want = ar.predict(c.w, c.batch.X, "sigmoid").T                                # [N, R]
    h_all = st.encode(csr, torch.arange(R, dtype=torch.int32, device=ctx.device))
    for start, stop in ((0, c.N), (3, 100), (100, c.N)):
        got = cpu(st.predict_columns(h_all, start, stop))
        assert got.shape == (stop - start, R)
        err = np.abs(got - want[start:stop]).max()
        print("item block [%d, %d): max |r - fp64| %.3g" % (start, stop, err))
        assert err < 1e-4
