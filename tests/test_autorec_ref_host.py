"""CPU: tests/helpers/autorec_ref.py before any GPU holds a kernel to it.
  - its hand-written gradients equal torch CPU autograd in fp64 of the same dense formula, to 1e-12
  - a FLOAT32 evaluation of the dense formula stays within the GPU tests' bounds on every case, at most half of each (a case beyond that
    is changed, not the bound): the bounds ask for fp32-level accuracy, not for more than the reference's own arithmetic gives
  - the plugin test's data: the float32 restatement's distance from fp64 after the same steps is what the helper's constant says, and
    the float32 restatement alone satisfies the top-10 rule of the GPU test
"""
import numpy as np
import pytest
import torch

from tests.helpers import autorec_ref as ar

f32 = np.float32


@pytest.mark.parametrize("head", ar.HEADS)
@pytest.mark.parametrize("name", ["edge", "cpl-H260"])
def test_hand_written_gradients_equal_autograd_in_fp64(name, head):
    c = ar.case_inputs(name)
    for n_global in (None, 2 * c.B):
        loss, g = ar.ref_grads(c.w, c.Xb, head, n_global)
        t = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in c.w.items()}
        batch = torch.tensor(c.Xb.astype(np.float64))
        reconstructed = torch.sigmoid(batch @ t["W1"] + t["b1"]) @ t["W2"] + t["b2"]
        if head == "sigmoid":
            reconstructed = torch.sigmoid(reconstructed)
        reconstructed = reconstructed * torch.sign(batch)
        error = batch - reconstructed
        tl = torch.mean(torch.sum(error ** 2, dim=1)) * (c.B / (n_global or c.B))
        tl.backward()
        want = {"W1": t["W1"].grad.numpy(), "b1": t["b1"].grad.numpy(), "W2T": t["W2"].grad.numpy().T, "b2": t["b2"].grad.numpy()}
        assert abs(float(loss) - float(tl)) <= 1e-12 * max(1.0, abs(float(tl)))
        for k in ar.ORDER:
            err = float(np.abs(g[k] - want[k]).max())
            assert err <= 1e-12 * max(1.0, float(np.abs(want[k]).max())), (name, head, k, err)


@pytest.mark.parametrize("head", ar.HEADS)
@pytest.mark.parametrize("name", list(ar.CASES))
def test_cases_hold_what_they_promise_and_float32_stays_within_half_of_every_bound(name, head):
    c = ar.case_inputs(name)
    b = c.batch
    cnt = ar.batch_counts(b.indptr, b.indices, b.rows, c.N)
    for item, n in c.want_counts.items():
        assert cnt[item] == n, (name, item, int(cnt[item]), n)
    assert (cnt == c.counts).all() and c.nnz == cnt.sum()
    if hasattr(c, "straddle"):
        assert (c.pos17 >= c.hi17[0]).all() and c.pos16.min() < c.straddle <= c.pos16.max()
    if c.dup:
        assert b.rows[c.dup[0]] == b.rows[c.dup[1]]
    for e in c.empty:
        assert c.Xb[e].sum() == 0
    for n_global in ((None, 2 * c.B) if name == "edge" else (None,)):
        want_loss, want = ar.run_reference(name, head, n_global)
        loss, got = ar.ref_grads(c.w, c.Xb, head, n_global, dtype=f32)
        v = ar.grad_violations(got, want, c.counts, n_global or c.B, c.special)
        share = abs(float(loss) - want_loss) / (ar.LOSS_RTOL * abs(want_loss))
        print(name, head, n_global, "float32: loss %.3g of its bound;" % share, " ".join("%s %.3g" % (k, m) for k, _, _, m in v))
        assert share <= 0.5
        for what, err, bound, margin in v:
            assert margin <= 0.5, (name, head, what, err, bound)
        assert (want["W1"][c.items.none] == 0).all() and (want["W2T"][c.items.none] == 0).all() and want["b2"][c.items.none] == 0


def _plugin_runs(which):
    P = ar.PLUGIN
    w = ar.plugin_weights(which)
    batches, evals, _ = ar.plugin_batches(which)
    th32 = ar.train_ref(w, ar.plugin_rows_matrix(which), batches, P.lr, ar.plugin_head(which), f32)[0]
    return w, ar.plugin_reference(which)[0], th32, evals


@pytest.mark.parametrize("which", ["UserAutoRec", "ItemAutoRec"])
def test_plugin_data_float32_distance_and_top10_rule(which):
    P = ar.PLUGIN
    X = ar.plugin_matrix()
    _, th64, th32, evals = _plugin_runs(which)
    dist = max(float(np.abs(th32[k].astype(np.float64) - th64[k]).max()) for k in ar.ORDER)
    const = ar.PLUGIN_F32_DISTANCE[which]
    print(which, "float32 restatement: max |variable - fp64| = %.3g (constant %.3g)" % (dist, const))
    assert 0.5 * const <= dist <= 1.5 * const, (dist, const)     # the constant IS this distance as measured (another BLAS may round otherwise)
    for order in [None] + ([evals[-1]] if which == "ItemAutoRec" else []):
        s64, s32 = ar.plugin_scores(th64, which, np.float64, order), ar.plugin_scores(th32, which, f32, order)
        ok = ar.decided_users(s64, X, P.k, 2 * const)
        print(which, "users decided by the gap rule: %d of %d" % (int(ok.sum()), P.U))
        assert (~ok).sum() <= 0.1 * P.U
        a, b = ar.topk_lists(s64, X, P.k), ar.topk_lists(s32.astype(np.float64), X, P.k)
        assert (a[ok] == b[ok]).all()


def test_plugin_batches_leave_random_alone():
    import random
    s = random.getstate()
    ar.plugin_batches("ItemAutoRec")
    assert random.getstate() == s
