"""GPU parity: BPR sampler, BPRMF_batch train step (TF semantics) and BPRMF per-sample SGD (NumPy
semantics) against the CPU oracle / the reference-generated fixtures."""
import numpy as np
import pytest
import torch

from elliot_amd import ops
from elliot_amd.synthetic import zipf_csr
from oracle import bprmf_batch as ob
from oracle import sampler as osampler
from oracle import sgd as osgd
from tests.gpu_util import cpu, dump

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------- sampler
def test_philox_sampler_bitexact_vs_oracle(ctx, golden):
    g = golden("sampler_ref.npz")
    U, I = int(g["n_users"]), int(g["n_items"])
    pos = ops.DeviceCSR(g["indptr"], g["indices"], I, ctx.device)
    n = 5000
    u, i, j = ops.bpr_sample(ctx, pos, n, seed=42, first_sample=1000)
    torch.cuda.synchronize()
    eu, ei, ej = osampler.philox_sample(g["indptr"], g["indices"], U, I, 42, 1000, n)
    assert np.array_equal(cpu(u), eu) and np.array_equal(cpu(i), ei) and np.array_equal(cpu(j), ej)


def test_philox_sampler_invariants_and_distribution(ctx):
    U, I = 5000, 3000
    indptr, indices = zipf_csr(U, I, mean_log=3.0, sigma_log=0.8, dmin=1, dmax=300, seed=3)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    n = 400_000
    u, i, j = (cpu(t).astype(np.int64) for t in ops.bpr_sample(ctx, pos, n, seed=7))
    assert u.min() >= 0 and u.max() < U and j.min() >= 0 and j.max() < I
    rowsets = [set(indices[indptr[x]:indptr[x + 1]].tolist()) for x in range(U)]
    for uu, ii, jj in zip(u[:20000], i[:20000], j[:20000]):
        assert ii in rowsets[uu] and jj not in rowsets[uu]
    # users uniform (custom_sampler.py:32): chi-square-ish bound on the bin counts
    cnt = np.bincount(u, minlength=U)
    assert abs(cnt.mean() - n / U) < 1e-9 and cnt.std() < 1.25 * np.sqrt(n / U)
    # sharded negatives stay in range
    u2, i2, j2 = (cpu(t) for t in ops.bpr_sample(ctx, pos, 10000, seed=7, item_lo=1000, item_hi=1500))
    assert j2.min() >= 1000 and j2.max() < 1500
    # different sample offsets reproduce the same stream
    a = cpu(ops.bpr_sample(ctx, pos, 100, seed=7, first_sample=50)[2])
    assert np.array_equal(a, j[50:150].astype(np.int32))


# ---------------------------------------------------------------------------------- BPRMF_batch
def _setup(rs, U, I, F):
    Gu = rs.normal(scale=0.1, size=(U, F)).astype(np.float32)
    Gi = rs.normal(scale=0.1, size=(I, F)).astype(np.float32)
    Bi = rs.normal(scale=0.01, size=I).astype(np.float32)
    return Gu, Gi, Bi


@pytest.mark.parametrize("algo", ["atomic", "sorted", "compact"])
@pytest.mark.parametrize("opt", ["adam_tf_dense", "adam_lazy", "sgd"])
@pytest.mark.parametrize("F", [64, 128, 10, 200])
def test_bprmf_train_steps_match_oracle(ctx, opt, F, algo):
    """algo "compact": the sorted path with compact user-gradient rows + stamps (el_bprmf_state.uslot) in place of the dense
    accumulator -- what large user tables run by default."""
    compact = algo == "compact"
    if compact and (opt != "adam_tf_dense" or F % 4):
        pytest.skip("compact user-gradient rows exist for the TF-dense Adam with F % 4 == 0")
    rs = np.random.RandomState(20 + F)
    U, I, B, steps = 500, 300, 1024, 6
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    dev_state = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer=opt, compact_user_grads=compact)
    assert dev_state.compact == compact
    if compact:
        algo = "sorted"
    orc = ob.BPRMFBatchOracle(Gu, Gi, Bi, lr, l_w, l_b, optimizer=opt)
    for s in range(steps):
        u = rs.randint(0, U, B).astype(np.int32)
        i = rs.randint(0, 40, B).astype(np.int32)           # few items -> heavy duplicate rows
        j = rs.randint(0, I, B).astype(np.int32)
        if s == 2:
            u, i, j = u[:1], i[:1], j[:1]                   # B = 1 (the reference's tf.squeeze bug case)
        exp_loss = orc.train_step((u, i, j))
        d = ctx.device
        dev_state.train_step(torch.from_numpy(u).to(d), torch.from_numpy(i).to(d), torch.from_numpy(j).to(d), lr, l_w, l_b,
                             algo=algo)
        got_loss = dev_state.pop_loss()
        assert abs(got_loss - exp_loss) <= 1e-4 * max(1.0, abs(exp_loss)), (s, got_loss, exp_loss)
        for name in ("Gu", "Gi", "Bi"):
            got, exp = cpu(getattr(dev_state, name)), getattr(orc, name)
            err = np.abs(got - exp)
            # Adam's m/(sqrt(v)+eps) is ill-conditioned where a summed gradient cancels to ~0: the fp32
            # summation ORDER of duplicate rows (atomics vs np.add.at) may flip such an element by O(lr).
            # Everything else must agree to fp32 round-off.
            frac_bad = float((err > 2e-5).mean())
            if not (frac_bad <= 2e-4 and err.max() < 5 * lr):
                dump(f"bprmf_{opt}_F{F}_{name}_s{s}", got=got, exp=exp)
            assert frac_bad <= 2e-4 and err.max() < 5 * lr, (opt, F, name, s, float(err.max()), frac_bad)
    # gradient accumulators are left clean
    assert (dev_state.gGu is None or not cpu(dev_state.gGu).any()) and not cpu(dev_state.gGi).any() and not cpu(dev_state.gBi).any()


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("F,B,U,I", [(64, 4096, 700, 300), (128, 20000, 900, 4000), (32, 3000, 40, 60)])
def test_bprmf_summed_gradients_match_oracle_tightly(ctx, compact, F, B, U, I):
    """The pre-optimiser gradients (what OptimizerV2 receives after its segment sum, BPRMF_batch_model.py:77-78) -- not only the
    Adam-squashed weights: gGu / gGi / gBi of el_bprmf_grads against the oracle's fp32 gradients, per tensor within
    1e-5 of the tensor's largest entry (fp32 summation order is the only freedom; hot rows sum thousands of terms)."""
    from elliot_amd import parallel
    rs = np.random.RandomState(7 + F)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    be = parallel.HipUserShardBackend(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense")
    if be.state.compact != compact:
        be.state = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=compact, deferred=False,
                                        fused_user_step=False)              # (what the backend builds: the two-pass form)
    st = be.state
    u = rs.randint(0, U, B).astype(np.int32)
    i = (rs.zipf(1.3, B) % I).astype(np.int32)             # Zipf items: the hottest row collects a large share of the batch
    j = rs.randint(0, I, B).astype(np.int32)
    d = ctx.device
    be.grads(torch.from_numpy(u).to(d), torch.from_numpy(i).to(d), torch.from_numpy(j).to(d), 0.1, 0.001)
    exp_bi, exp_gu, exp_gi = ob.gradients(Gu, Gi, Bi, u.astype(np.int64), i.astype(np.int64), j.astype(np.int64), 0.1, 0.001)
    exp64 = ob.gradients(Gu, Gi, Bi, u.astype(np.int64), i.astype(np.int64), j.astype(np.int64), 0.1, 0.001, dtype=np.float64)
    got = {"gGu": cpu(st.user_grad_dense()), "gGi": cpu(st.gGi), "gBi": cpu(st.gBi)}
    for name, exp, e64 in (("gGu", exp_gu, exp64[1]), ("gGi", exp_gi, exp64[2]), ("gBi", exp_bi, exp64[0])):
        scale = float(np.abs(e64).max())
        err = float(np.abs(got[name] - e64).max())
        ref_err = float(np.abs(exp.astype(np.float64) - e64).max())        # what fp32 summation costs the oracle itself
        assert err <= max(1e-5 * scale, 4 * ref_err), (name, compact, err, ref_err, scale)
    untouched = np.setdiff1d(np.arange(U), u)
    assert not got["gGu"][untouched].any()
    # the optimiser consumes them and hands the accumulators back clean; a second step sees no stale rows
    be.begin_step()
    be.apply_users(0.01)
    be.apply_items(0.01)
    orc = ob.BPRMFBatchOracle(Gu, Gi, Bi, 0.01, 0.1, 0.001)
    orc.train_step((u, i, j))
    u2 = rs.randint(0, max(1, U // 3), B).astype(np.int32)   # other users: rows stamped by step 1 must read as g = 0 in step 2
    be.grads(torch.from_numpy(u2).to(d), torch.from_numpy(i).to(d), torch.from_numpy(j).to(d), 0.1, 0.001)
    be.begin_step()
    be.apply_users(0.01)
    be.apply_items(0.01)
    orc.train_step((u2, i, j))
    assert (np.abs(cpu(st.Gu) - orc.Gu) > 2e-5).mean() <= 2e-4 and not cpu(st.gGi).any()


def test_bprmf_loss_within_1e4_on_ml1m_shaped_batch(ctx):
    """north_star tolerance: loss within 1e-4 (relative) of the oracle on an ML-1M-shaped input."""
    rs = np.random.RandomState(42)
    U, I, F, B = 6040, 3667, 64, 65536
    Gu, Gi, Bi = _setup(rs, U, I, F)
    indptr, indices = zipf_csr(U, I, mean_log=4.3, sigma_log=1.0, dmin=16, dmax=1800, zipf_a=0.8, seed=0)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    u, i, j = ops.bpr_sample(ctx, pos, B, seed=42)
    st = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense")
    orc = ob.BPRMFBatchOracle(Gu, Gi, Bi, 0.001, 0.1, 0.001)
    for s in range(3):
        st.train_step(u, i, j, 0.001, 0.1, 0.001, algo="sorted" if s != 1 else "atomic")
        got = st.pop_loss()
        exp = orc.train_step((cpu(u), cpu(i), cpu(j)))
        exp64 = float(ob.forward_loss(orc.Gu, orc.Gi, orc.Bi, cpu(u).astype(np.int64), cpu(i).astype(np.int64),
                                      cpu(j).astype(np.int64), 0.1, 0.001, dtype=np.float64)) if s == 2 else None
        assert abs(got - exp) / abs(exp) < 1e-4, (s, got, exp)
    assert (np.abs(cpu(st.Gu) - orc.Gu) > 1e-5).mean() < 2e-4 and (np.abs(cpu(st.Gi) - orc.Gi) > 1e-5).mean() < 2e-4


# ---------------------------------------------------------------------------------- BPRMF (NumPy SGD)
def test_bprsgd_level_schedule_equals_reference_sequence(ctx, golden):
    """The reference's own MFModel trace (BPRMF_model.py:87-117): 3000 sequential fp64 updates."""
    g = golden("bprmf_sgd_trace.npz")
    hp = {k: float(g[k]) for k in ("lr", "reg_bias", "reg_user", "reg_pos", "reg_neg")}
    st = ops.BprSgdDeviceState(ctx, g["P0"], g["Q0"], g["b0"], **hp)
    nlev = st.apply_sequential_equivalent(g["u"], g["i"], g["j"])
    torch.cuda.synchronize()
    assert nlev > 1
    for name, exp in (("P", g["P1"]), ("Q", g["Q1"]), ("b", g["b1"])):
        err = np.abs(cpu(getattr(st, name)) - exp).max()
        assert err < 1e-12, (name, err)        # fp64; exp() and the dot-product order differ in the last ulp


def test_bprsgd_conflict_free_batch_equals_oracle(ctx):
    rs = np.random.RandomState(5)
    U, I, n = 4000, 9000, 2000
    for F in (10, 64, 128):
        P, Q, b = osgd.initialize(U, I, F, 1)
        u = rs.permutation(U)[:n].astype(np.int32)
        ij = rs.permutation(I)[:2 * n].astype(np.int32)
        i, j = ij[:n], ij[n:]
        hp = dict(lr=0.05, reg_bias=0.01, reg_user=0.0025, reg_pos=0.0025, reg_neg=0.00025)
        st = ops.BprSgdDeviceState(ctx, P, Q, b, **hp)
        d = ctx.device
        st.apply(torch.from_numpy(u).to(d), torch.from_numpy(i).to(d), torch.from_numpy(j).to(d))
        torch.cuda.synchronize()
        osgd.train_sequential(P, Q, b, u, i, j, **hp)
        assert np.abs(cpu(st.P) - P).max() < 1e-13 and np.abs(cpu(st.Q) - Q).max() < 1e-13
        assert np.abs(cpu(st.b) - b).max() < 1e-13


def test_sorted_path_is_deterministic(ctx):
    """Stable sort -> fixed summation order, and the partial rows of a segment cut by chunk boundaries are added in chunk
    order (k_seg_combine / k_seg_combine_long, el_segcombine.h): two runs give the same bits in every table.  The hottest item's
    segment spans more than 256 chunks, so the workgroup kernel's scan for the segment's end takes more than one pass."""
    rs = np.random.RandomState(77)
    U, I, F, B = 400000, 500, 64, 20000
    Gu, Gi, Bi = _setup(rs, U, I, F)
    d = ctx.device
    u_h = rs.randint(0, U, B).astype(np.int32)
    i_h = (rs.zipf(1.3, B) % I).astype(np.int32)     # very hot items -> multi-chunk segments
    j_h = rs.randint(0, I, B).astype(np.int32)
    # the item side sorts the 2 B positions by item; at this batch size a lane group's chunk is 16 positions (the smallest)
    cnt = np.bincount(np.concatenate([i_h, j_h]), minlength=I)
    hot = int(cnt.argmax())
    p0 = int(cnt[:hot].sum())
    assert (p0 + int(cnt[hot]) - 1) // 16 - p0 // 16 + 1 > 256
    u, i, j = (torch.from_numpy(x).to(d) for x in (u_h, i_h, j_h))
    outs = []
    for _ in range(2):
        st = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense")
        st.train_step(u, i, j, 0.01, 0.1, 0.001, algo="sorted")
        outs.append((cpu(st.Gu).copy(), cpu(st.Gi).copy(), cpu(st.Bi).copy(), st.pop_loss()))
    for k in range(3):
        assert np.array_equal(outs[0][k].view(np.int32), outs[1][k].view(np.int32)), ("Gu", "Gi", "Bi")[k]
    assert abs(outs[0][3] - outs[1][3]) < 1e-3       # (the loss is summed with double-precision atomics)


# ---------------------------------------------------------------------------------- item-sharded path
def test_item_sharded_hip_path_equals_concatenated_batch(ctx):
    """Two virtual ranks on one GPU (the all-gather is emulated by torch.cat): the sharded kernels
    (el_bprmf_shard_grads / el_rows_segment_sum / el_bprmf_apply) must reproduce ONE reference-semantics step on
    the concatenated batch, and both user-table replicas must stay bit-identical."""
    from elliot_amd import parallel
    rs = np.random.RandomState(31)
    U, I, F, B, G = 700, 400, 64, 3000, 2
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    d = ctx.device
    bes, rng = [], []
    for r in range(G):
        lo, hi = parallel.item_range(I, r, G)
        rng.append((lo, hi))
        bes.append(parallel.HipBackend(ctx, Gu, Gi[lo:hi], Bi[lo:hi], optimizer="adam_tf_dense"))
    orc = ob.BPRMFBatchOracle(Gu, Gi, Bi, lr, l_w, l_b)
    for step in range(3):
        batches = [(rs.randint(0, U, B), rs.randint(lo, min(lo + 25, hi), B), rs.randint(lo, hi, B)) for lo, hi in rng]
        dUs, us = [], []
        for r, (be, (lo, hi), (u, i, j)) in enumerate(zip(bes, rng, batches)):
            tu = torch.from_numpy(u.astype(np.int32)).to(d)
            dUs.append(be.shard_grads(tu, torch.from_numpy((i - lo).astype(np.int32)).to(d),
                                      torch.from_numpy((j - lo).astype(np.int32)).to(d), l_w, l_b).clone())
            us.append(tu)
        ids, rows = torch.cat(us), torch.cat(dUs)
        loss = 0.0
        for be in bes:
            be.reduce_user_rows(ids, rows)
            be.apply(lr)
            loss += be.state.pop_loss()
        cu, ci, cj = (np.concatenate([b[x] for b in batches]) for x in range(3))
        exp = orc.train_step((cu, ci, cj))
        assert abs(loss - exp) <= 1e-4 * abs(exp), (step, loss, exp)
        assert torch.equal(bes[0].state.Gu, bes[1].state.Gu)
        assert (np.abs(cpu(bes[0].state.Gu) - orc.Gu) > 2e-5).mean() < 2e-4
        for be, (lo, hi) in zip(bes, rng):
            assert (np.abs(cpu(be.state.Gi) - orc.Gi[lo:hi]) > 2e-5).mean() < 2e-4
            assert (np.abs(cpu(be.state.Bi) - orc.Bi[lo:hi]) > 2e-5).mean() < 2e-3
            assert not cpu(be.state.gGu).any() and not cpu(be.state.gGi).any()


def test_item_sharded_dense_exchange_hip_path_equals_concatenated_batch(ctx):
    """"dense" exchange with two virtual ranks on one GPU: el_bprmf_grads -> (emulated) reduce-scatter of the dense
    gradient table -> el_bprmf_apply on the owned user rows -> (emulated) all-gather.  U is odd: padded rows."""
    from elliot_amd import parallel
    rs = np.random.RandomState(32)
    U, I, F, B, G = 701, 400, 64, 3000, 2
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    d = ctx.device
    bes, rng = [], []
    for r in range(G):
        lo, hi = parallel.item_range(I, r, G)
        rng.append((lo, hi))
        bes.append(parallel.HipDenseBackend(ctx, torch.from_numpy(Gu).to(d), Gi[lo:hi], Bi[lo:hi], r, G, optimizer="adam_tf_dense"))
    Us = bes[0].Us
    assert Us * G == 702 and bes[0].state.Gu.shape[0] == 702
    orc = ob.BPRMFBatchOracle(Gu, Gi, Bi, lr, l_w, l_b)
    for step in range(3):
        batches = [(rs.randint(0, U, B), rs.randint(lo, min(lo + 25, hi), B), rs.randint(lo, hi, B)) for lo, hi in rng]
        gs = []
        for be, (lo, hi), (u, i, j) in zip(bes, rng, batches):
            gs.append(be.grads(torch.from_numpy(u.astype(np.int32)).to(d), torch.from_numpy((i - lo).astype(np.int32)).to(d),
                               torch.from_numpy((j - lo).astype(np.int32)).to(d), l_w, l_b))
        gsum = gs[0] + gs[1]                                         # what the reduce-scatter delivers, slice by slice
        loss = 0.0
        for r, be in enumerate(bes):
            be.g_own.copy_(gsum[r * Us:(r + 1) * Us])
            gs[r].zero_()
            be.apply_own(lr)
            loss += be.state.pop_loss()
        full = torch.cat([be.Gu_own for be in bes])                  # the all-gather
        for be in bes:
            be.state.Gu.copy_(full)
        cu, ci, cj = (np.concatenate([b[x] for b in batches]) for x in range(3))
        exp = orc.train_step((cu, ci, cj))
        assert abs(loss - exp) <= 1e-4 * abs(exp), (step, loss, exp)
        assert (np.abs(cpu(bes[0].state.Gu)[:U] - orc.Gu) > 2e-5).mean() < 2e-4
        assert not cpu(bes[0].state.Gu)[U:].any()
        for be, (lo, hi) in zip(bes, rng):
            assert (np.abs(cpu(be.state.Gi) - orc.Gi[lo:hi]) > 2e-5).mean() < 2e-4
            assert (np.abs(cpu(be.state.Bi) - orc.Bi[lo:hi]) > 2e-5).mean() < 2e-3
            assert not cpu(be.state.gGu).any() and not cpu(be.state.gGi).any() and not cpu(be.g_own).any()


def test_user_sharded_hip_path_equals_concatenated_batch(ctx):
    """User shards (parallel.ShardedBprmfByUser) with two virtual ranks on one GPU: local user rows, full item replicas,
    the all-reduce of the item gradients emulated with a torch add (steps 0, 1) and the row-sparse exchange emulated with a
    concatenation of the ranks' touched-row lists (step 2): one reference-semantics step on the concatenated batch, item replicas
    bit-identical."""
    from elliot_amd import parallel
    rs = np.random.RandomState(33)
    U, I, F, B, G = 701, 400, 64, 3000, 2
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    d = ctx.device
    rng = [parallel.user_range(U, r, G) for r in range(G)]
    bes = [parallel.HipUserShardBackend(ctx, Gu[lo:hi], Gi, Bi, optimizer="adam_tf_dense") for lo, hi in rng]
    orc = ob.BPRMFBatchOracle(Gu, Gi, Bi, lr, l_w, l_b)
    for step in range(3):
        batches = [(rs.randint(lo, hi, B), rs.randint(0, 25, B), rs.randint(0, I, B)) for lo, hi in rng]    # hot positives
        for be, (lo, hi), (u, i, j) in zip(bes, rng, batches):
            be.grads(torch.from_numpy((u - lo).astype(np.int32)).to(d), torch.from_numpy(i.astype(np.int32)).to(d),
                     torch.from_numpy(j.astype(np.int32)).to(d), l_w, l_b)
        if step == 2:
            # the row-sparse exchange (ShardedBprmfByUser, item_exchange="rows"): every rank's touched (item id, row, bias) records,
            # the shorter list padded, concatenated in rank order = the all-gather; el_rows_segment_sum on every rank
            lists = [be.touched_item_rows(torch.from_numpy(b[1].astype(np.int32)).to(d), torch.from_numpy(b[2].astype(np.int32)).to(d))
                     for be, b in zip(bes, batches)]
            n_max = max(int(l[0].shape[0]) for l in lists)
            padded = []
            for ids, rows, bias in lists:
                pad = n_max - int(ids.shape[0])
                padded.append((torch.cat([ids, ids[:1].expand(pad)]), torch.cat([rows, torch.zeros((pad, F), device=d)]),
                               torch.cat([bias, torch.zeros(pad, device=d)])))
            gathered = tuple(torch.cat([p[x] for p in padded]).contiguous() for x in range(3))
            for be in bes:
                be.set_item_grads(*gathered)
        else:
            for gs in zip(*[be.item_grads() for be in bes]):         # the all-reduce
                tot = gs[0] + gs[1]
                for g in gs:
                    g.copy_(tot)
        loss = 0.0
        for be in bes:
            if step == 1:
                be.apply(lr)                                         # one call ...
            else:
                be.begin_step()                                      # ... or the split form ShardedBprmfByUser overlaps
                be.apply_users(lr)                                   # with the collective: same update
                be.apply_items(lr)
            loss += be.state.pop_loss()
        cu, ci, cj = (np.concatenate([b[x] for b in batches]) for x in range(3))
        exp = orc.train_step((cu, ci, cj))
        assert abs(loss - exp) <= 1e-4 * abs(exp), (step, loss, exp)
        assert torch.equal(bes[0].state.Gi, bes[1].state.Gi) and torch.equal(bes[0].state.Bi, bes[1].state.Bi)
        assert (np.abs(cpu(bes[0].state.Gi) - orc.Gi) > 2e-5).mean() < 2e-4
        assert (np.abs(cpu(bes[0].state.Bi) - orc.Bi) > 2e-5).mean() < 2e-3
        for be, (lo, hi) in zip(bes, rng):
            assert (np.abs(cpu(be.state.Gu) - orc.Gu[lo:hi]) > 2e-5).mean() < 2e-4
            assert not cpu(be.state.gGu).any() and not cpu(be.state.gGi).any()


# ---------------------------------------------------------------------------------- exact MT19937 replay
def test_mt19937_replay_sampler_equals_reference_stream(ctx, golden):
    """The reference's own custom_sampler.Sampler output (tests/golden/sampler_ref.npz, seed 42, batches of 512)."""
    g = golden("sampler_ref.npz")
    U, I = int(g["n_users"]), int(g["n_items"])
    lp, li = g["lists_indptr"], g["lists_items"]
    lists = [li[lp[u]:lp[u + 1]].tolist() for u in range(U)]
    pos = ops.DeviceCSR(g["indptr"], g["indices"], I, ctx.device)
    s = ops.MtReplaySampler(ctx, lists, pos, seed=42)
    n = g["u"].shape[0]
    got = [[], [], []]
    for start in range(0, n, 512):                      # stateful across calls, like Sampler.step batches
        b = s.sample(min(512, n - start))
        for x in range(3):
            got[x].append(cpu(b[x]))
    assert np.array_equal(np.concatenate(got[0]), g["u"])
    assert np.array_equal(np.concatenate(got[1]), g["i"])
    assert np.array_equal(np.concatenate(got[2]), g["j"])
    # generator state afterwards == NumPy's own state after the same number of draws is implied by the stream
    # continuing correctly over 12 calls; one more draw-by-draw check against the CPU restatement:
    o = osampler.RefSampler(lists, I, seed=42)
    for _ in o.step(n, 512):
        pass
    nxt = s.sample(100)
    exp = np.array([o.sample() for _ in range(100)])
    assert np.array_equal(cpu(nxt[0]), exp[:, 0]) and np.array_equal(cpu(nxt[2]), exp[:, 2])


# ---------------------------------------------------------------------------------- epoch loop inside the library
@pytest.mark.parametrize("B,algo,exact,timed", [(4096, "sorted", True, False), (512, "auto", False, False),
                                                (300, "atomic", False, False), (512, "auto", False, True)])
def test_train_loop_equals_per_batch_calls(ctx, B, algo, exact, timed):
    """el_bprmf_train_loop = sampler.step + train_step per batch (same Philox offsets, same kernels, short last batch).
    Small batches replay the captured hipGraph (per-step scalars in device memory); with per-kernel timing switched on the
    same loop runs eagerly (timed=True); large batches take the sorted path eagerly."""
    from elliot_amd.synthetic import zipf_csr
    rs = np.random.RandomState(5)
    U, I, F = 3000, 900, 32
    indptr, indices = zipf_csr(U, I, mean_log=2.0, sigma_log=0.6, dmin=1, dmax=80, seed=2)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    events, lr, l_w, l_b = 5 * B + B // 3, 0.003, 0.05, 0.001
    a = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense")
    b = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense")
    for epoch in range(2):
        first = 1000 + epoch * events
        for start in range(0, events, B):
            n = min(B, events - start)
            u, i, j = ops.bpr_sample(ctx, pos, n, seed=7, first_sample=first + start)
            a.train_step(u, i, j, lr, l_w, l_b, algo=algo)
        ctx.timing(timed)
        steps = b.train_loop(pos, events, B, 7, first, lr, l_w, l_b, algo=algo)
        if timed:
            names = set(ctx.timing_report())
            assert "k_bprmf_fwd_bwd" in names and "k_adam_dense3" in names, names
        ctx.timing(False)
        assert steps == 6 and a.step == b.step
        la, lb = a.pop_loss(), b.pop_loss()
        assert abs(la - lb) <= (1e-8 if exact else 1e-6) * abs(la), (la, lb)     # hot rows that cross chunks: atomics order
        for name in ("Gu", "Gi", "Bi", "mGu", "vGi"):
            x, y = cpu(getattr(a, name)), cpu(getattr(b, name))
            if exact:
                assert np.abs(x - y).max() < 1e-7, name          # chunk-crossing hot rows: atomics order only
            else:
                assert np.abs(x - y).max() < 1e-5, name
    with pytest.raises(ValueError):
        b.train_loop(ops.DeviceCSR(indptr[:11], indices[:indptr[10]], I, ctx.device), events, B, 7, 0, lr, l_w, l_b)


def test_sampler_records_give_the_same_triplets(ctx):
    """el_bpr_sample_meta (one 64-byte record per user: row start, length, 384-bit membership signature) == el_bpr_sample, bit
    for bit, incl. heavy rows whose signature is full, rows of one item, the sharded negative range and the epoch loop."""
    from elliot_amd.synthetic import zipf_csr
    indptr, indices = zipf_csr(5000, 1200, mean_log=2.2, sigma_log=1.3, dmin=1, dmax=1100, seed=6)
    pos = ops.DeviceCSR(indptr, indices, 1200, ctx.device)
    for kw in (dict(), dict(item_lo=300, item_hi=900)):
        a = ops.bpr_sample(ctx, pos, 200000, seed=11, first_sample=12345, use_meta=False, **kw)
        b = ops.bpr_sample(ctx, pos, 200000, seed=11, first_sample=12345, use_meta=True, **kw)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    meta = ops.sampler_meta(ctx, pos)
    assert meta.data_ptr() % 64 == 0 and meta.numel() == 64 * 5000
    rec = meta.view(torch.int32).view(5000, 16).cpu().numpy()
    assert np.array_equal(rec[:, 2], np.diff(indptr))                      # row lengths
    lo = rec[:, 0].astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(lo | (rec[:, 1].astype(np.int64) << 32), indptr[:-1])
    bits = np.unpackbits(rec[:, 4:].copy().view(np.uint8), axis=1, bitorder="little").sum(1)
    assert (bits <= np.minimum(np.diff(indptr), 384)).all() and bits[np.diff(indptr) > 0].min() >= 1


def test_presorted_gradients_equal_the_one_call_form(ctx):
    """el_bprmf_presort + el_bprmf_grads_presorted == el_bprmf_grads (the split lets a multi-GPU step order the next batch under
    its collective); the workspace is reused batch after batch."""
    from elliot_amd import parallel
    rs = np.random.RandomState(44)
    U, I, F, B = 900, 500, 32, 5000
    Gu, Gi, Bi = _setup(rs, U, I, F)
    a = parallel.HipUserShardBackend(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense")
    b = parallel.HipUserShardBackend(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense")
    d = ctx.device
    for step in range(3):
        u, i, j = (torch.from_numpy(x.astype(np.int32)).to(d) for x in (rs.randint(0, U, B), rs.randint(0, 30, B), rs.randint(0, I, B)))
        a.grads(u, i, j, 0.1, 0.001)
        b.presort(u, i, j)
        b.grads(u, i, j, 0.1, 0.001, presorted=True)
        for name in ("gGu", "gGi", "gBi"):
            x, y = cpu(getattr(a.state, name)), cpu(getattr(b.state, name))
            assert np.abs(x - y).max() <= 1e-5 * max(1.0, np.abs(x).max()), (step, name)       # hot rows: atomics order only
        la, lb = a.state.pop_loss(), b.state.pop_loss()
        assert abs(la - lb) <= 1e-8 * abs(la), (la, lb)
        a.apply(0.01)
        b.apply(0.01)
    assert np.abs(cpu(a.state.Gi) - cpu(b.state.Gi)).max() < 1e-5


def test_pipelined_step_equals_the_sequential_step(ctx):
    """bench.py's software pipeline -- the batch of step t+1 drawn AND ordered (sampler, prep, radix sort) on a side stream while
    step t's segment kernels and optimiser pass run, the step itself on a high-priority stream -- against the plain sequence of
    train_step calls on the same Philox stream: same triplets, same losses, same weights (hot rows: atomics order only)."""
    from elliot_amd.pipeline import PrefetchSampler
    from elliot_amd.synthetic import zipf_csr
    rs = np.random.RandomState(91)
    U, I, F, B, steps = 20000, 3000, 64, 8192, 7
    indptr, indices = zipf_csr(U, I, mean_log=2.5, sigma_log=0.8, dmin=2, dmax=200, seed=5)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    a = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True)
    b = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True)
    sampler = PrefetchSampler(ctx, pos, B, 42, enabled=True, presort_state=b)
    hi = torch.cuda.Stream(device=ctx.device, priority=-1)
    hi.wait_stream(torch.cuda.current_stream())
    la, lb = [], []
    for s in range(steps):
        t = ops.bpr_sample(ctx, pos, B, seed=42, first_sample=s * B)
        a.train_step(t[0], t[1], t[2], lr, l_w, l_b, algo="sorted")
        la.append(a.pop_loss())
        with torch.cuda.stream(hi):
            tb, buf = sampler.next()
            b.train_step_presorted(tb[0], tb[1], tb[2], lr, l_w, l_b, sampler.ws[buf])
            sampler.release(buf)
        torch.cuda.current_stream().wait_stream(hi)
        assert all(torch.equal(x, y) for x, y in zip(t, tb)), s          # the look-ahead drew the batch of THIS step
        lb.append(b.pop_loss())
    torch.cuda.synchronize()
    for s, (x, y) in enumerate(zip(la, lb)):
        assert abs(x - y) <= 1e-7 * abs(x), (s, x, y)
    for name in ("Gu", "Gi", "Bi"):
        x, y = cpu(getattr(a, name)), cpu(getattr(b, name))
        assert (np.abs(x - y) > 2e-6).mean() < 1e-4 and np.abs(x - y).max() < 5 * lr, name


@pytest.mark.parametrize("F,U", [(128, 30000), (64, 5001), (256, 9000), (16, 777), (384, 2000)])
def test_fused_user_side_equals_the_two_kernel_form_bit_for_bit(ctx, F, U):
    """el_bprmf_state.Gu_next: user segments + Keras Adam over every user row in ONE kernel, the new rows written to the second
    table (ping-pong).  Same operations in the same order as k_bpr_user_seg + k_adam_rows -- the user table, its Adam slots and the
    item side come out BIT-identical over several steps (odd and even numbers of swaps; users without triplets, users with many; a
    row count that is not a multiple of the rows a lane group owns); the loss differs by the order of its fp32 partial sums only.
    Also through train_loop (the library swaps the pair per batch) and train_step_presorted."""
    from elliot_amd.synthetic import zipf_csr
    rs = np.random.RandomState(F + U)
    I, B = 1500, 8192
    indptr, indices = zipf_csr(U, I, mean_log=2.0, sigma_log=0.9, dmin=1, dmax=150, seed=F)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    a = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, fused_user_step=False)
    b = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=False, fused_item_step=False)
    assert b.fused and not a.fused and b.Gu_next is not None and not b.deferred and not b.item_fused
    for s in range(5):
        n = B if s != 3 else 2500                                  # a short batch: most rows have no triplet
        t = ops.bpr_sample(ctx, pos, n, seed=7, first_sample=s * B)
        a.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        if s % 2:
            ws = b.sort_workspace(n)
            b.presort(t[0], t[1], t[2], ws)
            b.train_step_presorted(t[0], t[1], t[2], lr, l_w, l_b, ws)
        else:
            b.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        la, lb = a.pop_loss(), b.pop_loss()
        assert abs(la - lb) <= 2e-6 * abs(la), (s, la, lb)
        for name in ("Gu", "mGu", "vGu", "Gi", "mGi", "vGi", "Bi"):
            x, y = getattr(a, name), getattr(b, name)
            if s == 0 and name in ("Gu", "mGu", "vGu"):
                # same inputs -> the same bits.  (From the second step on the INPUTS differ in the last bit: the item-side kernel, the
                # same in both forms, combines the chunk-crossing segments of hot items with float atomics whose order varies
                # from launch to launch.)
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (s, name)
            else:                                                  # (Adam's m / (sqrt(v) + eps) amplifies a last-bit input difference where v ~ 0)
                err = (x - y).abs()
                assert float((err > 2e-6).float().mean()) < 1e-4 and float(err.max()) < 5 * lr, (s, name, float(err.max()))
    # the epoch loop inside the library: 3 batches (an odd number of swaps), same Philox stream in both forms
    a.train_loop(pos, 3 * B, B, 11, 0, lr, l_w, l_b)
    b.train_loop(pos, 3 * B, B, 11, 0, lr, l_w, l_b)
    la, lb = a.pop_loss(), b.pop_loss()
    assert abs(la - lb) <= 1e-5 * abs(la)
    assert float(((a.Gu - b.Gu).abs() > 4e-6).float().mean()) < 1e-4 and float((a.vGu - b.vGu).abs().max()) <= 1e-7
    # grads() / apply() on the fused state take the two-kernel form and leave the pair alone: from equal tables, equal bits
    b.Gu.copy_(a.Gu), b.mGu.copy_(a.mGu), b.vGu.copy_(a.vGu), b.Gi.copy_(a.Gi), b.mGi.copy_(a.mGi), b.vGi.copy_(a.vGi)
    b.Bi.copy_(a.Bi), b.mBi.copy_(a.mBi), b.vBi.copy_(a.vBi)
    t = ops.bpr_sample(ctx, pos, B, seed=9, first_sample=0)
    for st in (a, b):
        st.grads(t[0], t[1], t[2], l_w, l_b)
        st.apply(lr)
    assert torch.equal(a.Gu.view(torch.int32), b.Gu.view(torch.int32))


@pytest.mark.parametrize("F,U,hist", [(128, 5003, None), (64, 1024, 8), (256, 2001, 4)])
def test_deferred_decay_of_the_user_table_equals_the_every_row_pass_bit_for_bit(ctx, F, U, hist, monkeypatch, lib_option):
    """el_bprmf_state.Gu_last: a step moves only the user rows of its batch, the gradient-free Adam steps of every other row are
    replayed when a batch next contains the user or when the table is read.  Against the every-row fused form on the same batches:
    theta, m, v of the user table BIT-identical at every read -- after stretches of steps that leave most users untouched (batches
    drawn for a tenth of the users), after a read in the middle, through train_step, train_step_presorted and train_loop, with a
    4- / 8-step lr ring whose half-way flushes kick in, and across a grads() + apply() pair (the every-row pass on a deferred
    state).  The item side is the same code in both; the `ichunk` option makes its summation order fixed (one lane group walks the whole
    sorted batch: no chunk-crossing atomics), so both runs see identical inputs at every step."""
    from elliot_amd.synthetic import zipf_csr
    lib_option("ichunk", 1 << 20)
    if hist:
        monkeypatch.setattr(ops.BprmfDeviceState, "_LR_HIST", hist)
    rs = np.random.RandomState(F + U)
    I, B = 700, 4096
    indptr, indices = zipf_csr(U, I, mean_log=2.0, sigma_log=0.9, dmin=1, dmax=150, seed=F)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    # positives of the first tenth of the users only: batches drawn from it leave the other rows waiting
    cut = int(indptr[U // 10])
    ip2 = np.minimum(indptr, cut)
    few = ops.DeviceCSR(ip2, indices[:cut].copy(), I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    a = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=False)
    b = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=True)
    assert a.fused and not a.deferred and b.deferred and b.Gu_next is None

    def same(tag):
        b.sync()
        for name in ("Gu", "mGu", "vGu", "Gi", "mGi", "vGi", "Bi"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (tag, name, int((x != y).sum()), float((x - y).abs().max()))

    for s in range(14):
        src = pos if s in (0, 6, 13) else few
        n = B if s != 3 else 600
        t = ops.bpr_sample(ctx, src, n, seed=7, first_sample=s * B)
        for st in (a, b):
            if s % 3 == 1:
                ws = st.sort_workspace(n)
                st.presort(t[0], t[1], t[2], ws)
                st.train_step_presorted(t[0], t[1], t[2], lr, l_w, l_b, ws)
            else:
                st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        la, lb = a.pop_loss(), b.pop_loss()
        assert abs(la - lb) <= 2e-6 * abs(la), (s, la, lb)
        if s in (0, 5, 12, 13):
            same(s)
    # the table read through the property is current without an explicit sync
    a.train_loop(few, 5 * B, B, 11, 0, lr, l_w, l_b)
    b.train_loop(few, 5 * B, B, 11, 0, lr, l_w, l_b)
    assert b._pending
    assert torch.equal(a.Gu.view(torch.int32), b.Gu.view(torch.int32)) and not b._pending
    same("loop")
    # grads() + apply(): the every-row two-kernel form on both; the deferred state carries on afterwards
    t = ops.bpr_sample(ctx, pos, B, seed=9, first_sample=0)
    for st in (a, b):
        st.grads(t[0], t[1], t[2], l_w, l_b)
        st.apply(lr)
    same("apply")
    t = ops.bpr_sample(ctx, few, B, seed=10, first_sample=0)
    for st in (a, b):
        st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
    same("after apply")


@pytest.mark.parametrize("F,I,defer,hist", [(128, 3001, False, None), (64, 700, True, 8), (256, 5000, True, None), (16, 901, True, 4),
                                            (128, 2000, None, None)])
def test_fused_item_side_equals_the_two_pass_form_bit_for_bit(ctx, F, I, defer, hist, monkeypatch, lib_option):
    """el_bprmf_state.Gi_last: the item segments take Keras' Adam step on their rows in place (no dense gradient table written,
    re-read and cleared); the rows a batch leaves alone are replayed at the end of every step (item_deferred=False) or when a batch
    next contains the item / the table is read (item_deferred=True).  Against the two-pass form (k_bpr_item_seg -> gGi ->
    k_adam_dense_pair) on the same batches: Gi, Bi and their Adam slots BIT-identical at every read, the user table too (it reads
    the item rows) -- through train_step, train_step_presorted, train_loop, a grads() + apply() pair in the middle, stretches of
    batches whose positives AND negatives stay inside an eighth of the catalogue (rows wait up to 9 steps), a 4- / 8-entry lr ring
    whose half-way flushes kick in.  the `ichunk` option pins the summation order of both forms (one lane group walks the whole sorted batch);
    segments cut by chunk boundaries are exercised by the next test.  defer=None: the state decides by the batch size (2 B <= I)."""
    lib_option("ichunk", 1 << 20)
    if hist:
        monkeypatch.setattr(ops.BprmfDeviceState, "_LR_HIST", hist)
    rs = np.random.RandomState(F + I)
    U, B = 4000, (4096 if defer is not None else 512)
    indptr, indices = zipf_csr(U, I, mean_log=2.0, sigma_log=0.9, dmin=1, dmax=150, seed=F)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    # positives inside the first eighth of the catalogue only; negatives restricted to the same range by the sampler
    cutI = max(I // 8, 8)
    keep = indices < cutI
    ip2 = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), indptr[:-1]) * (np.diff(indptr) > 0))]).astype(np.int64)
    few = ops.DeviceCSR(ip2, indices[keep].astype(np.int32), I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    a = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=False, fused_item_step=False)
    b = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=False, fused_item_step=True,
                             item_deferred=defer)
    assert not a.item_fused and b.item_fused and b.fused

    def same(tag):
        b.sync()
        assert not b._pending_items
        for name in ("Gi", "mGi", "vGi", "Bi", "mBi", "vBi", "Gu", "mGu", "vGu"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (tag, name, int((x != y).sum()), float((x - y).abs().max()))
        assert float(b.gGi.abs().max()) == 0.0 and float(b.gBi.abs().max()) == 0.0
        assert int(b.Gi_last.min()) == b.step and int(b.Gi_last.max()) == b.step

    for s in range(14):
        narrow = s not in (0, 6, 13)
        n = B if s != 3 else 600
        t = ops.bpr_sample(ctx, few if narrow else pos, n, seed=7, first_sample=s * B, item_lo=0, item_hi=cutI if narrow else I)
        for st in (a, b):
            if s % 3 == 1:
                ws = st.sort_workspace(n)
                st.presort(t[0], t[1], t[2], ws)
                st.train_step_presorted(t[0], t[1], t[2], lr, l_w, l_b, ws)
            else:
                st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        la, lb = a.pop_loss(), b.pop_loss()
        assert abs(la - lb) <= 2e-6 * abs(la), (s, la, lb)
        if s in (0, 5, 12, 13):
            same(s)
    if defer is None:
        assert b.item_deferred == (2 * B <= I)
    elif defer:
        assert b.item_deferred
    a.train_loop(few, 5 * B, B, 11, 0, lr, l_w, l_b)
    b.train_loop(few, 5 * B, B, 11, 0, lr, l_w, l_b)
    assert b._pending_items == bool(b.item_deferred)
    assert torch.equal(a.Bi.view(torch.int32), b.Bi.view(torch.int32)) and not b._pending_items
    same("loop")
    t = ops.bpr_sample(ctx, pos, B, seed=9, first_sample=0)
    for st in (a, b):
        st.grads(t[0], t[1], t[2], l_w, l_b)
        st.apply(lr)
    same("apply")
    t = ops.bpr_sample(ctx, few, B, seed=10, first_sample=0, item_lo=0, item_hi=cutI)
    for st in (a, b):
        st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
    same("after apply")


@pytest.mark.parametrize("chunk", [16, 64])
@pytest.mark.parametrize("defer", [False, True])
def test_fused_item_side_with_segments_cut_by_chunk_boundaries(ctx, chunk, defer, lib_option):
    """Zipf catalogue, small chunks: the popular items' segments span many lane groups, each of which leaves a partial row;
    k_seg_combine / k_seg_combine_long add them in chunk order and take the Adam step on the row (fused form) or store the gradient
    row (two-pass form), so the two forms agree bit for bit in every table; every row is stamped."""
    lib_option("ichunk", chunk)
    F, U, I, B = 128, 3000, 1200, 8192
    rs = np.random.RandomState(chunk)
    indptr, indices = zipf_csr(U, I, mean_log=2.5, sigma_log=0.9, dmin=1, dmax=200, seed=5)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    a = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=False, fused_item_step=False)
    b = ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=False, fused_item_step=True,
                             item_deferred=defer)
    for s in range(6):
        t = ops.bpr_sample(ctx, pos, B, seed=3, first_sample=s * B)
        for st in (a, b):
            st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
    b.sync()
    assert int(b.Gi_last.min()) == 6 and int(b.Gi_last.max()) == 6
    assert ops.deterministic_item_sums(ctx)
    for name in ("Gi", "mGi", "vGi", "Bi", "mBi", "vBi", "Gu", "mGu", "vGu"):
        x, y = getattr(a, name), getattr(b, name)
        # the partial rows of a cut segment are added in chunk order by k_seg_combine in BOTH forms: no atomics, the same bits
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, int((x != y).sum()), float((x - y).abs().max()))
    la, lb = a.pop_loss(), b.pop_loss()
    assert abs(la - lb) <= 1e-5 * abs(la)


@pytest.mark.parametrize("F,I", [(128, 900), (64, 5000), (256, 300), (20, 700)])
def test_sorted_step_is_deterministic_and_equals_the_oracle_on_a_zipf_catalogue(ctx, F, I):
    """Default chunking, a Zipf catalogue whose hottest items own thousands of the 2 B sorted positions (segments cut into dozens of
    partials, lists of hundreds of cut rows): two runs from the same tables on the same batches give the same bits in every table --
    k_seg_combine adds a cut segment's partials in chunk order -- in the fused + deferred form and in the two-pass form, the two
    forms agree bit for bit with each other, and the result is the oracle's to fp32 re-association accuracy (F = 20: rows of 80 bytes on
    eight-lane groups; F = 256: 64-lane groups, four per combine workgroup)."""
    rs = np.random.RandomState(F)
    U, B = 6000, 16384
    indptr, indices = zipf_csr(U, I, mean_log=2.5, sigma_log=0.9, dmin=1, dmax=min(200, I // 2), seed=F + 1)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    mk = lambda **kw: ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, **kw)
    runs = [mk(), mk(), mk(deferred=False, fused_user_step=False, fused_item_step=False)]
    orc = ob.BPRMFBatchOracle(Gu, Gi, Bi, lr, l_w, l_b)
    for s in range(5):
        t = ops.bpr_sample(ctx, pos, B, seed=3, first_sample=s * B)
        if s == 0:
            cnt = torch.bincount(torch.cat([t[1], t[2]]).long(), minlength=I)
            assert int(cnt.max()) > 300                            # a segment of hundreds of positions: dozens of 16-position partials
        for st in runs:
            st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        orc.train_step(tuple(cpu(x) for x in t))
    for st in runs:
        st.sync()
    for name in ("Gu", "mGu", "vGu", "Gi", "mGi", "vGi", "Bi", "mBi", "vBi"):
        x0, x1, x2 = (getattr(st, name) for st in runs)
        assert torch.equal(x0.view(torch.int32), x1.view(torch.int32)), ("run to run", name)
        assert torch.equal(x0.view(torch.int32), x2.view(torch.int32)), ("fused vs two-pass", name, int((x0 != x2).sum()))
    for name in ("Gu", "Gi", "Bi"):
        err = np.abs(cpu(getattr(runs[0], name)) - getattr(orc, name))
        assert (err > 2e-5).mean() < 2e-3 and err.max() < 3 * lr, (name, float(err.max()))


@pytest.mark.parametrize("F,U,I,item_defer", [(128, 5003, 700, False), (64, 1500, 4000, True), (256, 2001, 3000, True)])
def test_series_replay_matches_the_step_by_step_replay(ctx, F, U, I, item_defer, lib_option):
    """el_bprmf_state.replay_series: a waiting row brought forward in closed form (four row-level sums over the lr_t history, O(1) per
    element) against the step-by-step replay (the bits of Keras' every-row pass) on the same batches -- stretches of batches that leave
    nine users in ten (and seven items in eight) waiting, gaps of 1 .. 13 steps, a sync in the middle, the lr ring's half-way flush.
    Not the same rounding sequence: theta within 1e-6 of the row's scale on all but isolated elements, m and v to 1e-4 of the table scale
    (median 1e-6; the two runs' gradients drift apart at that level over 70 steps), the
    loss of every step to 1e-6 -- the distance the fp32 step-by-step form itself keeps from the exact-arithmetic recurrence
    (scripts/exp/series_check.py)."""
    from elliot_amd.synthetic import zipf_csr
    lib_option("ichunk", 1 << 20)                               # one summation order on the item side: the two runs see the same gradients
    rs = np.random.RandomState(F + U)
    B = 4096
    indptr, indices = zipf_csr(U, I, mean_log=2.0, sigma_log=0.9, dmin=1, dmax=150, seed=F)
    pos = ops.DeviceCSR(indptr, indices, I, ctx.device)
    cutI = max(I // 8, 8)
    cutU = U // 10
    keep = (indices < cutI) & (np.repeat(np.arange(U), np.diff(indptr)) < cutU)
    ip2 = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(U), np.diff(indptr))[keep], minlength=U))]).astype(np.int64)
    few = ops.DeviceCSR(ip2, indices[keep].astype(np.int32), I, ctx.device)
    Gu, Gi, Bi = _setup(rs, U, I, F)
    lr, l_w, l_b = 0.01, 0.1, 0.001
    mk = lambda mode: ops.BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=True, deferred=True,
                                           fused_item_step=True, item_deferred=item_defer, replay=mode)
    a, b = mk("exact"), mk("series")
    assert a.deferred and b.deferred and b._c.replay_series == 1 and a._c.replay_series == 0

    def close(tag):
        a.sync(), b.sync()
        for name in ("Gu", "Gi", "Bi"):
            x, y = getattr(a, name), getattr(b, name)
            err = (x - y).abs()
            assert float((err > 1e-6 * (1 + x.abs())).float().mean()) < 1e-4 and float(err.max()) < 5 * lr, (tag, name, float(err.max()))
        for name in ("mGu", "vGu", "mGi", "vGi", "mBi", "vBi"):
            x, y = getattr(a, name), getattr(b, name)
            rel = (x - y).abs() / (x.abs() + float(x.abs().mean()) + 1e-30)     # (an element near zero is a cancelled sum: table scale)
            assert float((rel > 1e-4).float().mean()) < 1e-4 and float(rel.median()) < 1e-6, (tag, name, float(rel.max()))

    for s in range(30):
        src = pos if s in (0, 14, 29) else few
        t = ops.bpr_sample(ctx, src, B, seed=7, first_sample=s * B, item_lo=0, item_hi=I if src is pos else cutI)
        for st in (a, b):
            if s % 3 == 1:
                ws = st.sort_workspace(B)
                st.presort(t[0], t[1], t[2], ws)
                st.train_step_presorted(t[0], t[1], t[2], lr, l_w, l_b, ws)
            else:
                st.train_step(t[0], t[1], t[2], lr, l_w, l_b)
        la, lb = a.pop_loss(), b.pop_loss()
        assert abs(la - lb) <= 1e-6 * abs(la), (s, la, lb)
        if s in (0, 9, 14):
            close(s)
    close("end")
    # 40 more steps inside the library's epoch loop: nine rows in ten wait for all of them
    for st in (a, b):
        st.train_loop(few, 40 * B, B, 11, 0, lr, l_w, l_b)
    close("loop")


def test_packed_replay_arithmetic_is_exact(ctx):
    """The replay kernels of the deferred decay take the gradient-free Adam step on packed fp32 instructions (el_common.h:
    el_adam_replay2): a square root by v_rsq + fma refinements and a division by v_rcp + fma refinements instead of the compiler's
    IEEE expansions -- half the issue slots, and the SAME bits: the square root is compared with sqrtf() for EVERY float of the range
    the guard admits (1.6e9 inputs, exhaustive), the division on 2^31 pairs (random and near-tie mantissas over the guard's
    exponent range) with `/`, the whole step on 2^31 random states with el_adam_elem."""
    import ctypes as C
    out = torch.zeros(3, dtype=torch.int64, device=ctx.device)
    ops.check(ctx.lib.el_selftest_replay_math(ctx.handle, ctx.stream(), 1 << 31, C.c_void_p(out.data_ptr())), "el_selftest_replay_math")
    assert out.tolist() == [0, 0, 0], out.tolist()
