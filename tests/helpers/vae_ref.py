"""What tests/test_gpu_vae_edges.py holds the Mult-VAE / Mult-DAE kernels (elliot_amd/csrc/el_vae.hip) to, restated in NumPy:
  make_batch        a binary train matrix and a list of batch rows in which chosen items occur in a prescribed number of batch rows
  drop_mask         the dropout mask of vae_drop_scale (Philox4x32-10 keyed by user, item, step and seed), vectorised
  ref_grads         loss and the eight gradient tensors of oracle/multi_vae.py / oracle/multi_dae.py in the device's layout
  adam_f32          TF's dense ApplyAdam in fp32, one IEEE operation at a time in the kernel's order
  RUNS / run_inputs the inputs of every GPU case, shared with tests/test_vae_ref_host.py (which checks them without a GPU)
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import multi_dae as od
from oracle import multi_vae as ov

f32 = np.float32
ORDER = ("W1", "b1", "Wmv", "bmv", "W3", "b3", "W4", "b4")                # ops.VaeDeviceState.ORDER
LOSS_RTOL = 1e-4                 # the project's bound on the loss
GRAD_RTOL = 2e-5                 # ... and on a gradient tensor, relative to the largest |entry| of its reference
W1_LIGHT = 16                    # el_vae.hip: an item in more batch rows than this is summed by k_vae_w1_rows


# ---- batches with prescribed in-batch item counts ----------------------------------------------------------------------------------------
def make_batch(n_users, n_items, B, density, seed, every=(), at=None, empty=(), dup=None):
    """A binary [n_users, n_items] train matrix and B batch rows (users) such that, counted over the batch POSITIONS,
      every     items present in every batch row that has any item
      at        {item: batch positions}: the item is in exactly these rows (an empty list: in none)
      empty     batch positions whose user has no train item at all
      dup       (b1, b2): both positions hold the same user
    and every other (position, item) is present with probability `density`.  Users outside the batch get random rows too."""
    at = {int(k): np.asarray(v, dtype=np.int64) for k, v in (at or {}).items()}
    rs = np.random.RandomState(seed)
    P = rs.rand(B, n_items) < density
    for item, pos in at.items():
        P[:, item] = False
        P[pos, item] = True
    P[:, list(every)] = True
    P[list(empty)] = False
    if dup is not None:
        b1, b2 = dup
        for item, pos in at.items():
            assert (b1 in pos) == (b2 in pos), "a prescribed item must be in both positions of the repeated user, or in neither"
        assert (b1 in empty) == (b2 in empty)
        P[b2] = P[b1]
    n_distinct = B - (dup is not None)
    assert n_users >= n_distinct
    users = rs.permutation(n_users)
    rows = np.empty(B, np.int32)
    free = [b for b in range(B) if dup is None or b != dup[1]]
    rows[free] = users[:n_distinct]
    if dup is not None:
        rows[dup[1]] = rows[dup[0]]
    X = (rs.rand(n_users, n_items) < density).astype(f32)
    X[rows] = P.astype(f32)
    indptr = np.concatenate([[0], np.cumsum((X != 0).sum(1))]).astype(np.int64)
    indices = np.nonzero(X)[1].astype(np.int32)                            # row-major: sorted within a row
    return SimpleNamespace(X=X, rows=rows, indptr=indptr, indices=indices, n_users=n_users, n_items=n_items)


def batch_counts(indptr, indices, rows, n_items):
    """Number of batch rows each item occurs in, from the CSR arrays the kernels read."""
    got = np.zeros(n_items, np.int64)
    for u in rows:
        got += np.bincount(indices[indptr[u]:indptr[u + 1]], minlength=n_items)
    return got


# ---- dropout -----------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (oracle.sampler.philox4x32_10, which takes Python ints, is the scalar original)."""
    u64, lo32 = np.uint64, np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=u64) & lo32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = u64(int(k0) & 0xFFFFFFFF), u64(int(k1) & 0xFFFFFFFF)
    M0, M1, W0, W1, s32 = u64(0xD2511F53), u64(0xCD9E8D57), u64(0x9E3779B9), u64(0xBB67AE85), u64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                                      # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & lo32, p1 & lo32, ((p0 >> s32) ^ c3 ^ k1) & lo32, p0 & lo32
        k0, k1 = (k0 + W0) & lo32, (k1 + W1) & lo32
    return c0, c1, c2, c3


def drop_mask(users, n_items, rate, seed, step):
    """[len(users), n_items] fp32 of {0, 1/(1-rate)}: vae_drop_scale for every (user, item); all ones at rate 0."""
    users = np.asarray(users, dtype=np.int64)
    if rate <= 0:
        return np.ones((len(users), n_items), f32)
    x = philox4x32_10(users[:, None], np.arange(n_items)[None, :], step, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    uni = (x >> np.uint64(8)).astype(f32) * f32(1.0 / 16777216.0)
    return np.where(uni < f32(rate), f32(0.0), f32(1.0) / (f32(1.0) - f32(rate))).astype(f32)


# ---- loss and gradients ------------------------------------------------------------------------------------------------------------------
def init_weights(n_items, hidden, latent, dae, seed):
    """Glorot kernels, small random biases (zero biases would hide a bias that is never added)."""
    w = (od if dae else ov).init_weights(n_items, hidden, latent, seed)
    rs = np.random.RandomState(seed + 1)
    for k in w:
        if k.startswith("b"):
            w[k] = rs.normal(scale=0.01, size=w[k].shape).astype(f32)
    return w


def ref_grads(w, X, eps, anneal, drop, n_global, dae, dtype=np.float64):
    """(loss, {name: gradient}) of the batch X [B, I] in the layout of VaeDeviceState.g (the mean and log-variance heads side by side).
    The oracle takes its means over the B rows it is given, the kernels over n_global: loss, KL and every gradient are linear in 1/B,
    so all of them are scaled by B / n_global.  eps None = zeros (what the kernel samples without eps)."""
    B = X.shape[0]
    if dae:
        c = od.forward(w, X, drop, dtype=dtype)
        loss, g = od.loss_from(c), od.gradients(w, c)
        out = {"W1": g["W1"], "b1": g["b1"], "Wmv": g["Wm"], "bmv": g["bm"], "W3": g["W3"], "b3": g["b3"], "W4": g["W4"], "b4": g["b4"]}
    else:
        L = w["Wm"].shape[1]
        c = ov.forward(w, X, np.zeros((B, L), f32) if eps is None else eps, drop, dtype=dtype)
        loss, g = ov.loss_from(c, dtype(anneal)), ov.gradients(w, c, dtype(anneal))
        out = {"W1": g["W1"], "b1": g["b1"], "Wmv": np.concatenate([g["Wm"], g["Wv"]], axis=1), "bmv": np.concatenate([g["bm"], g["bv"]]),
               "W3": g["W3"], "b3": g["b3"], "W4": g["W4"], "b4": g["b4"]}
    s = dtype(B) / dtype(n_global)
    return loss * s, {k: v * s for k, v in out.items()}


def ref_predict(w, X, eps, dae):
    """fp64 log_softmax(logits) without dropout."""
    if dae:
        return od.log_softmax(od.forward(w, X, dtype=np.float64)["logits"])
    L = w["Wm"].shape[1]
    return ov.log_softmax(ov.forward(w, X, np.zeros((X.shape[0], L), f32) if eps is None else eps, dtype=np.float64)["logits"])


def grad_violations(got, ref, rows_of_w1):
    """The gradient assertions of the edge cases as a list of (what, error, bound, margin = error / bound): each tensor against
    GRAD_RTOL x its reference's largest |entry|, and the listed rows of gW1 each against that row's own largest |entry| (a row whose
    reference is all zero must be exactly zero: margin 0 or inf)."""
    out = []
    for k in ORDER:
        err, bound = float(np.abs(got[k] - ref[k]).max()), GRAD_RTOL * float(np.abs(ref[k]).max())
        out.append((k, err, bound))
    for item in rows_of_w1:
        err, bound = float(np.abs(got["W1"][item] - ref["W1"][item]).max()), GRAD_RTOL * float(np.abs(ref["W1"][item]).max())
        out.append((f"W1[{item}]", err, bound))
    return [(k, e, b, (e / b if b > 0 else (0.0 if e == 0 else float("inf")))) for k, e, b in out]


# ---- dense Adam --------------------------------------------------------------------------------------------------------------------------
def adam_f32(th, g, m, v, alpha):
    """k_adam_apply_oct on fp32 arrays, every operation rounded once to fp32 in the kernel's order:
    m += (g - m)(1 - b1); v += (g g - v)(1 - b2); th -= (m alpha) / (sqrt(v) + eps).  Returns (th, m, v, update)."""
    th, g, m, v = (np.asarray(a, dtype=f32) for a in (th, g, m, v))
    omb1, omb2, alpha = f32(1.0) - f32(0.9), f32(1.0) - f32(0.999), f32(alpha)
    m = m + (g - m) * omb1
    v = v + (g * g - v) * omb2
    upd = (m * alpha) / (np.sqrt(v) + f32(1e-7))
    return th - upd, m, v, upd


# ---- the GPU cases -----------------------------------------------------------------------------------------------------------------------
# every case: item 0 in every non-empty batch row, item 1 in exactly 16 rows (the last that k_vae_w1_light sums), item 2 in exactly 17
# (the first of k_vae_w1_rows), item 3 in none, the last item in the last batch row alone
def _positions(B, n, lo, hi, seed, avoid=()):
    pool = np.setdiff1d(np.arange(lo, min(hi, B - 1)), np.asarray(avoid, dtype=np.int64))
    return np.sort(np.random.RandomState(seed).choice(pool, n, replace=False))


def _edge(dae, rate):
    # I = 203 (rows of the logits not 16-byte aligned, b4 with a scalar tail), L = 7, three users without items, one user twice
    return dict(I=203, H=64, L=7, B=150, U=160, dae=dae, rate=rate, density=0.05, empty=(5, 70, 131), dup=(20, 97), seed=31)


CASES = {
    "edge-vae-r0": _edge(False, 0.0), "edge-vae-r0.5": _edge(False, 0.5), "edge-dae-r0": _edge(True, 0.0), "edge-dae-r0.5": _edge(True, 0.5),
    # chunks of four hidden units per lane: H/4 = 1, 65, 129, 193, 256 -> CPL 1, 2, 3, 4, 4 (H = 1024: the largest vae_check allows)
    **{f"cpl-H{H}": dict(I=120, H=H, L=8, B=70, U=80, dae=False, rate=0.5, density=0.05, seed=seed)
       for H, seed in ((4, 44), (260, 410), (516, 556), (772, 812), (1024, 1064))},
    # presence flags of k_vae_w1_rows beyond 1024: 17 rows all at positions >= 1024, 16 rows across position 1024
    "cap-B1100": dict(I=64, H=32, L=4, B=1100, U=1110, dae=False, rate=0.5, density=0.012, seed=151, hi17=(1024, 1100), straddle=1024),
    "cap-B2048": dict(I=64, H=32, L=4, B=2048, U=2060, dae=False, rate=0.0, density=0.006, seed=52, hi17=(1024, 2048), straddle=1024),
    # B > 2048: k_vae_densify + one transposed product
    "dense-B2049": dict(I=40, H=32, L=4, B=2049, U=2060, dae=False, rate=0.5, density=0.02, seed=153),
}
# (the seeds are such that at step 1 dropout keeps the last item's one entry: test_vae_ref_host.py asserts it)
# (case, variant): plain = one grads call with eps; nglobal = batch means over 2 B rows; oneside = the same with the option vae_side = 0;
# step2 = a second call, at step 2 (another dropout mask), without eps
RUNS = [(c, v) for c in CASES for v in (("plain", "nglobal", "oneside", "step2") if c.startswith("edge") else ("plain",))]
ANNEAL, DROP_SEED = 0.1, 42


@functools.lru_cache(None)
def case_inputs(name):
    c = SimpleNamespace(**CASES[name])
    B, I = c.B, c.I
    empty, dup = getattr(c, "empty", ()), getattr(c, "dup", None)
    avoid = tuple(empty) + tuple(dup or ())
    if hasattr(c, "straddle"):
        p16 = np.arange(c.straddle - 8, c.straddle + 8)
        p17 = _positions(B, 17, c.hi17[0], c.hi17[1], c.seed + 1)
    else:
        p16, p17 = _positions(B, 16, 0, B, c.seed + 1, avoid), _positions(B, 17, 0, B, c.seed + 2, avoid)
    c.items = SimpleNamespace(every=0, n16=1, n17=2, none=3, last=I - 1)
    c.batch = make_batch(c.U, I, B, c.density, c.seed, every=(0,), at={1: p16, 2: p17, 3: [], I - 1: [B - 1]}, empty=empty, dup=dup)
    c.want_counts = {0: B - len(empty), 1: 16, 2: 17, 3: 0, I - 1: 1}
    c.pos16, c.pos17 = p16, p17
    c.w = init_weights(I, c.H, c.L, c.dae, c.seed + 3)
    c.eps = None if c.dae else np.random.RandomState(c.seed + 4).normal(size=(B, c.L)).astype(f32)
    c.Xb = c.batch.X[c.batch.rows]
    c.name = name
    return c


def run_inputs(name, variant):
    """(case, step, eps, n_global, drop mask) of one grads call."""
    c = case_inputs(name)
    step = 2 if variant == "step2" else 1
    eps = None if variant == "step2" else c.eps
    n_global = 2 * c.B if variant == "nglobal" else c.B
    return c, step, eps, n_global, drop_mask(c.batch.rows, c.I, c.rate, DROP_SEED, step)


@functools.lru_cache(None)
def run_reference(name, variant):
    """fp64 (loss, gradients) of one run; computed once, shared, never written to."""
    c, step, eps, n_global, drop = run_inputs(name, variant)
    loss, g = ref_grads(c.w, c.Xb, eps, ANNEAL, drop, n_global, c.dae)
    for a in g.values():
        a.setflags(write=False)
    return float(loss), g
