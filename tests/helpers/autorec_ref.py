"""What tests/test_gpu_autorec_edges.py and tests/test_gpu_autorec_plugin.py hold the AutoRec kernels (elliot_amd/csrc/el_autorec.hip)
to, restated in NumPy exactly as the reference's lines read (userautorec_model.py:93-107, itemautorec_model.py:90-104), DENSELY:

    encoded = sigmoid(batch W1 + b1);  reconstructed = act(encoded W2 + b2)            act: linear (user), sigmoid (item)
    reconstructed = reconstructed * sign(batch);  error = batch - reconstructed;  loss = reduce_mean(reduce_sum(error**2, axis=1))

  forward / ref_grads   loss and the four gradients in the device's layout (W1, b1, W2T, b2), hand-written backward pass
  train_ref             Keras' dense Adam on a list of batches, in fp64 or -- one IEEE operation at a time -- in fp32 (vae_ref.adam_f32)
  CASES / case_inputs   the inputs of every GPU case, shared with tests/test_autorec_ref_host.py (which checks them without a GPU)
  plugin_*              the 60 x 45 data set of the plugin test and the restatement of its two epochs
"""
import functools
import random
from types import SimpleNamespace

import numpy as np

from tests.helpers.vae_ref import GRAD_RTOL, LOSS_RTOL, adam_f32, batch_counts, make_batch  # noqa: F401

f32 = np.float32
ORDER = ("W1", "b1", "W2T", "b2")                  # ops.AutoRecDeviceState.ORDER
HEADS = ("linear", "sigmoid")                      # UserAutoRec, ItemAutoRec
AR_LIGHT = 16                                      # el_autorec.hip: an item in more batch rows than this is summed by k_ar_item_heavy


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---- loss and gradients ------------------------------------------------------------------------------------------------------------------
def forward(w, X, head, dtype=np.float64):
    """The reference's lines on a dense batch X [B, N]; w = {W1 [N,H], b1, W2 [H,N], b2} (Keras layouts)."""
    W1, b1, W2, b2 = (np.asarray(w[k], dtype=dtype) for k in ("W1", "b1", "W2", "b2"))
    X = np.asarray(X, dtype=dtype)
    h = _sigmoid(X @ W1 + b1)
    pre = h @ W2 + b2
    r = _sigmoid(pre) if head == "sigmoid" else pre
    sign = np.sign(X)
    error = X - r * sign
    loss = np.mean(np.sum(error ** 2, axis=1, dtype=dtype), dtype=dtype)
    return SimpleNamespace(X=X, h=h, r=r, sign=sign, error=error, loss=loss, W2=W2)


def predict(w, X, head, dtype=np.float64):
    return forward(w, X, head, dtype).r


def ref_grads(w, X, head, n_global=None, dtype=np.float64):
    """(loss, {W1, b1, W2T, b2}) with the batch mean over n_global rows (default: the rows of X)."""
    c = forward(w, X, head, dtype)
    B = X.shape[0]
    s = dtype(B) / dtype(B if n_global is None else n_global)
    dr = (dtype(-2.0) / dtype(B)) * c.error * c.sign
    dpre = dr * c.r * (1 - c.r) if head == "sigmoid" else dr
    dpre1 = (dpre @ c.W2.T) * c.h * (1 - c.h)
    # (column sums over the contiguous axis of a transposed copy: NumPy then adds pairwise.  Its axis-0 sum of a C-ordered array adds
    #  row after row, and 2 048 sequential fp32 additions are an error of their own, 100 x that of the terms)
    colsum = lambda a: np.ascontiguousarray(a.T).sum(1)
    g = {"W1": c.X.T @ dpre1, "b1": colsum(dpre1), "W2T": (c.h.T @ dpre).T, "b2": colsum(dpre)}
    return c.loss * s, {k: np.ascontiguousarray(v * s) for k, v in g.items()}


def to_device_layout(w):
    return {"W1": w["W1"], "b1": w["b1"], "W2T": np.ascontiguousarray(np.asarray(w["W2"]).T), "b2": w["b2"]}


def adam_lr_t(lr, step, dtype):
    """Keras' bias-corrected step size in `dtype` (ops.adam_lr_t is the fp32 one)."""
    b1p, b2p = np.power(dtype(0.9), dtype(step)), np.power(dtype(0.999), dtype(step))
    return dtype(lr) * np.sqrt(dtype(1.0) - b2p) / (dtype(1.0) - b1p)


def adam(th, g, m, v, alpha, dtype):
    """TF's dense ApplyAdam in `dtype`: vae_ref.adam_f32's arithmetic."""
    if dtype == f32:
        return adam_f32(th, g, m, v, alpha)[:3]
    omb1, omb2 = 1.0 - 0.9, 1.0 - 0.999
    m = m + (g - m) * omb1
    v = v + (g * g - v) * omb2
    return th - (m * alpha) / (np.sqrt(v) + 1e-7), m, v


def train_ref(w, X_all, batches, lr, head, dtype=np.float64):
    """Variables (device layout) after one Adam step per batch (lists of row ids of X_all); returns (variables, losses)."""
    th = {k: np.asarray(v, dtype=dtype).copy() for k, v in to_device_layout(w).items()}
    m = {k: np.zeros_like(v) for k, v in th.items()}
    v = {k: np.zeros_like(x) for k, x in th.items()}
    losses = []
    for step, rows in enumerate(batches, 1):
        keras = {"W1": th["W1"], "b1": th["b1"], "W2": th["W2T"].T, "b2": th["b2"]}
        loss, g = ref_grads(keras, X_all[np.asarray(rows)], head, dtype=dtype)
        losses.append(float(loss))
        alpha = adam_lr_t(lr, step, dtype)
        for k in ORDER:
            th[k], m[k], v[k] = adam(th[k], g[k].astype(dtype), m[k], v[k], alpha, dtype)
    return th, losses


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
def grad_violations(got, ref, counts, n_global, special):
    """The gradient assertions as (what, error, bound, margin = error / bound):
      each of the four tensors      GRAD_RTOL x the reference's largest |entry|
      rows of gW1 of `special`      GRAD_RTOL x that row's largest |entry|
      row j of gW2T, entry j of gb2 GRAD_RTOL x (2 / n_global) x n_j, n_j = counts[j] batch rows holding j: |d| <= 2 |1 - r| / n_global per
                                    entry, and with the linear head 1 - r cancels, so the row's own size is no yardstick (the fp32
                                    restatement itself misses a bound relative to it); a row no batch row holds must be exactly zero."""
    out = []
    for k in ORDER:
        out.append((k, float(np.abs(got[k] - ref[k]).max()), GRAD_RTOL * float(np.abs(ref[k]).max())))
    for j in special:
        out.append((f"W1[{j}]", float(np.abs(got["W1"][j] - ref["W1"][j]).max()), GRAD_RTOL * float(np.abs(ref["W1"][j]).max())))
    per_j = GRAD_RTOL * (2.0 / n_global) * np.asarray(counts, dtype=np.float64)
    e2 = np.abs(got["W2T"] - ref["W2T"]).max(axis=1)
    eb = np.abs(got["b2"] - ref["b2"])
    for name, e in (("W2T rows", e2), ("b2 entries", eb)):
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(per_j > 0, e / per_j, np.where(e == 0, 0.0, np.inf))
        j = int(np.argmax(ratio))
        out.append((f"{name} (worst: {j})", float(e[j]), float(per_j[j])))
    return [(k, e, b, (e / b if b > 0 else (0.0 if e == 0 else float("inf")))) for k, e, b in out]


# ---- the GPU cases -----------------------------------------------------------------------------------------------------------------------
# every case: item 0 in every non-empty batch row, item 1 in exactly 16 rows (the last that k_ar_item_light sums), item 2 in exactly 17
# (the first of k_ar_item_heavy), item 3 in none, the last item in the last batch row alone
def _positions(B, n, lo, hi, seed, avoid=()):
    pool = np.setdiff1d(np.arange(lo, min(hi, B - 1)), np.asarray(avoid, dtype=np.int64))
    return np.sort(np.random.RandomState(seed).choice(pool, n, replace=False))


CASES = {
    # N = 203 (b2 with a scalar tail), B = 150 (no multiple of 64), three rows without entries, one row id at two batch positions
    "edge": dict(N=203, H=64, B=150, R=160, density=0.05, empty=(5, 70, 131), dup=(20, 97), seed=31),
    # chunks of four hidden units per lane: H/4 = 1, 65, 129, 193, 256 -> CPL 1, 2, 3, 4, 4 (H = 1024: the widest layer admitted)
    **{f"cpl-H{H}": dict(N=120, H=H, B=70, R=80, density=0.05, seed=seed)
       for H, seed in ((4, 44), (260, 410), (516, 556), (772, 812), (1024, 1064))},
    # presence bits beyond position 1024: the 17-row item only at positions >= 1024, the 16-row item across position 1024
    "big-B1100": dict(N=64, H=32, B=1100, R=1110, density=0.012, seed=151, hi17=(1024, 1100), straddle=1024),
    "big-B2048": dict(N=64, H=32, B=2048, R=2060, density=0.006, seed=52, hi17=(1024, 2048), straddle=1024),
    # beyond the VAE's 2 048 presence flags: the same sparse path
    "big-B2049": dict(N=203, H=64, B=2049, R=2060, density=0.01, seed=153, hi17=(1024, 2049), straddle=1024),
    "big-B5000": dict(N=203, H=64, B=5000, R=5010, density=0.01, seed=154, hi17=(4096, 5000), straddle=4096),
}
SPECIAL = ("none", "last", "n16", "n17")


def init_weights(N, H, seed):
    """Glorot-sized normal kernels; biases near the reference's ones (exact ones would hide a bias that is added twice or scaled)."""
    rs = np.random.RandomState(seed)
    std = np.sqrt(2.0 / (N + H))
    return {"W1": (rs.normal(size=(N, H)) * std).astype(f32), "b1": (1 + 0.1 * rs.normal(size=H)).astype(f32),
            "W2": (rs.normal(size=(H, N)) * std).astype(f32), "b2": (1 + 0.1 * rs.normal(size=N)).astype(f32)}


@functools.lru_cache(None)
def case_inputs(name):
    c = SimpleNamespace(**CASES[name])
    B, N = c.B, c.N
    empty, dup = getattr(c, "empty", ()), getattr(c, "dup", None)
    avoid = tuple(empty) + tuple(dup or ())
    if hasattr(c, "straddle"):
        p16 = np.arange(c.straddle - 8, c.straddle + 8)
        p17 = _positions(B, 17, c.hi17[0], c.hi17[1], c.seed + 1)
    else:
        p16, p17 = _positions(B, 16, 0, B, c.seed + 1, avoid), _positions(B, 17, 0, B, c.seed + 2, avoid)
    c.items = SimpleNamespace(every=0, n16=1, n17=2, none=3, last=N - 1)
    c.batch = make_batch(c.R, N, B, c.density, c.seed, every=(0,), at={1: p16, 2: p17, 3: [], N - 1: [B - 1]}, empty=empty, dup=dup)
    c.want_counts = {0: B - len(empty), 1: 16, 2: 17, 3: 0, N - 1: 1}
    c.pos16, c.pos17, c.empty, c.dup = p16, p17, tuple(empty), dup
    c.w = init_weights(N, c.H, c.seed + 3)
    c.Xb = c.batch.X[c.batch.rows]
    c.counts = (c.Xb != 0).sum(0)
    c.nnz = int(c.counts.sum())
    c.special = tuple(getattr(c.items, s) for s in SPECIAL)
    c.name = name
    return c


@functools.lru_cache(None)
def run_reference(name, head, n_global=None):
    """fp64 (loss, gradients) of one case; computed once, shared, never written to."""
    c = case_inputs(name)
    loss, g = ref_grads(c.w, c.Xb, head, n_global)
    for a in g.values():
        a.setflags(write=False)
    return float(loss), g


# ---- the plugin test's data and its restatement ------------------------------------------------------------------------------------------
PLUGIN = SimpleNamespace(U=60, I=45, H=16, lr=0.01, epochs=2, seed=42, k=10, data_seed=7,
                         batch={"UserAutoRec": 25, "ItemAutoRec": 20})
# max |variable - fp64| of the FLOAT32 restatement after the plugin test's steps (tests/test_autorec_ref_host.py measures and asserts it):
# the GPU test allows 4 x this
PLUGIN_F32_DISTANCE = {"UserAutoRec": 1.4e-7, "ItemAutoRec": 3.6e-7}


@functools.lru_cache(None)
def plugin_matrix():
    """Binary [60, 45] train matrix with popular and rare items, two users and one item without any entry."""
    rs = np.random.RandomState(PLUGIN.data_seed)
    pop = 0.05 + 0.5 * rs.rand(PLUGIN.I) ** 2
    X = (rs.rand(PLUGIN.U, PLUGIN.I) < pop[None, :]).astype(f32)
    X[[11, 47]] = 0
    X[:, 30] = 0
    X.setflags(write=False)
    return X


def plugin_rows_matrix(which):
    X = plugin_matrix()
    return X if which == "UserAutoRec" else np.ascontiguousarray(X.T)


def plugin_batches(which, evaluations=True):
    """The batches `sparse_sampler.Sampler` hands the plugin over the test's epochs: random.seed(42) in its constructor, one
    random.sample per epoch -- and, for ItemAutoRec, one more per evaluation (itemautorec.py:102).  Returns (batches, the
    evaluation shuffles, random's state at the end); leaves the global generator as it found it."""
    keep = random.getstate()
    try:
        random.seed(42)
        n = PLUGIN.U if which == "UserAutoRec" else PLUGIN.I
        bs = PLUGIN.batch[which]
        batches, evals = [], []
        for _ in range(PLUGIN.epochs):
            order = random.sample(range(n), n)
            batches += [order[s:s + bs] for s in range(0, n, bs)]
            if which == "ItemAutoRec" and evaluations:
                evals.append(random.sample(range(n), n))
        return batches, evals, random.getstate()
    finally:
        random.setstate(keep)


def plugin_weights(which):
    """The plugin's start values at seed 42 (autorec_model.py): Glorot-normal kernels drawn W1 first, biases of ones."""
    from elliot_amd.recommender.autoencoders.vae.multi_vae_model import _glorot_normal
    N = plugin_rows_matrix(which).shape[1]
    rs = np.random.RandomState(PLUGIN.seed)
    return {"W1": _glorot_normal(rs, N, PLUGIN.H), "b1": np.ones(PLUGIN.H, f32), "W2": _glorot_normal(rs, PLUGIN.H, N), "b2": np.ones(N, f32)}


@functools.lru_cache(None)
def plugin_reference(which):
    """fp64 (variables, per-step losses) of the plugin test's run; computed once, shared, never written to."""
    batches, _, _ = plugin_batches(which)
    th, losses = train_ref(plugin_weights(which), plugin_rows_matrix(which), batches, PLUGIN.lr, plugin_head(which), np.float64)
    for a in th.values():
        a.setflags(write=False)
    return th, tuple(losses)


def plugin_head(which):
    return "linear" if which == "UserAutoRec" else "sigmoid"


def plugin_scores(th, which, dtype=np.float64, order=None):
    """[U, I] scores of the trained variables `th` (device layout): the user variant's reconstruction, or the item variant's
    transposed one -- column c holding item order[c] when an evaluation shuffle is given."""
    w = {"W1": th["W1"], "b1": th["b1"], "W2": np.asarray(th["W2T"]).T, "b2": th["b2"]}
    Xr = plugin_rows_matrix(which)
    if which == "UserAutoRec":
        return predict(w, Xr, "linear", dtype)
    rows = np.arange(PLUGIN.I) if order is None else np.asarray(order)
    return predict(w, Xr[rows], "sigmoid", dtype).T


def topk_lists(scores, train, k):
    """Top-k item ids per user among the items the user has no train entry for (ties: the smaller id)."""
    s = np.where(train != 0, -np.inf, scores)
    return np.argsort(-s, axis=1, kind="stable")[:, :k]


def decided_users(scores64, train, k, gap):
    """Users whose fp64 gap between ranks k and k + 1 exceeds `gap`: their top-k SET does not depend on errors below gap / 2."""
    s = np.sort(np.where(train != 0, -np.inf, scores64), axis=1)[:, ::-1]
    return (s[:, k - 1] - s[:, k]) > gap
