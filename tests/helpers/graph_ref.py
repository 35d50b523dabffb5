"""NumPy / SciPy restatements of what elliot_amd/csrc/el_graph.hip computes, and the hand-built CSR its edge tests run on.

  edge_csr / exact_vals / exact_table   a CSR whose row lengths sit on every boundary of k_spmm_csr's three nested strides (4 gathers in
                                        flight, lpt indices per pass, 512 per chunk) and of k_spmm_finish's eight partials in flight, with
                                        values for which fp32 arithmetic is EXACT
  spmm_f64                              Y = L X through SciPy in fp64
  spmm_chunk_order_f32                  the same product summed in fp32 in the kernels' order (chunks of 512 in sequence, partials in order)
  lightgcn_propagate_f64                LightGCN_model.py:68-94 in fp64, alpha_k = 1 / (1 + k) rounded to fp32 as the kernel's is
  ngcf_pre / leaky_relu / l2_normalize_f64 / ngcf_propagate_f64
                                        the dense half of an NGCF layer (NGCF_model.py:106-142)
  dropout_keep                          k_ngcf_post's counter-based message-dropout mask from the host Philox (oracle/sampler.py)
  adam_l2_dense                         NGCFOracle.train_step (oracle/ngcf.py), the Keras dense Adam step on g = two_lw * theta, in fp32 or fp64

Everything is fp64 except where a test claims bitwise equality with one fp32 rounding per element (ngcf_pre, leaky_relu, adam_l2_dense
with dtype=float32) or asks what fp32 summation in the kernels' order costs (spmm_chunk_order_f32).
"""
import numpy as np
import scipy.sparse as sp

from oracle import tf_clauses
from oracle.sampler import philox4x32_10

f32, f64 = np.float32, np.float64

SPMM_CHUNK = 512
# every length the strides of k_spmm_csr / k_spmm_finish can go wrong at: around 4 (gathers in flight), around lpt = 8 / 16 / 32 / 64,
# around one chunk (512), around 2 and 8 chunks, and the partial counts 8, 9, 10, 16 and 17 of the finish pass
ROW_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 511, 512, 513, 1023, 1024, 1025, 4096, 4097, 4609, 8192, 8197)
_FILLER = (0, 0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65)


def edge_csr(N=9000, seed=0):
    """(indptr int64, indices int32 ascending and distinct per row, {length: [rows]}) of an N x N pattern.  Rows 0 and N - 1 are
    multi-chunk rows (17 and 16 partials), multi-chunk rows lie on both sides of N // 2 and directly around it, every long row has an
    empty neighbour, and every length of ROW_LENGTHS occurs on both sides of N // 2; the other rows draw short lengths at random."""
    rs = np.random.RandomState(seed)
    mid = N // 2
    lens = np.asarray(_FILLER)[rs.randint(0, len(_FILLER), N)]
    placed = {0: 8197, 1: 0, 2: 4097, 3: 0, 4: 513, 5: 1025, 6: 0, mid - 3: 0, mid - 2: 1024, mid - 1: 4096, mid: 4609, mid + 1: 0,
              mid + 2: 1023, mid + 3: 8197, mid + 4: 0, N - 5: 0, N - 4: 4097, N - 3: 513, N - 2: 0, N - 1: 8192}
    for k, n in enumerate(ROW_LENGTHS):
        placed.setdefault(10 + k, n)
        placed.setdefault(mid + 10 + k, n)
    for r, n in placed.items():
        lens[r] = n
    assert lens.max() <= N
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.empty(int(indptr[-1]), np.int32)
    for r in range(N):
        n = int(lens[r])
        if n > 65:
            cols = np.sort(rs.choice(N, n, replace=False))
        elif n:
            gaps = rs.randint(1, (N - 1) // 66, n)                # ascending and distinct: a random start plus positive gaps
            cols = rs.randint(0, N - int(gaps.sum())) + np.cumsum(gaps)
        else:
            continue
        indices[indptr[r]:indptr[r + 1]] = cols
    where = {}
    for r in range(N):
        where.setdefault(int(lens[r]), []).append(r)
    return indptr, indices, where


def exact_vals(nnz, rs):
    """Non-zero weights from {0.5, 1, 2} with a random sign."""
    return (rs.choice(np.asarray([0.5, 1.0, 2.0], f32), nnz) * rs.choice(np.asarray([-1.0, 1.0], f32), nnz)).astype(f32)


def exact_table(rows, F, rs):
    """Integers in [-8, 8] as fp32.  With exact_vals every product is a multiple of 0.5 of magnitude <= 16 and every partial sum of at
    most 8 197 of them stays below 2^18, i.e. is a multiple of 0.5 below 2^18 and so one of fp32's 2^24 exactly representable
    neighbours: every fp32 sum is exact in ANY order, with or without fused multiply-add, and the product must equal the fp64 one bit
    for bit -- a dropped, repeated or zero-weighted term cannot hide in a tolerance."""
    return rs.randint(-8, 9, size=(rows, F)).astype(f32)


def spmm_f64(indptr, indices, vals, X):
    N = len(indptr) - 1
    L = sp.csr_matrix((np.asarray(vals, f64), np.asarray(indices), np.asarray(indptr)), shape=(N, N))
    return L @ np.asarray(X, f64)


def spmm_magnitude(indptr, indices, vals, X):
    """sum_p |vals[p]| |X[indices[p]]|: the scale of the existing test's bound 4e-7 * mag + 1e-12."""
    return spmm_f64(indptr, indices, np.abs(vals), np.abs(X))


def spmm_chunk_order_f32(indptr, indices, vals, X, chunk=SPMM_CHUNK):
    """The product in fp32 as the kernels sum it: every chunk of <= 512 consecutive non-zeros of a row from zero, term by term (a product
    rounded, then added); a row of several chunks adds its partial rows, from zero, in chunk order."""
    X = np.asarray(X, f32)
    vals = np.asarray(vals, f32)
    N, F = len(indptr) - 1, X.shape[1]
    lens = np.diff(indptr)
    nch = np.maximum((lens + chunk - 1) // chunk, 1)
    row_of = np.repeat(np.arange(N), nch)
    k_in_row = np.arange(len(row_of)) - np.repeat(np.cumsum(nch) - nch, nch)
    lo = indptr[:-1][row_of] + k_in_row * chunk
    hi = np.minimum(lo + chunk, indptr[1:][row_of])
    part = np.zeros((len(row_of), F), f32)
    for t in range(chunk):
        live = np.nonzero(lo + t < hi)[0]
        if not len(live):
            break
        p = lo[live] + t
        part[live] = part[live] + vals[p][:, None] * X[indices[p]]
    Y = np.zeros((N, F), f32)
    for k in range(int(nch.max())):                               # partial k of every row that has one, in order
        sel = np.nonzero(k_in_row == k)[0]
        Y[row_of[sel]] = Y[row_of[sel]] + part[sel]
    return Y


def lightgcn_propagate_f64(Gu, Gi, L, n_layers):
    """:68-94 in fp64: mean over k = 0 .. n_layers of alpha_k L^k [Gu; Gi], alpha_0 = 1, alpha_k = fl32(1 / (1 + k))."""
    U = Gu.shape[0]
    L = sp.csr_matrix(L).astype(f64)
    ego = np.concatenate([Gu, Gi], 0).astype(f64)
    tot = ego.copy()
    for k in range(1, n_layers + 1):
        ego = L @ ego
        tot = tot + f64(f32(1 / (1 + k))) * ego
    mean = tot / f64(n_layers + 1)
    return mean[:U], mean[U:]


def ngcf_pre(ego, lap, dtype=f32):
    """X2 = [lap + ego | ego * lap] (k_ngcf_pre): one rounding per element in fp32."""
    ego, lap = np.asarray(ego, dtype), np.asarray(lap, dtype)
    return np.concatenate([lap + ego, ego * lap], 1)


def leaky_relu(s, dtype=f32):
    """tf.nn.leaky_relu with its default slope 0.2 (held in fp32, as the kernel holds it)."""
    s = np.asarray(s, dtype)
    return np.where(s > 0, s, dtype(f32(0.2)) * s).astype(dtype)


def l2_normalize_f64(x):
    """tf.nn.l2_normalize(x, axis=1) = x / sqrt(max(sum x^2, 1e-12)) in fp64."""
    x = np.asarray(x, f64)
    return x / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), 1e-12))


def ngcf_propagate_f64(Gu, Gi, L, layers, embed_k):
    """NGCF_model.py:106-142 with message dropout 0, in fp64, from the pieces above: the new full-width (Gu, Gi)."""
    U = Gu.shape[0]
    L = sp.csr_matrix(L).astype(f64)
    ego = np.concatenate([Gu[:, :embed_k], Gi[:, :embed_k]], 0).astype(f64)
    out = [ego]
    for l in layers:
        x2 = ngcf_pre(ego, L @ ego, f64)
        w = np.concatenate([l["W1"], l["W2"]], 0).astype(f64)
        ego = leaky_relu(x2 @ w + (l["b1"].astype(f64) + l["b2"].astype(f64)), f64)
        out.append(l2_normalize_f64(ego))
    allc = np.concatenate(out, 1)
    return allc[:U], allc[U:]


def dropout_keep(N, kout, rate, seed, step):
    """k_ngcf_post's mask: entry (r, c) draws Philox4x32-10 at counter (r lo, r hi, c, step) under key (seed lo, seed hi); its first
    word's upper 24 bits are the uniform; the entry is KEPT iff uniform >= fl32(rate)."""
    keep = np.empty((N, kout), bool)
    for r in range(N):
        for c in range(kout):
            x = philox4x32_10(r & 0xffffffff, r >> 32, c, step, seed & 0xffffffff, (seed >> 32) & 0xffffffff)[0]
            keep[r, c] = f32(x >> 8) * f32(2.0 ** -24) >= f32(rate)
    return keep


def adam_l2_dense(th, m, v, lr_t, two_lw, dtype=f32):
    """NGCFOracle.train_step's GraphLayers update: Keras' dense Adam apply on g = two_lw * theta -> (theta', m', v', the three
    updates).  dtype = float32 follows the kernel rounding for rounding; float64 takes the same fp32 constants (lr_t, two_lw, 1 - beta,
    epsilon) through fp64 arithmetic."""
    th, m, v = (np.asarray(x, dtype) for x in (th, m, v))
    c1, c2 = dtype(tf_clauses.one_minus(0.9)), dtype(tf_clauses.one_minus(0.999))
    g = dtype(f32(two_lw)) * th
    dm = (g - m) * c1
    m2 = m + dm
    dv = (g * g - v) * c2
    v2 = v + dv
    dth = (m2 * dtype(f32(lr_t))) / (np.sqrt(v2) + dtype(f32(1e-7)))
    return th - dth, m2, v2, (dth, dm, dv)
