"""Tensor-level wrappers over the C ABI.

torch tensors are used ONLY as device-buffer holders (allocation, streams, H2D/D2H copies);
all arithmetic happens inside libelliot_hip.so.  Every function raises if the library or a
GPU is missing -- there is no CPU path here.
"""
import ctypes as C
import os
import math

import numpy as np
import torch

from . import _lib
from ._lib import (EL_OPT_ADAM_LAZY, EL_OPT_ADAM_TF_DENSE, EL_OPT_SGD, EL_TOPK_AUTO, EL_TOPK_MFMA, EL_TOPK_SCREEN,
                   EL_TOPK_SIMPLE, BprmfState, BprsgdState, check)

OPTIMIZERS = {"adam": EL_OPT_ADAM_TF_DENSE, "adam_tf_dense": EL_OPT_ADAM_TF_DENSE,
              "adam_lazy": EL_OPT_ADAM_LAZY, "sgd": EL_OPT_SGD, "sgd_dense": EL_OPT_SGD}
TOPK_ALGOS = {"auto": EL_TOPK_AUTO, "mfma": EL_TOPK_MFMA, "simple": EL_TOPK_SIMPLE, "screen": EL_TOPK_SCREEN}
BPR_ALGOS = {"auto": _lib.EL_BPR_AUTO, "atomic": _lib.EL_BPR_ATOMIC, "sorted": _lib.EL_BPR_SORTED}


def _ptr(t, dtype=None, name="tensor"):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise _lib.ElliotHipError(f"{name}: tensor must live on the GPU (got {t.device})")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def workspace(holder, attr, need, device):
    """Every workspace a library call is handed comes from here: the uint8 device tensor cached as holder.<attr>, replaced by a
    larger one when it holds fewer than `need` bytes (never a zero-length buffer).  attr = None: a fresh tensor, kept nowhere."""
    ws = getattr(holder, attr, None) if attr else None
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=device)
        if attr:
            setattr(holder, attr, ws)
    return ws


def _own(x, device, dtype=torch.float32):
    """A state's private copy of a parameter: a numpy array, host tensor or device tensor as a contiguous `dtype` tensor on `device`
    that never aliases the caller's.  None stays None."""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    t = x.to(device=device, dtype=dtype).contiguous()
    return t.clone() if t.untyped_storage().data_ptr() == x.untyped_storage().data_ptr() else t


class Context:
    """One el_ctx per device (include/elliot_hip.h: el_ctx_create)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.ElliotHipError("no GPU visible: elliot_amd needs an MI355X (gfx950)")
        self.device = torch.device("cuda", int(device))
        h = C.c_void_p()
        check(self.lib.el_ctx_create(int(device), C.byref(h)), "el_ctx_create")
        self.handle = h
        name = C.create_string_buffer(64)
        cus = C.c_int()
        hbm = C.c_int64()
        check(self.lib.el_device_info(h, name, 64, C.byref(cus), C.byref(hbm)), "el_device_info")
        self.arch, self.cus, self.hbm_bytes = name.value.decode(), cus.value, hbm.value

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_option(self, name, value):
        """A switch of the library on this context (include/elliot_hip.h: el_ctx_set_option); returns the previous value."""
        old = self.get_option(name)
        check(self.lib.el_ctx_set_option(self.handle, name.encode(), float(value)), "el_ctx_set_option")
        return old

    def get_option(self, name):
        v = C.c_double()
        check(self.lib.el_ctx_get_option(self.handle, name.encode(), C.byref(v)), "el_ctx_get_option")
        return v.value

    def option(self, name, value):
        """with ctx.option("ichunk", 64): ... -- the switch set inside the block, its previous value restored afterwards."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = self.set_option(name, value)
            try:
                yield
            finally:
                self.set_option(name, old)
        return scope()

    def timing(self, on, only=None):
        """Bracket kernel launches with hipEvents; `only` = a kernel name: just those launches (an event between two kernels
        costs their overlap, so timed regions keep them on the kernel of interest)."""
        check(self.lib.el_timing_filter(self.handle, only.encode() if only else None), "el_timing_filter")
        check(self.lib.el_timing_enable(self.handle, 1 if on else 0), "el_timing_enable")

    def timing_report(self):
        """{kernel_name: (launches, total_ms)} since the last report (synchronises the events)."""
        buf = C.create_string_buffer(1 << 16)
        check(self.lib.el_timing_report(self.handle, buf, len(buf)), "el_timing_report")
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.split()
            out[name] = (int(cnt), float(ms))
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.lib.el_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ctx_cache = {}


def get_context(device=0):
    device = int(device)
    if device not in _ctx_cache:
        _ctx_cache[device] = Context(device)
    return _ctx_cache[device]


class DeviceCSR:
    """CSR (int64 indptr, int32 indices, rows sorted ascending) resident in HBM.

    Stands in for the reference's dense bool masks (dataset.py:230-245) and the sampler's
    per-user positive lists (custom_sampler.py:19-22)."""

    def __init__(self, indptr, indices, n_cols, device):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        if indptr.ndim != 1 or indptr[0] != 0 or indptr[-1] != indices.shape[0]:
            raise ValueError("malformed CSR")
        self.n_rows = indptr.shape[0] - 1
        self.n_cols = int(n_cols)
        self.nnz = int(indices.shape[0])
        self.indptr = torch.from_numpy(indptr).to(device)
        # never hand a zero-length buffer's null pointer to the kernels
        self.indices = torch.from_numpy(indices if self.nnz else np.zeros(1, np.int32)).to(device)

    @classmethod
    def from_tensors(cls, indptr, indices, n_cols):
        """Adopt device tensors (int64 indptr, int32 indices) without a host round trip."""
        self = cls.__new__(cls)
        assert indptr.dtype == torch.int64 and indices.dtype == torch.int32
        self.n_rows = indptr.shape[0] - 1
        self.n_cols = int(n_cols)
        self.nnz = int(indices.shape[0])
        self.indptr = indptr.contiguous()
        self.indices = indices.contiguous() if self.nnz else torch.zeros(1, dtype=torch.int32, device=indptr.device)
        return self

    @staticmethod
    def from_scipy(m, device):
        m = m.tocsr()
        m.sort_indices()
        return DeviceCSR(m.indptr, m.indices, m.shape[1], device)


def _csr_ptrs(csr):
    if csr is None:
        return None, None
    return _ptr(csr.indptr, torch.int64, "indptr"), _ptr(csr.indices, torch.int32, "indices")


def _topk_io(ctx, n, k, dtype, excl, cand, out_idx=None, out_val=None):
    """What the four wave top-k wrappers share: the (n, k) outputs (the caller's where given) and the tail of the library call,
    (excl indptr, excl indices, cand indptr, cand indices, k, out_idx, out_val)."""
    if out_idx is None:
        out_idx = torch.empty((n, k), dtype=torch.int32, device=ctx.device)
    if out_val is None:
        out_val = torch.empty((n, k), dtype=dtype, device=ctx.device)
    tail = (*_csr_ptrs(excl), *_csr_ptrs(cand), int(k), _ptr(out_idx, torch.int32), _ptr(out_val, dtype))
    return out_idx, out_val, tail


# ------------------------------------------------------------------------------------------
# scoring + top-k
# ------------------------------------------------------------------------------------------
def score_topk(ctx, Gu, Gi, Bi, u_start, u_stop, k, excl=None, cand=None, item_offset=0, algo="auto",
               out_idx=None, out_val=None, items_unchanged=False):
    """BPRMF_batch_model.predict + get_top_k (BPRMF_batch_model.py:83-88) for users
    [u_start, u_stop): returns (idx int32 [n,k], val float32 [n,k]) on the device.
    items_unchanged: Gi / Bi are exactly what the previous call on this context scored against (block after block of one
    evaluation): the screened kernels keep that call's item-side image."""
    n = int(u_stop) - int(u_start)
    I_local, F = Gi.shape
    if Gu.shape[1] != F:
        raise ValueError("Gu/Gi factor mismatch")
    out_idx, out_val, tail = _topk_io(ctx, n, k, torch.float32, excl, cand, out_idx, out_val)
    algo_id = TOPK_ALGOS[algo] if isinstance(algo, str) else int(algo)
    ws, need = None, 0
    if cand is None and algo_id in (EL_TOPK_AUTO, EL_TOPK_SCREEN):
        need = int(ctx.lib.el_score_topk_ws_bytes(int(n), int(I_local), int(F), int(k), int(excl.nnz) if excl is not None else 0, algo_id))
        if need:
            ws = _ptr(workspace(ctx, "_topk_ws", need, ctx.device))
    check(ctx.lib.el_score_topk(ctx.handle, ctx.stream(), _ptr(Gu, torch.float32, "Gu"),
                                _ptr(Gi, torch.float32, "Gi"), _ptr(Bi, torch.float32, "Bi"),
                                int(u_start), int(u_stop), int(item_offset), int(I_local), int(F), *tail,
                                algo_id | (_lib.EL_TOPK_ITEMS_UNCHANGED if items_unchanged else 0), ws, need),
          "el_score_topk")
    return out_idx, out_val


def score_topk_f64(ctx, P, Q, b, u_start, u_stop, k, excl=None, cand=None, item_offset=0):
    """MFModel.get_user_predictions (BPRMF_model.py:70-85), fp64 tables."""
    n = int(u_stop) - int(u_start)
    I_local, F = Q.shape
    out_idx, out_val, tail = _topk_io(ctx, n, k, torch.float64, excl, cand)
    check(ctx.lib.el_score_topk_f64(ctx.handle, ctx.stream(), _ptr(P, torch.float64, "P"),
                                    _ptr(Q, torch.float64, "Q"), _ptr(b, torch.float64, "b"),
                                    int(u_start), int(u_stop), int(item_offset), int(I_local), int(F), *tail), "el_score_topk_f64")
    return out_idx, out_val


def dense_topk(ctx, preds, u_start, u_stop, k, excl=None, cand=None):
    """get_top_k (multi_vae_model.py:158-159 et al.) over a materialised [n_users, I] block."""
    n, I = preds.shape
    if n != int(u_stop) - int(u_start):
        raise ValueError("preds rows must equal u_stop - u_start")
    out_idx, out_val, tail = _topk_io(ctx, n, k, torch.float32, excl, cand)
    check(ctx.lib.el_dense_topk(ctx.handle, ctx.stream(), _ptr(preds, torch.float32, "preds"), int(preds.stride(0)),
                                int(u_start), int(u_stop), int(I), *tail), "el_dense_topk")
    return out_idx, out_val


def topk_merge(ctx, parts_idx, parts_val):
    """Merge [G, n_users, k] partial lists (item shards) into [n_users, k]."""
    G, n, k = parts_idx.shape
    out_idx = torch.empty((n, k), dtype=torch.int32, device=ctx.device)
    out_val = torch.empty((n, k), dtype=torch.float32, device=ctx.device)
    check(ctx.lib.el_topk_merge(ctx.handle, ctx.stream(), _ptr(parts_idx, torch.int32), _ptr(parts_val, torch.float32),
                                int(G), int(n), int(k), _ptr(out_idx), _ptr(out_val)), "el_topk_merge")
    return out_idx, out_val


# ------------------------------------------------------------------------------------------
# neighbourhood models (ItemKNN / UserKNN, implementation: standard)
# ------------------------------------------------------------------------------------------
KNN_SIMILARITIES = {"cosine": _lib.EL_KNN_COSINE, "dot": _lib.EL_KNN_DOT}


def device_values(values, device, dtype=np.float32):
    """The values of a CSR as a device tensor (float32 unless told otherwise) beside its DeviceCSR (never a zero-length buffer)."""
    v = np.ascontiguousarray(values, dtype=dtype)
    return torch.from_numpy(v if v.shape[0] else np.zeros(1, dtype)).to(device)


def _w_alloc(ctx, n, N):
    """(w_indptr, w_indices, w_vals) for a W of n rows with at most n * N entries (never a zero-length buffer)."""
    return (torch.empty(n + 1, dtype=torch.int64, device=ctx.device), torch.empty(max(n * N, 1), dtype=torch.int32, device=ctx.device),
            torch.empty(max(n * N, 1), dtype=torch.float32, device=ctx.device))


def _w_result(w_indptr, w_indices, w_vals):
    """(DeviceCSR W [n, n], float32 values) of filled _w_alloc arrays: what knn_build, rp3_cut and slim_w return."""
    nnz = int(w_indptr[-1].item())
    W = DeviceCSR.from_tensors(w_indptr, w_indices[:nnz], w_indptr.shape[0] - 1)
    return W, (w_vals[:nnz] if nnz else w_vals[:1])


def knn_integer_ratings(values):
    """(scale, int32 values): ratings times 1 (integers) or 2 (half steps), exactly.  Anything else is refused."""
    v = np.asarray(values, dtype=np.float64)
    for scale in (1, 2):
        s = v * scale
        if np.all(np.isfinite(s)) and np.all(s == np.round(s)) and (s.size == 0 or np.abs(s).max() < 2 ** 31):
            return scale, s.astype(np.int32)
    raise ValueError("ItemKNN / UserKNN need integer or half-step ratings (the similarity counts are exact integers); "
                     "this train matrix holds other values")


def _pair_operands(ctx, M, targets, integer=None):
    """What a co-occurrence kernel reads of a scipy sparse M: P = the targets' side (targets = "rows": M, "cols": M^T) and
    Q = P^T, both with sorted rows.  integer: knn_integer_ratings or its like, which turns the values into exact int32 (or
    refuses them with its caller's message); None: float32 values as they are.
    Returns (Pc, pvt, Qc, qvt, scale, max_deg, max_abs): the two DeviceCSRs with their value tensors, then -- integer only,
    else None -- the scale of the values, the longest row of P and the largest |value|."""
    import scipy.sparse as sp
    M = sp.csr_matrix(M) if integer else sp.csr_matrix(M, dtype=np.float32)
    M.sum_duplicates()
    M.sort_indices()
    Mt = M.T.tocsr()
    Mt.sort_indices()
    P, Q = (M, Mt) if targets == "rows" else (Mt, M)
    n, n_other = P.shape
    scale = max_deg = max_abs = None
    pv, qv, dtype = P.data, Q.data, np.float32
    if integer:
        dtype = np.int32
        scale, pv = integer(P.data)
        _, qv = integer(Q.data)
        max_deg = int(np.diff(P.indptr).max()) if n else 0
        max_abs = int(np.abs(pv).max()) if pv.size else 0
    dev = ctx.device
    return (DeviceCSR(P.indptr, P.indices, n_other, dev), device_values(pv, dev, dtype),
            DeviceCSR(Q.indptr, Q.indices, n, dev), device_values(qv, dev, dtype), scale, max_deg, max_abs)


def _knn_w(ctx, entry, ws_query, Pc, pvt, Qc, qvt, n_neighbors, sim, *extra):
    """W of el_knn_build / el_knn_build_f32 (`entry`; `extra`: its arguments between sim and the outputs) on _pair_operands."""
    n, n_other = Pc.n_rows, Pc.n_cols
    need = int(getattr(ctx.lib, ws_query)(n, int(n_neighbors)))
    ws = workspace(ctx, None, need, ctx.device)
    w_indptr, w_indices, w_vals = _w_alloc(ctx, n, min(int(n_neighbors), n))
    check(getattr(ctx.lib, entry)(ctx.handle, ctx.stream(), _ptr(Pc.indptr), _ptr(Pc.indices), _ptr(pvt), _ptr(Qc.indptr),
                                  _ptr(Qc.indices), _ptr(qvt), n, n_other, int(n_neighbors), KNN_SIMILARITIES[sim], *extra,
                                  _ptr(w_indptr), _ptr(w_indices), _ptr(w_vals), C.c_void_p(ws.data_ptr()), need), entry)
    return _w_result(w_indptr, w_indices, w_vals)


def knn_build(ctx, R, side, n_neighbors, sim):
    """Similarity.initialize (item_knn_similarity.py / user_knn_similarity.py:46-80): W of ItemKNN (side="item": the columns
    of R) or UserKNN (side="user": its rows), top-`n_neighbors` non-zeros per column.  R: scipy sparse [U, I] with values.
    Returns (DeviceCSR W, float32 values tensor); W is [n, n], columns ascending in every row."""
    if sim not in KNN_SIMILARITIES:
        raise ValueError(f"similarity {sim!r} is not supported; supported: {sorted(KNN_SIMILARITIES)}")
    if side not in ("item", "user"):
        raise ValueError("side must be 'item' or 'user'")
    Pc, pvt, Qc, qvt, scale, max_deg, max_abs = _pair_operands(ctx, R, "cols" if side == "item" else "rows", knn_integer_ratings)
    return _knn_w(ctx, "el_knn_build", "el_knn_ws_bytes", Pc, pvt, Qc, qvt, n_neighbors, sim, int(scale), max_deg, max_abs)


def knn_score_topk(ctx, A, A_vals, B, B_vals, u_start, u_stop, k, excl=None, cand=None, out_idx=None, out_val=None):
    """R.dot(W) (ItemKNN: A = R, B = W) or W.dot(R) (UserKNN: A = W, B = R) for users [u_start, u_stop), masked top-k
    (get_user_recs, item_knn_similarity.py:159-175) without the [U, I] block: (idx int32 [n, k], val float32 [n, k])."""
    n = int(u_stop) - int(u_start)
    if out_idx is None:
        out_idx = torch.empty((n, k), dtype=torch.int32, device=ctx.device)
    if out_val is None:
        out_val = torch.empty((n, k), dtype=torch.float32, device=ctx.device)
    ep, ei = _csr_ptrs(excl)
    cp, ci = _csr_ptrs(cand)
    check(ctx.lib.el_knn_score_topk(ctx.handle, ctx.stream(), _ptr(A.indptr, torch.int64), _ptr(A.indices, torch.int32),
                                    _ptr(A_vals, torch.float32), _ptr(B.indptr, torch.int64), _ptr(B.indices, torch.int32),
                                    _ptr(B_vals, torch.float32), int(u_start), int(u_stop), int(B.n_cols), ep, ei, cp, ci,
                                    int(k), _ptr(out_idx, torch.int32), _ptr(out_val, torch.float32)), "el_knn_score_topk")
    return out_idx, out_val


# ------------------------------------------------------------------------------------------
# attribute-aware baselines (AttributeItemKNN / AttributeUserKNN / VSM)
# ------------------------------------------------------------------------------------------
PROFILE_MODES = {"add": _lib.EL_PROFILE_ADD, "last": _lib.EL_PROFILE_LAST}


def _feature_operands(ctx, who, r_indptr, r_indices, F, f_weights):
    """What profile_build and kahfm_init (`who`) read: the train rows and the items' features as DeviceCSRs, the weights (or
    None) as a float64 tensor.  Returns (r_indptr as host int64, Rc, Fc, fw)."""
    r_indptr = np.ascontiguousarray(r_indptr, dtype=np.int64)
    U, (I, nF) = r_indptr.shape[0] - 1, F.shape
    if U < 1 or I < 1 or nF < 1:
        raise ValueError(f"{who}: empty operand (users {U}, items {I}, features {nF})")
    dev = ctx.device
    Rc, Fc = DeviceCSR(r_indptr, r_indices, I, dev), DeviceCSR(F.indptr, F.indices, nF, dev)
    fw = None
    if f_weights is not None:
        fw = np.ascontiguousarray(f_weights, dtype=np.float64)
        if fw.shape[0] != F.nnz:
            raise ValueError(f"{who}: one weight per entry of F")
        fw = device_values(fw, dev, np.float64)
    return r_indptr, Rc, Fc, fw


def profile_build(ctx, r_indptr, r_indices, F, f_weights, mode, by_len):
    """User profiles over item features (compute_binary_profile / TFIDF.get_profiles + build_feature_sparse_values of the
    reference's attribute plug-ins) as a host scipy CSR [U, nF] float32, columns ascending, zeros kept.
    r_indptr / r_indices: the train rows in train_dict order; F: scipy CSR [I, nF], the features of every item (its values are
    not read); f_weights: float64 per entry of F (mode "last") or None; mode "add" | "last"; by_len: divide by the row length."""
    import scipy.sparse as sp
    if mode not in PROFILE_MODES:
        raise ValueError(f"profile_build: mode {mode!r} is not supported; supported: {sorted(PROFILE_MODES)}")
    if mode == "last" and f_weights is None:
        raise ValueError("profile_build: mode 'last' needs one weight per entry of F")
    r_indptr, Rc, Fc, fw = _feature_operands(ctx, "profile_build", r_indptr, r_indices, F, f_weights if mode == "last" else None)
    U, (I, nF), dev = Rc.n_rows, F.shape, ctx.device
    # an entry per feature touched: at most the features of the user's items, and at most nF
    deg = np.concatenate([[0], np.cumsum(np.diff(F.indptr)[np.asarray(r_indices, dtype=np.int64)])])
    cap = int(np.minimum(deg[r_indptr[1:]] - deg[r_indptr[:-1]], nF).sum())
    out_indptr = torch.empty(U + 1, dtype=torch.int64, device=dev)
    out_indices = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    out_vals = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    need = int(ctx.lib.el_profile_ws_bytes(U))
    ws = workspace(ctx, None, need, dev)
    check(ctx.lib.el_profile_build(ctx.handle, ctx.stream(), _ptr(Rc.indptr), _ptr(Rc.indices), _ptr(Fc.indptr), _ptr(Fc.indices),
                                   _ptr(fw), U, I, nF, PROFILE_MODES[mode], 1 if by_len else 0, _ptr(out_indptr), _ptr(out_indices),
                                   _ptr(out_vals), cap, C.c_void_p(ws.data_ptr()), need), "el_profile_build")
    indptr = out_indptr.cpu().numpy()
    nnz = int(indptr[-1])
    assert nnz <= cap
    return sp.csr_matrix((out_vals[:nnz].cpu().numpy(), out_indices[:nnz].cpu().numpy(), indptr), shape=(U, nF))


def kahfm_init(ctx, r_indptr, r_indices, F, f_weights, P0=None, Q0=None):
    """The start tables of KAHFMModel.initialize (kahfm_model.py:47-72) as device tensors (P0 [U, nF], Q0 [I, nF]) float64.
    r_indptr / r_indices: the train rows in train_dict order; F: scipy CSR [I, nF], the features of every item (its values are not
    read); f_weights: the float64 TF-IDF weight of every entry of F.  P0[u, f]: the weight of f in the last item of row u that
    carries it, divided by the row's length; Q0[i, f]: the weight.  P0 / Q0: tensors to fill instead of new ones."""
    _, Rc, Fc, fw = _feature_operands(ctx, "kahfm_init", r_indptr, r_indices, F, f_weights)
    U, (I, nF), dev = Rc.n_rows, F.shape, ctx.device
    if P0 is None:
        P0 = torch.empty((U, nF), dtype=torch.float64, device=dev)
    if Q0 is None:
        Q0 = torch.empty((I, nF), dtype=torch.float64, device=dev)
    if tuple(P0.shape) != (U, nF) or tuple(Q0.shape) != (I, nF):
        raise ValueError(f"kahfm_init: P0 {tuple(P0.shape)} / Q0 {tuple(Q0.shape)} do not fit ({U}, {nF}) / ({I}, {nF})")
    check(ctx.lib.el_kahfm_init(ctx.handle, ctx.stream(), _ptr(Rc.indptr), _ptr(Rc.indices), _ptr(Fc.indptr), _ptr(Fc.indices),
                                _ptr(fw), U, I, nF, _ptr(P0, torch.float64, "P0"), _ptr(Q0, torch.float64, "Q0")), "el_kahfm_init")
    torch.cuda.synchronize(dev)                     # the operands above are released on return
    return P0, Q0


def knn_build_f32(ctx, A, n_neighbors, sim):
    """Similarity.initialize of attribute_user_knn_similarity.py: W of the rows of A (scipy sparse [n, n_other], float32 values,
    explicit zeros kept), top-`n_neighbors` non-zeros per column, self-similarity kept.  fp64 sums in the stored (ascending)
    order of A's rows.  Returns (DeviceCSR W, float32 values tensor) as knn_build."""
    if sim not in KNN_SIMILARITIES:
        raise ValueError(f"similarity {sim!r} is not supported; supported: {sorted(KNN_SIMILARITIES)}")
    return _knn_w(ctx, "el_knn_build_f32", "el_knn_f32_ws_bytes", *_pair_operands(ctx, A, "rows")[:4], n_neighbors, sim)


# ------------------------------------------------------------------------------------------
# RP3beta (graph_based/RP3beta; beta = 0 is P3alpha)
# ------------------------------------------------------------------------------------------
RP3_ROWS_WS_BYTES = 1 << 28          # bound of el_rp3_rows' workspace: longer row ranges are built in pieces


def csr_row_l1(ctx, indptr, vals, n_rows=None):
    """sklearn's normalize(., 'l1') on the values of a device CSR (el_csr_row_l1): fp64 sequential row sums in stored order,
    out of place.  indptr int64 / vals float32 device tensors; returns the float32 values."""
    n = int(indptr.shape[0] - 1 if n_rows is None else n_rows)
    out = torch.empty_like(vals)
    if vals.shape[0] and n:
        check(ctx.lib.el_csr_row_l1(ctx.handle, ctx.stream(), _ptr(indptr, torch.int64, "indptr"), _ptr(vals, torch.float32, "vals"),
                                    n, _ptr(out, torch.float32, "out")), "el_csr_row_l1")
    return out


def _rp3_power(ctx, vals, alpha):
    """np.power on float32, on the host, exactly as the reference writes it (a device powf differs in the last bit)."""
    return torch.from_numpy(np.power(vals.cpu().numpy(), alpha)).to(ctx.device)


def rp3_operands(ctx, R, alpha, beta):
    """rp3beta.py:77-96: (Piu DeviceCSR [I, U], its values, Pui DeviceCSR [U, I], its values, degree fp64 [I]) on the device from a
    scipy [U, I] ratings matrix with any float values.  The row sums run over R's stored order; both CSRs come out with ascending
    columns.  The two powers (degree, alpha) are NumPy's, on float32 arrays on the host."""
    import scipy.sparse as sp
    alpha, beta = float(alpha), float(beta)                          # Python floats: a NumPy float64 scalar would promote the powers
    R = sp.csr_matrix(R, dtype=np.float32)
    U, I = R.shape
    dev = ctx.device
    pui_vals = csr_row_l1(ctx, torch.from_numpy(R.indptr.astype(np.int64)).to(dev), device_values(R.data, dev), U)
    indices = R.indices
    if not R.has_sorted_indices:                                     # the sums are taken; the order inside a row is free now
        rows = np.repeat(np.arange(U), np.diff(R.indptr))
        perm = np.lexsort((R.indices, rows))
        indices = R.indices[perm]
        pui_vals = pui_vals[torch.from_numpy(perm).to(dev)].contiguous()
    Pui = DeviceCSR(R.indptr, indices, I, dev)
    X = sp.csr_matrix((np.ones(R.nnz, np.float32), indices, R.indptr), shape=(U, I)).T.tocsr()
    X.sort_indices()
    Piu = DeviceCSR(X.indptr, X.indices, U, dev)
    piu_vals = csr_row_l1(ctx, Piu.indptr, device_values(X.data, dev), I)
    cnt = np.diff(X.indptr).astype(np.float32)                       # X_bool.sum(axis=1) of a float32 matrix
    degree = np.zeros(I)
    nz = cnt != 0.0
    degree[nz] = np.power(cnt[nz], -beta)
    if alpha != 1.:
        pui_vals, piu_vals = _rp3_power(ctx, pui_vals, alpha), _rp3_power(ctx, piu_vals, alpha)
    return Piu, piu_vals, Pui, pui_vals, torch.from_numpy(degree).to(dev)


def _rp3_n(n_neighbors, I):
    return int(I) if int(n_neighbors) == -1 else int(n_neighbors)


def rp3_rows(ctx, Piu, piu_vals, Pui, pui_vals, degree, n_neighbors, i_start=0, i_stop=None):
    """rp3beta.py:111-141 for the rows [i_start, i_stop) (el_rp3_rows): (idx int32 [n, N], val float32 [n, N], cnt int32 [n]) on the
    device, N = min(n_neighbors, I), every row's kept (column, value) pairs in rank order."""
    I, U = Piu.n_rows, Pui.n_rows
    n_neighbors = _rp3_n(n_neighbors, I)
    if n_neighbors < 1:
        raise ValueError("neighborhood must be >= 1 (or -1: every item)")
    i_stop = I if i_stop is None else int(i_stop)
    n, N = i_stop - int(i_start), min(n_neighbors, I)
    idx = torch.empty((max(n, 1), N), dtype=torch.int32, device=ctx.device)
    val = torch.empty((max(n, 1), N), dtype=torch.float32, device=ctx.device)
    cnt = torch.empty(max(n, 1), dtype=torch.int32, device=ctx.device)
    per_row = max(int(ctx.lib.el_rp3_ws_bytes(I, n_neighbors, 1)), 1)
    block = max(min(RP3_ROWS_WS_BYTES // per_row, n), 1)
    need = int(ctx.lib.el_rp3_ws_bytes(I, n_neighbors, block))
    ws = workspace(ctx, None, need, ctx.device)
    for r0 in range(0, n, block):
        r1 = min(r0 + block, n)
        check(ctx.lib.el_rp3_rows(ctx.handle, ctx.stream(), _ptr(Piu.indptr, torch.int64), _ptr(Piu.indices, torch.int32),
                                  _ptr(piu_vals, torch.float32), _ptr(Pui.indptr, torch.int64), _ptr(Pui.indices, torch.int32),
                                  _ptr(pui_vals, torch.float32), _ptr(degree, torch.float64, "degree"), I, U, n_neighbors,
                                  int(i_start) + r0, int(i_start) + r1, _ptr(idx[r0:], torch.int32), _ptr(val[r0:], torch.float32),
                                  _ptr(cnt[r0:], torch.int32), C.c_void_p(ws.data_ptr()), need), "el_rp3_rows")
    return idx[:n], val[:n], cnt[:n]


def rp3_cut(ctx, idx, val, cnt, n_neighbors, normalize):
    """rp3beta.py:143-174 on the row lists of all I rows (el_rp3_cut): (DeviceCSR W [I, I] columns ascending, float32 values), the
    shape knn_build returns."""
    I = int(cnt.shape[0])
    n_neighbors = _rp3_n(n_neighbors, I)
    N = min(n_neighbors, I)
    if idx.shape != (I, N) or val.shape != (I, N):
        raise ValueError(f"row lists must be [{I}, {N}], got {tuple(idx.shape)}")
    need = int(ctx.lib.el_rp3_ws_bytes(I, n_neighbors, 0))
    ws = workspace(ctx, None, need, ctx.device)
    w_indptr, w_indices, w_vals = _w_alloc(ctx, I, N)
    check(ctx.lib.el_rp3_cut(ctx.handle, ctx.stream(), _ptr(idx, torch.int32), _ptr(val, torch.float32), _ptr(cnt, torch.int32), I,
                             n_neighbors, 1 if normalize else 0, _ptr(w_indptr), _ptr(w_indices), _ptr(w_vals),
                             C.c_void_p(ws.data_ptr()), need), "el_rp3_cut")
    return _w_result(w_indptr, w_indices, w_vals)


def rp3_build(ctx, Piu, piu_vals, Pui, pui_vals, degree, n_neighbors, normalize):
    """W of RP3beta from finished operands (rp3_operands): rp3_rows + rp3_cut.  knn_score_topk(A = R, B = W) takes it directly."""
    idx, val, cnt = rp3_rows(ctx, Piu, piu_vals, Pui, pui_vals, degree, n_neighbors)
    return rp3_cut(ctx, idx, val, cnt, n_neighbors, normalize)


# ------------------------------------------------------------------------------------------
# SLIM (latent_factor_models/Slim): elastic-net coordinate descent per item
# ------------------------------------------------------------------------------------------
SLIM_EXCLUSIONS = {"column": _lib.EL_SLIM_COLUMN, "reference": _lib.EL_SLIM_REFERENCE}
SLIM_FIT_WS_BYTES = 1 << 28          # bound of el_slim_fit's workspace: longer column ranges are fitted in pieces
SLIM_MAX_ITER, SLIM_TOL = 100, 1e-4  # the ElasticNet arguments of slim_model.py:30-39


def slim_seed_state(seed):
    """The xorshift state sklearn draws for every fit of ElasticNet(random_state=seed)."""
    return int(np.random.RandomState(seed).randint(0, 2147483647))


def slim_order(ctx, seed_state, I, n_draws):
    """The coordinates sklearn's selection='random' visits (el_slim_order): int32 [n_draws] on the device."""
    order = torch.empty(max(int(n_draws), 1), dtype=torch.int32, device=ctx.device)
    check(ctx.lib.el_slim_order(ctx.handle, ctx.stream(), int(seed_state) & 0xffffffff, int(I), int(n_draws), _ptr(order, torch.int32)),
          "el_slim_order")
    return order[:int(n_draws)]


def slim_csc(ctx, R):
    """(DeviceCSR of the CSC of a scipy [U, I] matrix: row i = column i of R, its users ascending; float32 values)."""
    import scipy.sparse as sp
    X = sp.csc_matrix(R, dtype=np.float32)
    X.sum_duplicates()
    X.sort_indices()
    return DeviceCSR(X.indptr, X.indices, R.shape[0], ctx.device), device_values(X.data, ctx.device)


def slim_penalties(alpha, l1_ratio, U):
    """sklearn's l1_reg, l2_reg as the float32 solver receives them: the products in Python floats, rounded once."""
    alpha, l1_ratio = float(alpha), float(l1_ratio)
    return float(np.float32(alpha * l1_ratio * U)), float(np.float32(alpha * (1.0 - l1_ratio) * U))


def slim_fit(ctx, csc, csc_vals, alpha, l1_ratio, order, n_neighbors, j_start=0, j_stop=None, exclusion="column",
             max_iter=SLIM_MAX_ITER, tol=SLIM_TOL, coef=False, ws_bytes=None):
    """slim_model.py:58-92 for the target columns [j_start, j_stop) (el_slim_fit), in blocks that bound the workspace:
    (idx int32 [n, N], val float32 [n, N], cnt int32 [n], n_iter int32 [n]) on the device, N = min(n_neighbors, I); with coef=True
    also the dense weights before the cut, float32 [n, I] (tests).  ws_bytes: a workspace size to pass instead of the needed one."""
    if exclusion not in SLIM_EXCLUSIONS:
        raise ValueError(f"exclusion {exclusion!r} is not supported; supported: {sorted(SLIM_EXCLUSIONS)}")
    I, U = csc.n_rows, csc.n_cols
    n_neighbors = int(n_neighbors)
    if n_neighbors < 1:
        raise ValueError("neighborhood must be >= 1")
    if order.shape[0] < int(max_iter) * I:
        raise ValueError(f"order holds {order.shape[0]} draws, {int(max_iter) * I} needed")
    j_stop = I if j_stop is None else int(j_stop)
    n, N = j_stop - int(j_start), min(n_neighbors, I)
    l1, l2 = slim_penalties(alpha, l1_ratio, U)
    dev = ctx.device
    idx = torch.zeros((max(n, 1), N), dtype=torch.int32, device=dev)
    val = torch.zeros((max(n, 1), N), dtype=torch.float32, device=dev)
    cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    n_iter = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    dense = torch.zeros((max(n, 1), I), dtype=torch.float32, device=dev) if coef else None
    per_col = max(int(ctx.lib.el_slim_ws_bytes(U, I, 2, n_neighbors)) - int(ctx.lib.el_slim_ws_bytes(U, I, 1, n_neighbors)), 1)
    block = max(min(SLIM_FIT_WS_BYTES // per_col, n), 1)
    need = int(ctx.lib.el_slim_ws_bytes(U, I, block, n_neighbors))
    given = need if ws_bytes is None else int(ws_bytes)
    ws = workspace(ctx, None, given, ctx.device)
    for c0 in range(0, n, block):
        c1 = min(c0 + block, n)
        check(ctx.lib.el_slim_fit(ctx.handle, ctx.stream(), _ptr(csc.indptr, torch.int64), _ptr(csc.indices, torch.int32),
                                  _ptr(csc_vals, torch.float32), U, I, l1, l2, int(max_iter), float(tol), _ptr(order, torch.int32),
                                  SLIM_EXCLUSIONS[exclusion], int(j_start) + c0, int(j_start) + c1, n_neighbors,
                                  _ptr(idx[c0:], torch.int32), _ptr(val[c0:], torch.float32), _ptr(cnt[c0:], torch.int32),
                                  _ptr(n_iter[c0:], torch.int32), _ptr(dense[c0:], torch.float32) if coef else None,
                                  C.c_void_p(ws.data_ptr()), given), "el_slim_fit")
    out = (idx[:n], val[:n], cnt[:n], n_iter[:n])
    return out + (dense[:n],) if coef else out


def slim_w(ctx, idx, val, cnt):
    """slim_model.py:109 on the column lists of all I targets (el_slim_w): (DeviceCSR W [I, I] columns ascending, float32 values),
    the shape knn_build returns."""
    I, N = int(cnt.shape[0]), int(idx.shape[1])
    if idx.shape != (I, N) or val.shape != (I, N):
        raise ValueError(f"column lists must be [{I}, {N}], got {tuple(idx.shape)} / {tuple(val.shape)}")
    need = int(ctx.lib.el_slim_ws_bytes(I, I, 0, N))
    ws = workspace(ctx, None, need, ctx.device)
    w_indptr, w_indices, w_vals = _w_alloc(ctx, I, N)
    check(ctx.lib.el_slim_w(ctx.handle, ctx.stream(), _ptr(idx, torch.int32), _ptr(val, torch.float32), _ptr(cnt, torch.int32), I, N,
                            _ptr(w_indptr), _ptr(w_indices), _ptr(w_vals), C.c_void_p(ws.data_ptr()), need), "el_slim_w")
    return _w_result(w_indptr, w_indices, w_vals)


def slim_build(ctx, csc, csc_vals, alpha, l1_ratio, n_neighbors, seed, exclusion="column", max_iter=SLIM_MAX_ITER, tol=SLIM_TOL):
    """W of SLIM from the CSC of R (slim_csc): slim_order + slim_fit over every column + slim_w; also the sweeps per column.
    knn_score_topk(A = R, B = W) takes W directly."""
    I = csc.n_rows
    order = slim_order(ctx, slim_seed_state(seed), I, int(max_iter) * I)
    idx, val, cnt, n_iter = slim_fit(ctx, csc, csc_vals, alpha, l1_ratio, order, n_neighbors, exclusion=exclusion,
                                     max_iter=max_iter, tol=tol)
    W, w_vals = slim_w(ctx, idx, val, cnt)
    return W, w_vals, n_iter


# ------------------------------------------------------------------------------------------
# alternating least squares (iALS / WRMF)
# ------------------------------------------------------------------------------------------
ALS_PIECE_LEN = 8192          # rows longer than this are summed in pieces (el_als_solve's long-row plan)


def als_plan(indptr, piece_len=ALS_PIECE_LEN):
    """Host: the long-row plan of a CSR for el_als_solve -- (long_rows int32, long_first int64, n_pieces)."""
    lens = np.diff(np.asarray(indptr, dtype=np.int64))
    rows = np.flatnonzero(lens > piece_len).astype(np.int32)
    first = np.zeros(rows.shape[0] + 1, np.int64)
    np.cumsum((lens[rows] + piece_len - 1) // piece_len, out=first[1:])
    return rows, first, int(first[-1])


class AlsCSR:
    """One orientation of the train pattern for el_als_solve: the DeviceCSR plus its long-row plan."""

    def __init__(self, indptr, indices, n_cols, device, piece_len=ALS_PIECE_LEN):
        self.csr = DeviceCSR(indptr, indices, n_cols, device)
        rows, first, self.n_pieces = als_plan(indptr, piece_len)
        self.piece_len = int(piece_len)
        self.n_long = int(rows.shape[0])
        self.long_rows = torch.from_numpy(rows if rows.size else np.zeros(1, np.int32)).to(device)
        self.long_first = torch.from_numpy(first).to(device)
        self.empty = np.diff(np.asarray(indptr, dtype=np.int64)) == 0


def als_gram(ctx, Y, out=None, holder=None):
    """G = Y^T Y (fp64 [F, F], el_als_gram): fixed slots, symmetric bit for bit."""
    n, F = Y.shape
    if out is None:
        out = torch.empty((F, F), dtype=torch.float64, device=ctx.device)
    need = int(ctx.lib.el_als_gram_ws_bytes(int(n), int(F)))
    ws = _ptr(workspace(holder if holder is not None else ctx, "_als_gram_ws", need, ctx.device)) if need else None
    check(ctx.lib.el_als_gram(ctx.handle, ctx.stream(), _ptr(Y, torch.float64, "Y"), int(n), int(F), _ptr(out, torch.float64, "G"),
                              ws, need), "el_als_gram")
    return out


def als_solve(ctx, pattern, Y, G, w_A, w_b, lam, X, skip_empty=False, holder=None):
    """One ALS half-step (el_als_solve): X[r] = (G + w_A sum y y^T + lam I)^-1 (w_b sum y) for every row of `pattern` (AlsCSR over
    the rows of Y).  Raises numpy.linalg.LinAlgError naming the first row met with a non-positive pivot."""
    n_rows, F = X.shape
    if Y.shape[1] != F or tuple(G.shape) != (F, F):
        raise ValueError("X / Y / G factor mismatch")
    if pattern.csr.n_rows != n_rows or pattern.csr.n_cols != Y.shape[0]:
        raise ValueError("pattern shape does not match X / Y")
    holder = holder if holder is not None else ctx
    need = int(ctx.lib.el_als_solve_ws_bytes(int(pattern.n_pieces), int(F)))
    ws = _ptr(workspace(holder, "_als_solve_ws", need, ctx.device)) if need else None
    status = getattr(holder, "_als_status", None)
    if status is None:
        status = holder._als_status = torch.empty(2, dtype=torch.int32, device=ctx.device)
    check(ctx.lib.el_als_solve(ctx.handle, ctx.stream(), _ptr(pattern.csr.indptr, torch.int64), _ptr(pattern.csr.indices, torch.int32),
                               int(n_rows), _ptr(Y, torch.float64, "Y"), int(Y.shape[0]), int(F), _ptr(G, torch.float64, "G"),
                               float(w_A), float(w_b), float(lam), _lib.EL_ALS_SKIP_EMPTY if skip_empty else 0,
                               _ptr(pattern.long_rows, torch.int32), _ptr(pattern.long_first, torch.int64), pattern.n_long,
                               pattern.n_pieces, pattern.piece_len, _ptr(X, torch.float64, "X"), _ptr(status, torch.int32), ws, need),
          "el_als_solve")
    bad, plan = (int(v) for v in status.cpu().tolist())
    if plan != 0x7fffffff:
        raise _lib.ElliotHipError(f"el_als_solve: the long-row plan does not describe row {plan}")
    if bad != 0x7fffffff:
        raise np.linalg.LinAlgError(f"ALS: the normal equations of row {bad} are not positive definite (non-positive pivot)")
    return X


class AlsDeviceState:
    """X [U, F], Y [I, F] (fp64), both orientations of the train pattern and the two weights of iALS / WRMF in HBM.

    step() is one reference train_step: the user half with G = Y^T Y, then the item half --
      gram="fresh" (iALS, iALS_model.py:61): G = X^T X of the NEW X, empty items keep their row (warm items only, :37-38)
      gram="stale" (WRMF, wrmf_model.py:41-42): G = X^T X taken at the top of the step from the OLD X, every item solved."""

    def __init__(self, ctx, X, Y, indptr, indices, w_A, w_b, reg, gram="fresh", piece_len=ALS_PIECE_LEN):
        if gram not in ("fresh", "stale"):
            raise ValueError("gram must be 'fresh' (iALS) or 'stale' (WRMF)")
        self.ctx = ctx
        dev = ctx.device
        self.X, self.Y = _own(X, dev, torch.float64), _own(Y, dev, torch.float64)
        self.U, self.F = int(self.X.shape[0]), int(self.X.shape[1])
        self.I = int(self.Y.shape[0])
        if self.F > _lib.EL_ALS_MAX_F:
            raise ValueError(f"factors={self.F} unsupported (at most {_lib.EL_ALS_MAX_F})")
        import scipy.sparse as sp
        R = sp.csr_matrix((np.ones(len(indices), np.float32), np.asarray(indices), np.asarray(indptr)), shape=(self.U, self.I))
        R.sort_indices()
        Rt = R.T.tocsr()
        Rt.sort_indices()
        self.users = AlsCSR(R.indptr, R.indices, self.I, dev, piece_len)
        self.items = AlsCSR(Rt.indptr, Rt.indices, self.U, dev, piece_len)
        self.w_A, self.w_b, self.reg, self.gram = float(w_A), float(w_b), float(reg), gram
        self.Gy = torch.empty((self.F, self.F), dtype=torch.float64, device=dev)
        self.Gx = torch.empty((self.F, self.F), dtype=torch.float64, device=dev)
        self._zero_bias = None

    def user_half(self):
        als_gram(self.ctx, self.Y, out=self.Gy, holder=self)
        als_solve(self.ctx, self.users, self.Y, self.Gy, self.w_A, self.w_b, self.reg, self.X, holder=self)

    def item_half(self):
        als_gram(self.ctx, self.X, out=self.Gx, holder=self)
        als_solve(self.ctx, self.items, self.X, self.Gx, self.w_A, self.w_b, self.reg, self.Y, skip_empty=True, holder=self)

    def step(self):
        if self.gram == "fresh":
            self.user_half()
            self.item_half()
            return
        als_gram(self.ctx, self.Y, out=self.Gy, holder=self)
        als_gram(self.ctx, self.X, out=self.Gx, holder=self)
        als_solve(self.ctx, self.users, self.Y, self.Gy, self.w_A, self.w_b, self.reg, self.X, holder=self)
        als_solve(self.ctx, self.items, self.X, self.Gx, self.w_A, self.w_b, self.reg, self.Y, holder=self)

    def recommend(self, mask, k, start, stop):
        """X Y^T (fp64) for users [start, stop) and the masked top-k (el_score_topk_f64 with b = 0): (idx, val) on the device."""
        if self._zero_bias is None:
            self._zero_bias = torch.zeros(self.I, dtype=torch.float64, device=self.ctx.device)
        return score_topk_f64(self.ctx, self.X, self.Y, self._zero_bias, start, stop, k, **mask_kwargs(mask))

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by (el_score_rank_f64)."""
        if self._zero_bias is None:
            self._zero_bias = torch.zeros(self.I, dtype=torch.float64, device=self.ctx.device)
        return score_rank_f64(self.ctx, self.X, self.Y, self._zero_bias, start, stop, targets, **mask_kwargs(mask))


# ------------------------------------------------------------------------------------------
# what the dense item-item models (EASE^R, SlopeOne, BPRSlim) share: the memory guard and the blocked recommend()
# ------------------------------------------------------------------------------------------
SCORE_BLOCK_BYTES = 1 << 28          # bound of one [Ub, I] score block
EASE_SCORE_BLOCK_BYTES = SLOPE_SCORE_BLOCK_BYTES = BPRSLIM_SCORE_BLOCK_BYTES = SCORE_BLOCK_BYTES


def score_block_rows(I, U, itemsize):
    return min(max(SCORE_BLOCK_BYTES // (itemsize * max(int(I), 1)), 1), max(int(U), 1))


class _DenseScoreState:
    """A model that scores [Ub, I] blocks of SCORE_DTYPE (float32 | float64) with _score_block(s, e, out) and selects from them.
    A subclass sets ctx, U and I, then calls _guard_memory() before it allocates anything."""
    SCORE_DTYPE = torch.float64

    def _guard_memory(self, need, what):
        """ValueError naming the bytes when `need` exceeds the free device memory; what: the model's own sentence."""
        self.need = need
        free, _total = torch.cuda.mem_get_info(self.ctx.device)
        if need > free:
            raise ValueError(f"{what}; {free} bytes are free")
        self.block_rows = score_block_rows(self.I, self.U, self.SCORE_DTYPE.itemsize)
        self._S = None                            # the score block, allocated by the first recommend() from block_rows

    def recommend(self, mask, k, start, stop):
        """Top-k of users [start, stop) under the tagged mask ("excl" | "cand", DeviceCSR): (idx int32, val SCORE_DTYPE) [n, k]
        on the device; lists short of k are padded with (-1, -inf)."""
        ctx, dt = self.ctx, self.SCORE_DTYPE
        m = mask_kwargs(mask)
        (ep, ei), (cp, ci) = _csr_ptrs(m["excl"]), _csr_ptrs(m["cand"])
        sfx = "" if dt == torch.float32 else "_f64"
        topk, pad = getattr(ctx.lib, "el_dense_topk" + sfx), getattr(ctx.lib, "el_topk_pad" + sfx)
        start, stop = int(start), int(stop)
        n = stop - start
        out_idx = torch.empty((n, k), dtype=torch.int32, device=ctx.device)
        out_val = torch.empty((n, k), dtype=dt, device=ctx.device)
        if self._S is None:
            self._S = torch.empty((self.block_rows, self.I), dtype=dt, device=ctx.device)
        for s in range(start, stop, self.block_rows):
            e = min(s + self.block_rows, stop)
            self._score_block(s, e, self._S)
            check(topk(ctx.handle, ctx.stream(), _ptr(self._S, dt), int(self._S.stride(0)), s, e, int(self.I), ep, ei, cp,
                       ci, int(k), _ptr(out_idx[s - start:], torch.int32), _ptr(out_val[s - start:], dt)), "el_dense_topk" + sfx)
        check(pad(ctx.handle, ctx.stream(), _ptr(out_idx, torch.int32), _ptr(out_val, dt), int(n * k)), "el_topk_pad" + sfx)
        return out_idx, out_val

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the users' full rankings under the tagged mask
        (dense_rank / dense_rank_f64 on the blocks recommend() selects from): int32 on the device."""
        ctx, dt = self.ctx, self.SCORE_DTYPE
        fn = dense_rank if dt == torch.float32 else dense_rank_f64
        start, stop = int(start), int(stop)
        hp = _host_indptr(targets)
        pos = torch.empty(max(int(hp[stop] - hp[start]), 1), dtype=torch.int32, device=ctx.device)[:int(hp[stop] - hp[start])]
        if self._S is None:
            self._S = torch.empty((self.block_rows, self.I), dtype=dt, device=ctx.device)
        for s in range(start, stop, self.block_rows):
            e = min(s + self.block_rows, stop)
            self._score_block(s, e, self._S)
            fn(ctx, self._S, s, e, targets, pos=pos[int(hp[s] - hp[start]):int(hp[e] - hp[start])], I=self.I, **mask_kwargs(mask))
        return pos


# ------------------------------------------------------------------------------------------
# EASE^R (Gram, fp64 inverse, weights, CSR x dense scores)
# ------------------------------------------------------------------------------------------


def ease_integer_ratings(values):
    """(scale, int32 values) as knn_integer_ratings; EASER refuses anything else with its own message."""
    try:
        return knn_integer_ratings(values)
    except ValueError:
        raise ValueError("EASER needs integer or half-step ratings (the Gram counts are exact integers); "
                         "this train matrix holds other values") from None


def ease_gram(ctx, R, l2_norm, out=None):
    """ease_r.py:76-82: G = R^T R of a scipy [U, I] train matrix with the diagonal replaced by (float)(n_i + l2_norm), as an fp64
    [I, I] device tensor (el_ease_gram: exact integer counts)."""
    Tc, tvt, Rc, rvt, scale, max_deg, max_abs = _pair_operands(ctx, R, "cols", ease_integer_ratings)
    I, U, dev = Tc.n_rows, Tc.n_cols, ctx.device
    if out is None:
        out = torch.empty((I, I), dtype=torch.float64, device=dev)
    check(ctx.lib.el_ease_gram(ctx.handle, ctx.stream(), _ptr(Tc.indptr), _ptr(Tc.indices), _ptr(tvt), _ptr(Rc.indptr),
                               _ptr(Rc.indices), _ptr(rvt), int(I), int(U), int(scale), max_deg, max_abs, float(l2_norm),
                               _ptr(out, torch.float64, "G"), int(out.stride(0))), "el_ease_gram")
    return out


def inv_f64(ctx, A, ipiv=None, ws=None):
    """A <- A^-1 in place (el_inv_f64: LU with partial pivoting, fp64 MFMA updates).  Returns ipiv (int32 [n], 0-based, getrf
    order).  Raises numpy.linalg.LinAlgError naming the first column whose pivot is zero or NaN."""
    n = int(A.shape[0])
    if A.dim() != 2 or A.shape[1] != n:
        raise ValueError("inv_f64: A must be square")
    if ipiv is None:
        ipiv = torch.empty(n, dtype=torch.int32, device=ctx.device)
    status = torch.empty(1, dtype=torch.int32, device=ctx.device)
    need = int(ctx.lib.el_inv_f64_ws_bytes(n))
    if ws is None or ws.numel() < need:
        ws = workspace(ctx, None, need, ctx.device)
    check(ctx.lib.el_inv_f64(ctx.handle, ctx.stream(), _ptr(A, torch.float64, "A"), int(A.stride(0)), n, _ptr(ipiv, torch.int32), _ptr(status, torch.int32),
                             C.c_void_p(ws.data_ptr()), need), "el_inv_f64")
    bad = int(status.item())
    if bad != 0x7fffffff:
        raise np.linalg.LinAlgError(f"Singular matrix: the pivot of column {bad} is zero or NaN")
    return ipiv


def lu_f64(ctx, A, ipiv=None):
    """P A = L U in place (el_lu_f64, getrf): returns ipiv; raises LinAlgError as inv_f64."""
    n = int(A.shape[0])
    if A.dim() != 2 or A.shape[1] != n:
        raise ValueError("lu_f64: A must be square")
    if ipiv is None:
        ipiv = torch.empty(n, dtype=torch.int32, device=ctx.device)
    status = torch.empty(1, dtype=torch.int32, device=ctx.device)
    check(ctx.lib.el_lu_f64(ctx.handle, ctx.stream(), _ptr(A, torch.float64, "A"), int(A.stride(0)), n, _ptr(ipiv, torch.int32),
                            _ptr(status, torch.int32)), "el_lu_f64")
    bad = int(status.item())
    if bad != 0x7fffffff:
        raise np.linalg.LinAlgError(f"Singular matrix: the pivot of column {bad} is zero or NaN")
    return ipiv


def ease_weights(ctx, P, out=None):
    """ease_r.py:86-88: B = P / (-diag(P)) by columns with a zero diagonal, as float32 [I, I] (el_ease_weights)."""
    I = int(P.shape[0])
    if out is None:
        out = torch.empty((I, I), dtype=torch.float32, device=ctx.device)
    need = int(ctx.lib.el_ease_weights_ws_bytes(I))
    ws = workspace(ctx, None, need, ctx.device)
    check(ctx.lib.el_ease_weights(ctx.handle, ctx.stream(), _ptr(P, torch.float64, "P"), int(P.stride(0)), I,
                                  _ptr(out, torch.float32, "B"), int(out.stride(0)), C.c_void_p(ws.data_ptr()), need), "el_ease_weights")
    return out


def csr_dense_scores(ctx, R, R_vals, B, u_start, u_stop, out=None):
    """self._train.dot(B) (ease_r.py:93) for users [u_start, u_stop) in scipy's order: float32 [n, I] (el_csr_dense_scores)."""
    n, I = int(u_stop) - int(u_start), int(B.shape[1])
    if out is None:
        out = torch.empty((n, I), dtype=torch.float32, device=ctx.device)
    if out.shape[0] < n or out.shape[1] != I:
        raise ValueError("csr_dense_scores: the output block is smaller than [n, I]")
    check(ctx.lib.el_csr_dense_scores(ctx.handle, ctx.stream(), _ptr(R.indptr, torch.int64), _ptr(R.indices, torch.int32),
                                      _ptr(R_vals, torch.float32), int(u_start), int(u_stop),
                                      _rows_ptr(B, torch.float32, "B"), int(B.stride(0)), I, _rows_ptr(out, torch.float32, "S"),
                                      int(out.stride(0))), "el_csr_dense_scores")
    return out


def ease_memory_need(I, U):
    """Device bytes EaseDeviceState needs at its peak: G / P and the inverse's right-hand sides (8 I^2 each), B (4 I^2), one
    score block and the CSRs."""
    I, U = int(I), int(U)
    return 8 * I * I + 8 * I * I + 4 * I * I + score_block_rows(I, U, 4) * 4 * I


class EaseDeviceState(_DenseScoreState):
    """R (float32 CSR, stored order) and B (float32 [I, I]) of EASE^R in HBM.

    build() forms G (el_ease_gram), P = G^-1 (el_inv_f64), B (el_ease_weights) and frees G / P; recommend() scores blocks of at
    most EASE_SCORE_BLOCK_BYTES with el_csr_dense_scores and selects with el_dense_topk; lists short of k are padded with
    (-1, -inf) (el_topk_pad).  The device memory is checked before anything is allocated."""
    SCORE_DTYPE = torch.float32

    def __init__(self, ctx, R, l2_norm):
        import scipy.sparse as sp
        self.ctx = ctx
        R = sp.csr_matrix(R, dtype=np.float32)
        self.U, self.I = int(R.shape[0]), int(R.shape[1])
        self.l2_norm = float(l2_norm)
        need = ease_memory_need(self.I, self.U)
        self._guard_memory(need, f"EASER: {self.I} items need {need} bytes of device memory (G / P and the inverse's right-hand "
                                 f"sides 2 x {8 * self.I * self.I}, B {4 * self.I * self.I}, one score block)")
        ease_integer_ratings(R.data)
        self._host = R
        self.R = DeviceCSR(R.indptr, R.indices, self.I, ctx.device)
        self.R_vals = device_values(R.data, ctx.device)
        self.B = None

    def build(self):
        G = ease_gram(self.ctx, self._host, self.l2_norm)
        inv_f64(self.ctx, G)
        self.B = ease_weights(self.ctx, G)
        del G
        torch.cuda.empty_cache()
        return self.B

    def set_weights(self, B):
        B = np.ascontiguousarray(B, dtype=np.float32)
        if B.shape != (self.I, self.I):
            raise ValueError(f"EASER weights have shape {B.shape}, the model expects {(self.I, self.I)}")
        self.B = torch.from_numpy(B).to(self.ctx.device)

    def _score_block(self, s, e, out):
        csr_dense_scores(self.ctx, self.R, self.R_vals, self.B, s, e, out=out)


# ------------------------------------------------------------------------------------------
# SlopeOne (exact deviation build, scoring table, ordered fp64 scoring)
# ------------------------------------------------------------------------------------------
SLOPE_TILE = 8192                    # LDS cells per pass of k_slope_build over the catalogue (el_slope.hip)


def slope_integer_ratings(values):
    """(scale, int32 values) as knn_integer_ratings; SlopeOne refuses anything else with its own message."""
    try:
        return knn_integer_ratings(values)
    except ValueError:
        raise ValueError("SlopeOne needs integer or half-step ratings (the deviation sums are exact integers); "
                         "this train matrix holds other values") from None


def slope_build(ctx, R, freq=None, dev=None, table=True):
    """SlopeOneModel.initialize (slope_one_model.py:19-37) of a scipy [U, I] train matrix: (freq int32 [I, I], dev float64
    [I, I], T float64 [I, I] or None) on the device (el_slope_build).  freq and dev start from zero, where the reference starts
    them from np.empty and relies on fresh pages being zero.  A CSR R is brought to sorted rows in place, as by ease_gram."""
    Tc, tvt, Rc, rvt, scale, max_deg, max_abs = _pair_operands(ctx, R, "cols", slope_integer_ratings)
    I, U, d = Tc.n_rows, Tc.n_cols, ctx.device
    if freq is None:
        freq = torch.empty((I, I), dtype=torch.int32, device=d)
    if dev is None:
        dev = torch.empty((I, I), dtype=torch.float64, device=d)
    T = torch.empty((I, I), dtype=torch.float64, device=d) if table else None
    check(ctx.lib.el_slope_build(ctx.handle, ctx.stream(), _ptr(Tc.indptr), _ptr(Tc.indices), _ptr(tvt), _ptr(Rc.indptr),
                                 _ptr(Rc.indices), _ptr(rvt), int(I), int(U), int(scale), max_deg, max_abs,
                                 _ptr(freq, torch.int32, "freq"), int(freq.stride(0)), _ptr(dev, torch.float64, "dev"),
                                 int(dev.stride(0)), _ptr(T, torch.float64, "T"), int(I)), "el_slope_build")
    return freq, dev, T


def slope_table(ctx, freq, dev, out=None):
    """The scoring table of a (freq int32, dev float64) pair: T[j, i] = dev[i, j] where freq[i, j] > 0, NaN elsewhere
    (el_slope_table)."""
    I = int(freq.shape[0])
    if out is None:
        out = torch.empty((I, I), dtype=torch.float64, device=ctx.device)
    check(ctx.lib.el_slope_table(ctx.handle, ctx.stream(), _rows_ptr(freq, torch.int32, "freq"), int(freq.stride(0)),
                                 _rows_ptr(dev, torch.float64, "dev"), int(dev.stride(0)), I, _rows_ptr(out, torch.float64, "T"),
                                 int(out.stride(0))), "el_slope_table")
    return out


def slope_scores(ctx, rows, user_mean, T, u_start, u_stop, out=None):
    """SlopeOneModel.predict (slope_one_model.py:42-47) for users [u_start, u_stop) and every item: float64 [n, I]
    (el_slope_scores).  rows: the train matrix as a DeviceCSR in dict order; user_mean: float64 [U] on the device."""
    n, I = int(u_stop) - int(u_start), int(T.shape[1])
    if out is None:
        out = torch.empty((n, I), dtype=torch.float64, device=ctx.device)
    if out.shape[0] < n or out.shape[1] != I:
        raise ValueError("slope_scores: the output block is smaller than [n, I]")
    check(ctx.lib.el_slope_scores(ctx.handle, ctx.stream(), _ptr(rows.indptr, torch.int64), _ptr(rows.indices, torch.int32),
                                  _ptr(user_mean, torch.float64, "user_mean"), int(u_start), int(u_stop),
                                  _rows_ptr(T, torch.float64, "T"), int(T.stride(0)), I, _rows_ptr(out, torch.float64, "P"),
                                  int(out.stride(0))), "el_slope_scores")
    return out


def dense_topk_f64(ctx, preds, u_start, u_stop, k, excl=None, cand=None, out_idx=None, out_val=None, pad=False):
    """dense_topk over a float64 [n_users, I] block: (idx int32 [n, k], val float64 [n, k]) by (value desc, index asc)
    (el_dense_topk_f64).  pad: entries at -inf become (-1, -inf) (el_topk_pad_f64)."""
    n, I = int(u_stop) - int(u_start), int(preds.shape[1])
    if preds.shape[0] < n:
        raise ValueError("preds rows must cover u_stop - u_start")
    out_idx, out_val, tail = _topk_io(ctx, n, k, torch.float64, excl, cand, out_idx, out_val)
    check(ctx.lib.el_dense_topk_f64(ctx.handle, ctx.stream(), _ptr(preds, torch.float64, "preds"), int(preds.stride(0)),
                                    int(u_start), int(u_stop), I, *tail), "el_dense_topk_f64")
    if pad:
        check(ctx.lib.el_topk_pad_f64(ctx.handle, ctx.stream(), _ptr(out_idx, torch.int32), _ptr(out_val, torch.float64),
                                      int(n * k)), "el_topk_pad_f64")
    return out_idx, out_val


def slope_user_mean(indptr, ratings):
    """np.mean of every user's train ratings (slope_one_model.py:40) on the host: the exact sum (integer or half-step ratings)
    and one fp64 division; nan for a user without ratings, as np.mean of nothing."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ratings = np.asarray(ratings, dtype=np.float64)
    n = np.diff(indptr)
    users = np.repeat(np.arange(n.shape[0]), n)
    s2 = np.bincount(users, weights=ratings * 2.0, minlength=n.shape[0])       # integers: exact in any order
    with np.errstate(divide="ignore", invalid="ignore"):
        return (s2 * 0.5) / n


def slope_block_rows(I, U):
    return score_block_rows(I, U, 8)


def slope_memory_need(I, U):
    """Device bytes SlopeDeviceState needs: freq (4 I^2), dev and T (8 I^2 each) and one float64 score block."""
    I, U = int(I), int(U)
    return 4 * I * I + 8 * I * I + 8 * I * I + slope_block_rows(I, U) * 8 * I


class SlopeDeviceState(_DenseScoreState):
    """The train matrix in dict order (DeviceCSR), user_mean, freq (int32), dev and the scoring table T (float64 [I, I]) of
    SlopeOne in HBM.

    build() forms freq, dev and T (el_slope_build); set_model() takes a restored (freq, dev, user_mean) and forms T from it
    (el_slope_table); recommend() scores blocks of at most SLOPE_SCORE_BLOCK_BYTES with el_slope_scores and selects with
    el_dense_topk_f64; lists short of k are padded with (-1, -inf).  The device memory is checked before anything is allocated.

    R: scipy [U, I] train matrix with the ratings; rows: (indptr, indices) of the same matrix in the order of the reference's
    train dict (DataSet.dict_order_csr) -- the order the prediction's sum runs in."""

    def __init__(self, ctx, R, rows):
        import scipy.sparse as sp
        self.ctx = ctx
        R = sp.csr_matrix(R, dtype=np.float64)
        self.U, self.I = int(R.shape[0]), int(R.shape[1])
        need = slope_memory_need(self.I, self.U)
        self._guard_memory(need, f"SlopeOne: {self.I} items need {need} bytes of device memory (freq {4 * self.I * self.I}, dev "
                                 f"and the scoring table 2 x {8 * self.I * self.I}, one score block)")
        slope_integer_ratings(R.data)
        indptr, indices = rows
        indptr = np.asarray(indptr, dtype=np.int64)
        if indptr.shape[0] != self.U + 1 or int(indptr[-1]) != R.nnz:
            raise ValueError("SlopeOne: the dict-order rows do not describe the train matrix")
        self._host = R
        self.rows = DeviceCSR(indptr, indices, self.I, ctx.device)
        users = np.repeat(np.arange(self.U), np.diff(indptr))
        ratings = np.asarray(R[users, np.asarray(indices, dtype=np.int64)], dtype=np.float64).ravel() if R.nnz else np.zeros(0)
        self.user_mean_host = slope_user_mean(indptr, ratings)
        self.user_mean = torch.from_numpy(self.user_mean_host).to(ctx.device)
        self.freq = self.dev = self.T = None

    def build(self):
        self.freq, self.dev, self.T = slope_build(self.ctx, self._host)
        return self.freq, self.dev

    def set_model(self, freq, dev, user_mean):
        freq, dev = np.asarray(freq), np.ascontiguousarray(dev, dtype=np.float64)
        mean = np.ascontiguousarray(np.asarray(user_mean, dtype=np.float64))
        if freq.shape != (self.I, self.I) or dev.shape != (self.I, self.I) or mean.shape != (self.U,):
            raise ValueError(f"SlopeOne state has shapes {freq.shape}, {dev.shape}, {mean.shape}; the model expects "
                             f"{(self.I, self.I)} twice and {(self.U,)}")
        self.freq = torch.from_numpy(np.ascontiguousarray(freq, dtype=np.int32)).to(self.ctx.device)
        self.dev = torch.from_numpy(dev).to(self.ctx.device)
        self.user_mean_host = mean
        self.user_mean = torch.from_numpy(mean).to(self.ctx.device)
        self.T = slope_table(self.ctx, self.freq, self.dev)

    def recommend(self, mask, k, start, stop):
        if self.T is None:
            raise _lib.ElliotHipError("SlopeOne: recommend() before build() or set_model()")
        return super().recommend(mask, k, start, stop)

    def rank(self, mask, targets, start, stop):
        if self.T is None:
            raise _lib.ElliotHipError("SlopeOne: rank() before build() or set_model()")
        return super().rank(mask, targets, start, stop)

    def _score_block(self, s, e, out):
        slope_scores(self.ctx, self.rows, self.user_mean, self.T, s, e, out=out)


# ------------------------------------------------------------------------------------------
# BPRSlim (per-triplet BPR SGD on a dense fp64 item-item matrix, ordered fp64 scoring)
# ------------------------------------------------------------------------------------------
def _levels_host(fn, ids, sizes):
    """(order int32 [n], level_start int64 [n_levels + 1]) from one of the el_*_levels_host entry points: the id arrays (int32,
    contiguous, of one length), n, the table sizes, then the outputs."""
    n = ids[0].shape[0]
    order = np.empty(n, dtype=np.int32)
    starts = np.empty(n + 2, dtype=np.int64)
    nl = C.c_int64()
    check(getattr(_lib.load(), fn)(*(a.ctypes.data_as(C.c_void_p) for a in ids), n, *(int(x) for x in sizes),
                                   order.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p), n + 2, C.byref(nl)), fn)
    return order, starts[: nl.value + 1].copy()


def bprslim_levels(i_host, j_host, I):
    """Host-only: (order int32 [n], level_start int64 [n_levels + 1]) of a BPRSlim triplet sequence (el_bprslim_levels_host).
    A triplet depends on the last earlier one that shares row i or row j of S; the user is no dependency."""
    i = np.ascontiguousarray(i_host, dtype=np.int32).reshape(-1)
    j = np.ascontiguousarray(j_host, dtype=np.int32).reshape(-1)
    if i.shape != j.shape:
        raise ValueError("bprslim_levels: i and j differ in length")
    return _levels_host("el_bprslim_levels_host", (i, j), (I,))


def _bprslim_matrix(S, I, name):
    """(I, leading dimension) of a contiguous float64 [rows >= I, ld >= I] device tensor that holds an [I, I] matrix."""
    I = int(S.shape[1] if I is None else I)
    if S.dim() != 2 or S.shape[0] < I or S.shape[1] < I:
        raise ValueError(f"{name}: a [{I}, {I}] matrix does not fit a tensor of shape {tuple(S.shape)}")
    return I, int(S.stride(0))


def bprslim_apply(ctx, u, i, j, rows, S, lr, li_reg, lj_reg, first=0, n=None, I=None, x_out=None, g_out=None, level_start=None):
    """BPRSlimModel.train_step (bprslim_model.py:36-67) for the device triplets [first, first + n), concurrently
    (el_bprslim_apply); with level_start (int64 host array) one launch per level instead (el_bprslim_apply_levels).
    rows: the train matrix as a DeviceCSR; S: float64 device tensor holding the [I, I] matrix in its leading rows and columns;
    x_out / g_out: optional float64 [>= number of triplets], the sum and the gradient of every triplet."""
    I, lds = _bprslim_matrix(S, I, "bprslim_apply")
    total = int(u.numel())
    if int(i.numel()) != total or int(j.numel()) != total:
        raise ValueError("bprslim_apply: u, i and j differ in length")
    for name, t in (("x_out", x_out), ("g_out", g_out)):
        if t is not None and int(t.numel()) < total:
            raise ValueError(f"bprslim_apply: {name} holds fewer than {total} values")
    tail = (_ptr(rows.indptr, torch.int64), _ptr(rows.indices, torch.int32), int(rows.n_rows), _ptr(S, torch.float64, "S"), lds, I,
            float(lr), float(li_reg), float(lj_reg), _ptr(x_out, torch.float64, "x_out"), _ptr(g_out, torch.float64, "g_out"))
    head = (ctx.handle, ctx.stream(), _ptr(u, torch.int32, "u"), _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"))
    if level_start is not None:
        starts = np.ascontiguousarray(level_start, dtype=np.int64)
        if starts.shape[0] < 1 or int(starts[-1]) > total or np.any(np.diff(starts) < 0) or int(starts[0]) < 0:
            raise ValueError("bprslim_apply: the level table does not describe the triplet arrays")
        check(ctx.lib.el_bprslim_apply_levels(*head, starts.ctypes.data_as(C.c_void_p), int(starts.shape[0] - 1), *tail),
              "el_bprslim_apply_levels")
        return
    n = total - int(first) if n is None else int(n)
    if first < 0 or n < 0 or first + n > total:
        raise ValueError(f"bprslim_apply: triplets [{first}, {first + n}) of {total}")
    check(ctx.lib.el_bprslim_apply(*head, int(first), n, *tail), "el_bprslim_apply")


def bprslim_table(ctx, S, out=None, I=None):
    """St[s, i] = S[i, s] (el_bprslim_table): the table el_bprslim_scores reads."""
    I, lds = _bprslim_matrix(S, I, "bprslim_table")
    if out is None:
        out = torch.empty((I, I), dtype=torch.float64, device=ctx.device)
    _, ldt = _bprslim_matrix(out, I, "bprslim_table")
    check(ctx.lib.el_bprslim_table(ctx.handle, ctx.stream(), _ptr(S, torch.float64, "S"), lds, I, _ptr(out, torch.float64, "St"),
                                   ldt), "el_bprslim_table")
    return out


def bprslim_scores(ctx, rows, St, u_start, u_stop, out=None, I=None):
    """BPRSlimModel.predict (bprslim_model.py:69-84) for users [u_start, u_stop) and every item: float64 [n, I]
    (el_bprslim_scores).  rows: the train matrix as a DeviceCSR, summed in its stored order."""
    I, ldt = _bprslim_matrix(St, I, "bprslim_scores")
    n = int(u_stop) - int(u_start)
    if u_start < 0 or n < 0 or u_stop > rows.n_rows:
        raise ValueError(f"bprslim_scores: users [{u_start}, {u_stop}) of {rows.n_rows}")
    if out is None:
        out = torch.empty((n, I), dtype=torch.float64, device=ctx.device)
    if out.shape[0] < n or out.shape[1] < I:
        raise ValueError("bprslim_scores: the output block is smaller than [n, I]")
    check(ctx.lib.el_bprslim_scores(ctx.handle, ctx.stream(), _ptr(rows.indptr, torch.int64), _ptr(rows.indices, torch.int32),
                                    int(u_start), int(u_stop), _ptr(St, torch.float64, "St"), ldt, I,
                                    _ptr(out, torch.float64, "P"), int(out.stride(0))), "el_bprslim_scores")
    return out


def bprslim_block_rows(I, U):
    return score_block_rows(I, U, 8)


def bprslim_memory_need(I, U):
    """Device bytes BprSlimDeviceState needs: S and the scoring table St (8 I^2 each) and one float64 score block."""
    I, U = int(I), int(U)
    return 8 * I * I + 8 * I * I + bprslim_block_rows(I, U) * 8 * I


class BprSlimDeviceState(_DenseScoreState):
    """The train matrix (DeviceCSR, rows in the order the reference's scipy matrix stores them: ascending item id), the dense
    item-item matrix S and its transposed scoring table St (float64 [I, I]) of BPRSlim in HBM.

    S starts as zero (the reference starts it from np.empty).  apply_sequential_equivalent() applies a triplet sequence in
    dependency levels (el_bprslim_levels_host, el_bprslim_apply_levels); set_model() takes a restored S; recommend() rebuilds St
    when S has moved (el_bprslim_table), scores blocks of at most BPRSLIM_SCORE_BLOCK_BYTES with el_bprslim_scores and selects
    with el_dense_topk_f64; lists short of k are padded with (-1, -inf).  The device memory is checked before anything is
    allocated."""

    def __init__(self, ctx, R, lr, li_reg, lj_reg):
        import scipy.sparse as sp
        self.ctx = ctx
        self.U, self.I = int(R.shape[0]), int(R.shape[1])
        need = bprslim_memory_need(self.I, self.U)
        self._guard_memory(need, f"BPRSlim: {self.I} items need {need} bytes of device memory (S and the scoring table 2 x "
                                 f"{8 * self.I * self.I}, one score block)")
        R = sp.csr_matrix(R)
        if not R.has_canonical_format:
            R = R.copy()
            R.sum_duplicates()
        self.lr, self.li_reg, self.lj_reg = float(lr), float(li_reg), float(lj_reg)
        self.rows = DeviceCSR(np.asarray(R.indptr, dtype=np.int64), R.indices, self.I, ctx.device)
        self.S = torch.zeros((self.I, self.I), dtype=torch.float64, device=ctx.device)
        self.St = None                                # rebuilt from S by the first recommend() after S has moved

    def apply_sequential_equivalent(self, u_host, i_host, j_host):
        """The sequential order of BPRSlimModel.train_step on these triplets: (n_levels, x) with x the float64 host array of
        every triplet's sum x_uij in the order given."""
        u, i, j = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (u_host, i_host, j_host))
        n = u.shape[0]
        if n and (u.min() < 0 or u.max() >= self.U or min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= self.I):
            raise ValueError("BPRSlim: a triplet is out of range")
        if n == 0:
            return 0, np.zeros(0, dtype=np.float64)
        order, starts = bprslim_levels(i, j, self.I)
        dev = self.ctx.device
        du, di, dj = (torch.from_numpy(np.ascontiguousarray(a[order])).to(dev) for a in (u, i, j))
        x_dev = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        bprslim_apply(self.ctx, du, di, dj, self.rows, self.S, self.lr, self.li_reg, self.lj_reg, x_out=x_dev, level_start=starts)
        self.St = None
        x = np.empty(n, dtype=np.float64)
        x[order] = x_dev[:n].cpu().numpy()
        return int(starts.shape[0] - 1), x

    def set_model(self, S):
        S = np.ascontiguousarray(S, dtype=np.float64)
        if S.shape != (self.I, self.I):
            raise ValueError(f"BPRSlim state has shape {S.shape}; the model expects {(self.I, self.I)}")
        self.S.copy_(torch.from_numpy(S))
        self.St = None

    def _score_block(self, s, e, out):
        if self.St is None:
            self.St = bprslim_table(self.ctx, self.S)
        bprslim_scores(self.ctx, self.rows, self.St, s, e, out=out)


# ------------------------------------------------------------------------------------------
# PureSVD (randomized truncated SVD: CSR x dense fp64, Gram, Cholesky-QR2, projection)
# ------------------------------------------------------------------------------------------
PSVD_PIECE_LEN = 2048         # rows longer than this are summed in pieces (el_spmm_csr_f64's long-row plan)
PSVD_OVERSAMPLES = 10         # sklearn's n_oversamples default
PSVD_NONE = 0x7fffffff


class SpmmCSR:
    """One orientation of a sparse matrix for el_spmm_csr_f64: DeviceCSR, values (None: all ones) and the long-row plan."""

    def __init__(self, indptr, indices, n_cols, device, vals=None, piece_len=PSVD_PIECE_LEN):
        self.csr = DeviceCSR(indptr, indices, n_cols, device)
        self.vals = None if vals is None else device_values(vals, device)
        rows, first, self.n_pieces = als_plan(indptr, piece_len)
        self.piece_len = int(piece_len)
        self.n_long = int(rows.shape[0])
        self.long_rows = torch.from_numpy(rows if rows.size else np.zeros(1, np.int32)).to(device)
        self.long_first = torch.from_numpy(first).to(device)
        self.n_rows, self.n_cols, self.nnz = self.csr.n_rows, self.csr.n_cols, self.csr.nnz


def _rows_ptr(t, dtype, name):
    """Pointer of a 2-D device tensor whose rows may be strided (unit column stride): the kernels take a leading dimension."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.ElliotHipError(f"{name}: expected a tensor on the GPU")
    if t.dtype != dtype or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
        raise TypeError(f"{name}: expected a 2-D {dtype} tensor with unit column stride")
    return C.c_void_p(t.data_ptr())


def spmm_csr_f64(ctx, A, X, out=None, holder=None, verify=True):
    """Y = A X (el_spmm_csr_f64) for a SpmmCSR A and an fp64 [n_cols, R] device tensor X (rows may be strided): stored order inside
    a row, long rows in pieces.  verify: read the status back and raise on a plan or column-index fault."""
    R = int(X.shape[1])
    if X.shape[0] != A.n_cols:
        raise ValueError(f"spmm_csr_f64: X has {X.shape[0]} rows, the matrix {A.n_cols} columns")
    if out is None:
        out = torch.empty((A.n_rows, R), dtype=torch.float64, device=ctx.device)
    holder = holder if holder is not None else ctx
    need = int(ctx.lib.el_spmm_csr_f64_ws_bytes(int(A.n_pieces), R))
    ws = _ptr(workspace(holder, "_spmm64_ws", need, ctx.device)) if need else None
    status = getattr(holder, "_spmm64_status", None)
    if status is None:
        status = holder._spmm64_status = torch.empty(2, dtype=torch.int32, device=ctx.device)
    check(ctx.lib.el_spmm_csr_f64(ctx.handle, ctx.stream(), _ptr(A.csr.indptr, torch.int64), _ptr(A.csr.indices, torch.int32),
                                  _ptr(A.vals, torch.float32) if A.vals is not None else None, int(A.n_rows), int(A.n_cols),
                                  _rows_ptr(X, torch.float64, "X"), int(X.stride(0)), R, _rows_ptr(out, torch.float64, "Y"),
                                  int(out.stride(0)),
                                  _ptr(A.long_rows, torch.int32), _ptr(A.long_first, torch.int64), A.n_long, A.n_pieces,
                                  A.piece_len, _ptr(status, torch.int32), ws, need), "el_spmm_csr_f64")
    if verify:
        plan, col = (int(v) for v in status.cpu().tolist())
        if plan != PSVD_NONE:
            raise _lib.ElliotHipError(f"el_spmm_csr_f64: the long-row plan does not describe row {plan}")
        if col != PSVD_NONE:
            raise _lib.ElliotHipError(f"el_spmm_csr_f64: row {col} holds a column index outside the matrix")
    return out


def gram_f64(ctx, Y, out=None, holder=None):
    """G = Y^T Y (fp64 [R, R], el_gram_f64): the fp64 matrix instruction, fixed slots, symmetric bit for bit."""
    n, R = int(Y.shape[0]), int(Y.shape[1])
    if out is None:
        out = torch.empty((R, R), dtype=torch.float64, device=ctx.device)
    need = int(ctx.lib.el_gram_f64_ws_bytes(n, R))
    ws = _ptr(workspace(holder if holder is not None else ctx, "_gram64_ws", need, ctx.device)) if need else None
    check(ctx.lib.el_gram_f64(ctx.handle, ctx.stream(), _rows_ptr(Y, torch.float64, "Y"), int(Y.stride(0)), n, R,
                              _ptr(out, torch.float64, "G"), int(out.stride(0)), ws, need), "el_gram_f64")
    return out


def psvd_orth(ctx, Y, holder=None, status=None):
    """Orthonormalise the columns of fp64 Y [n, R] in place (el_psvd_orth: Cholesky-QR twice).  Returns the device status tensor
    (int32[1]: the smallest refused column, 0x7fffffff = none); reading it is the caller's synchronisation."""
    n, R = int(Y.shape[0]), int(Y.shape[1])
    holder = holder if holder is not None else ctx
    need = int(ctx.lib.el_psvd_orth_ws_bytes(n, R))
    ws = _ptr(workspace(holder, "_orth_ws", need, ctx.device)) if need else None
    if status is None:
        status = torch.empty(1, dtype=torch.int32, device=ctx.device)
    check(ctx.lib.el_psvd_orth(ctx.handle, ctx.stream(), _rows_ptr(Y, torch.float64, "Y"), int(Y.stride(0)), n, R,
                               _ptr(status, torch.int32), ws, need), "el_psvd_orth")
    return status


def psvd_project(ctx, Y, W, col_scale=None, out64=None, out32=None, f64=True, f32=False):
    """T = (Y W) diag(col_scale) (el_psvd_project) for fp64 Y [n, R] and W [R, k]: (T64 or None, T32 or None), each rounded once."""
    n, R = int(Y.shape[0]), int(Y.shape[1])
    k = int(W.shape[1])
    if W.shape[0] != R:
        raise ValueError("psvd_project: Y / W inner dimensions differ")
    if out64 is None and f64:
        out64 = torch.empty((n, k), dtype=torch.float64, device=ctx.device)
    if out32 is None and f32:
        out32 = torch.empty((n, k), dtype=torch.float32, device=ctx.device)
    check(ctx.lib.el_psvd_project(ctx.handle, ctx.stream(), _rows_ptr(Y, torch.float64, "Y"), int(Y.stride(0)), n, R,
                                  _rows_ptr(W, torch.float64, "W"), int(W.stride(0)), k, _ptr(col_scale, torch.float64, "col_scale"),
                                  _rows_ptr(out64, torch.float64, "T64"), int(out64.stride(0)) if out64 is not None else 0,
                                  _rows_ptr(out32, torch.float32, "T32"), int(out32.stride(0)) if out32 is not None else 0),
          "el_psvd_project")
    return out64, out32


def psvd_signs(ctx, T, holder=None):
    """svd_flip's signs of the columns of fp64 T [n, k] (el_psvd_signs): a device tensor double[k] of +-1."""
    n, k = int(T.shape[0]), int(T.shape[1])
    signs = torch.empty(k, dtype=torch.float64, device=ctx.device)
    need = int(ctx.lib.el_psvd_signs_ws_bytes(n, k))
    ws = _ptr(workspace(holder if holder is not None else ctx, "_signs_ws", need, ctx.device)) if need else None
    check(ctx.lib.el_psvd_signs(ctx.handle, ctx.stream(), _rows_ptr(T, torch.float64, "T"), int(T.stride(0)), n, k,
                                _ptr(signs, torch.float64), ws, need), "el_psvd_signs")
    return signs


def psvd_plan(U, I, factors):
    """The shape rules of sklearn's randomized_svd at its defaults and this library's refusals: (R, n_iter, transposed).
    transposed: the method runs on A^T (more items than users)."""
    U, I = int(U), int(I)
    try:
        f = int(factors)
    except (TypeError, ValueError):
        raise ValueError(f"PureSVD: factors={factors!r} is not an integer") from None
    if f != factors or f < 1:
        raise ValueError(f"PureSVD: factors={factors!r} must be an integer >= 1")
    R = f + PSVD_OVERSAMPLES
    if R > _lib.EL_PSVD_MAX_R:
        raise ValueError(f"PureSVD: factors={f} needs a table of factors + {PSVD_OVERSAMPLES} = {R} columns; the kernels hold at most "
                         f"{_lib.EL_PSVD_MAX_R} (factors <= {_lib.EL_PSVD_MAX_R - PSVD_OVERSAMPLES})")
    if R > min(U, I):
        raise ValueError(f"PureSVD: factors + {PSVD_OVERSAMPLES} = {R} exceeds min(users, items) = {min(U, I)}: the basis would be "
                         f"thinner than the method asks for (the reference degrades there; this implementation refuses)")
    n_iter = 7 if f < 0.1 * min(U, I) else 4
    return R, n_iter, U < I


def psvd_check_rank(col, R):
    """The status of el_psvd_orth as the model's refusal: a set status names the column whose pivot was refused (NaN, not positive,
    or small against its diagonal entry: rank deficiency, or a condition number beyond what Cholesky-QR2 is proved for)."""
    if int(col) != PSVD_NONE:
        raise ValueError(f"PureSVD: the orthonormalisation refused the pivot of column {int(col)} of {int(R)} (relative test: not "
                         f"above 8 (n R + R (R + 1)) 2^-53 times its diagonal entry): the train matrix has numerical rank below "
                         f"factors + {PSVD_OVERSAMPLES} = {int(R)}, or its power iterates are too ill-conditioned for Cholesky-QR "
                         f"(the reference's LU / QR normalisers tolerate both)")


def psvd_start_matrix(n, R, seed):
    """The reference's only randomness: RandomState(seed).normal(size=(n, R)) rounded to float32 (its matrix is float32), as fp64."""
    return np.random.RandomState(seed).normal(size=(int(n), int(R))).astype(np.float32).astype(np.float64)


def psvd_small_svd(G, factors, transposed):
    """Host step: from G = Z^T Z (R x R, symmetric) the leading eigenpairs by numpy.linalg.eigh -> (s, W_user, W_item), the
    singular values and the two [R, factors] matrices that turn the orthonormal basis Q and Z = M^T Q into the tables:
    not transposed  user = Q U^,       item = Z U^            (U = Q U^, diag(s) Vt = (Z U^)^T)
    transposed      user = Z U^ / s,   item = Q U^ s."""
    lam, vec = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    order = np.argsort(lam)[::-1][:int(factors)]
    s = np.sqrt(np.maximum(lam[order], 0.0))
    Uh = np.ascontiguousarray(vec[:, order])
    if not transposed:
        return s, Uh, Uh.copy()
    return s, np.ascontiguousarray(Uh / s[None, :]), np.ascontiguousarray(Uh * s[None, :])


def psvd_memory_need(U, I, nnz, factors, n_long=0, n_pieces=0):
    """Device bytes PureSvdDeviceState needs at its peak: both orientations of the pattern with their long-row plans (n_long long
    rows in all), the two R-wide fp64 tables, the product's piece slots (n_pieces: the larger orientation's), the Gram /
    orthonormalisation workspace, the fp64 user-side projection the signs are read from with its block maxima, the float32 tables."""
    U, I, nnz, f = int(U), int(I), int(nnz), int(factors)
    R = f + PSVD_OVERSAMPLES
    csr = 2 * (4 * nnz) + 8 * (U + I + 2) + 12 * (int(n_long) + 2)
    tables = 8 * R * (U + I)
    slots = min(max((max(U, I) + 1023) // 1024, 1), 256)
    ws = 8 * R * R * (slots + 3) + 8 * R * int(n_pieces) + 8 * f * ((U + 511) // 512)
    out = 8 * f * U + 4 * f * (U + I)
    return csr + tables + ws + out


class PureSvdDeviceState:
    """The PureSVD tables (float32 user_vec [U, factors], item_vec [I, factors]) in HBM.

    build() restates sklearn's randomized_svd at its defaults: the host draws the Gaussian start matrix exactly as the reference
    does, the device runs the power iterations (el_spmm_csr_f64 + el_psvd_orth instead of the LU / QR normalisers), the host
    takes the R x R eigenproblem of Z^T Z (numpy.linalg.eigh), the device projects (el_psvd_project) and flips the signs
    (el_psvd_signs).  The train pattern is on the device, in both orientations, for the build only.  recommend() is el_score_topk with a
    zero bias and el_topk_pad.  The device memory is checked first."""

    def __init__(self, ctx, sp_i_train, factors, seed, piece_len=PSVD_PIECE_LEN):
        import scipy.sparse as sp
        self.ctx = ctx
        A = sp.csr_matrix(sp_i_train, dtype=np.float32)
        self.U, self.I = int(A.shape[0]), int(A.shape[1])
        self.R, self.n_iter, self.transposed = psvd_plan(self.U, self.I, factors)
        self.factors, self.seed = int(factors), seed
        self._piece_len = int(piece_len)
        plans = [als_plan(np.concatenate(([0], np.cumsum(lens))), self._piece_len)
                 for lens in (np.diff(A.indptr), np.bincount(A.indices, minlength=self.I))]
        self.need = psvd_memory_need(self.U, self.I, A.nnz, self.factors, n_long=sum(p[0].shape[0] for p in plans),
                                     n_pieces=max(p[2] for p in plans))
        free, _total = torch.cuda.mem_get_info(ctx.device)
        if self.need > free:
            raise ValueError(f"PureSVD: {self.U} x {self.I} with factors={self.factors} needs {self.need} bytes of device memory "
                             f"(two orientations of the pattern, two fp64 tables of {self.R} columns, workspaces, the tables); "
                             f"{free} bytes are free")
        self._host = A
        self.user_vec = self.item_vec = None
        self.user_vec64 = self.item_vec64 = None
        self.sigma = None
        self._zero_bias = None
        self._oriented = None

    def upload(self):
        """Both orientations of the pattern on the device, (M, M^T): transposed on the host, uploaded here, released by build()."""
        if self._oriented is not None:
            return self._oriented
        A = self._host if self._host.has_sorted_indices else self._host.sorted_indices()    # never reorders the caller's arrays
        At = A.T.tocsr()
        At.sort_indices()
        dev = self.ctx.device
        ones = lambda m: None if np.all(m.data == 1.0) else m.data
        a = SpmmCSR(A.indptr, A.indices, self.I, dev, vals=ones(A), piece_len=self._piece_len)
        at = SpmmCSR(At.indptr, At.indices, self.U, dev, vals=ones(At), piece_len=self._piece_len)
        self._oriented = (at, a) if self.transposed else (a, at)
        return self._oriented

    def build(self, keep_f64=False):
        """Runs the method; leaves user_vec / item_vec (float32, rounded once from fp64) on the device and sigma on the host, and
        releases the device copies of the pattern and the workspaces.  keep_f64: also keep the fp64 tables (user_vec64 / item_vec64)."""
        ctx, dev = self.ctx, self.ctx.device
        M, Mt = self.upload()
        Qn = torch.from_numpy(psvd_start_matrix(M.n_cols, self.R, self.seed)).to(dev)        # [M.shape[1], R]
        Qm = torch.empty((M.n_rows, self.R), dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        bad = torch.full((1,), PSVD_NONE, dtype=torch.int32, device=dev)

        def orth(Y):
            psvd_orth(ctx, Y, holder=self, status=status)
            torch.minimum(bad, status, out=bad)                  # (buffer plumbing: the smallest refused column of any call)

        for it in range(self.n_iter + 1):                        # the last round is Q = qr(M Q), Z = M^T Q (B = Q^T M transposed)
            spmm_csr_f64(ctx, M, Qn, out=Qm, holder=self, verify=it == 0)
            orth(Qm)
            spmm_csr_f64(ctx, Mt, Qm, out=Qn, holder=self, verify=it == 0)
            if it < self.n_iter:
                orth(Qn)
        psvd_check_rank(int(bad.item()), self.R)
        G = gram_f64(ctx, Qn, holder=self)
        self.sigma, w_user, w_item = psvd_small_svd(G.cpu().numpy(), self.factors, self.transposed)
        Wu, Wi = torch.from_numpy(w_user).to(dev), torch.from_numpy(w_item).to(dev)
        Yu, Yi = (Qn, Qm) if self.transposed else (Qm, Qn)         # the user-side and the item-side basis
        T, _ = psvd_project(ctx, Yu, Wu)
        signs = psvd_signs(ctx, T, holder=self)                  # svd_flip decides on the user-side table in both orientations
        del T
        self.user_vec64, self.user_vec = psvd_project(ctx, Yu, Wu, col_scale=signs, f64=keep_f64, f32=True)
        self.item_vec64, self.item_vec = psvd_project(ctx, Yi, Wi, col_scale=signs, f64=keep_f64, f32=True)
        self._oriented = None                                    # recommend() does not need the pattern: its HBM is released
        for name in ("_spmm64_ws", "_gram64_ws", "_orth_ws", "_signs_ws"):
            if hasattr(self, name):
                delattr(self, name)
        return self.user_vec, self.item_vec

    def set_weights(self, user_vec, item_vec):
        u = np.ascontiguousarray(user_vec, dtype=np.float32)
        i = np.ascontiguousarray(item_vec, dtype=np.float32)
        if u.ndim != 2 or i.ndim != 2 or u.shape[0] != self.U or i.shape[0] != self.I or u.shape[1] != i.shape[1]:
            raise ValueError(f"PureSVD tables have shapes {u.shape} / {i.shape}, the model expects ({self.U}, f) / ({self.I}, f)")
        self.user_vec = torch.from_numpy(u).to(self.ctx.device)
        self.item_vec = torch.from_numpy(i).to(self.ctx.device)
        self.user_vec64 = self.item_vec64 = None

    def recommend(self, mask, k, start, stop):
        """user_vec item_vec^T for users [start, stop) and the masked top-k (el_score_topk with a zero bias); lists short of k are
        padded with (-1, -inf) (el_topk_pad): (idx, val) [n, k] on the device."""
        if self.user_vec is None:
            raise _lib.ElliotHipError("PureSVD: recommend() before build() or set_weights()")
        if self._zero_bias is None:
            self._zero_bias = torch.zeros(self.I, dtype=torch.float32, device=self.ctx.device)
        idx, val = score_topk(self.ctx, self.user_vec, self.item_vec, self._zero_bias, start, stop, k, **mask_kwargs(mask))
        check(self.ctx.lib.el_topk_pad(self.ctx.handle, self.ctx.stream(), _ptr(idx, torch.int32), _ptr(val, torch.float32),
                                       int(idx.numel())), "el_topk_pad")
        return idx, val

    def rank(self, mask, targets, start, stop):
        """Positions of the entries of rows [start, stop) of `targets` in the order recommend() selects by (el_score_rank)."""
        if self.user_vec is None:
            raise _lib.ElliotHipError("PureSVD: rank() before build() or set_weights()")
        if self._zero_bias is None:
            self._zero_bias = torch.zeros(self.I, dtype=torch.float32, device=self.ctx.device)
        return score_rank(self.ctx, self.user_vec, self.item_vec, self._zero_bias, start, stop, targets, **mask_kwargs(mask))


# ------------------------------------------------------------------------------------------
# accuracy metrics on the device
# ------------------------------------------------------------------------------------------
METRIC_NAMES = ("nDCG", "Precision", "Recall", "HR", "MAP", "MRR", "F1")


def discount_table(cutoff, device):
    """ln 2 / ln(rank + 2) exactly as relevance.py:71-82 computes it (Python doubles), shipped to the device."""
    import math
    return torch.tensor([math.log(2) / math.log(r + 2) for r in range(cutoff)], dtype=torch.float64, device=device)


class DeviceTestSet:
    """Held-out interactions as a device CSR in PRIVATE ids: rows = users, columns ascending, float ratings."""

    def __init__(self, indptr, indices, ratings, device):
        indptr = np.asarray(indptr, dtype=np.int64)
        indices = np.asarray(indices, dtype=np.int32)
        self.nnz = int(indices.shape[0])
        self.n_rows = int(indptr.shape[0] - 1)
        self.indptr = torch.from_numpy(indptr).to(device)
        self.indices = torch.from_numpy(indices if self.nnz else np.zeros(1, np.int32)).to(device)
        self.ratings = None
        if ratings is not None:
            r = np.asarray(ratings, dtype=np.float32)
            self.ratings = torch.from_numpy(r if self.nnz else np.zeros(1, np.float32)).to(device)


    @classmethod
    def from_tensors(cls, indptr, indices, ratings):
        self = cls.__new__(cls)
        self.indptr, self.indices, self.ratings = indptr.contiguous(), indices.contiguous(), ratings
        self.nnz, self.n_rows = int(indices.shape[0]), int(indptr.shape[0] - 1)
        return self


def rec_metrics(ctx, rec_idx, test, threshold, cutoff, u_start=0, sums=None, per_user=False):
    """Sums of the seven accuracy metrics over the users of rec_idx's rows (absolute ids u_start ...) that have at
    least one relevant test item, plus their count: float64[8] on the device (ADDED to `sums` when given)."""
    n, ld = rec_idx.shape
    if sums is None:
        sums = torch.zeros(8, dtype=torch.float64, device=ctx.device)
    rows = torch.empty((n, 8), dtype=torch.float64, device=ctx.device) if per_user else None
    ws = workspace(ctx, "_metrics_ws", max(int(ctx.lib.el_rec_metrics_ws_bytes(int(n))), 8), ctx.device)
    disc = discount_table(cutoff, ctx.device)
    check(ctx.lib.el_rec_metrics(ctx.handle, ctx.stream(), _ptr(rec_idx, torch.int32), int(ld), int(u_start), int(u_start + n),
                                 _ptr(test.indptr, torch.int64), _ptr(test.indices, torch.int32),
                                 _ptr(test.ratings, torch.float32), float(threshold), int(cutoff),
                                 C.c_void_p(disc.data_ptr()), C.c_void_p(sums.data_ptr()),
                                 C.c_void_p(rows.data_ptr()) if rows is not None else None,
                                 C.c_void_p(ws.data_ptr()), int(ws.numel())), "el_rec_metrics")
    return (sums, rows) if per_user else sums


# ------------------------------------------------------------------------------------------
# rank metrics on the device: positions of the held-out items in the full ranking, AUC / GAUC / LAUC sums (el_rank.hip)
# ------------------------------------------------------------------------------------------
RANK_METRIC_NAMES = ("AUC", "GAUC", "LAUC")
RANK_SUMS = 6           # el_rank_metrics' sums (include/elliot_hip.h lists the slots)
RANK_WAVE_CAP = 512     # targets per catalogue pass of k_rank_wave (el_rank.hip: RANK_CAP)
RANK_MFMA_CAP = 63      # targets per user of the fused route; users with more take the wave kernel (el_rank.hip: RANK_TCAP)
RANK_ALGOS = {"auto": EL_TOPK_AUTO, "simple": EL_TOPK_SIMPLE, "mfma": EL_TOPK_MFMA}


def _host_indptr(csr):
    """The row pointers of a device CSR on the host, copied once per object."""
    h = getattr(csr, "_indptr_host", None)
    if h is None:
        h = csr._indptr_host = csr.indptr.cpu().numpy()
    return h


def _rank_io(ctx, targets, u_start, u_stop, excl, cand, pos=None):
    """What the four rank wrappers share: the int32 positions of the target entries of rows [u_start, u_stop) (the caller's where
    given) and the tail of the library call, (excl CSR, cand CSR, target CSR, pos)."""
    hp = _host_indptr(targets)
    n = int(hp[int(u_stop)] - hp[int(u_start)])
    if pos is None:
        pos = torch.empty(max(n, 1), dtype=torch.int32, device=ctx.device)[:n]
    elif pos.shape[0] != n:
        raise ValueError(f"pos must hold the {n} target entries of the rows")
    tail = (*_csr_ptrs(excl), *_csr_ptrs(cand), _ptr(targets.indptr, torch.int64, "targets.indptr"),
            _ptr(targets.indices, torch.int32, "targets.indices"), C.c_void_p(pos.data_ptr()) if n else _ptr(targets.indices))
    return pos, tail


def score_rank(ctx, Gu, Gi, Bi, u_start, u_stop, targets, excl=None, cand=None, algo="auto", pos=None):
    """For users [u_start, u_stop) and each entry of their rows of `targets` (DeviceTestSet / DeviceCSR, absolute user rows): the
    number of admissible items score_topk would list ahead of it -- its index in the k = I list; -1 for ids >= I and masked
    targets.  int32 on the device, entry e at pos[e - targets.indptr[u_start]]."""
    I, F = Gi.shape
    if Gu.shape[1] != F:
        raise ValueError("Gu/Gi factor mismatch")
    pos, tail = _rank_io(ctx, targets, u_start, u_stop, excl, cand, pos)
    algo_id = RANK_ALGOS[algo] if isinstance(algo, str) else int(algo)
    ws, need = None, 0
    if cand is None:
        need = int(ctx.lib.el_score_rank_ws_bytes(int(u_stop) - int(u_start), int(I), int(F), int(pos.shape[0]),
                                                  int(excl.nnz) if excl is not None else 0, algo_id))
        if need:
            ws = _ptr(workspace(ctx, "_rank_ws", need, ctx.device))
    check(ctx.lib.el_score_rank(ctx.handle, ctx.stream(), _ptr(Gu, torch.float32, "Gu"), _ptr(Gi, torch.float32, "Gi"),
                                _ptr(Bi, torch.float32, "Bi"), int(u_start), int(u_stop), int(I), int(F), *tail, algo_id, ws, need),
          "el_score_rank")
    return pos


def score_rank_f64(ctx, P, Q, b, u_start, u_stop, targets, excl=None, cand=None, pos=None):
    """score_rank for fp64 tables: the order of score_topk_f64."""
    I, F = Q.shape
    pos, tail = _rank_io(ctx, targets, u_start, u_stop, excl, cand, pos)
    check(ctx.lib.el_score_rank_f64(ctx.handle, ctx.stream(), _ptr(P, torch.float64, "P"), _ptr(Q, torch.float64, "Q"),
                                    _ptr(b, torch.float64, "b"), int(u_start), int(u_stop), int(I), int(F), *tail), "el_score_rank_f64")
    return pos


def _dense_rank(ctx, preds, dtype, u_start, u_stop, targets, excl, cand, pos, I):
    n = int(u_stop) - int(u_start)
    if preds.shape[0] < n:
        raise ValueError("preds rows must cover u_stop - u_start")
    pos, tail = _rank_io(ctx, targets, u_start, u_stop, excl, cand, pos)
    fn = "el_dense_rank" if dtype == torch.float32 else "el_dense_rank_f64"
    check(getattr(ctx.lib, fn)(ctx.handle, ctx.stream(), _ptr(preds, dtype, "preds"), int(preds.stride(0)), int(u_start), int(u_stop),
                               int(preds.shape[1] if I is None else I), *tail), fn)
    return pos


def dense_rank(ctx, preds, u_start, u_stop, targets, excl=None, cand=None, pos=None, I=None):
    """score_rank over a materialised float32 [n_users, I] block: the order of dense_topk."""
    return _dense_rank(ctx, preds, torch.float32, u_start, u_stop, targets, excl, cand, pos, I)


def dense_rank_f64(ctx, preds, u_start, u_stop, targets, excl=None, cand=None, pos=None, I=None):
    """score_rank over a float64 block: the order of dense_topk_f64."""
    return _dense_rank(ctx, preds, torch.float64, u_start, u_stop, targets, excl, cand, pos, I)


def mask_kwargs(mask):
    """The tagged mask of the models' recommend() / rank() (("excl" | "cand", DeviceCSR) or None) as excl= / cand= arguments."""
    kind, csr = mask if mask is not None else (None, None)
    return {"excl": csr if kind == "excl" else None, "cand": csr if kind == "cand" else None}


def rank_metrics(ctx, pos, test, threshold, train, n_items, cutoff, u_start=0, u_stop=None, sums=None, per_user=False):
    """The six sums of the rank metrics (RANK_SUMS; include/elliot_hip.h lists the slots) of users [u_start, u_stop) from the
    positions of their held-out entries (score_rank and its kin on `test`): float64[6] on the device, ADDED to `sums` when
    given.  train: the DeviceCSR whose row lengths are len(train_dict[u])."""
    u_stop = test.n_rows if u_stop is None else int(u_stop)
    n = u_stop - int(u_start)
    if sums is None:
        sums = torch.zeros(RANK_SUMS, dtype=torch.float64, device=ctx.device)
    rows = torch.empty((n, 4), dtype=torch.float64, device=ctx.device) if per_user else None
    ws = workspace(ctx, "_rank_metrics_ws", max(int(ctx.lib.el_rank_metrics_ws_bytes(int(n))), 8), ctx.device)
    check(ctx.lib.el_rank_metrics(ctx.handle, ctx.stream(), C.c_void_p(pos.data_ptr()) if pos.numel() else _ptr(test.indices), int(u_start),
                                  u_stop, _ptr(test.indptr, torch.int64), _ptr(test.indices, torch.int32),
                                  _ptr(test.ratings, torch.float32), float(threshold), _ptr(train.indptr, torch.int64), int(n_items),
                                  int(cutoff), C.c_void_p(sums.data_ptr()), C.c_void_p(rows.data_ptr()) if rows is not None else None,
                                  C.c_void_p(ws.data_ptr()), int(ws.numel())), "el_rank_metrics")
    return (sums, rows) if per_user else sums


# ------------------------------------------------------------------------------------------
# beyond-accuracy metrics on the device: coverage, concentration, novelty, popularity bias
# ------------------------------------------------------------------------------------------
BEYOND_METRIC_NAMES = ("ItemCoverage", "UserCoverage", "NumRetrieved", "Gini", "SEntropy", "EFD", "EPC", "ARP", "APLT", "ACLT",
                       "PopREO", "PopRSP")
BEYOND_SUMS = 18        # el_beyond_metrics' sums (include/elliot_hip.h lists the slots)


class DeviceItemTables:
    """The per-item tables of evaluation/beyond.py::ItemTables in HBM: pop int32, head uint8, efd / epc float64."""

    def __init__(self, tables, device):
        self.host = tables
        self.num_items, self.n_head = int(tables.num_items), int(tables.n_head)
        self.pop = torch.from_numpy(tables.pop.astype(np.int32)).to(device)
        self.head = torch.from_numpy(tables.head.astype(np.uint8)).to(device)
        self.efd = torch.from_numpy(np.ascontiguousarray(tables.efd, dtype=np.float64)).to(device)
        self.epc = torch.from_numpy(np.ascontiguousarray(tables.epc, dtype=np.float64)).to(device)


def beyond_metrics(ctx, rec_idx, test, train, tables, threshold, cutoff, u_start=0, hist=None, sums=None, per_user=False, direct=False):
    """First pass of the beyond-accuracy metrics over the users of rec_idx's rows (absolute ids u_start ...): their terms ADDED to
    `sums` (float64[BEYOND_SUMS]) and their lists to the item histogram `hist` (int32[num_items]); train = the DeviceCSR of the
    train interactions.  direct=True: one integer add per list entry instead of one per distinct id of a tile."""
    n, ld = rec_idx.shape
    I = tables.num_items
    if sums is None:
        sums = torch.zeros(BEYOND_SUMS, dtype=torch.float64, device=ctx.device)
    if hist is None:
        hist = torch.zeros(I, dtype=torch.int32, device=ctx.device)
    rows = torch.empty((n, BEYOND_SUMS), dtype=torch.float64, device=ctx.device) if per_user else None
    ws = workspace(ctx, "_beyond_ws", max(int(ctx.lib.el_beyond_ws_bytes(int(n), int(I))), 8), ctx.device)
    disc = discount_table(cutoff, ctx.device)
    check(ctx.lib.el_beyond_metrics(ctx.handle, ctx.stream(), _ptr(rec_idx, torch.int32), int(ld), int(u_start), int(u_start + n),
                                    _ptr(test.indptr, torch.int64), _ptr(test.indices, torch.int32),
                                    _ptr(test.ratings, torch.float32), float(threshold), int(cutoff),
                                    _ptr(train.indptr, torch.int64), _ptr(train.indices, torch.int32), int(I), int(tables.n_head),
                                    _ptr(tables.pop, torch.int32), _ptr(tables.head, torch.uint8), _ptr(tables.efd, torch.float64),
                                    _ptr(tables.epc, torch.float64), C.c_void_p(disc.data_ptr()), _ptr(hist, torch.int32),
                                    _ptr(sums, torch.float64), C.c_void_p(rows.data_ptr()) if rows is not None else None,
                                    _lib.EL_BEYOND_HIST_DIRECT if direct else 0, C.c_void_p(ws.data_ptr()), int(ws.numel())),
          "el_beyond_metrics")
    return (sums, hist, rows) if per_user else (sums, hist)


def beyond_hist_finish(ctx, hist):
    """(stats int64[4] = #items in a list, free = sum of the counts, the exact Gini numerator G, 0;  nov float64[I] = -log2(hist / free))"""
    I = int(hist.shape[0])
    stats = torch.empty(4, dtype=torch.int64, device=ctx.device)
    nov = torch.empty(I, dtype=torch.float64, device=ctx.device)
    ws = workspace(ctx, "_beyond_ws", max(int(ctx.lib.el_beyond_ws_bytes(0, int(I))), 8), ctx.device)
    check(ctx.lib.el_beyond_hist_finish(ctx.handle, ctx.stream(), _ptr(hist, torch.int32), I, _ptr(stats, torch.int64),
                                        _ptr(nov, torch.float64), C.c_void_p(ws.data_ptr()), int(ws.numel())), "el_beyond_hist_finish")
    return stats, nov


def beyond_entropy(ctx, rec_idx, test, nov, cutoff, u_start=0, total=None):
    """Sum over the users of the block that have a held-out row of (1 / n_u) sum of nov over the list, ADDED to `total` (float64[1])."""
    n, ld = rec_idx.shape
    if total is None:
        total = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    ws = workspace(ctx, "_beyond_ws", max(int(ctx.lib.el_beyond_ws_bytes(int(n), int(nov.shape[0]))), 8), ctx.device)
    check(ctx.lib.el_beyond_entropy(ctx.handle, ctx.stream(), _ptr(rec_idx, torch.int32), int(ld), int(u_start), int(u_start + n),
                                    _ptr(test.indptr, torch.int64), int(cutoff), int(nov.shape[0]), _ptr(nov, torch.float64),
                                    _ptr(total, torch.float64), C.c_void_p(ws.data_ptr()), int(ws.numel())), "el_beyond_entropy")
    return total


# ------------------------------------------------------------------------------------------
# fairness metrics on the device (el_metrics_fair.hip): RSP, REO, BiasDisparity, the four MADs
# ------------------------------------------------------------------------------------------
FAIR_MAX_GROUPS = 64
FAIR_ROW = 4            # el_fair_metrics' per-user row: nDCG, in R, mean list score, has a score


class DeviceGrouping:
    """A clustering of evaluation/fairness.py::Grouping in HBM: labels int32[n] (-1 = none), sizes int64[n_groups]."""

    def __init__(self, grouping, device):
        self.host = grouping
        self.n_groups = int(grouping.n_groups)
        if not 1 <= self.n_groups <= FAIR_MAX_GROUPS:
            raise ValueError(f"{self.n_groups} groups: the fairness kernels keep 1..{FAIR_MAX_GROUPS} user groups and item groups")
        self.labels = torch.from_numpy(np.ascontiguousarray(grouping.labels, dtype=np.int32)).to(device)
        self.sizes = torch.from_numpy(np.ascontiguousarray(grouping.sizes, dtype=np.int64)).to(device)


class DeviceTestColumns:
    """The item-major copy of a held-out CSR for el_fair_item_finish: col_indptr int64[I + 1], col_entry int64 = the entries'
    indices in the CSR, users ascending inside a column; entries with an id >= I (no model row) are left out."""

    def __init__(self, indptr, indices, n_items, device):
        indices = np.asarray(indices, dtype=np.int64)
        keep = np.flatnonzero(indices < n_items)
        cols = indices[keep]
        col_indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=int(n_items)))]).astype(np.int64)
        self.indptr = torch.from_numpy(col_indptr).to(device)
        entry = keep[np.argsort(cols, kind="stable")]           # by item; entries of the CSR run by user, so users ascend
        self.entry = torch.from_numpy(entry if entry.shape[0] else np.zeros(1, np.int64)).to(device)


class FairState:
    """What one (grouping pair, split, cutoff) accumulates over the blocks: 8 bytes per held-out entry, 4 bytes per item and the
    group tables."""

    def __init__(self, ctx, test, n_items, items, users):
        dev, Gi, Gu = ctx.device, items.n_groups, users.n_groups
        self.item_counts = torch.zeros((4, Gi), dtype=torch.int64, device=dev)
        self.pair = torch.zeros((Gu, Gi), dtype=torch.int64, device=dev)
        self.user_sums = torch.zeros((Gu, FAIR_ROW), dtype=torch.float64, device=dev)
        self.user_cnt = torch.zeros(Gu, dtype=torch.int64, device=dev)
        self.hit_pos = torch.full((max(test.nnz, 1),), -1, dtype=torch.int32, device=dev)
        self.hit_score = torch.zeros(max(test.nnz, 1), dtype=torch.float32, device=dev)
        self.hist = torch.zeros(int(n_items), dtype=torch.int32, device=dev)
        self.item_sums = torch.zeros((Gi, 2), dtype=torch.float64, device=dev)
        self.item_cnt = torch.zeros(Gi, dtype=torch.int64, device=dev)

    def host_terms(self):
        """The layout of evaluation/fairness.py::numpy_terms."""
        return {"item_counts": self.item_counts.cpu().numpy(), "pair": self.pair.cpu().numpy(), "user_sums": self.user_sums.cpu().numpy(),
                "item_sums": self.item_sums.cpu().numpy(), "item_cnt": self.item_cnt.cpu().numpy()}


def group_sums(ctx, rows, labels, n_groups, sums=None, counts=None):
    """The rows [n, W <= 4] (float64) summed by label (int32[n], -1 = none) in a shape that depends on n alone: float64
    [n_groups, W] and the rows per label int64[n_groups], both ADDED to `sums` / `counts` when given."""
    n, W = rows.shape
    if sums is None:
        sums = torch.zeros((n_groups, W), dtype=torch.float64, device=ctx.device)
    if counts is None:
        counts = torch.zeros(n_groups, dtype=torch.int64, device=ctx.device)
    if not 1 <= int(n_groups) <= FAIR_MAX_GROUPS:
        raise ValueError(f"{n_groups} groups: 1..{FAIR_MAX_GROUPS}")
    if sums.shape[1] != W:
        raise ValueError("sums must be [n_groups, W]")
    ws = workspace(ctx, "_fair_ws", max(int(ctx.lib.el_group_sums_ws_bytes(int(n), int(n_groups))), 8), ctx.device)
    check(ctx.lib.el_group_sums(ctx.handle, ctx.stream(), _ptr(rows, torch.float64), int(W), _ptr(labels, torch.int32), int(n),
                                int(n_groups), _ptr(sums, torch.float64), _ptr(counts, torch.int64), C.c_void_p(ws.data_ptr()),
                                int(ws.numel())), "el_group_sums")
    return sums, counts


def group_counts(ctx, csr, n_items, items, users, counts=None):
    """int64[user groups, item groups]: the entries of the CSR's rows by (row label, column label), ADDED to `counts` when given
    (BiasDisparityBS on the train matrix)."""
    if counts is None:
        counts = torch.zeros((users.n_groups, items.n_groups), dtype=torch.int64, device=ctx.device)
    n_rows = int(csr.indptr.shape[0] - 1)
    if users.labels.shape[0] < n_rows:
        raise ValueError("user labels must cover the rows")
    check(ctx.lib.el_group_counts(ctx.handle, ctx.stream(), _ptr(csr.indptr, torch.int64), _ptr(csr.indices, torch.int32), n_rows,
                                  int(n_items), _ptr(items.labels, torch.int32), items.n_groups, _ptr(users.labels, torch.int32),
                                  users.n_groups, _ptr(counts, torch.int64)), "el_group_counts")
    return counts


def fair_metrics(ctx, rec_idx, rec_val, test, train, items, users, threshold, cutoff, n_items, state, u_start=0):
    """The fairness pass over the users of rec_idx's rows (absolute ids u_start ...): integer tables, hit entries and the
    R-histogram ADDED to `state` (FairState), the per-user rows summed by user label into state.user_sums / user_cnt.
    rec_val: the float32 scores of the lists or None.  Returns (user_label int32[n], user_rows float64[n, 4])."""
    n, ld = rec_idx.shape
    if items.labels.shape[0] < n_items or users.labels.shape[0] < u_start + n:
        raise ValueError("group labels must cover the items and the users")
    if rec_val is not None and (rec_val.shape != rec_idx.shape or rec_val.stride(0) != ld):
        raise ValueError("rec_val must have the layout of rec_idx")
    label = torch.empty(n, dtype=torch.int32, device=ctx.device)
    rows = torch.empty((n, FAIR_ROW), dtype=torch.float64, device=ctx.device)
    disc = discount_table(cutoff, ctx.device)
    check(ctx.lib.el_fair_metrics(ctx.handle, ctx.stream(), _ptr(rec_idx, torch.int32), _ptr(rec_val, torch.float32) if rec_val is not None
                                  else None, int(ld), int(u_start), int(u_start + n), _ptr(test.indptr, torch.int64),
                                  _ptr(test.indices, torch.int32), _ptr(test.ratings, torch.float32), float(threshold), int(cutoff),
                                  _ptr(train.indptr, torch.int64), _ptr(train.indices, torch.int32), int(n_items),
                                  _ptr(items.labels, torch.int32), items.n_groups, _ptr(items.sizes, torch.int64),
                                  _ptr(users.labels, torch.int32), users.n_groups, C.c_void_p(disc.data_ptr()),
                                  _ptr(state.item_counts, torch.int64), _ptr(state.pair, torch.int64), _ptr(label, torch.int32),
                                  _ptr(rows, torch.float64), _ptr(state.hit_pos, torch.int32), _ptr(state.hit_score, torch.float32),
                                  _ptr(state.hist, torch.int32)), "el_fair_metrics")
    group_sums(ctx, rows, label, users.n_groups, sums=state.user_sums, counts=state.user_cnt)
    return label, rows


def fair_item_finish(ctx, test, cols, items, threshold, state, per_item=False):
    """After the last block: per item the mean gain / score of its hit entries over the lists of R that hold it (in ascending
    user order), summed by item label into state.item_sums / item_cnt.  per_item=True also returns float64[I, 2]."""
    I = int(state.hist.shape[0])
    rows = torch.empty((I, 2), dtype=torch.float64, device=ctx.device) if per_item else None
    ws = workspace(ctx, "_fair_ws", max(int(ctx.lib.el_fair_item_finish_ws_bytes(I, items.n_groups)), 8), ctx.device)
    check(ctx.lib.el_fair_item_finish(ctx.handle, ctx.stream(), _ptr(cols.indptr, torch.int64), _ptr(cols.entry, torch.int64),
                                      _ptr(test.ratings, torch.float32), float(threshold), _ptr(state.hit_pos, torch.int32),
                                      _ptr(state.hit_score, torch.float32), _ptr(state.hist, torch.int32), I,
                                      _ptr(items.labels, torch.int32), items.n_groups, _ptr(state.item_sums, torch.float64),
                                      _ptr(state.item_cnt, torch.int64), C.c_void_p(rows.data_ptr()) if rows is not None else None,
                                      C.c_void_p(ws.data_ptr()), int(ws.numel())), "el_fair_item_finish")
    return rows


def topk_screen_stats(ctx):
    """Diagnostics of the last screened score_topk call (el_topk_screen_stats; synchronises): users of the block, records the bf16 pass
    kept for them, users that took the exact fallback."""
    u, r, f = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(ctx.lib.el_topk_screen_stats(ctx.handle, ctx.stream(), C.byref(u), C.byref(r), C.byref(f)), "el_topk_screen_stats")
    return {"users": int(u.value), "records": int(r.value), "records_per_user": (r.value / u.value) if u.value else 0.0,
            "fallback_users": int(f.value)}


def topk_fragile(ctx, Gu, Gi, idx, val, k, u_start=0, item_offset=0, flags=False, counts=None):
    """el_topk_fragile on [n, >= k + 1] lists (idx int32 in absolute item ids, val float32) of the users u_start .. u_start + n:
    Gu holds every user, Gi the items from item_offset on.  ADDS to `counts` (int64[2] on the device: fragile users, lists with
    fewer than k + 1 entries); returns it, and the uint8 flag per user when flags=True."""
    n = int(idx.shape[0])
    if counts is None:
        counts = torch.zeros(2, dtype=torch.int64, device=ctx.device)
    fl = torch.zeros(n, dtype=torch.uint8, device=ctx.device) if flags else None
    check(ctx.lib.el_topk_fragile(ctx.handle, ctx.stream(), _ptr(Gu, torch.float32), _ptr(Gi, torch.float32), int(Gu.shape[1]),
                                  int(u_start), int(u_start + n), _ptr(idx, torch.int32), _ptr(val, torch.float32), int(idx.shape[1]),
                                  int(k), int(item_offset), C.c_void_p(fl.data_ptr()) if fl is not None else None,
                                  _ptr(counts, torch.int64)), "el_topk_fragile")
    return (counts, fl) if flags else counts


def fragile_users(ctx, Gu, Gi, Bi, u_start, u_stop, k, excl=None, cand=None, item_offset=0, algo="auto", flags=False):
    """Fragile-user report: how many of the users [u_start, u_stop) have a rank-k / rank-(k+1) score gap
    below the fp32 re-association bound F 2^-23 |u| max|i| -- for those (and only those) the top-k SET could differ under
    another correct fp32 summation order (TensorFlow's `tf.matmul`, BPRMF_batch_model.py:83-84).  Scores k + 1 entries per
    user with the fused kernels, then el_topk_fragile.  Returns a dict (and the uint8 flag tensor when flags=True)."""
    idx, val = score_topk(ctx, Gu, Gi, Bi, u_start, u_stop, k + 1, excl=excl, cand=cand, item_offset=item_offset, algo=algo)
    n = u_stop - u_start
    out = topk_fragile(ctx, Gu, Gi, idx, val, k, u_start=u_start, item_offset=item_offset, flags=flags)
    counts, fl = out if flags else (out, None)
    c = counts.cpu().tolist()
    rep = {"users": int(n), "k": int(k), "fragile": int(c[0]), "short_lists": int(c[1]),
           "bound": "score[k-1] - score[k] < F * 2^-23 * |u| * max(|i_k|, |i_k+1|)"}
    return (rep, fl) if flags else rep


# ------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------
def sampler_meta(ctx, pos):
    """The sampler's per-user records of a positives CSR (el_bpr_sampler_meta_build), built once and cached on the CSR object:
    row start, row length and a 384-bit membership signature in one 64-byte line per user."""
    meta = getattr(pos, "_sampler_meta", None)
    if meta is None:
        nbytes = int(ctx.lib.el_bpr_sampler_meta_bytes(int(pos.n_rows)))
        meta = torch.empty(nbytes + 64, dtype=torch.uint8, device=ctx.device)
        off = (-meta.data_ptr()) % 64
        meta = meta[off:off + nbytes]                                 # 64-byte aligned view
        check(ctx.lib.el_bpr_sampler_meta_build(ctx.handle, ctx.stream(), *_csr_ptrs(pos), int(pos.n_rows),
                                                C.c_void_p(meta.data_ptr())), "el_bpr_sampler_meta_build")
        try:
            pos._sampler_meta = meta
        except Exception:
            pass
    return meta


def bpr_sample(ctx, pos, n, seed, first_sample=0, item_lo=0, item_hi=None, out=None, use_meta=True):
    """custom_sampler.Sampler.step (custom_sampler.py:31-46) on the device: n triplets.  use_meta: draw through the per-user
    records (same triplets, fewer cache lines per draw); False = the plain CSR path."""
    U, I = pos.n_rows, pos.n_cols
    if item_hi is None:
        item_hi = I
    if out is None:
        out = tuple(torch.empty((n,), dtype=torch.int32, device=ctx.device) for _ in range(3))
    meta = sampler_meta(ctx, pos) if use_meta else None
    check(ctx.lib.el_bpr_sample_meta(ctx.handle, ctx.stream(), *_csr_ptrs(pos), C.c_void_p(meta.data_ptr()) if meta is not None else None,
                                     int(U), int(I), int(item_lo), int(item_hi), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sample),
                                     int(n), _ptr(out[0], torch.int32), _ptr(out[1], torch.int32), _ptr(out[2], torch.int32)),
          "el_bpr_sample_meta")
    return out


def mt19937_init_state(seed):
    """np.random.seed(int) = MT19937 init_genrand: 624 words + position 624 (next draw twists)."""
    mt = np.empty(625, dtype=np.uint32)
    x = int(seed) & 0xFFFFFFFF
    mt[0] = x
    for i in range(1, 624):
        x = (1812433253 * (x ^ (x >> 30)) + i) & 0xFFFFFFFF
        mt[i] = x
    mt[624] = 624
    return mt


class MtReplaySampler:
    """Device replay of custom_sampler.Sampler's exact triplet stream (el_bpr_sample_mt19937)."""

    def __init__(self, ctx, ui_lists, pos, seed=42):
        """ui_lists: per-user positive lists in the reference's order (list(set(...)), custom_sampler.py:21);
        pos: DeviceCSR of the same rows sorted ascending."""
        self.ctx, self.pos = ctx, pos
        lp = np.concatenate([[0], np.cumsum([len(l) for l in ui_lists])]).astype(np.int64)
        li = np.concatenate([np.asarray(l, dtype=np.int32) for l in ui_lists]) if len(ui_lists) else np.zeros(0, np.int32)
        self.lists = DeviceCSR.__new__(DeviceCSR)
        self.lists.n_rows, self.lists.n_cols, self.lists.nnz = len(ui_lists), pos.n_cols, int(li.shape[0])
        self.lists.indptr = torch.from_numpy(lp).to(ctx.device)
        self.lists.indices = torch.from_numpy(li if li.size else np.zeros(1, np.int32)).to(ctx.device)
        self.state = torch.from_numpy(mt19937_init_state(seed).view(np.int32).copy()).to(ctx.device)

    def sample(self, n):
        ctx = self.ctx
        ws = workspace(self, "_ws", int(ctx.lib.el_bpr_sample_mt19937_ws_bytes(int(n))), ctx.device)
        out = tuple(torch.empty(n, dtype=torch.int32, device=ctx.device) for _ in range(3))
        check(ctx.lib.el_bpr_sample_mt19937(ctx.handle, ctx.stream(), C.c_void_p(self.state.data_ptr()),
                                            _ptr(self.lists.indptr, torch.int64), _ptr(self.lists.indices, torch.int32),
                                            *_csr_ptrs(self.pos), int(self.pos.n_rows), int(self.pos.n_cols), int(n),
                                            _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                            _ptr(ws), ws.numel()), "el_bpr_sample_mt19937")
        return out


# ------------------------------------------------------------------------------------------
# BPRMF_batch (TF semantics)
# ------------------------------------------------------------------------------------------
def deterministic_item_sums(ctx):
    """True when the item segments a chunk boundary cuts are summed in a fixed order (no floating-point atomics anywhere in the
    sorted BPR step): two runs on the same batches then give the same bits, and the fused / deferred forms equal the every-row
    two-pass form bit for bit at any size."""
    fn = getattr(ctx.lib, "el_bprmf_deterministic", None)
    return bool(fn()) if fn is not None else False


def adam_lr_t(lr, step, beta1=0.9, beta2=0.999):
    """Keras Adam bias-corrected step size, computed in fp32 like TF does."""
    b1p = np.power(np.float32(beta1), np.float32(step))
    b2p = np.power(np.float32(beta2), np.float32(step))
    return float(np.float32(lr) * np.sqrt(np.float32(1.0) - b2p) / (np.float32(1.0) - b1p))


# ------------------------------------------------------------------------------------------
# HBM placement of the four streams of the dense Adam pass
# ------------------------------------------------------------------------------------------
_LAYOUT_CANDIDATES_MIB = (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5)
BIG_TABLE_BYTES = 64 << 20          # an embedding table from here on gets the tuned Adam block (and compact user gradients in BPR)


def _strided_tables(rows, F, count, gap_bytes, device):
    """`count` zeroed float32 [rows, F] tables carved from ONE allocation, consecutive tables `gap_bytes` apart."""
    n = rows * F
    stride = n + (int(gap_bytes) // 4 + 63) // 64 * 64            # in floats, 256 B granules
    big = torch.zeros(stride * count, dtype=torch.float32, device=device)
    return [big[t * stride:t * stride + n].view(rows, F) for t in range(count)], big


def tune_table_layout(ctx, rows, F, compact=False):
    """The TF-dense Adam pass streams theta, g, m and v of a table at once (4 reads + 3 writes per element; with compact
    gradient rows: theta, m, v and the rows of the batch's users).  How far apart those arrays sit in HBM decides how their
    channel / bank sequences collide: measured on MI355X, 0.61 to 0.82 ms for the same 1M x 128 table, periodic in the
    distance (about 6 MiB) -- and with one allocation per array it is the allocator's luck.  So the arrays of a large table
    are carved from one allocation and the distance is picked by timing the pass itself on a scratch copy (a dozen
    candidates, ~0.1 s, once per table shape and process).  Returns the gap in bytes."""
    key = (int(rows), int(F), bool(compact))
    cache = ctx.__dict__.setdefault("_layout_cache", {})
    if key in cache:
        return cache[key]
    if os.environ.get("EL_TUNE_LAYOUT", "1") == "0" or rows * F * 4 < BIG_TABLE_BYTES:
        cache[key] = 0
        return 0
    dev = ctx.device
    dummy = [torch.zeros((64, F), dtype=torch.float32, device=dev) for _ in range(4)] + \
            [torch.zeros(64, dtype=torch.float32, device=dev) for _ in range(4)]
    uslot = grows = hit = slot = None
    if compact:
        # what a step looks like: ~63 % of the rows (1 - 1/e at B = U) carry a gradient row, slots ascending with the user id
        try:
            grows = torch.zeros((rows, F), dtype=torch.float32, device=dev)
        except RuntimeError:
            cache[key] = 0
            return 0
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        hit = (torch.rand(rows, generator=g, device=dev) < 0.63).to(torch.int64)
        slot = torch.arange(rows, dtype=torch.int64, device=dev) * hit
        uslot = torch.zeros(rows, dtype=torch.int64, device=dev)
    best, best_ms = 0, None
    check(ctx.lib.el_tuning_mode(ctx.handle, 1), "el_tuning_mode")      # probes under their own kernel symbols (profiles)
    for mib in _LAYOUT_CANDIDATES_MIB:
        gap = int(mib * (1 << 20))
        try:
            tabs, big = _strided_tables(rows, F, 3 if compact else 4, gap, dev)
        except RuntimeError:                                      # out of memory for the scratch copy: keep the plain layout
            break
        if compact:
            c = BprmfState(Gu=tabs[0].data_ptr(), gGu=None, mGu=tabs[1].data_ptr(), vGu=tabs[2].data_ptr(),
                           uslot=uslot.data_ptr(), gGu_rows=grows.data_ptr(), gGu_cap=rows,
                           Gi=dummy[0].data_ptr(), gGi=dummy[1].data_ptr(), mGi=dummy[2].data_ptr(), vGi=dummy[3].data_ptr(),
                           Bi=dummy[4].data_ptr(), gBi=dummy[5].data_ptr(), mBi=dummy[6].data_ptr(), vBi=dummy[7].data_ptr(),
                           tGu=None, tGi=None, tBi=None, U=rows, I=64, F=F)
        else:
            c = BprmfState(Gu=tabs[0].data_ptr(), gGu=tabs[1].data_ptr(), mGu=tabs[2].data_ptr(), vGu=tabs[3].data_ptr(),
                           Gi=dummy[0].data_ptr(), gGi=dummy[1].data_ptr(), mGi=dummy[2].data_ptr(), vGi=dummy[3].data_ptr(),
                           Bi=dummy[4].data_ptr(), gBi=dummy[5].data_ptr(), mBi=dummy[6].data_ptr(), vBi=dummy[7].data_ptr(),
                           tGu=None, tGi=None, tBi=None, U=rows, I=64, F=F)

        def run(it):
            if compact:
                torch.add(slot, hit, alpha=it << 32, out=uslot)          # stamps of step `it` on the touched rows
            check(ctx.lib.el_bprmf_apply(ctx.handle, ctx.stream(), C.byref(c), 0.001, EL_OPT_ADAM_TF_DENSE, it, 0.001), "el_bprmf_apply")

        for it in range(2):
            run(it + 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(4):
            run(it + 3)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / 4
        if best_ms is None or ms < best_ms:
            best, best_ms = gap, ms
        del tabs, big
    check(ctx.lib.el_tuning_mode(ctx.handle, 0), "el_tuning_mode")
    cache[key] = best
    return best


def _tuned_adam_block(ctx, theta, count, compact=False):
    """The arrays the dense Adam pass streams for one big table, from ONE allocation at the tuned distance (tune_table_layout):
    `count` zeroed float32 tables of theta's shape, theta copied into the first.  Returns (tables, the block to keep alive, gap)."""
    rows, F = int(theta.shape[0]), int(theta.shape[1])
    gap = tune_table_layout(ctx, rows, F, compact=compact)
    tabs, block = _strided_tables(rows, F, count, gap, ctx.device)
    tabs[0].copy_(theta if isinstance(theta, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(theta)))
    return tabs, block, gap


class BprmfDeviceState:
    """Gu/Gi/Bi + gradient accumulators + Adam slots in HBM (BPRMF_batch_model.py:39-44)."""

    _LR_HIST = 1 << 16          # lr_t ring of the deferred decay (a power of two)

    def __init__(self, ctx, Gu, Gi, Bi, optimizer="adam", compact_user_grads=None, fused_user_step=None, deferred=None,
                 fused_item_step=None, item_deferred=None, replay="exact"):
        """compact_user_grads: user-row gradients as compact rows + per-user stamps (el_bprmf_state.uslot) instead of a dense
        [U,F] accumulator -- the dense Adam pass then reads a gradient only for the batch's users and re-zeroes nothing.
        None = automatic (TF-dense Adam on a user table of >= 64 MB with F % 4 == 0), True / False force it.
        deferred: Keras' every-row Adam decay of the USER table postponed per row and replayed bit for bit when a batch next
        contains the user or when the table is read (el_bprmf_state.Gu_last): a step moves only the batch's user rows.  It pays
        when a batch touches a small part of the users (10 M users, 1 M triplets: the user side of the step 7.2 -> ~2 ms) and costs
        when it touches most of them (B = U: +10 %), so None = decided at the first training call: on when 4 B <= U and the fused
        user-side step applies; reading `.Gu` syncs, `.mGu` / `.vGu` want sync() first.
        fused_item_step: the item side of the step as ONE kernel (el_bprmf_state.Gi_last): the item segments take Keras' Adam step on
        their rows in place, no dense gradient table is written, re-read and cleared.  None = whenever the fused user side applies
        (fused_item_step=False turns it off); grads() / apply() always run the two-pass form.
        item_deferred: with the fused item side, the item rows a batch leaves alone wait for their gradient-free Adam updates like the
        user rows do (replayed bit for bit when a batch next contains the item, or on sync() / reading `.Gi` / `.Bi`); False = they
        are replayed at the end of every step.  None = decided by the first batch size: on when 2 B <= I.
        replay: how a waiting row is brought forward over its gradient-free steps -- "exact": step by step, the bits of Keras'
        every-row pass; "series": in closed form from four row-level sums over the lr_t history (el_bprmf_state.replay_series:
        O(1) per element whatever the gap; as close to the exact-arithmetic recurrence as the fp32 step-by-step form, not its bits)."""
        self.ctx = ctx
        if replay not in ("exact", "series"):
            raise ValueError("replay must be 'exact' or 'series'")
        self.replay = replay
        self.opt = OPTIMIZERS[optimizer] if isinstance(optimizer, str) else int(optimizer)
        dev = ctx.device
        big = int(Gu.shape[0]) * int(Gu.shape[1]) * 4 >= BIG_TABLE_BYTES
        self.compact = bool(self.opt == EL_OPT_ADAM_TF_DENSE and int(Gu.shape[1]) % 4 == 0 and optimizer != "sgd_dense" and
                            (big if compact_user_grads is None else compact_user_grads))

        # fused user side (el_bprmf_state.Gu_next): segments + Keras Adam over every user row in ONE kernel, the new rows written to a
        # second table that swaps roles with Gu after every step -- whenever the compact form applies (fused_user_step=False: the
        # two-kernel form, which grads() / apply() always use)
        self.fused = bool(self.compact and fused_user_step is not False
                          and int(Gu.shape[1]) <= 512)
        self.Gu_next = None
        self._deferred_auto = bool(self.fused and deferred is None)    # decided by the first batch size (_resolve_deferred)
        self.deferred = bool(self.fused and deferred is True)
        self._pending = False
        self.item_fused = bool(self.fused and fused_item_step is not False)
        self._item_deferred_auto = bool(self.item_fused and item_deferred is None)
        self.item_deferred = bool(self.item_fused and item_deferred is True)
        self._pending_items = False

        self._Gi, self._Bi = _own(Gi, dev), _own(Bi, dev)
        self.U, self.F = int(Gu.shape[0]), int(Gu.shape[1])
        self.I = self._Gi.shape[0]
        z = torch.zeros_like
        adam = self.opt in (EL_OPT_ADAM_TF_DENSE, EL_OPT_ADAM_LAZY)
        self.uslot = self.gGu_rows = None
        if self.opt == EL_OPT_ADAM_TF_DENSE and self.U * self.F * 4 >= BIG_TABLE_BYTES:
            self.gGu = None
            if self.compact and self.fused and not self.deferred:
                # (deferred=None: the pair is allocated; if the first batch turns the deferred decay on, Gu_next just stays unused)
                names = ("Gu", "mGu", "vGu", "Gu_next")
            else:
                names = ("Gu", "mGu", "vGu") if self.compact else ("Gu", "gGu", "mGu", "vGu")
            tabs, self._user_block, self.layout_gap = _tuned_adam_block(ctx, Gu, len(names), compact=self.compact)
            for n, t in zip(names, tabs):
                setattr(self, n, t)
        else:
            self.Gu = _own(Gu, dev)
            if self.fused and not self.deferred:
                self.Gu_next = torch.empty_like(self.Gu)
            self.gGu = None if self.compact else z(self.Gu)
            self.mGu = z(self.Gu) if adam else None
            self.vGu = z(self.Gu) if adam else None
            self.layout_gap = None
        if self.compact:
            self.uslot = torch.zeros(self.U, dtype=torch.int64, device=dev)       # (step << 32) | slot; step 0 is never used
        # item-side gradients in ONE buffer (gGi rows, then gBi): a data-parallel caller all-reduces `item_grad_flat` once
        rows_end = (self.I * self.F + 3) // 4 * 4                       # gBi starts on a 16-byte boundary
        self.item_grad_flat = torch.zeros(rows_end + self.I, dtype=torch.float32, device=dev)
        self.gGi = self.item_grad_flat[:self.I * self.F].view(self.I, self.F)
        self.gBi = self.item_grad_flat[rows_end:]
        self._item_block = None
        # (theta, m, v of the item table from ONE allocation a fixed distance apart was tried in round 5: consistent, not faster -- and the
        #  process-to-process spread of the item kernels is not about these tables at all: profiles/r06_placement_probe.md)
        self.mGi = z(self._Gi) if adam else None
        self.vGi = z(self._Gi) if adam else None
        self.mBi = z(self._Bi) if adam else None
        self.vBi = z(self._Bi) if adam else None
        rows = self.opt in (EL_OPT_ADAM_LAZY, EL_OPT_SGD) and optimizer != "sgd_dense"
        self.tGu = torch.zeros(self.U, dtype=torch.int32, device=dev) if rows else None
        self.tGi = torch.zeros(self.I, dtype=torch.int32, device=dev) if rows else None
        self.tBi = torch.zeros(self.I, dtype=torch.int32, device=dev) if rows else None
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._step = 0
        self._ws = None
        self._c = BprmfState(
            Gu=self._Gu.data_ptr(), Gi=self._Gi.data_ptr(), Bi=self._Bi.data_ptr(),
            gGu=self.gGu.data_ptr() if self.gGu is not None else None, gGi=self.gGi.data_ptr(), gBi=self.gBi.data_ptr(),
            uslot=self.uslot.data_ptr() if self.compact else None, gGu_rows=None, gGu_cap=0,
            mGu=self.mGu.data_ptr() if adam else None, vGu=self.vGu.data_ptr() if adam else None,
            mGi=self.mGi.data_ptr() if adam else None, vGi=self.vGi.data_ptr() if adam else None,
            mBi=self.mBi.data_ptr() if adam else None, vBi=self.vBi.data_ptr() if adam else None,
            tGu=self.tGu.data_ptr() if rows else None, tGi=self.tGi.data_ptr() if rows else None,
            tBi=self.tBi.data_ptr() if rows else None, U=self.U, I=self.I, F=self.F,
            Gu_next=self.Gu_next.data_ptr() if self.Gu_next is not None else None, replay_series=int(replay == "series"))
        self.Gu_last = self.lr_hist = None
        self.Gi_last = None
        if self.deferred:
            self._enable_deferred()
        if self.item_fused:
            # fused item side: the step each item row is current at
            self.Gi_last = torch.zeros(self.I, dtype=torch.int32, device=dev)
            self._ensure_hist()
            self._c.Gi_last, self._c.Gi_defer = self.Gi_last.data_ptr(), int(self.item_deferred)

    def _ensure_hist(self):
        """The ring of the last _LR_HIST bias-corrected step sizes (what the replay of postponed row updates reads)."""
        if self.lr_hist is None:
            self.lr_hist = torch.zeros(self._LR_HIST, dtype=torch.float32, device=self.ctx.device)
            self._c.lr_hist, self._c.lr_hist_cap = self.lr_hist.data_ptr(), self._LR_HIST

    def _enable_deferred(self):
        dev = self.ctx.device
        self.deferred = True
        self.Gu_last = torch.full((self.U,), int(self._step), dtype=torch.int32, device=dev)     # every row is current now
        self._ensure_hist()
        self._c.Gu_last = self.Gu_last.data_ptr()
        if getattr(self, "_user_block", None) is None and not self._deferred_auto:
            self.Gu_next = None                                  # in-place updates: the second table is not needed
            self._c.Gu_next = None

    def _resolve_deferred(self, B):
        """A state built with deferred=None follows the batch size: the deferred decay pays when a batch leaves most user rows
        alone (4 B <= U), the every-row fused step when it touches most of them.  Switching costs one replay of the pending rows."""
        if int(B) == getattr(self, "_resolved_B", None):
            return
        self._resolved_B = int(B)
        if self._deferred_auto:
            want = 4 * int(B) <= self.U
            if want != self.deferred:
                auto = self._deferred_auto
                self.set_deferred(want)
                self._deferred_auto = auto
        if self._item_deferred_auto:
            # the item side: a batch draws B negatives uniformly over the catalogue (custom_sampler.py:39-41) and B positives: it pays
            # when those leave most item rows alone
            self.set_item_deferred(2 * int(B) <= self.I, _auto=True)

    # -- deferred decay of the user table (el_bprmf_state.Gu_last) ----------------------------------------------------------
    @property
    def Gu(self):
        """The user table, every row current (pending row updates of the deferred decay are replayed first)."""
        if self._pending:
            self.sync()
        return self._Gu

    @Gu.setter
    def Gu(self, t):
        self._Gu = t

    @property
    def Gi(self):
        """The item table, every row current (pending row updates of the deferred item decay are replayed first)."""
        if self._pending_items:
            self.sync()
        return self._Gi

    @property
    def Bi(self):
        if self._pending_items:
            self.sync()
        return self._Bi

    def sync(self):
        """Deferred decay: bring every user row and every item row (theta, m, v) to the current step; no-op otherwise."""
        if self.deferred and self._pending:
            self._pending = False
            check(self.ctx.lib.el_bprmf_sync_users(self.ctx.handle, self.ctx.stream(), C.byref(self._c), int(self._step)),
                  "el_bprmf_sync_users")
        if self.item_fused and self._pending_items:
            self._pending_items = False
            check(self.ctx.lib.el_bprmf_sync_items(self.ctx.handle, self.ctx.stream(), C.byref(self._c), int(self._step)),
                  "el_bprmf_sync_items")

    def set_item_deferred(self, on, _auto=False):
        """Fused item side: let the item rows a batch leaves alone wait for their gradient-free updates (True) or replay them at
        the end of every step (False)."""
        on = bool(on) and self.item_fused
        if not _auto:
            self._item_deferred_auto = False
        if on == self.item_deferred:
            return
        if not on:
            self.sync()
        self.item_deferred = on
        self._c.Gi_defer = int(on)

    def set_deferred(self, on):
        """Switch the deferred decay off (data-parallel owners that run the step as grads + collective + apply) or on again."""
        on = bool(on)
        self._deferred_auto = False
        if on == self.deferred:
            return
        if on:
            if not self.fused:
                raise ValueError("the deferred decay needs the fused user-side step (TF-dense Adam, compact user gradients, F % 4 == 0)")
            self._enable_deferred()
            return
        self.sync()
        self.deferred = False
        self._c.Gu_last = self.Gu_last = None                   # (the lr ring stays: the fused item side reads it too)
        if self.fused:                                          # the fused user-side step needs its second table from here on
            if self.Gu_next is None:
                self.Gu_next = torch.empty_like(self._Gu)
            self._c.Gu_next = self.Gu_next.data_ptr()

    def _swap_user_tables(self, steps=1):
        """After `steps` fused train steps the current user table is the other one of the pair (include/elliot_hip.h, Gu_next)."""
        if self.deferred:
            self._pending = True                                # in place; rows outside the batches wait for their replay
            return
        if self.fused and steps % 2:
            self._Gu, self.Gu_next = self.Gu_next, self._Gu
            self._c.Gu, self._c.Gu_next = self._Gu.data_ptr(), self.Gu_next.data_ptr()
            for c in getattr(self, "_c_clones", ()):
                c.Gu, c.Gu_next = self._c.Gu, self._c.Gu_next

    @property
    def step(self):
        return self._step

    @step.setter
    def step(self, value):
        """Moving the counter from outside (a checkpoint's count, a data-parallel owner's begin_step) is not an optimiser step:
        every row is first brought up to date at the old count and then stamped with the new one.  (The training calls of this
        class advance the counter through _advance.)"""
        value = int(value)
        if self.compact and value < self._step:
            self.uslot.zero_()                 # stamps of later steps must not be mistaken for this step's gradient rows
        if value != self._step:
            if getattr(self, "deferred", False):
                self.sync()
                self.Gu_last.fill_(value)
            if getattr(self, "item_fused", False):
                self.sync()
                self.Gi_last.fill_(value)
        self._step = value

    def _advance(self, n=1):
        """The counter of a training call: the library performs (or postpones, per row) exactly these optimiser steps."""
        self._step += int(n)

    def _after_steps(self, steps=1):
        self._swap_user_tables(steps)
        if self.item_fused and self.item_deferred:
            self._pending_items = True

    def _two_pass(self, on):
        """grads() / apply() run the every-row two-pass form: the per-row features stand aside (rows current first) and come back
        with every row stamped at the step the dense pass left it at."""
        if on:
            self.sync()
            self._c.Gu_last = None
            self._c.Gi_last = None
            return
        if self.deferred:
            self.Gu_last.fill_(self._step)
            self._c.Gu_last = self.Gu_last.data_ptr()
        if self.item_fused:
            self.Gi_last.fill_(self._step)
            self._c.Gi_last = self.Gi_last.data_ptr()

    def ensure_rows(self, B):
        """Compact mode: gradient rows for a batch of B triplets (slot = sorted position of a user's first occurrence)."""
        if self.compact and (self.gGu_rows is None or self.gGu_rows.shape[0] < B):
            self.gGu_rows = torch.empty((int(B), self.F), dtype=torch.float32, device=self.ctx.device)
            self._c.gGu_rows = self.gGu_rows.data_ptr()
            self._c.gGu_cap = int(B)
            for c in getattr(self, "_c_clones", ()):                      # (multi-GPU: split user / item apply states)
                c.gGu_rows, c.gGu_cap = self._c.gGu_rows, self._c.gGu_cap

    def user_grad_dense(self):
        """Dense [U,F] view of the user-row gradients of the LAST gradient pass (tests / diagnostics): the accumulator itself, or
        the compact rows scattered by their stamps."""
        if not self.compact:
            return self.gGu
        out = torch.zeros((self.U, self.F), dtype=torch.float32, device=self.ctx.device)
        ent = self.uslot
        hit = (ent >> 32) == max(int(self.uslot.max().item()) >> 32, 1)
        rows = torch.nonzero(hit).flatten()
        out[rows] = self.gGu_rows[(ent[rows] & 0xFFFFFFFF)]
        return out

    def train_step(self, u, i, j, lr, l_w, l_b, algo="auto"):
        """BPRMF_batch_model.train_step (BPRMF_batch_model.py:58-80).  u,i,j: int32 device tensors.
        The batch loss is accumulated into self.loss (device double) -- no host sync here."""
        B = u.numel()
        if self.compact:
            self._resolve_deferred(B)           # (before the step counter moves: switching the deferred decay stamps the rows with it)
        self._advance()
        lr_t = adam_lr_t(lr, self.step)
        algo = BPR_ALGOS[algo] if isinstance(algo, str) else int(algo)
        ws, ws_bytes = None, 0
        if self.compact:
            if algo == _lib.EL_BPR_ATOMIC:
                raise ValueError("compact user-gradient rows need the sorted gradient path")
            if not self.fused:
                self.ensure_rows(B)
        if algo == _lib.EL_BPR_SORTED or (algo == _lib.EL_BPR_AUTO and B >= 2048) or self.compact:
            t = self.sort_workspace(B, "_ws")
            ws, ws_bytes = _ptr(t), t.numel()
        check(self.ctx.lib.el_bprmf_train_step(self.ctx.handle, self.ctx.stream(), C.byref(self._c),
                                               _ptr(u, torch.int32, "u"), _ptr(i, torch.int32, "i"),
                                               _ptr(j, torch.int32, "j"), int(B), float(lr), float(l_w), float(l_b),
                                               self.opt, int(self.step), float(lr_t), _ptr(self.loss, torch.float64),
                                               algo, ws, ws_bytes),
              "el_bprmf_train_step")
        self._after_steps()

    def grads(self, u, i, j, l_w, l_b):
        """First half of train_step: loss + the summed row gradients of the batch (what OptimizerV2 receives after its segment
        sum, BPRMF_batch_model.py:77) into gGu (or the compact rows) / gGi / gBi, no optimiser.  apply() consumes them."""
        B = u.numel()
        ws = self.sort_workspace(B, "_ws")
        self.ensure_rows(B)
        if self.deferred or self.item_fused:
            # the two-call form runs the every-row passes (apply); the rows are brought up to date and the features stand aside
            self._two_pass(True)
        check(self.ctx.lib.el_bprmf_grads(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32, "u"),
                                          _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"), int(B), float(l_w), float(l_b),
                                          int(self.step + 1), _ptr(self.loss, torch.float64), _ptr(ws), ws.numel()),
              "el_bprmf_grads")

    def apply(self, lr):
        """Second half: the optimiser (TF-dense Adam / dense SGD) on the accumulated gradients; accumulators come back clean."""
        if self.deferred or self.item_fused:
            self._two_pass(True)                               # (apply() without a grads() in front: the same stand-aside)
        self._advance()
        check(self.ctx.lib.el_bprmf_apply(self.ctx.handle, self.ctx.stream(), C.byref(self._c), float(lr), int(self.opt),
                                          int(self.step), float(adam_lr_t(lr, self.step))), "el_bprmf_apply")
        if self.deferred or self.item_fused:
            self._two_pass(False)                              # the every-row passes moved every row

    # -- the step in two halves for a software pipeline: ordering a batch (prep + radix sort) reads only its triplets, so the
    #    batch of step t+1 can be drawn and ordered on a side stream while step t's segment kernels and optimiser pass run
    def sort_workspace(self, B, attr=None):
        """A workspace tensor for presort() / train_step_presorted() (el_bprmf_ws_bytes): one per batch in flight -- or, with
        attr, the one this state keeps for its own steps."""
        return workspace(self, attr, int(self.ctx.lib.el_bprmf_ws_bytes(int(B), int(self.U), int(self.I), int(self.F))), self.ctx.device)

    def presort(self, u, i, j, ws):
        """First half of the sorted gradient path: (row, triplet) pairs of the batch, ordered, into `ws` (current stream)."""
        check(self.ctx.lib.el_bprmf_presort(self.ctx.handle, self.ctx.stream(), _ptr(u, torch.int32, "u"), _ptr(i, torch.int32, "i"),
                                            _ptr(j, torch.int32, "j"), int(u.numel()), int(self.U), int(self.I),
                                            C.c_void_p(ws.data_ptr()), ws.numel()), "el_bprmf_presort")

    def train_step_presorted(self, u, i, j, lr, l_w, l_b, ws):
        """train_step on a batch that presort() ordered into `ws`: segment kernels + loss, then the optimiser -- the same kernels,
        the same results as train_step(algo="sorted")."""
        B = u.numel()
        if self.opt not in (EL_OPT_ADAM_TF_DENSE, EL_OPT_SGD) or self.tGu is not None:
            raise ValueError("train_step_presorted: the dense optimisers only (adam_tf_dense, sgd_dense)")
        if not self.fused:
            self.ensure_rows(B)
        self._resolve_deferred(B)
        self._advance()
        check(self.ctx.lib.el_bprmf_train_step_presorted(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32, "u"),
                                                         _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"), int(B), float(lr), float(l_w),
                                                         float(l_b), int(self.opt), int(self.step), float(adam_lr_t(lr, self.step)),
                                                         _ptr(self.loss, torch.float64), C.c_void_p(ws.data_ptr()), ws.numel()),
              "el_bprmf_train_step_presorted")
        self._after_steps()

    def train_loop(self, pos, events, B, seed, first_sample, lr, l_w, l_b, algo="auto"):
        """One epoch of `for batch in sampler.step(events, B): train_step(batch)` (BPRMF_batch.py:100-109) from a single
        library call: the same Philox stream and the same kernels as the per-batch calls, no host round trip in between."""
        steps = (int(events) + int(B) - 1) // int(B)
        if steps == 0:
            return 0
        if pos.n_rows != self.U or pos.n_cols != self.I:
            raise ValueError("train_loop: the positives' CSR must describe this state's users x items")
        algo = BPR_ALGOS[algo] if isinstance(algo, str) else int(algo)
        lr_t = self._lr_t_host = np.array([adam_lr_t(lr, self.step + 1 + k) for k in range(steps)], dtype=np.float32)
        # (kept alive on self: the library may copy the table with an asynchronous memcpy on the stream)
        if not self.fused:
            self.ensure_rows(B)
        self._resolve_deferred(B)
        need = int(self.ctx.lib.el_bprmf_ws_bytes(int(B), int(self.U), int(self.I), int(self.F))) if (B >= 2048 or self.compact) else 0
        ws = workspace(self, "_ws", need, self.ctx.device) if need else None
        lneed = int(self.ctx.lib.el_bprmf_train_loop_ws_bytes(int(events), int(B)))
        buf = getattr(self, "_loop_ws", None)
        if buf is None or buf.numel() != lneed:                          # (a stable address keeps the captured graph valid)
            buf = self._loop_ws = torch.empty(lneed, dtype=torch.uint8, device=self.ctx.device)
        check(self.ctx.lib.el_bprmf_train_loop(
            self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(pos), int(seed) & 0xFFFFFFFFFFFFFFFF,
            int(first_sample), int(events), int(B), float(lr), float(l_w), float(l_b), self.opt, int(self.step + 1),
            lr_t.ctypes.data_as(C.c_void_p), _ptr(self.loss, torch.float64), algo,
            _ptr(ws), ws.numel() if ws is not None else 0,
            C.c_void_p(buf.data_ptr()), lneed, C.c_void_p(sampler_meta(self.ctx, pos).data_ptr())), "el_bprmf_train_loop")
        self._advance(steps)                                    # (consecutive steps: not a jump of the counter)
        self._after_steps(steps)
        return steps

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v


class AmfDeviceState:
    """AMF_model's variables (adversarial/AMF/AMF_model.py:41-51): a BprmfDeviceState with the dense accumulators -- Gu, Gi, Bi and
    ONE Adam whose step counter plain and adversarial steps share -- plus the two perturbation tables, which are not trained, and
    the device list of their non-zero rows (el_amf_delta).  An AMF step is el_amf_grads + the state's own apply()."""

    def __init__(self, ctx, Gu, Gi, Bi, delta_Gu=None, delta_Gi=None):
        self.ctx = ctx
        # (without compact user gradients the wrapped state has no per-row features: nothing stands aside for the library's calls)
        self.base = BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam", compact_user_grads=False)
        b, dev = self.base, ctx.device
        self.U, self.I, self.F = b.U, b.I, b.F
        self.dGu = torch.zeros((self.U, self.F), dtype=torch.float32, device=dev)
        self.dGi = torch.zeros((self.I, self.F), dtype=torch.float32, device=dev)
        self.rows_u = torch.zeros(self.U, dtype=torch.int32, device=dev)
        self.rows_i = torch.zeros(self.I, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int32, device=dev)
        self._d = _lib.AmfDelta(dGu=self.dGu.data_ptr(), dGi=self.dGi.data_ptr(), rows_u=self.rows_u.data_ptr(),
                                rows_i=self.rows_i.data_ptr(), counts=self.counts.data_ptr())
        self.delta_is_zero = True               # known on the host: plain steps may then take the BPR fast path
        self._ws = self._Pu = self._Pi = None
        if delta_Gu is not None:
            self.set_delta(delta_Gu, delta_Gi)

    loss = property(lambda self: self.base.loss)
    step = property(lambda self: self.base.step)

    def pop_loss(self):
        return self.base.pop_loss()

    def _workspace(self, B):
        return workspace(self, "_ws", int(self.ctx.lib.el_amf_ws_bytes(int(B), self.U, self.I, self.F)), self.ctx.device)

    def _call(self, fn, name, u, i, j, *rest):
        ws = self._workspace(u.numel())
        head = (self.ctx.handle, self.ctx.stream(), C.byref(self.base._c), C.byref(self._d), _ptr(u, torch.int32, "u"),
                _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"), int(u.numel()))
        check(fn(*head, *rest, _ptr(ws), ws.numel()), name)

    def grads(self, u, i, j, l_w, l_b, l_adv=0.0, eps=0.0, adversarial=False):
        """Loss and tape.gradient of train_step (AMF_model.py:70-102) into the accumulators; adversarial=True adds the l_adv term and
        rebuilds delta from this batch (the gradients still read the delta of the previous step)."""
        self._call(self.ctx.lib.el_amf_grads, "el_amf_grads", u, i, j, float(l_w), float(l_b), float(l_adv), float(eps),
                   _lib.EL_AMF_ADVERSARIAL if adversarial else 0, _ptr(self.base.loss, torch.float64))
        if adversarial:
            self.delta_is_zero = False

    def apply(self, lr):
        self.base.apply(lr)

    def train_step(self, u, i, j, lr, l_w, l_b, l_adv, eps, adversarial):
        self.grads(u, i, j, l_w, l_b, l_adv, eps, adversarial)
        self.apply(lr)

    def perturb(self, u, i, j, l_w, l_b, eps, eps_iter=0.0, nb_iter=0):
        """build_perturbation (nb_iter = 0) / build_msap_perturbation (AMF_model.py:133-197): delta only, no optimiser."""
        self._call(self.ctx.lib.el_amf_perturb, "el_amf_perturb", u, i, j, float(l_w), float(l_b), float(eps), float(eps_iter),
                   int(nb_iter))
        self.delta_is_zero = False

    def clear_delta(self):
        check(self.ctx.lib.el_amf_delta_clear(self.ctx.handle, self.ctx.stream(), C.byref(self.base._c), C.byref(self._d)),
              "el_amf_delta_clear")
        self.delta_is_zero = True

    def set_delta(self, delta_Gu, delta_Gi):
        """Perturbation tables from outside (a checkpoint): the row lists are rebuilt from their non-zero rows."""
        for dst, rows, slot, src in ((self.dGu, self.rows_u, 0, delta_Gu), (self.dGi, self.rows_i, 1, delta_Gi)):
            dst.copy_(torch.as_tensor(np.ascontiguousarray(src)) if isinstance(src, np.ndarray) else src)
            nz = torch.nonzero((dst != 0).any(dim=1)).flatten().to(torch.int32)
            rows[:nz.numel()] = nz
            self.counts[slot] = int(nz.numel())
        self.delta_is_zero = int(self.counts.sum().item()) == 0

    def perturbed_tables(self):
        """(Gu + dGu, Gi + dGi) in fp32 scratch tables -- what predict(adversarial=True) multiplies (AMF_model.py:110-111)."""
        if self._Pu is None:
            self._Pu, self._Pi = torch.empty_like(self.dGu), torch.empty_like(self.dGi)
        check(self.ctx.lib.el_amf_perturbed_tables(self.ctx.handle, self.ctx.stream(), C.byref(self.base._c), C.byref(self._d),
                                                   _ptr(self._Pu, torch.float32), _ptr(self._Pi, torch.float32)),
              "el_amf_perturbed_tables")
        return self._Pu, self._Pi


class VbprDeviceState:
    """VBPR_model's variables (visual_recommenders/VBPR/VBPR_model.py:40-53): a BprmfDeviceState with the dense accumulators for
    Gu, Gi, Bi and ONE Adam step counter, plus Tu [U, Fd] and EB = [E | Bp] [D, Fd + 1] with their accumulators and slots, and
    the item features `feat` [I, D] (a device tensor, shared, never written).  A step is el_vbpr_grads + el_vbpr_apply; scoring
    goes through the image (P, Q, bq) = ([Gu | Tu], [Gi | feat E], Bi + feat Bp), rebuilt by image() on demand."""

    def __init__(self, ctx, Gu, Gi, Bi, Tu, E, Bp, feat):
        self.ctx = ctx
        self.base = BprmfDeviceState(ctx, Gu, Gi, Bi, optimizer="adam", compact_user_grads=False)
        b, dev = self.base, ctx.device
        self.U, self.I, self.F = b.U, b.I, b.F

        self.Tu = _own(Tu, dev)
        self.Fd = int(self.Tu.shape[1])
        if not isinstance(feat, torch.Tensor) or feat.device != dev or feat.dtype != torch.float32 or not feat.is_contiguous():
            raise ValueError("VbprDeviceState: feat must be a contiguous float32 tensor on the context's device")
        self.feat = feat
        self.D = int(feat.shape[1])
        E, Bp = _own(E, dev), _own(Bp, dev).reshape(-1, 1)
        if tuple(feat.shape) != (self.I, self.D) or tuple(E.shape) != (self.D, self.Fd) or Bp.shape[0] != self.D \
                or self.Tu.shape[0] != self.U:
            raise ValueError("VbprDeviceState: shapes of Tu / E / Bp / feat do not fit")
        self.EB = torch.cat([E, Bp], dim=1).contiguous()
        z = torch.zeros_like
        self.gTu, self.mTu, self.vTu = z(self.Tu), z(self.Tu), z(self.Tu)
        self.gEB, self.mEB, self.vEB = z(self.EB), z(self.EB), z(self.EB)
        self._c = _lib.VbprState(mf=b._c, Tu=self.Tu.data_ptr(), gTu=self.gTu.data_ptr(), mTu=self.mTu.data_ptr(),
                                 vTu=self.vTu.data_ptr(), EB=self.EB.data_ptr(), gEB=self.gEB.data_ptr(), mEB=self.mEB.data_ptr(),
                                 vEB=self.vEB.data_ptr(), Feat=self.feat.data_ptr(), Fd=self.Fd, D=self.D)
        self._ws = self._image_ws = self._P = self._Q = self._bq = None
        self.last_distinct_items = 0

    loss = property(lambda self: self.base.loss)
    step = property(lambda self: self.base.step)
    E = property(lambda self: self.EB[:, :self.Fd])
    Bp = property(lambda self: self.EB[:, self.Fd:])

    def pop_loss(self):
        return self.base.pop_loss()

    def grads(self, u, i, j, l_w, l_b, l_e):
        """Loss and tape.gradient of train_step (VBPR_model.py:72-92) into the accumulators; apply() consumes them."""
        B = int(u.numel())
        ws = workspace(self, "_ws", int(self.ctx.lib.el_vbpr_ws_bytes(self.ctx.handle, B, self.U, self.I, self.F, self.Fd, self.D)),
                       self.ctx.device)
        n = C.c_int64(0)
        check(self.ctx.lib.el_vbpr_grads(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32, "u"),
                                         _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"), B, float(l_w), float(l_b), float(l_e),
                                         _ptr(self.base.loss, torch.float64), C.byref(n), _ptr(ws), ws.numel()), "el_vbpr_grads")
        self.last_distinct_items = int(n.value)

    def apply(self, lr):
        self.base._advance()
        check(self.ctx.lib.el_vbpr_apply(self.ctx.handle, self.ctx.stream(), C.byref(self._c), float(lr), int(self.step),
                                         float(adam_lr_t(lr, self.step))), "el_vbpr_apply")

    def train_step(self, u, i, j, lr, l_w, l_b, l_e):
        self.grads(u, i, j, l_w, l_b, l_e)
        self.apply(lr)

    def image(self):
        """(P, Q, bq) of the current weights: x(u, i) = bq[i] + P[u] . Q[i] (el_vbpr_item_image)."""
        W = self.F + self.Fd
        if self._Q is None:
            dev = self.ctx.device
            self._P = torch.empty((self.U, W), dtype=torch.float32, device=dev)
            self._Q = torch.empty((self.I, W), dtype=torch.float32, device=dev)
            self._bq = torch.empty(self.I, dtype=torch.float32, device=dev)
        ws = workspace(self, "_image_ws", int(self.ctx.lib.el_vbpr_image_ws_bytes(self.ctx.handle, self.I, self.Fd, self.D)),
                       self.ctx.device)
        check(self.ctx.lib.el_vbpr_item_image(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(self._Q, torch.float32),
                                              _ptr(self._bq, torch.float32), _ptr(self._P, torch.float32), _ptr(ws), ws.numel()),
              "el_vbpr_item_image")
        return self._P, self._Q, self._bq


# ------------------------------------------------------------------------------------------
# graph propagation: LightGCN (graph_based/lightgcn) -- SURVEY 8f N3
# ------------------------------------------------------------------------------------------
SPMM_CHUNK = 512          # el_graph.hip: SPMM_CH


def normalized_bipartite_laplacian(train_csr_indptr, train_csr_indices, n_users, n_items):
    """LightGCN._create_adj_mat (LightGCN.py:96-118) without the dok / lil detour: the symmetric adjacency over U + I nodes (users first),
    D^-1/2 A D^-1/2 with the reference's arithmetic -- fp32 row sums + 1e-7 (added in fp32), power -1/2 in fp32, the two diagonal
    products one fp32 multiplication each: value(r, c) = fl(fl(1 * dinv[c]) * dinv[r]).  Returns CSR (indptr int64, indices int32
    ascending, vals fp32) as NumPy arrays.  (The reference's own construction is pinned against this one in tests/test_oracle_graph.py.)"""
    import scipy.sparse as sp
    indptr = np.asarray(train_csr_indptr, dtype=np.int64)
    cols = np.asarray(train_csr_indices, dtype=np.int64)
    T = cols.shape[0]
    rows = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(indptr))
    N = n_users + n_items
    A = sp.csr_matrix((np.ones(2 * T, np.float32), (np.concatenate([rows, cols + n_users]), np.concatenate([cols + n_users, rows]))), shape=(N, N))
    A.sum_duplicates()
    A.data[:] = 1.0                                              # (a dok assignment of the ratings matrix: entries are the stored values;
    #                                                               sp_i_train holds ones, dataset.py:236-241)
    rowsum = np.asarray(A.sum(1), dtype=np.float32).reshape(-1)
    rowsum = rowsum + np.float32(1e-7)
    dinv = np.power(rowsum, np.float32(-0.5)).astype(np.float32)
    dinv[np.isinf(dinv)] = 0.0
    A.sort_indices()
    r = np.repeat(np.arange(N, dtype=np.int64), np.diff(A.indptr))
    vals = (A.data.astype(np.float32) * dinv[A.indices]).astype(np.float32) * dinv[r]
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), vals.astype(np.float32)


def normalized_bipartite_laplacian_device(indptr, indices, n_users, n_items):
    """The same operator built on the device from a device CSR (large synthetic graphs: 1.6e8 non-zeros take a minute through SciPy).
    Same pattern and order; the values come from torch's fp32 pow, which may differ from NumPy's in the last bit -- the plugin (whose
    values are pinned to the reference's, tests/test_oracle_graph.py) uses the host builder above."""
    dev = indptr.device
    U, I = int(n_users), int(n_items)
    deg_u = (indptr[1:] - indptr[:-1])
    cols = indices.to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(U, device=dev, dtype=torch.int64), deg_u)
    deg_i = torch.bincount(cols, minlength=I)
    deg = torch.cat([deg_u, deg_i]).to(torch.float32) + torch.tensor(1e-7, dtype=torch.float32, device=dev)
    dinv = deg.pow(-0.5)
    order = torch.sort(cols * U + rows, stable=True).indices                       # item rows: (item, user) ascending
    t_rows, t_cols = cols[order], rows[order]
    lap_indptr = torch.cat([indptr, indptr[-1] + torch.cumsum(deg_i, 0)]).to(torch.int64)
    lap_indices = torch.cat([cols + U, t_cols]).to(torch.int32)
    r_all = torch.cat([rows, t_rows + U])
    vals = (dinv[lap_indices.long()] * dinv[r_all]).to(torch.float32)
    return lap_indptr, lap_indices, vals


class GraphCSR:
    """el_graph_csr: a sparse N x N operator over the stacked [users; items] table, device-resident, with the chunk decomposition
    of its product (every row cut into chunks of <= 512 non-zeros; multi-chunk rows reduce their partial rows in order)."""

    def __init__(self, ctx, indptr, indices, vals, n_users, width):
        dev = ctx.device
        self.ctx = ctx
        t = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
        self.indptr, self.indices, self.vals = t(indptr, torch.int64), t(indices, torch.int32), t(vals, torch.float32)
        self.N, self.n0, self.width = int(self.indptr.numel() - 1), int(n_users), int(width)
        ln = self.indptr[1:] - self.indptr[:-1]
        nch = torch.clamp((ln + SPMM_CHUNK - 1) // SPMM_CHUNK, min=1)                 # an empty row keeps one (empty) chunk
        first = torch.cumsum(nch, 0) - nch                                            # first chunk of every row
        n_chunks = int(nch.sum().item())
        row_of = torch.repeat_interleave(torch.arange(self.N, device=dev, dtype=torch.int64), nch)
        k_in_row = torch.arange(n_chunks, device=dev, dtype=torch.int64) - first[row_of]
        self.chunk_row = row_of.to(torch.int32)
        self.chunk_lo = (self.indptr[:-1][row_of] + k_in_row * SPMM_CHUNK).contiguous()
        multi = nch > 1
        mrows = torch.nonzero(multi).flatten()
        mcnt = nch[mrows]
        mfirst = torch.cumsum(mcnt, 0) - mcnt                                         # first partial slot of every multi-chunk row
        slot_of_row = torch.full((self.N,), -1, dtype=torch.int64, device=dev)
        slot_of_row[mrows] = mfirst
        cs = slot_of_row[row_of]
        self.chunk_slot = torch.where(cs >= 0, cs + k_in_row, cs).to(torch.int32)
        self.multi_row, self.multi_slot, self.multi_cnt = mrows.to(torch.int32), mfirst.to(torch.int32), mcnt.to(torch.int32)
        n_part = int(mcnt.sum().item()) if mrows.numel() else 0
        self.part = torch.empty((max(n_part, 1), self.width), dtype=torch.float32, device=dev)
        p = lambda x: x.data_ptr()
        self._c = _lib.GraphCsr(indptr=p(self.indptr), indices=p(self.indices), vals=p(self.vals), N=self.N, n0=self.n0,
                                chunk_row=p(self.chunk_row), chunk_lo=p(self.chunk_lo), chunk_slot=p(self.chunk_slot), n_chunks=n_chunks,
                                multi_row=p(self.multi_row) if mrows.numel() else None, multi_slot=p(self.multi_slot) if mrows.numel() else None,
                                multi_cnt=p(self.multi_cnt) if mrows.numel() else None, n_multi=int(mrows.numel()), part=p(self.part))

    @property
    def nnz(self):
        return int(self.indices.numel())

    def spmm(self, X0, X1, out0=None, out1=None):
        """[Y0; Y1] = L [X0; X1] (el_spmm_csr_f32)."""
        F = int(X0.shape[1])
        if F > self.width:
            raise ValueError("GraphCSR was sized for narrower tables")
        out0 = torch.empty_like(X0) if out0 is None else out0
        out1 = torch.empty_like(X1) if out1 is None else out1
        check(self.ctx.lib.el_spmm_csr_f32(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(X0, torch.float32), _ptr(X1, torch.float32),
                                           F, _ptr(out0, torch.float32), _ptr(out1, torch.float32)), "el_spmm_csr_f32")
        return out0, out1


class LightGcnDeviceState:
    """LightGCN_model (graph_based/lightgcn/LightGCN_model.py:19-172) in HBM: Gu / Gi with Keras Adam slots + the normalised adjacency.
    One train step = `_propagate_embeddings` (ASSIGNED to the variables, :93-94) + the BPR head of BPRMF_batch without an item bias and
    with the L2 term doubled (:150-158) + Adam's every-row apply -- the head runs on the segment kernels of the BPR-MF path
    (BprmfDeviceState with the every-row fused forms: the propagation reads and rewrites every row each step, nothing may wait)."""

    def __init__(self, ctx, Gu, Gi, graph, n_layers=1):
        self.ctx, self.graph, self.n_layers = ctx, graph, int(n_layers)
        self.bpr = BprmfDeviceState(ctx, Gu, Gi, np.zeros(int(Gi.shape[0]), np.float32), optimizer="adam_tf_dense", deferred=False,
                                    item_deferred=False)
        self.U, self.I, self.F = self.bpr.U, self.bpr.I, self.bpr.F
        if graph.N != self.U + self.I or graph.n0 != self.U:
            raise ValueError("the graph does not describe these tables")
        need = int(ctx.lib.el_lightgcn_ws_bytes(self.U, self.I, self.F, self.n_layers))
        self._ws = workspace(self, None, max(need, 16), ctx.device)

    @property
    def Gu(self):
        return self.bpr.Gu

    @property
    def Gi(self):
        return self.bpr.Gi

    @property
    def step(self):
        return self.bpr.step

    def propagate(self):
        """_propagate_embeddings (:68-94), in place."""
        st = self.bpr
        st.sync()
        check(self.ctx.lib.el_lightgcn_propagate(self.ctx.handle, self.ctx.stream(), C.byref(self.graph._c), _ptr(st._Gu, torch.float32),
                                                 _ptr(st._Gi, torch.float32), self.F, self.n_layers, C.c_void_p(self._ws.data_ptr()),
                                                 self._ws.numel()), "el_lightgcn_propagate")

    def train_step(self, u, i, j, lr, l_w):
        """train_step (:136-167): propagate, then the BPR step on the propagated tables.  reg_loss = l_w * sum(l2_loss) * 2 is the
        BPRMF_batch head's l_w * sum(l2_loss) with twice the coefficient; there is no item bias: the bias slot of the BPR state is
        kept at zero (its gradient -- the triplet's dloss/dd -- is discarded after every step), l_b = 0."""
        self.propagate()
        st = self.bpr
        st.train_step(u, i, j, lr, 2.0 * float(l_w), 0.0)
        st.sync()
        st._Bi.zero_()
        st.mBi.zero_()
        st.vBi.zero_()

    def pop_loss(self):
        return self.bpr.pop_loss()


class NgcfDeviceState:
    """NGCFModel (graph_based/ngcf/NGCF_model.py:18-226) in HBM.  Gu / Gi are [rows, sum(weight_size_list)] wide (:88-91): the first
    embed_k columns are the trainable layer-0 embeddings, the others are REWRITTEN by every `_propagate_embeddings` (:106-142) with the
    row-normalised outputs of the propagation layers; the BPR head (bias-free, L2 doubled, :199-209) and Adam act on the full-width rows.
    The GraphLayers (W_1, b_1, W_2, b_2 per layer) see the loss through reg_loss only -- the propagated tables are ASSIGNED (:141-142) --
    so their Adam step runs on g = 2 l_w theta (el_adam_l2_dense).  layers: [{"W1": [kin, kout], "b1": [1, kout], "W2", "b2"}, ...]."""

    def __init__(self, ctx, Gu, Gi, graph, layers, embed_k, message_dropout=None, dropout_seed=42):
        self.ctx, self.graph, self.embed_k = ctx, graph, int(embed_k)
        dev = ctx.device
        self.bpr = BprmfDeviceState(ctx, Gu, Gi, np.zeros(int(Gi.shape[0]), np.float32), optimizer="adam_tf_dense", deferred=False,
                                    item_deferred=False)
        self.U, self.I, self.W = self.bpr.U, self.bpr.I, self.bpr.F
        self.layers = [{k: _own(v, dev) for k, v in l.items()} for l in layers]
        self.slots = [{k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in l.items()} for l in self.layers]
        sizes = [self.embed_k] + [int(l["W1"].shape[1]) for l in self.layers]
        if sum(sizes) != self.W or any(int(l["W1"].shape[0]) != sizes[n] for n, l in enumerate(self.layers)):
            raise ValueError("layer shapes do not chain to the table width")
        self.sizes = sizes
        self.message_dropout = [float(x) for x in (message_dropout or [0.0] * len(self.layers))]
        self.dropout_seed = int(dropout_seed)
        N, kmax = self.U + self.I, max(sizes)
        self._lap = torch.empty((N, kmax), dtype=torch.float32, device=dev)
        self._x2 = torch.empty((N, 2 * kmax), dtype=torch.float32, device=dev)
        self._s = torch.empty((N, kmax), dtype=torch.float32, device=dev)
        self._ego = [torch.empty((N, kmax), dtype=torch.float32, device=dev) for _ in range(2)]

    @property
    def Gu(self):
        return self.bpr.Gu

    @property
    def Gi(self):
        return self.bpr.Gi

    @property
    def step(self):
        return self.bpr.step

    def propagate(self):
        """_propagate_embeddings (:106-142), in place on the column blocks of Gu / Gi."""
        st, ctx, U, N = self.bpr, self.ctx, self.U, self.U + self.I
        st.sync()
        k0 = self.embed_k
        ego = self._ego[0].view(-1)[:N * k0].view(N, k0)
        ego[:U].copy_(st._Gu[:, :k0])
        ego[U:].copy_(st._Gi[:, :k0])
        off = k0
        for n, l in enumerate(self.layers):
            kin, kout = self.sizes[n], self.sizes[n + 1]
            lap = self._lap.view(-1)[:N * kin].view(N, kin)
            self.graph.spmm(ego[:U], ego[U:], lap[:U], lap[U:])
            x2 = self._x2.view(-1)[:N * 2 * kin].view(N, 2 * kin)
            check(ctx.lib.el_ngcf_pre(ctx.handle, ctx.stream(), _ptr(ego, torch.float32), _ptr(lap, torch.float32), N, kin, _ptr(x2, torch.float32)), "el_ngcf_pre")
            wcat = torch.cat([l["W1"], l["W2"]], 0)
            bcat = (l["b1"] + l["b2"]).reshape(-1)
            s = self._s.view(-1)[:N * kout].view(N, kout)
            gemm(ctx, x2, wcat, bias=bcat, out=s)
            nxt = self._ego[(n + 1) & 1].view(-1)[:N * kout].view(N, kout)
            check(ctx.lib.el_ngcf_post(ctx.handle, ctx.stream(), _ptr(s, torch.float32), N, U, kout, float(self.message_dropout[n]),
                                       self.dropout_seed & 0xFFFFFFFFFFFFFFFF, int(st.step * 16 + n) & 0xFFFFFFFF, _ptr(nxt, torch.float32),
                                       _ptr(st._Gu, torch.float32), _ptr(st._Gi, torch.float32), self.W, off), "el_ngcf_post")
            ego, off = nxt, off + kout

    def train_step(self, u, i, j, lr, l_w):
        """train_step (:187-217): propagate, the bias-free BPR step with the doubled L2 term on the full-width rows, the GraphLayers' L2-only
        Adam step; the batch loss includes l_w * sum ||layer parameter||^2 (:203-206)."""
        self.propagate()
        st, ctx = self.bpr, self.ctx
        st.train_step(u, i, j, lr, 2.0 * float(l_w), 0.0)
        st.sync()
        st._Bi.zero_(), st.mBi.zero_(), st.vBi.zero_()
        reg = sum((p.double() ** 2).sum() for l in self.layers for p in l.values())
        st.loss += float(l_w) * reg                                   # (device arithmetic: no synchronisation)
        lr_t = adam_lr_t(lr, st.step)
        for l, sl in zip(self.layers, self.slots):
            for k, p in l.items():
                m, v = sl[k]
                check(ctx.lib.el_adam_l2_dense(ctx.handle, ctx.stream(), _ptr(p, torch.float32), _ptr(m, torch.float32), _ptr(v, torch.float32),
                                               p.numel(), float(lr_t), 2.0 * float(l_w)), "el_adam_l2_dense")

    def pop_loss(self):
        return self.bpr.pop_loss()

# ------------------------------------------------------------------------------------------
# BPRMF (NumPy semantics, fp64)
# ------------------------------------------------------------------------------------------
class BprSgdDeviceState:
    """MFModel parameters in HBM (BPRMF_model.py:40-56), fp64."""

    def __init__(self, ctx, P, Q, b, lr, reg_bias, reg_user, reg_pos, reg_neg):
        self.ctx = ctx
        dev = ctx.device

        self.P, self.Q, self.b = (_own(x, dev, torch.float64) for x in (P, Q, b))
        self.U, self.F = self.P.shape
        self.I = self.Q.shape[0]
        self._c = BprsgdState(P=self.P.data_ptr(), Q=self.Q.data_ptr(), b=self.b.data_ptr(), U=self.U, I=self.I,
                              F=self.F, lr=float(lr), reg_bias=float(reg_bias), reg_user=float(reg_user),
                              reg_pos=float(reg_pos), reg_neg=float(reg_neg))

    def apply(self, u, i, j, first=0, n=None):
        """Concurrent application of triplets [first, first+n) (Hogwild unless conflict-free)."""
        if n is None:
            n = u.numel() - first
        check(self.ctx.lib.el_bprsgd_apply(self.ctx.handle, self.ctx.stream(), C.byref(self._c),
                                           _ptr(u, torch.int32), _ptr(i, torch.int32), _ptr(j, torch.int32),
                                           int(first), int(n)), "el_bprsgd_apply")

    def apply_sequential_equivalent(self, u_host, i_host, j_host):
        """Bit-for-bit the sequential order of MFModel.train_step (BPRMF_model.py:87-89): triplets are
        grouped into dependency levels on the host, each level is one conflict-free launch."""
        order, starts = sgd_levels(u_host, i_host, j_host, self.U, self.I)
        dev = self.ctx.device
        u = torch.from_numpy(np.ascontiguousarray(u_host[order], dtype=np.int32)).to(dev)
        i = torch.from_numpy(np.ascontiguousarray(i_host[order], dtype=np.int32)).to(dev)
        j = torch.from_numpy(np.ascontiguousarray(j_host[order], dtype=np.int32)).to(dev)
        check(self.ctx.lib.el_bprsgd_apply_levels(self.ctx.handle, self.ctx.stream(), C.byref(self._c),
                                                  _ptr(u), _ptr(i), _ptr(j), starts.ctypes.data_as(C.c_void_p),
                                                  int(starts.shape[0] - 1)), "el_bprsgd_apply_levels")
        return int(starts.shape[0] - 1)


class Mf2020DeviceState:
    """MFModel of MF2020 (latent_factor_models/MF2020/MF_model.py:14-56) in HBM, fp64: user / item factors, the two bias vectors, the
    global bias.  train(samples) = MFModel.train_step (:80-113) on one batch of (user, item, rating) rows, in order."""

    def __init__(self, ctx, P, Q, bu=None, bi=None, gb=0.0, lr=0.05, reg=0.0):
        self.ctx = ctx
        dev = ctx.device
        self.P, self.Q = _own(P, dev, torch.float64), _own(Q, dev, torch.float64)
        self.U, self.F = int(self.P.shape[0]), int(self.P.shape[1])
        self.I = int(self.Q.shape[0])
        self.bu = _own(bu, dev, torch.float64) if bu is not None else torch.zeros(self.U, dtype=torch.float64, device=dev)
        self.bi = _own(bi, dev, torch.float64) if bi is not None else torch.zeros(self.I, dtype=torch.float64, device=dev)
        self.gb = torch.full((1,), float(gb), dtype=torch.float64, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.lr, self.reg = float(lr), float(reg)
        self._c = _lib.Mf2020State(P=self.P.data_ptr(), Q=self.Q.data_ptr(), bu=self.bu.data_ptr(), bi=self.bi.data_ptr(), gb=self.gb.data_ptr(),
                                   U=self.U, I=self.I, F=self.F, lr=self.lr, reg=self.reg)

    def train(self, samples):
        """samples: int32 [n, 3] device tensor of (user, item, rating) rows; the sum of their losses accumulates in self.loss."""
        s = samples.to(device=self.ctx.device, dtype=torch.int32).contiguous()
        check(self.ctx.lib.el_mf2020_train(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(s, torch.int32), int(s.shape[0]),
                                           _ptr(self.loss, torch.float64)), "el_mf2020_train")

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v

    def predictions(self):
        """prepare_predictions (:115-116): user_bias[:, None] + (global_bias + item_bias + P Q^T), fp64 [U, I] (small catalogues only:
        the reference materialises it too)."""
        return self.bu[:, None] + (self.gb + self.bi[None, :] + self.P @ self.Q.T)


def sgd_levels(u_host, i_host, j_host, U, I):
    """Host-only: dependency levels of a triplet sequence (el_bprsgd_levels_host)."""
    return _levels_host("el_bprsgd_levels_host", [np.ascontiguousarray(a, dtype=np.int32) for a in (u_host, i_host, j_host)],
                        (U, I))


# ------------------------------------------------------------------------------------------
# dense layers (fp32 MFMA GEMM) and Mult-VAE
# ------------------------------------------------------------------------------------------
ACTS = {None: 0, "none": 0, "tanh": 1, "relu": 2, "sigmoid": 3}


def gemm(ctx, A, B, transA=False, transB=False, bias=None, act=None, out=None, ws=True):
    """C = act(op(A) op(B) + bias) through el_gemm_f32 (keras Dense forward / backward products).  ws=False: no workspace (the
    library then never splits K)."""
    M = A.shape[1] if transA else A.shape[0]
    K = A.shape[0] if transA else A.shape[1]
    N = B.shape[0] if transB else B.shape[1]
    Kb = B.shape[1] if transB else B.shape[0]
    if K != Kb:
        raise ValueError(f"inner dimensions differ: {K} vs {Kb}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=ctx.device)
    need = int(ctx.lib.el_gemm_ws_bytes(ctx.handle, int(M), int(N), int(K))) if ws else 0
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=ctx.device) if need else None
    check(ctx.lib.el_gemm_f32(ctx.handle, ctx.stream(), int(bool(transA)), int(bool(transB)), int(M), int(N), int(K),
                              _ptr(A, torch.float32, "A"), int(A.stride(0)), _ptr(B, torch.float32, "B"),
                              int(B.stride(0)), _ptr(out, torch.float32, "C"), int(out.stride(0)),
                              _ptr(bias, torch.float32, "bias"), ACTS[act],
                              C.c_void_p(ws.data_ptr()) if ws is not None else None, need), "el_gemm_f32")
    return out


class VaeDeviceState:
    """Variables, Adam slots and activation buffers of the Mult-VAE in HBM (multi_vae_model.py:86-109).

    weights: dict with W1[I,H] b1[H] Wm[H,L] bm[L] Wv[H,L] bv[L] W3[L,H] b3[H] W4[H,I] b4[I] (Keras Dense
    kernel layout [in, out]); the mean / log-variance heads are stored side by side as one [H, 2L] matrix."""
    ORDER = ("W1", "b1", "Wmv", "bmv", "W3", "b3", "W4", "b4")

    def __init__(self, ctx, weights, max_batch):
        self.ctx = ctx
        dev = ctx.device
        f = {n: _own(x, dev) for n, x in weights.items()}
        W1, W4 = f["W1"], f["W4"]
        self.I, self.H = W1.shape
        self.L = int(weights["Wm"].shape[1])
        self.Bmax = int(max_batch)
        self.dae = "Wv" not in weights          # MultiDAE: mean head only, tanh on it, no sampling / KL (multi_dae_model.py)
        if self.dae:
            wmv, bmv = f["Wm"], f["bm"]
        else:
            wmv = torch.cat([f["Wm"], f["Wv"]], dim=1).contiguous()
            bmv = torch.cat([f["bm"], f["bv"]]).contiguous()
        t = {"W1": W1, "b1": f["b1"], "Wmv": wmv, "bmv": bmv, "W3": f["W3"], "b3": f["b3"], "W4": W4, "b4": f["b4"]}
        self.w = [t[n] for n in self.ORDER]
        self.g = [torch.zeros_like(x) for x in self.w]
        self.m = [torch.zeros_like(x) for x in self.w]
        self.v = [torch.zeros_like(x) for x in self.w]
        B, H, L, I = self.Bmax, self.H, self.L, self.I
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.h, self.mv, self.z, self.dz, self.h2 = z(B, H), z(B, 2 * L), z(B, L), z(B, L), z(B, H)
        self.logits, self.dh2, self.dmv, self.dh, self.rnorm = z(B, I), z(B, H), z(B, 2 * L), z(B, H), z(B)
        need = max(int(ctx.lib.el_gemm_ws_bytes(ctx.handle, *mnk)) for mnk in
                   ((B, H, I), (B, L, H), (B, H, 2 * L), (H, 2 * L, B), (L, H, B), (B, 2 * L, H), (H, I, B)))
        # twice what the products (and the dW1 scratch) need: el_vae_grads then runs the weight-gradient products on the library's
        # second stream with the upper half as their workspace (el_vae.hip, vae_grads)
        w1 = ((4 * (I + 1) + 4) * 4 + 255) // 256 * 256         # dW1's index arrays: at the end of the side half
        need = max(need, w1)
        self._ws = torch.empty(2 * ((max(need, 16) + 255) // 256 * 256 + w1) + 256, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.step = 0
        arr = lambda ts: (C.c_void_p * 8)(*[x.data_ptr() for x in ts])
        self._c = _lib.VaeState(I=I, H=H, L=L, Bmax=B, w=arr(self.w), g=arr(self.g), m=arr(self.m), v=arr(self.v),
                                h=self.h.data_ptr(), mv=self.mv.data_ptr(), z=self.z.data_ptr(), dz=self.dz.data_ptr(),
                                h2=self.h2.data_ptr(), logits=self.logits.data_ptr(), dh2=self.dh2.data_ptr(),
                                dmv=self.dmv.data_ptr(), dh=self.dh.data_ptr(), rnorm=self.rnorm.data_ptr(),
                                ws=self._ws.data_ptr(), ws_bytes=self._ws.numel(), dae=int(self.dae))

    def weights(self):
        """Host copies keyed like the constructor argument."""
        L = self.L
        w = {n: x.cpu().numpy() for n, x in zip(self.ORDER, self.w)}
        if self.dae:
            return {"W1": w["W1"], "b1": w["b1"], "Wm": w["Wmv"], "bm": w["bmv"], "W3": w["W3"], "b3": w["b3"],
                    "W4": w["W4"], "b4": w["b4"]}
        return {"W1": w["W1"], "b1": w["b1"], "Wm": w["Wmv"][:, :L].copy(), "Wv": w["Wmv"][:, L:].copy(),
                "bm": w["bmv"][:L].copy(), "bv": w["bmv"][L:].copy(), "W3": w["W3"], "b3": w["b3"], "W4": w["W4"],
                "b4": w["b4"]}

    def train_step(self, train_csr, rows, lr, anneal, eps=None, dropout_rate=0.0, dropout_seed=42):
        """VariationalAutoEncoder.train_step (multi_vae_model.py:125-142) on users `rows` (int32 device tensor)."""
        self.step += 1
        B = rows.numel()
        check(self.ctx.lib.el_vae_train_step(self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(train_csr),
                                             _ptr(rows, torch.int32, "rows"), int(B), _ptr(eps, torch.float32, "eps"),
                                             float(anneal), float(dropout_rate), int(dropout_seed), int(self.step),
                                             float(adam_lr_t(lr, self.step)), _ptr(self.loss, torch.float64)),
              "el_vae_train_step")

    def grads(self, train_csr, rows, anneal, eps=None, dropout_rate=0.0, dropout_seed=42, n_global=None):
        """Forward + loss + backward only; the batch means run over n_global rows (multi-GPU).  dense_grads() lists the buffers a
        data-parallel caller all-reduces before apply()."""
        B = rows.numel()
        check(self.ctx.lib.el_vae_grads(self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(train_csr),
                                        _ptr(rows, torch.int32, "rows"), int(B), int(B if n_global is None else n_global),
                                        _ptr(eps, torch.float32, "eps"), float(anneal), float(dropout_rate), int(dropout_seed),
                                        int(self.step + 1), _ptr(self.loss, torch.float64)), "el_vae_grads")

    def apply(self, lr):
        self.step += 1
        check(self.ctx.lib.el_vae_apply(self.ctx.handle, self.ctx.stream(), C.byref(self._c), float(adam_lr_t(lr, self.step))),
              "el_vae_apply")

    def dense_grads(self):
        return list(self.g)

    def predict(self, train_csr, rows, eps=None):
        """log_softmax(logits) [B, I] view of the activation buffer (multi_vae_model.py:144-155)."""
        B = rows.numel()
        check(self.ctx.lib.el_vae_predict(self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(train_csr),
                                          _ptr(rows, torch.int32, "rows"), int(B), _ptr(eps, torch.float32, "eps")),
              "el_vae_predict")
        return self.logits[:B]

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v


class AutoRecDeviceState:
    """Variables, Adam slots and step buffers of ItemAutoRec / UserAutoRec in HBM (userautorec_model.py:54-90,
    itemautorec_model.py:51-87).

    weights: dict with W1[N,H] b1[H] W2[H,N] b2[N] in Keras' Dense kernel layout [in, out]; the decoder kernel is held transposed
    on the device (W2T [N,H]).  out_act: None / "none" (UserAutoRec's linear head) or "sigmoid" (ItemAutoRec).  max_batch rows and
    nnz_max entries are what one training batch may hold (el_autorec_state)."""
    ORDER = ("W1", "b1", "W2T", "b2")

    def __init__(self, ctx, weights, out_act, max_batch, nnz_max):
        self.ctx = ctx
        dev = ctx.device
        W1, W2 = _own(weights["W1"], dev), _own(weights["W2"], dev)
        self.N, self.H = (int(x) for x in W1.shape)
        if tuple(W2.shape) != (self.H, self.N):
            raise ValueError(f"W2 must be [H, N] = {(self.H, self.N)}, got {tuple(W2.shape)}")
        self.out_act = ACTS[out_act]
        self.Bmax, self.nnz_max = int(max_batch), int(nnz_max)
        self.w = [W1, _own(weights["b1"], dev), W2.t().contiguous(), _own(weights["b2"], dev)]
        self.g = [torch.zeros_like(x) for x in self.w]
        self.m = [torch.zeros_like(x) for x in self.w]
        self.v = [torch.zeros_like(x) for x in self.w]
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.h, self.dh, self.d = z(self.Bmax, self.H), z(self.Bmax, self.H), z(max(self.nnz_max, 1))
        need = int(ctx.lib.el_autorec_ws_bytes(self.N, self.Bmax, self.nnz_max))
        self._ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)          # (zeros: its first word is the status)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.step = 0
        arr = lambda ts: (C.c_void_p * 4)(*[x.data_ptr() for x in ts])
        self._c = _lib.AutoRecState(N=self.N, H=self.H, out_act=self.out_act, Bmax=self.Bmax, nnz_max=self.nnz_max,
                                    w=arr(self.w), g=arr(self.g), m=arr(self.m), v=arr(self.v), h=self.h.data_ptr(),
                                    dh=self.dh.data_ptr(), d=self.d.data_ptr(), ws=self._ws.data_ptr(), ws_bytes=self._ws.numel())

    def weights(self):
        """Host copies keyed like the constructor argument (W2 back in Keras' [H, N] layout)."""
        w = {n: x.cpu().numpy() for n, x in zip(self.ORDER, self.w)}
        return {"W1": w["W1"], "b1": w["b1"], "W2": np.ascontiguousarray(w["W2T"].T), "b2": w["b2"]}

    def train_step(self, csr, rows, lr):
        """train_step (userautorec_model.py:92-107) on the rows `rows` (int32 device tensor) of `csr`."""
        self.step += 1
        check(self.ctx.lib.el_autorec_train_step(self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(csr),
                                                 _ptr(rows, torch.int32, "rows"), int(rows.numel()),
                                                 float(adam_lr_t(lr, self.step)), _ptr(self.loss, torch.float64)),
              "el_autorec_train_step")

    def grads(self, csr, rows, n_global=None):
        """Forward + loss + backward only; the batch mean runs over n_global rows."""
        B = rows.numel()
        check(self.ctx.lib.el_autorec_grads(self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(csr),
                                            _ptr(rows, torch.int32, "rows"), int(B), int(B if n_global is None else n_global),
                                            _ptr(self.loss, torch.float64)), "el_autorec_grads")

    def apply(self, lr):
        self.step += 1
        check(self.ctx.lib.el_autorec_apply(self.ctx.handle, self.ctx.stream(), C.byref(self._c),
                                            float(adam_lr_t(lr, self.step))), "el_autorec_apply")

    def dense_grads(self):
        return list(self.g)

    def encode(self, csr, rows, out=None):
        """sigmoid(x W1 + b1) [B, H] of the rows `rows` of `csr`."""
        B = rows.numel()
        if out is None:
            out = torch.empty((B, self.H), dtype=torch.float32, device=self.ctx.device)
        check(self.ctx.lib.el_autorec_encode(self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(csr),
                                             _ptr(rows, torch.int32, "rows"), int(B), _ptr(out, torch.float32, "out")),
              "el_autorec_encode")
        return out

    def predict_rows(self, csr, rows):
        """The model's output [B, N] for the rows `rows` of `csr` (predict, userautorec_model.py:109-119): act(h W2 + b2)."""
        h = self.encode(csr, rows)
        return gemm(self.ctx, h, self.w[2], transB=True, bias=self.w[3], act={0: None, 3: "sigmoid"}[self.out_act])

    def predict_columns(self, h_all, start, stop):
        """Rows [start, stop) of the TRANSPOSED output: out[u, i] = act(W2T[u] . h_all[i] + b2[u]) for the encodings h_all [n, H] of
        n rows -- the block itemautorec.py:104 gets by transposing on the host."""
        out = gemm(self.ctx, self.w[2][start:stop], h_all, transB=True)
        check(self.ctx.lib.el_autorec_rowbias_act(self.ctx.handle, self.ctx.stream(), _ptr(out, torch.float32, "C"),
                                                  int(out.shape[0]), int(out.shape[1]), int(out.stride(0)),
                                                  _ptr(self.w[3][start:stop], torch.float32, "bias"), int(self.out_act)),
              "el_autorec_rowbias_act")
        return out

    def pop_loss(self):
        """The loss summed since the last call.  Raises when a batch held more entries than nnz_max (that step computed nothing)."""
        v = float(self.loss.item())
        self.loss.zero_()
        if int(self._ws[:4].view(torch.int32).item()) != 0:
            self._ws[:4].zero_()
            raise _lib.ElliotHipError("el_autorec: a batch held more than nnz_max = %d entries" % self.nnz_max)
        return v


# ------------------------------------------------------------------------------------------
# NeuMF / GMF
# ------------------------------------------------------------------------------------------
def pointwise_sample(ctx, pos, n, seed, first_sample=0, use_meta=True, out=None):
    """pointwise_pos_neg_sampler.Sampler.step (pointwise_pos_neg_sampler.py:26-50) on the device (use_meta: through the per-user
    sampler records -- same draws, fewer cache lines).  out: (u int32[n], i int32[n], label float32[n]) to fill."""
    if out is not None:
        u, i, y = out
    else:
        u = torch.empty(n, dtype=torch.int32, device=ctx.device)
        i = torch.empty(n, dtype=torch.int32, device=ctx.device)
        y = torch.empty(n, dtype=torch.float32, device=ctx.device)
    meta = sampler_meta(ctx, pos) if use_meta else None
    check(ctx.lib.el_pointwise_sample_meta(ctx.handle, ctx.stream(), *_csr_ptrs(pos),
                                           C.c_void_p(meta.data_ptr()) if meta is not None else None, int(pos.n_rows),
                                           int(pos.n_cols), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sample), int(n), _ptr(u),
                                           _ptr(i), _ptr(y)), "el_pointwise_sample_meta")
    return u, i, y


class NmfDeviceState:
    """NeuMF / GMF variables, optimiser slots and activation buffers in HBM.

    weights: dict with optional "Umf" [U,F], "Imf" [I,F] (MF branch), "Umlp" [U,E], "Imlp" [I,E], "W" list of
    [in,out] kernels and "b" list of biases (MLP branch), "hw" head weights [F + units[-1]] and optional "hb" [1]."""

    _LR_HIST = 1 << 16          # optimiser steps of lr_t history kept on the device by the deferred decay

    def __init__(self, ctx, weights, max_batch, dropout=0.0, dropout_seed=42, deferred=None, replay="exact"):
        """deferred: Keras' every-row Adam decay of the embedding tables is postponed per row and replayed bit for bit when the
        row is next needed (include/elliot_hip.h, el_nmf_state.row_last).  None = on; a data-parallel
        owner that all-reduces gtab of replicated tables turns it off (set_deferred(False); parallel.ShardedNmf does)."""
        self.ctx = ctx
        dev = ctx.device
        if replay not in ("exact", "series"):
            raise ValueError("replay must be 'exact' or 'series'")
        self.replay = replay                                         # how waiting rows are brought forward (BprmfDeviceState: the same two modes)
        self.dropout, self.dropout_seed = float(dropout), int(dropout_seed)
        self.deferred = True if deferred is None else bool(deferred)
        self.use_mf = "Umf" in weights
        self.use_mlp = "Umlp" in weights
        self.head_bias = "hb" in weights
        names = ["Umf", "Imf", "Umlp", "Imlp"]
        self.tab = [_own(weights.get(n), dev) for n in names]
        ref = self.tab[0] if self.use_mf else self.tab[2]
        self.U = ref.shape[0]
        self.I = (self.tab[1] if self.use_mf else self.tab[3]).shape[0]
        self.F = self.tab[0].shape[1] if self.use_mf else 0
        self.E = self.tab[2].shape[1] if self.use_mlp else 0
        z = lambda t: None if t is None else torch.zeros_like(t)
        self.gtab, self.mtab, self.vtab, self._tab_blocks = [None] * 4, [None] * 4, [None] * 4, []
        for t in range(4):
            tb = self.tab[t]
            if tb is None:
                continue
            if tb.numel() * 4 >= BIG_TABLE_BYTES:
                (self.tab[t], self.gtab[t], self.mtab[t], self.vtab[t]), blk, _gap = _tuned_adam_block(ctx, tb, 4)
                self._tab_blocks.append(blk)
                del tb
            else:
                self.gtab[t], self.mtab[t], self.vtab[t] = z(tb), z(tb), z(tb)
        self.W = [_own(w, dev) for w in weights.get("W", [])]
        self.b = [_own(b, dev) for b in weights.get("b", [])]
        self.units = [w.shape[1] for w in self.W]
        self.gW, self.mW, self.vW = [z(w) for w in self.W], [z(w) for w in self.W], [z(w) for w in self.W]
        self.gb, self.mb, self.vb = [z(b) for b in self.b], [z(b) for b in self.b], [z(b) for b in self.b]
        self.hw, self.hb = _own(weights["hw"], dev), _own(weights.get("hb"), dev)
        self.ghw, self.mhw, self.vhw = z(self.hw), z(self.hw), z(self.hw)
        self.ghb, self.mhb, self.vhb = z(self.hb), z(self.hb), z(self.hb)
        B = int(max_batch)
        self._alloc_activations(B)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.step = 0
        p = lambda t: None if t is None else t.data_ptr()
        a4 = lambda ts: _lib._P4(*([p(t) for t in ts] + [None] * (4 - len(ts))))
        self._c = _lib.NmfState(
            U=self.U, I=self.I, Bmax=B, F=self.F, E=self.E, n_layers=len(self.units), use_mf=int(self.use_mf),
            use_mlp=int(self.use_mlp), head_bias=int(self.head_bias),
            units=(C.c_int32 * 4)(*(self.units + [0] * (4 - len(self.units)))),
            tab=a4(self.tab), gtab=a4(self.gtab), mtab=a4(self.mtab), vtab=a4(self.vtab),
            W=a4(self.W), b=a4(self.b), gW=a4(self.gW), gb=a4(self.gb), mW=a4(self.mW), vW=a4(self.vW),
            mb=a4(self.mb), vb=a4(self.vb),
            hw=p(self.hw), hb=p(self.hb), ghw=p(self.ghw), ghb=p(self.ghb), mhw=p(self.mhw), vhw=p(self.vhw),
            mhb=p(self.mhb), vhb=p(self.vhb), X0=p(self.X0), dX0=p(self.dX0), MF=p(self.MF), dlogit=p(self.dlogit),
            act=a4(self.act), dact=a4(self.dact), ws=self._ws.data_ptr(), ws_bytes=self._ws.numel(),
            dropout=self.dropout, drop_step=0, drop_seed=self.dropout_seed & 0xFFFFFFFFFFFFFFFF)
        self._drop_calls = 0
        self._c.hist_base = 1
        self._c.replay_series = int(replay == "series")
        self._alloc_step_ws()
        if self.deferred:
            self._alloc_deferred()

    def _alloc_step_ws(self):
        """el_nmf_state.step_ws: sort buffers of the batch's (row, sample) keys, the MF factor copies, partial rows of the reductions."""
        need = int(self.ctx.lib.el_nmf_step_ws_bytes(self.ctx.handle, C.byref(self._c)))
        if need <= 0:
            raise RuntimeError("el_nmf_step_ws_bytes failed: " + (_lib.load().el_last_error() or b"").decode())
        self._step_ws = torch.empty(need + 256, dtype=torch.uint8, device=self.ctx.device)
        base = (self._step_ws.data_ptr() + 255) // 256 * 256
        self._c.step_ws, self._c.step_ws_bytes = base, need
        self._c.pre_u = self._c.pre_i = None                        # (a batch ordered ahead into the old workspace is forgotten)
        self._c.pre_n, self._c.sort_set = 0, 0

    def _alloc_deferred(self):
        dev, c = self.ctx.device, self._c
        zi = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        self._row_last = [zi(self.U), zi(self.I)]
        if self.step:
            for t in self._row_last:
                t.fill_(self.step)                                    # switched on mid-run: every row is current
        self._lr_hist = torch.zeros(self._LR_HIST, dtype=torch.float32, device=dev)
        c.row_last = (C.c_void_p * 2)(*[t.data_ptr() for t in self._row_last])
        c.lr_hist, c.lr_hist_cap = self._lr_hist.data_ptr(), self._LR_HIST
        c.hist_base, c.claim_seq = self.step + 1, 0
        c.opt_step = c.flushed_step = self.step

    def sync(self):
        """Deferred decay: replay what is pending so that tab / mtab / vtab hold every row at the current step (no-op otherwise).
        Called by everything in this class that reads the tables; call it before reading the tensors directly."""
        if self.deferred:
            check(self.ctx.lib.el_nmf_sync_tables(self.ctx.handle, self.ctx.stream(), C.byref(self._c)), "el_nmf_sync_tables")

    def set_deferred(self, on):
        on = bool(on)
        if on == self.deferred:
            return
        if not on:
            self.sync()
            self.deferred = False
            c = self._c
            c.row_last = (C.c_void_p * 2)(None, None)
            c.lr_hist = None
            self._row_last = self._lr_hist = None
        else:
            self.deferred = True
            self._alloc_deferred()

    def _alloc_activations(self, B):
        """Activation / backward buffers for batches of up to B samples (+ the GEMM workspace sized for them)."""
        ctx, dev = self.ctx, self.ctx.device
        self.Bmax = B = int(B)
        zz = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.X0 = zz(B, 2 * self.E) if self.use_mlp else None
        self.dX0 = zz(B, 2 * self.E) if self.use_mlp else None
        self.MF = zz(B, self.F) if self.use_mf else None
        self.dlogit = zz(B)
        self.act = [zz(B, n) for n in self.units]
        self.dact = [zz(B, n) for n in self.units]
        dims = [2 * self.E] + self.units
        need = 16
        for l in range(len(self.units)):
            for mnk in ((B, dims[l + 1], dims[l]), (dims[l], dims[l + 1], B), (B, dims[l], dims[l + 1])):
                need = max(need, int(ctx.lib.el_gemm_ws_bytes(ctx.handle, *mnk)))
        # twice the products' need: the weight-gradient products of the backward pass then run on the library's second stream with the
        # upper half as their split-K workspace (el_neural.hip, nmf_grads)
        self._ws = torch.empty(2 * ((need + 255) // 256 * 256) + 256, dtype=torch.uint8, device=dev)

    def ensure_batch(self, n):
        """Grow the activation buffers to hold a batch of n samples: the reference takes ONE optimiser step per batch
        (neural_matrix_factorization_model.py:96-106), whatever its size.  Raises (torch's out-of-memory error) when HBM cannot
        hold the activations -- never splits the batch into several steps behind the caller's back."""
        if n <= self.Bmax:
            return
        self.X0 = self.dX0 = self.MF = self.dlogit = self._ws = self._step_ws = None
        self.act, self.dact = [], []
        torch.cuda.empty_cache()
        self._alloc_activations(n)
        p = lambda t: None if t is None else t.data_ptr()
        a4 = lambda ts: _lib._P4(*([p(t) for t in ts] + [None] * (4 - len(ts))))
        c = self._c
        c.Bmax, c.X0, c.dX0, c.MF, c.dlogit = self.Bmax, p(self.X0), p(self.dX0), p(self.MF), p(self.dlogit)
        c.act, c.dact, c.ws, c.ws_bytes = a4(self.act), a4(self.dact), self._ws.data_ptr(), self._ws.numel()
        self._alloc_step_ws()

    def _next_mask(self):
        self._drop_calls += 1                                        # a fresh dropout mask per gradient evaluation
        self._c.drop_step = self._drop_calls & 0x7FFFFFFF

    def weights(self):
        self.sync()
        out = {}
        for n, t in zip(["Umf", "Imf", "Umlp", "Imlp"], self.tab):
            if t is not None:
                out[n] = t.cpu().numpy()
        if self.use_mlp:
            out["W"] = [w.cpu().numpy() for w in self.W]
            out["b"] = [b.cpu().numpy() for b in self.b]
        out["hw"] = self.hw.cpu().numpy()
        if self.head_bias:
            out["hb"] = self.hb.cpu().numpy()
        return out

    def train_step(self, u, i, label, lr):
        n = u.numel()
        if n == 0:
            return                                                   # (the library takes no optimiser step on an empty batch either)
        self._margin = _PW_MARGIN
        self._next_mask()
        t = self.step + 1                                            # the counter moves only when the library has taken the step
        check(self.ctx.lib.el_nmf_train_step(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                             _ptr(i, torch.int32), _ptr(label, torch.float32), int(n), int(t),
                                             float(adam_lr_t(lr, t)), _ptr(self.loss, torch.float64)),
              "el_nmf_train_step")
        self.step = t

    def presort(self, u, i):
        """Order the batch's (embedding row, sample) keys ahead of its step, on the CURRENT stream (a side stream, while the previous
        step trains: el_nmf_presort); the train_step / grads call that follows with the same tensors skips its sort."""
        self.ensure_batch(u.numel())
        check(self.ctx.lib.el_nmf_presort(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32), _ptr(i, torch.int32),
                                          int(u.numel())), "el_nmf_presort")

    def grads(self, u, i, label, n_global=None):
        """Forward + loss + backward only (multi-GPU: the BCE mean runs over n_global samples); gradients stay in the
        state's buffers (replicated_grads() lists the ones a data-parallel caller has to all-reduce)."""
        n = u.numel()
        self._next_mask()
        if self.deferred and n_global is not None and int(n_global) != n:
            # a step shared with other ranks: the replicated tables take gradient rows of samples this rank never saw (all-reduce
            # of gtab), so which rows move is not known from the local batch -- back to the eager every-row passes
            self.set_deferred(False)
        self._batch_keep = (u, i)                                    # deferred decay: el_nmf_apply walks the batch's rows again
        check(self.ctx.lib.el_nmf_grads(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                        _ptr(i, torch.int32), _ptr(label, torch.float32), int(n),
                                        int(n if n_global is None else n_global), _ptr(self.loss, torch.float64)), "el_nmf_grads")

    def apply(self, lr):
        self._margin = _PW_MARGIN
        t = self.step + 1
        check(self.ctx.lib.el_nmf_apply(self.ctx.handle, self.ctx.stream(), C.byref(self._c), int(t),
                                        float(adam_lr_t(lr, t))), "el_nmf_apply")
        self.step = t

    def replicated_grads(self, shard="user"):
        """Gradient tensors of the variables every rank holds a full copy of: Dense layers, head, and the embedding tables
        that are NOT sharded -- the item tables with user shards (shard="user"), the user tables with item shards."""
        keep = (1, 3) if shard == "user" else (0, 2)
        out = [self.gtab[t] for t in keep if self.gtab[t] is not None]
        out += list(self.gW) + list(self.gb) + [self.ghw]
        if self.head_bias:
            out.append(self.ghb)
        return out

    def forward(self, u, i, out=None):
        n = u.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=self.ctx.device)
        check(self.ctx.lib.el_nmf_forward(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                          _ptr(i, torch.int32), int(n), _ptr(out, torch.float32)), "el_nmf_forward")
        return out

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v

    # -- full-catalogue scoring -> masked top-k --------------------------------------------------------------------
    def fused_supported(self, k):
        """True when el_nmf_score_topk takes this network and list length (three Dense layers, units <= (1024, 256, 128), ...)."""
        return bool(self.use_mlp and self.ctx.lib.el_nmf_score_supported(C.byref(self._c), int(k)))

    def score_topk_logits(self, u_start, u_stop, k, excl=None, cand=None, item_offset=0, I_local=None, items_unchanged=False, screen=None):
        """el_nmf_score_topk: the k best unmasked items of users [u_start, u_stop) by (logit desc, item asc) and their logits --
        layer 1 in its separable form, layers 2-3 and the head per (user, item) pair on fp32 MFMA tiles, selection fused.
        screen (full-catalogue calls only): layers 2-3 first on the half-precision matrix instruction with a per-pair error bound, the
        fp32 kernel on the surviving pairs -- the same lists and logit bits (EL_NMF_SCREEN in the header).  True / False force it;
        None (default) screens, and when a call had to take the unscreened
        route (the bound depends on the weights: el_nmf_screen_stats) leaves the next 15 calls unscreened before it tries again."""
        n = int(u_stop) - int(u_start)
        I_local = self.I - int(item_offset) if I_local is None else int(I_local)
        auto = screen is None
        if auto:
            screen = True
        screen = bool(screen) and cand is None
        use = screen
        if auto and screen and getattr(self, "_screen_skip", 0) > 0:
            self._screen_skip -= 1
            use = False
        need = int(self.ctx.lib.el_nmf_score_ws_bytes(self.ctx.handle, C.byref(self._c), n, I_local, int(k),
                                                      1 if cand is not None else (2 if screen else 0)))   # (auto: room for the screen
        #                                                                                   on every call, one workspace for the evaluation)
        if need == 0:
            raise _lib.ElliotHipError("el_nmf_score_topk does not take this network shape / k (NmfDeviceState.fused_supported)")
        held = getattr(self, "_score_ws", None)
        ws = workspace(self, "_score_ws", need, self.ctx.device)
        if ws is not held:
            items_unchanged = False
        out_idx = torch.empty((n, k), dtype=torch.int32, device=self.ctx.device)
        out_val = torch.empty((n, k), dtype=torch.float32, device=self.ctx.device)
        ep, ei = _csr_ptrs(excl)
        cp, ci = _csr_ptrs(cand)
        check(self.ctx.lib.el_nmf_score_topk(self.ctx.handle, self.ctx.stream(), C.byref(self._c), int(u_start), int(u_stop),
                                             int(item_offset), I_local, ep, ei, cp, ci, int(k), _ptr(out_idx), _ptr(out_val),
                                             (_lib.EL_TOPK_ITEMS_UNCHANGED if items_unchanged else 0) | (_lib.EL_NMF_SCREEN if use else 0),
                                             C.c_void_p(ws.data_ptr()), ws.numel()), "el_nmf_score_topk")
        if auto and use and self.screen_stats()[1]:
            self._screen_skip = 15
        return out_idx, out_val

    def screen_stats(self):
        """(pairs the exact fp32 kernel scored, a call that asked for the screen went without it) of the last score_topk_logits call."""
        pairs, fb = C.c_int64(0), C.c_int(0)
        self.ctx.lib.el_nmf_screen_stats(self.ctx.handle, C.byref(pairs), C.byref(fb))
        return int(pairs.value), bool(fb.value)

    def _dot_tables(self, items_unchanged):
        """The MF-only network (GMF; NeuMF with is_mlp_train False) is sigmoid(<Umf[u], Imf[i] * h> (+ b)): tables for the fused
        dot-product top-k kernels -- the item image Imf * h (el_gmf_item_image) and a constant bias row for the Dense(1) bias."""
        self.sync()
        img = getattr(self, "_gmf_image", None)
        if img is None or not items_unchanged:
            if img is None:
                img = self._gmf_image = (torch.empty_like(self.tab[1]),
                                         torch.empty(self.I, dtype=torch.float32, device=self.ctx.device) if self.head_bias else None)
            check(self.ctx.lib.el_gmf_item_image(self.ctx.handle, self.ctx.stream(), _ptr(self.tab[1], torch.float32),
                                                 _ptr(self.hw, torch.float32), int(self.I), int(self.F), _ptr(img[0], torch.float32)),
                  "el_gmf_item_image")
            if self.head_bias:
                img[1].copy_(self.hb.expand(self.I))
        return img

    def _pairs_topk(self, u_start, u_stop, k, excl, cand):
        """The reference's own route (index grids -> get_recs -> get_top_k, neural_matrix_factorization.py:111-119) for networks
        the fused kernel does not take: probabilities of every (user, item) pair in blocks of Bmax pairs, dense top-k."""
        nu, dev = int(u_stop) - int(u_start), self.ctx.device
        items = torch.arange(self.I, dtype=torch.int32, device=dev)
        preds = torch.empty((nu, self.I), dtype=torch.float32, device=dev)
        per = max(1, self.Bmax // self.I)
        for s in range(0, nu, per):
            e = min(s + per, nu)
            ug = torch.arange(u_start + s, u_start + e, dtype=torch.int32, device=dev).repeat_interleave(self.I)
            self.forward(ug, items.repeat(e - s), out=preds[s:e].reshape(-1))
        return dense_topk(self.ctx, preds, u_start, u_stop, k, excl=excl, cand=cand)

    def recommend(self, u_start, u_stop, k, excl=None, cand=None, items_unchanged=False):
        """get_recs + get_top_k of NeuMF / GMF for users [u_start, u_stop): (idx int32 [n, k], probabilities fp32 [n, k]).
        The fused kernels rank by the logit; sigmoid is monotone, so the ranking by probability can differ only where distinct
        logits round to one probability (tf.nn.top_k orders those by item index): the list is taken a few entries longer, linked
        (el_pwmf_link_values), re-ranked by (value desc, index asc) and cut -- the rule of PwmfDeviceState.recommend."""
        if self.use_mlp and not self.fused_supported(min(self.I, k + _PW_MARGIN)):
            return self._pairs_topk(u_start, u_stop, k, excl, cand)
        max_list = _NMF_MAX_LIST if self.use_mlp else _PW_MAX_LIST

        def score(kk):
            nonlocal items_unchanged
            same, items_unchanged = items_unchanged, True          # a longer list of this call meets the image of its first pass
            if self.use_mlp:
                return self.score_topk_logits(u_start, u_stop, kk, excl=excl, cand=cand, items_unchanged=same)
            img, brow = self._dot_tables(same)
            return score_topk(self.ctx, self.tab[0], img, brow, u_start, u_stop, kk, excl=excl, cand=cand, items_unchanged=same)

        def link(val, kk):
            check(self.ctx.lib.el_pwmf_link_values(self.ctx.handle, self.ctx.stream(), _ptr(val, torch.float32), int(val.shape[0]),
                                                   int(val.stride(0)), int(kk), _lib.EL_PW_MSE_SIGMOID, None, int(u_start)),
                  "el_pwmf_link_values")

        return _linked_topk(self, k, score, link, max_list, lambda: self._pairs_topk(u_start, u_stop, k, excl, cand))


# ------------------------------------------------------------------------------------------
# point-wise factor models: MF, PMF, FunkSVD, LogisticMF
# ------------------------------------------------------------------------------------------
PW_KINDS = {"mse": _lib.EL_PW_MSE, "mse_sigmoid": _lib.EL_PW_MSE_SIGMOID, "logistic": _lib.EL_PW_LOGISTIC}
PW_OPTS = {"adam": _lib.EL_PW_ADAM, "adagrad": _lib.EL_PW_ADAGRAD}
PW_SIDES = {"both": _lib.EL_PW_BOTH, "items": _lib.EL_PW_ITEMS, "users": _lib.EL_PW_USERS}
# entries beyond k taken before the link: two keep k' = k + 2 <= 12 on the fastest screening policy for the usual k = 10; a row
# whose ranks k .. k' all collapse to one linked float (probability ~1e-8 per row) is redone with a 4x longer list
_PW_MARGIN, _PW_MAX_LIST, _PW_DENSE_ROWS = 2, 4032, 4096
_NMF_MAX_LIST = 448          # el_nmf_score_topk keeps k <= 448 candidates per wave in LDS
_CML_MARGIN = 16             # CML re-scores with another formula: its fp32 rounding may reorder near-ties a few ranks deep


def topk_rerank(ctx, idx, val):
    """Rows of (idx, val) re-ordered in place by (value desc, index asc) -- tf.nn.top_k's order -- after the values were
    transformed (link, CML re-score): el_topk_rerank, lists of up to 4096 entries.  Returns (idx, val)."""
    kk = idx.shape[1]
    if kk > 4096:
        raise ValueError("topk_rerank: lists of more than 4096 entries are not produced by any caller")
    check(ctx.lib.el_topk_rerank(ctx.handle, ctx.stream(), _ptr(idx, torch.int32), _ptr(val, torch.float32), int(idx.shape[0]),
                                 int(idx.stride(0)), int(kk)), "el_topk_rerank")
    return idx, val


def _linked_topk(state, k, score, link, max_list, dense):
    """Top-k by a linked score from kernels that rank by the raw one.  score(kk) -> (idx, val) lists of length kk by raw score;
    link(val, kk) maps the values in place; the list is taken `state._margin` entries longer than k, linked, and while some row's
    k-th value still equals its last one taken longer (k + 16, then x4) up to `max_list`, past which dense() answers; then re-ranked
    by (value desc, index asc) and cut.  The length that resolved this block stays in state._margin: small-score models (untrained:
    everything near link(0)) collapse often, and the next blocks of the evaluation start there (the training calls reset it)."""
    kk = min(state.I, k + getattr(state, "_margin", _PW_MARGIN))
    while True:
        idx, val = score(kk)
        link(val, kk)
        if kk >= state.I:
            break
        open_rows = (val[:, k - 1] == val[:, kk - 1]) & (val[:, k - 1] > float("-inf"))
        if not bool(open_rows.any()):
            break
        if kk >= max_list:
            return dense()
        kk = min(state.I, max_list, k + 16 if kk < k + 16 else kk * 4)
    state._margin = kk - k
    idx, val = topk_rerank(state.ctx, idx, val)
    return idx[:, :k].contiguous(), val[:, :k].contiguous()


class PwmfDeviceState:
    """Variables + optimiser slots of one point-wise factor model in HBM (include/elliot_hip.h, el_pwmf_state).

    Gu [U,F], Gi [I,F], optional biases Bu [U] / Bi [I] (both or neither); kind: "mse" (MF, FunkSVD), "mse_sigmoid"
    (PMF), "logistic" (LogisticMF, with alpha / l_w); optimizer "adam" (TF sparse-apply semantics) or "adagrad"."""

    def __init__(self, ctx, Gu, Gi, Bu=None, Bi=None, kind="mse", optimizer="adam", alpha=0.0, l_w=0.0):
        self.ctx, dev = ctx, ctx.device
        if (Bu is None) != (Bi is None):
            raise ValueError("Bu and Bi go together")
        self.Gu, self.Gi, self.Bu, self.Bi = (_own(x, dev) for x in (Gu, Gi, Bu, Bi))
        if self.Bu is not None:
            self.Bu, self.Bi = self.Bu.reshape(-1).contiguous(), self.Bi.reshape(-1).contiguous()
        self.U, self.F = self.Gu.shape
        self.I = self.Gi.shape[0]
        self.kind, self.optimizer = kind, optimizer
        self.alpha, self.l_w = float(alpha), float(l_w)
        adam = optimizer == "adam"
        z = lambda t: None if t is None else torch.zeros_like(t)
        slot = (lambda t: z(t)) if adam else (lambda t: None if t is None else torch.full_like(t, 0.1))
        names = ("Gu", "Gi", "Bu", "Bi")
        for n in names:
            t = getattr(self, n)
            if n == "Gu" and adam and self.U * self.F * 4 >= BIG_TABLE_BYTES:
                (self.Gu, self.gGu, self.mGu, self.vGu), self._user_block, _gap = _tuned_adam_block(ctx, self.Gu, 4)
                continue
            setattr(self, "g" + n, z(t))
            setattr(self, "m" + n, slot(t))
            setattr(self, "v" + n, z(t) if adam else None)
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self.step = 0
        p = lambda t: None if t is None else t.data_ptr()
        self._c = _lib.PwmfState(U=self.U, I=self.I, F=self.F, kind=PW_KINDS[kind], alpha=self.alpha, l_w=self.l_w,
                                 **{pre + n: p(getattr(self, pre + n)) for pre in ("", "g", "m", "v") for n in names})

    def _step_ws(self, n):
        need = int(self.ctx.lib.el_pwmf_ws_bytes(int(n), int(self.U), int(self.I), int(self.F)))
        return _ptr(workspace(self, "_ws", need, self.ctx.device)), need

    def train_step(self, u, i, label, lr, side="both"):
        self.step += 1
        self._margin = _PW_MARGIN
        n = u.numel()
        ws, need = self._step_ws(n)
        lr_t = adam_lr_t(lr, self.step) if self.optimizer == "adam" else float(lr)
        check(self.ctx.lib.el_pwmf_train_step(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                              _ptr(i, torch.int32), _ptr(label, torch.float32), int(n),
                                              PW_OPTS[self.optimizer], PW_SIDES[side], int(self.step), float(lr_t),
                                              _ptr(self.loss, torch.float64), ws, need), "el_pwmf_train_step")

    def train_loop(self, pos, events, B, seed, first_sample, lr, side="both"):
        """One sampler pass of an epoch -- `for batch in sampler.step(events, B): train_step(batch)` -- from a single library
        call (el_pwmf_train_loop): the same Philox stream and kernels as the per-batch calls, no host work in between."""
        steps = (int(events) + int(B) - 1) // int(B)
        if steps == 0:
            return 0
        if pos.n_rows != self.U or pos.n_cols != self.I:
            raise ValueError("train_loop: the positives' CSR must describe this state's users x items")
        adam = self.optimizer == "adam"
        lr_t = np.array([adam_lr_t(lr, self.step + 1 + k) if adam else lr for k in range(steps)], dtype=np.float32)
        ws, need = self._step_ws(min(int(B), int(events)) if events < B else int(B))
        lneed = int(self.ctx.lib.el_pwmf_train_loop_ws_bytes(int(events), int(B)))
        buf = workspace(self, "_loop_ws", lneed, self.ctx.device)
        self._margin = _PW_MARGIN
        check(self.ctx.lib.el_pwmf_train_loop(
            self.ctx.handle, self.ctx.stream(), C.byref(self._c), *_csr_ptrs(pos), C.c_void_p(sampler_meta(self.ctx, pos).data_ptr()),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sample), int(events), int(B), PW_OPTS[self.optimizer], PW_SIDES[side],
            int(self.step + 1), lr_t.ctypes.data_as(C.c_void_p), _ptr(self.loss, torch.float64), ws, need,
            C.c_void_p(buf.data_ptr()), lneed), "el_pwmf_train_loop")
        self.step += steps
        return steps

    def grads(self, u, i, label, n_global=None, side="both"):
        """Forward + loss + gradient sums only (multi-GPU: a batch-mean loss runs over n_global samples); the accumulators of
        `side` are complete on return -- item_grads() lists the replicated ones a data-parallel caller all-reduces."""
        n = u.numel()
        ws, need = self._step_ws(n)
        check(self.ctx.lib.el_pwmf_grads(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                         _ptr(i, torch.int32), _ptr(label, torch.float32), int(n),
                                         int(n if n_global is None else n_global), PW_SIDES[side], _ptr(self.loss, torch.float64),
                                         ws, need), "el_pwmf_grads")

    def apply(self, lr, side="both", advance=True):
        if advance:
            self.step += 1
            self._margin = _PW_MARGIN
        lr_t = adam_lr_t(lr, self.step) if self.optimizer == "adam" else float(lr)
        check(self.ctx.lib.el_pwmf_apply(self.ctx.handle, self.ctx.stream(), C.byref(self._c), PW_OPTS[self.optimizer],
                                         PW_SIDES[side], int(self.step), float(lr_t)), "el_pwmf_apply")

    def item_grads(self):
        return [t for t in (self.gGi, self.gBi) if t is not None]

    def forward(self, u, i, out=None):
        n = u.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=self.ctx.device)
        check(self.ctx.lib.el_pwmf_forward(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                           _ptr(i, torch.int32), int(n), _ptr(out, torch.float32)), "el_pwmf_forward")
        return out

    def pop_loss(self):
        v = float(self.loss.item())
        self.loss.zero_()
        return v

    def weights(self):
        out = {"Gu": self.Gu.cpu().numpy(), "Gi": self.Gi.cpu().numpy(), "step": self.step}
        if self.Bu is not None:
            out["Bu"], out["Bi"] = self.Bu.cpu().numpy(), self.Bi.cpu().numpy()
        for pre in ("m", "v"):
            for n in ("Gu", "Gi", "Bu", "Bi"):
                t = getattr(self, pre + n)
                if t is not None:
                    out[pre + n] = t.cpu().numpy()
        return out

    def load(self, d):
        for key, val in d.items():
            if key == "step":
                self.step = int(val)
            elif getattr(self, key, None) is not None:
                getattr(self, key).copy_(torch.from_numpy(np.asarray(val, dtype=np.float32)).reshape(getattr(self, key).shape))

    # -- full-catalogue scores -> masked top-k ------------------------------------------------------------------
    def _link(self, vals, k, u_start):
        check(self.ctx.lib.el_pwmf_link_values(self.ctx.handle, self.ctx.stream(), _ptr(vals, torch.float32),
                                               int(vals.shape[0]), int(vals.stride(0)), int(k), PW_KINDS[self.kind],
                                               _ptr(self.Bu, torch.float32), int(u_start)), "el_pwmf_link_values")

    def recommend(self, u_start, u_stop, k, excl=None, cand=None):
        """get_recs + get_top_k of the reference models (e.g. matrix_factorization.py:99-113 +
        matrix_factorization_model.py:100-101) for users [u_start, u_stop): the fused scoring kernel ranks by
        Bi[i] + <Gu[u], Gi[i]>; the model's score is link(that + Bu[u]) with a monotone link, so the ranking is the same
        except where distinct raw scores round to ONE linked float -- tf.nn.top_k orders those by item index.  The list is
        therefore taken `margin` entries longer, linked, re-ranked by (value desc, index asc) and cut; a row whose k-th
        value still equals its last one is redone with a longer list (and, past 4032 entries, from dense scores)."""
        plain = self.kind != "mse_sigmoid" and self.Bu is None
        if plain:
            return score_topk(self.ctx, self.Gu, self.Gi, None, u_start, u_stop, k, excl=excl, cand=cand)
        return _linked_topk(self, k, lambda kk: score_topk(self.ctx, self.Gu, self.Gi, self.Bi, u_start, u_stop, kk, excl=excl, cand=cand),
                            lambda val, kk: self._link(val, kk, u_start), _PW_MAX_LIST,
                            lambda: self._recommend_dense(u_start, u_stop, k, excl, cand))

    def _recommend_dense(self, u_start, u_stop, k, excl, cand):
        out_i, out_v = [], []
        for s in range(u_start, u_stop, _PW_DENSE_ROWS):
            e = min(s + _PW_DENSE_ROWS, u_stop)
            preds = gemm(self.ctx, self.Gu[s:e], self.Gi, transB=True, bias=self.Bi)
            self._link(preds, self.I, s)
            bi, bv = dense_topk(self.ctx, preds, s, e, k, excl=excl, cand=cand)
            out_i.append(bi)
            out_v.append(bv)
        return torch.cat(out_i), torch.cat(out_v)


# ------------------------------------------------------------------------------------------
# Collaborative Metric Learning
# ------------------------------------------------------------------------------------------
class CmlDeviceState(BprmfDeviceState):
    """CML_model's variables (Gu, Gi, Bi) + Adam slots: the BPR state with the metric-learning step and scoring."""

    def __init__(self, ctx, Gu, Gi, Bi):
        super().__init__(ctx, Gu, Gi, Bi, optimizer="adam_tf_dense", compact_user_grads=False)
        self._items2 = None

    def train_step(self, u, i, j, lr, l_w, l_b, margin):
        self.step += 1
        B = u.numel()
        ws, need = self._cml_ws_for(B, B)
        check(self.ctx.lib.el_cml_train_step(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                             _ptr(i, torch.int32), _ptr(j, torch.int32), int(B), float(l_w), float(l_b),
                                             float(margin), int(self.step), float(adam_lr_t(lr, self.step)),
                                             _ptr(self.loss, torch.float64), ws, need),
              "el_cml_train_step")
        self._items2 = None

    def _cml_ws_for(self, B, B_all):
        need = int(self.ctx.lib.el_cml_ws_bytes(int(B), int(B_all), int(self.U), int(self.I), int(self.F)))
        return _ptr(workspace(self, "_cml_ws", need, self.ctx.device)), need

    def forward_de(self, u, i, j, l_w, l_b):
        """Phase 1 of the multi-GPU step: the rank's D_a, E_a (device float [B] each) + its share of the regulariser."""
        B = u.numel()
        D = torch.empty(B, dtype=torch.float32, device=self.ctx.device)
        E = torch.empty(B, dtype=torch.float32, device=self.ctx.device)
        check(self.ctx.lib.el_cml_forward(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                          _ptr(i, torch.int32), _ptr(j, torch.int32), int(B), float(l_w), float(l_b), _ptr(D), _ptr(E),
                                          _ptr(self.loss, torch.float64)), "el_cml_forward")
        return D, E

    def grads_de(self, u, i, j, l_w, l_b, margin, D, E, D_all, E_all):
        """Phase 2: the rank's triplets against the gathered D / E of the global batch; gradients stay in the accumulators."""
        B, B_all = u.numel(), D_all.numel()
        ws, need = self._cml_ws_for(B, B_all)
        check(self.ctx.lib.el_cml_grads(self.ctx.handle, self.ctx.stream(), C.byref(self._c), _ptr(u, torch.int32),
                                        _ptr(i, torch.int32), _ptr(j, torch.int32), int(B), float(l_w), float(l_b), float(margin),
                                        _ptr(D, torch.float32), _ptr(E, torch.float32), _ptr(D_all, torch.float32),
                                        _ptr(E_all, torch.float32), int(B_all), _ptr(self.loss, torch.float64),
                                        ws, need), "el_cml_grads")
        self._items2 = None

    # -- optimiser alone (multi-GPU step): the split form overlaps the item-gradient all-reduce with the user rows' update
    def item_grads(self):
        return [self.item_grad_flat]

    def begin_step(self):
        self.step += 1

    def _apply(self, c_state, lr):
        check(self.ctx.lib.el_bprmf_apply(self.ctx.handle, self.ctx.stream(), C.byref(c_state), float(lr), int(self.opt), int(self.step),
                                          float(adam_lr_t(lr, self.step))), "el_bprmf_apply")
        self._items2 = None

    def apply_users(self, lr):
        if not hasattr(self, "_c_users"):
            clone = lambda c: type(c).from_buffer_copy(c)
            self._c_users, self._c_items = clone(self._c), clone(self._c)
            self._c_users.I = 0
            self._c_items.U = 0
        self._apply(self._c_users, lr)

    def apply_items(self, lr):
        self._apply(self._c_items, lr)

    def _item_side(self):
        if self._items2 is None:
            Gi2, Bi2 = torch.empty_like(self.Gi), torch.empty_like(self.Bi)
            check(self.ctx.lib.el_cml_prepare_items(self.ctx.handle, self.ctx.stream(), _ptr(self.Gi, torch.float32),
                                                    _ptr(self.Bi, torch.float32), int(self.I), int(self.F), _ptr(Gi2), _ptr(Bi2)),
                  "el_cml_prepare_items")
            self._items2 = (Gi2, Bi2)
        return self._items2

    def rescore(self, idx, u_start):
        val = torch.empty(idx.shape, dtype=torch.float32, device=self.ctx.device)
        check(self.ctx.lib.el_cml_rescore(self.ctx.handle, self.ctx.stream(), _ptr(self.Gu, torch.float32),
                                          _ptr(self.Gi, torch.float32), _ptr(self.Bi, torch.float32), int(self.F),
                                          _ptr(idx, torch.int32), int(idx.shape[0]), int(idx.stride(0)), int(idx.shape[1]),
                                          int(u_start), _ptr(val)), "el_cml_rescore")
        return val

    def recommend(self, u_start, u_stop, k, excl=None, cand=None):
        """CML_model.predict + get_top_k (CML_model.py:97-106): the fused kernel ranks by (Bi - |Gi|^2) + <Gu, 2 Gi>, which is
        the score plus the per-user constant |Gu[u]|^2; the k + 16 best are re-scored with the reference's own formula
        -sum (u - i)^2 + b_i and re-ranked by (value desc, index asc), so values and order are those of the direct
        evaluation (the two formulas differ by fp32 rounding only; a difference that straddles rank k + 16 is not seen)."""
        Gi2, Bi2 = self._item_side()
        kk = min(self.I, k + _CML_MARGIN)
        idx, raw = score_topk(self.ctx, self.Gu, Gi2, Bi2, u_start, u_stop, kk, excl=excl, cand=cand)
        val = self.rescore(idx, u_start)
        val = torch.where(raw == float("-inf"), raw, val)           # -inf padding (masked items) stays padding
        idx, val = topk_rerank(self.ctx, idx, val)
        return idx[:, :k].contiguous(), val[:, :k].contiguous()
