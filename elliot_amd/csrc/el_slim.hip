// SLIM (Ning & Karypis 2011; the ElasticNet form of Levy & Jack 2013): one non-negative elastic-net regression per item.
//
// Replaces SlimModel.train of the reference (slim_model.py:44-110: one sklearn ElasticNet.fit per item); the scores and lists
// are el_knn_score_topk(A = R, B = W):
//   el_slim_order  the xorshift32 visiting order of sklearn's selection='random', once per model
//   el_slim_fit    sklearn's sparse_enet_coordinate_descent (positive, no intercept) for a block of target columns, fused
//                  with the cut of every column; nothing I x I or U x I is written (except the optional test output)
//   el_slim_w      the column lists of all targets -> W as CSR with ascending columns
//
// Numerics contract (tests/helpers/slim_ref.py restates it in NumPy):
//   norm[c]  float32 sum of x * x over column c, sequentially in stored order
//   step c   r += w[c] X[:, c] (if w[c] != 0), every product and sum rounded to float32, no contraction;
//            tmp = (float)(X[:, c] . r): the products are exact in fp64, every lane adds its entries (stride 64) in fp64, the 64
//            partial sums are added by a butterfly -- a fixed order, and closer to the exact dot than sklearn's sequential
//            float32 sum; w[c] = tmp < 0 ? 0 : (float)(max((double)tmp - l1, 0) / (double)(float)(norm[c] + l2)): the
//            subtraction and the division in double, rounded once (the .pyx promotes through libc's fabs);
//            r -= w[c] X[:, c] (if w[c] != 0)
//   stop     after a sweep with w_max == 0 or d_w_max / w_max < tol (float32) or the last one: the duality gap of the
//            `positive` branch with X^T r, r . r, w . w, |w|_1, r . y and the gap itself in fp64; gap < (float)(tol * y . y)
//   y == 0   w = 0 at once, n_iter = max_iter (sklearn runs every sweep: its test is 0 < 0)
//   cut      of the weights != 0 the min(nnz - 1, N) largest by (value desc, index asc)
// Mapping: ONE WAVE PER TARGET.  A target is a strictly sequential chain of coordinate steps; a step is a gather-dot and at most
// two scatter-updates of one sparse column against the dense residual, so the lanes share the column's entries.  The residual
// and the weights of the target live in LDS (4 (U + I) bytes) while that fits in a workgroup's 160 KiB, so a CU holds several
// targets; beyond that in a slice of the workspace (the L2 serves it).  Every wave walks the same order, so the CSC streams
// through the caches once per front of waves; the order is known in advance, so the loads run three draws ahead of the
// step (order, column bounds and norm, the first 256 entries) and no step waits for a chain of dependent loads.
// Deterministic: the same input gives the same bytes.  No float atomics.
#include "el_common.h"

#include "el_knn_csr.h"
#include "el_topk_common.h"

#define SLIM_MAX_NEIGHBORS 2048                   // as KNN_MAX_NEIGHBORS: the cut's selection buffer lives in LDS
#define SLIM_LDS_BYTES (160 * 1024)               // what one workgroup may declare on gfx950
#define SLIM_REG 4                                // 64-entry pieces of a column a wave holds in registers through a step

namespace {

__global__ __launch_bounds__(64) void k_slim_order(u32 state, u32 I, int64_t n, int32_t* __restrict__ order) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    u32 s = state;
    for (int64_t t = 0; t < n; ++t) {
        if (s == 0u) s = 1u;
        s ^= s << 13;
        s ^= s >> 17;
        s ^= s << 5;
        order[t] = (int32_t)((s & 0x7fffffffu) % I);
    }
}

// norm[c] of the whole matrix (exclusion = column: the target's own column is skipped by its index)
__global__ __launch_bounds__(256) void k_slim_norm(const int64_t* __restrict__ cp, const float* __restrict__ cv, int64_t I,
                                                   float* __restrict__ norm) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= I) return;
    float s = 0.f;
    for (int64_t e = cp[c]; e < cp[c + 1]; ++e) s = __fadd_rn(s, __fmul_rn(cv[e], cv[e]));
    norm[c] = s;
}

struct SlimFit {
    const int64_t* cp;     // CSC of R: column -> its rows ascending
    const int32_t* ci;
    const float* cv;
    const int32_t* order;  // [max_iter * I]
    const float* norm;     // [I] (column) or per target [n, I] (reference)
    float* gr;             // global placement: residuals [n, U]
    float* gw;             // ... and weights [n, I]
    int64_t U, I, j_start;
    float l1, l2, tol;
    int max_iter, reference;
    int N, cap;            // list width, selection slots (power of two >= N + 64)
    int w_bytes;           // LDS placement: bytes of the weights in front of the residual
    int32_t* lx;
    float* lv;
    int32_t* lcnt;
    int32_t* n_iter;
    float* coef;           // [n, I] or null
};

// Orders one wave's accesses to its own residual / weights: other lanes read what a lane wrote.  LDS: serviced in program order.
// Global: the stores are acknowledged (vmcnt(0)) before a later load is issued; the wave's CU has one vector L1, written through.
template <bool LDS>
__device__ __forceinline__ void slim_sync() {
    if (LDS) {
        el_wave_lds_sync();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

__device__ __forceinline__ double slim_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));      // commutative pairs: the same bits in every lane
    return v;
}

__device__ __forceinline__ double slim_wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

template <bool LDS, bool REF>
__global__ __launch_bounds__(64) void k_slim_fit(SlimFit p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int32_t j = (int32_t)(p.j_start + t);
    const int64_t U = p.U, I = p.I;
    float* w;
    float* r;
    u64* keys;
    if (LDS) {
        w = reinterpret_cast<float*>(smem);
        r = reinterpret_cast<float*>(smem + p.w_bytes);
        keys = reinterpret_cast<u64*>(smem + p.w_bytes);       // the cut reuses the residual's bytes
    } else {
        w = p.gw + t * I;
        r = p.gr + t * U;
        keys = reinterpret_cast<u64*>(smem);
    }
    const int64_t* __restrict__ cp = p.cp;
    const int32_t* __restrict__ ci = p.ci;
    const float* __restrict__ cv = p.cv;
    const int32_t* __restrict__ order = p.order;
    const float* __restrict__ norm = REF ? p.norm + t * I : p.norm;

    for (int64_t i = lane; i < I; i += 64) w[i] = 0.f;
    for (int64_t i = lane; i < U; i += 64) r[i] = 0.f;
    slim_sync<LDS>();
    const int64_t y0 = cp[j], y1 = cp[j + 1];
    double yy = 0.0;
    for (int64_t e = y0 + lane; e < y1; e += 64) {
        const float v = cv[e];
        r[ci[e]] = v;
        yy += (double)v * (double)v;
    }
    yy = slim_wave_sum(yy);
    slim_sync<LDS>();

    int sweeps = p.max_iter;
    if (yy != 0.0) {
        const float tol_abs = __fmul_rn(p.tol, (float)yy);
        const double l1 = (double)p.l1, l2 = (double)p.l2;
        const int64_t total = (int64_t)p.max_iter * I;
        // Three loads deep, one level per step, so that no step waits for a chain of dependent loads: the coordinate three
        // draws ahead (order), the column bounds and norm of the one two ahead, and the lane's entries of the first
        // SLIM_REG * 64 of the next one, which stay in registers from the dot to the second update.
        const int64_t last = total - 1;
        int32_t c1 = order[0], c2 = order[1 < last ? 1 : last], c3 = order[2 < last ? 2 : last];
        int64_t b1 = cp[c1], f1 = cp[c1 + 1], b2 = cp[c2], f2 = cp[c2 + 1];
        float n1 = norm[c1], n2 = norm[c2];
        int32_t ni[SLIM_REG];
        float nx[SLIM_REG];
#pragma unroll
        for (int k = 0; k < SLIM_REG; ++k) {
            ni[k] = 0, nx[k] = 0.f;
            if (b1 + 64 * k + lane < f1) ni[k] = ci[b1 + 64 * k + lane], nx[k] = cv[b1 + 64 * k + lane];
        }
        int64_t draw = 0;
        for (int it = 0; it < p.max_iter; ++it) {
            float w_max = 0.f, d_w_max = 0.f;
            for (int64_t f = 0; f < I; ++f) {
                const int32_t c = c1;
                const int64_t e0 = b1, e1 = f1;
                const float nrm = n1;
                int32_t xi[SLIM_REG];
                float xv[SLIM_REG];
#pragma unroll
                for (int k = 0; k < SLIM_REG; ++k) xi[k] = ni[k], xv[k] = nx[k];
                ++draw;
                c1 = c2, b1 = b2, f1 = f2, n1 = n2;
#pragma unroll
                for (int k = 0; k < SLIM_REG; ++k)
                    if (b1 + 64 * k + lane < f1) ni[k] = ci[b1 + 64 * k + lane], nx[k] = cv[b1 + 64 * k + lane];
                c2 = c3, b2 = cp[c2], f2 = cp[c2 + 1], n2 = norm[c2];
                c3 = order[draw + 2 < last ? draw + 2 : last];
                if (nrm == 0.f || (!REF && c == j)) continue;
                const float wc = w[c];
                bool act[SLIM_REG];
                float rk[SLIM_REG];
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < SLIM_REG; ++k) {
                    act[k] = e0 + 64 * k + lane < e1 && !(REF && xi[k] == j);
                    rk[k] = 0.f;
                    if (act[k]) rk[k] = r[xi[k]];
                }
#pragma unroll
                for (int k = 0; k < SLIM_REG; ++k) {
                    if (act[k]) {
                        if (wc != 0.f) rk[k] = __fadd_rn(rk[k], __fmul_rn(xv[k], wc));
                        acc += (double)rk[k] * (double)xv[k];
                    }
                }
                for (int64_t e = e0 + 64 * SLIM_REG + lane; e < e1; e += 64) {
                    const int32_t idx = ci[e];
                    const float x = cv[e];
                    if (REF && idx == j) continue;
                    float rv = r[idx];
                    if (wc != 0.f) {
                        rv = __fadd_rn(rv, __fmul_rn(x, wc));
                        r[idx] = rv;
                    }
                    acc += (double)rv * (double)x;
                }
                const float tmp = (float)slim_wave_sum(acc);
                float wn = 0.f;
                if (!(tmp < 0.f)) wn = (float)__ddiv_rn(fmax((double)tmp - l1, 0.0), (double)__fadd_rn(nrm, p.l2));
                if (wn != 0.f || wc != 0.f) {
#pragma unroll
                    for (int k = 0; k < SLIM_REG; ++k)
                        if (act[k]) r[xi[k]] = wn != 0.f ? __fsub_rn(rk[k], __fmul_rn(xv[k], wn)) : rk[k];
                }
                if (wn != 0.f) {
                    for (int64_t e = e0 + 64 * SLIM_REG + lane; e < e1; e += 64) {
                        const int32_t idx = ci[e];
                        if (REF && idx == j) continue;
                        r[idx] = __fsub_rn(r[idx], __fmul_rn(cv[e], wn));
                    }
                }
                if (lane == 0) w[c] = wn;
                d_w_max = fmaxf(d_w_max, fabsf(__fsub_rn(wn, wc)));
                w_max = fmaxf(w_max, fabsf(wn));
                slim_sync<LDS>();
            }
            if (w_max == 0.f || __fdiv_rn(d_w_max, w_max) < p.tol || it == p.max_iter - 1) {
                // duality gap (positive branch): max over c of X[:, c] . r - l2 w[c]; a zeroed column gives -l2 w[c] = 0
                double dual = -INFINITY;
                for (int64_t c = 0; c < I; ++c) {
                    double acc = 0.0;
                    if (REF || c != j) {
                        for (int64_t e = cp[c] + lane; e < cp[c + 1]; e += 64) {
                            const int32_t idx = ci[e];
                            if (REF && idx == j) continue;
                            acc += (double)cv[e] * (double)r[idx];
                        }
                    }
                    dual = fmax(dual, slim_wave_sum(acc) - l2 * (double)w[c]);
                }
                double rr = 0.0, ww = 0.0, wl = 0.0, ry = 0.0;
                for (int64_t i = lane; i < U; i += 64) rr += (double)r[i] * (double)r[i];
                for (int64_t i = lane; i < I; i += 64) {
                    const double wi = (double)w[i];
                    ww += wi * wi;
                    wl += fabs(wi);
                }
                for (int64_t e = y0 + lane; e < y1; e += 64) ry += (double)r[ci[e]] * (double)cv[e];
                rr = slim_wave_sum(rr), ww = slim_wave_sum(ww), wl = slim_wave_sum(wl), ry = slim_wave_sum(ry);
                double cst = 1.0, gap = rr;
                if (dual > l1) {
                    cst = l1 / dual;
                    gap = 0.5 * (rr + rr * (cst * cst));
                }
                gap += l1 * wl - cst * ry + 0.5 * l2 * (1.0 + cst * cst) * ww;
                if (gap < (double)tol_abs) {
                    sweeps = it + 1;
                    break;
                }
            }
        }
    }
    if (lane == 0) p.n_iter[t] = sweeps;
    if (p.coef)
        for (int64_t i = lane; i < I; i += 64) p.coef[t * I + i] = w[i];

    // the cut: the weights are >= 0, so the non-zeros are the positives
    int nnz = 0;
    for (int64_t base = 0; base < I; base += 64) nnz += __popcll(__ballot(base + lane < I && w[base + lane] != 0.f));
    const int K = nnz - 1 < p.N ? nnz - 1 : p.N;
    if (K <= 0) {
        if (lane == 0) p.lcnt[t] = 0;
        return;
    }
    slim_sync<LDS>();
    ElWaveSelect<ElPackedKey> sel(keys, p.cap, K);
    for (int64_t base = 0; base < I; base += 64) {
        const int64_t i = base + lane;
        float v = 0.f;
        if (i < I) v = w[i];
        sel.push(v != 0.f && v >= sel.tau, v, (int32_t)i, lane);
    }
    sel.finish(lane);                                          // K <= nnz - 1: the stream holds more than K
    for (int q = lane; q < K; q += 64) {
        p.lx[t * p.N + q] = el_key_item(keys[q]);
        p.lv[t * p.N + q] = el_key_score(keys[q]);
    }
    if (lane == 0) p.lcnt[t] = K;
}

// exclusion = reference: norm of every column without the entry of user row j, per target (one column per lane)
__global__ __launch_bounds__(64) void k_slim_norm_ref(const int64_t* __restrict__ cp, const int32_t* __restrict__ ci,
                                                      const float* __restrict__ cv, int64_t I, int64_t j_start,
                                                      float* __restrict__ norm) {
    const int64_t t = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= I) return;
    const int32_t j = (int32_t)(j_start + t);
    float s = 0.f;
    for (int64_t e = cp[c]; e < cp[c + 1]; ++e)
        if (ci[e] != j) s = __fadd_rn(s, __fmul_rn(cv[e], cv[e]));
    norm[t * I + c] = s;
}

size_t slim_cut_lds(int N) { return ElPackedKey::lds_bytes(el_select_cap(N)); }

size_t slim_w_bytes(int64_t I) { return ((size_t)I * 4 + 15) & ~(size_t)15; }

// bytes of LDS of the LDS placement (0: the residual goes to the workspace)
size_t slim_lds_placement(int64_t U, int64_t I, int N) {
    const size_t rb = (size_t)U * 4, cut = slim_cut_lds(N);
    const size_t need = slim_w_bytes(I) + (rb > cut ? rb : cut);
    return need <= SLIM_LDS_BYTES ? need : 0;
}

struct SlimFitWs {      // norm [I], the per-target norm [n, I] (reference); global placement: residuals [n, U], coefficients [n, I] (else NULL)
    float *norm, *norm_t, *gr, *gw;
};
size_t slim_fit_carve(int64_t U, int64_t I, int N, int64_t n, void* base, SlimFitWs* w) {
    ElCarve c{(char*)base};
    w->norm = c.take<float>((size_t)I);
    w->norm_t = c.take<float>((size_t)n * I);
    const bool global = !slim_lds_placement(U, I, N);
    w->gr = global ? c.take<float>((size_t)n * U) : nullptr;
    w->gw = global ? c.take<float>((size_t)n * I) : nullptr;
    return c.off;
}

struct SlimWWs {        // the row counts [I], then the list-to-CSR arrays
    int32_t* rowcnt;
    KnnCsrWs csr;
};
size_t slim_w_carve(int64_t I, int N, void* base, SlimWWs* w) {
    ElCarve c{(char*)base};
    w->rowcnt = c.take<int32_t>((size_t)I);
    w->csr = el_knn_csr_carve(c, I, N);
    return c.off;
}

}  // namespace

extern "C" int el_slim_order(el_ctx* ctx, void* stream, uint32_t seed_state, int64_t I, int64_t n_draws, int32_t* order) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(order, "el_slim_order: null pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && n_draws >= 0, "el_slim_order: bad sizes I=%lld n_draws=%lld", (long long)I,
               (long long)n_draws);
    if (n_draws == 0) return 0;
    EL_LAUNCH("k_slim_order", k_slim_order, dim3(1), dim3(64), 0, (hipStream_t)stream, (u32)seed_state, (u32)I, n_draws, order);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t el_slim_ws_bytes(int64_t U, int64_t I, int64_t n_cols, int32_t n_neighbors) {
    if (U <= 0 || I <= 0 || n_neighbors <= 0 || n_cols < 0) return 0;
    const int N = (int)(n_neighbors < I ? n_neighbors : I);
    SlimFitWs f;
    SlimWWs w;
    return n_cols > 0 ? slim_fit_carve(U, I, N, n_cols < I ? n_cols : I, nullptr, &f) : slim_w_carve(I, N, nullptr, &w);
}

extern "C" int el_slim_fit(el_ctx* ctx, void* stream, const int64_t* csc_indptr, const int32_t* csc_indices, const float* csc_vals,
                           int64_t U, int64_t I, float l1, float l2, int32_t max_iter, float tol, const int32_t* order,
                           int exclusion, int64_t j_start, int64_t j_stop, int32_t n_neighbors, int32_t* list_idx, float* list_val,
                           int32_t* list_cnt, int32_t* n_iter, float* coef_or_null, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(csc_indptr && csc_indices && csc_vals && order, "el_slim_fit: null input pointer");
    EL_REQUIRE(list_idx && list_val && list_cnt && n_iter, "el_slim_fit: null output pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && U >= 1 && U < 0x7fffffffLL, "el_slim_fit: bad sizes U=%lld I=%lld", (long long)U,
               (long long)I);
    EL_REQUIRE(max_iter >= 1 && tol >= 0.f && l1 >= 0.f && l2 >= 0.f, "el_slim_fit: bad solver arguments (max_iter %d)", max_iter);
    EL_REQUIRE(exclusion == EL_SLIM_COLUMN || exclusion == EL_SLIM_REFERENCE, "el_slim_fit: unknown exclusion %d", exclusion);
    EL_REQUIRE(exclusion != EL_SLIM_REFERENCE || I <= U,
               "el_slim_fit: exclusion = reference with %lld items and %lld users: the reference reads indptr[item] of a CSR with "
               "U + 1 entries and raises IndexError at item %lld",
               (long long)I, (long long)U, (long long)U);
    EL_REQUIRE(n_neighbors >= 1, "el_slim_fit: n_neighbors must be >= 1");
    const int N = (int)(n_neighbors < I ? n_neighbors : I);
    EL_REQUIRE(N <= SLIM_MAX_NEIGHBORS, "el_slim_fit: n_neighbors %d > %d unsupported", N, SLIM_MAX_NEIGHBORS);
    EL_REQUIRE(j_start >= 0 && j_stop >= j_start && j_stop <= I, "el_slim_fit: bad column range [%lld, %lld)", (long long)j_start,
               (long long)j_stop);
    const int64_t n = j_stop - j_start;
    if (n == 0) return 0;
    SlimFitWs w;
    const size_t need = slim_fit_carve(U, I, N, n, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_slim_fit: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    const bool ref = exclusion == EL_SLIM_REFERENCE;
    const size_t lds_fit = slim_lds_placement(U, I, N);
    SlimFit p;
    p.cp = csc_indptr, p.ci = csc_indices, p.cv = csc_vals, p.order = order;
    p.gr = w.gr, p.gw = w.gw;
    p.U = U, p.I = I, p.j_start = j_start;
    p.l1 = l1, p.l2 = l2, p.tol = tol, p.max_iter = max_iter, p.reference = ref ? 1 : 0;
    p.N = N, p.cap = el_select_cap(N), p.w_bytes = (int)slim_w_bytes(I);
    p.lx = list_idx, p.lv = list_val, p.lcnt = list_cnt, p.n_iter = n_iter, p.coef = coef_or_null;
    if (ref) {
        EL_LAUNCH("k_slim_norm_ref", k_slim_norm_ref, dim3((unsigned)((I + 63) / 64), (unsigned)n), dim3(64), 0, st, csc_indptr,
                  csc_indices, csc_vals, I, j_start, w.norm_t);
        p.norm = w.norm_t;
    } else {
        EL_LAUNCH("k_slim_norm", k_slim_norm, dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st, csc_indptr, csc_vals, I, w.norm);
        p.norm = w.norm;
    }
    EL_CHECK_LAUNCH();
    const size_t lds = lds_fit ? lds_fit : slim_cut_lds(N);
    void (*kern)(SlimFit) = lds_fit ? (ref ? k_slim_fit<true, true> : k_slim_fit<true, false>)
                                    : (ref ? k_slim_fit<false, true> : k_slim_fit<false, false>);
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    EL_LAUNCH(lds_fit ? "k_slim_fit_lds" : "k_slim_fit_global", kern, dim3((unsigned)n), dim3(64), lds, st, p);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_slim_w(el_ctx* ctx, void* stream, const int32_t* list_idx, const float* list_val, const int32_t* list_cnt,
                         int64_t I, int32_t N, int64_t* w_indptr, int32_t* w_indices, float* w_vals, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(list_idx && list_val && list_cnt, "el_slim_w: null input pointer");
    EL_REQUIRE(w_indptr && w_indices && w_vals, "el_slim_w: null output pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL, "el_slim_w: bad item count %lld", (long long)I);
    EL_REQUIRE(N >= 1 && N <= I && N <= SLIM_MAX_NEIGHBORS, "el_slim_w: list width %d outside [1, min(I, %d)]", N, SLIM_MAX_NEIGHBORS);
    SlimWWs w;
    const size_t need = slim_w_carve(I, N, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_slim_w: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    EL_CHECK_HIP(hipMemsetAsync(w.rowcnt, 0, (size_t)I * 4, st));
    EL_LAUNCH("k_knn_count", k_knn_count, dim3((unsigned)(((size_t)I * N + 255) / 256)), dim3(256), 0, st, list_idx, list_cnt, I, N,
              w.rowcnt);
    EL_CHECK_LAUNCH();
    return el_knn_csr_launch(st, list_idx, list_val, list_cnt, I, N, w.rowcnt, w_indptr, w_indices, w_vals, w.csr);
}
