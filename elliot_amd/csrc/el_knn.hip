// Neighbourhood models (ItemKNN / UserKNN, implementation: standard).
//
// Replaces item_knn_similarity.py / user_knn_similarity.py (Similarity.initialize, get_user_recs) of the reference:
//   el_knn_build       co-occurrence similarity of one side of R, top-N non-zeros per target column, then W as CSR
//   el_knn_score_topk  score[u, :] = sum over A row u (stored order) of A[u,a] * B[a, :], masked top-k
//
// Numerics contract (tests/helpers/knn_ref.py restates it in NumPy):
//   cnt[c, x] = sum_t r_tc * r_tx    exact: integer-scaled ratings, integer LDS atomics (no float atomics, any order)
//   n_c       = sum_t r_tc^2         exact, int64
//   dot       = (float)((double)cnt / s^2)
//   cosine    = (float)(cnt_d / sqrt(n_c_d * n_x_d)),  every operand a double divided by s^2, fp64 correctly rounded
//   top-N     = non-zero values only, (value desc, index asc)
//   score     = __fadd_rn(acc, __fmul_rn(a, b)) in A's stored order, from +0 for every item (scipy csr_matmat)
//   top-k     = (score desc, index asc) over unmasked items, zero scores included; (-1, -inf) padding
// Neither n x n similarity nor the [U, I] score block is ever written to memory: both kernels accumulate one LDS tile of
// the x / item range at a time and carry their running selection from tile to tile.
#include "el_common.h"

#include "el_knn_csr.h"
#include "el_knn_select.h"
#include "el_topk_common.h"

#define KNN_TILE_BYTES 65536                      // LDS accumulator tile of both kernels
#define KNN_MAX_K 4032                            // running top-k of the scoring wave (cap = el_select_cap(k) <= 4096)

namespace {

struct KnnBuild {
    const int64_t* pp;   // targets -> other side (t), integer-scaled values
    const int32_t* pi;
    const int32_t* pv;
    const int64_t* qp;   // other side (t) -> x, columns ascending
    const int32_t* qi;
    const int32_t* qv;
    int64_t n;           // targets == x range
    int N;               // neighbours kept (<= n)
    int sim;
    double inv_s2;       // 1 / scale^2 (exact)
    int tile;            // accumulator entries per pass
    int cap;             // running-selection slots (power of two >= 2 N + 256)
    const int64_t* nrm;  // [n] sum of squares
    int32_t* lx;         // [n, N] neighbour lists
    float* lv;
    int32_t* lcnt;       // [n] list lengths
    int32_t* rowcnt;     // [n] entries per row of W
};

__global__ __launch_bounds__(256) void k_knn_norms(const int64_t* __restrict__ pp, const int32_t* __restrict__ pv, int64_t n,
                                                   int64_t* __restrict__ nrm) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    int64_t s = 0;
    for (int64_t e = pp[c]; e < pp[c + 1]; ++e) s += (int64_t)pv[e] * (int64_t)pv[e];
    nrm[c] = s;
}

__device__ __forceinline__ float knn_value(int64_t cnt, double nc, int64_t nx_int, int sim, double inv_s2) {
    const double cd = __dmul_rn((double)cnt, inv_s2);
    if (sim == EL_KNN_DOT) return (float)cd;
    const double nx = __dmul_rn((double)nx_int, inv_s2);
    return (float)__ddiv_rn(cd, __dsqrt_rn(__dmul_rn(nc, nx)));
}

// One workgroup per target column c: expand every t of P row c over Q row t into an LDS tile of the x range (integer
// atomics), turn the tile into values, keep the running top-N non-zeros; the next tile of x reuses the LDS.
template <typename ACC>
__global__ __launch_bounds__(KNN_BUILD_THREADS) void k_knn_topn(KnnBuild p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                                  // [cap]
    ACC* acc = reinterpret_cast<ACC*>(smem + (size_t)p.cap * 8);               // [tile]
    __shared__ int s_cnt;
    __shared__ u64 s_tau;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nw = KNN_BUILD_THREADS / 64;
    const int64_t c = blockIdx.x;
    const int64_t p0 = p.pp[c], p1 = p.pp[c + 1];
    const double nc = __dmul_rn((double)p.nrm[c], p.inv_s2);
    if (tid == 0) {
        s_cnt = 0;
        s_tau = 0ull;
    }
    for (int64_t x0 = 0; x0 < p.n; x0 += p.tile) {
        const int64_t x1 = (x0 + p.tile < p.n) ? x0 + p.tile : p.n;
        const int w = (int)(x1 - x0);
        const bool tiled = p.tile < p.n;
        for (int i = tid; i < w; i += KNN_BUILD_THREADS) acc[i] = 0;
        __syncthreads();
        for (int64_t e = p0 + wv; e < p1; e += nw) {
            const int32_t t = p.pi[e];
            const ACC rv = (ACC)p.pv[e];
            int64_t q0 = p.qp[t], q1 = p.qp[t + 1];
            if (tiled) {
                q0 = el_lower_bound(p.qi, q0, q1, (int32_t)x0);
                q1 = el_lower_bound(p.qi, q0, q1, (int32_t)x1);
            }
            for (int64_t f = q0 + lane; f < q1; f += 64) atomicAdd(&acc[p.qi[f] - x0], rv * (ACC)p.qv[f]);
        }
        __syncthreads();
        for (int base = 0; base < w; base += KNN_BUILD_THREADS) {
            const int i = base + tid;
            const u64 tau = s_tau;
            if (i < w) {
                const ACC a = acc[i];
                if (a != 0) {
                    const u64 key = el_make_key(knn_value((int64_t)a, nc, p.nrm[x0 + i], p.sim, p.inv_s2), (int32_t)(x0 + i));
                    if (key > tau) keys[atomicAdd(&s_cnt, 1)] = key;
                }
            }
            __syncthreads();
            const int cnt = s_cnt;
            __syncthreads();                                  // every thread has read s_cnt before it changes
            if (cnt > p.cap - KNN_BUILD_THREADS) knn_block_compact(keys, cnt, p.cap, p.N, &s_cnt, &s_tau);
        }
    }
    __syncthreads();
    const int cnt = s_cnt;
    __syncthreads();
    knn_block_compact(keys, cnt, p.cap, p.N, &s_cnt, &s_tau);
    const int m = cnt < p.N ? cnt : p.N;
    for (int j = tid; j < m; j += KNN_BUILD_THREADS) {
        const u64 key = keys[j];
        const int32_t x = el_key_item(key);
        p.lx[c * p.N + j] = x;
        p.lv[c * p.N + j] = el_key_score(key);
        atomicAdd(&p.rowcnt[x], 1);
    }
    if (tid == 0) p.lcnt[c] = m;
}

struct KnnScore {
    const int64_t* ap;
    const int32_t* ai;
    const float* av;
    const int64_t* bp;   // columns ascending inside each row
    const int32_t* bi;
    const float* bv;
    int64_t u_start, I;
    const int64_t* excl_indptr;
    const int32_t* excl_indices;
    const int64_t* cand_indptr;
    const int32_t* cand_indices;
    int k, tile, cap;
    int32_t* out_idx;
    float* out_val;
};

// One wave per user: walk A's row in stored order, lanes over B's row (distinct columns: one add per item per step, in
// scipy's order, no barrier but the wave's own LDS ordering), then select from the tile; the running top-k buffer carries
// from one item tile to the next.
__global__ __launch_bounds__(64) void k_knn_score(KnnScore p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                                  // [cap]
    int* cnt_s = reinterpret_cast<int*>(smem + (size_t)p.cap * 8);             // [1] (+pad)
    float* acc = reinterpret_cast<float*>(smem + (size_t)p.cap * 8 + 16);      // [tile]
    const int lane = threadIdx.x;
    const int64_t urel = blockIdx.x;
    const int64_t u = p.u_start + urel;
    const int64_t a0 = p.ap[u], a1 = p.ap[u + 1];
    int64_t e0 = 0, e1 = 0, c0 = 0, c1 = 0;
    const bool use_cand = p.cand_indptr != nullptr;
    if (use_cand) {
        c0 = p.cand_indptr[u];
        c1 = p.cand_indptr[u + 1];
    } else if (p.excl_indptr) {
        e0 = p.excl_indptr[u];
        e1 = p.excl_indptr[u + 1];
    }
    const bool tiled = p.tile < p.I;
    ElWaveSelect sel(keys, cnt_s, p.cap, p.k);
    for (int64_t i0 = 0; i0 < p.I; i0 += p.tile) {
        const int64_t i1 = (i0 + p.tile < p.I) ? i0 + p.tile : p.I;
        const int w = (int)(i1 - i0);
        for (int i = lane; i < w; i += 64) acc[i] = 0.f;
        el_wave_lds_sync();
        for (int64_t a = a0; a < a1; ++a) {
            const int32_t j = p.ai[a];
            const float x = p.av[a];
            int64_t q0 = p.bp[j], q1 = p.bp[j + 1];
            if (tiled) {
                q0 = el_lower_bound(p.bi, q0, q1, (int32_t)i0);
                q1 = el_lower_bound(p.bi, q0, q1, (int32_t)i1);
            }
            for (int64_t f = q0 + lane; f < q1; f += 64) {
                float* s = &acc[p.bi[f] - i0];
                *s = __fadd_rn(*s, __fmul_rn(x, p.bv[f]));
            }
            el_wave_lds_sync();
        }
        int64_t s0 = 0, s1 = w;                                                // positions to scan in this tile
        if (use_cand) {
            s0 = el_lower_bound(p.cand_indices, c0, c1, (int32_t)i0);
            s1 = el_lower_bound(p.cand_indices, s0, c1, (int32_t)i1);
        } else if (e1 > e0) {                                                  // excluded items of the tile -> NaN (never selected)
            const int64_t f0 = el_lower_bound(p.excl_indices, e0, e1, (int32_t)i0);
            const int64_t f1 = el_lower_bound(p.excl_indices, f0, e1, (int32_t)i1);
            for (int64_t f = f0 + lane; f < f1; f += 64) acc[p.excl_indices[f] - i0] = __builtin_nanf("");
            el_wave_lds_sync();
        }
        for (int64_t base = s0; base < s1; base += 64) {
            const int64_t pos = base + lane;
            bool hit = false;
            float s = 0.f;
            int32_t item = -1;
            if (pos < s1) {
                item = use_cand ? p.cand_indices[pos] : (int32_t)(i0 + pos);
                s = acc[item - i0] + 0.0f;
                hit = (s == s) && s >= sel.tau;
            }
            sel.push(hit, s, item, lane);
        }
        el_wave_lds_sync();
    }
    const int nv = sel.finish(lane);
    for (int t = lane; t < p.k; t += 64) {
        int32_t oi = -1;
        float ov = -INFINITY;
        if (t < nv) {
            oi = el_key_item(keys[t]);
            ov = el_key_score(keys[t]);
        }
        p.out_idx[urel * p.k + t] = oi;
        p.out_val[urel * p.k + t] = ov;
    }
}

struct KnnWs {          // the workspace of el_knn_build: KnnBuild's nrm, lcnt, rowcnt [n] and lx, lv [n, N], then the list-to-CSR arrays
    int64_t* nrm;
    int32_t *lcnt, *rowcnt, *lx;
    float* lv;
    KnnCsrWs csr;
};
size_t knn_carve(int64_t n, int N, void* base, KnnWs* w) {
    ElCarve c{(char*)base};
    w->nrm = c.take<int64_t>((size_t)n);
    w->lcnt = c.take<int32_t>((size_t)n);
    w->rowcnt = c.take<int32_t>((size_t)n);
    w->lx = c.take<int32_t>((size_t)n * N);
    w->lv = c.take<float>((size_t)n * N);
    w->csr = el_knn_csr_carve(c, n, N);
    return c.off;
}

}  // namespace

extern "C" size_t el_knn_ws_bytes(int64_t n, int32_t n_neighbors) {
    if (n <= 0 || n_neighbors <= 0) return 0;
    KnnWs w;
    return knn_carve(n, (int)(n_neighbors < n ? n_neighbors : n), nullptr, &w);
}

extern "C" int el_knn_build(el_ctx* ctx, void* stream, const int64_t* p_indptr, const int32_t* p_indices, const int32_t* p_vals,
                            const int64_t* q_indptr, const int32_t* q_indices, const int32_t* q_vals, int64_t n, int64_t n_other,
                            int32_t n_neighbors, int sim, int32_t scale, int64_t max_deg, int32_t max_abs, int64_t* w_indptr,
                            int32_t* w_indices, float* w_vals, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(p_indptr && p_indices && p_vals && q_indptr && q_indices && q_vals, "el_knn_build: null input pointer");
    EL_REQUIRE(w_indptr && w_indices && w_vals, "el_knn_build: null output pointer");
    EL_REQUIRE(n >= 1 && n < 0x7fffffffLL && n_other >= 1 && n_other < 0x7fffffffLL, "el_knn_build: bad sizes n=%lld n_other=%lld",
               (long long)n, (long long)n_other);
    EL_REQUIRE(sim == EL_KNN_COSINE || sim == EL_KNN_DOT, "el_knn_build: similarity %d unsupported (EL_KNN_COSINE, EL_KNN_DOT)", sim);
    EL_REQUIRE(scale == 1 || scale == 2, "el_knn_build: scale %d unsupported (1: integer ratings, 2: half steps)", scale);
    EL_REQUIRE(n_neighbors >= 1, "el_knn_build: n_neighbors must be >= 1");
    EL_REQUIRE(max_deg >= 0 && max_abs >= 0, "el_knn_build: bad bounds");
    const int N = (int)(n_neighbors < n ? n_neighbors : n);
    EL_REQUIRE(N <= KNN_MAX_NEIGHBORS, "el_knn_build: n_neighbors %d > %d unsupported", N, KNN_MAX_NEIGHBORS);
    // every count and norm is a sum of at most max_deg terms of magnitude <= max_abs^2
    const double bound = (double)max_deg * (double)max_abs * (double)max_abs;
    EL_REQUIRE(bound < 4.0e18, "el_knn_build: max degree %lld x max |r|^2 %lld overflows the int64 accumulator",
               (long long)max_deg, (long long)max_abs * max_abs);
    const bool acc64 = bound > 2147483647.0;
    KnnWs w;
    const size_t need = knn_carve(n, N, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_knn_build: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    EL_CHECK_HIP(hipMemsetAsync(w.rowcnt, 0, (size_t)n * 4, st));
    EL_LAUNCH("k_knn_norms", k_knn_norms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p_indptr, p_vals, n, w.nrm);
    EL_CHECK_LAUNCH();
    KnnBuild p;
    p.pp = p_indptr, p.pi = p_indices, p.pv = p_vals;
    p.qp = q_indptr, p.qi = q_indices, p.qv = q_vals;
    p.n = n, p.N = N, p.sim = sim, p.inv_s2 = 1.0 / ((double)scale * scale);
    p.tile = KNN_TILE_BYTES / (acc64 ? 8 : 4);
    p.cap = knn_build_cap(N);
    p.nrm = w.nrm, p.lx = w.lx, p.lv = w.lv, p.lcnt = w.lcnt, p.rowcnt = w.rowcnt;
    const size_t lds = (size_t)p.cap * 8 + KNN_TILE_BYTES;
    if (acc64) {
        EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_topn<unsigned long long>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        EL_LAUNCH("k_knn_topn", k_knn_topn<unsigned long long>, dim3((unsigned)n), dim3(KNN_BUILD_THREADS), lds, st, p);
    } else {
        EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_topn<int>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
        EL_LAUNCH("k_knn_topn", k_knn_topn<int>, dim3((unsigned)n), dim3(KNN_BUILD_THREADS), lds, st, p);
    }
    EL_CHECK_LAUNCH();
    return el_knn_csr_launch(st, w.lx, w.lv, w.lcnt, n, N, w.rowcnt, w_indptr, w_indices, w_vals, w.csr);
}

extern "C" int el_knn_score_topk(el_ctx* ctx, void* stream, const int64_t* a_indptr, const int32_t* a_indices, const float* a_vals,
                                 const int64_t* b_indptr, const int32_t* b_indices, const float* b_vals, int64_t u_start,
                                 int64_t u_stop, int64_t I, const int64_t* excl_indptr, const int32_t* excl_indices,
                                 const int64_t* cand_indptr, const int32_t* cand_indices, int32_t k, int32_t* out_idx,
                                 float* out_val) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(a_indptr && a_indices && a_vals && b_indptr && b_indices && b_vals, "el_knn_score_topk: null input pointer");
    EL_REQUIRE(out_idx && out_val, "el_knn_score_topk: null output pointer");
    EL_REQUIRE(u_start >= 0 && u_stop >= u_start && u_stop - u_start < 0x7fffffffLL, "el_knn_score_topk: bad user range");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL, "el_knn_score_topk: bad item count %lld", (long long)I);
    EL_REQUIRE(k >= 1 && k <= KNN_MAX_K, "el_knn_score_topk: k=%d unsupported (1..%d)", k, KNN_MAX_K);
    EL_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), "el_knn_score_topk: excl CSR needs both arrays");
    EL_REQUIRE((cand_indptr == nullptr) == (cand_indices == nullptr), "el_knn_score_topk: cand CSR needs both arrays");
    if (u_stop == u_start) return 0;
    KnnScore p;
    p.ap = a_indptr, p.ai = a_indices, p.av = a_vals;
    p.bp = b_indptr, p.bi = b_indices, p.bv = b_vals;
    p.u_start = u_start, p.I = I;
    p.excl_indptr = excl_indptr, p.excl_indices = excl_indices;
    p.cand_indptr = cand_indptr, p.cand_indices = cand_indices;
    p.k = k;
    p.cap = el_select_cap(k);
    const int64_t max_tile = KNN_TILE_BYTES / 4;
    p.tile = (int)(I < max_tile ? ((I + 63) / 64) * 64 : max_tile);
    p.out_idx = out_idx, p.out_val = out_val;
    const size_t lds = (size_t)p.cap * 8 + 16 + (size_t)p.tile * 4;
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    EL_LAUNCH("k_knn_score", k_knn_score, dim3((unsigned)(u_stop - u_start)), dim3(64), lds, (hipStream_t)stream, p);
    EL_CHECK_LAUNCH();
    return 0;
}
