// Neighbourhood models (ItemKNN / UserKNN, implementation: standard; AttributeItemKNN / AttributeUserKNN / VSM).
//
// Replaces item_knn_similarity.py / user_knn_similarity.py / attribute_user_knn_similarity.py (Similarity.initialize,
// get_user_recs) of the reference:
//   el_knn_build       co-occurrence similarity of one side of R, top-N non-zeros per target column, then W as CSR
//   el_knn_build_f32   the same for float-valued rows (attribute profiles), self-similarity kept
//   el_knn_score_topk  score[u, :] = sum over A row u (stored order) of A[u,a] * B[a, :], masked top-k
//
// One similarity kernel, k_knn_topn<CELL>, for three kinds of rows; the kind is the type of an LDS cell:
//   int, unsigned long long   integer-scaled ratings, exact counts               (tests/helpers/knn_ref.py restates it in NumPy)
//     cnt[c, x] = sum_t r_tc * r_tx    integer LDS atomics, the waves side by side (no float atomics, any order)
//     n_c       = sum_t r_tc^2         exact, int64
//     d         = (double)cnt / s^2,   every norm likewise a double divided by s^2
//   double                    float rows, fp64 sums in stored order              (tests/helpers/attr_ref.py restates it)
//     d[c, x]   = sum_t P[c,t] Q[t,x]  one __dadd_rn(acc, __dmul_rn(p, q)) per entry t of P row c IN STORED ORDER, from +0 (the
//                                      product of two floats is exact in fp64): the whole workgroup takes one entry at a time,
//                                      every cell is written by one lane per step and a barrier orders the steps
//     n_c       = sum_t P[c,t]^2       likewise
//   dot       = (float)d
//   cosine    = (float)(d / sqrt(n_c * n_x)), fp64 correctly rounded
//   top-N     = cells with d != 0 whose value does not round to 0.0f (only a float row's can), (value desc, index asc)
//   score     = __fadd_rn(acc, __fmul_rn(a, b)) in A's stored order, from +0 for every item (scipy csr_matmat)
//   top-k     = (score desc, index asc) over unmasked items, zero scores included; (-1, -inf) padding
// Neither n x n similarity nor the [U, I] score block is ever written to memory: both kernels accumulate one LDS tile of
// the x / item range at a time and carry their running selection from tile to tile.
#include "el_common.h"

#include "el_knn_csr.h"
#include "el_topk_common.h"

#define KNN_TILE_BYTES 65536                      // LDS accumulator tile of both kernels
#define KNN_MAX_K 4032                            // running top-k of the scoring wave (cap = el_select_cap(k) <= 4096)
#define KNN_BUILD_THREADS 256
#define KNN_MAX_NEIGHBORS 2048                    // running top-N lives in LDS next to the tile

namespace {

// ---- running top-N of one workgroup in LDS: keys (el_make_key: value desc, index asc) are appended to keys[0 .. cap) and cut
// back to the best N whenever fewer than one pass of the workgroup fits behind them -----------------------------------------------
// block-wide bitonic sort (descending) of n = 2^m keys in LDS
__device__ void knn_block_bitonic_desc(u64* a, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                int i = 2 * t - (t & (stride - 1));
                int j = i + stride;
                bool desc = ((i & size) == 0);
                u64 x = a[i], y = a[j];
                if (desc ? (x < y) : (x > y)) {
                    a[i] = y;
                    a[j] = x;
                }
            }
            __syncthreads();
        }
    }
}

// keep the best N of the cnt keys in keys[0 .. cap); every thread passes the same cnt
__device__ void knn_block_compact(u64* keys, int cnt, int cap, int N, int* s_cnt, u64* s_tau) {
    for (int t = cnt + (int)threadIdx.x; t < cap; t += blockDim.x) keys[t] = 0ull;
    __syncthreads();
    knn_block_bitonic_desc(keys, cap);
    if (threadIdx.x == 0) {
        *s_cnt = cnt < N ? cnt : N;
        *s_tau = cnt >= N ? keys[N - 1] : 0ull;
    }
    __syncthreads();
}

// running-selection slots: a power of two >= 2 N + one pass of the workgroup
inline int knn_build_cap(int N) { return el_pow2(2 * N + KNN_BUILD_THREADS); }

// ---- the kinds of rows ------------------------------------------------------------------------------------------------------
template <typename CELL>
struct KnnKind {                 // integer counts, CELL = int or unsigned long long
    typedef int32_t val_t;       // a stored value
    typedef int64_t sum_t;       // a norm; a cell widens to it with its sign
    static int tile(int64_t) { return KNN_TILE_BYTES / sizeof(CELL); }          // cells per pass: the 64 KiB whatever n is
};
template <>
struct KnnKind<double> {         // float rows
    typedef float val_t;
    typedef double sum_t;
    static int tile(int64_t n) { return (int)(n < KNN_TILE_BYTES / 8 ? ((n + 63) / 64) * 64 : KNN_TILE_BYTES / 8); }
};

// s + a * b: exact for counts; two correctly rounded fp64 steps, never fused, for float rows
__device__ __forceinline__ int64_t knn_madd(int64_t s, int64_t a, int64_t b) { return s + a * b; }
__device__ __forceinline__ double knn_madd(double s, double a, double b) { return __dadd_rn(s, __dmul_rn(a, b)); }
// a count or a norm as the double the similarity is made of
__device__ __forceinline__ double knn_real(int64_t s, double inv_s2) { return __dmul_rn((double)s, inv_s2); }
__device__ __forceinline__ double knn_real(double s, double) { return s; }

template <typename CELL>
struct KnnBuild {
    typedef typename KnnKind<CELL>::val_t val_t;
    typedef typename KnnKind<CELL>::sum_t sum_t;
    const int64_t* pp;   // targets -> other side (t); float rows: stored order = summation order
    const int32_t* pi;
    const val_t* pv;
    const int64_t* qp;   // other side (t) -> x, columns ascending
    const int32_t* qi;
    const val_t* qv;
    int64_t n;           // targets == x range
    int N;               // neighbours kept (<= n)
    int sim;
    double inv_s2;       // 1 / scale^2 (exact; integer kinds only)
    int tile;            // accumulator entries per pass
    int cap;             // running-selection slots (power of two >= 2 N + 256)
    const sum_t* nrm;    // [n] sum of squares
    int32_t* lx;         // [n, N] neighbour lists
    float* lv;
    int32_t* lcnt;       // [n] list lengths
    int32_t* rowcnt;     // [n] entries per row of W
};

template <typename V, typename S>
__global__ __launch_bounds__(256) void k_knn_norms(const int64_t* __restrict__ pp, const V* __restrict__ pv, int64_t n,
                                                   S* __restrict__ nrm) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    S s = 0;
    for (int64_t e = pp[c]; e < pp[c + 1]; ++e) s = knn_madd(s, (S)pv[e], (S)pv[e]);
    nrm[c] = s;
}

// P row [p0, p1) over the rows of Q into the zeroed tile acc of [x0, x1); every thread sees the finished tile on return.
// Counts: the waves side by side, integer atomics.
template <typename CELL>
__device__ __forceinline__ void knn_expand(CELL* acc, const KnnBuild<CELL>& p, int64_t p0, int64_t p1, int64_t x0, int64_t x1,
                                           bool tiled) {
    el_count_expand<KNN_BUILD_THREADS / 64>(acc, p.pi, p.pv, p0, p1, p.qp, p.qi, p.qv, x0, x1, tiled);
    __syncthreads();
}
// Float rows: the whole workgroup walks the row one entry at a time, its lanes across Q row t (columns distinct: one add per cell
// per step, a barrier between steps fixes the order).
__device__ __forceinline__ void knn_expand(double* acc, const KnnBuild<double>& p, int64_t p0, int64_t p1, int64_t x0, int64_t x1,
                                           bool tiled) {
    for (int64_t e = p0; e < p1; ++e) {
        const int32_t t = p.pi[e];
        const double rv = (double)p.pv[e];
        int64_t q0 = p.qp[t], q1 = p.qp[t + 1];
        if (tiled) {
            q0 = el_lower_bound(p.qi, q0, q1, (int32_t)x0);
            q1 = el_lower_bound(p.qi, q0, q1, (int32_t)x1);
        }
        for (int64_t f = q0 + threadIdx.x; f < q1; f += KNN_BUILD_THREADS) {
            double* a = &acc[p.qi[f] - x0];
            *a = knn_madd(*a, rv, (double)p.qv[f]);
        }
        __syncthreads();
    }
}

// One workgroup per target column c: expand P row c over the rows of Q into an LDS tile of the x range, turn the tile into
// values, keep the running top-N; the next tile of x reuses the LDS.
template <typename CELL>
__global__ __launch_bounds__(KNN_BUILD_THREADS) void k_knn_topn(KnnBuild<CELL> p) {
    typedef typename KnnKind<CELL>::sum_t sum_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                                  // [cap]
    CELL* acc = reinterpret_cast<CELL*>(smem + (size_t)p.cap * 8);             // [tile]
    __shared__ int s_cnt;
    __shared__ u64 s_tau;
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int64_t p0 = p.pp[c], p1 = p.pp[c + 1];
    const double nc = knn_real(p.nrm[c], p.inv_s2);
    if (tid == 0) {
        s_cnt = 0;
        s_tau = 0ull;
    }
    for (int64_t x0 = 0; x0 < p.n; x0 += p.tile) {
        const int64_t x1 = (x0 + p.tile < p.n) ? x0 + p.tile : p.n;
        const int w = (int)(x1 - x0);
        for (int i = tid; i < w; i += KNN_BUILD_THREADS) acc[i] = 0;
        __syncthreads();
        knn_expand(acc, p, p0, p1, x0, x1, p.tile < p.n);
        for (int base = 0; base < w; base += KNN_BUILD_THREADS) {
            const int i = base + tid;
            const u64 tau = s_tau;
            if (i < w) {
                const CELL a = acc[i];
                if (a != 0) {
                    const double d = knn_real((sum_t)a, p.inv_s2);
                    const float v = p.sim == EL_KNN_DOT
                                        ? (float)d
                                        : (float)__ddiv_rn(d, __dsqrt_rn(__dmul_rn(nc, knn_real(p.nrm[x0 + i], p.inv_s2))));
                    if (v != 0.0f) {
                        const u64 key = el_make_key(v, (int32_t)(x0 + i));
                        if (key > tau) keys[atomicAdd(&s_cnt, 1)] = key;
                    }
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
    float* acc = reinterpret_cast<float*>(smem + (size_t)p.cap * 8);           // [tile]
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
    ElWaveSelect<ElPackedKey> sel(keys, p.cap, p.k);
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

struct KnnWs {          // the workspace of a build: KnnBuild's nrm (8 bytes per target in every kind), lcnt, rowcnt [n] and
    void* nrm;          // lx, lv [n, N], then the list-to-CSR arrays
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

// What both builds do behind their own checks; `who` is the entry point, k_norms / k_topn the kernels' names in the timing report.
template <typename CELL>
int knn_build(const char* who, const char* k_norms, const char* k_topn, void* stream, const int64_t* p_indptr,
              const int32_t* p_indices, const typename KnnKind<CELL>::val_t* p_vals, const int64_t* q_indptr,
              const int32_t* q_indices, const typename KnnKind<CELL>::val_t* q_vals, int64_t n, int64_t n_other, int32_t n_neighbors,
              int sim, double inv_s2, int64_t* w_indptr, int32_t* w_indices, float* w_vals, void* ws, size_t ws_bytes) {
    typedef typename KnnKind<CELL>::val_t val_t;
    typedef typename KnnKind<CELL>::sum_t sum_t;
    EL_REQUIRE(p_indptr && p_indices && p_vals && q_indptr && q_indices && q_vals, "%s: null input pointer", who);
    EL_REQUIRE(w_indptr && w_indices && w_vals, "%s: null output pointer", who);
    EL_REQUIRE(n >= 1 && n < 0x7fffffffLL && n_other >= 1 && n_other < 0x7fffffffLL, "%s: bad sizes n=%lld n_other=%lld", who,
               (long long)n, (long long)n_other);
    EL_REQUIRE(sim == EL_KNN_COSINE || sim == EL_KNN_DOT, "%s: similarity %d unsupported (EL_KNN_COSINE, EL_KNN_DOT)", who, sim);
    EL_REQUIRE(n_neighbors >= 1, "%s: n_neighbors must be >= 1", who);
    const int N = (int)(n_neighbors < n ? n_neighbors : n);
    EL_REQUIRE(N <= KNN_MAX_NEIGHBORS, "%s: n_neighbors %d > %d unsupported", who, N, KNN_MAX_NEIGHBORS);
    KnnWs w;
    const size_t need = knn_carve(n, N, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "%s: workspace too small (need %zu bytes)", who, need);
    hipStream_t st = (hipStream_t)stream;
    EL_CHECK_HIP(hipMemsetAsync(w.rowcnt, 0, (size_t)n * 4, st));
    EL_LAUNCH(k_norms, (k_knn_norms<val_t, sum_t>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p_indptr, p_vals, n,
              (sum_t*)w.nrm);
    EL_CHECK_LAUNCH();
    KnnBuild<CELL> p;
    p.pp = p_indptr, p.pi = p_indices, p.pv = p_vals;
    p.qp = q_indptr, p.qi = q_indices, p.qv = q_vals;
    p.n = n, p.N = N, p.sim = sim, p.inv_s2 = inv_s2;
    p.tile = KnnKind<CELL>::tile(n);
    p.cap = knn_build_cap(N);
    p.nrm = (const sum_t*)w.nrm, p.lx = w.lx, p.lv = w.lv, p.lcnt = w.lcnt, p.rowcnt = w.rowcnt;
    const size_t lds = (size_t)p.cap * 8 + (size_t)p.tile * sizeof(CELL);
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_topn<CELL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    EL_LAUNCH(k_topn, k_knn_topn<CELL>, dim3((unsigned)n), dim3(KNN_BUILD_THREADS), lds, st, p);
    EL_CHECK_LAUNCH();
    return el_knn_csr_launch(st, w.lx, w.lv, w.lcnt, n, N, w.rowcnt, w_indptr, w_indices, w_vals, w.csr);
}

}  // namespace

extern "C" size_t el_knn_ws_bytes(int64_t n, int32_t n_neighbors) {
    if (n <= 0 || n_neighbors <= 0) return 0;
    KnnWs w;
    return knn_carve(n, (int)(n_neighbors < n ? n_neighbors : n), nullptr, &w);
}

extern "C" size_t el_knn_f32_ws_bytes(int64_t n, int32_t n_neighbors) { return el_knn_ws_bytes(n, n_neighbors); }

extern "C" int el_knn_build(el_ctx* ctx, void* stream, const int64_t* p_indptr, const int32_t* p_indices, const int32_t* p_vals,
                            const int64_t* q_indptr, const int32_t* q_indices, const int32_t* q_vals, int64_t n, int64_t n_other,
                            int32_t n_neighbors, int sim, int32_t scale, int64_t max_deg, int32_t max_abs, int64_t* w_indptr,
                            int32_t* w_indices, float* w_vals, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(scale == 1 || scale == 2, "el_knn_build: scale %d unsupported (1: integer ratings, 2: half steps)", scale);
    EL_REQUIRE(max_deg >= 0 && max_abs >= 0, "el_knn_build: bad bounds");
    // every count and norm is a sum of at most max_deg terms of magnitude <= max_abs^2
    const double bound = (double)max_deg * (double)max_abs * (double)max_abs;
    EL_REQUIRE(bound < 4.0e18, "el_knn_build: max degree %lld x max |r|^2 %lld overflows the int64 accumulator",
               (long long)max_deg, (long long)max_abs * max_abs);
    const auto build = bound > 2147483647.0 ? knn_build<unsigned long long> : knn_build<int>;
    return build("el_knn_build", "k_knn_norms", "k_knn_topn", stream, p_indptr, p_indices, p_vals, q_indptr, q_indices, q_vals, n,
                 n_other, n_neighbors, sim, 1.0 / ((double)scale * scale), w_indptr, w_indices, w_vals, ws, ws_bytes);
}

extern "C" int el_knn_build_f32(el_ctx* ctx, void* stream, const int64_t* p_indptr, const int32_t* p_indices, const float* p_vals,
                                const int64_t* q_indptr, const int32_t* q_indices, const float* q_vals, int64_t n, int64_t n_other,
                                int32_t n_neighbors, int sim, int64_t* w_indptr, int32_t* w_indices, float* w_vals, void* ws,
                                size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    return knn_build<double>("el_knn_build_f32", "k_knn_norms_f32", "k_knn_topn_f32", stream, p_indptr, p_indices, p_vals, q_indptr,
                             q_indices, q_vals, n, n_other, n_neighbors, sim, 1.0, w_indptr, w_indices, w_vals, ws, ws_bytes);
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
    const size_t lds = (size_t)p.cap * 8 + (size_t)p.tile * 4;
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    EL_LAUNCH("k_knn_score", k_knn_score, dim3((unsigned)(u_stop - u_start)), dim3(64), lds, (hipStream_t)stream, p);
    EL_CHECK_LAUNCH();
    return 0;
}
