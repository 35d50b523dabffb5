// RP3beta (random walk of length three with popularity penalty; P3alpha is beta = 0).
//
// Replaces RP3beta.train of the reference (rp3beta.py:77-174); the scores and lists are el_knn_score_topk(A = R, B = W):
//   el_csr_row_l1  sklearn's normalize(., 'l1') of a CSR (Pui, Piu, normalize_similarity)
//   el_rp3_rows    S = Piu * Pui fused with the row cut: nothing I x I is written
//   el_rp3_cut     optional row-l1 of the row lists, the column cut, W as CSR with ascending columns
//
// Numerics contract (tests/helpers/rp3_ref.py restates it in NumPy):
//   row-l1   s = sum |x| in fp64, sequentially in stored order; x <- (float)((double)x / s); rows with s == 0 left alone
//   S[i, j]  = __fadd_rn(acc, __fmul_rn(Piu[i, u], Pui[u, j])) over the users of Piu row i IN ASCENDING ORDER, from +0
//              (scipy csr_matmat).  The terms are float32 transition probabilities, so the integer LDS atomics that make
//              k_knn_topn exact in any order do not apply: the order is kept by giving every (row, column slice) ONE wave
//              that walks the row's users in order; the parallelism is across columns (and rows), never across users.
//   row cut  v = (double)S[i, j] * degree[j] (one fp64 multiply), v[i] = 0; the N largest of the whole row by
//            (v desc, j asc) with the zeros dropped, stored as (float)v.  The selection key is ord(double) with the index
//            carried beside it: two doubles that round to the same float still rank by their fp64 value.
//   col cut  per column the N largest non-zero floats by (value desc, row asc)
// Deterministic: the same input gives the same bytes.  No float atomics.
#include "el_common.h"

#include "el_knn_csr.h"
#include "el_topk_common.h"

#define RP3_MAX_NEIGHBORS 2048                    // as KNN_MAX_NEIGHBORS: running top-N lives in LDS next to the tile
#define RP3_TILE 4096                             // float accumulators of one column slice (16 KiB of LDS per wave)
#define RP3_MIN_SLICE 256                         // a narrow catalogue is still cut into up to RP3_SPREAD slices of
#define RP3_SPREAD 8                              // at least this width, so that one long row occupies several CUs

namespace {

__global__ __launch_bounds__(256) void k_rp3_row_l1(const int64_t* __restrict__ indptr, const float* __restrict__ x, int64_t n,
                                                    float* __restrict__ y) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t e0 = indptr[r], e1 = indptr[r + 1];
    double s = 0.0;
    for (int64_t e = e0; e < e1; ++e) s = __dadd_rn(s, fabs((double)x[e]));
    if (s == 0.0) {
        for (int64_t e = e0; e < e1; ++e) y[e] = x[e];
        return;
    }
    for (int64_t e = e0; e < e1; ++e) y[e] = (float)__ddiv_rn((double)x[e], s);
}

// The row cut's running selection: ord(double) keys with the column beside them, larger key first, then smaller column
// (a key of a value that is not a negative NaN is never 0, the empty slot's).
typedef ElWaveSelect<ElPairKey<u64>> Rp3Select;

struct Rp3Rows {
    const int64_t* pp;   // Piu: item -> its users ascending
    const int32_t* pi;
    const float* pv;
    const int64_t* qp;   // Pui: user -> items ascending
    const int32_t* qi;
    const float* qv;
    const double* deg;   // [I]
    int64_t I, i_start;
    int N;               // entries kept per row (<= I)
    int S;               // column slices
    int width;           // columns per slice (<= RP3_TILE, multiple of 64)
    int cap;             // running-selection slots (power of two >= N + 64)
    u64* sk;             // [rows, S, N] keys of the slices' lists
    int32_t* sx;         // [rows, S, N] their columns
    int32_t* sc;         // [rows, S, 4] kept, non-zeros, positives
};

// One wave per (row i, column slice): walk the users of Piu row i in order; 64 users' (value, slice of their Pui row) are
// fetched at a time, one user per lane (the chain pi[a] -> qp[u] -> binary search in qi is three or more dependent loads), and
// broadcast; the first 64 entries of the next user's slice are loaded before the current user's are added, so the walk does
// not pay a memory round trip per user.  Lanes over the user's columns: the columns of one user are distinct, the wave's LDS
// accesses are served in program order, so every column sees its terms in user order.
__global__ __launch_bounds__(64) void k_rp3_slice(Rp3Rows p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* acc = reinterpret_cast<float*>(smem + (size_t)p.cap * 12);                  // [width], behind the selection's [cap] pairs
    const int lane = threadIdx.x;
    const int64_t rrel = blockIdx.x;
    const int64_t i = p.i_start + rrel;
    const int s = blockIdx.y;
    const int64_t c0 = (int64_t)s * p.width;
    const int64_t c1 = c0 + p.width < p.I ? c0 + p.width : p.I;
    const int w = (int)(c1 - c0);
    const bool sliced = p.S > 1;
    for (int t = lane; t < w; t += 64) acc[t] = 0.f;
    el_wave_lds_sync();
    const int64_t a0 = p.pp[i], a1 = p.pp[i + 1];
    for (int64_t ab = a0; ab < a1; ab += 64) {
        const int m = (int)(a1 - ab < 64 ? a1 - ab : 64);
        float x = 0.f;
        int64_t q0 = 0, q1 = 0;
        if (lane < m) {
            const int32_t u = p.pi[ab + lane];
            x = p.pv[ab + lane];
            q0 = p.qp[u], q1 = p.qp[u + 1];
            if (sliced) {
                q0 = el_lower_bound(p.qi, q0, q1, (int32_t)c0);
                q1 = el_lower_bound(p.qi, q0, q1, (int32_t)c1);
            }
        }
        int32_t nj = 0;
        float nb = 0.f;
        {
            const int64_t f = __shfl(q0, 0, 64) + lane;
            if (f < __shfl(q1, 0, 64)) nj = p.qi[f], nb = p.qv[f];
        }
        for (int t = 0; t < m; ++t) {
            const float xt = __shfl(x, t, 64);
            const int64_t t0 = __shfl(q0, t, 64), t1 = __shfl(q1, t, 64);
            const int32_t cj = nj;
            const float cb = nb;
            if (t + 1 < m) {
                const int64_t f = __shfl(q0, t + 1, 64) + lane;
                if (f < __shfl(q1, t + 1, 64)) nj = p.qi[f], nb = p.qv[f];
            }
            if (t0 + lane < t1) {
                float* d = &acc[cj - c0];
                *d = __fadd_rn(*d, __fmul_rn(xt, cb));
            }
            for (int64_t f = t0 + 64 + lane; f < t1; f += 64) {
                float* d = &acc[p.qi[f] - c0];
                *d = __fadd_rn(*d, __fmul_rn(xt, p.qv[f]));
            }
            el_wave_lds_sync();
        }
    }
    // the slice's N best non-zeros of v = (double)S * degree, and how many non-zeros / positives it holds
    int n_nz = 0, n_pos = 0;
    Rp3Select sel(ElPairKey<u64>(smem, p.cap), p.cap, p.N);
    for (int base = 0; base < w; base += 64) {
        const int pos = base + lane;
        bool nz = false, hit = false;
        u64 key = 0ull;
        double v = 0.0;
        if (pos < w) {
            const float sv = acc[pos];
            if (sv != 0.f && c0 + pos != i) {
                v = __dmul_rn((double)sv, p.deg[c0 + pos]);
                nz = v != 0.0;
                key = el_d2ord(v);
                hit = nz && key >= sel.tau;
            }
        }
        n_nz += __popcll(__ballot(nz));
        n_pos += __popcll(__ballot(nz && v > 0.0));
        sel.push(hit, key, (int32_t)(c0 + pos), lane);
    }
    const int m = sel.finish(lane);
    const int64_t slot = rrel * p.S + s;
    for (int t = lane; t < m; t += 64) {
        p.sk[slot * p.N + t] = sel.keys.value(t);
        p.sx[slot * p.N + t] = sel.keys.index(t);
    }
    if (lane == 0) {
        p.sc[slot * 4 + 0] = m;
        p.sc[slot * 4 + 1] = n_nz;
        p.sc[slot * 4 + 2] = n_pos;
        p.sc[slot * 4 + 3] = 0;
    }
}

// One wave per row: the slices' lists merged by the same key.  The whole row ranks positives, then its zeros (never stored),
// then negatives: with P positives and Z zeros the row keeps min(N, P) positives and max(0, N - P - Z) negatives.
__global__ __launch_bounds__(64) void k_rp3_merge(Rp3Rows p, int32_t* __restrict__ lx, float* __restrict__ lv, int32_t* __restrict__ lcnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int64_t rrel = blockIdx.x;
    Rp3Select sel(ElPairKey<u64>(smem, p.cap), p.cap, p.N);
    int64_t n_nz = 0, n_pos = 0;
    for (int s = 0; s < p.S; ++s) {
        const int64_t slot = rrel * p.S + s;
        const int m = p.sc[slot * 4 + 0];
        n_nz += p.sc[slot * 4 + 1];
        n_pos += p.sc[slot * 4 + 2];
        for (int base = 0; base < m; base += 64) {             // the lanes that hold an entry are a prefix of the wave
            const int t = base + lane;
            const bool has = t < m;
            sel.push(has, has ? p.sk[slot * p.N + t] : 0ull, has ? p.sx[slot * p.N + t] : 0, lane);
        }
    }
    const int m = sel.finish(lane);                            // the N best non-zeros: positives first
    const int64_t zeros = p.I - n_nz;
    const int take_pos = (int)(n_pos < p.N ? n_pos : p.N);
    int64_t take_neg = n_pos < p.N ? (int64_t)p.N - n_pos - zeros : 0;
    if (take_neg < 0) take_neg = 0;
    if (take_neg > m - take_pos) take_neg = m - take_pos;
    const int out = take_pos + (int)take_neg;
    for (int t = lane; t < out; t += 64) {
        lx[rrel * p.N + t] = sel.keys.index(t);
        lv[rrel * p.N + t] = (float)el_ord2d(sel.keys.value(t));
    }
    if (lane == 0) lcnt[rrel] = out;
}

// normalize_similarity: one wave per row list; the entries are ordered by column (the COO -> CSR conversion of the reference),
// lane 0 takes the fp64 sum in that order, every entry is divided.  lv -> ln, the list order is kept.
__global__ __launch_bounds__(64) void k_rp3_list_l1(const int32_t* __restrict__ lx, const float* __restrict__ lv,
                                                    const int32_t* __restrict__ lcnt, int N, int cap, float* __restrict__ ln) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                                          // [cap]
    double* sum = reinterpret_cast<double*>(smem + (size_t)cap * 8);
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int m = lcnt[r];
    if (m == 0) return;
    for (int t = lane; t < cap; t += 64)                       // descending in ~column = ascending in column; empty slots last
        keys[t] = t < m ? ((u64)(0xffffffffu - (u32)lx[r * N + t]) << 32) | (u64)__float_as_uint(lv[r * N + t]) : 0ull;
    el_wave_lds_sync();
    el_wave_bitonic_desc(keys, cap, lane);
    if (lane == 0) {
        double s = 0.0;
        for (int t = 0; t < m; ++t) s = __dadd_rn(s, fabs((double)__uint_as_float((u32)keys[t])));
        *sum = s;
    }
    el_wave_lds_sync();
    const double s = *sum;
    for (int t = lane; t < m; t += 64) {
        const float x = lv[r * N + t];
        ln[r * N + t] = s == 0.0 ? x : (float)__ddiv_rn((double)x, s);
    }
}

// One wave per column j: its bucket of (row, value) in any order -> the N largest non-zero values by (value desc, row asc),
// as the per-column list k_knn_scan / k_knn_place / k_knn_rank turn into W's rows.
__global__ __launch_bounds__(64) void k_rp3_coltop(const int64_t* __restrict__ colptr, const int32_t* __restrict__ tc,
                                                   const float* __restrict__ tv, int N, int cap, int32_t* __restrict__ cx,
                                                   float* __restrict__ cv, int32_t* __restrict__ ccnt, int32_t* __restrict__ rowcnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                                          // [cap]
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int64_t e0 = colptr[j], e1 = colptr[j + 1];
    ElWaveSelect<ElPackedKey> sel(keys, cap, N);
    for (int64_t base = e0; base < e1; base += 64) {
        const int64_t e = base + lane;
        bool hit = false;
        float v = 0.f;
        int32_t r = -1;
        if (e < e1) {
            v = tv[e];
            r = tc[e];
            hit = v != 0.f && v >= sel.tau;
        }
        sel.push(hit, v, r, lane);
    }
    const int m = sel.finish(lane);
    for (int t = lane; t < m; t += 64) {
        const int32_t r = el_key_item(keys[t]);
        cx[j * N + t] = r;
        cv[j * N + t] = el_key_score(keys[t]);
        atomicAdd(&rowcnt[r], 1);
    }
    if (lane == 0) ccnt[j] = m;
}

// slices of the catalogue: as few as the tile allows, but a catalogue narrower than RP3_SPREAD tiles is still spread
void rp3_slices(int64_t I, int* S, int* width) {
    int64_t s = (I + RP3_TILE - 1) / RP3_TILE;
    int64_t spread = (I + RP3_MIN_SLICE - 1) / RP3_MIN_SLICE;
    if (spread > RP3_SPREAD) spread = RP3_SPREAD;
    if (s < spread) s = spread;
    int64_t wd = ((I + s - 1) / s + 63) / 64 * 64;
    *width = (int)wd;
    *S = (int)((I + wd - 1) / wd);
}

struct Rp3RowsWs {      // the slice lists of el_rp3_rows: Rp3Rows' sk, sx [rows, S, N] and sc [rows, S, 4]
    u64* sk;
    int32_t *sx, *sc;
};
size_t rp3_rows_carve(int64_t I, int N, int64_t n_rows, void* base, Rp3RowsWs* w) {
    int S, width;
    rp3_slices(I, &S, &width);
    const size_t slots = (size_t)n_rows * S;
    ElCarve c{(char*)base};
    w->sk = c.take<u64>(slots * N);
    w->sx = c.take<int32_t>(slots * N);
    w->sc = c.take<int32_t>(slots * 4);
    return c.off;
}

struct Rp3CutWs {
    int32_t *colcnt, *ccnt, *rowcnt;     // [I]
    int64_t* colptr;                     // [I + 1]
    float *ln, *cv;                      // [I, N] the lists' values, normalised; the per-column lists' values
    int32_t* cx;                         // [I, N] the per-column lists' rows
    KnnCsrWs b;                          // the buckets of the counting sort; el_knn_csr_launch reuses them
};

size_t rp3_cut_carve(int64_t I, int N, void* base, Rp3CutWs* w) {
    const size_t L = (size_t)I * N;
    ElCarve c{(char*)base};
    w->colcnt = c.take<int32_t>((size_t)I);
    w->ccnt = c.take<int32_t>((size_t)I);
    w->rowcnt = c.take<int32_t>((size_t)I);
    w->colptr = c.take<int64_t>((size_t)(I + 1));
    w->ln = c.take<float>(L);
    w->cx = c.take<int32_t>(L);
    w->cv = c.take<float>(L);
    w->b = el_knn_csr_carve(c, I, N);
    return c.off;
}

}  // namespace

extern "C" int el_csr_row_l1(el_ctx* ctx, void* stream, const int64_t* indptr, const float* vals, int64_t n_rows, float* out) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(indptr && vals && out, "el_csr_row_l1: null pointer");
    EL_REQUIRE(n_rows >= 0 && n_rows < 0x7fffffffLL, "el_csr_row_l1: bad row count %lld", (long long)n_rows);
    EL_REQUIRE(vals != out, "el_csr_row_l1: out of place only");
    if (n_rows == 0) return 0;
    EL_LAUNCH("k_rp3_row_l1", k_rp3_row_l1, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, indptr, vals,
              n_rows, out);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t el_rp3_ws_bytes(int64_t I, int32_t n_neighbors, int64_t n_rows) {
    if (I <= 0 || n_neighbors <= 0 || n_rows < 0) return 0;
    const int N = (int)(n_neighbors < I ? n_neighbors : I);
    Rp3RowsWs r;
    Rp3CutWs w;
    return n_rows > 0 ? rp3_rows_carve(I, N, n_rows < I ? n_rows : I, nullptr, &r) : rp3_cut_carve(I, N, nullptr, &w);
}

extern "C" int el_rp3_rows(el_ctx* ctx, void* stream, const int64_t* piu_indptr, const int32_t* piu_indices, const float* piu_vals,
                           const int64_t* pui_indptr, const int32_t* pui_indices, const float* pui_vals, const double* degree,
                           int64_t I, int64_t U, int32_t n_neighbors, int64_t i_start, int64_t i_stop, int32_t* list_idx,
                           float* list_val, int32_t* list_cnt, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(piu_indptr && piu_indices && piu_vals && pui_indptr && pui_indices && pui_vals && degree,
               "el_rp3_rows: null input pointer");
    EL_REQUIRE(list_idx && list_val && list_cnt, "el_rp3_rows: null output pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && U >= 1 && U < 0x7fffffffLL, "el_rp3_rows: bad sizes I=%lld U=%lld", (long long)I,
               (long long)U);
    EL_REQUIRE(n_neighbors >= 1, "el_rp3_rows: n_neighbors must be >= 1");
    const int N = (int)(n_neighbors < I ? n_neighbors : I);
    EL_REQUIRE(N <= RP3_MAX_NEIGHBORS, "el_rp3_rows: n_neighbors %d > %d unsupported (neighborhood -1 needs at most %d items)", N,
               RP3_MAX_NEIGHBORS, RP3_MAX_NEIGHBORS);
    EL_REQUIRE(i_start >= 0 && i_stop >= i_start && i_stop <= I, "el_rp3_rows: bad row range [%lld, %lld)", (long long)i_start,
               (long long)i_stop);
    const int64_t rows = i_stop - i_start;
    if (rows == 0) return 0;
    Rp3Rows p;
    rp3_slices(I, &p.S, &p.width);
    EL_REQUIRE(p.S <= 65535, "el_rp3_rows: %lld items need %d column slices (at most 65535)", (long long)I, p.S);
    Rp3RowsWs w;
    const size_t need = rp3_rows_carve(I, N, rows, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_rp3_rows: workspace too small (need %zu bytes)", need);
    p.pp = piu_indptr, p.pi = piu_indices, p.pv = piu_vals;
    p.qp = pui_indptr, p.qi = pui_indices, p.qv = pui_vals;
    p.deg = degree, p.I = I, p.i_start = i_start, p.N = N;
    p.sk = w.sk, p.sx = w.sx, p.sc = w.sc;
    p.cap = el_select_cap(N);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)p.cap * 12 + (size_t)p.width * 4;
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rp3_slice), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    EL_LAUNCH("k_rp3_slice", k_rp3_slice, dim3((unsigned)rows, (unsigned)p.S), dim3(64), lds, st, p);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_rp3_merge", k_rp3_merge, dim3((unsigned)rows), dim3(64), (size_t)p.cap * 12, st, p, list_idx, list_val, list_cnt);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_rp3_cut(el_ctx* ctx, void* stream, const int32_t* list_idx, const float* list_val, const int32_t* list_cnt,
                          int64_t I, int32_t n_neighbors, int normalize, int64_t* w_indptr, int32_t* w_indices, float* w_vals,
                          void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(list_idx && list_val && list_cnt, "el_rp3_cut: null input pointer");
    EL_REQUIRE(w_indptr && w_indices && w_vals, "el_rp3_cut: null output pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL, "el_rp3_cut: bad item count %lld", (long long)I);
    EL_REQUIRE(n_neighbors >= 1, "el_rp3_cut: n_neighbors must be >= 1");
    const int N = (int)(n_neighbors < I ? n_neighbors : I);
    EL_REQUIRE(N <= RP3_MAX_NEIGHBORS, "el_rp3_cut: n_neighbors %d > %d unsupported (neighborhood -1 needs at most %d items)", N,
               RP3_MAX_NEIGHBORS, RP3_MAX_NEIGHBORS);
    Rp3CutWs w;
    const size_t need = rp3_cut_carve(I, N, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_rp3_cut: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    const size_t L = (size_t)I * N;
    const int cap = el_select_cap(N);
    const unsigned eblocks = (unsigned)((L + 255) / 256);
    const float* lv = list_val;
    if (normalize) {
        const int ncap = el_pow2(N < 64 ? 64 : N);
        EL_LAUNCH("k_rp3_list_l1", k_rp3_list_l1, dim3((unsigned)I), dim3(64), (size_t)ncap * 8 + 16, st, list_idx, list_val, list_cnt,
                  N, ncap, w.ln);
        EL_CHECK_LAUNCH();
        lv = w.ln;
    }
    EL_CHECK_HIP(hipMemsetAsync(w.colcnt, 0, (size_t)I * 4, st));
    EL_CHECK_HIP(hipMemsetAsync(w.rowcnt, 0, (size_t)I * 4, st));
    EL_LAUNCH("k_knn_count", k_knn_count, dim3(eblocks), dim3(256), 0, st, list_idx, list_cnt, I, N, w.colcnt);
    EL_CHECK_LAUNCH();
    // counting sort of the row lists by column: bucket j = (row, value) of every entry in column j
    EL_LAUNCH("k_knn_scan", k_knn_scan, dim3(1), dim3(1024), 0, st, (const int32_t*)w.colcnt, I, w.colptr, w.b.cursor);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_knn_place", k_knn_place, dim3(eblocks), dim3(256), 0, st, list_idx, lv, list_cnt, I, N, w.b.cursor, w.b.tc, w.b.tv);
    EL_CHECK_LAUNCH();
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rp3_coltop), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)((size_t)cap * 8)));
    EL_LAUNCH("k_rp3_coltop", k_rp3_coltop, dim3((unsigned)I), dim3(64), (size_t)cap * 8, st, (const int64_t*)w.colptr,
              (const int32_t*)w.b.tc, (const float*)w.b.tv, N, cap, w.cx, w.cv, w.ccnt, w.rowcnt);
    EL_CHECK_LAUNCH();
    // the per-column lists to W's rows, columns ascending (the buckets are free again)
    return el_knn_csr_launch(st, w.cx, w.cv, w.ccnt, I, N, w.rowcnt, w_indptr, w_indices, w_vals, w.b);
}
