// Per-column neighbour lists -> W as CSR with ascending columns: shared by el_knn.hip (ItemKNN / UserKNN), el_slim.hip (SLIM)
// and el_rp3.hip (RP3beta, which also uses scan + place as its counting sort by column).
//   lists     lx / lv [n, N] with lcnt[c] entries for target column c, rowcnt[x] = entries that name row x
//   k_knn_count  rowcnt of finished lists (a kernel that writes its lists may count as it goes instead)
//   k_knn_scan   rowcnt -> indptr, cursor
//   k_knn_place  every list entry to its row (arbitrary order inside the row)
//   k_knn_rank   orders each row by column
//   el_knn_csr_launch  scan, place and rank on the workspace of el_knn_csr_carve
#pragma once
#include "el_common.h"

#define KNN_RANK_WORDS 2048                       // transpose: presence bitmap of 2048 * 32 targets per pass

namespace {

// entries of the lists per row of W (integer atomics: any order, the same counts)
__global__ __launch_bounds__(256) void k_knn_count(const int32_t* __restrict__ lx, const int32_t* __restrict__ lcnt, int64_t n,
                                                   int N, int32_t* __restrict__ rowcnt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * N) return;
    const int64_t c = e / N;
    if ((int)(e - c * N) >= lcnt[c]) return;
    atomicAdd(&rowcnt[lx[e]], 1);
}

// indptr[0] = 0, indptr[x + 1] = sum rowcnt[0 .. x]; cursor[x] = indptr[x].  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void k_knn_scan(const int32_t* __restrict__ rowcnt, int64_t n, int64_t* __restrict__ indptr,
                                                   int64_t* __restrict__ cursor) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (int64_t x = lo; x < hi; ++x) s += rowcnt[x];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        int64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - s;                          // exclusive prefix of this thread's chunk
    for (int64_t x = lo; x < hi; ++x) {
        indptr[x] = run;
        cursor[x] = run;
        run += rowcnt[x];
    }
    if (tid == 1023) indptr[n] = part[1023];
}

// entries of every list to their row of W (arbitrary order inside the row; k_knn_rank orders it)
__global__ __launch_bounds__(256) void k_knn_place(const int32_t* __restrict__ lx, const float* __restrict__ lv,
                                                   const int32_t* __restrict__ lcnt, int64_t n, int N, int64_t* __restrict__ cursor,
                                                   int32_t* __restrict__ tc, float* __restrict__ tv) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * N) return;
    const int64_t c = e / N;
    const int j = (int)(e - c * N);
    if (j >= lcnt[c]) return;
    const int32_t x = lx[e];
    const int64_t pos = (int64_t)atomicAdd(reinterpret_cast<unsigned long long*>(&cursor[x]), 1ull);
    tc[pos] = (int32_t)c;
    tv[pos] = lv[e];
}

// One workgroup per row x of W: the targets of the row are distinct, so the rank of c in the row is the number of set bits
// below c in a presence bitmap (built with LDS atomicOr, ranked with a block scan of popcounts).  Rows ascending in c.
__global__ __launch_bounds__(256) void k_knn_rank(const int64_t* __restrict__ indptr, const int32_t* __restrict__ tc,
                                                  const float* __restrict__ tv, int64_t n, int32_t* __restrict__ wi,
                                                  float* __restrict__ wv) {
    __shared__ u32 bits[KNN_RANK_WORDS];
    __shared__ int32_t pre[KNN_RANK_WORDS];
    __shared__ int32_t part[256];
    const int tid = threadIdx.x;
    const int64_t x = blockIdx.x;
    const int64_t r0 = indptr[x], r1 = indptr[x + 1];
    if (r1 == r0) return;
    const int64_t span = (int64_t)KNN_RANK_WORDS * 32;
    int64_t base = 0;
    for (int64_t c0 = 0; c0 < n; c0 += span) {
        const int64_t c1 = c0 + span < n ? c0 + span : n;
        const int nwd = (int)((c1 - c0 + 31) >> 5);
        for (int w = tid; w < nwd; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int64_t e = r0 + tid; e < r1; e += 256) {
            const int64_t c = tc[e];
            if (c >= c0 && c < c1) atomicOr(&bits[(c - c0) >> 5], 1u << ((c - c0) & 31));
        }
        __syncthreads();
        const int per = (nwd + 255) / 256;
        const int w0 = tid * per < nwd ? tid * per : nwd, w1 = w0 + per < nwd ? w0 + per : nwd;
        int s = 0;
        for (int w = w0; w < w1; ++w) s += __popc(bits[w]);
        part[tid] = s;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            int v = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        int run = part[tid] - s;
        for (int w = w0; w < w1; ++w) {
            pre[w] = run;
            run += __popc(bits[w]);
        }
        const int total = part[255];
        __syncthreads();
        for (int64_t e = r0 + tid; e < r1; e += 256) {
            const int64_t c = tc[e];
            if (c >= c0 && c < c1) {
                const int w = (int)((c - c0) >> 5), b = (int)((c - c0) & 31);
                const int64_t pos = r0 + base + pre[w] + __popc(bits[w] & ((1u << b) - 1u));
                wi[pos] = (int32_t)c;
                wv[pos] = tv[e];
            }
        }
        base += total;
        __syncthreads();
    }
}

// what scan / place / rank need beside the lists and W: the rows' cursors and the placed, not yet ordered entries
struct KnnCsrWs {
    int64_t* cursor;     // [n]
    int32_t* tc;         // [n, N]
    float* tv;           // [n, N]
};

// the only description of that workspace; callers nest it at the end of their own layout
KnnCsrWs el_knn_csr_carve(ElCarve& a, int64_t n, int N) {
    KnnCsrWs c;
    c.cursor = a.take<int64_t>((size_t)n);
    c.tc = a.take<int32_t>((size_t)n * N);
    c.tv = a.take<float>((size_t)n * N);
    return c;
}

// lists + filled rowcnt -> W (w_indptr [n + 1], w_indices / w_vals [n * N]); c: el_knn_csr_carve(.., n, N)
int el_knn_csr_launch(hipStream_t st, const int32_t* lx, const float* lv, const int32_t* lcnt, int64_t n, int N,
                      const int32_t* rowcnt, int64_t* w_indptr, int32_t* w_indices, float* w_vals, const KnnCsrWs& c) {
    EL_LAUNCH("k_knn_scan", k_knn_scan, dim3(1), dim3(1024), 0, st, rowcnt, n, w_indptr, c.cursor);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_knn_place", k_knn_place, dim3((unsigned)((n * N + 255) / 256)), dim3(256), 0, st, lx, lv, lcnt, n, N, c.cursor, c.tc,
              c.tv);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_knn_rank", k_knn_rank, dim3((unsigned)n), dim3(256), 0, st, (const int64_t*)w_indptr, (const int32_t*)c.tc,
              (const float*)c.tv, n, w_indices, w_vals);
    EL_CHECK_LAUNCH();
    return 0;
}

}  // namespace
