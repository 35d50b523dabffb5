// Running top-N of one workgroup in LDS, shared by the two similarity builders (el_knn.hip: integer counts, el_attr.hip: fp64
// sums of float rows): keys (el_make_key: value desc, index asc) are appended to keys[0 .. cap) and cut back to the best N
// whenever fewer than one pass of the workgroup fits behind them.
#pragma once
#include "el_common.h"

#define KNN_BUILD_THREADS 256
#define KNN_MAX_NEIGHBORS 2048                    // running top-N lives in LDS next to the tile

namespace {

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

}  // namespace
