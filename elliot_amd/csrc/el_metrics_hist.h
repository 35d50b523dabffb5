// Item histogram of recommendation lists, shared by the beyond-accuracy metrics (el_metrics_beyond.hip: the lists of the users with a
// held-out row) and the fairness metrics (el_metrics_fair.hip: the lists of the users with a relevant held-out item).
//
// One popular item can sit in most lists of a block, and adds on one word serialise.  k_beyond_hist therefore sorts a tile of BEY_TILE
// list entries in LDS and issues one add per DISTINCT id of the tile (guideline: aggregate inside the workgroup before touching memory).
//   BY_FLAG false: the users whose row of the held-out CSR `tp` is non-empty
//   BY_FLAG true:  the users whose flag[row * flag_ld] is non-zero (a column of per-user fp64 rows)
#pragma once
#include "el_common.h"

#define BEY_TILE 2048

template <bool BY_FLAG>
__global__ __launch_bounds__(256) void k_beyond_hist(const int32_t* __restrict__ rec, int64_t ld, int64_t u_start, int64_t n,
                                                     const int64_t* __restrict__ tp, const double* __restrict__ flag, int flag_ld,
                                                     int cutoff, int32_t I, int32_t* __restrict__ hist) {
    __shared__ u32 key[BEY_TILE];
    const int64_t e0 = (int64_t)blockIdx.x * BEY_TILE, total = n * cutoff;
    const int64_t row0 = e0 / cutoff;
    const u32 rem0 = (u32)(e0 - row0 * cutoff);
    for (int t = threadIdx.x; t < BEY_TILE; t += 256) {
        u32 k = 0xffffffffu;
        if (e0 + t < total) {
            const u32 x = rem0 + (u32)t;
            const int64_t row = row0 + x / (u32)cutoff;
            const u32 col = x % (u32)cutoff;
            const int64_t user = u_start + row;
            if (BY_FLAG ? flag[row * flag_ld] != 0.0 : tp[user + 1] > tp[user]) {
                const int32_t item = rec[row * ld + col];
                if (item >= 0 && item < I) k = (u32)item;
            }
        }
        key[t] = k;
    }
    __syncthreads();
    for (int size = 2; size <= BEY_TILE; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (BEY_TILE >> 1); t += 256) {
                const int i = 2 * t - (t & (stride - 1));
                const int j = i + stride;
                const bool asc = ((i & size) == 0);
                const u32 x = key[i], y = key[j];
                if (asc ? (x > y) : (x < y)) {
                    key[i] = y;
                    key[j] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < BEY_TILE; t += 256) {
        const u32 k = key[t];
        if (k != 0xffffffffu && (t == 0 || key[t - 1] != k)) {
            int lo = t + 1, hi = BEY_TILE;                    // first position behind the run of k
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key[mid] <= k)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            atomicAdd(hist + k, lo - t);
        }
    }
}
