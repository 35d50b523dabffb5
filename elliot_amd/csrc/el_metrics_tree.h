// Column sums of per-user metric rows [n, W] (fp64) in a fixed shape, shared by the accuracy metrics (el_metrics.hip, W = 8), the
// beyond-accuracy metrics (el_metrics_beyond.hip, W = 18 and 1) and the rank metrics (el_rank.hip, W = 6); the fairness metrics
// (el_metrics_fair.hip) take met_groups for their grouped sums.  G workgroups x contiguous row ranges -> partial[G][W]; then one wave
// adds the G rows to the caller's sums.  The shape depends on n alone, so the same input gives the same bytes.
//   VALID >= 0: only the rows whose column VALID is non-zero are added (the accuracy metrics' "has a relevant item" flag)
//   VALID <  0: every row is added (the kernel writes zeros where a term does not count)
#pragma once
#include "el_common.h"

template <int W, int VALID>
__global__ __launch_bounds__(256) void k_metrics_partial(const double* __restrict__ rows, int64_t n, int64_t per, double* __restrict__ part) {
    __shared__ double sh[256];
    const int64_t lo = (int64_t)blockIdx.x * per, hi = (lo + per < n) ? lo + per : n;
    double acc[W];
#pragma unroll
    for (int m = 0; m < W; ++m) acc[m] = 0.0;
    for (int64_t r = lo + threadIdx.x; r < hi; r += 256) {
        if (VALID < 0 || rows[r * W + (VALID < 0 ? 0 : VALID)] != 0.0) {
#pragma unroll
            for (int m = 0; m < W; ++m) acc[m] += rows[r * W + m];
        }
    }
#pragma unroll
    for (int m = 0; m < W; ++m) {
        sh[threadIdx.x] = acc[m];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[(int64_t)blockIdx.x * W + m] = sh[0];
        __syncthreads();
    }
}

template <int W>
__global__ __launch_bounds__(64) void k_metrics_final(const double* __restrict__ part, int G, double* __restrict__ out) {
    const int m = threadIdx.x;
    if (m >= W) return;
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += part[(int64_t)g * W + m];
    out[m] += a;
}

static inline int met_groups(int64_t n) {
    int64_t g = (n + 4095) / 4096;
    return (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

// the workspace of a metric call: the n per-user rows and, straight behind them (neither block is rounded), the partial rows
struct MetWs {
    double *rows, *part;
};
static inline size_t met_carve(int64_t n, int W, void* base, MetWs* w) {
    ElCarve c{(char*)base};
    w->rows = c.take<double>((size_t)n * W, 8);
    w->part = c.take<double>((size_t)met_groups(n) * W, 8);
    return c.off;
}

// sums[0 .. W) += column sums of rows[n, W]; part = MetWs::part
template <int W, int VALID>
static inline int met_tree_sum(hipStream_t st, const double* rows, int64_t n, double* part, double* sums) {
    const int G = met_groups(n);
    const int64_t per = (n + G - 1) / G;
    EL_LAUNCH("k_metrics_partial", (k_metrics_partial<W, VALID>), dim3(G), dim3(256), 0, st, rows, n, per, part);
    EL_LAUNCH("k_metrics_final", (k_metrics_final<W>), dim3(1), dim3(64), 0, st, (const double*)part, G, sums);
    return 0;
}
