// The ordered row scorer and the fp64 tile transpose that EASE^R, SlopeOne and BPRSlim share (el_ease.hip, el_slope.hip,
// el_bprslim.hip).
//
// k_row_scores   out[u, c] = finish(chain over row u of the CSR, in stored order, of step(table[column, c])): one user per
//                blockIdx.x (the fastest-dispatched index: workgroups in flight share one slab of the table), EL_ROW_SLAB
//                targets per blockIdx.y, lanes across targets.  Every target's chain is sequential: the bits depend on the row's
//                stored order alone.
// k_transpose_f64  dst[j, i] = load(i, j) by EL_TR x EL_TR tiles through LDS
#pragma once
#include "el_common.h"

#define EL_ROW_SLAB 1024         // targets per workgroup of k_row_scores
#define EL_TR 32                 // k_transpose_f64 moves EL_TR x EL_TR tiles

namespace {

// What a model's Op (passed by value) says about its chain; it inherits these and names only what differs.
template <class T_>
struct RowScoreOp {
    typedef T_ T, Acc;                                            // the table's and output's type; a target's state, from zero
    const T_* table;
    int64_t ld;
    static constexpr bool CHECK_COLS = false;                     // skip a column outside [0, I) (no row of the table) or trust it
    __device__ int weight(int64_t) const { return 0; }            // what entry e brings besides its column, read once per entry
    // step(a, w, x): one link of the chain, table cell x under the entry's weight w -- every Op has its own
    __device__ int base(int64_t) const { return 0; }              // what the finish needs of user u, read once behind the chain
    __device__ T_ finish(const T_& a, int) const { return a; }    // the value stored
};

template <class Op>
__global__ __launch_bounds__(256) void k_row_scores(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                    int64_t u_start, Op op, int64_t I, typename Op::T* __restrict__ out,
                                                    int64_t ld_out) {
    constexpr int Q = EL_ROW_SLAB / 256;
    const int64_t u = u_start + blockIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * EL_ROW_SLAB + threadIdx.x;
    const int64_t e0 = indptr[u], e1 = indptr[u + 1];
    typename Op::Acc acc[Q] = {};
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t s = indices[e];
        if (Op::CHECK_COLS && (s < 0 || s >= I)) continue;
        const auto w = op.weight(e);
        const typename Op::T* t = op.table + s * op.ld;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int64_t c = c0 + 256 * q;
            if (c < I) op.step(acc[q], w, t[c]);
        }
    }
    const auto b = op.base(u);
    typename Op::T* o = out + (int64_t)blockIdx.x * ld_out;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int64_t c = c0 + 256 * q;
        if (c < I) o[c] = op.finish(acc[q], b);
    }
}

// The checks and the grid of k_row_scores for the entry point `who`; ptrs: no pointer of the call is null.
template <class Op>
int el_row_scores(const char* who, const char* label, el_ctx* ctx, void* stream, bool ptrs, const int64_t* indptr,
                  const int32_t* indices, int64_t u_start, int64_t u_stop, const Op& op, int64_t I, typename Op::T* out,
                  int64_t ld_out) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(ptrs, "%s: null pointer", who);
    EL_REQUIRE(u_start >= 0 && u_stop >= u_start && u_stop - u_start < 0x7fffffffLL, "%s: bad user range", who);
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && (I + EL_ROW_SLAB - 1) / EL_ROW_SLAB < 65536, "%s: bad item count %lld", who,
               (long long)I);
    EL_REQUIRE(op.ld >= I && ld_out >= I, "%s: leading dimensions below I", who);
    if (u_stop == u_start) return 0;
    EL_LAUNCH(label, k_row_scores<Op>, dim3((unsigned)(u_stop - u_start), (unsigned)((I + EL_ROW_SLAB - 1) / EL_ROW_SLAB)),
              dim3(256), 0, (hipStream_t)stream, indptr, indices, u_start, op, I, out, ld_out);
    EL_CHECK_LAUNCH();
    return 0;
}

template <class Load>
__global__ __launch_bounds__(EL_TR * 8) void k_transpose_f64(Load load, int64_t I, double* __restrict__ dst, int64_t ldd) {
    __shared__ double tile[EL_TR][EL_TR + 1];
    const int tx = threadIdx.x % EL_TR, ty = threadIdx.x / EL_TR;
    const int64_t i0 = (int64_t)blockIdx.y * EL_TR, j0 = (int64_t)blockIdx.x * EL_TR;
    for (int r = ty; r < EL_TR; r += 8) {
        const int64_t i = i0 + r, j = j0 + tx;
        if (i < I && j < I) tile[r][tx] = load(i, j);
    }
    __syncthreads();
    for (int r = ty; r < EL_TR; r += 8) {
        const int64_t j = j0 + r, i = i0 + tx;
        if (i < I && j < I) dst[j * ldd + i] = tile[tx][r];
    }
}

// The checks and the grid of k_transpose_f64 for the entry point `who`; ptrs / lds: no null pointer, every leading dimension >= I.
template <class Load>
int el_transpose_f64(const char* who, const char* label, el_ctx* ctx, void* stream, bool ptrs, bool lds, const Load& load,
                     int64_t I, double* dst, int64_t ldd) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(ptrs, "%s: null pointer", who);
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && (I + EL_TR - 1) / EL_TR < 65536, "%s: bad item count %lld", who, (long long)I);
    EL_REQUIRE(lds, "%s: leading dimensions below I", who);
    const unsigned nt = (unsigned)((I + EL_TR - 1) / EL_TR);
    EL_LAUNCH(label, k_transpose_f64<Load>, dim3(nt, nt), dim3(EL_TR * 8), 0, (hipStream_t)stream, load, I, dst, ldd);
    EL_CHECK_LAUNCH();
    return 0;
}

}  // namespace
