// Per-sample BPR SGD in fp64 for WIDE rows (KaHFM: one factor per knowledge-graph feature, hundreds to thousands).
//
//   k_bprsgd_apply_wide   the update of k_bprsgd_apply (el_bpr.hip), line for line, with one workgroup of 256 lanes per triplet
//
// Reached from launch_bprsgd (el_bpr.hip) only for the shapes k_bprsgd_apply cannot hold in the registers of 64 lanes x 4 pieces;
// every shape that kernel accepts keeps it.
//
// Numerics contract:
//   piece   VW doubles (2 = one 16-byte access when F is even and both tables are 16-byte aligned, else 1); piece k of a row
//           belongs to lane k mod 256 and is that lane's piece number k / 256
//   dot     every lane adds its products in ascending piece order from +0 (mul, then add: no contraction); the 64 lane sums of
//           a wave go through the xor shuffle tree (32, 16, ..., 1), the four wave sums are added in wave order
//           ((w0 + w1) + w2) + w3 by every lane from LDS.  A fixed shape: the same input gives the same bytes on every run.
//   update  user row first, item rows from the UPDATED user row, the two biases by lane 0 -- as k_bprsgd_apply
// CPL >= 1: a lane keeps its CPL pieces of the three rows in registers between the two passes (F <= 256 * CPL * VW, CPL <= 8).
// CPL == 0: any F; the update pass reads the rows again (every element is read and written by the same lane).
// No float atomics.  No lane touches an element at or beyond F of a row.
#include "el_common.h"

#define WIDE_THREADS 256
#define WIDE_MAX_CPL 8

namespace {

template <int VW>
__device__ __forceinline__ void ld_piece(const double* p, double* dst) {
    if (VW == 2) {
        double2 t = *reinterpret_cast<const double2*>(p);
        dst[0] = t.x;
        dst[1] = t.y;
    } else {
        dst[0] = p[0];
    }
}
template <int VW>
__device__ __forceinline__ void st_piece(double* p, const double* src) {
    if (VW == 2) {
        *reinterpret_cast<double2*>(p) = make_double2(src[0], src[1]);
    } else {
        p[0] = src[0];
    }
}

// the sums of `a` and `b` over the workgroup in the fixed shape of the contract, in every lane; `slot` holds 2 x 4 doubles
__device__ __forceinline__ void wide_block_sum2(double& a, double& b, double (*slot)[4]) {
    a = el_group_sum(a, 64);
    b = el_group_sum(b, 64);
    if ((threadIdx.x & 63) == 0) {
        slot[0][threadIdx.x >> 6] = a;
        slot[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = ((slot[0][0] + slot[0][1]) + slot[0][2]) + slot[0][3];
    b = ((slot[1][0] + slot[1][1]) + slot[1][2]) + slot[1][3];
}

template <int VW>
__device__ __forceinline__ void wide_update(const el_bprsgd_state& st, double z, const double* vu, const double* vi, const double* vj,
                                            double* nu, double* ni, double* nj) {
    const double lr = st.lr;
#pragma unroll
    for (int x = 0; x < VW; ++x) {
        nu[x] = vu[x] + lr * ((vi[x] - vj[x]) * z - st.reg_user * vu[x]);      // BPRMF_model.py:108-109 / kahfm_model.py:151-152
        ni[x] = vi[x] + lr * (nu[x] * z - st.reg_pos * vi[x]);                  // :112-113 / :156-157: the UPDATED user row
        nj[x] = vj[x] + lr * (-nu[x] * z - st.reg_neg * vj[x]);                 // :116-117 / :161-162
    }
}

template <int VW, int CPL>
__global__ __launch_bounds__(WIDE_THREADS) void k_bprsgd_apply_wide(el_bprsgd_state st, const int32_t* __restrict__ bu,
                                                                    const int32_t* __restrict__ bi_, const int32_t* __restrict__ bj,
                                                                    int64_t first) {
    __shared__ double s_dot[2][4];
    const int F = st.F;
    const int tid = threadIdx.x;
    const int64_t t = first + blockIdx.x;
    const int32_t uu = bu[t], ii = bi_[t], jj = bj[t];
    double* pu = st.P + (int64_t)uu * F;
    double* qi = st.Q + (int64_t)ii * F;
    double* qj = st.Q + (int64_t)jj * F;
    constexpr int NREG = CPL > 0 ? CPL : 1;
    double vu[NREG][VW], vi[NREG][VW], vj[NREG][VW];
    double di = 0.0, dj = 0.0;
    if (CPL > 0) {
#pragma unroll
        for (int q = 0; q < NREG; ++q) {
            const int e = (tid + q * WIDE_THREADS) * VW;
#pragma unroll
            for (int x = 0; x < VW; ++x) vu[q][x] = vi[q][x] = vj[q][x] = 0.0;
            if (e < F) {
                ld_piece<VW>(pu + e, vu[q]);
                ld_piece<VW>(qi + e, vi[q]);
                ld_piece<VW>(qj + e, vj[q]);
            }
#pragma unroll
            for (int x = 0; x < VW; ++x) {
                di += vu[q][x] * vi[q][x];
                dj += vu[q][x] * vj[q][x];
            }
        }
    } else {
        for (int e = tid * VW; e < F; e += WIDE_THREADS * VW) {
            ld_piece<VW>(pu + e, vu[0]);
            ld_piece<VW>(qi + e, vi[0]);
            ld_piece<VW>(qj + e, vj[0]);
#pragma unroll
            for (int x = 0; x < VW; ++x) {
                di += vu[0][x] * vi[0][x];
                dj += vu[0][x] * vj[0][x];
            }
        }
    }
    wide_block_sum2(di, dj, s_dot);
    const double b_i = st.b[ii], b_j = st.b[jj];
    // z = 1/(1+exp(x_ui - x_uj)), x = global_bias(0) + b + p.q
    const double xui = (0.0 + b_i) + di, xuj = (0.0 + b_j) + dj;
    const double z = 1.0 / (1.0 + exp(xui - xuj));
    __syncthreads();                                            // every wave has read both biases before lane 0 writes them
    if (tid == 0) {
        st.b[ii] = b_i + st.lr * (z - st.reg_bias * b_i);
        st.b[jj] = b_j + st.lr * (-z - st.reg_bias * b_j);
    }
    double nu[VW], ni[VW], nj[VW];
    if (CPL > 0) {
#pragma unroll
        for (int q = 0; q < NREG; ++q) {
            const int e = (tid + q * WIDE_THREADS) * VW;
            if (e < F) {
                wide_update<VW>(st, z, vu[q], vi[q], vj[q], nu, ni, nj);
                st_piece<VW>(pu + e, nu);
                st_piece<VW>(qi + e, ni);
                st_piece<VW>(qj + e, nj);
            }
        }
    } else {
        for (int e = tid * VW; e < F; e += WIDE_THREADS * VW) {
            ld_piece<VW>(pu + e, vu[0]);
            ld_piece<VW>(qi + e, vi[0]);
            ld_piece<VW>(qj + e, vj[0]);
            wide_update<VW>(st, z, vu[0], vi[0], vj[0], nu, ni, nj);
            st_piece<VW>(pu + e, nu);
            st_piece<VW>(qi + e, ni);
            st_piece<VW>(qj + e, nj);
        }
    }
}

}  // namespace

int el_bprsgd_launch_wide(const el_bprsgd_state& st, const int32_t* u, const int32_t* i, const int32_t* j, int64_t first,
                          int64_t n, hipStream_t s) {
    EL_REQUIRE(n >= 1 && n < 0x7fffffffLL, "el_bprsgd_apply: %lld triplets in one call unsupported", (long long)n);
    const bool vec = (st.F % 2 == 0) && (((uintptr_t)st.P) % 16 == 0) && (((uintptr_t)st.Q) % 16 == 0);
    const int vw = vec ? 2 : 1;
    const int pieces = (st.F + vw - 1) / vw;
    int cpl = 1;
    while (cpl * WIDE_THREADS < pieces) cpl <<= 1;
    if (cpl > WIDE_MAX_CPL) cpl = 0;                            // the two-pass loop
    const dim3 grid((unsigned)n), block(WIDE_THREADS);
#define EL_WIDE_LAUNCH(VW_, CPL_) \
    EL_LAUNCH("k_bprsgd_apply_wide", (k_bprsgd_apply_wide<VW_, CPL_>), grid, block, 0, s, st, u, i, j, first)
    if (vec) {
        if (cpl == 1) EL_WIDE_LAUNCH(2, 1);
        else if (cpl == 2) EL_WIDE_LAUNCH(2, 2);
        else if (cpl == 4) EL_WIDE_LAUNCH(2, 4);
        else if (cpl == 8) EL_WIDE_LAUNCH(2, 8);
        else EL_WIDE_LAUNCH(2, 0);
    } else {
        if (cpl == 1) EL_WIDE_LAUNCH(1, 1);
        else if (cpl == 2) EL_WIDE_LAUNCH(1, 2);
        else if (cpl == 4) EL_WIDE_LAUNCH(1, 4);
        else if (cpl == 8) EL_WIDE_LAUNCH(1, 8);
        else EL_WIDE_LAUNCH(1, 0);
    }
#undef EL_WIDE_LAUNCH
    EL_CHECK_LAUNCH();
    return 0;
}
