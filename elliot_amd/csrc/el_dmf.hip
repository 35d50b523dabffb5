// DMF (deep matrix factorization, Xue et al. 2017) -- contract in include/elliot_hip.h, DESIGN 3.32;
// reference: elliot/recommender/neural/DMF/deep_matrix_factorization_model.py.
//
// No embedding table: a user is their rating row R[u, :], an item its rating column R[:, i]; each goes through its own MLP (the last
// layer linear, the others ReLU) and the two outputs p, q [D] meet in a dot product or a cosine.  Tower 0 is the user tower (first
// kernel W1 [I, H1], rows of R), tower 1 the item tower (W1 [U, H1], rows of R^T).  All tower work is done once per DISTINCT row of
// the batch: el_fism_keys.h turns (u, i) into sorted keys, slots and per-slot sample runs.
//
// THE PRIMITIVE (k_dmf_cut + k_dmf_combine + k_dmf_combine_long): the rating-weighted ordered sum of gathered rows over a CSR list,
//     out[l] = sum_{k in list(l), map(index_k) >= 0} value_k * src[map(index_k)]        (list order, a double per lane, rounded once)
// cut into pieces of `fism_piece` positions exactly as el_fism.hip cuts its unweighted sum: one packed scan places the pieces, a lane
// group per piece (16 bytes per lane where H1 allows), one-piece lists finished in place, cut lists combined in piece order by a lane
// group (2 .. 16 pieces) or a workgroup (more).  Two instantiations per tower:
//   forward   lists = the batch's distinct rows (or ALL rows: el_dmf_towers), src = W1, finish: + b1, ReLU -> the first activation
//   fan-out   lists = ALL rows of the TRANSPOSED matrix, map = the row -> slot map of the batch (-1: absent), src = dz1 of the slots,
//             finish: the row of gW1 is complete in registers -- it is written out (el_dmf_grads) or W1, m, v of that row are read,
//             moved by Adam and written, once, in the same lane group (el_dmf_train_step): no [N, H1] gradient goes through HBM, and
//             a row no sample reaches takes its move with g = 0 (Keras' dense Adam moves every element every step).
// Between them: el_gemm_f32 for the inner layers on n_max = min(B, rows) slot rows (the unused slots hold zeros and add zeros; the
// last layer's forward alone is k_dmf_last, in double), the
// similarity family over [B, D] (k_dmf_colred / k_dmf_colfin: the batch-axis sums of squares and their backward coupling, two-level in
// sample order; k_dmf_sim: y, clip, loss, dy; k_dmf_dslot: dp / dq per slot as the ordered sum over the slot's samples).
// No floating-point atomics, a fixed order in every sum: the same input gives the same bytes.
#include "el_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

#define DM_STG 64            // list positions whose indices and ratings a lane group stages in LDS at once
#define DM_COMB_LONG 16      // a list of more pieces than this is combined by a workgroup
#define DM_CHUNK 256         // samples per first-level partial of a batch-axis column sum
#define DM_NORM_FLOOR 1e-12  // tf.nn.l2_normalize: x * rsqrt(max(sum x^2, 1e-12))

#include "el_fism_keys.h"

template <int VW, int CPL>
__device__ __forceinline__ void dm_ld_row(const float* row, int H, int sub, int lpt, bool ok, float (&r)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
#pragma unroll
        for (int x = 0; x < VW; ++x) r[q][x] = 0.f;
        if (ok && e < H) ldv<VW>(row + e, r[q]);
    }
}
template <int VW, int CPL>
__device__ __forceinline__ void dm_st_row(float* row, int H, int sub, int lpt, const float (&r)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
        if (e < H) stv<VW>(row + e, r[q]);
    }
}

// ---- the cut primitive --------------------------------------------------------------------------------------------------------
struct DmCut {
    const int64_t* indptr;    // the lists (CSR with values)
    const int32_t* indices;
    const float* values;
    const int32_t* ids;       // list l -> CSR row (NULL: l)
    const int32_t* map;       // index -> source row (NULL: the index itself); negative: the position is skipped
    const float* src;         // [., H]
    const u64* pstart;        // [nl + 1] exclusive scan: low word = first piece of list l, high word = its first partial row
    int64_t nl, pcap;
    int piece, H, lpt;
    float* part;              // [pcap, H]
};

// list positions [k0, k1) by ONE lane group: DM_STG mapped indices and ratings staged in LDS together, then value * row added in
// list order, four row loads in flight.  A product of two floats is exact in double; the sum is rounded once, by the caller.
template <int VW, int CPL>
__device__ __forceinline__ void dm_walk(const DmCut& c, int64_t k0, int64_t k1, int32_t* six, float* sw, int sub, double (&acc)[CPL][VW]) {
    const int lpt = c.lpt, H = c.H;
    for (int64_t base = k0; base < k1; base += DM_STG) {
        const int cs = (int)((k1 - base < DM_STG) ? k1 - base : DM_STG);
        for (int t = sub; t < cs; t += lpt) {
            const int32_t ix = c.indices[base + t];
            six[t] = c.map ? c.map[ix] : ix;
            sw[t] = c.values[base + t];
        }
        el_wave_lds_sync();
        for (int b4 = 0; b4 < cs; b4 += 4) {
            int32_t sl[4];
            float w[4], r[4][CPL][VW];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sl[k] = b4 + k < cs ? six[b4 + k] : -1;
                w[k] = b4 + k < cs ? sw[b4 + k] : 0.f;
                dm_ld_row<VW, CPL>(c.src + (int64_t)(sl[k] < 0 ? 0 : sl[k]) * H, H, sub, lpt, sl[k] >= 0, r[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (sl[k] < 0) continue;
#pragma unroll
                for (int q = 0; q < CPL; ++q)
#pragma unroll
                    for (int x = 0; x < VW; ++x) acc[q][x] += (double)w[k] * (double)r[k][q][x];
            }
        }
        el_wave_lds_sync();
    }
}

// one lane group per piece
template <int VW, int CPL, class FIN>
__global__ __launch_bounds__(256) void k_dmf_cut(DmCut c, FIN fin) {
    __shared__ int32_t s_ix[32][DM_STG];
    __shared__ float s_w[32][DM_STG];
    const int lpt = c.lpt;
    const int64_t grp = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1)), gl = (int)(threadIdx.x / lpt);
    if (grp >= fi_lo(c.pstart[c.nl])) return;
    int64_t lo = 0, hi = c.nl;                                   // the last list whose first piece is <= grp
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (fi_lo(c.pstart[mid]) <= grp) lo = mid;
        else hi = mid;
    }
    const u64 ps = c.pstart[lo];
    const int64_t k = grp - fi_lo(ps), np = fi_lo(c.pstart[lo + 1]) - fi_lo(ps), pslot = (int64_t)(ps >> 32) + k;
    if (np < 1) return;                                          // (a slot no row took)
    const int64_t row = c.ids ? c.ids[lo] : lo;
    const int64_t r0 = c.indptr[row], r1 = c.indptr[row + 1];
    const int64_t k0 = r0 + k * c.piece < r1 ? r0 + k * c.piece : r1, k1 = k0 + c.piece < r1 ? k0 + c.piece : r1;
    double accw[CPL][VW];
    float acc[CPL][VW];
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) accw[q][x] = 0.0;
    dm_walk<VW, CPL>(c, k0, k1, s_ix[gl], s_w[gl], sub, accw);
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) acc[q][x] = (float)accw[q][x];
    if (np == 1) fin(lo, row, sub, lpt, acc);
    else if (pslot < c.pcap) dm_st_row<VW, CPL>(c.part + pslot * c.H, c.H, sub, lpt, acc);
}

// partial rows [p0, p1) added in ascending order, four in flight
template <int VW, int CPL>
__device__ __forceinline__ void dm_add_parts(const DmCut& c, int64_t p0, int64_t p1, int sub, float (&acc)[CPL][VW]) {
    for (int64_t p = p0; p < p1; p += 4) {
        float v[4][CPL][VW];
#pragma unroll
        for (int t = 0; t < 4; ++t) dm_ld_row<VW, CPL>(c.part + (p + t < p1 ? p + t : p) * c.H, c.H, sub, c.lpt, true, v[t]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (p + t >= p1) continue;
#pragma unroll
            for (int q = 0; q < CPL; ++q)
#pragma unroll
                for (int x = 0; x < VW; ++x) acc[q][x] += v[t][q][x];
        }
    }
}
template <int VW, int CPL>
__device__ __forceinline__ void dm_zero(float (&a)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) a[q][x] = 0.f;
}

// lists of 2 .. DM_COMB_LONG pieces: one lane group per list
template <int VW, int CPL, class FIN>
__global__ __launch_bounds__(256) void k_dmf_combine(DmCut c, FIN fin) {
    const int lpt = c.lpt;
    const int64_t l = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    if (l >= c.nl) return;
    const u64 ps = c.pstart[l];
    const int64_t np = fi_lo(c.pstart[l + 1]) - fi_lo(ps), p0 = (int64_t)(ps >> 32);
    if (np < 2 || np > DM_COMB_LONG || p0 + np > c.pcap) return;
    float acc[CPL][VW];
    dm_zero<VW, CPL>(acc);
    dm_add_parts<VW, CPL>(c, p0, p0 + np, sub, acc);
    fin(l, c.ids ? (int64_t)c.ids[l] : l, sub, lpt, acc);
}

// lists of more pieces: one workgroup per list; its 256 / lpt lane groups take contiguous shares of the partial rows in order, the
// shares are added through LDS in lane-group order
template <int VW, int CPL, class FIN>
__global__ __launch_bounds__(256) void k_dmf_combine_long(DmCut c, FIN fin) {
    __shared__ __attribute__((aligned(16))) float s_red[256 * 4];   // (256 / lpt) lane groups x at most lpt * VW * CPL floats
    const int H = c.H, lpt = c.lpt;
    const int ngl = 256 / lpt, gl = (int)(threadIdx.x / lpt), sub = (int)(threadIdx.x & (lpt - 1));
    const int hs = lpt * VW * CPL;                                   // floats a lane group's share takes in LDS (>= H)
    for (int64_t l = blockIdx.x; l < c.nl; l += gridDim.x) {
        const u64 ps = c.pstart[l];
        const int64_t np = fi_lo(c.pstart[l + 1]) - fi_lo(ps), p0 = (int64_t)(ps >> 32);
        if (np <= DM_COMB_LONG || p0 + np > c.pcap) continue;        // (uniform over the workgroup)
        const int64_t per = (np + ngl - 1) / ngl;
        const int64_t k0 = gl * per < np ? gl * per : np, k1 = k0 + per < np ? k0 + per : np;
        float acc[CPL][VW];
        dm_zero<VW, CPL>(acc);
        dm_add_parts<VW, CPL>(c, p0 + k0, p0 + k1, sub, acc);
        dm_st_row<VW, CPL>(s_red + gl * hs, H, sub, lpt, acc);
        __syncthreads();
        if (gl == 0) {
            float gg[CPL][VW];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int e = (sub + q * lpt) * VW;
#pragma unroll
                for (int x = 0; x < VW; ++x) gg[q][x] = 0.f;
                if (e >= H) continue;
                for (int h = 0; h < ngl; ++h) {
                    float t4[VW];
                    ldv<VW>(s_red + h * hs + e, t4);
#pragma unroll
                    for (int x = 0; x < VW; ++x) gg[q][x] += t4[x];
                }
            }
            fin(l, c.ids ? (int64_t)c.ids[l] : l, sub, lpt, gg);
        }
        __syncthreads();
    }
}

// finish of a pooled rating row: the first Dense layer's output, out[l] = act(sum + b1)
struct DmFinAct {
    const float* bias;
    float* out;
    int H, relu;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t l, int64_t, int sub, int lpt, const float (&acc)[CPL][VW]) const {
        float b[CPL][VW], o[CPL][VW];
        dm_ld_row<VW, CPL>(bias, H, sub, lpt, true, b);
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) {
                const float z = acc[q][x] + b[q][x];
                o[q][x] = relu ? (z > 0.f ? z : 0.f) : z;
            }
        dm_st_row<VW, CPL>(out + l * H, H, sub, lpt, o);
    }
};

// finish of a fanned-out row of gW1: written out (g != NULL) or applied -- TF dense ApplyAdam on W1[row], m[row], v[row], each read
// and written once, by the lane group that holds the row's gradient
struct DmFinAdam {
    float *W, *m, *v, *g;
    int H;
    float alpha;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t, int64_t row, int sub, int lpt, const float (&acc)[CPL][VW]) const {
        if (g) {
            dm_st_row<VW, CPL>(g + row * H, H, sub, lpt, acc);
            return;
        }
        const float omb1 = 1.0f - 0.9f, omb2 = 1.0f - 0.999f, eps = 1e-7f;
        float th[CPL][VW], mm[CPL][VW], vv[CPL][VW];
        dm_ld_row<VW, CPL>(W + row * H, H, sub, lpt, true, th);
        dm_ld_row<VW, CPL>(m + row * H, H, sub, lpt, true, mm);
        dm_ld_row<VW, CPL>(v + row * H, H, sub, lpt, true, vv);
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) {
                const float gg = acc[q][x];
                mm[q][x] = mm[q][x] + (gg - mm[q][x]) * omb1;
                vv[q][x] = vv[q][x] + (gg * gg - vv[q][x]) * omb2;
                th[q][x] = th[q][x] - (mm[q][x] * alpha) / (sqrtf(vv[q][x]) + eps);
            }
        dm_st_row<VW, CPL>(W + row * H, H, sub, lpt, th);
        dm_st_row<VW, CPL>(m + row * H, H, sub, lpt, mm);
        dm_st_row<VW, CPL>(v + row * H, H, sub, lpt, vv);
    }
};

// ---- slots --------------------------------------------------------------------------------------------------------------------
// the head of every segment of one side (keys carry key_off): the row's slot, the slot's row, its first sorted position and its
// pieces; the slots past the batch's ns distinct rows get no piece; first[ns] = B closes the runs
__global__ __launch_bounds__(256) void k_dmf_slots(const u32* __restrict__ keys, u32 key_off, const int32_t* __restrict__ hd,
                                                   const int32_t* __restrict__ hs, int64_t B, int64_t N, int64_t n_max,
                                                   const int64_t* __restrict__ indptr, int piece, int32_t* __restrict__ rows,
                                                   int32_t* __restrict__ slot, int32_t* __restrict__ first, u64* __restrict__ plen,
                                                   int32_t* __restrict__ n_out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t ns = hs[B - 1] + hd[B - 1];
    ns = ns < n_max ? ns : n_max;
    if (p == 0) *n_out = (int32_t)ns, first[ns] = (int32_t)B;
    if (p >= ns && p <= n_max) plen[p] = 0ull;
    if (p >= B || !hd[p]) return;
    const int64_t row = (int64_t)(keys[p] - key_off), sl = hs[p];
    if (row >= N || sl >= n_max) return;                          // (an id past the table writes nothing outside the map)
    rows[sl] = (int32_t)row;
    slot[row] = (int32_t)sl;
    first[sl] = (int32_t)p;
    plen[sl] = fi_plen(indptr[row + 1] - indptr[row], piece);
}

// the piece counts of ALL nl lists of a CSR (the fan-out, the towers of every row); entry nl closes the scan
__global__ __launch_bounds__(256) void k_dmf_plen(const int64_t* __restrict__ indptr, int64_t nl, int piece, u64* __restrict__ plen) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l > nl) return;
    plen[l] = l < nl ? fi_plen(indptr[l + 1] - indptr[l], piece) : 0ull;
}

__global__ __launch_bounds__(256) void k_dmf_zero(float* __restrict__ x, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) x[e] = 0.f;
}

// dz <- dz where the layer's ReLU output is positive, else 0
__global__ __launch_bounds__(256) void k_dmf_relu_mask(float* __restrict__ dz, const float* __restrict__ act, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride)
        if (!(act[e] > 0.f)) dz[e] = 0.f;
}

// the last, linear layer of a step's slot rows, kept in double: out[s, d] = b[d] + sum_k a[s, k] W[k, d], k ascending (W = NULL: the
// tower has one layer and a is its output already).  A thread per output; a warp reads one row of W side by side.
__global__ __launch_bounds__(256) void k_dmf_last(const float* __restrict__ a, const float* __restrict__ W, const float* __restrict__ b,
                                                  int64_t n, int K, int D, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * D) return;
    const int64_t s = e / D;
    const int d = (int)(e - s * D);
    if (!W) {
        out[e] = (double)a[e];
        return;
    }
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc += (double)a[s * K + k] * (double)W[(int64_t)k * D + d];
    out[e] = acc + (double)b[d];
}

// ---- similarity, loss and their backward over [B, D] ----------------------------------------------------------------------------
// TAB: double for a step (the slot rows of k_dmf_last: dy = -t / (y + 1e-7) weighs a sample with a small y by 1 / y, so y is formed
// from tower outputs that were never rounded to float), float for the tables of el_dmf_towers
template <class TAB>
struct DmSimT {
    const TAB *P, *Q;                     // tower outputs [., D]: slot rows (training) or rows of all users / items (forward)
    const int32_t *u, *i;                 // the samples
    const int32_t *mu, *mi;               // id -> row of P / Q (NULL: the id itself)
    const float* label;
    int64_t B;
    int D, lpt, sim;
    float max_rating;
    const double* S;                      // [4 D] batch-axis sums of squares of p | q, then their rsqrt(max(., 1e-12))   (EL_DMF_COS_BATCH)
    const double* T;                      // [2 D] sum_b dpn_b[d] p_b[d] | the same for q
    double* dy;                           // [B]
    float* y_out;                         // [B] or NULL
    double* lossp;                        // per-workgroup partials of the loss, or NULL
};
template <class TAB>
__device__ __forceinline__ int64_t dm_prow(const DmSimT<TAB>& p, int64_t b) { return p.mu ? p.mu[p.u[b]] : p.u[b]; }
template <class TAB>
__device__ __forceinline__ int64_t dm_qrow(const DmSimT<TAB>& p, int64_t b) { return p.mi ? p.mi[p.i[b]] : p.i[b]; }
__device__ __forceinline__ double dm_rnorm(double s) { return 1.0 / sqrt(s > DM_NORM_FLOOR ? s : DM_NORM_FLOOR); }

// first level of a batch-axis column sum: workgroup k adds samples [k DM_CHUNK, (k + 1) DM_CHUNK) in sample order, a thread per
// column of [p | q].  MODE 0: x^2.  MODE 1: dy_b * (other side normalised) * x -- the coupling term of the normalisation's backward.
template <int MODE, class TAB>
__global__ __launch_bounds__(256) void k_dmf_colred(DmSimT<TAB> p, double* __restrict__ part) {
    const int D = p.D;
    const int64_t b0 = (int64_t)blockIdx.x * DM_CHUNK, b1 = b0 + DM_CHUNK < p.B ? b0 + DM_CHUNK : p.B;
    for (int c = threadIdx.x; c < 2 * D; c += 256) {
        const bool qs = c >= D;
        const int d = qs ? c - D : c;
        const double ro = MODE == 1 ? p.S[2 * D + (qs ? d : D + d)] : 0.0;
        double a = 0.0;
        for (int64_t b = b0; b < b1; ++b) {
            const double x = (double)p.P[dm_prow(p, b) * D + d], z = (double)p.Q[dm_qrow(p, b) * D + d];
            if (MODE == 0) a += qs ? z * z : x * x;
            else a += p.dy[b] * ((qs ? x : z) * ro) * (qs ? z : x);
        }
        part[(int64_t)blockIdx.x * 2 * D + c] = a;
    }
}
// second level: the partials in chunk order
__global__ __launch_bounds__(256) void k_dmf_colfin(const double* __restrict__ part, int64_t nchunk, int C, int norms, double* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0;
    for (int64_t k = 0; k < nchunk; ++k) a += part[k * C + c];
    out[c] = a;
    if (norms) out[C + c] = dm_rnorm(a);                            // (once per column: the per-sample kernels multiply)
}

// one lane group per sample: y, its clip, the sample's loss and dy = dL/dy (0 outside the clip)
template <class TAB>
__global__ __launch_bounds__(256) void k_dmf_sim(DmSimT<TAB> p) {
    const int D = p.D, lpt = p.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t groups = (int64_t)gridDim.x * 256 / lpt;
    double lossv = 0.0;
    for (int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt; b < p.B; b += groups) {
        const TAB *pr = p.P + dm_prow(p, b) * D, *qr = p.Q + dm_qrow(p, b) * D;
        double dot = 0.0, pp = 0.0, qq = 0.0;
        for (int d = sub; d < D; d += lpt) {
            const double x = (double)pr[d], z = (double)qr[d];
            if (p.sim == EL_DMF_COS_BATCH) dot += (x * p.S[2 * D + d]) * (z * p.S[3 * D + d]);
            else dot += x * z;
            pp += x * x, qq += z * z;
        }
        dot = el_group_sum(dot, lpt);
        if (p.sim == EL_DMF_COS_ROW) dot = dot * dm_rnorm(el_group_sum(pp, lpt)) * dm_rnorm(el_group_sum(qq, lpt));
        if (sub == 0) {
            if (p.y_out) p.y_out[b] = (float)dot;
            if (p.dy) {                                            // Keras BinaryCrossentropy()(label / max_rating, y), mean over B
                const double eps = 1e-7, t = (double)(p.label[b] / p.max_rating);
                const double yc = dot < eps ? eps : (dot > 1.0 - eps ? 1.0 - eps : dot);
                const bool pass = dot >= eps && dot <= 1.0 - eps;
                lossv += -(t * log(yc + eps) + (1.0 - t) * log(1.0 - yc + eps)) / (double)p.B;
                p.dy[b] = pass ? -(t / (yc + eps) - (1.0 - t) / (1.0 - yc + eps)) / (double)p.B : 0.0;
            }
        }
    }
    if (!p.lossp) return;
    __shared__ double part[4];
    for (int o = 32; o > 0; o >>= 1) lossv += __shfl_xor(lossv, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = lossv;
    __syncthreads();
    if (threadIdx.x == 0) p.lossp[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// one lane group per slot of one side: dx[s] = the sum over the slot's samples, in sample order, of dL/dx_b -- x the slot's own
// tower output (p for side 0), o_b the other side's row of sample b.  With c_b = dy_b (dot, batch cosine) or dy_b / |o_b| (row cosine)
//   A[d] = sum_b c_b o_b[d]          (and, row cosine, a = sum_b c_b (o_b . x))
//   dot    dx = A        batch  dx = rx (ro A - n_s x T rx^2)        row  dx = rx (A - x rx^2 a)            (rx^2 terms only above the floor)
// Slots past the batch's distinct rows get zeros: the products behind run on n_max rows.
template <class TAB>
__global__ __launch_bounds__(256) void k_dmf_dslot(DmSimT<TAB> p, int side, const u32* __restrict__ vals, const int32_t* __restrict__ first,
                                                   const int32_t* __restrict__ n_dev, int64_t n_max, float* __restrict__ dx) {
    const int D = p.D, lpt = p.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    if (s >= n_max) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, x[4] = {0.0, 0.0, 0.0, 0.0};
    const bool live = s < *n_dev;
    const TAB* X = side ? p.Q : p.P;
    const TAB* O = side ? p.P : p.Q;
    if (live) {
        double xx = 0.0, a = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = sub + q * lpt;
            if (d < D) x[q] = (double)X[s * D + d];
            xx += x[q] * x[q];
        }
        xx = el_group_sum(xx, lpt);
        const int64_t k0 = first[s], k1 = first[s + 1];
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t b = (int64_t)vals[k];
            const TAB* orow = O + (side ? dm_prow(p, b) : dm_qrow(p, b)) * D;
            double o[4] = {0.0, 0.0, 0.0, 0.0}, c = p.dy[b];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = sub + q * lpt;
                if (d < D) o[q] = (double)orow[d];
            }
            if (p.sim == EL_DMF_COS_ROW) {
                double oo = 0.0, ox = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) oo += o[q] * o[q], ox += o[q] * x[q];
                oo = el_group_sum(oo, lpt), ox = el_group_sum(ox, lpt);
                c = c * dm_rnorm(oo);
                a += c * ox;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += c * o[q];
        }
        const double cnt = (double)(k1 - k0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = sub + q * lpt;
            if (d >= D) continue;
            if (p.sim == EL_DMF_COS_BATCH) {
                const double sx = p.S[side ? D + d : d], rx = p.S[2 * D + (side ? D + d : d)], ro = p.S[2 * D + (side ? d : D + d)];
                const double t = sx > DM_NORM_FLOOR ? cnt * x[q] * p.T[side ? D + d : d] * rx * rx : 0.0;
                acc[q] = rx * (ro * acc[q] - t);
            } else if (p.sim == EL_DMF_COS_ROW) {
                const double rx = dm_rnorm(xx);
                acc[q] = rx * (acc[q] - (xx > DM_NORM_FLOOR ? x[q] * rx * rx * a : 0.0));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = sub + q * lpt;
        if (d < D) dx[s * D + d] = (float)acc[q];
    }
}

// the step's loss from the per-workgroup partials in index order (workgroup 0); both slot maps back to -1 through the lists of the
// batch's distinct rows (every workgroup): the last kernel that reads the maps clears them
__global__ __launch_bounds__(256) void k_dmf_finish(const int32_t* __restrict__ rows_u, const int32_t* __restrict__ nu, int32_t* __restrict__ slot_u,
                                                    const int32_t* __restrict__ rows_i, const int32_t* __restrict__ ni, int32_t* __restrict__ slot_i,
                                                    const double* __restrict__ part, int nparts, double* loss_out) {
    const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t s = t0; s < *nu; s += stride) slot_u[rows_u[s]] = -1;
    for (int64_t s = t0; s < *ni; s += stride) slot_i[rows_i[s]] = -1;
    if (blockIdx.x != 0) return;
    __shared__ double red[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) a += part[k];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_out += red[0];
}

// ---- scoring: the normalised factor tables of one evaluation chunk ----------------------------------------------------------------
// S[d] = sum over users [u0, u1) of P[u, d]^2: ONE workgroup, its 256 / Dp row groups (Dp = D rounded up to a power of two) take
// contiguous shares of the users in user order, the shares are added in row-group order
__global__ __launch_bounds__(256) void k_dmf_chunk_sq(const float* __restrict__ P, int64_t u0, int64_t u1, int D, double* __restrict__ S) {
    __shared__ double red[256];
    int Dp = 1;
    while (Dp < D) Dp <<= 1;
    const int d = (int)threadIdx.x % Dp, rg = (int)threadIdx.x / Dp, nrg = 256 / Dp;
    const int64_t n = u1 - u0, per = (n + nrg - 1) / nrg;
    const int64_t a0 = u0 + (rg * per < n ? rg * per : n), a1 = a0 + per < u1 ? a0 + per : u1;
    double a = 0.0;
    if (d < D)
        for (int64_t u = a0; u < a1; ++u) a += (double)P[u * D + d] * (double)P[u * D + d];
    red[threadIdx.x] = a;
    __syncthreads();
    if (rg != 0 || d >= D) return;
    double t = 0.0;
    for (int h = 0; h < nrg; ++h) t += red[h * Dp + d];
    S[d] = t;
}
// one wave per row: out[r] = X[r0 + r] * rsqrt(max(n, 1e-12)) with n = S[d] (S != NULL: the chunk's users), uc * x^2 (uc > 0: get_recs'
// item side, whose batch axis holds uc copies of the item) or the row's own sum of squares (the feature-axis cosine)
__global__ __launch_bounds__(256) void k_dmf_scale(const float* __restrict__ X, int64_t r0, int64_t n, int D, const double* __restrict__ S,
                                                   double uc, float* __restrict__ out) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const float* x = X + (r0 + r) * D;
    double rr = 0.0;
    for (int d = lane; d < D; d += 64) rr += (double)x[d] * (double)x[d];
    rr = el_group_sum(rr, 64);
    for (int d = lane; d < D; d += 64) {
        const double v = (double)x[d], nn = S ? S[d] : (uc > 0.0 ? uc * (v * v) : rr);
        out[r * D + d] = (float)(v * dm_rnorm(nn));
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct DmCutWs {
    u64 *plen, *pstart;
    void* scan_tmp;
    size_t scan_bytes;
    float* part;
    int64_t pcap;
};
struct DmfWs {
    u32 *key_in, *val_in, *key, *val;
    int32_t *hd[2], *hs[2], *rows[2], *first[2], *n_dev[2], *dummy;
    float *act[2][4], *dact[2][4];
    double *dy, *cpart, *S, *T, *lossp, *pd[2];
    void *sort_tmp, *scan_tmp, *gemm;
    size_t sort_bytes, scan_bytes, gemm_bytes, total;
    int64_t n_max[2], nchunk;
    DmCutWs cut;
};

int dmf_piece(el_ctx* ctx) {
    const double v = ctx->opt.fism_piece;
    const int p = (int)v;
    return ((double)p == v && p >= 8 && p <= 4096 && (p & (p - 1)) == 0) ? p : 0;
}
int64_t dmf_sim_cap(el_ctx* ctx) { return (int64_t)ctx->cus * 16; }
int64_t dmf_rows(const el_dmf_state* st, int t) { return t == 0 ? st->U : st->I; }      // rows a tower serves
int64_t dmf_cols(const el_dmf_state* st, int t) { return t == 0 ? st->I : st->U; }      // rows of its first kernel
int dmf_D(const el_dmf_state* st) { return st->tw[0].width[st->tw[0].n_layers - 1]; }

// the scratch of one run of the primitive over at most nl lists of at most nnz positions: a list of more than one piece has fewer
// than 2 len / piece of them, and there are at most nl + nnz / piece pieces
int dmf_cut_carve(ElCarve& c, int64_t nl, int64_t nnz, int piece, int H, DmCutWs* w) {
    w->plen = c.take<u64>((size_t)(nl + 1));
    w->pstart = c.take<u64>((size_t)(nl + 1));
    size_t t = 0;
    u64* np = nullptr;
    if (rocprim::exclusive_scan(nullptr, t, np, np, (u64)0, (size_t)(nl + 1), rocprim::plus<u64>(), (hipStream_t)0) != hipSuccess) return 1;
    w->scan_bytes = t;
    w->scan_tmp = c.take<char>(t);
    const int64_t a = 2 * (nnz / piece) + 1, b = nl + nnz / piece;
    w->pcap = a < b ? a : b;
    w->part = c.take<float>((size_t)w->pcap * (size_t)H);
    return 0;
}

// the largest el_gemm_f32 scratch of a tower's products on n rows
size_t dmf_gemm_bytes(el_ctx* ctx, const el_dmf_tower& tw, int64_t n, bool backward) {
    size_t m = 0;
    for (int l = 1; l < tw.n_layers; ++l) {
        const int64_t kin = tw.width[l - 1], kout = tw.width[l];
        size_t a = el_gemm_ws_bytes(ctx, n, kout, kin);
        if (backward) {
            const size_t b = el_gemm_ws_bytes(ctx, kin, kout, n), d = el_gemm_ws_bytes(ctx, n, kin, kout);
            a = a > b ? a : b;
            a = a > d ? a : d;
        }
        m = m > a ? m : a;
    }
    return m;
}

int dmf_carve(el_ctx* ctx, const el_dmf_state* st, int64_t B, void* base, DmfWs* w) {
    ElCarve c{(char*)base};
    const int D = dmf_D(st), piece = dmf_piece(ctx);
    w->key_in = c.take<u32>((size_t)(2 * B));
    w->val_in = c.take<u32>((size_t)(2 * B));
    w->key = c.take<u32>((size_t)(2 * B));
    w->val = c.take<u32>((size_t)(2 * B));
    w->dummy = c.take<int32_t>(4);
    w->gemm_bytes = 0;
    for (int t = 0; t < 2; ++t) {
        const el_dmf_tower& tw = st->tw[t];
        const int64_t n = B < dmf_rows(st, t) ? B : dmf_rows(st, t);
        w->n_max[t] = n;
        w->hd[t] = c.take<int32_t>((size_t)B);
        w->hs[t] = c.take<int32_t>((size_t)B);
        w->rows[t] = c.take<int32_t>((size_t)n);
        w->first[t] = c.take<int32_t>((size_t)(n + 1));
        w->n_dev[t] = c.take<int32_t>(1);
        for (int l = 0; l < tw.n_layers; ++l) {
            w->act[t][l] = c.take<float>((size_t)n * (size_t)tw.width[l]);
            w->dact[t][l] = c.take<float>((size_t)n * (size_t)tw.width[l]);
        }
        w->pd[t] = c.take<double>((size_t)n * (size_t)D);
        const size_t g = dmf_gemm_bytes(ctx, tw, n, true);
        w->gemm_bytes = w->gemm_bytes > g ? w->gemm_bytes : g;
    }
    w->gemm = c.take<char>(w->gemm_bytes);
    w->nchunk = (B + DM_CHUNK - 1) / DM_CHUNK;
    w->dy = c.take<double>((size_t)B);
    w->cpart = c.take<double>((size_t)w->nchunk * 2 * (size_t)D);
    w->S = c.take<double>((size_t)(4 * D));
    w->T = c.take<double>((size_t)(2 * D));
    w->lossp = c.take<double>((size_t)dmf_sim_cap(ctx));
    size_t t1 = 0, t2 = 0;
    u32* np = nullptr;
    int32_t* ip = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (unsigned)(2 * B), 0, el_bits_for(st->U + st->I), (hipStream_t)0) != hipSuccess)
        return 1;
    if (rocprim::exclusive_scan(nullptr, t2, ip, ip, (int32_t)0, (size_t)B, rocprim::plus<int32_t>(), (hipStream_t)0) != hipSuccess) return 1;
    w->sort_bytes = t1, w->scan_bytes = t2;
    w->sort_tmp = c.take<char>(t1);
    w->scan_tmp = c.take<char>(t2);
    // ONE scratch of the primitive serves the two forwards (n_max lists each) and the two fan-outs (I and U lists), one after the other
    const int64_t nl = st->U > st->I ? st->U : st->I;
    const int H = st->tw[0].width[0] > st->tw[1].width[0] ? st->tw[0].width[0] : st->tw[1].width[0];
    if (dmf_cut_carve(c, nl > B ? nl : B, st->nnz, piece, H, &w->cut)) return 1;
    w->total = c.off;
    return 0;
}

// the scratch of el_dmf_towers: the activations of every row below the last layer, the products' scratch, the primitive's
struct DmfTowersWs {
    float* act[4];
    void* gemm;
    size_t gemm_bytes, total;
    DmCutWs cut;
};
int dmf_towers_carve(el_ctx* ctx, const el_dmf_state* st, void* base, DmfTowersWs* w) {
    ElCarve c{(char*)base};
    w->gemm_bytes = 0;
    for (int l = 0; l < 4; ++l) {
        size_t n = 0;
        for (int t = 0; t < 2; ++t)
            if (l < st->tw[t].n_layers - 1) {
                const size_t m = (size_t)dmf_rows(st, t) * (size_t)st->tw[t].width[l];
                n = n > m ? n : m;
            }
        w->act[l] = c.take<float>(n);
    }
    for (int t = 0; t < 2; ++t) {
        const size_t g = dmf_gemm_bytes(ctx, st->tw[t], dmf_rows(st, t), false);
        w->gemm_bytes = w->gemm_bytes > g ? w->gemm_bytes : g;
    }
    w->gemm = c.take<char>(w->gemm_bytes);
    const int H = st->tw[0].width[0] > st->tw[1].width[0] ? st->tw[0].width[0] : st->tw[1].width[0];
    if (dmf_cut_carve(c, st->U > st->I ? st->U : st->I, st->nnz, dmf_piece(ctx), H, &w->cut)) return 1;
    w->total = c.off;
    return 0;
}

// the scratch of el_dmf_scores for a chunk of n users and of el_dmf_forward for n pairs
struct DmfScoreWs {
    double *S, *cpart;
    float* Pt;
    void* gemm;
    size_t gemm_bytes, total;
    int64_t nchunk;
};
void dmf_score_carve(el_ctx* ctx, const el_dmf_state* st, int64_t n, bool pairs, void* base, DmfScoreWs* w) {
    ElCarve c{(char*)base};
    const int D = dmf_D(st);
    w->S = c.take<double>((size_t)(4 * D));
    w->nchunk = pairs ? (n + DM_CHUNK - 1) / DM_CHUNK : 0;
    w->cpart = c.take<double>((size_t)w->nchunk * 2 * (size_t)D);
    w->Pt = c.take<float>(pairs ? 0 : (size_t)n * (size_t)D);
    w->gemm_bytes = pairs ? 0 : el_gemm_ws_bytes(ctx, n, st->I, D);
    w->gemm = c.take<char>(w->gemm_bytes);
    w->total = c.off;
}

bool dmf_al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

int dmf_check_tower(const el_dmf_tower& tw, const char* who, const char* side, int level) {
    EL_REQUIRE(tw.n_layers >= 1 && tw.n_layers <= 4, "%s: %s tower has %d layers (1 .. 4)", who, side, tw.n_layers);
    for (int l = 0; l < tw.n_layers; ++l) {
        EL_REQUIRE(tw.width[l] >= 1 && tw.width[l] <= 256, "%s: %s tower layer %d has width %d (1 .. 256)", who, side, l, tw.width[l]);
        EL_REQUIRE(tw.W[l] && tw.b[l], "%s: %s tower layer %d has no kernel or bias", who, side, l);
        if (level >= 1) EL_REQUIRE(tw.gb[l] && (l == 0 || tw.gW[l]), "%s: %s tower layer %d has no gradient buffers", who, side, l);
        if (level >= 2) EL_REQUIRE(tw.mW[l] && tw.vW[l] && tw.mb[l] && tw.vb[l], "%s: %s tower layer %d: Adam slots missing", who, side, l);
    }
    return 0;
}

int dmf_check_state(el_ctx* ctx, const el_dmf_state* st, const char* who, int level) {   // 0: scoring, 1: + gradients, 2: + Adam slots
    EL_REQUIRE(st != nullptr, "%s: null state", who);
    EL_REQUIRE(st->U > 0 && st->I > 0 && st->nnz >= 0, "%s: bad shape U=%lld I=%lld nnz=%lld", who, (long long)st->U, (long long)st->I,
               (long long)st->nnz);
    EL_REQUIRE(st->U + st->I < (1LL << 31) && st->nnz < (1LL << 40), "%s: U + I must fit a 32-bit sort key", who);
    if (int rc = dmf_check_tower(st->tw[0], who, "user", level)) return rc;
    if (int rc = dmf_check_tower(st->tw[1], who, "item", level)) return rc;
    EL_REQUIRE(dmf_D(st) == st->tw[1].width[st->tw[1].n_layers - 1], "%s: the towers end in different widths (%d, %d)", who, dmf_D(st),
               st->tw[1].width[st->tw[1].n_layers - 1]);
    EL_REQUIRE(st->sim == EL_DMF_DOT || st->sim == EL_DMF_COS_BATCH || st->sim == EL_DMF_COS_ROW, "%s: unknown similarity %d", who, st->sim);
    EL_REQUIRE(st->max_rating > 0.f, "%s: max_rating must be positive", who);
    EL_REQUIRE(st->r_indptr && st->r_indices && st->r_values && st->t_indptr && st->t_indices && st->t_values,
               "%s: needs the rating matrix user-major and item-major, with values", who);
    EL_REQUIRE(dmf_piece(ctx) != 0, "%s: option fism_piece must be a power of two in 8 .. 4096", who);
    if (level >= 1) EL_REQUIRE(st->slot_u && st->slot_i, "%s: needs the two slot maps", who);
    return 0;
}

#define DM_DISPATCH(vec, cpl, CALL)        \
    do {                                   \
        if (vec) CALL(4, 1);               \
        else if ((cpl) == 1) CALL(1, 1);   \
        else if ((cpl) == 2) CALL(1, 2);   \
        else CALL(1, 4);                   \
    } while (0)

// one run of the primitive: the scan of the piece counts (already in cw.plen), the pieces, the two combines
template <class FIN>
int dmf_run_cut(el_ctx* ctx, hipStream_t s, const DmCutWs& cw, DmCut c, int64_t nnz, bool vec, const FIN& fin, const char* nm) {
    {
        ElKernelTimer t("rocprim_exclusive_scan", s);
        size_t tb = cw.scan_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(cw.scan_tmp, tb, cw.plen, cw.pstart, (u64)0, (size_t)(c.nl + 1), rocprim::plus<u64>(), s));
    }
    int cpl = 1;
    c.lpt = el_pick_lpt(c.H, vec ? 4 : 1, &cpl);
    c.pstart = cw.pstart, c.pcap = cw.pcap, c.part = cw.part;
    const int64_t pieces = c.nl + nnz / c.piece;                     // (an upper bound: the lane groups past the scan's total leave at once)
    const unsigned gp = (unsigned)((pieces * c.lpt + 255) / 256), gc = (unsigned)((c.nl * c.lpt + 255) / 256);
    const int64_t capl = (int64_t)ctx->cus * 4;
    const unsigned gl = (unsigned)(c.nl < capl ? c.nl : capl);
#define DM_CUT(VW_, CPL_)                                                                                            \
    do {                                                                                                             \
        EL_LAUNCH(nm, (k_dmf_cut<VW_, CPL_, FIN>), dim3(gp), dim3(256), 0, s, c, fin);                                 \
        EL_LAUNCH("k_dmf_combine", (k_dmf_combine<VW_, CPL_, FIN>), dim3(gc), dim3(256), 0, s, c, fin);                \
        EL_LAUNCH("k_dmf_combine_long", (k_dmf_combine_long<VW_, CPL_, FIN>), dim3(gl), dim3(256), 0, s, c, fin);      \
    } while (0)
    DM_DISPATCH(vec, cpl, DM_CUT);
#undef DM_CUT
    return 0;
}

struct DmCsr {
    const int64_t* indptr;
    const int32_t* indices;
    const float* values;
};
DmCsr dmf_csr(const el_dmf_state* st, int t, bool transposed) {
    if ((t == 0) != transposed) return {st->r_indptr, st->r_indices, st->r_values};
    return {st->t_indptr, st->t_indices, st->t_values};
}

// layers 1 .. L - 1 of one tower on n rows: act[l] = relu(act[l - 1] W[l] + b[l]), the last one linear into `last` (NULL: left to
// k_dmf_last)
int dmf_inner_forward(el_ctx* ctx, hipStream_t s, const el_dmf_tower& tw, int64_t n, float* const* act, float* last, void* gws, size_t gwb) {
    for (int l = 1; l < tw.n_layers; ++l) {
        const bool end = l == tw.n_layers - 1;
        if (end && !last) break;
        if (int rc = el_gemm_f32(ctx, s, 0, 0, n, tw.width[l], tw.width[l - 1], act[l - 1], tw.width[l - 1], tw.W[l], tw.width[l],
                                 end ? last : act[l], tw.width[l], tw.b[l], end ? 0 : 2, gws, gwb))
            return rc;
    }
    return 0;
}

int dmf_sim_lpt(int D) {
    int cpl = 1;
    return el_pick_lpt(D, 1, &cpl);                                  // 8 .. 64 lanes, at most 4 columns per lane (D <= 256)
}

// batch-axis sums over the samples of p: both levels
template <int MODE, class TAB>
int dmf_colsum(hipStream_t s, const DmSimT<TAB>& p, int64_t nchunk, double* cpart, double* out) {
    EL_LAUNCH(MODE ? "k_dmf_colred_T" : "k_dmf_colred_S", (k_dmf_colred<MODE, TAB>), dim3((unsigned)nchunk), dim3(256), 0, s, p, cpart);
    EL_LAUNCH("k_dmf_colfin", k_dmf_colfin, dim3((unsigned)((2 * p.D + 255) / 256)), dim3(256), 0, s, cpart, nchunk, 2 * p.D, MODE == 0 ? 1 : 0, out);
    return 0;
}

int dmf_grads(el_ctx* ctx, hipStream_t s, const el_dmf_state* st, const int32_t* u, const int32_t* i, const float* y, int64_t B,
              double* loss_out, void* ws, size_t ws_bytes, bool apply, float lr_t, const char* who) {
    EL_REQUIRE(u && i && y && loss_out, "%s: null argument", who);
    EL_REQUIRE(B >= 1 && B < (1LL << 30), "%s: batch size %lld out of range", who, (long long)B);
    DmfWs w;
    EL_REQUIRE(dmf_carve(ctx, st, B, ws, &w) == 0, "%s: rocprim size query failed", who);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    if (!apply) EL_REQUIRE(st->tw[0].gW[0] && st->tw[1].gW[0], "%s: needs gW of both first layers", who);
    const int D = dmf_D(st), piece = dmf_piece(ctx);
    int32_t* const slot[2] = {st->slot_u, st->slot_i};

    // 1: the sorted pairs, the batch's distinct users and items, their slots, sample runs and piece counts
    const unsigned gb = (unsigned)((B + 256) / 256);
    EL_LAUNCH("k_fism_keys", k_fism_keys, dim3(gb), dim3(256), 0, s, u, i, B, (u32)st->U, w.key_in, w.val_in, w.dummy, w.dummy + 1, w.cut.plen,
              (int64_t)0);
    {
        ElKernelTimer t("rocprim_radix_sort_pairs", s);
        size_t tb = w.sort_bytes;
        EL_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tb, w.key_in, w.key, w.val_in, w.val, (unsigned)(2 * B), 0,
                                               el_bits_for(st->U + st->I), s));
    }
    for (int t = 0; t < 2; ++t) {
        EL_LAUNCH("k_fism_heads", k_fism_heads, dim3(gb), dim3(256), 0, s, w.key + t * B, B, w.hd[t]);
        ElKernelTimer tm("rocprim_exclusive_scan", s);
        size_t tb = w.scan_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(w.scan_tmp, tb, w.hd[t], w.hs[t], (int32_t)0, (size_t)B, rocprim::plus<int32_t>(), s));
    }

    // 2: the towers of the distinct rows
    for (int t = 0; t < 2; ++t) {
        const el_dmf_tower& tw = st->tw[t];
        const DmCsr m = dmf_csr(st, t, false);
        const int H = tw.width[0];
        const int64_t n = w.n_max[t];
        EL_LAUNCH("k_dmf_slots", k_dmf_slots, dim3(gb), dim3(256), 0, s, w.key + t * B, t ? (u32)st->U : 0u, w.hd[t], w.hs[t], B, dmf_rows(st, t), n,
                  m.indptr, piece, w.rows[t], slot[t], w.first[t], w.cut.plen, w.n_dev[t]);
        EL_LAUNCH("k_dmf_zero", k_dmf_zero, dim3(el_stream_grid(ctx, n * H)), dim3(256), 0, s, w.act[t][0], n * H);
        const bool vec = H % 4 == 0 && dmf_al16(tw.W[0]) && dmf_al16(tw.b[0]);
        DmCut c = {m.indptr, m.indices, m.values, w.rows[t], nullptr, tw.W[0], nullptr, n, 0, piece, H, 0, nullptr};
        DmFinAct fin = {tw.b[0], w.act[t][0], H, tw.n_layers > 1 ? 1 : 0};
        if (int rc = dmf_run_cut(ctx, s, w.cut, c, st->nnz, vec, fin, "k_dmf_cut_fwd")) return rc;
        if (int rc = dmf_inner_forward(ctx, s, tw, n, w.act[t], nullptr, w.gemm, w.gemm_bytes)) return rc;
        const int L = tw.n_layers, K = L > 1 ? tw.width[L - 2] : D;
        EL_LAUNCH("k_dmf_last", k_dmf_last, dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, s, w.act[t][L > 1 ? L - 2 : 0],
                  L > 1 ? tw.W[L - 1] : nullptr, tw.b[L - 1], n, K, D, w.pd[t]);
    }

    // 3: similarity, loss, dy; dp and dq per slot
    const int Lu = st->tw[0].n_layers, Li = st->tw[1].n_layers;
    DmSimT<double> p = {w.pd[0], w.pd[1], u, i, st->slot_u, st->slot_i, y, B, D, dmf_sim_lpt(D), st->sim, st->max_rating,
               w.S, w.T, w.dy, nullptr, w.lossp};
    if (st->sim == EL_DMF_COS_BATCH)
        if (int rc = dmf_colsum<0>(s, p, w.nchunk, w.cpart, w.S)) return rc;
    const int64_t want = (B * p.lpt + 255) / 256, cap = dmf_sim_cap(ctx);
    const unsigned gsim = (unsigned)(want < cap ? want : cap);
    EL_LAUNCH("k_dmf_sim", k_dmf_sim<double>, dim3(gsim), dim3(256), 0, s, p);
    if (st->sim == EL_DMF_COS_BATCH)
        if (int rc = dmf_colsum<1>(s, p, w.nchunk, w.cpart, w.T)) return rc;
    for (int t = 0; t < 2; ++t)
        EL_LAUNCH("k_dmf_dslot", k_dmf_dslot<double>, dim3((unsigned)((w.n_max[t] * p.lpt + 255) / 256)), dim3(256), 0, s, p, t, w.val + t * B, w.first[t],
                  w.n_dev[t], w.n_max[t], w.dact[t][st->tw[t].n_layers - 1]);

    // 4: back through the towers; the first layer's weight gradient fans out over the transposed matrix and meets Adam there
    for (int t = 0; t < 2; ++t) {
        const el_dmf_tower& tw = st->tw[t];
        const int64_t n = w.n_max[t];
        for (int l = tw.n_layers - 1; l >= 1; --l) {
            const int kin = tw.width[l - 1], kout = tw.width[l];
            if (int rc = el_colsum_finish(s, w.dact[t][l], (int)n, kout, tw.gb[l])) return rc;
            if (int rc = el_gemm_f32(ctx, s, 1, 0, kin, kout, n, w.act[t][l - 1], kin, w.dact[t][l], kout, tw.gW[l], kout, nullptr, 0, w.gemm,
                                     w.gemm_bytes))
                return rc;
            if (int rc = el_gemm_f32(ctx, s, 0, 1, n, kin, kout, w.dact[t][l], kout, tw.W[l], kout, w.dact[t][l - 1], kin, nullptr, 0, w.gemm,
                                     w.gemm_bytes))
                return rc;
            EL_LAUNCH("k_dmf_relu_mask", k_dmf_relu_mask, dim3(el_stream_grid(ctx, n * kin)), dim3(256), 0, s, w.dact[t][l - 1], w.act[t][l - 1],
                      n * kin);
        }
        const int H = tw.width[0];
        if (int rc = el_colsum_finish(s, w.dact[t][0], (int)n, H, tw.gb[0])) return rc;
        const DmCsr m = dmf_csr(st, t, true);
        const int64_t nl = dmf_cols(st, t);
        EL_LAUNCH("k_dmf_plen", k_dmf_plen, dim3((unsigned)((nl + 256) / 256)), dim3(256), 0, s, m.indptr, nl, piece, w.cut.plen);
        const bool vec = H % 4 == 0 && dmf_al16(tw.W[0]) && (apply ? dmf_al16(tw.mW[0]) && dmf_al16(tw.vW[0]) : dmf_al16(tw.gW[0]));
        DmCut c = {m.indptr, m.indices, m.values, nullptr, slot[t], w.dact[t][0], nullptr, nl, 0, piece, H, 0, nullptr};
        DmFinAdam fin = {tw.W[0], tw.mW[0], tw.vW[0], apply ? nullptr : tw.gW[0], H, lr_t};
        if (int rc = dmf_run_cut(ctx, s, w.cut, c, st->nnz, vec, fin, apply ? "k_dmf_cut_fan_adam" : "k_dmf_cut_fan")) return rc;
    }

    // 5: the loss; the slot maps are -1 again
    const int64_t nm = w.n_max[0] > w.n_max[1] ? w.n_max[0] : w.n_max[1];
    EL_LAUNCH("k_dmf_finish", k_dmf_finish, dim3(el_stream_grid(ctx, nm)), dim3(256), 0, s, w.rows[0], w.n_dev[0], st->slot_u, w.rows[1],
              w.n_dev[1], st->slot_i, w.lossp, (int)gsim, loss_out);
    EL_CHECK_LAUNCH();
    return 0;
}

// TF dense ApplyAdam on the variables whose gradients sit in HBM: every bias and inner kernel, and with first = true the two first
// kernels from gW[0] (the unfused pair el_dmf_grads + el_dmf_apply)
int dmf_apply(el_ctx* ctx, hipStream_t s, const el_dmf_state* st, float lr_t, bool first) {
    for (int t = 0; t < 2; ++t) {
        const el_dmf_tower& tw = st->tw[t];
        for (int l = 0; l < tw.n_layers; ++l) {
            const int64_t kin = l == 0 ? dmf_cols(st, t) : tw.width[l - 1], nw = kin * tw.width[l];
            if (l > 0 || first)
                EL_LAUNCH("k_dmf_opt_W", k_adam_apply_dense, dim3(el_stream_grid(ctx, nw)), dim3(256), 0, s, tw.W[l], tw.gW[l], tw.mW[l], tw.vW[l],
                          nw, lr_t, 0.9f, 0.999f, 1e-7f, 0);
            EL_LAUNCH("k_dmf_opt_b", k_adam_apply_dense, dim3(1), dim3(256), 0, s, tw.b[l], tw.gb[l], tw.mb[l], tw.vb[l], (int64_t)tw.width[l], lr_t,
                      0.9f, 0.999f, 1e-7f, 0);
        }
    }
    EL_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t el_dmf_ws_bytes(el_ctx* ctx, const el_dmf_state* st, int64_t n, int32_t what) {
    if (!ctx || el_bind(ctx) || dmf_check_state(ctx, st, "el_dmf_ws_bytes", 0)) return 0;
    if (what == EL_DMF_WS_TOWERS) {
        DmfTowersWs w;
        return dmf_towers_carve(ctx, st, nullptr, &w) ? 0 : w.total;
    }
    if (n < 1 || n >= (1LL << 30)) return 0;
    if (what == EL_DMF_WS_STEP) {
        DmfWs w;
        return dmf_carve(ctx, st, n, nullptr, &w) ? 0 : w.total;
    }
    if (what != EL_DMF_WS_SCORES && what != EL_DMF_WS_FORWARD) return 0;
    DmfScoreWs w;
    dmf_score_carve(ctx, st, n, what == EL_DMF_WS_FORWARD, nullptr, &w);
    return w.total;
}

extern "C" int el_dmf_grads(el_ctx* ctx, void* stream, const el_dmf_state* st, const int32_t* u, const int32_t* i, const float* label,
                            int64_t B, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = dmf_check_state(ctx, st, "el_dmf_grads", 1)) return rc;
    return dmf_grads(ctx, (hipStream_t)stream, st, u, i, label, B, loss_out, ws, ws_bytes, false, 0.f, "el_dmf_grads");
}

extern "C" int el_dmf_apply(el_ctx* ctx, void* stream, const el_dmf_state* st, int32_t step, float lr_t) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = dmf_check_state(ctx, st, "el_dmf_apply", 2)) return rc;
    EL_REQUIRE(step >= 1, "el_dmf_apply: step must be >= 1");
    EL_REQUIRE(st->tw[0].gW[0] && st->tw[1].gW[0], "el_dmf_apply: needs gW of both first layers");
    return dmf_apply(ctx, (hipStream_t)stream, st, lr_t, true);
}

extern "C" int el_dmf_train_step(el_ctx* ctx, void* stream, const el_dmf_state* st, const int32_t* u, const int32_t* i, const float* label,
                                 int64_t B, int32_t step, float lr_t, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = dmf_check_state(ctx, st, "el_dmf_train_step", 2)) return rc;
    EL_REQUIRE(step >= 1, "el_dmf_train_step: step must be >= 1");
    if (int rc = dmf_grads(ctx, (hipStream_t)stream, st, u, i, label, B, loss_out, ws, ws_bytes, true, lr_t, "el_dmf_train_step")) return rc;
    return dmf_apply(ctx, (hipStream_t)stream, st, lr_t, false);
}

extern "C" int el_dmf_towers(el_ctx* ctx, void* stream, const el_dmf_state* st, float* P, float* Q, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = dmf_check_state(ctx, st, "el_dmf_towers", 0)) return rc;
    EL_REQUIRE(P && Q, "el_dmf_towers: null output");
    DmfTowersWs w;
    EL_REQUIRE(dmf_towers_carve(ctx, st, ws, &w) == 0, "el_dmf_towers: rocprim size query failed");
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "el_dmf_towers: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    const int piece = dmf_piece(ctx);
    for (int t = 0; t < 2; ++t) {
        const el_dmf_tower& tw = st->tw[t];
        const DmCsr m = dmf_csr(st, t, false);
        const int64_t n = dmf_rows(st, t);
        const int H = tw.width[0];
        float* out = t ? Q : P;
        float* a0 = tw.n_layers > 1 ? w.act[0] : out;
        EL_LAUNCH("k_dmf_plen", k_dmf_plen, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, s, m.indptr, n, piece, w.cut.plen);
        const bool vec = H % 4 == 0 && dmf_al16(tw.W[0]) && dmf_al16(tw.b[0]) && dmf_al16(a0);
        DmCut c = {m.indptr, m.indices, m.values, nullptr, nullptr, tw.W[0], nullptr, n, 0, piece, H, 0, nullptr};
        DmFinAct fin = {tw.b[0], a0, H, tw.n_layers > 1 ? 1 : 0};
        if (int rc = dmf_run_cut(ctx, s, w.cut, c, st->nnz, vec, fin, "k_dmf_cut_rows")) return rc;
        if (int rc = dmf_inner_forward(ctx, s, tw, n, w.act, out, w.gemm, w.gemm_bytes)) return rc;
    }
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_dmf_forward(el_ctx* ctx, void* stream, const el_dmf_state* st, const float* P, const float* Q, const int32_t* u,
                              const int32_t* i, int64_t n, float* out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = dmf_check_state(ctx, st, "el_dmf_forward", 0)) return rc;
    if (n <= 0) return 0;
    EL_REQUIRE(P && Q && u && i && out && n < (1LL << 30), "el_dmf_forward: bad arguments");
    DmfScoreWs w;
    dmf_score_carve(ctx, st, n, true, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "el_dmf_forward: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    const int D = dmf_D(st);
    DmSimT<float> p = {P, Q, u, i, nullptr, nullptr, nullptr, n, D, dmf_sim_lpt(D), st->sim, st->max_rating, w.S, nullptr, nullptr, out, nullptr};
    if (st->sim == EL_DMF_COS_BATCH)
        if (int rc = dmf_colsum<0>(s, p, w.nchunk, w.cpart, w.S)) return rc;
    const int64_t want = (n * p.lpt + 255) / 256, cap = dmf_sim_cap(ctx);
    EL_LAUNCH("k_dmf_sim", k_dmf_sim<float>, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, s, p);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_dmf_scores(el_ctx* ctx, void* stream, const el_dmf_state* st, const float* P, const float* Q, int64_t u_start,
                             int64_t u_stop, float* Qt, int32_t qt_ready, float* out, int64_t ld, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = dmf_check_state(ctx, st, "el_dmf_scores", 0)) return rc;
    EL_REQUIRE(P && Q && out && u_start >= 0 && u_start < u_stop && u_stop <= st->U && ld >= st->I, "el_dmf_scores: bad arguments");
    EL_REQUIRE(st->sim == EL_DMF_DOT || Qt, "el_dmf_scores: a cosine needs the scaled item table Qt [I, D]");
    const int64_t n = u_stop - u_start;
    DmfScoreWs w;
    dmf_score_carve(ctx, st, n, false, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "el_dmf_scores: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    const int D = dmf_D(st);
    const float *A = P + u_start * D, *Bm = Q;
    if (st->sim != EL_DMF_DOT) {
        const bool batch = st->sim == EL_DMF_COS_BATCH;
        if (batch) EL_LAUNCH("k_dmf_chunk_sq", k_dmf_chunk_sq, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, P, u_start, u_stop, D, w.S);
        EL_LAUNCH("k_dmf_scale_P", k_dmf_scale, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, P, u_start, n, D, batch ? w.S : nullptr, 0.0, w.Pt);
        if (!qt_ready)
            EL_LAUNCH("k_dmf_scale_Q", k_dmf_scale, dim3((unsigned)((st->I + 3) / 4)), dim3(256), 0, s, Q, (int64_t)0, st->I, D, nullptr,
                      batch ? (double)n : 0.0, Qt);
        A = w.Pt, Bm = Qt;
    }
    if (int rc = el_gemm_f32(ctx, s, 0, 1, n, st->I, D, A, D, Bm, D, out, ld, nullptr, 0, w.gemm, w.gemm_bytes)) return rc;
    EL_CHECK_LAUNCH();
    return 0;
}
