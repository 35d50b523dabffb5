// NAIS (neural attentive item similarity, He et al. 2018), `algorithm: concat` -- contract in include/elliot_hip.h, DESIGN 3.31;
// reference: elliot/recommender/neural/NAIS/nais_model.py.
//
// A sample is b = (u, j, label), H(u) = (h_1 .. h_n) the user's train items in CSR order, t = Gj[j], coef_u = n^-alpha (uploaded).
//   s_k = Gi[h_k] . t     v_k = [Gi[h_k], t] W1 + b1     a_k = (relu(v_k) W2 + b2) W3 + b3     x_k = exp(a_k)
//   S = sum x_k     N = sum x_k s_k     out = sigma(coef_u N / S^beta + Bu[u] + Bi[j])
// THE ALGEBRA
//   1. The first layer splits.  W1a = W1[:F], W1b = W1[F:]:  v_k = A[h_k] + Bt[j] with A = Gi W1a [I, 2F] and Bt = Gj W1b + b1
//      [I, 2F], one product each per call (el_gemm_f32).  A (history row, target) pair costs 2F adds, not a 2F x 2F product.
//   2. The two linear layers collapse.  a_k = relu(v_k) . w + c with w = W2 W3 [2F] and c = b2 . W3 + b3 (k_nais_collapse).
//   3. Gradients.  With r_b = dL/dx_b coef_u S^-beta:
//        ds_k = r x_k      da_k = r x_k (s_k - beta N / S)      dv_k = da_k w * [v_k > 0]      (TF's ReLU gradient is 0 at exactly 0)
//        gGi[h] = sum over pairs (b, k) with h_k = h of ds_k t_b  + gA[h] W1a^T        gA[h]  = sum of dv_k over the same pairs
//        gGj[j] = sum over samples with j_b = j of sum_k ds_k Gi[h_k]  + gBt[j] W1b^T   gBt[j] = sum over the same samples of sum_k dv_k
//        gW1a = Gi^T gA     gW1b = Gj^T gBt     gb1 = column sums of gBt     gw = sum da_k relu(v_k)     gc = sum da_k
//        gW2 = gw W3^T     gW3 = W2^T gw + gc b2     gb2 = gc W3     gb3 = gc
//      Biases and regulariser are FISM's with beta = 1, lambda = gamma = l_b (el_fism.hip).
//   4. Nothing per pair is stored.  The backward walks recompute s_k, v_k, x_k from the rows they gather anyway and from three
//      numbers kept per sample: r_b, beta N_b / S_b and dL/dx_b.
// THE KERNELS.  A lane group of lpt = min(64, pow2(F)) lanes holds a row of F floats as CPL elements per lane (sub + q lpt) and a row
// of 2F as 2 CPL.  Lists are cut into pieces of `fism_piece` positions; a piece leaves a partial in double, the partials of a list
// are added in ascending piece order by one lane group.  The pieces of all lists are packed by one scan; lane group q takes partial row
// q and finds its list by a binary search in the scanned starts.  The sample-major rows are B + max(B, nnz / piece) whatever the batch
// draws: the piece length of the histories doubles from fism_piece until the batch's pairs fit (k_nais_pe).  Inside a piece a lane group takes lpt positions at a time: all lanes form
// (s_k, a_k) of one position together, lane k keeps them and takes exp() in double for its own position alone.
//   k_nais_fwd      (sample, piece): S, N and sum |Gi[h_k]|^2              k_nais_fwd_fin   out, dL/dx, r, beta N / S, the loss share
//   k_nais_bwd      (sample, piece): sum ds Gi[h_k] | sum dv | sum da relu(v) | sum da       k_nais_bwd_fin   the pieces in order
//   k_nais_seg_item one lane group per item segment of the sorted keys: gGj (before the product), gBt[j], gBi
//   k_nais_seg_user one lane per user segment: gBu
//   k_nais_fan      (item, piece of its user list): Gi[h], A[h] stay in registers; for every user of the piece that is in the batch
//                   (slot[u] >= 0) and every sample of that user's sorted segment the pair is recomputed: ds t_b -> gGi[h], dv -> gA[h]
//   k_nais_fan_fin  the pieces in order, the regulariser's count, row 0's padded slots
//   k_nais_scores   one workgroup: 64 history positions of one user x 64 targets.  The A / Gi rows of the positions and the Bt / Gj
//                   rows of the targets are staged in LDS 32 columns at a time; a lane holds a 4 x 4 block of (position, target)
//                   cells and runs acc += max(a + b, 0) w over it, the similarity Gi[h] . Gj[j] riding in the same loop for the
//                   first F columns (the fp32 matrix instruction's accumulator layout does not meet this block's, so it is not used).
//                   Every 32 columns the float sums go into double cells.  S and N per target are carried across the position tiles
//                   in ascending order; the padded slots are one more position of weight L - n.
// No floating-point atomics, a fixed order in every sum: the same input gives the same bytes.
#include "el_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

#include "el_fism_keys.h"

#define NS_T 64              // positions and targets of a scoring tile
#define NS_KC 32             // columns staged at once

template <int C>
__device__ __forceinline__ void nr_ld(const float* __restrict__ row, int n, int sub, int lpt, float (&r)[C]) {
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int e = sub + q * lpt;
        r[q] = e < n ? row[e] : 0.f;
    }
}
template <int C>
__device__ __forceinline__ void nr_zero(double (&r)[C]) {
#pragma unroll
    for (int q = 0; q < C; ++q) r[q] = 0.0;
}
template <int C, typename T>
__device__ __forceinline__ void nr_st(T* __restrict__ row, int n, int sub, int lpt, const double (&r)[C]) {
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int e = sub + q * lpt;
        if (e < n) row[e] = (T)r[q];
    }
}
// value of lane `t` of this lane's group
__device__ __forceinline__ double nr_bcast(double v, int t, int lpt) { return __shfl(v, (int)((threadIdx.x & 63) & ~(lpt - 1)) + t, 64); }

// (s, a - c) of one pair, the same value in every lane of the group
template <int CPL>
__device__ __forceinline__ void nais_pair(const float (&g)[CPL], const float (&av)[2 * CPL], const float (&t)[CPL], const float (&bt)[2 * CPL],
                                          const float (&w)[2 * CPL], int lpt, double& s, double& a) {
    float ps = 0.f, pa = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) ps = fmaf(g[q], t[q], ps);
#pragma unroll
    for (int q = 0; q < 2 * CPL; ++q) pa = fmaf(fmaxf(av[q] + bt[q], 0.f), w[q], pa);
    s = el_group_sum((double)ps, lpt);
    a = el_group_sum((double)pa, lpt);
}

struct NaisTabs {
    const float *Gi, *A, *Gj, *Bt, *w;
    const double* c;
    const int64_t* h_indptr;
    const int32_t* h_indices;
    int F, lpt, piece;
};

// positions [k0, k1) of a history against one target: S, N, Q = sum |Gi[h_k]|^2 of this piece (the same in every lane)
template <int CPL>
__device__ __forceinline__ void nais_walk_fwd(const NaisTabs& p, int64_t k0, int64_t k1, const float (&t)[CPL], const float (&bt)[2 * CPL],
                                              const float (&w)[2 * CPL], double cc, int sub, double& S, double& N, double& Q) {
    const int F = p.F, lpt = p.lpt;
    double ls = 0.0, ln = 0.0, lq = 0.0;
    for (int64_t base = k0; base < k1; base += lpt) {
        const int cs = (int)(k1 - base < lpt ? k1 - base : lpt);
        double my_s = 0.0, my_a = 0.0;
        for (int tt = 0; tt < cs; ++tt) {
            const int64_t h = p.h_indices[base + tt];
            float g[CPL], av[2 * CPL];
            nr_ld<CPL>(p.Gi + h * F, F, sub, lpt, g);
            nr_ld<2 * CPL>(p.A + h * 2 * F, 2 * F, sub, lpt, av);
            double s, a;
            nais_pair<CPL>(g, av, t, bt, w, lpt, s, a);
#pragma unroll
            for (int q = 0; q < CPL; ++q) lq += (double)g[q] * (double)g[q];
            if (tt == sub) my_s = s, my_a = a;
        }
        if (sub < cs) {
            const double x = exp(my_a + cc);
            ls += x, ln += x * my_s;
        }
    }
    S = el_group_sum(ls, lpt), N = el_group_sum(ln, lpt), Q = el_group_sum(lq, lpt);
}

struct NaisStep {
    NaisTabs t;
    const int32_t *bu, *bi;
    int64_t B, scap;
    const int64_t* pe;      // positions per piece of this batch's histories (k_nais_pe)
    const int64_t* sstart;  // [B + 1] first partial row of a sample: the exclusive scan of the samples' piece counts
    double* pfw;         // [scap, 3]  S, N, Q of a piece
    double* pbw;         // [scap, 5F + 1]  the backward partial rows
    const double *R, *NS;   // [B] r_b and beta N_b / S_b
};

// last list whose first partial row is <= q (start[0] = 0, start ascending over n + 1 entries)
__device__ __forceinline__ int64_t nais_list_of(const int64_t* __restrict__ start, int64_t n, int64_t q) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (start[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// the (sample, piece) of a lane group: lane group q takes partial row q of the packed rows; false: none
__device__ __forceinline__ bool nais_piece_of(const NaisStep& p, int64_t& b, int64_t& q, int64_t& k0, int64_t& k1) {
    q = ((int64_t)blockIdx.x * 256 + threadIdx.x) / p.t.lpt;
    if (q >= p.scap || q >= p.sstart[p.B]) return false;
    b = nais_list_of(p.sstart, p.B, q);
    const int64_t u = p.bu[b], r0 = p.t.h_indptr[u], r1 = p.t.h_indptr[u + 1], pe = *p.pe;
    k0 = r0 + (q - p.sstart[b]) * pe;
    if (k0 > r1) k0 = r1;
    k1 = k0 + pe < r1 ? k0 + pe : r1;
    return true;
}

// The sample-major scratch holds scap = B + room partial rows whatever the histories are.  The batch's pairs P = sum_b n_{u_b} are
// counted first; the piece length is fism_piece, doubled until B + P / pe <= scap: a sample has max(1, ceil(n / pe)) pieces.
__global__ __launch_bounds__(256) void k_nais_pe(const int32_t* __restrict__ bu, const int64_t* __restrict__ h_indptr, int64_t B, int piece,
                                                 int64_t room, int64_t* pe_out) {
    __shared__ unsigned long long red[256];
    unsigned long long a = 0;
    for (int64_t b = threadIdx.x; b < B; b += 256) a += (unsigned long long)(h_indptr[bu[b] + 1] - h_indptr[bu[b]]);
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        unsigned long long pe = (unsigned long long)piece;
        while (pe * (unsigned long long)room < red[0]) pe <<= 1;
        *pe_out = (int64_t)pe;
    }
}
__global__ __launch_bounds__(256) void k_nais_splen(const int32_t* __restrict__ bu, const int64_t* __restrict__ h_indptr, int64_t B,
                                                    const int64_t* __restrict__ pe, int64_t* __restrict__ plen) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > B) return;
    const int64_t len = b < B ? h_indptr[bu[b] + 1] - h_indptr[bu[b]] : 0;
    plen[b] = b < B ? (len <= *pe ? 1 : (len + *pe - 1) / *pe) : 0;
}

template <int CPL>
__global__ __launch_bounds__(256) void k_nais_fwd(NaisStep p) {
    int64_t b, q, k0, k1;
    if (!nais_piece_of(p, b, q, k0, k1)) return;
    const int F = p.t.F, lpt = p.t.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t j = p.bi[b];
    float t[CPL], bt[2 * CPL], w[2 * CPL];
    nr_ld<CPL>(p.t.Gj + j * F, F, sub, lpt, t);
    nr_ld<2 * CPL>(p.t.Bt + j * 2 * F, 2 * F, sub, lpt, bt);
    nr_ld<2 * CPL>(p.t.w, 2 * F, sub, lpt, w);
    double S, N, Q;
    nais_walk_fwd<CPL>(p.t, k0, k1, t, bt, w, *p.t.c, sub, S, N, Q);
    if (sub == 0) {
        double* o = p.pfw + q * 3;
        o[0] = S, o[1] = N, o[2] = Q;
    }
}

struct NaisFin {
    NaisStep s;
    const float *Bu, *Bi, *coef, *label;
    double* cb;          // [B] dL/dx_b
    double *R, *NS, *lossb, *padb;
    int64_t pad_len;
    int loss_kind;
    float beta, l_b;
    double inv_n;
};

// one lane group per sample: the pieces in order, out, dL/dx, the loss share with the regulariser
template <int CPL>
__global__ __launch_bounds__(256) void k_nais_fwd_fin(NaisFin p) {
    const NaisTabs& tb = p.s.t;
    const int F = tb.F, lpt = tb.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    if (b >= p.s.B) return;
    const int64_t u = p.s.bu[b], j = p.s.bi[b], n = tb.h_indptr[u + 1] - tb.h_indptr[u];
    const int64_t p0 = p.s.sstart[b], p1 = p.s.sstart[b + 1] < p.s.scap ? p.s.sstart[b + 1] : p.s.scap;
    double S = 0.0, N = 0.0, Q = 0.0;
    for (int64_t k = p0; k < p1; ++k) {
        const double* o = p.s.pfw + k * 3;
        S += o[0], N += o[1], Q += o[2];
    }
    float t[CPL], g0[CPL];
    nr_ld<CPL>(tb.Gj + j * F, F, sub, lpt, t);
    nr_ld<CPL>(tb.Gi, F, sub, lpt, g0);
    double tsq = 0.0, gsq = 0.0;
#pragma unroll
    for (int q = 0; q < CPL; ++q) tsq += (double)t[q] * (double)t[q], gsq += (double)g0[q] * (double)g0[q];
    tsq = el_group_sum(tsq, lpt), gsq = el_group_sum(gsq, lpt);
    if (sub != 0) return;
    const double beta = (double)p.beta, cf = (double)p.coef[u], sb = S > 0.0 ? pow(S, -beta) : 0.0;
    const float bu = p.Bu[u], bi = p.Bi[j];
    const double od = 1.0 / (1.0 + exp(-(cf * N * sb + (double)bu + (double)bi)));
    const double y = (double)p.label[b], eps = 1e-7;
    double data, d;
    if (p.loss_kind == EL_FISM_LOSS_REFERENCE) {          // Keras BCE(y_true = out, y_pred = label): linear in out
        const double yh = y < eps ? eps : (y > 1.0 - eps ? 1.0 - eps : y);
        const double la = log(yh + eps), lb = log(1.0 - yh + eps);
        data = -(od * la + (1.0 - od) * lb);
        d = -(la - lb);
    } else {                                              // the cross-entropy that was meant
        const double pc = od < eps ? eps : (od > 1.0 - eps ? 1.0 - eps : od);
        const bool pass = od >= eps && od <= 1.0 - eps;
        data = y > 0.0 ? -log(pc + eps) : -log(1.0 - pc + eps);
        d = !pass ? 0.0 : (y > 0.0 ? -1.0 / (pc + eps) : 1.0 / (1.0 - pc + eps));
    }
    const double cb = d * p.inv_n * (od * (1.0 - od));            // (kept in double: gc and the bias sums cancel between samples)
    p.cb[b] = cb;
    p.R[b] = cb * cf * sb;
    p.NS[b] = S > 0.0 ? beta * N / S : 0.0;
    const double padn = p.pad_len > n ? (double)(p.pad_len - n) : 0.0;
    p.padb[b] = padn;
    p.lossb[b] = data * p.inv_n + 0.5 * ((double)p.l_b * ((double)(bu * bu) + (double)(bi * bi)) + tsq + Q + padn * gsq);
}

// a partial row of the backward walk: [0, F) sum ds Gi[h_k], [F, 3F) sum dv_k, [3F, 5F) sum da_k relu(v_k), [5F] sum da_k
template <int CPL>
__global__ __launch_bounds__(256) void k_nais_bwd(NaisStep p) {
    int64_t b, q, k0, k1;
    if (!nais_piece_of(p, b, q, k0, k1)) return;
    const NaisTabs& tb = p.t;
    const int F = tb.F, lpt = tb.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t j = p.bi[b];
    float t[CPL], bt[2 * CPL], w[2 * CPL];
    nr_ld<CPL>(tb.Gj + j * F, F, sub, lpt, t);
    nr_ld<2 * CPL>(tb.Bt + j * 2 * F, 2 * F, sub, lpt, bt);
    nr_ld<2 * CPL>(tb.w, 2 * F, sub, lpt, w);
    const double cc = *tb.c, r = p.R[b], ns = p.NS[b];
    double aT[CPL], aB[2 * CPL], aW[2 * CPL], gc = 0.0;
    nr_zero<CPL>(aT), nr_zero<2 * CPL>(aB), nr_zero<2 * CPL>(aW);
    for (int64_t base = k0; base < k1; base += lpt) {
        const int cs = (int)(k1 - base < lpt ? k1 - base : lpt);
        double my_s = 0.0, my_a = 0.0;
        for (int tt = 0; tt < cs; ++tt) {
            const int64_t h = tb.h_indices[base + tt];
            float g[CPL], av[2 * CPL];
            nr_ld<CPL>(tb.Gi + h * F, F, sub, lpt, g);
            nr_ld<2 * CPL>(tb.A + h * 2 * F, 2 * F, sub, lpt, av);
            double s, a;
            nais_pair<CPL>(g, av, t, bt, w, lpt, s, a);
            if (tt == sub) my_s = s, my_a = a;
        }
        double my_ds = 0.0, my_da = 0.0;
        if (sub < cs) {
            my_ds = r * exp(my_a + cc);
            my_da = my_ds * (my_s - ns);
        }
        for (int tt = 0; tt < cs; ++tt) {
            const int64_t h = tb.h_indices[base + tt];
            const double ds = nr_bcast(my_ds, tt, lpt), da = nr_bcast(my_da, tt, lpt);
            float g[CPL], av[2 * CPL];
            nr_ld<CPL>(tb.Gi + h * F, F, sub, lpt, g);
            nr_ld<2 * CPL>(tb.A + h * 2 * F, 2 * F, sub, lpt, av);
#pragma unroll
            for (int q = 0; q < CPL; ++q) aT[q] += ds * (double)g[q];
#pragma unroll
            for (int q = 0; q < 2 * CPL; ++q) {
                const float v = av[q] + bt[q];
                if (v > 0.f) aB[q] += da * (double)w[q], aW[q] += da * (double)v;
            }
            gc += da;
        }
    }
    double* o = p.pbw + q * (5 * F + 1);
    nr_st<CPL>(o, F, sub, lpt, aT);
    nr_st<2 * CPL>(o + F, 2 * F, sub, lpt, aB);
    nr_st<2 * CPL>(o + 3 * F, 2 * F, sub, lpt, aW);
    if (sub == 0) o[5 * F] = gc;
}

// the pieces of a sample in order: rowS[b] = [sum ds Gi | sum dv] (3F), gwS[b] = [sum da relu(v) | sum da] (2F + 1).  The gw / gc
// shares stay in double: they are rounded once, after the sum over the samples.
__global__ __launch_bounds__(256) void k_nais_bwd_fin(NaisStep p, float* __restrict__ rowS, double* __restrict__ gwS) {
    const int F = p.t.F, W = 5 * F + 1;
    const int64_t b = blockIdx.x;
    const int64_t p0 = p.sstart[b], p1 = p.sstart[b + 1] < p.scap ? p.sstart[b + 1] : p.scap;
    for (int e = threadIdx.x; e < W; e += blockDim.x) {
        double acc = 0.0;
        for (int64_t k = p0; k < p1; ++k) acc += p.pbw[k * W + e];
        if (e < 3 * F) rowS[b * 3 * F + e] = (float)acc;
        else gwS[b * (2 * F + 1) + (e - 3 * F)] = acc;
    }
}

// Column sums in a fixed order, in double, on two levels: part[g, c] = sum of src[r, c] over the rows [g NC_ROWS, + NC_ROWS) in
// ascending order, then out[c] = sum of part[g, c] in ascending g.
#define NC_ROWS 128
template <typename T>
__global__ __launch_bounds__(256) void k_nais_colsum(const T* __restrict__ src, int64_t R, int64_t C, double* __restrict__ part) {
    const int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x, r0 = (int64_t)blockIdx.x * NC_ROWS;
    if (c >= C) return;
    const int64_t r1 = r0 + NC_ROWS < R ? r0 + NC_ROWS : R;
    double acc = 0.0;
    for (int64_t r = r0; r < r1; r += 8) {
        T v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = r + k < r1 ? src[(r + k) * C + c] : (T)0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += (double)v[k];
    }
    part[(int64_t)blockIdx.x * C + c] = acc;
}
__global__ __launch_bounds__(256) void k_nais_colsum_fin(const double* __restrict__ part, int64_t G, int64_t C, float* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double acc = 0.0;
    for (int64_t g = 0; g < G; ++g) acc += part[g * C + c];
    out[c] = (float)acc;
}

// tot[0] = sum lossb, tot[1] = sum padb: lane t adds b = t, t + 256, ... in order, the 256 sums through a fixed tree
__global__ __launch_bounds__(256) void k_nais_sums(const double* __restrict__ lossb, const double* __restrict__ padb, int64_t B, double* tot) {
    __shared__ double red[2][256];
    double a = 0.0, c = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += 256) a += lossb[b], c += padb[b];
    red[0][threadIdx.x] = a, red[1][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[0][threadIdx.x] += red[0][threadIdx.x + o], red[1][threadIdx.x] += red[1][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[0] = red[0][0], tot[1] = red[1][0];
}

__global__ __launch_bounds__(256) void k_nais_zero(float* __restrict__ p, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) p[e] = 0.f;
}
// dst[r, :F] += src[r, :F]
__global__ __launch_bounds__(256) void k_nais_add(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) dst[e] += src[e];
}

struct NaisSeg {
    const u32 *keys, *vals;     // the item half of the sorted keys (U + j) and the sample of each position
    u32 key_off;
    int64_t B;
    const float *rowS, *Gj, *Bi;
    const double* cb;
    float *gGj, *gBt, *gBi;
    float l_b;
    int F, lpt;
};

// one lane group per head of an item segment: the segment's samples in sorted order (ascending b: the sort is stable)
template <int CPL>
__global__ __launch_bounds__(256) void k_nais_seg_item(NaisSeg p) {
    const int F = p.F, lpt = p.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t pos = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    if (pos >= p.B) return;
    const u32 key = p.keys[pos];
    if (pos > 0 && p.keys[pos - 1] == key) return;
    const int64_t j = (int64_t)(key - p.key_off);
    double acc[3 * CPL], cs = 0.0;
    nr_zero<3 * CPL>(acc);
    int64_t m = 0;
    for (int64_t q = pos; q < p.B && p.keys[q] == key; ++q, ++m) {
        const int64_t b = p.vals[q];
        float r[3 * CPL];
        nr_ld<3 * CPL>(p.rowS + b * 3 * F, 3 * F, sub, lpt, r);
#pragma unroll
        for (int x = 0; x < 3 * CPL; ++x) acc[x] += (double)r[x];
        cs += p.cb[b];
    }
    // elements [0, F) -> gGj[j] with the regulariser m Gj[j]; [F, 3F) -> gBt[j]
#pragma unroll
    for (int x = 0; x < 3 * CPL; ++x) {
        const int e = sub + x * lpt;
        if (e < F) p.gGj[j * F + e] = (float)(acc[x] + (double)m * (double)p.Gj[j * F + e]);
        else if (e < 3 * F) p.gBt[j * 2 * F + (e - F)] = (float)acc[x];
    }
    if (sub == 0) p.gBi[j] = (float)(cs + (double)p.l_b * (double)m * (double)p.Bi[j]);
}

__global__ __launch_bounds__(256) void k_nais_seg_user(const u32* __restrict__ keys, const u32* __restrict__ vals, int64_t B, int64_t U,
                                                       const double* __restrict__ cb, const float* __restrict__ Bu, float l_b,
                                                       float* __restrict__ gBu) {
    const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= B) return;
    const u32 key = keys[pos];
    if ((pos > 0 && keys[pos - 1] == key) || (int64_t)key >= U) return;
    double cs = 0.0;
    int64_t m = 0;
    for (int64_t q = pos; q < B && keys[q] == key; ++q, ++m) cs += cb[vals[q]];
    gBu[key] = (float)(cs + (double)l_b * (double)m * (double)Bu[key]);
}

__global__ __launch_bounds__(256) void k_nais_plen(const int64_t* __restrict__ indptr, int64_t nl, int piece, int64_t* __restrict__ plen) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l > nl) return;
    const int64_t len = l < nl ? indptr[l + 1] - indptr[l] : 0;
    plen[l] = l < nl ? (len <= piece ? 1 : (len + piece - 1) / piece) : 0;
}

struct NaisFan {
    NaisTabs t;
    const int64_t* t_indptr;
    const int32_t* t_indices;
    const int32_t *slot, *bi;
    const u32 *keys, *vals;     // the user half of the sorted keys
    int64_t B, I, pcap;
    const double *R, *NS;
    const int64_t* pstart;      // [I + 1] first partial row of an item
    double* part;               // [pcap, 3F + 1]: sum ds t_b | sum dv | pairs
    const double* tot;          // tot[1] = sum_b (L - n_{u_b})
    float *gGi, *gA;
};

// (item, piece of its user list), the pieces packed by the scan of k_nais_plen
template <int CPL>
__global__ __launch_bounds__(256) void k_nais_fan(NaisFan p) {
    const NaisTabs& tb = p.t;
    const int F = tb.F, lpt = tb.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t prow = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;      // lane group q takes partial row q of the packed rows
    if (prow >= p.pcap || prow >= p.pstart[p.I]) return;
    const int64_t h = nais_list_of(p.pstart, p.I, prow);
    const int64_t r0 = p.t_indptr[h], r1 = p.t_indptr[h + 1];
    int64_t k0 = r0 + (prow - p.pstart[h]) * tb.piece;
    if (k0 > r1) k0 = r1;
    const int64_t k1 = k0 + tb.piece < r1 ? k0 + tb.piece : r1;
    float g[CPL], av[2 * CPL], w[2 * CPL];
    nr_ld<CPL>(tb.Gi + h * F, F, sub, lpt, g);
    nr_ld<2 * CPL>(tb.A + h * 2 * F, 2 * F, sub, lpt, av);
    nr_ld<2 * CPL>(tb.w, 2 * F, sub, lpt, w);
    const double cc = *tb.c;
    double aG[CPL], aA[2 * CPL], pairs = 0.0;
    nr_zero<CPL>(aG), nr_zero<2 * CPL>(aA);
    const int lane = (int)(threadIdx.x & 63), gbase = lane & ~(lpt - 1);
    const u64 gmask = lpt >= 64 ? ~0ull : (((1ull << lpt) - 1ull) << gbase);
    for (int64_t base = k0; base < k1; base += lpt) {
        const int32_t uu = base + sub < k1 ? p.t_indices[base + sub] : -1;
        const bool in = uu >= 0 && p.slot[uu] >= 0;
        u64 m = __ballot(in) & gmask;
        while (m) {                                                  // the users of the batch among these lpt, ascending
            const int src = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const u32 user = (u32)__shfl(uu, src, 64);
            for (int64_t q = fi_first(p.keys, p.B, user); q < p.B && p.keys[q] == user; ++q) {
                const int64_t b = p.vals[q], j = p.bi[b];
                float t[CPL], bt[2 * CPL];
                nr_ld<CPL>(tb.Gj + j * F, F, sub, lpt, t);
                nr_ld<2 * CPL>(tb.Bt + j * 2 * F, 2 * F, sub, lpt, bt);
                double s, a;
                nais_pair<CPL>(g, av, t, bt, w, lpt, s, a);
                const double ds = p.R[b] * exp(a + cc), da = ds * (s - p.NS[b]);
#pragma unroll
                for (int x = 0; x < CPL; ++x) aG[x] += ds * (double)t[x];
#pragma unroll
                for (int x = 0; x < 2 * CPL; ++x)
                    if (av[x] + bt[x] > 0.f) aA[x] += da * (double)w[x];
                pairs += 1.0;
            }
        }
    }
    double* o = p.part + prow * (3 * F + 1);
    nr_st<CPL>(o, F, sub, lpt, aG);
    nr_st<2 * CPL>(o + F, 2 * F, sub, lpt, aA);
    if (sub == 0) o[3 * F] = pairs;
}

// the pieces of an item in order; gGi[h] = sum ds t + pairs Gi[h] (+ Gi[0] sum_b (L - n_{u_b}) for h = 0), gA[h] = sum dv
__global__ __launch_bounds__(256) void k_nais_fan_fin(NaisFan p) {
    const int F = p.t.F, W = 3 * F + 1;
    const int64_t h = blockIdx.x;
    const int64_t p0 = p.pstart[h], p1 = p.pstart[h + 1] < p.pcap ? p.pstart[h + 1] : p.pcap;
    double pairs = 0.0;
    for (int64_t k = p0; k < p1; ++k) pairs += p.part[k * W + 3 * F];
    if (h == 0) pairs += p.tot[1];
    for (int e = threadIdx.x; e < 3 * F; e += blockDim.x) {
        double acc = 0.0;
        for (int64_t k = p0; k < p1; ++k) acc += p.part[k * W + e];
        if (e < F) p.gGi[h * F + e] = (float)(acc + pairs * (double)p.t.Gi[h * F + e]);
        else p.gA[h * 2 * F + (e - F)] = (float)acc;
    }
}

// w = W2 W3, c = b2 . W3 + b3
__global__ __launch_bounds__(256) void k_nais_collapse(const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
                                                       const float* __restrict__ b3, int F2, int Ws, float* __restrict__ w, double* c) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e > F2) return;
    double acc = 0.0;
    if (e < F2) {
        for (int s = 0; s < Ws; ++s) acc += (double)W2[(int64_t)e * Ws + s] * (double)W3[s];
        w[e] = (float)acc;
    } else {
        for (int s = 0; s < Ws; ++s) acc += (double)b2[s] * (double)W3[s];
        *c = acc + (double)b3[0];
    }
}

// gwc = [gw (2F) | gc]:  gW2 = gw W3^T, gW3 = W2^T gw + gc b2, gb2 = gc W3, gb3 = gc
__global__ __launch_bounds__(256) void k_nais_mlp_grads(const float* __restrict__ gwc, const float* __restrict__ W2, const float* __restrict__ b2,
                                                        const float* __restrict__ W3, int F2, int Ws, float* __restrict__ gW2,
                                                        float* __restrict__ gW3, float* __restrict__ gb2, float* __restrict__ gb3) {
    const int64_t n = (int64_t)F2 * Ws, stride = (int64_t)gridDim.x * 256, id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t x = id; x < n; x += stride) gW2[x] = gwc[x / Ws] * W3[x % Ws];
    const float gc = gwc[F2];
    for (int64_t s = id; s < Ws; s += stride) {
        double acc = 0.0;
        for (int e = 0; e < F2; ++e) acc += (double)W2[(int64_t)e * Ws + s] * (double)gwc[e];
        gW3[s] = (float)(acc + (double)gc * (double)b2[s]);
        gb2[s] = gc * W3[s];
    }
    if (id == 0) gb3[0] = gc;
}

__global__ __launch_bounds__(256) void k_nais_finish(const int32_t* __restrict__ rows, const int32_t* __restrict__ n_dev,
                                                     int32_t* __restrict__ slot, const double* __restrict__ tot, double* loss_out) {
    const int64_t n = *n_dev, stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) slot[rows[s]] = -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) *loss_out += tot[0];
}

// ---- scoring ------------------------------------------------------------------------------------------------------------------
struct NaisPred {
    NaisTabs t;
    const float *Bu, *Bi, *coef;
    int64_t pad_len;
    float beta;
};

__device__ __forceinline__ float nais_out(double S, double N, double beta, double cf, float bu, float bi) {
    const double prod = S > 0.0 ? cf * N * pow(S, -beta) : 0.0;
    return (float)(1.0 / (1.0 + exp(-(prod + (double)bu + (double)bi))));
}

// explicit pairs: one lane group walks the whole history, then the padded slots as one position of weight L - n
template <int CPL>
__global__ __launch_bounds__(256) void k_nais_pairs(NaisPred p, const int32_t* __restrict__ bu, const int32_t* __restrict__ bi, int64_t n,
                                                    float* __restrict__ out) {
    const NaisTabs& tb = p.t;
    const int F = tb.F, lpt = tb.lpt, sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    if (b >= n) return;
    const int64_t u = bu[b], j = bi[b], r0 = tb.h_indptr[u], r1 = tb.h_indptr[u + 1];
    float t[CPL], bt[2 * CPL], w[2 * CPL];
    nr_ld<CPL>(tb.Gj + j * F, F, sub, lpt, t);
    nr_ld<2 * CPL>(tb.Bt + j * 2 * F, 2 * F, sub, lpt, bt);
    nr_ld<2 * CPL>(tb.w, 2 * F, sub, lpt, w);
    const double cc = *tb.c;
    double S, N, Q;
    nais_walk_fwd<CPL>(tb, r0, r1, t, bt, w, cc, sub, S, N, Q);
    if (p.pad_len > r1 - r0) {
        float g[CPL], av[2 * CPL];
        nr_ld<CPL>(tb.Gi, F, sub, lpt, g);
        nr_ld<2 * CPL>(tb.A, 2 * F, sub, lpt, av);
        double s, a;
        nais_pair<CPL>(g, av, t, bt, w, lpt, s, a);
        const double x = (double)(p.pad_len - (r1 - r0)) * exp(a + cc);
        S += x, N += x * s;
    }
    if (sub == 0) out[b] = nais_out(S, N, (double)p.beta, (double)p.coef[u], p.Bu[u], p.Bi[j]);
}

// one workgroup: user u_start + blockIdx.y, targets [64 blockIdx.x, + 64), every tile of 64 positions in ascending order
__global__ __launch_bounds__(256) void k_nais_scores(NaisPred p, int64_t I, int64_t u_start, float* __restrict__ out, int64_t ld) {
    __shared__ float sA[NS_T][NS_KC + 1], sB[NS_T][NS_KC + 1], sG[NS_T][NS_KC + 1], sJ[NS_T][NS_KC + 1];
    __shared__ float sW[NS_KC], sWt[NS_T];
    __shared__ int32_t sH[NS_T];
    __shared__ double sRed[2][16][NS_T];
    const NaisTabs& tb = p.t;
    const int F = tb.F, F2 = 2 * F, tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t u = u_start + blockIdx.y, j0 = (int64_t)blockIdx.x * NS_T;
    const int64_t r0 = tb.h_indptr[u], n = tb.h_indptr[u + 1] - r0;
    const int64_t padn = p.pad_len > n ? p.pad_len - n : 0, np = n + (padn > 0 ? 1 : 0);
    const double cc = *tb.c;
    double S = 0.0, N = 0.0;                                        // of target j0 + tid in the lanes tid < 64
    for (int64_t pt = 0; pt < np; pt += NS_T) {
        if (tid < NS_T) {
            const int64_t k = pt + tid;
            sH[tid] = k < n ? tb.h_indices[r0 + k] : 0;
            sWt[tid] = k < n ? 1.f : (k < np ? (float)padn : 0.f);
        }
        __syncthreads();
        double accA[4][4], accS[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) accA[r][c] = 0.0, accS[r][c] = 0.0;
        for (int e0 = 0; e0 < F2; e0 += NS_KC) {
            const bool sim = e0 < F;
#pragma unroll
            for (int i = 0; i < NS_T * NS_KC / 256; ++i) {
                const int idx = tid + 256 * i, row = idx / NS_KC, col = idx % NS_KC, e = e0 + col;
                const int64_t hh = sH[row], jj = j0 + row;
                const bool okj = jj < I;
                sA[row][col] = e < F2 ? tb.A[hh * F2 + e] : 0.f;
                sB[row][col] = (okj && e < F2) ? tb.Bt[jj * F2 + e] : 0.f;
                if (sim) {
                    sG[row][col] = e < F ? tb.Gi[hh * F + e] : 0.f;
                    sJ[row][col] = (okj && e < F) ? tb.Gj[jj * F + e] : 0.f;
                }
            }
            if (tid < NS_KC) sW[tid] = e0 + tid < F2 ? tb.w[e0 + tid] : 0.f;
            __syncthreads();
            float fa[4][4], fs[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) fa[r][c] = 0.f, fs[r][c] = 0.f;
#pragma unroll 8
            for (int e = 0; e < NS_KC; ++e) {
                float a[4], bb[4];
                const float wv = sW[e];
#pragma unroll
                for (int r = 0; r < 4; ++r) a[r] = sA[ty + 16 * r][e], bb[r] = sB[tx + 16 * r][e];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) fa[r][c] = fmaf(fmaxf(a[r] + bb[c], 0.f), wv, fa[r][c]);
            }
            if (sim) {
#pragma unroll 8
                for (int e = 0; e < NS_KC; ++e) {
                    float a[4], bb[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] = sG[ty + 16 * r][e], bb[r] = sJ[tx + 16 * r][e];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) fs[r][c] = fmaf(a[r], bb[c], fs[r][c]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) accA[r][c] += (double)fa[r][c], accS[r][c] += (double)fs[r][c];
            __syncthreads();
        }
        double ps[4] = {0.0, 0.0, 0.0, 0.0}, pn[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float wt = sWt[ty + 16 * r];
            if (wt > 0.f) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double x = (double)wt * exp(accA[r][c] + cc);
                    ps[c] += x, pn[c] += x * accS[r][c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) sRed[0][ty][tx + 16 * c] = ps[c], sRed[1][ty][tx + 16 * c] = pn[c];
        __syncthreads();
        if (tid < NS_T) {
            for (int h = 0; h < 16; ++h) S += sRed[0][h][tid], N += sRed[1][h][tid];
        }
        __syncthreads();
    }
    if (tid < NS_T && j0 + tid < I)
        out[(int64_t)blockIdx.y * ld + j0 + tid] = nais_out(S, N, (double)p.beta, (double)p.coef[u], p.Bu[u], p.Bi[j0 + tid]);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
int nais_piece(el_ctx* ctx) {
    const double v = ctx->opt.fism_piece;
    const int p = (int)v;
    return ((double)p == v && p >= 8 && p <= 4096 && (p & (p - 1)) == 0) ? p : 0;
}
int nais_lpt(int F, int* cpl) {
    const int lpt = F >= 64 ? 64 : el_pow2(F);
    const int c = (F + lpt - 1) / lpt;
    *cpl = c <= 1 ? 1 : (c == 2 ? 2 : 4);
    return lpt;
}

#define NA_DISPATCH(cpl, CALL) \
    do {                       \
        if ((cpl) == 1) CALL(1); \
        else if ((cpl) == 2) CALL(2); \
        else CALL(4);          \
    } while (0)

// A, Bt, w, c of the current weights and the scratch of the products
struct NaisPrepWs {
    float *A, *Bt, *w;
    double* c;
    void* gemm;
    size_t gemm_bytes;
};
void nais_prep_carve(el_ctx* ctx, ElCarve& c, const el_nais_state* st, int64_t rows_max, NaisPrepWs* w) {
    const int64_t I = st->I, F = st->F;
    w->A = c.take<float>((size_t)(I * 2 * F));
    w->Bt = c.take<float>((size_t)(I * 2 * F));
    w->w = c.take<float>((size_t)(2 * F));
    w->c = c.take<double>(1);
    size_t g = el_gemm_ws_bytes(ctx, rows_max, 2 * F, F);
    const size_t g2 = el_gemm_ws_bytes(ctx, F, 2 * F, rows_max), g3 = el_gemm_ws_bytes(ctx, rows_max, F, 2 * F);
    g = g > g2 ? g : g2;
    w->gemm_bytes = g > g3 ? g : g3;
    w->gemm = c.take<char>(w->gemm_bytes);
}
int nais_prepare(el_ctx* ctx, hipStream_t s, const el_nais_state* st, const NaisPrepWs& w) {
    const int64_t I = st->I, F = st->F, F2 = 2 * F;
    if (int rc = el_gemm_f32(ctx, s, 0, 0, I, F2, F, st->Gi, F, st->W1, F2, w.A, F2, nullptr, 0, w.gemm, w.gemm_bytes)) return rc;
    if (int rc = el_gemm_f32(ctx, s, 0, 0, I, F2, F, st->Gj, F, st->W1 + F * F2, F2, w.Bt, F2, st->b1, 0, w.gemm, w.gemm_bytes)) return rc;
    EL_LAUNCH("k_nais_collapse", k_nais_collapse, dim3((unsigned)((F2 + 256) / 256)), dim3(256), 0, s, st->W2, st->b2, st->W3, st->b3, (int)F2,
              st->Ws, w.w, w.c);
    return 0;
}

struct NaisWs {
    NaisPrepWs prep;
    u32 *key_in, *val_in, *key, *val;
    int32_t *hd, *hs, *rows, *n_dev, *split;
    u64* uplen;
    float *rowS, *gwc, *gBt, *gA, *tmp;
    double *cb, *R, *NS, *lossb, *padb, *tot, *pfw, *pbw, *part, *gwS, *cpart;
    int64_t *plen, *pstart, *splen, *sstart, *pe;
    void *sort_tmp, *scan_tmp, *scan64_tmp;
    size_t sort_bytes, scan_bytes, scan64_bytes, total;
    int64_t n_max, scap, pcap;
};

int nais_carve(el_ctx* ctx, const el_nais_state* st, int64_t B, void* base, NaisWs* w) {
    ElCarve c{(char*)base};
    const int64_t U = st->U, I = st->I, F = st->F, n_max = B < U ? B : U;
    const int piece = nais_piece(ctx);
    w->n_max = n_max;
    // partial rows: a sample and an item have one each, plus one per `piece` positions.  The item lists hold nnz positions; the
    // batch's histories hold what the batch draws, so their piece length grows until max(B, nnz / piece) further rows do (k_nais_pe)
    w->pcap = I + st->nnz / piece;
    w->scap = B + (B > st->nnz / piece ? B : st->nnz / piece);
    nais_prep_carve(ctx, c, st, I, &w->prep);
    w->key_in = c.take<u32>((size_t)(2 * B));
    w->val_in = c.take<u32>((size_t)(2 * B));
    w->key = c.take<u32>((size_t)(2 * B));
    w->val = c.take<u32>((size_t)(2 * B));
    w->hd = c.take<int32_t>((size_t)B);
    w->hs = c.take<int32_t>((size_t)B);
    w->rows = c.take<int32_t>((size_t)n_max);
    w->n_dev = c.take<int32_t>(1);
    w->split = c.take<int32_t>(2);
    w->uplen = c.take<u64>((size_t)(n_max + 1));
    w->cb = c.take<double>((size_t)B);
    w->rowS = c.take<float>((size_t)(B * 3 * F));
    w->gwc = c.take<float>((size_t)(2 * F + 1));
    w->gBt = c.take<float>((size_t)(I * 2 * F));
    w->gA = c.take<float>((size_t)(I * 2 * F));
    w->tmp = c.take<float>((size_t)(I * F));
    w->R = c.take<double>((size_t)B);
    w->NS = c.take<double>((size_t)B);
    w->lossb = c.take<double>((size_t)B);
    w->padb = c.take<double>((size_t)B);
    w->tot = c.take<double>(2);
    w->gwS = c.take<double>((size_t)(B * (2 * F + 1)));
    w->cpart = c.take<double>((size_t)((((B > I ? B : I) + NC_ROWS - 1) / NC_ROWS) * (2 * F + 1)));
    w->pfw = c.take<double>((size_t)(w->scap * 3));
    w->pbw = c.take<double>((size_t)(w->scap * (5 * F + 1)));
    w->part = c.take<double>((size_t)(w->pcap * (3 * F + 1)));
    w->plen = c.take<int64_t>((size_t)(I + 1));
    w->pstart = c.take<int64_t>((size_t)(I + 1));
    w->splen = c.take<int64_t>((size_t)(B + 1));
    w->sstart = c.take<int64_t>((size_t)(B + 1));
    w->pe = c.take<int64_t>(1);
    size_t t1 = 0, t2 = 0, t3 = 0;
    u32* np = nullptr;
    int32_t* ip = nullptr;
    int64_t* lp = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (unsigned)(2 * B), 0, el_bits_for(U + I), (hipStream_t)0) != hipSuccess) return 1;
    if (rocprim::exclusive_scan(nullptr, t2, ip, ip, (int32_t)0, (size_t)B, rocprim::plus<int32_t>(), (hipStream_t)0) != hipSuccess) return 1;
    if (rocprim::exclusive_scan(nullptr, t3, lp, lp, (int64_t)0, (size_t)(I + 1), rocprim::plus<int64_t>(), (hipStream_t)0) != hipSuccess) return 1;
    size_t t4 = 0;
    if (rocprim::exclusive_scan(nullptr, t4, lp, lp, (int64_t)0, (size_t)(B + 1), rocprim::plus<int64_t>(), (hipStream_t)0) != hipSuccess) return 1;
    w->sort_bytes = t1, w->scan_bytes = t2, w->scan64_bytes = t3 > t4 ? t3 : t4;
    w->sort_tmp = c.take<char>(t1);
    w->scan_tmp = c.take<char>(t2);
    w->scan64_tmp = c.take<char>(w->scan64_bytes);                 // (both int64 scans use it: over I + 1 and over B + 1 entries)
    w->total = c.off;
    return 0;
}

int nais_check_state(el_ctx* ctx, const el_nais_state* st, const char* who, int level) {      // 0: scoring, 1: + accumulators, 2: + Adam slots
    EL_REQUIRE(st != nullptr, "%s: null state", who);
    EL_REQUIRE(st->U > 0 && st->I > 0 && st->nnz >= 0, "%s: bad shape U=%lld I=%lld nnz=%lld", who, (long long)st->U, (long long)st->I,
               (long long)st->nnz);
    EL_REQUIRE(st->F >= 1 && st->F <= 256, "%s: F=%d out of range (1 .. 256)", who, st->F);
    EL_REQUIRE(st->Ws >= 1 && st->Ws < (1 << 20), "%s: Ws=%d out of range", who, st->Ws);
    EL_REQUIRE(st->U + st->I < (1LL << 32) && st->nnz < (1LL << 40), "%s: U + I must fit a 32-bit sort key", who);
    EL_REQUIRE(st->Gi && st->Gj && st->Bu && st->Bi && st->W1 && st->b1 && st->W2 && st->b2 && st->W3 && st->b3, "%s: null variable", who);
    EL_REQUIRE(st->coef != nullptr, "%s: coef is NULL (n_u^-alpha is computed by the caller)", who);
    EL_REQUIRE(st->h_indptr && st->h_indices && st->t_indptr && st->t_indices, "%s: needs the train matrix user-major and item-major", who);
    EL_REQUIRE(st->pad_len >= 0 && st->pad_len < (1LL << 24), "%s: pad_len out of range", who);
    EL_REQUIRE(st->loss_kind == EL_FISM_LOSS_REFERENCE || st->loss_kind == EL_FISM_LOSS_BCE, "%s: unknown loss_kind %d", who, st->loss_kind);
    const int piece = nais_piece(ctx);
    EL_REQUIRE(piece != 0, "%s: option fism_piece must be a power of two in 8 .. 4096", who);
    if (level >= 1)
        EL_REQUIRE(st->gGi && st->gGj && st->gBu && st->gBi && st->gW1 && st->gb1 && st->gW2 && st->gb2 && st->gW3 && st->gb3 && st->slot,
                   "%s: needs the ten accumulators and the slot map", who);
    if (level >= 2)
        EL_REQUIRE(st->mGi && st->vGi && st->mGj && st->vGj && st->mBu && st->vBu && st->mBi && st->vBi && st->mW1 && st->vW1 && st->mb1 &&
                       st->vb1 && st->mW2 && st->vW2 && st->mb2 && st->vb2 && st->mW3 && st->vW3 && st->mb3 && st->vb3,
                   "%s: Adam slots missing", who);
    return 0;
}

NaisTabs nais_tabs(const el_nais_state* st, const NaisPrepWs& w, int lpt, int piece) {
    return NaisTabs{st->Gi, w.A, st->Gj, w.Bt, w.w, w.c, st->h_indptr, st->h_indices, st->F, lpt, piece};
}

// out[c] = the sum of src[r, c] over the R rows
template <typename T>
void nais_colsum(hipStream_t s, const T* src, int64_t R, int64_t C, double* part, float* out) {
    const int64_t G = (R + NC_ROWS - 1) / NC_ROWS;
    const unsigned gc = (unsigned)((C + 255) / 256);
    EL_LAUNCH("k_nais_colsum", (k_nais_colsum<T>), dim3((unsigned)G, gc), dim3(256), 0, s, src, R, C, part);
    EL_LAUNCH("k_nais_colsum_fin", k_nais_colsum_fin, dim3(gc), dim3(256), 0, s, part, G, C, out);
}

int nais_grads(el_ctx* ctx, hipStream_t s, const el_nais_state* st, const int32_t* u, const int32_t* j, const float* y, int64_t B,
               double* loss_out, void* ws, size_t ws_bytes, const char* who) {
    EL_REQUIRE(u && j && y && loss_out, "%s: null argument", who);
    EL_REQUIRE(B >= 1 && B < (1LL << 30), "%s: batch size %lld out of range", who, (long long)B);
    NaisWs w;
    EL_REQUIRE(nais_carve(ctx, st, B, ws, &w) == 0, "%s: rocprim size query failed", who);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    const int F = st->F, piece = nais_piece(ctx);
    const int64_t U = st->U, I = st->I, F2 = 2 * F;
    int cpl = 1;
    const int lpt = nais_lpt(F, &cpl);

    // 1: A, Bt, w, c;  the sorted pairs and the batch's distinct users
    if (int rc = nais_prepare(ctx, s, st, w.prep)) return rc;
    const unsigned gb = (unsigned)((B + 255) / 256);
    EL_LAUNCH("k_fism_keys", k_fism_keys, dim3(gb), dim3(256), 0, s, u, j, B, (u32)U, w.key_in, w.val_in, w.split, w.split + 1, w.uplen, w.n_max);
    {
        ElKernelTimer t("rocprim_radix_sort_pairs", s);
        size_t tb = w.sort_bytes;
        EL_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tb, w.key_in, w.key, w.val_in, w.val, (unsigned)(2 * B), 0, el_bits_for(U + I), s));
    }
    const u32 *keyU = w.key, *keyI = w.key + B, *valU = w.val, *valI = w.val + B;
    EL_LAUNCH("k_fism_heads", k_fism_heads, dim3(gb), dim3(256), 0, s, keyU, B, w.hd);
    {
        ElKernelTimer t("rocprim_exclusive_scan", s);
        size_t tb = w.scan_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(w.scan_tmp, tb, w.hd, w.hs, (int32_t)0, (size_t)B, rocprim::plus<int32_t>(), s));
    }
    EL_LAUNCH("k_fism_users", k_fism_users, dim3(gb), dim3(256), 0, s, keyU, w.hd, w.hs, B, U, w.n_max, st->h_indptr, piece, w.rows, st->slot,
              w.uplen, w.n_dev);

    // 2: the sample-major forward and backward walks
    EL_LAUNCH("k_nais_pe", k_nais_pe, dim3(1), dim3(256), 0, s, u, st->h_indptr, B, piece, w.scap - B, w.pe);
    EL_LAUNCH("k_nais_splen", k_nais_splen, dim3((unsigned)((B + 256) / 256)), dim3(256), 0, s, u, st->h_indptr, B, w.pe, w.splen);
    {
        ElKernelTimer t("rocprim_exclusive_scan", s);
        size_t tb = w.scan64_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(w.scan64_tmp, tb, w.splen, w.sstart, (int64_t)0, (size_t)(B + 1), rocprim::plus<int64_t>(), s));
    }
    NaisStep sp = {nais_tabs(st, w.prep, lpt, piece), u, j, B, w.scap, w.pe, w.sstart, w.pfw, w.pbw, w.R, w.NS};
    const dim3 gwalk((unsigned)((w.scap * lpt + 255) / 256)), gsample((unsigned)((B * lpt + 255) / 256));
    NaisFin fin = {sp, st->Bu, st->Bi, st->coef, y, w.cb, w.R, w.NS, w.lossb, w.padb, st->pad_len, st->loss_kind, st->beta_smooth, st->l_b,
                   1.0 / (double)B};
#define NA_WALK(C_)                                                                          \
    do {                                                                                     \
        EL_LAUNCH("k_nais_fwd", (k_nais_fwd<C_>), gwalk, dim3(256), 0, s, sp);               \
        EL_LAUNCH("k_nais_fwd_fin", (k_nais_fwd_fin<C_>), gsample, dim3(256), 0, s, fin);    \
        EL_LAUNCH("k_nais_bwd", (k_nais_bwd<C_>), gwalk, dim3(256), 0, s, sp);               \
    } while (0)
    NA_DISPATCH(cpl, NA_WALK);
#undef NA_WALK
    EL_LAUNCH("k_nais_bwd_fin", k_nais_bwd_fin, dim3((unsigned)B), dim3(256), 0, s, sp, w.rowS, w.gwS);
    nais_colsum(s, w.gwS, B, F2 + 1, w.cpart, w.gwc);
    EL_LAUNCH("k_nais_sums", k_nais_sums, dim3(1), dim3(256), 0, s, w.lossb, w.padb, B, w.tot);

    // 3: the item and user segments: gGj (before the product), gBt, gBi, gBu
    EL_LAUNCH("k_nais_zero", k_nais_zero, dim3(el_stream_grid(ctx, I * F2)), dim3(256), 0, s, w.gBt, I * F2);
    NaisSeg sg = {keyI, valI, (u32)U, B, w.rowS, st->Gj, st->Bi, w.cb, st->gGj, w.gBt, st->gBi, st->l_b, F, lpt};
#define NA_SEG(C_) EL_LAUNCH("k_nais_seg_item", (k_nais_seg_item<C_>), gsample, dim3(256), 0, s, sg)
    NA_DISPATCH(cpl, NA_SEG);
#undef NA_SEG
    EL_LAUNCH("k_nais_seg_user", k_nais_seg_user, dim3(gb), dim3(256), 0, s, keyU, valU, B, U, w.cb, st->Bu, st->l_b, st->gBu);

    // 4: the item-major fan-out: gGi (before the product), gA
    EL_LAUNCH("k_nais_plen", k_nais_plen, dim3((unsigned)((I + 256) / 256)), dim3(256), 0, s, st->t_indptr, I, piece, w.plen);
    {
        ElKernelTimer t("rocprim_exclusive_scan", s);
        size_t tb = w.scan64_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(w.scan64_tmp, tb, w.plen, w.pstart, (int64_t)0, (size_t)(I + 1), rocprim::plus<int64_t>(), s));
    }
    NaisFan fp = {nais_tabs(st, w.prep, lpt, piece), st->t_indptr, st->t_indices, st->slot, j, keyU, valU, B, I, w.pcap, w.R, w.NS,
                  w.pstart, w.part, w.tot, st->gGi, w.gA};
    const dim3 gfan((unsigned)((w.pcap * lpt + 255) / 256));
#define NA_FAN(C_) EL_LAUNCH("k_nais_fan", (k_nais_fan<C_>), gfan, dim3(256), 0, s, fp)
    NA_DISPATCH(cpl, NA_FAN);
#undef NA_FAN
    EL_LAUNCH("k_nais_fan_fin", k_nais_fan_fin, dim3((unsigned)I), dim3(256), 0, s, fp);
    // the loss; the slot map is -1 again before anything below can return early
    EL_LAUNCH("k_nais_finish", k_nais_finish, dim3(el_stream_grid(ctx, w.n_max)), dim3(256), 0, s, w.rows, w.n_dev, st->slot, w.tot, loss_out);

    // 5: the products: gGi += gA W1a^T, gGj += gBt W1b^T, gW1 = [Gi^T gA; Gj^T gBt], gb1; the chain behind w and c
    const unsigned gadd = el_stream_grid(ctx, I * F);
    if (int rc = el_gemm_f32(ctx, s, 0, 1, I, F, F2, w.gA, F2, st->W1, F2, w.tmp, F, nullptr, 0, w.prep.gemm, w.prep.gemm_bytes)) return rc;
    EL_LAUNCH("k_nais_add", k_nais_add, dim3(gadd), dim3(256), 0, s, st->gGi, w.tmp, I * F);
    if (int rc = el_gemm_f32(ctx, s, 0, 1, I, F, F2, w.gBt, F2, st->W1 + (int64_t)F * F2, F2, w.tmp, F, nullptr, 0, w.prep.gemm, w.prep.gemm_bytes))
        return rc;
    EL_LAUNCH("k_nais_add", k_nais_add, dim3(gadd), dim3(256), 0, s, st->gGj, w.tmp, I * F);
    if (int rc = el_gemm_f32(ctx, s, 1, 0, F, F2, I, st->Gi, F, w.gA, F2, st->gW1, F2, nullptr, 0, w.prep.gemm, w.prep.gemm_bytes)) return rc;
    if (int rc = el_gemm_f32(ctx, s, 1, 0, F, F2, I, st->Gj, F, w.gBt, F2, st->gW1 + (int64_t)F * F2, F2, nullptr, 0, w.prep.gemm, w.prep.gemm_bytes))
        return rc;
    nais_colsum(s, w.gBt, I, F2, w.cpart, st->gb1);
    EL_LAUNCH("k_nais_mlp_grads", k_nais_mlp_grads, dim3(el_stream_grid(ctx, F2 * (int64_t)st->Ws)), dim3(256), 0, s, w.gwc, st->W2, st->b2, st->W3,
              (int)F2, st->Ws, st->gW2, st->gW3, st->gb2, st->gb3);
    EL_CHECK_LAUNCH();
    return 0;
}

int nais_apply(el_ctx* ctx, hipStream_t s, const el_nais_state* st, float lr_t) {
    const int64_t F = st->F, ne = st->I * F, Ws = st->Ws;
    struct V {
        const char* nm;
        float *th, *g, *m, *v;
        int64_t n;
    } vars[10] = {{"k_nais_opt_Gi", st->Gi, st->gGi, st->mGi, st->vGi, ne},           {"k_nais_opt_Gj", st->Gj, st->gGj, st->mGj, st->vGj, ne},
                  {"k_nais_opt_Bu", st->Bu, st->gBu, st->mBu, st->vBu, st->U},        {"k_nais_opt_Bi", st->Bi, st->gBi, st->mBi, st->vBi, st->I},
                  {"k_nais_opt_W1", st->W1, st->gW1, st->mW1, st->vW1, 4 * F * F},    {"k_nais_opt_b1", st->b1, st->gb1, st->mb1, st->vb1, 2 * F},
                  {"k_nais_opt_W2", st->W2, st->gW2, st->mW2, st->vW2, 2 * F * Ws},   {"k_nais_opt_b2", st->b2, st->gb2, st->mb2, st->vb2, Ws},
                  {"k_nais_opt_W3", st->W3, st->gW3, st->mW3, st->vW3, Ws},           {"k_nais_opt_b3", st->b3, st->gb3, st->mb3, st->vb3, 1}};
    for (const V& x : vars)
        EL_LAUNCH(x.nm, k_adam_dense, dim3(el_stream_grid(ctx, x.n / 4 + 1)), dim3(256), 0, s, x.th, x.g, x.m, x.v, x.n, lr_t, 0.9f, 0.999f,
                  1e-7f);
    EL_CHECK_LAUNCH();
    return 0;
}

size_t nais_score_carve(el_ctx* ctx, const el_nais_state* st, void* base, NaisPrepWs* w) {
    ElCarve c{(char*)base};
    nais_prep_carve(ctx, c, st, st->I, w);
    return c.off;
}

}  // namespace

extern "C" size_t el_nais_ws_bytes(el_ctx* ctx, const el_nais_state* st, int64_t B) {
    if (!ctx || !st || B < 1 || B >= (1LL << 30) || st->U < 1 || st->I < 1 || st->nnz < 0 || st->F < 1 || st->F > 256 || nais_piece(ctx) == 0)
        return 0;
    NaisWs w;
    if (nais_carve(ctx, st, B, nullptr, &w)) return 0;
    return w.total;
}

extern "C" size_t el_nais_scores_ws_bytes(el_ctx* ctx, const el_nais_state* st) {
    if (!ctx || !st || st->I < 1 || st->F < 1 || st->F > 256) return 0;
    NaisPrepWs w;
    return nais_score_carve(ctx, st, nullptr, &w);
}

extern "C" int el_nais_grads(el_ctx* ctx, void* stream, const el_nais_state* st, const int32_t* u, const int32_t* j, const float* y, int64_t B,
                             double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = nais_check_state(ctx, st, "el_nais_grads", 1)) return rc;
    return nais_grads(ctx, (hipStream_t)stream, st, u, j, y, B, loss_out, ws, ws_bytes, "el_nais_grads");
}

extern "C" int el_nais_apply(el_ctx* ctx, void* stream, const el_nais_state* st, int32_t step, float lr_t) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = nais_check_state(ctx, st, "el_nais_apply", 2)) return rc;
    EL_REQUIRE(step >= 1, "el_nais_apply: step must be >= 1");
    return nais_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_nais_train_step(el_ctx* ctx, void* stream, const el_nais_state* st, const int32_t* u, const int32_t* j, const float* y,
                                  int64_t B, int32_t step, float lr_t, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = nais_check_state(ctx, st, "el_nais_train_step", 2)) return rc;
    EL_REQUIRE(step >= 1, "el_nais_train_step: step must be >= 1");
    if (int rc = nais_grads(ctx, (hipStream_t)stream, st, u, j, y, B, loss_out, ws, ws_bytes, "el_nais_train_step")) return rc;
    return nais_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_nais_forward(el_ctx* ctx, void* stream, const el_nais_state* st, const int32_t* u, const int32_t* j, int64_t n, float* out,
                               void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = nais_check_state(ctx, st, "el_nais_forward", 0)) return rc;
    if (n <= 0) return 0;
    EL_REQUIRE(u && j && out && n < (1LL << 30), "el_nais_forward: bad arguments");
    NaisPrepWs w;
    const size_t need = nais_score_carve(ctx, st, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_nais_forward: workspace too small (%zu < %zu)", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = nais_prepare(ctx, s, st, w)) return rc;
    int cpl = 1;
    const int lpt = nais_lpt(st->F, &cpl);
    NaisPred p = {nais_tabs(st, w, lpt, nais_piece(ctx)), st->Bu, st->Bi, st->coef, st->pad_len, st->beta_smooth};
    const unsigned grid = (unsigned)((n * lpt + 255) / 256);
#define NA_PAIRS(C_) EL_LAUNCH("k_nais_pairs", (k_nais_pairs<C_>), dim3(grid), dim3(256), 0, s, p, u, j, n, out)
    NA_DISPATCH(cpl, NA_PAIRS);
#undef NA_PAIRS
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_nais_scores(el_ctx* ctx, void* stream, const el_nais_state* st, int64_t u_start, int64_t u_stop, float* out, int64_t ld,
                              void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = nais_check_state(ctx, st, "el_nais_scores", 0)) return rc;
    EL_REQUIRE(u_start >= 0 && u_stop <= st->U && u_start <= u_stop && u_stop - u_start <= 65535, "el_nais_scores: bad user block [%lld, %lld)",
               (long long)u_start, (long long)u_stop);
    if (u_start == u_stop) return 0;
    EL_REQUIRE(out != nullptr && ld >= st->I, "el_nais_scores: bad output");
    NaisPrepWs w;
    const size_t need = nais_score_carve(ctx, st, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_nais_scores: workspace too small (%zu < %zu)", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = nais_prepare(ctx, s, st, w)) return rc;
    NaisPred p = {nais_tabs(st, w, 64, nais_piece(ctx)), st->Bu, st->Bi, st->coef, st->pad_len, st->beta_smooth};
    EL_LAUNCH("k_nais_scores", k_nais_scores, dim3((unsigned)((st->I + NS_T - 1) / NS_T), (unsigned)(u_stop - u_start)), dim3(256), 0, s, p,
              st->I, u_start, out, ld);
    EL_CHECK_LAUNCH();
    return 0;
}
