// FISM (factored item similarity, Kabbur et al. 2013) -- contract in include/elliot_hip.h, DESIGN 3.30;
// reference: elliot/recommender/latent_factor_models/FISM/FISM_model.py.
//
// No user table: a user is the sum of the Gi rows of their train items H(u), n_u = |H(u)|, coef_u = n_u^-alpha (uploaded, never
// computed here).  With P_u = coef_u sum_{k in H(u)} Gi[k] (stored order):  x(u, i) = P_u . Gj[i] + Bu[u] + Bi[i],  out = sigma(x).
// With c_b = dL/dx_b, per distinct user of the batch T_u = sum c_b Gj[i_b], cnt_u = #samples, R_u = coef_u T_u:
//   gBu[u] = sum c_b + lambda cnt_u Bu[u]        gBi[i] = sum c_b + gamma m_i Bi[i]        gGj[i] = sum c_b P_{u_b} + beta m_i Gj[i]
//   gGi[k] = sum_{u in batch, k in H(u)} R_u + beta Gi[k] sum cnt_u        (+ beta Gi[0] sum_b (pad_len - n_{u_b}) for k = 0)
//
// THE PRIMITIVE (k_fism_cut + k_fism_combine + k_fism_combine_long): the ordered sum of gathered rows over a CSR list, cut into pieces
// of `fism_piece` positions.  A list of len positions has max(1, ceil(len / piece)) pieces; ONE exclusive scan (rocprim) over a packed
// 64-bit count -- low word: pieces, high word: pieces of lists that have more than one -- maps a lane group to (list, piece) by binary
// search and gives every cut list a contiguous run of partial rows.  A lane group stages 64 indices of its piece in LDS at a time
// and walks them in order, four row loads in flight.  A list of one piece is finished in place (FIN); a longer one leaves a partial
// row, a double and an int per piece, which are added in ascending piece order by one lane group (2 .. 16 pieces) or by a workgroup
// whose lane groups take contiguous shares that are then added in lane-group order (more than 16).  No list is walked end to end by
// one workgroup.  Three instantiations:
//   forward   lists H(u) of the batch's distinct users, gathers Gi[k] unfiltered (+ sum |Gi[k]|^2 for the regulariser) -> P_u, q_u in slot n(u)
//   fan-out   the user lists of ALL I items (item-major copy of the train matrix), gathers R[slot[u]] and cnt where slot[u] >= 0 -> gGi
//   image     lists H(u) of ALL users -> P[u] = coef_u (p_u + (pad_len - n_u) Gi[0])  for el_score_topk
// Around it, one gradient pass:
//   1. k_fism_keys + ONE stable radix sort of (u, b) and (U + i, b);  k_fism_heads + scan: slot n(u) of every distinct user;  k_fism_users
//   2. the forward instantiation
//   3. k_fism_fwd   one lane group per sample: x, out, c_b; per workgroup double partials of the loss and of sum (pad_len - n_u)
//   4. k_fism_seg (the sorted-segment walk of k_pw_seg) for users (T_u -> R_u, cnt_u, gBu) and items (gGj, gBi); cut segments through
//      k_seg_combine / k_seg_combine_long (el_segcombine.h)
//   5. the fan-out instantiation
//   6. k_fism_finish  the partials added in index order, slot[] back to -1 through the list of distinct users
// No floating-point atomics on any row, a fixed order in every sum: the same input gives the same bytes.  No matrix instruction:
// every product here is a gather or a segment sum.  The optimiser is k_adam_dense (Keras Adam on IndexedSlices: every row moves), one
// launch per variable from the dense accumulators.
#include "el_common.h"
#include "el_segcombine.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

#define FI_STG 64            // list / segment positions whose indices a lane group stages in LDS at once
#define FI_COMB_LONG 16      // a list of more pieces than this is combined by a workgroup

#include "el_fism_keys.h"

// a lane's elements of one row (zero where the lane holds none or !ok): the split of fm_ld_row
template <int VW, int CPL>
__device__ __forceinline__ void fi_ld_row(const float* row, int F, int sub, int lpt, bool ok, float (&r)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
#pragma unroll
        for (int x = 0; x < VW; ++x) r[q][x] = 0.f;
        if (ok && e < F) ldv<VW>(row + e, r[q]);
    }
}
template <int VW, int CPL>
__device__ __forceinline__ void fi_st_row(float* row, int F, int sub, int lpt, const float (&r)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
        if (e < F) stv<VW>(row + e, r[q]);
    }
}
template <int VW, int CPL>
__device__ __forceinline__ float fi_dot(const float (&a)[CPL][VW], const float (&b)[CPL][VW], int lpt) {
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) d = fmaf(a[q][x], b[q][x], d);
    return el_group_sum(d, lpt);
}
template <int VW, int CPL>
__device__ __forceinline__ void fi_zero(float (&a)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) a[q][x] = 0.f;
}

// ---- the cut primitive --------------------------------------------------------------------------------------------------------
struct FismCut {
    const int64_t* indptr;    // the lists (CSR)
    const int32_t* indices;
    const int32_t* ids;       // list l -> CSR row (NULL: l)
    const u64* pstart;        // [nl + 1] exclusive scan: low word = first piece of list l, high word = its first partial row
    int64_t nl, pcap;         // lists; partial rows the scratch holds
    int piece, F, lpt;
    float* part;              // [pcap, F]
    double* part_s;           // [pcap]
    int32_t* part_c;          // [pcap]
};

// forward source: the history's own rows, unfiltered; the float beside the row is sum |row|^2
struct FismSrcHist {
    const float* Gi;
    static constexpr bool SQ = true;
    typedef double acc_t;        // a history of hundreds of rows is pooled in double and rounded once (the loss reads it at one float ulp)
    __device__ __forceinline__ int32_t map(int32_t k) const { return k; }
    __device__ __forceinline__ const float* rows() const { return Gi; }
    __device__ __forceinline__ int count(int32_t) const { return 0; }
};
// fan-out source: the slot rows of the users that are in the batch; the int beside the row is sum cnt_u
struct FismSrcSlot {
    const int32_t* slot;
    const float* R;
    const int32_t* Cn;
    static constexpr bool SQ = false;
    typedef float acc_t;
    __device__ __forceinline__ int32_t map(int32_t u) const { return slot[u]; }
    __device__ __forceinline__ const float* rows() const { return R; }
    __device__ __forceinline__ int count(int32_t sl) const { return sl >= 0 ? Cn[sl] : 0; }
};

// list positions [k0, k1) by ONE lane group: FI_STG mapped indices staged in LDS together, then the rows whose index is >= 0 added in
// list order, four in flight
template <int VW, int CPL, class SRC>
__device__ __forceinline__ void fi_walk(const SRC& src, const int32_t* __restrict__ indices, int64_t k0, int64_t k1, int32_t* stage, int F,
                                        int sub, int lpt, typename SRC::acc_t (&acc)[CPL][VW], double& sacc, int& cacc) {
    typedef typename SRC::acc_t A;
    const float* tab = src.rows();
    for (int64_t base = k0; base < k1; base += FI_STG) {
        const int cs = (int)((k1 - base < FI_STG) ? k1 - base : FI_STG);
        for (int t = sub; t < cs; t += lpt) stage[t] = src.map(indices[base + t]);
        el_wave_lds_sync();
        for (int b4 = 0; b4 < cs; b4 += 4) {
            int32_t sl[4];
            float r[4][CPL][VW];
            int cv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sl[k] = b4 + k < cs ? stage[b4 + k] : -1;
                fi_ld_row<VW, CPL>(tab + (int64_t)(sl[k] < 0 ? 0 : sl[k]) * F, F, sub, lpt, sl[k] >= 0, r[k]);
                cv[k] = src.count(sl[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (sl[k] < 0) continue;
                cacc += cv[k];
#pragma unroll
                for (int q = 0; q < CPL; ++q)
#pragma unroll
                    for (int x = 0; x < VW; ++x) {
                        acc[q][x] += (A)r[k][q][x];
                        if (SRC::SQ) sacc += (double)r[k][q][x] * (double)r[k][q][x];
                    }
            }
        }
        el_wave_lds_sync();
    }
}

// one lane group per piece
template <int VW, int CPL, class SRC, class FIN>
__global__ __launch_bounds__(256) void k_fism_cut(FismCut c, SRC src, FIN fin) {
    __shared__ int32_t s_st[32][FI_STG];
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
    if (np < 1) return;                                          // (a slot no user took: an id past the table)
    const int64_t row = c.ids ? c.ids[lo] : lo;
    const int64_t r0 = c.indptr[row], r1 = c.indptr[row + 1];
    const int64_t k0 = r0 + k * c.piece < r1 ? r0 + k * c.piece : r1, k1 = k0 + c.piece < r1 ? k0 + c.piece : r1;
    typename SRC::acc_t accw[CPL][VW];
    float acc[CPL][VW];
    double sacc = 0.0;
    int cacc = 0;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) accw[q][x] = 0;
    fi_walk<VW, CPL, SRC>(src, c.indices, k0, k1, s_st[gl], c.F, sub, lpt, accw, sacc, cacc);
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) acc[q][x] = (float)accw[q][x];
    if (SRC::SQ) sacc = el_group_sum(sacc, lpt);
    if (np == 1) {
        fin(lo, row, sub, lpt, acc, sacc, cacc);
    } else if (pslot < c.pcap) {
        fi_st_row<VW, CPL>(c.part + pslot * c.F, c.F, sub, lpt, acc);
        if (sub == 0) c.part_s[pslot] = sacc, c.part_c[pslot] = cacc;
    }
}

// partial rows [p0, p1) added to (acc, sacc, cacc) in ascending order, four in flight
template <int VW, int CPL>
__device__ __forceinline__ void fi_add_parts(const FismCut& c, int64_t p0, int64_t p1, int sub, int lpt, float (&acc)[CPL][VW], double& sacc,
                                             int& cacc) {
    for (int64_t p = p0; p < p1; p += 4) {
        float v[4][CPL][VW];
        double vs[4];
        int vc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t sl = p + t < p1 ? p + t : p;
            fi_ld_row<VW, CPL>(c.part + sl * c.F, c.F, sub, lpt, true, v[t]);
            vs[t] = c.part_s[sl], vc[t] = c.part_c[sl];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (p + t >= p1) continue;
            sacc += vs[t], cacc += vc[t];
#pragma unroll
            for (int q = 0; q < CPL; ++q)
#pragma unroll
                for (int x = 0; x < VW; ++x) acc[q][x] += v[t][q][x];
        }
    }
}

// lists of 2 .. FI_COMB_LONG pieces: one lane group per list
template <int VW, int CPL, class FIN>
__global__ __launch_bounds__(256) void k_fism_combine(FismCut c, FIN fin) {
    const int lpt = c.lpt;
    const int64_t l = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    if (l >= c.nl) return;
    const u64 ps = c.pstart[l];
    const int64_t np = fi_lo(c.pstart[l + 1]) - fi_lo(ps), p0 = (int64_t)(ps >> 32);
    if (np < 2 || np > FI_COMB_LONG || p0 + np > c.pcap) return;
    float acc[CPL][VW];
    double sacc = 0.0;
    int cacc = 0;
    fi_zero<VW, CPL>(acc);
    fi_add_parts<VW, CPL>(c, p0, p0 + np, sub, lpt, acc, sacc, cacc);
    fin(l, c.ids ? (int64_t)c.ids[l] : l, sub, lpt, acc, sacc, cacc);
}

// lists of more pieces: one workgroup per list; its 256 / lpt lane groups take contiguous shares of the partial rows in order, the
// shares are added through LDS in lane-group order
template <int VW, int CPL, class FIN>
__global__ __launch_bounds__(256) void k_fism_combine_long(FismCut c, FIN fin) {
    __shared__ __attribute__((aligned(16))) float s_red[4096];      // (256 / lpt) lane groups x F floats, as k_seg_combine_long
    __shared__ double s_rs[32];
    __shared__ int s_rc[32];
    const int F = c.F, lpt = c.lpt;
    const int ngl = 256 / lpt, gl = (int)(threadIdx.x / lpt), sub = (int)(threadIdx.x & (lpt - 1));
    for (int64_t l = blockIdx.x; l < c.nl; l += gridDim.x) {
        const u64 ps = c.pstart[l];
        const int64_t np = fi_lo(c.pstart[l + 1]) - fi_lo(ps), p0 = (int64_t)(ps >> 32);
        if (np <= FI_COMB_LONG || p0 + np > c.pcap) continue;       // (uniform over the workgroup)
        const int64_t per = (np + ngl - 1) / ngl;
        const int64_t k0 = gl * per < np ? gl * per : np, k1 = k0 + per < np ? k0 + per : np;
        float acc[CPL][VW];
        double sacc = 0.0;
        int cacc = 0;
        fi_zero<VW, CPL>(acc);
        fi_add_parts<VW, CPL>(c, p0 + k0, p0 + k1, sub, lpt, acc, sacc, cacc);
        fi_st_row<VW, CPL>(s_red + gl * F, F, sub, lpt, acc);
        if (sub == 0) s_rs[gl] = sacc, s_rc[gl] = cacc;
        __syncthreads();
        if (gl == 0) {
            float gg[CPL][VW];
            double gs = 0.0;
            int gc = 0;
            for (int h = 0; h < ngl; ++h) gs += s_rs[h], gc += s_rc[h];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int e = (sub + q * lpt) * VW;
#pragma unroll
                for (int x = 0; x < VW; ++x) gg[q][x] = 0.f;
                if (e >= F) continue;
                for (int h = 0; h < ngl; ++h) {
                    float t4[VW];
                    ldv<VW>(s_red + h * F + e, t4);
#pragma unroll
                    for (int x = 0; x < VW; ++x) gg[q][x] += t4[x];
                }
            }
            fin(l, c.ids ? (int64_t)c.ids[l] : l, sub, lpt, gg, gs, gc);
        }
        __syncthreads();
    }
}

// finish of a pooled history: out[l] = coef_u (sum + (pad_len - n_u) Gi[0]), q[l] = sum |Gi[k]|^2   (pad_len = 0, q = NULL: without)
struct FismFinPool {
    const float* coef;
    const int64_t* indptr;
    const float* Gi0;
    float* out;
    double* q;
    int64_t pad_len;
    int F;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t l, int64_t row, int sub, int lpt, const float (&acc)[CPL][VW], double s, int) const {
        const float cf = coef[row];
        float g0[CPL][VW], o[CPL][VW];
        const float padn = pad_len > 0 ? (float)(pad_len - (indptr[row + 1] - indptr[row])) : 0.f;
        fi_ld_row<VW, CPL>(Gi0, F, sub, lpt, pad_len > 0, g0);
#pragma unroll
        for (int qq = 0; qq < CPL; ++qq)
#pragma unroll
            for (int x = 0; x < VW; ++x) o[qq][x] = cf * fmaf(padn, g0[qq][x], acc[qq][x]);
        fi_st_row<VW, CPL>(out + l * F, F, sub, lpt, o);
        if (sub == 0 && q) q[l] = s;
    }
};

// finish of an item's fan-out: gGi[k] = sum R_u + beta Gi[k] sum cnt_u, row 0 with the padded slots of the batch (padp: the
// per-workgroup partials of k_fism_fwd, integers held in doubles -- every order gives the same sum)
struct FismFinFan {
    const float* Gi;
    float* gGi;
    const double* padp;         // NULL with pad_len = 0
    int nparts, F;
    float beta;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t, int64_t row, int sub, int lpt, const float (&acc)[CPL][VW], double, int c) const {
        double extra = 0.0;
        if (row == 0 && padp) {
            for (int k = sub; k < nparts; k += lpt) extra += padp[2 * k + 1];
            extra = el_group_sum(extra, lpt);
        }
        const float w = beta * (float)((double)c + extra);
        float e[CPL][VW], g[CPL][VW];
        fi_ld_row<VW, CPL>(Gi + row * F, F, sub, lpt, true, e);
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) g[q][x] = fmaf(w, e[q][x], acc[q][x]);
        fi_st_row<VW, CPL>(gGi + row * F, F, sub, lpt, g);
    }
};

// ---- keys, slots: k_fism_keys, k_fism_heads, k_fism_users (el_fism_keys.h) ------------------------------------------------------
// the piece counts of ALL nl lists of a CSR (the fan-out, the image); entry nl closes the scan
__global__ __launch_bounds__(256) void k_fism_plen(const int64_t* __restrict__ indptr, int64_t nl, int piece, u64* __restrict__ plen) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l > nl) return;
    plen[l] = l < nl ? fi_plen(indptr[l + 1] - indptr[l], piece) : 0ull;
}

// ---- scores, c_b, loss ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fi_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct FismFwd {
    const float *Gj, *Bu, *Bi, *S;
    const double* Q;
    const int32_t *slot, *bu, *bi;
    const int64_t* h_indptr;
    const float* label;
    float* cb;
    int64_t n, pad_len;
    int F, lpt, loss_kind;
    float beta, lambda, gamma;
    double inv_n;
    double* part;        // [2 gridDim.x]: per workgroup the loss and sum (pad_len - n_u)
};

template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fism_fwd(FismFwd p) {
    const int F = p.F, lpt = p.lpt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    double lossv = 0.0, padv = 0.0;
    for (int64_t b = gid / lpt; b < p.n; b += groups) {
        const int64_t u = p.bu[b], i = p.bi[b], sl = p.slot[u];
        float a[CPL][VW], g[CPL][VW];
        fi_ld_row<VW, CPL>(p.S + sl * F, F, sub, lpt, true, a);
        fi_ld_row<VW, CPL>(p.Gj + i * F, F, sub, lpt, true, g);
        double dot = 0.0, gsq = 0.0;                              // (a handful of products per lane: in double, as the loss is)
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) dot += (double)a[q][x] * (double)g[q][x], gsq += (double)g[q][x] * (double)g[q][x];
        dot = el_group_sum(dot, lpt), gsq = el_group_sum(gsq, lpt);
        if (sub == 0) {
            const float bu = p.Bu[u], bi = p.Bi[i];
            const double od = 1.0 / (1.0 + exp(-(dot + (double)bu + (double)bi)));
            const float o = (float)od;
            const double y = (double)p.label[b], eps = 1e-7;
            double data, d;
            if (p.loss_kind == EL_FISM_LOSS_REFERENCE) {          // Keras BCE(y_true = out, y_pred = label): linear in out
                const double yh = y < eps ? eps : (y > 1.0 - eps ? 1.0 - eps : y);
                const double la = log(yh + eps), lb = log(1.0 - yh + eps);
                data = -(od * la + (1.0 - od) * lb);
                d = -(la - lb);
            } else {                                              // the cross-entropy that was meant: y_true = (label > 0), y_pred = out
                const double pc = od < eps ? eps : (od > 1.0 - eps ? 1.0 - eps : od);
                const bool pass = od >= eps && od <= 1.0 - eps;
                data = y > 0.0 ? -log(pc + eps) : -log(1.0 - pc + eps);
                d = !pass ? 0.0 : (y > 0.0 ? -1.0 / (pc + eps) : 1.0 / (1.0 - pc + eps));
            }
            p.cb[b] = (float)(d * p.inv_n) * (o * (1.0f - o));     // (the gradient is cast to float before the sigmoid's derivative)
            const double reg = 0.5 * ((double)p.lambda * (double)(bu * bu) + (double)p.gamma * (double)(bi * bi) +
                                      (double)p.beta * (gsq + p.Q[sl]));
            lossv += data * p.inv_n + reg;
            if (p.pad_len > 0) padv += (double)(p.pad_len - (p.h_indptr[u + 1] - p.h_indptr[u]));
        }
    }
    __shared__ double part[2][4];
    for (int o = 32; o > 0; o >>= 1) lossv += __shfl_xor(lossv, o, 64), padv += __shfl_xor(padv, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) part[0][wv] = lossv, part[1][wv] = padv;
    __syncthreads();
    if (threadIdx.x == 0) {
        p.part[2 * blockIdx.x] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        p.part[2 * blockIdx.x + 1] = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    }
}

struct FismTabs {
    const float *Gi, *Gj, *Bu, *Bi, *coef;
    const int64_t* h_indptr;
    const int32_t* h_indices;
    int64_t pad_len;
    int F;
};

// out of explicit pairs straight from the tables (the model's scoring: batch_predict, with its padded slots): p_u is formed on the
// fly by the pair's lane group, no scratch
template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fism_predict(FismTabs t, const int32_t* __restrict__ bu, const int32_t* __restrict__ bi, int64_t n,
                                                      int lpt, float* __restrict__ out) {
    __shared__ int32_t s_st[32][FI_STG];
    const int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1)), gl = (int)(threadIdx.x / lpt);
    if (b >= n) return;
    const int64_t u = bu[b], i = bi[b], r0 = t.h_indptr[u], r1 = t.h_indptr[u + 1];
    float acc[CPL][VW], g0[CPL][VW], g[CPL][VW];
    double accw[CPL][VW], sacc = 0.0;
    int cacc = 0;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) accw[q][x] = 0.0;
    fi_walk<VW, CPL, FismSrcHist>(FismSrcHist{t.Gi}, t.h_indices, r0, r1, s_st[gl], t.F, sub, lpt, accw, sacc, cacc);
    const float padn = t.pad_len > 0 ? (float)(t.pad_len - (r1 - r0)) : 0.f, cf = t.coef[u];
    fi_ld_row<VW, CPL>(t.Gi, t.F, sub, lpt, t.pad_len > 0, g0);
    fi_ld_row<VW, CPL>(t.Gj + i * t.F, t.F, sub, lpt, true, g);
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) acc[q][x] = cf * fmaf(padn, g0[q][x], (float)accw[q][x]);
    const float dot = fi_dot<VW, CPL>(acc, g, lpt);
    if (sub == 0) out[b] = fi_sigmoid(dot + t.Bu[u] + t.Bi[i]);
}

// ---- the two sorted-segment passes ------------------------------------------------------------------------------------------------
// (fi_count, the samples of one row: el_fism_keys.h)
// finish of a complete user row (T_u, sum c_b): R_u = coef_u T_u and cnt_u to the user's slot, gBu
struct FismFinUser {
    const u32* keys;
    int64_t n;
    const float *coef, *Bu;
    const int32_t* slot;
    float *R, *gBu;
    int32_t* Cn;
    float lambda;
    int F;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t row, int sub, int lpt, const float (&gg)[CPL][VW], float b) const {
        const int64_t sl = slot[row];
        const float cf = coef[row];
        float r[CPL][VW];
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) r[q][x] = cf * gg[q][x];
        fi_st_row<VW, CPL>(R + sl * F, F, sub, lpt, r);
        if (sub == 0) {
            const int cnt = fi_count(keys, n, (u32)row);
            Cn[sl] = cnt;
            gBu[row] = fmaf(lambda * (float)cnt, Bu[row], b);
        }
    }
};

// finish of a complete item row (sum c_b P_u, sum c_b): gGj and gBi with their regularisers (m_i samples)
struct FismFinItem {
    const u32* keys;
    int64_t n;
    u32 key_off;
    const float *Gj, *Bi;
    float *gGj, *gBi;
    float beta, gamma;
    int F;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t row, int sub, int lpt, const float (&gg)[CPL][VW], float b) const {
        const float m = (float)fi_count(keys, n, (u32)row + key_off);
        float e[CPL][VW], g[CPL][VW];
        fi_ld_row<VW, CPL>(Gj + row * F, F, sub, lpt, true, e);
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) g[q][x] = fmaf(beta * m, e[q][x], gg[q][x]);
        fi_st_row<VW, CPL>(gGj + row * F, F, sub, lpt, g);
        if (sub == 0) gBi[row] = fmaf(gamma * m, Bi[row], b);
    }
};

struct FismSeg {
    const u32 *keys, *vals;     // sorted row ids of THIS side (+ key_off) and the sample of each position
    u32 key_off;
    const float* cb;
    const int32_t* other_ids;   // the sample's row on the other side ...
    const int32_t* other_map;   // ... sent through the slot map (item pass: rows of the pooled image) or NULL (user pass: rows of Gj)
    const float* other;
    int64_t n;
    int F, chunk, lpt;
    float *part, *part_b;       // pieces of segments cut by chunk boundaries (el_segcombine.h)
};

// the sorted-segment walk of k_pw_seg (el_pwmf.hip): a lane group per chunk of sorted positions, the index chain staged in LDS,
// a complete segment finished here by FIN, a cut piece left in its partial slot
template <int VW, int CPL, typename FIN>
__global__ __launch_bounds__(256) void k_fism_seg(FismSeg p, FIN fin) {
    const int F = p.F, lpt = p.lpt;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t p0 = grp * p.chunk;
    if (p0 >= p.n) return;
    const int64_t p1 = (p0 + p.chunk < p.n) ? p0 + p.chunk : p.n;
    int64_t cur = -1;
    bool started_inside = false;
    float acc[CPL][VW];
    float bacc = 0.f;
    auto flush = [&](bool ends_inside) {
        if (started_inside && ends_inside) {
            fin(cur, sub, lpt, acc, bacc);
            return;
        }
        // a cut piece: slot 2 grp + 1 when the segment starts in this chunk (the head piece), 2 grp otherwise
        const int64_t slot = 2 * grp + (started_inside ? 1 : 0);
        fi_st_row<VW, CPL>(p.part + slot * F, F, sub, lpt, acc);
        if (sub == 0) p.part_b[slot] = bacc;
    };
    __shared__ u32 s_key[32][FI_STG];
    __shared__ u32 s_oth[32][FI_STG];
    __shared__ float s_cf[32][FI_STG];
    const int gl = (int)(threadIdx.x / lpt);
    constexpr int SUB = (CPL == 1) ? 4 : (CPL == 2 ? 2 : 1);     // positions whose row loads are in flight together
    for (int64_t sbase = p0; sbase < p1; sbase += FI_STG) {
        const int cs = (int)((p1 - sbase < FI_STG) ? p1 - sbase : FI_STG);
        for (int t = sub; t < cs; t += lpt) {
            const int64_t b = (int64_t)p.vals[sbase + t];
            const int32_t o = p.other_ids[b];
            s_key[gl][t] = p.keys[sbase + t] - p.key_off;
            s_cf[gl][t] = p.cb[b];
            s_oth[gl][t] = (u32)(p.other_map ? p.other_map[o] : o);
        }
        el_wave_lds_sync();
        for (int base = 0; base < cs; base += SUB) {
            int64_t keyv[SUB];
            float cv[SUB];
            bool okv[SUB];
            float rr[SUB][CPL][VW];
#pragma unroll
            for (int t = 0; t < SUB; ++t) {
                okv[t] = base + t < cs;
                const int tt = okv[t] ? base + t : base;
                keyv[t] = (int64_t)s_key[gl][tt];
                cv[t] = s_cf[gl][tt];
                fi_ld_row<VW, CPL>(p.other + (int64_t)s_oth[gl][tt] * F, F, sub, lpt, okv[t], rr[t]);
            }
#pragma unroll
            for (int t = 0; t < SUB; ++t) {
                if (!okv[t]) continue;
                const int64_t pos = sbase + base + t, key = keyv[t];
                if (key != cur) {
                    if (cur >= 0) flush(true);
                    cur = key;
                    started_inside = (pos > p0) || (pos == 0) || ((int64_t)(p.keys[pos - 1] - p.key_off) != key);
                    bacc = 0.f;
                    fi_zero<VW, CPL>(acc);
                }
#pragma unroll
                for (int q = 0; q < CPL; ++q)
#pragma unroll
                    for (int x = 0; x < VW; ++x) acc[q][x] = fmaf(cv[t], rr[t][q][x], acc[q][x]);
                bacc += cv[t];
            }
        }
        el_wave_lds_sync();
    }
    flush(p1 == p.n || (int64_t)(p.keys[p1] - p.key_off) != cur);
}

// the step's loss from the per-workgroup partials in index order (workgroup 0) with the padded slots' share, and the slot map back
// to -1 through the list of the batch's distinct users (every workgroup): the last kernel that reads the map clears it
__global__ __launch_bounds__(256) void k_fism_finish(const int32_t* __restrict__ rows, const int32_t* __restrict__ n_dev,
                                                     int32_t* __restrict__ slot, const double* __restrict__ part, int nparts,
                                                     const float* __restrict__ Gi0, int F, float beta, double* loss_out) {
    const int64_t n = *n_dev, stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) slot[rows[s]] = -1;
    if (blockIdx.x != 0) return;
    __shared__ double red[2][256];
    double a = 0.0, c = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) a += part[2 * k], c += part[2 * k + 1];
    red[0][threadIdx.x] = a, red[1][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[0][threadIdx.x] += red[0][threadIdx.x + o], red[1][threadIdx.x] += red[1][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double sq = 0.0;
        if (red[1][0] != 0.0)
            for (int e = 0; e < F; ++e) sq += (double)Gi0[e] * (double)Gi0[e];
        *loss_out += red[0][0] + 0.5 * (double)beta * sq * red[1][0];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct FismCutWs {
    u64 *plen, *pstart;
    void* scan_tmp;
    size_t scan_bytes;
    float* part;
    double* part_s;
    int32_t* part_c;
    int64_t pcap;
};
struct FismWs {
    u32 *key_in, *val_in, *key, *val;
    float* cb;
    int32_t *hd, *hs, *rows, *n_dev, *Cn;
    float *S, *R;
    double* Q;
    double* lossp;
    void *sort_tmp, *scan_tmp;
    size_t sort_bytes, scan_bytes, total;
    float *part, *part_b;
    int32_t *split_u, *split_i;
    int64_t n_max;
    FismCutWs cut;
};

// the scratch of one run of the primitive over at most nl lists of at most nnz positions in all: a list of more than one piece has
// fewer than 2 len / piece of them, and there are at most nl + nnz / piece pieces
int fism_cut_carve(ElCarve& c, int64_t nl, int64_t nnz, int piece, int F, FismCutWs* w) {
    w->plen = c.take<u64>((size_t)(nl + 1));
    w->pstart = c.take<u64>((size_t)(nl + 1));
    size_t t = 0;
    u64* np = nullptr;
    if (rocprim::exclusive_scan(nullptr, t, np, np, (u64)0, (size_t)(nl + 1), rocprim::plus<u64>(), (hipStream_t)0) != hipSuccess) return 1;
    w->scan_bytes = t;
    w->scan_tmp = c.take<char>(t);
    const int64_t a = 2 * (nnz / piece) + 1, b = nl + nnz / piece;
    w->pcap = a < b ? a : b;
    w->part = c.take<float>((size_t)w->pcap * (size_t)F);
    w->part_s = c.take<double>((size_t)w->pcap);
    w->part_c = c.take<int32_t>((size_t)w->pcap);
    return 0;
}

// positions per lane group of the two passes: the point-wise step's (el_pwmf.hip)
int fism_item_chunk(int64_t n) {
    const int64_t c = n / 16384;
    return (int)(c < 16 ? 16 : (c > 256 ? 256 : c));
}
int fism_user_chunk(int64_t n) {
    const int64_t c = n / 65536;
    return (int)(c < 4 ? 4 : (c > 16 ? 16 : c));
}
int64_t fism_fwd_cap(el_ctx* ctx) { return (int64_t)ctx->cus * 16; }

int fism_piece(el_ctx* ctx) {
    const double v = ctx->opt.fism_piece;
    const int p = (int)v;
    return ((double)p == v && p >= 8 && p <= 4096 && (p & (p - 1)) == 0) ? p : 0;
}

int fism_carve(el_ctx* ctx, int64_t B, int64_t U, int64_t I, int64_t nnz, int F, void* base, FismWs* w) {
    ElCarve c{(char*)base};
    const int64_t n = 2 * B, n_max = B < U ? B : U;
    w->n_max = n_max;
    w->key_in = c.take<u32>((size_t)n);
    w->val_in = c.take<u32>((size_t)n);
    w->key = c.take<u32>((size_t)n);
    w->val = c.take<u32>((size_t)n);
    w->cb = c.take<float>((size_t)B);
    w->hd = c.take<int32_t>((size_t)B);
    w->hs = c.take<int32_t>((size_t)B);
    w->rows = c.take<int32_t>((size_t)n_max);
    w->n_dev = c.take<int32_t>(1);
    w->Cn = c.take<int32_t>((size_t)n_max);
    w->S = c.take<float>((size_t)n_max * (size_t)F);
    w->Q = c.take<double>((size_t)n_max);
    w->R = c.take<float>((size_t)n_max * (size_t)F);
    w->lossp = c.take<double>((size_t)(2 * fism_fwd_cap(ctx)));
    size_t t1 = 0, t2 = 0;
    u32* np = nullptr;
    int32_t* ip = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (unsigned)n, 0, el_bits_for(U + I), (hipStream_t)0) != hipSuccess) return 1;
    if (rocprim::exclusive_scan(nullptr, t2, ip, ip, (int32_t)0, (size_t)B, rocprim::plus<int32_t>(), (hipStream_t)0) != hipSuccess) return 1;
    w->sort_bytes = t1, w->scan_bytes = t2;
    w->sort_tmp = c.take<char>(t1);
    w->scan_tmp = c.take<char>(t2);
    const int cu = fism_user_chunk(B), ci = fism_item_chunk(B), cm = cu < ci ? cu : ci;
    const int64_t groups = (B + cm - 1) / cm + 1;
    w->part = c.take<float>((size_t)2 * groups * (size_t)F);
    w->part_b = c.take<float>((size_t)2 * groups);
    w->split_u = c.take<int32_t>((size_t)(2 * groups + 4));
    w->split_i = c.take<int32_t>((size_t)(2 * groups + 4));
    // ONE scratch of the primitive serves the forward (n_max lists) and the fan-out (I lists), one after the other
    if (fism_cut_carve(c, n_max > I ? n_max : I, nnz, fism_piece(ctx), F, &w->cut)) return 1;
    w->total = c.off;
    return 0;
}

bool fism_al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

int fism_check_state(el_ctx* ctx, const el_fism_state* st, const char* who, int level) {      // level 0: scoring, 1: + accumulators, 2: + Adam slots
    EL_REQUIRE(st != nullptr, "%s: null state", who);
    EL_REQUIRE(st->U > 0 && st->I > 0 && st->nnz >= 0, "%s: bad shape U=%lld I=%lld nnz=%lld", who, (long long)st->U, (long long)st->I,
               (long long)st->nnz);
    EL_REQUIRE(st->F >= 1 && st->F <= 512, "%s: F=%d out of range (1 .. 512)", who, st->F);
    EL_REQUIRE(st->U + st->I < (1LL << 32) && st->nnz < (1LL << 40), "%s: U + I must fit a 32-bit sort key", who);
    EL_REQUIRE(st->Gi && st->Gj && st->Bu && st->Bi, "%s: null tables", who);
    EL_REQUIRE(st->coef != nullptr, "%s: coef is NULL (n_u^-alpha is computed by the caller)", who);
    EL_REQUIRE(st->h_indptr && st->h_indices && st->t_indptr && st->t_indices, "%s: needs the train matrix user-major and item-major", who);
    EL_REQUIRE(st->pad_len >= 0 && st->pad_len < (1LL << 31), "%s: pad_len out of range", who);
    EL_REQUIRE(st->loss_kind == EL_FISM_LOSS_REFERENCE || st->loss_kind == EL_FISM_LOSS_BCE, "%s: unknown loss_kind %d", who, st->loss_kind);
    EL_REQUIRE(fism_piece(ctx) != 0, "%s: option fism_piece must be a power of two in 8 .. 4096", who);
    if (level >= 1) EL_REQUIRE(st->gGi && st->gGj && st->gBu && st->gBi && st->slot, "%s: needs the four accumulators and the slot map", who);
    if (level >= 2)
        EL_REQUIRE(st->mGi && st->vGi && st->mGj && st->vGj && st->mBu && st->vBu && st->mBi && st->vBi, "%s: Adam slots missing", who);
    return 0;
}

// the row split: 16-byte lanes where the rows allow it (VW = 4: up to 2 vectors per lane), else one float per lane and up to 8
#define FI_DISPATCH(vec, cpl, CALL)        \
    do {                                   \
        if (vec) {                         \
            if ((cpl) == 1) CALL(4, 1);    \
            else CALL(4, 2);               \
        } else if ((cpl) == 1) CALL(1, 1); \
        else if ((cpl) == 2) CALL(1, 2);   \
        else if ((cpl) == 4) CALL(1, 4);   \
        else CALL(1, 8);                   \
    } while (0)

int fism_split(int F, bool vec, int* cpl) { return el_pick_lpt(F, vec ? 4 : 1, cpl); }

// one run of the primitive: the scan of the piece counts (already in cw.plen), the pieces, the two combines
template <class SRC, class FIN>
int fism_run_cut(el_ctx* ctx, hipStream_t s, const FismCutWs& cw, FismCut c, int64_t nnz, bool vec, int cpl, const SRC& src, const FIN& fin,
                 const char* nm) {
    {
        ElKernelTimer t("rocprim_exclusive_scan", s);
        size_t tb = cw.scan_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(cw.scan_tmp, tb, cw.plen, cw.pstart, (u64)0, (size_t)(c.nl + 1), rocprim::plus<u64>(), s));
    }
    c.pstart = cw.pstart, c.pcap = cw.pcap, c.part = cw.part, c.part_s = cw.part_s, c.part_c = cw.part_c;
    const int64_t pieces = c.nl + nnz / c.piece;                     // (an upper bound: the lane groups past the scan's total leave at once)
    const unsigned gp = (unsigned)((pieces * c.lpt + 255) / 256), gc = (unsigned)((c.nl * c.lpt + 255) / 256);
    const int64_t capl = (int64_t)ctx->cus * 4;
    const unsigned gl = (unsigned)(c.nl < capl ? c.nl : capl);
#define FI_CUT(VW_, CPL_)                                                                                               \
    do {                                                                                                                \
        EL_LAUNCH(nm, (k_fism_cut<VW_, CPL_, SRC, FIN>), dim3(gp), dim3(256), 0, s, c, src, fin);                         \
        EL_LAUNCH("k_fism_combine", (k_fism_combine<VW_, CPL_, FIN>), dim3(gc), dim3(256), 0, s, c, fin);                 \
        EL_LAUNCH("k_fism_combine_long", (k_fism_combine_long<VW_, CPL_, FIN>), dim3(gl), dim3(256), 0, s, c, fin);       \
    } while (0)
    FI_DISPATCH(vec, cpl, FI_CUT);
#undef FI_CUT
    return 0;
}

int fism_grads(el_ctx* ctx, hipStream_t s, const el_fism_state* st, const int32_t* u, const int32_t* i, const float* y, int64_t B,
               double* loss_out, void* ws, size_t ws_bytes, const char* who) {
    EL_REQUIRE(u && i && y && loss_out, "%s: null argument", who);
    EL_REQUIRE(B >= 1 && B < (1LL << 30), "%s: batch size %lld out of range", who, (long long)B);
    FismWs w;
    const int F = st->F, piece = fism_piece(ctx);
    const int64_t U = st->U, I = st->I;
    EL_REQUIRE(fism_carve(ctx, B, U, I, st->nnz, F, ws, &w) == 0, "%s: rocprim size query failed", who);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    const bool vec = F % 4 == 0 && fism_al16(st->Gi) && fism_al16(st->Gj) && fism_al16(st->gGi) && fism_al16(st->gGj);
    int cpl = 1;
    const int lpt = fism_split(F, vec, &cpl);

    // 1: the sorted pairs, the batch's distinct users, their slots and piece counts
    const unsigned gb = (unsigned)((B + 255) / 256);
    EL_LAUNCH("k_fism_keys", k_fism_keys, dim3(gb), dim3(256), 0, s, u, i, B, (u32)U, w.key_in, w.val_in, w.split_u, w.split_i, w.cut.plen,
              w.n_max);
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
              w.cut.plen, w.n_dev);

    // 2: the pooled rows P_u and q_u of the distinct users
    {
        FismCut c = {st->h_indptr, st->h_indices, w.rows, nullptr, w.n_max, 0, piece, F, lpt, nullptr, nullptr, nullptr};
        FismFinPool fin = {st->coef, st->h_indptr, st->Gi, w.S, w.Q, 0, F};
        if (int rc = fism_run_cut(ctx, s, w.cut, c, st->nnz, vec, cpl, FismSrcHist{st->Gi}, fin, "k_fism_cut_fwd")) return rc;
    }

    // 3: scores, c_b, the partials of the loss
    const int64_t want = (B * lpt + 255) / 256, cap = fism_fwd_cap(ctx);
    const unsigned gfwd = (unsigned)(want < cap ? want : cap);
    {
        FismFwd p = {st->Gj, st->Bu, st->Bi, w.S, w.Q, st->slot, u, i, st->h_indptr, y, w.cb, B, st->pad_len, F, lpt, st->loss_kind,
                     st->beta, st->lambda, st->gamma, 1.0 / (double)B, w.lossp};
#define FI_FWD(VW_, CPL_) EL_LAUNCH("k_fism_fwd", (k_fism_fwd<VW_, CPL_>), dim3(gfwd), dim3(256), 0, s, p)
        FI_DISPATCH(vec, cpl, FI_FWD);
#undef FI_FWD
    }

    // 4: the two sorted-segment passes
    {
        FismSeg pu = {keyU, valU, 0u, w.cb, i, nullptr, st->Gj, B, F, fism_user_chunk(B), lpt, w.part, w.part_b};
        FismSeg pi = {keyI, valI, (u32)U, w.cb, u, st->slot, w.S, B, F, fism_item_chunk(B), lpt, w.part, w.part_b};
        FismFinUser fu = {keyU, B, st->coef, st->Bu, st->slot, w.R, st->gBu, w.Cn, st->lambda, F};
        FismFinItem fi = {keyI, B, (u32)U, st->Gj, st->Bi, st->gGj, st->gBi, st->beta, st->gamma, F};
        const int64_t gu = (B + pu.chunk - 1) / pu.chunk, gi = (B + pi.chunk - 1) / pi.chunk;
        const unsigned gridu = (unsigned)((gu * lpt + 255) / 256), gridi = (unsigned)((gi * lpt + 255) / 256);
        SegParts su = {keyU, 0u, B, pu.chunk, lpt, F, w.split_u, w.part, w.part_b};
        SegParts si = {keyI, (u32)U, B, pi.chunk, lpt, F, w.split_i, w.part, w.part_b};
        const unsigned glu = (unsigned)(gu < 1024 ? gu : 1024), gli = (unsigned)(gi < 1024 ? gi : 1024);
#define FI_SEG(VW_, CPL_)                                                                                                       \
    do {                                                                                                                        \
        EL_LAUNCH("k_fism_seg_user", (k_fism_seg<VW_, CPL_, FismFinUser>), dim3(gridu), dim3(256), 0, s, pu, fu);                 \
        EL_LAUNCH("k_seg_combine", (k_seg_combine<VW_, CPL_, FismFinUser>), dim3(gridu), dim3(256), 0, s, su, fu);                \
        EL_LAUNCH("k_seg_combine_long", (k_seg_combine_long<VW_, CPL_, FismFinUser>), dim3(glu), dim3(256), 0, s, su, fu);        \
        EL_LAUNCH("k_fism_seg_item", (k_fism_seg<VW_, CPL_, FismFinItem>), dim3(gridi), dim3(256), 0, s, pi, fi);                 \
        EL_LAUNCH("k_seg_combine", (k_seg_combine<VW_, CPL_, FismFinItem>), dim3(gridi), dim3(256), 0, s, si, fi);                \
        EL_LAUNCH("k_seg_combine_long", (k_seg_combine_long<VW_, CPL_, FismFinItem>), dim3(gli), dim3(256), 0, s, si, fi);        \
    } while (0)
        FI_DISPATCH(vec, cpl, FI_SEG);
#undef FI_SEG
    }

    // 5: the fan-out over the item-major lists
    {
        EL_LAUNCH("k_fism_plen", k_fism_plen, dim3((unsigned)((I + 256) / 256)), dim3(256), 0, s, st->t_indptr, I, piece, w.cut.plen);
        FismCut c = {st->t_indptr, st->t_indices, nullptr, nullptr, I, 0, piece, F, lpt, nullptr, nullptr, nullptr};
        FismFinFan fin = {st->Gi, st->gGi, st->pad_len > 0 ? w.lossp : nullptr, (int)gfwd, F, st->beta};
        if (int rc = fism_run_cut(ctx, s, w.cut, c, st->nnz, vec, cpl, FismSrcSlot{st->slot, w.R, w.Cn}, fin, "k_fism_cut_fan")) return rc;
    }

    // 6: the loss; the slot map is -1 again
    EL_LAUNCH("k_fism_finish", k_fism_finish, dim3(el_stream_grid(ctx, w.n_max)), dim3(256), 0, s, w.rows, w.n_dev, st->slot, w.lossp, (int)gfwd,
              st->Gi, F, st->beta, loss_out);
    EL_CHECK_LAUNCH();
    return 0;
}

int fism_apply(el_ctx* ctx, hipStream_t s, const el_fism_state* st, float lr_t) {
    const int64_t ne = st->I * (int64_t)st->F;
    struct V {
        const char* nm;
        float *th, *g, *m, *v;
        int64_t n;
    } vars[4] = {{"k_fism_opt_Gi", st->Gi, st->gGi, st->mGi, st->vGi, ne}, {"k_fism_opt_Gj", st->Gj, st->gGj, st->mGj, st->vGj, ne},
                 {"k_fism_opt_Bu", st->Bu, st->gBu, st->mBu, st->vBu, st->U}, {"k_fism_opt_Bi", st->Bi, st->gBi, st->mBi, st->vBi, st->I}};
    for (const V& x : vars)
        EL_LAUNCH(x.nm, k_adam_dense, dim3(el_stream_grid(ctx, x.n / 4 + 1)), dim3(256), 0, s, x.th, x.g, x.m, x.v, x.n, lr_t, 0.9f, 0.999f,
                  1e-7f);
    EL_CHECK_LAUNCH();
    return 0;
}

size_t fism_image_carve(int64_t U, int64_t nnz, int piece, int F, void* base, FismCutWs* w) {
    ElCarve c{(char*)base};
    if (fism_cut_carve(c, U, nnz, piece, F, w)) return 0;
    return c.off;
}

}  // namespace

extern "C" size_t el_fism_ws_bytes(el_ctx* ctx, int64_t B, int64_t U, int64_t I, int64_t nnz, int32_t F) {
    if (!ctx || B < 1 || B >= (1LL << 30) || U < 1 || I < 1 || nnz < 0 || F < 1 || F > 512 || fism_piece(ctx) == 0) return 0;
    FismWs w;
    if (fism_carve(ctx, B, U, I, nnz, F, nullptr, &w)) return 0;
    return w.total;
}

extern "C" size_t el_fism_image_ws_bytes(el_ctx* ctx, int64_t U, int64_t nnz, int32_t F) {
    if (!ctx || U < 1 || nnz < 0 || F < 1 || F > 512 || fism_piece(ctx) == 0) return 0;
    FismCutWs w;
    return fism_image_carve(U, nnz, fism_piece(ctx), F, nullptr, &w);
}

extern "C" int el_fism_grads(el_ctx* ctx, void* stream, const el_fism_state* st, const int32_t* u, const int32_t* i, const float* y,
                             int64_t B, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fism_check_state(ctx, st, "el_fism_grads", 1)) return rc;
    return fism_grads(ctx, (hipStream_t)stream, st, u, i, y, B, loss_out, ws, ws_bytes, "el_fism_grads");
}

extern "C" int el_fism_apply(el_ctx* ctx, void* stream, const el_fism_state* st, int32_t step, float lr_t) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fism_check_state(ctx, st, "el_fism_apply", 2)) return rc;
    EL_REQUIRE(step >= 1, "el_fism_apply: step must be >= 1");
    return fism_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_fism_train_step(el_ctx* ctx, void* stream, const el_fism_state* st, const int32_t* u, const int32_t* i, const float* y,
                                  int64_t B, int32_t step, float lr_t, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fism_check_state(ctx, st, "el_fism_train_step", 2)) return rc;
    EL_REQUIRE(step >= 1, "el_fism_train_step: step must be >= 1");
    if (int rc = fism_grads(ctx, (hipStream_t)stream, st, u, i, y, B, loss_out, ws, ws_bytes, "el_fism_train_step")) return rc;
    return fism_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_fism_forward(el_ctx* ctx, void* stream, const el_fism_state* st, const int32_t* u, const int32_t* i, int64_t n, float* out) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fism_check_state(ctx, st, "el_fism_forward", 0)) return rc;
    if (n <= 0) return 0;
    EL_REQUIRE(u && i && out && n < (1LL << 30), "el_fism_forward: bad arguments");
    const bool vec = st->F % 4 == 0 && fism_al16(st->Gi) && fism_al16(st->Gj);
    int cpl = 1;
    const int lpt = fism_split(st->F, vec, &cpl);
    const FismTabs tabs = {st->Gi, st->Gj, st->Bu, st->Bi, st->coef, st->h_indptr, st->h_indices, st->pad_len, st->F};
    const unsigned grid = (unsigned)((n * lpt + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
#define FI_PRED(VW_, CPL_) EL_LAUNCH("k_fism_predict", (k_fism_predict<VW_, CPL_>), dim3(grid), dim3(256), 0, s, tabs, u, i, n, lpt, out)
    FI_DISPATCH(vec, cpl, FI_PRED);
#undef FI_PRED
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_fism_user_image(el_ctx* ctx, void* stream, const el_fism_state* st, float* P, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fism_check_state(ctx, st, "el_fism_user_image", 0)) return rc;
    EL_REQUIRE(P != nullptr, "el_fism_user_image: null output");
    const int piece = fism_piece(ctx), F = st->F;
    FismCutWs cw;
    const size_t need = fism_image_carve(st->U, st->nnz, piece, F, ws, &cw);
    EL_REQUIRE(need != 0 && ws != nullptr && ws_bytes >= need, "el_fism_user_image: workspace too small (%zu < %zu)", ws_bytes, need);
    const bool vec = F % 4 == 0 && fism_al16(st->Gi) && fism_al16(P);
    int cpl = 1;
    const int lpt = fism_split(F, vec, &cpl);
    hipStream_t s = (hipStream_t)stream;
    EL_LAUNCH("k_fism_plen", k_fism_plen, dim3((unsigned)((st->U + 256) / 256)), dim3(256), 0, s, st->h_indptr, st->U, piece, cw.plen);
    FismCut c = {st->h_indptr, st->h_indices, nullptr, nullptr, st->U, 0, piece, F, lpt, nullptr, nullptr, nullptr};
    FismFinPool fin = {st->coef, st->h_indptr, st->Gi, P, nullptr, st->pad_len, F};
    if (int rc = fism_run_cut(ctx, s, cw, c, st->nnz, vec, cpl, FismSrcHist{st->Gi}, fin, "k_fism_cut_image")) return rc;
    EL_CHECK_LAUNCH();
    return 0;
}
