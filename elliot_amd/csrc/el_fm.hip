// FM (factorization machine over users, items and item attributes, Rendle 2010) -- contract in include/elliot_hip.h, DESIGN 3.29;
// reference: elliot/recommender/latent_factor_models/FM/factorization_machine_model.py.
//
// One table E [N, F] and one bias vector w [N], N = U + I + nF (user u = row u, item i = row U + i, feature f = row U + I + f), one
// scalar g0.  The active rows of a sample are X = {u, U + i} + A(i), A(i) the item's feature rows:
//   y^(u, i) = g0 + sum_X w_x + 1/2 (|sum_X e_x|^2 - sum_X |e_x|^2)
// Everything below the user factors through the item:  s_i = e_{U+i} + sum_A e_f,  q_i = |e_{U+i}|^2 + sum_A |e_f|^2,
// l_i = w_{U+i} + sum_A w_f,  h_i = l_i + 1/2 (|s_i|^2 - q_i)   ->   y^(u, i) = g0 + w_u + h_i + e_u . s_i.
// (1/2 (|s_i|^2 - q_i) is the sum of the pairwise products of the item's rows and is accumulated as that: fm_item_sums.)
// With c_b = 2 (y^_b - y_b) / B:  dL/de_u = sum c_b s_i,  and with T_i = sum c_b e_u, C_i = sum c_b, R_i = T_i + C_i s_i:
// dL/de_{U+i} = R_i - C_i e_{U+i},  dL/de_f = sum_{i: f in A(i)} R_i - (sum C_i) e_f;  dL/dw_x = the same sums of c_b alone.
//
// One gradient pass:
//   1. k_fm_keys        the (row, sample) sort pairs -- users as u, items as U + i -- and ONE rocprim radix sort of the 2 B pairs
//                       (stable -> a row's samples are summed in batch order)
//   2. k_fm_heads + rocprim exclusive scan: the slot n(i) of every DISTINCT item of the batch (items ascending)
//   3. k_fm_item_rows   one lane group per distinct item walks A(i) in stored order, four feature rows in flight: s_i and h_i to slot
//                       n(i) of the scratch image, slot[i] = n(i)
//   4. k_fm_fwd         one lane group per sample: y^, c_b; per workgroup one double partial of the loss and one of sum c_b
//   5. k_fm_seg_user / k_fm_seg_item: the two sorted-segment passes (the walk of k_pw_seg): gE[u] = sum c_b s_i, and per item T_i, C_i,
//                       finished by FmFinItem as R_i (kept in the slot) and the item's own row.  Cut segments go through
//                       k_seg_combine / k_seg_combine_long (el_segcombine.h) with the same functors.
//   6. k_fm_feat / k_fm_feat_long: the fan-out.  Per feature the items of its list (feature-major copy of the attribute matrix, item
//                       ids ascending) that are in the batch (slot >= 0) add R_i, C_i in list order: a lane group per feature, or,
//                       for a list of more than FM_FEAT_LONG items, a workgroup whose lane groups take contiguous shares in order
//                       and are added through LDS in lane-group order.
//   7. k_fm_finish      the partials of 4 added in index order (loss, dL/dg0); slot[] back to -1 through the list of distinct items.
// No floating-point atomics on any row, a fixed order in every sum: the same input gives the same bytes.  No matrix instruction:
// every sum is a gather or a segment sum.  The optimiser is k_adam_apply_dense (el_vae.hip: TensorFlow's fused dense ApplyAdam) on
// E and w; g0, one scalar, takes the same step in double in one thread (k_fm_adam_g0).
#include "el_common.h"
#include "el_segcombine.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

#define FM_STG 64            // list / segment positions whose index chain a lane group stages in LDS at once
#define FM_FEAT_LONG 256     // a feature on more items than this takes the workgroup route of the fan-out

struct FmTabs {
    const float *E, *w;
    const int64_t* a_ptr;     // item -> features (NULL with nF = 0)
    const int32_t* a_idx;
    int64_t U, I;
    int F;
};

// a lane's elements of one row (zero where the lane holds none or !ok)
template <int VW, int CPL>
__device__ __forceinline__ void fm_ld_row(const float* row, int F, int sub, int lpt, bool ok, float (&r)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
#pragma unroll
        for (int x = 0; x < VW; ++x) r[q][x] = 0.f;
        if (ok && e < F) ldv<VW>(row + e, r[q]);
    }
}
template <int VW, int CPL>
__device__ __forceinline__ void fm_st_row(float* row, int F, int sub, int lpt, const float (&r)[CPL][VW]) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
        if (e < F) stv<VW>(row + e, r[q]);
    }
}
template <int VW, int CPL>
__device__ __forceinline__ float fm_dot(const float (&a)[CPL][VW], const float (&b)[CPL][VW], int lpt) {
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) d = fmaf(a[q][x], b[q][x], d);
    return el_group_sum(d, lpt);
}

// s_i (this lane's elements), l_i and the pair term p_i = 1/2 (|s_i|^2 - q_i) of one item: its own row, then A(i) in stored order, four
// feature rows in flight.  p_i is accumulated as sum_k (rows before k) . (row k) -- the same number, without forming |s_i|^2 and q_i
// and cancelling them (both grow with the number of features, their difference does not)
template <int VW, int CPL>
__device__ __forceinline__ void fm_item_sums(const FmTabs& t, int64_t item, int sub, int lpt, float (&s)[CPL][VW], float& pair, float& l) {
    const int F = t.F;
    fm_ld_row<VW, CPL>(t.E + (t.U + item) * F, F, sub, lpt, true, s);
    float cr = 0.f;
    l = t.w[t.U + item];
    const int64_t a0 = t.a_ptr ? t.a_ptr[item] : 0, a1 = t.a_ptr ? t.a_ptr[item + 1] : 0;
    const float* Ef = t.E + (t.U + t.I) * F;
    const float* wf = t.w + t.U + t.I;
    for (int64_t a = a0; a < a1; a += 4) {
        float r[4][CPL][VW], wv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = a + k < a1;
            const int64_t f = t.a_idx[ok ? a + k : a];
            fm_ld_row<VW, CPL>(Ef + f * F, F, sub, lpt, ok, r[k]);
            wv[k] = ok ? wf[f] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (a + k >= a1) continue;
            l += wv[k];
#pragma unroll
            for (int q = 0; q < CPL; ++q)
#pragma unroll
                for (int x = 0; x < VW; ++x) {
                    cr = fmaf(s[q][x], r[k][q][x], cr);
                    s[q][x] += r[k][q][x];
                }
        }
    }
    pair = el_group_sum(cr, lpt);
}

// users as u, items as U + i; the counters of the two combine passes start at zero
__global__ __launch_bounds__(256) void k_fm_keys(const int32_t* __restrict__ u, const int32_t* __restrict__ i, int64_t B, u32 U,
                                                 u32* __restrict__ key, u32* __restrict__ val, int32_t* split_u, int32_t* split_i) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b == 0) split_u[0] = 0, split_i[0] = 0;
    if (b >= B) return;
    key[b] = (u32)u[b], val[b] = (u32)b;
    key[B + b] = U + (u32)i[b], val[B + b] = (u32)b;
}

// 1 at the first sorted position of every item segment (keys: the item half of the sorted pairs)
__global__ __launch_bounds__(256) void k_fm_heads(const u32* __restrict__ keys, int64_t n, int32_t* __restrict__ hd) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    hd[p] = (p == 0 || keys[p - 1] != keys[p]) ? 1 : 0;
}

// one lane group per sorted item position; the head of a segment forms its item's slot row (hs = the exclusive scan of hd = the slot)
template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fm_item_rows(FmTabs t, const u32* __restrict__ keys, const int32_t* __restrict__ hd,
                                                      const int32_t* __restrict__ hs, int64_t B, int64_t n_max, int lpt,
                                                      float* __restrict__ S, float* __restrict__ H, int32_t* __restrict__ rows,
                                                      int32_t* __restrict__ slot, int32_t* __restrict__ n_out) {
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    if (p >= B) return;
    if (p == B - 1 && sub == 0) *n_out = hs[p] + hd[p];
    if (!hd[p]) return;
    const int64_t item = (int64_t)keys[p] - t.U, sl = hs[p];
    if (item >= t.I || sl >= n_max) return;                     // (an id past the catalogue writes nothing outside the map)
    float s[CPL][VW], pair, l;
    fm_item_sums<VW, CPL>(t, item, sub, lpt, s, pair, l);
    fm_st_row<VW, CPL>(S + sl * t.F, t.F, sub, lpt, s);
    if (sub == 0) {
        H[sl] = l + pair;
        rows[sl] = (int32_t)item;
        slot[item] = (int32_t)sl;
    }
}

struct FmFwd {
    const float *E, *w, *g0, *S, *H;
    const int32_t *slot, *bu, *bi;
    const float* label;
    float* coef;
    int64_t n;
    int F, lpt;
    float inv_n;
    double* part;        // [2 gridDim.x]: per workgroup the loss and sum c_b
};

template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fm_fwd(FmFwd p) {
    const int F = p.F, lpt = p.lpt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    const float g0 = p.g0[0];
    double lossv = 0.0, csum = 0.0;
    for (int64_t b = gid / lpt; b < p.n; b += groups) {
        const int64_t u = p.bu[b], sl = p.slot[p.bi[b]];
        float a[CPL][VW], s[CPL][VW];
        fm_ld_row<VW, CPL>(p.E + u * F, F, sub, lpt, true, a);
        fm_ld_row<VW, CPL>(p.S + sl * F, F, sub, lpt, true, s);
        const float dot = fm_dot<VW, CPL>(a, s, lpt);
        if (sub == 0) {
            // (the four terms and the residual in double: one lane, a handful of operations per sample)
            const double r = (((double)g0 + (double)p.w[u]) + (double)p.H[sl]) + (double)dot - (double)p.label[b];
            const float c = (float)(2.0 * r * (double)p.inv_n);
            p.coef[b] = c;
            lossv += r * r * (double)p.inv_n;
            csum += (double)c;
        }
    }
    __shared__ double part[2][4];
    for (int o = 32; o > 0; o >>= 1) lossv += __shfl_xor(lossv, o, 64), csum += __shfl_xor(csum, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) part[0][wv] = lossv, part[1][wv] = csum;
    __syncthreads();
    if (threadIdx.x == 0) {
        p.part[2 * blockIdx.x] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        p.part[2 * blockIdx.x + 1] = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    }
}

// y^ of explicit pairs straight from the tables (the model's predict): the item's sums are formed on the fly, no scratch image
template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fm_predict(FmTabs t, const float* __restrict__ g0, const int32_t* __restrict__ bu,
                                                    const int32_t* __restrict__ bi, int64_t n, int lpt, float* __restrict__ out) {
    const int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    if (b >= n) return;
    const int64_t u = bu[b];
    float sv[CPL][VW], a[CPL][VW], pair, l;
    fm_item_sums<VW, CPL>(t, bi[b], sub, lpt, sv, pair, l);
    fm_ld_row<VW, CPL>(t.E + u * t.F, t.F, sub, lpt, true, a);
    const float dot = fm_dot<VW, CPL>(a, sv, lpt);
    if (sub == 0) out[b] = (float)((((double)g0[0] + (double)t.w[u]) + ((double)l + (double)pair)) + (double)dot);
}

// finish of a complete user row: sum c_b s_i and sum c_b, stored  (every lane of the group holds b)
struct FmFinUser {
    float *gE, *gw;
    int F;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t row, int sub, int lpt, const float (&gg)[CPL][VW], float b) const {
        fm_st_row<VW, CPL>(gE + row * F, F, sub, lpt, gg);
        if (sub == 0) gw[row] = b;
    }
};

// finish of a complete item row (T_i, C_i): R_i = T_i + C_i s_i stays in the slot for the fan-out, the item's own row takes its term out
struct FmFinItem {
    const float *E, *S;
    const int32_t* slot;
    float *gE, *gw, *R, *Cn;
    int64_t U;
    int F;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t row, int sub, int lpt, const float (&gg)[CPL][VW], float b) const {
        const int64_t sl = slot[row];
        float s[CPL][VW], e[CPL][VW], r[CPL][VW], g[CPL][VW];
        fm_ld_row<VW, CPL>(S + sl * F, F, sub, lpt, true, s);
        fm_ld_row<VW, CPL>(E + (U + row) * F, F, sub, lpt, true, e);
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) {
                r[q][x] = fmaf(b, s[q][x], gg[q][x]);
                g[q][x] = fmaf(-b, e[q][x], r[q][x]);
            }
        fm_st_row<VW, CPL>(R + sl * F, F, sub, lpt, r);
        fm_st_row<VW, CPL>(gE + (U + row) * F, F, sub, lpt, g);
        if (sub == 0) gw[U + row] = b, Cn[sl] = b;
    }
};

struct FmSeg {
    const u32 *keys, *vals;     // sorted row ids of THIS side (+ key_off) and the sample of each position
    u32 key_off;
    const float* coef;
    const int32_t* other_ids;   // the sample's row on the other side ...
    const int32_t* other_map;   // ... sent through the slot map (user pass: rows of the scratch image) or NULL (item pass: rows of E)
    const float* other;
    int64_t n;
    int F, chunk, lpt;
    float *part, *part_b;       // pieces of segments cut by chunk boundaries (el_segcombine.h)
};

// the sorted-segment walk of k_pw_seg (el_pwmf.hip): a lane group per chunk of sorted positions, the index chain staged in LDS,
// a complete segment finished here by FIN, a cut piece left in its partial slot
template <int VW, int CPL, typename FIN>
__global__ __launch_bounds__(256) void k_fm_seg(FmSeg p, FIN fin) {
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
        fm_st_row<VW, CPL>(p.part + slot * F, F, sub, lpt, acc);
        if (sub == 0) p.part_b[slot] = bacc;
    };
    __shared__ u32 s_key[32][FM_STG];
    __shared__ u32 s_oth[32][FM_STG];
    __shared__ float s_cf[32][FM_STG];
    const int gl = (int)(threadIdx.x / lpt);
    constexpr int SUB = (CPL == 1) ? 4 : (CPL == 2 ? 2 : 1);     // positions whose row loads are in flight together
    for (int64_t sbase = p0; sbase < p1; sbase += FM_STG) {
        const int cs = (int)((p1 - sbase < FM_STG) ? p1 - sbase : FM_STG);
        for (int t = sub; t < cs; t += lpt) {
            const int64_t b = (int64_t)p.vals[sbase + t];
            const int32_t o = p.other_ids[b];
            s_key[gl][t] = p.keys[sbase + t] - p.key_off;
            s_cf[gl][t] = p.coef[b];
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
                fm_ld_row<VW, CPL>(p.other + (int64_t)s_oth[gl][tt] * F, F, sub, lpt, okv[t], rr[t]);
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
#pragma unroll
                    for (int q = 0; q < CPL; ++q)
#pragma unroll
                        for (int x = 0; x < VW; ++x) acc[q][x] = 0.f;
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

struct FmFeat {
    const int64_t* t_ptr;       // feature -> items, item ids ascending
    const int32_t* t_idx;
    const int32_t* slot;
    const float *R, *Cn, *E;
    float *gE, *gw;
    int64_t row0, nF;           // row0 = U + I: the first feature row
    int F, lpt;
};

// list positions [k0, k1) of one feature, by ONE lane group: the slots of FM_STG items are staged in LDS together, then the rows of
// the items that are in the batch are added in list order, four in flight
template <int VW, int CPL>
__device__ __forceinline__ void fm_feat_walk(const FmFeat& p, int64_t k0, int64_t k1, int32_t* stage, int sub, int lpt,
                                             float (&acc)[CPL][VW], float& cacc, bool& any) {
    for (int64_t base = k0; base < k1; base += FM_STG) {
        const int cs = (int)((k1 - base < FM_STG) ? k1 - base : FM_STG);
        for (int t = sub; t < cs; t += lpt) stage[t] = p.slot[p.t_idx[base + t]];
        el_wave_lds_sync();
        for (int b4 = 0; b4 < cs; b4 += 4) {
            int32_t sl[4];
            float r[4][CPL][VW], cv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sl[k] = b4 + k < cs ? stage[b4 + k] : -1;
                fm_ld_row<VW, CPL>(p.R + (int64_t)(sl[k] < 0 ? 0 : sl[k]) * p.F, p.F, sub, lpt, sl[k] >= 0, r[k]);
                cv[k] = sl[k] >= 0 ? p.Cn[sl[k]] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (sl[k] < 0) continue;
                any = true;
                cacc += cv[k];
#pragma unroll
                for (int q = 0; q < CPL; ++q)
#pragma unroll
                    for (int x = 0; x < VW; ++x) acc[q][x] += r[k][q][x];
            }
        }
        el_wave_lds_sync();
    }
}

// gE[f] = sum R_i - (sum C_i) e_f, gw[f] = sum C_i
template <int VW, int CPL>
__device__ __forceinline__ void fm_feat_store(const FmFeat& p, int64_t f, int sub, int lpt, const float (&acc)[CPL][VW], float c) {
    float e[CPL][VW], g[CPL][VW];
    fm_ld_row<VW, CPL>(p.E + (p.row0 + f) * p.F, p.F, sub, lpt, true, e);
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) g[q][x] = fmaf(-c, e[q][x], acc[q][x]);
    fm_st_row<VW, CPL>(p.gE + (p.row0 + f) * p.F, p.F, sub, lpt, g);
    if (sub == 0) p.gw[p.row0 + f] = c;
}

// short lists: one lane group per feature
template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fm_feat(FmFeat p) {
    __shared__ int32_t s_sl[32][FM_STG];
    const int lpt = p.lpt;
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1)), gl = (int)(threadIdx.x / lpt);
    if (f >= p.nF) return;
    const int64_t t0 = p.t_ptr[f], t1 = p.t_ptr[f + 1];
    if (t1 - t0 > FM_FEAT_LONG) return;
    float acc[CPL][VW], cacc = 0.f;
    bool any = false;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) acc[q][x] = 0.f;
    fm_feat_walk<VW, CPL>(p, t0, t1, s_sl[gl], sub, lpt, acc, cacc, any);
    if (any) fm_feat_store<VW, CPL>(p, f, sub, lpt, acc, cacc);       // (no item of the batch: the accumulator row is zero already)
}

// long lists: one workgroup per feature; its 256 / lpt lane groups (64 / lpt per wave, waves in order) take contiguous shares of the
// list in order, the shares are added through LDS in lane-group order
template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fm_feat_long(FmFeat p) {
    __shared__ int32_t s_sl[32][FM_STG];
    __shared__ __attribute__((aligned(16))) float s_red[4096];      // (256 / lpt) lane groups x F floats, as k_seg_combine_long
    __shared__ float s_rc[32];
    __shared__ int s_any[32];
    const int F = p.F, lpt = p.lpt;
    const int ngl = 256 / lpt, gl = (int)(threadIdx.x / lpt), sub = (int)(threadIdx.x & (lpt - 1));
    for (int64_t f = blockIdx.x; f < p.nF; f += gridDim.x) {
        const int64_t t0 = p.t_ptr[f], t1 = p.t_ptr[f + 1], len = t1 - t0;
        if (len <= FM_FEAT_LONG) continue;                           // (uniform over the workgroup)
        const int64_t per = (len + ngl - 1) / ngl;
        const int64_t k0 = t0 + gl * per < t1 ? t0 + gl * per : t1, k1 = k0 + per < t1 ? k0 + per : t1;
        float acc[CPL][VW], cacc = 0.f;
        bool any = false;
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int x = 0; x < VW; ++x) acc[q][x] = 0.f;
        fm_feat_walk<VW, CPL>(p, k0, k1, s_sl[gl], sub, lpt, acc, cacc, any);
        fm_st_row<VW, CPL>(s_red + gl * F, F, sub, lpt, acc);
        if (sub == 0) s_rc[gl] = cacc, s_any[gl] = any ? 1 : 0;
        __syncthreads();
        if (gl == 0) {
            float c = 0.f, gg[CPL][VW];
            int seen = 0;
            for (int h = 0; h < ngl; ++h) c += s_rc[h], seen |= s_any[h];
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
            if (seen) fm_feat_store<VW, CPL>(p, f, sub, lpt, gg, c);
        }
        __syncthreads();
    }
}

// the step's two scalars from the per-workgroup partials in index order (workgroup 0), and the slot map back to -1 through the list of
// the batch's distinct items (every workgroup): the last kernel that reads the map clears it
__global__ __launch_bounds__(256) void k_fm_finish(const int32_t* __restrict__ rows, const int32_t* __restrict__ n_dev,
                                                   int32_t* __restrict__ slot, const double* __restrict__ part, int nparts,
                                                   double* loss_out, double* gg0) {
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
        *loss_out += red[0][0];
        *gg0 = red[1][0];
    }
}

// The global bias's step of TensorFlow's fused dense ApplyAdam, one thread.  g0 is ONE scalar that every sample of every batch moves:
// its gradient arrives as the double it was reduced in, and the variable and its two slots are kept as doubles (g0d, m, v) -- three
// words of state.  A float scalar that is rounded at every step drifts by up to half an ulp per step, and v would lose another ulp to
// a float gradient squared; nothing averages that out as it does over the rows of a table.  Same formula and the same float constants
// (1 - beta, epsilon, lr_t) as k_adam_apply_dense.  The kernels read g0, the float image of g0d, rewritten here.  Clears the gradient.
__global__ void k_fm_adam_g0(float* g0, double* g0d, double* gg0, double* m, double* v, float lr_t) {
    const double g = *gg0, omb1 = (double)(1.0f - 0.9f), omb2 = (double)(1.0f - 0.999f);
    const double mm = *m + (g - *m) * omb1, vv = *v + (g * g - *v) * omb2;
    const double th = *g0d - (mm * (double)lr_t) / (sqrt(vv) + (double)1e-7f);
    *m = mm, *v = vv, *g0d = th;
    *g0 = (float)th;
    *gg0 = 0.0;
}

// Q [I, F] = s_i, bq [I] = g0 + h_i for ALL items: y^(u, i) = w_u + bq[i] + E[u] . Q[i]
template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_fm_image(FmTabs t, const float* __restrict__ g0, int lpt, float* __restrict__ Q,
                                                  float* __restrict__ bq) {
    const int64_t item = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    if (item >= t.I) return;
    float s[CPL][VW], pair, l;
    fm_item_sums<VW, CPL>(t, item, sub, lpt, s, pair, l);
    fm_st_row<VW, CPL>(Q + item * t.F, t.F, sub, lpt, s);
    if (sub == 0) bq[item] = g0[0] + (l + pair);
}

// y_b = the rating of (u_b, i_b) where the sampler's coin said positive, else 0 (pointwise_pos_neg_ratings_sampler.py); a positive
// the row does not hold is 0
__global__ __launch_bounds__(256) void k_fm_labels(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                   const float* __restrict__ values, const int32_t* __restrict__ u,
                                                   const int32_t* __restrict__ i, const float* coin, int64_t n, float* y) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    float v = 0.f;
    if (coin[b] > 0.f) {
        const int64_t r0 = indptr[u[b]], r1 = indptr[u[b] + 1], pos = el_lower_bound(indices, r0, r1, i[b]);
        if (pos < r1 && indices[pos] == i[b]) v = values[pos];
    }
    y[b] = v;
}

struct FmWs {
    u32 *key_in, *val_in, *key, *val;
    float* coef;
    int32_t *hd, *hs, *rows, *n_dev;
    float *S, *H, *R, *Cn;
    double* lossp;
    void *sort_tmp, *scan_tmp;
    size_t sort_bytes, scan_bytes, total;
    float *part, *part_b;
    int32_t *split_u, *split_i;
    int64_t n_max;
};

// positions per lane group of the two passes: the point-wise step's (el_pwmf.hip)
int fm_item_chunk(int64_t n) {
    const int64_t c = n / 16384;
    return (int)(c < 16 ? 16 : (c > 256 ? 256 : c));
}
int fm_user_chunk(int64_t n) {
    const int64_t c = n / 65536;
    return (int)(c < 4 ? 4 : (c > 16 ? 16 : c));
}
int64_t fm_fwd_cap(el_ctx* ctx) { return (int64_t)ctx->cus * 16; }

int fm_carve(el_ctx* ctx, int64_t B, int64_t U, int64_t I, int F, void* base, FmWs* w) {
    ElCarve c{(char*)base};
    const int64_t n = 2 * B, n_max = B < I ? B : I;
    w->n_max = n_max;
    w->key_in = c.take<u32>((size_t)n);
    w->val_in = c.take<u32>((size_t)n);
    w->key = c.take<u32>((size_t)n);
    w->val = c.take<u32>((size_t)n);
    w->coef = c.take<float>((size_t)B);
    w->hd = c.take<int32_t>((size_t)B);
    w->hs = c.take<int32_t>((size_t)B);
    w->rows = c.take<int32_t>((size_t)n_max);
    w->n_dev = c.take<int32_t>(1);
    w->S = c.take<float>((size_t)n_max * (size_t)F);
    w->H = c.take<float>((size_t)n_max);
    w->R = c.take<float>((size_t)n_max * (size_t)F);
    w->Cn = c.take<float>((size_t)n_max);
    w->lossp = c.take<double>((size_t)(2 * fm_fwd_cap(ctx)));
    size_t t1 = 0, t2 = 0;
    u32* np = nullptr;
    int32_t* ip = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (unsigned)n, 0, el_bits_for(U + I), (hipStream_t)0) != hipSuccess) return 1;
    if (rocprim::exclusive_scan(nullptr, t2, ip, ip, (int32_t)0, (size_t)B, rocprim::plus<int32_t>(), (hipStream_t)0) != hipSuccess) return 1;
    w->sort_bytes = t1, w->scan_bytes = t2;
    w->sort_tmp = c.take<char>(t1);
    w->scan_tmp = c.take<char>(t2);
    const int cu = fm_user_chunk(B), ci = fm_item_chunk(B), cm = cu < ci ? cu : ci;
    const int64_t groups = (B + cm - 1) / cm + 1;
    w->part = c.take<float>((size_t)2 * groups * (size_t)F);
    w->part_b = c.take<float>((size_t)2 * groups);
    w->split_u = c.take<int32_t>((size_t)(2 * groups + 4));
    w->split_i = c.take<int32_t>((size_t)(2 * groups + 4));
    w->total = c.off;
    return 0;
}

bool fm_al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

int fm_check_state(const el_fm_state* st, const char* who, bool train) {
    EL_REQUIRE(st != nullptr, "%s: null state", who);
    EL_REQUIRE(st->U > 0 && st->I > 0 && st->nF >= 0, "%s: bad shape U=%lld I=%lld nF=%lld", who, (long long)st->U, (long long)st->I,
               (long long)st->nF);
    EL_REQUIRE(st->F >= 1 && st->F <= 512, "%s: F=%d out of range (1 .. 512)", who, st->F);
    EL_REQUIRE(st->U + st->I < (1LL << 32), "%s: U + I must fit a 32-bit sort key", who);
    EL_REQUIRE(st->E && st->w && st->g0, "%s: null tables", who);
    EL_REQUIRE(st->nF == 0 || (st->a_indptr && st->a_indices && st->t_indptr && st->t_indices), "%s: nF > 0 needs both index structures", who);
    if (train) {
        EL_REQUIRE(st->gE && st->gw && st->gg0 && st->slot, "%s: needs the accumulators gE / gw / gg0 and the slot map", who);
    }
    return 0;
}

FmTabs fm_tabs(const el_fm_state* st) {
    const bool feats = st->nF > 0;
    return FmTabs{st->E, st->w, feats ? st->a_indptr : nullptr, feats ? st->a_indices : nullptr, st->U, st->I, st->F};
}

// the row split: 16-byte lanes where the rows allow it (VW = 4: up to 2 vectors per lane), else one float per lane and up to 8
#define FM_DISPATCH(vec, cpl, CALL)      \
    do {                                 \
        if (vec) {                       \
            if ((cpl) == 1) CALL(4, 1);  \
            else CALL(4, 2);             \
        } else if ((cpl) == 1) CALL(1, 1); \
        else if ((cpl) == 2) CALL(1, 2); \
        else if ((cpl) == 4) CALL(1, 4); \
        else CALL(1, 8);                 \
    } while (0)

int fm_split(int F, bool vec, int* cpl) { return el_pick_lpt(F, vec ? 4 : 1, cpl); }

int fm_grads(el_ctx* ctx, hipStream_t s, const el_fm_state* st, const int32_t* u, const int32_t* i, const float* y, int64_t B,
             double* loss_out, void* ws, size_t ws_bytes, const char* who) {
    if (int rc = fm_check_state(st, who, true)) return rc;
    EL_REQUIRE(u && i && y && loss_out, "%s: null argument", who);
    EL_REQUIRE(B >= 1 && B < (1LL << 30), "%s: batch size %lld out of range", who, (long long)B);
    FmWs w;
    const int F = st->F;
    const int64_t U = st->U, I = st->I;
    EL_REQUIRE(fm_carve(ctx, B, U, I, F, ws, &w) == 0, "%s: rocprim size query failed", who);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    const bool vec = F % 4 == 0 && fm_al16(st->E) && fm_al16(st->gE);
    int cpl = 1;
    const int lpt = fm_split(F, vec, &cpl);
    const FmTabs tabs = fm_tabs(st);

    // 1-3: the sorted pairs, the batch's distinct items and their slot rows
    const unsigned gb = (unsigned)((B + 255) / 256), grow = (unsigned)((B * lpt + 255) / 256);
    EL_LAUNCH("k_fm_keys", k_fm_keys, dim3(gb), dim3(256), 0, s, u, i, B, (u32)U, w.key_in, w.val_in, w.split_u, w.split_i);
    {
        ElKernelTimer t("rocprim_radix_sort_pairs", s);
        size_t tb = w.sort_bytes;
        EL_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tb, w.key_in, w.key, w.val_in, w.val, (unsigned)(2 * B), 0, el_bits_for(U + I), s));
    }
    const u32 *keyU = w.key, *keyI = w.key + B, *valU = w.val, *valI = w.val + B;
    EL_LAUNCH("k_fm_heads", k_fm_heads, dim3(gb), dim3(256), 0, s, keyI, B, w.hd);
    {
        ElKernelTimer t("rocprim_exclusive_scan", s);
        size_t tb = w.scan_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(w.scan_tmp, tb, w.hd, w.hs, (int32_t)0, (size_t)B, rocprim::plus<int32_t>(), s));
    }
#define FM_ROWS(VW_, CPL_)                                                                                                        \
    EL_LAUNCH("k_fm_item_rows", (k_fm_item_rows<VW_, CPL_>), dim3(grow), dim3(256), 0, s, tabs, keyI, w.hd, w.hs, B, w.n_max, lpt, w.S, \
              w.H, w.rows, st->slot, w.n_dev)
    FM_DISPATCH(vec, cpl, FM_ROWS);
#undef FM_ROWS

    // 4: scores, c_b, the partials of the loss and of dL/dg0
    const int64_t want = (B * lpt + 255) / 256, cap = fm_fwd_cap(ctx);
    const unsigned gfwd = (unsigned)(want < cap ? want : cap);
    {
        FmFwd p = {st->E, st->w, st->g0, w.S, w.H, st->slot, u, i, y, w.coef, B, F, lpt, 1.0f / (float)B, w.lossp};
#define FM_FWD(VW_, CPL_) EL_LAUNCH("k_fm_fwd", (k_fm_fwd<VW_, CPL_>), dim3(gfwd), dim3(256), 0, s, p)
        FM_DISPATCH(vec, cpl, FM_FWD);
#undef FM_FWD
    }

    // 5: the two sorted-segment passes
    {
        FmSeg pu = {keyU, valU, 0u, w.coef, i, st->slot, w.S, B, F, fm_user_chunk(B), lpt, w.part, w.part_b};
        FmSeg pi = {keyI, valI, (u32)U, w.coef, u, nullptr, st->E, B, F, fm_item_chunk(B), lpt, w.part, w.part_b};
        FmFinUser fu = {st->gE, st->gw, F};
        FmFinItem fi = {st->E, w.S, st->slot, st->gE, st->gw, w.R, w.Cn, U, F};
        const int64_t gu = (B + pu.chunk - 1) / pu.chunk, gi = (B + pi.chunk - 1) / pi.chunk;
        const unsigned gridu = (unsigned)((gu * lpt + 255) / 256), gridi = (unsigned)((gi * lpt + 255) / 256);
        SegParts su = {keyU, 0u, B, pu.chunk, lpt, F, w.split_u, w.part, w.part_b};
        SegParts si = {keyI, (u32)U, B, pi.chunk, lpt, F, w.split_i, w.part, w.part_b};
        const unsigned glu = (unsigned)(gu < 1024 ? gu : 1024), gli = (unsigned)(gi < 1024 ? gi : 1024);
#define FM_SEG(VW_, CPL_)                                                                                                       \
    do {                                                                                                                        \
        EL_LAUNCH("k_fm_seg_user", (k_fm_seg<VW_, CPL_, FmFinUser>), dim3(gridu), dim3(256), 0, s, pu, fu);                       \
        EL_LAUNCH("k_seg_combine", (k_seg_combine<VW_, CPL_, FmFinUser>), dim3(gridu), dim3(256), 0, s, su, fu);                  \
        EL_LAUNCH("k_seg_combine_long", (k_seg_combine_long<VW_, CPL_, FmFinUser>), dim3(glu), dim3(256), 0, s, su, fu);          \
        EL_LAUNCH("k_fm_seg_item", (k_fm_seg<VW_, CPL_, FmFinItem>), dim3(gridi), dim3(256), 0, s, pi, fi);                       \
        EL_LAUNCH("k_seg_combine", (k_seg_combine<VW_, CPL_, FmFinItem>), dim3(gridi), dim3(256), 0, s, si, fi);                  \
        EL_LAUNCH("k_seg_combine_long", (k_seg_combine_long<VW_, CPL_, FmFinItem>), dim3(gli), dim3(256), 0, s, si, fi);          \
    } while (0)
        FM_DISPATCH(vec, cpl, FM_SEG);
#undef FM_SEG
    }

    // 6: the fan-out to the feature rows
    if (st->nF > 0) {
        FmFeat p = {st->t_indptr, st->t_indices, st->slot, w.R, w.Cn, st->E, st->gE, st->gw, U + I, st->nF, F, lpt};
        const unsigned gs = (unsigned)((st->nF * lpt + 255) / 256);
        const int64_t capl = (int64_t)ctx->cus * 4;
        const unsigned gl = (unsigned)(st->nF < capl ? st->nF : capl);
        const bool any_long = st->t_longest > FM_FEAT_LONG;
#define FM_FEAT(VW_, CPL_)                                                                                        \
    do {                                                                                                          \
        EL_LAUNCH("k_fm_feat", (k_fm_feat<VW_, CPL_>), dim3(gs), dim3(256), 0, s, p);                             \
        if (any_long) EL_LAUNCH("k_fm_feat_long", (k_fm_feat_long<VW_, CPL_>), dim3(gl), dim3(256), 0, s, p);     \
    } while (0)
        FM_DISPATCH(vec, cpl, FM_FEAT);
#undef FM_FEAT
    }

    // 7: the two scalars; the slot map is -1 again
    EL_LAUNCH("k_fm_finish", k_fm_finish, dim3(el_stream_grid(ctx, w.n_max)), dim3(256), 0, s, w.rows, w.n_dev, st->slot, w.lossp, (int)gfwd,
              loss_out, st->gg0);
    EL_CHECK_LAUNCH();
    return 0;
}

int fm_apply(el_ctx* ctx, hipStream_t s, const el_fm_state* st, float lr_t) {
    EL_REQUIRE(st->mE && st->vE && st->mw && st->vw && st->g0d && st->mg0 && st->vg0, "el_fm_apply: Adam slots missing");
    const int64_t N = st->U + st->I + st->nF, ne = N * (int64_t)st->F;
    EL_LAUNCH("k_adam_apply_dense_E", k_adam_apply_dense, dim3(el_stream_grid(ctx, ne)), dim3(256), 0, s, st->E, st->gE, st->mE, st->vE, ne, lr_t,
              0.9f, 0.999f, 1e-7f, 1);
    EL_LAUNCH("k_adam_apply_dense_w", k_adam_apply_dense, dim3(el_stream_grid(ctx, N)), dim3(256), 0, s, st->w, st->gw, st->mw, st->vw, N, lr_t,
              0.9f, 0.999f, 1e-7f, 1);
    EL_LAUNCH("k_fm_adam_g0", k_fm_adam_g0, dim3(1), dim3(1), 0, s, st->g0, st->g0d, st->gg0, st->mg0, st->vg0, lr_t);
    EL_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t el_fm_ws_bytes(el_ctx* ctx, int64_t B, int64_t U, int64_t I, int32_t F) {
    if (!ctx || B < 1 || B >= (1LL << 30) || U < 1 || I < 1 || F < 1 || F > 512) return 0;
    FmWs w;
    if (fm_carve(ctx, B, U, I, F, nullptr, &w)) return 0;
    return w.total;
}

extern "C" int el_fm_grads(el_ctx* ctx, void* stream, const el_fm_state* st, const int32_t* u, const int32_t* i, const float* y, int64_t B,
                           double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    return fm_grads(ctx, (hipStream_t)stream, st, u, i, y, B, loss_out, ws, ws_bytes, "el_fm_grads");
}

extern "C" int el_fm_apply(el_ctx* ctx, void* stream, const el_fm_state* st, int32_t step, float lr_t) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fm_check_state(st, "el_fm_apply", true)) return rc;
    EL_REQUIRE(step >= 1, "el_fm_apply: step must be >= 1");
    return fm_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_fm_train_step(el_ctx* ctx, void* stream, const el_fm_state* st, const int32_t* u, const int32_t* i, const float* y,
                                int64_t B, int32_t step, float lr_t, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fm_check_state(st, "el_fm_train_step", true)) return rc;
    EL_REQUIRE(step >= 1, "el_fm_train_step: step must be >= 1");
    EL_REQUIRE(st->mE && st->vE && st->mw && st->vw && st->g0d && st->mg0 && st->vg0, "el_fm_train_step: Adam slots missing");
    if (int rc = fm_grads(ctx, (hipStream_t)stream, st, u, i, y, B, loss_out, ws, ws_bytes, "el_fm_train_step")) return rc;
    return fm_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_fm_forward(el_ctx* ctx, void* stream, const el_fm_state* st, const int32_t* u, const int32_t* i, int64_t n, float* out) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fm_check_state(st, "el_fm_forward", false)) return rc;
    if (n <= 0) return 0;
    EL_REQUIRE(u && i && out && n < (1LL << 30), "el_fm_forward: bad arguments");
    const bool vec = st->F % 4 == 0 && fm_al16(st->E);
    int cpl = 1;
    const int lpt = fm_split(st->F, vec, &cpl);
    const FmTabs tabs = fm_tabs(st);
    const unsigned grid = (unsigned)((n * lpt + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
#define FM_PRED(VW_, CPL_) EL_LAUNCH("k_fm_predict", (k_fm_predict<VW_, CPL_>), dim3(grid), dim3(256), 0, s, tabs, st->g0, u, i, n, lpt, out)
    FM_DISPATCH(vec, cpl, FM_PRED);
#undef FM_PRED
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_fm_item_image(el_ctx* ctx, void* stream, const el_fm_state* st, float* Q, float* bq) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = fm_check_state(st, "el_fm_item_image", false)) return rc;
    EL_REQUIRE(Q && bq, "el_fm_item_image: null output");
    const bool vec = st->F % 4 == 0 && fm_al16(st->E) && fm_al16(Q);
    int cpl = 1;
    const int lpt = fm_split(st->F, vec, &cpl);
    const FmTabs tabs = fm_tabs(st);
    const unsigned grid = (unsigned)((st->I * lpt + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
#define FM_IMG(VW_, CPL_) EL_LAUNCH("k_fm_image", (k_fm_image<VW_, CPL_>), dim3(grid), dim3(256), 0, s, tabs, st->g0, lpt, Q, bq)
    FM_DISPATCH(vec, cpl, FM_IMG);
#undef FM_IMG
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_fm_labels(el_ctx* ctx, void* stream, const int64_t* indptr, const int32_t* indices, const float* values, const int32_t* u,
                            const int32_t* i, const float* coin, int64_t n, float* y) {
    if (int rc = el_bind(ctx)) return rc;
    if (n <= 0) return 0;
    EL_REQUIRE(indptr && indices && values && u && i && coin && y, "el_fm_labels: null argument");
    EL_LAUNCH("k_fm_labels", k_fm_labels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, indptr, indices, values, u, i,
              coin, n, y);
    EL_CHECK_LAUNCH();
    return 0;
}
