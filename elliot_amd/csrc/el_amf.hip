// AMF / APR (adversarial matrix factorisation, He et al. 2018) on top of the BPR-MF state -- contract in include/elliot_hip.h,
// DESIGN 3.27; reference: elliot/recommender/adversarial/AMF/AMF_model.py.
//
// Variables, accumulators and Adam slots are an el_bprmf_state (dense accumulators); the two perturbation tables dGu / dGi and the
// list of their non-zero rows are an el_amf_delta.  Nothing here runs the optimiser: el_amf_grads leaves the summed row gradients
// of the batch in gGu / gGi / gBi exactly where el_bprmf_grads leaves them, and the unchanged el_bprmf_apply consumes them.
//
// One gradient pass:
//   1. k_amf_fwd        one lane group per triplet: ONE read of its three (theta, delta) row pairs gives x~ (perturbed rows) and x
//                       (plain rows), the loss, s~ = sigma(-x~) and s = sigma(-x) (0 where the clip blocks the gradient), and the
//                       (row, triplet) sort pairs -- users as u, items as U + i; a negative occurrence carries bit 31 of its value
//   2. ONE rocprim radix sort of the 3 B pairs (stable -> a row's occurrences are summed in batch order)
//   3. k_amf_seg        one lane group per chunk of sorted positions walks its segments: a user occurrence adds
//                       -s~ (i~ - j~) - l_adv s (g_i - g_j), an item occurrence -+(s~ u~ + l_adv s g_u), the L2 term is count * l_w *
//                       (the row as gathered) at the end of the piece.  A segment inside one chunk is finished there, the pieces of
//                       a cut one go to partial slots that k_seg_combine / k_seg_combine_long add in a FIXED order (el_segcombine.h):
//                       no floating-point atomics on a table row, the same bytes on every run.
// A finished row goes to a functor: AmfStore writes it to the accumulators, AmfFgsm normalises it and writes eps * g / |g| to the
// perturbation tables (build_perturbation).  The adversarial step reads the OLD delta in 1 and 3; the old rows are then cleared
// from the device list (k_amf_clear), the batch's distinct rows become the new list (k_amf_list, from the sorted keys) and a second
// k_amf_seg over the same sorted pairs -- plain rows, coefficient s -- writes the new delta through AmfFgsm: every read of the old
// delta is a kernel boundary ahead of the first write of the new one.
// MSAP (build_msap_perturbation) runs passes 1 and 3 per round into the accumulators and k_amf_msap_rows -- one lane group per
// distinct row of the batch -- moves delta by eps_iter * g / |g|, clips it to +-eps and clears the accumulator rows again.
// No kernel but k_amf_add (the scratch tables of predict(adversarial=True)) touches a U x F or I x F array end to end.
#include "el_common.h"
#include "el_segcombine.h"

#include <cstdlib>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

#define AMF_NEG 0x80000000u
#define AMF_STG 32

struct AmfFwd {
    const float *Gu, *Gi, *Bi, *dGu, *dGi;   // dGu == nullptr: the plain rows stand for the perturbed ones
    const int32_t *u, *i, *j;
    float* coefT;                             // [B] s~ (at the rows the pass gathers)
    float* coefP;                             // [B] s at the plain rows, or nullptr (no adversarial term)
    u32 *key, *val;                           // [3 B] sort pairs, or nullptr (already ordered)
    int64_t B;
    u32 U;
    int F, lpt;
    float l_w, l_b, l_adv;
    double* loss_out;                         // or nullptr
};

template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_amf_fwd(AmfFwd p) {
    const int F = p.F, lpt = p.lpt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    double lossv = 0.0;
    for (int64_t b = gid / lpt; b < p.B; b += groups) {
        const int64_t u = p.u[b], i = p.i[b], j = p.j[b];
        float dti = 0.f, dtj = 0.f, dpi = 0.f, dpj = 0.f, sq = 0.f;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = (sub + q * lpt) * VW;
            if (e < F) {
                float gu[VW], gi[VW], gj[VW];
                ldv<VW>(p.Gu + u * F + e, gu);
                ldv<VW>(p.Gi + i * F + e, gi);
                ldv<VW>(p.Gi + j * F + e, gj);
                float tu[VW], ti[VW], tj[VW];
#pragma unroll
                for (int x = 0; x < VW; ++x) tu[x] = gu[x], ti[x] = gi[x], tj[x] = gj[x];
                if (p.dGu) {
                    float du[VW], di[VW], dj[VW];
                    ldv<VW>(p.dGu + u * F + e, du);
                    ldv<VW>(p.dGi + i * F + e, di);
                    ldv<VW>(p.dGi + j * F + e, dj);
#pragma unroll
                    for (int x = 0; x < VW; ++x) tu[x] += du[x], ti[x] += di[x], tj[x] += dj[x];
                }
#pragma unroll
                for (int x = 0; x < VW; ++x) {
                    dti = fmaf(tu[x], ti[x], dti);
                    dtj = fmaf(tu[x], tj[x], dtj);
                    sq += tu[x] * tu[x] + ti[x] * ti[x] + tj[x] * tj[x];
                    if (p.coefP) {
                        dpi = fmaf(gu[x], gi[x], dpi);
                        dpj = fmaf(gu[x], gj[x], dpj);
                    }
                }
            }
        }
        dti = el_group_sum(dti, lpt);
        dtj = el_group_sum(dtj, lpt);
        sq = el_group_sum(sq, lpt);
        if (p.coefP) {
            dpi = el_group_sum(dpi, lpt);
            dpj = el_group_sum(dpj, lpt);
        }
        if (sub == 0) {
            const float bi = p.Bi[i], bj = p.Bi[j];
            const float xt = (bi + dti) - (bj + dtj);
            const float ct = fminf(fmaxf(xt, -80.0f), 1e8f);
            p.coefT[b] = (xt >= -80.0f && xt <= 1e8f) ? 1.0f / (1.0f + expf(ct)) : 0.f;
            // (the terms of one triplet are added in double: a clipped triplet's 80 would otherwise round the small ones away)
            double l = (double)el_softplus_tf(-ct) + (double)(p.l_w * 0.5f * sq) + (double)(p.l_b * 0.5f * bi * bi) +
                       (double)(p.l_b * 0.5f * bj * bj / 10.0f);
            if (p.coefP) {
                const float xp = (bi + dpi) - (bj + dpj);
                const float cp = fminf(fmaxf(xp, -80.0f), 1e8f);
                p.coefP[b] = (xp >= -80.0f && xp <= 1e8f) ? 1.0f / (1.0f + expf(cp)) : 0.f;
                l += (double)(p.l_adv * el_softplus_tf(-cp));
            }
            lossv += l;
            if (p.key) {
                p.key[b] = (u32)u, p.val[b] = (u32)b;
                p.key[p.B + b] = p.U + (u32)i, p.val[p.B + b] = (u32)b;
                p.key[2 * p.B + b] = p.U + (u32)j, p.val[2 * p.B + b] = (u32)b | AMF_NEG;
            }
        }
    }
    if (p.loss_out) {
        __shared__ double part[4];
        double l = lossv;
        for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0) part[wv] = l;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double t = (part[0] + part[1]) + (part[2] + part[3]);
            if (t != 0.0) atomicAdd(p.loss_out, t);
        }
    }
}

// finish of a complete row (key < U: user row `key`, else item row key - U): into the accumulators
struct AmfStore {
    float *gGu, *gGi, *gBi;
    int64_t U;
    int F;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t key, int sub, int lpt, const float (&gg)[CPL][VW], float b) const {
        const bool user = key < U;
        float* g = user ? gGu + key * F : gGi + (key - U) * F;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = (sub + q * lpt) * VW;
            if (e < F) stv<VW>(g + e, gg[q]);
        }
        if (sub == 0 && !user) gBi[key - U] = b;
    }
};

// tf.nn.l2_normalize(g, 1) * eps = g * rsqrt(max(sum g^2, 1e-12)) * eps of ONE row held by a lane group (AMF_model.py:160-161)
template <int CPL, int VW>
__device__ __forceinline__ float amf_row_rnorm(const float (&gg)[CPL][VW], int lpt) {
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int x = 0; x < VW; ++x) ss = fmaf(gg[q][x], gg[q][x], ss);   // (lanes past F hold zeros)
    ss = el_group_sum(ss, lpt);
    return 1.0f / sqrtf(fmaxf(ss, 1e-12f));
}

// The list of the batch's distinct rows from the sorted keys: one thread per sorted position, a segment's first position stands for
// its row.  A workgroup counts its heads and claims room with ONE integer atomic per table (one atomic per row on the two counters
// cost 9 ms at 750 K rows); the order of the list is not fixed, its content is.
__global__ __launch_bounds__(256) void k_amf_list(const u32* __restrict__ keys, int64_t n, int64_t U, int64_t I, el_amf_delta d) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool head = p < n && (p == 0 || keys[p - 1] != keys[p]);
    const int64_t key = head ? (int64_t)keys[p] : 0;
    const bool hu = head && key < U, hi = head && key >= U;
    __shared__ int s_cnt[2][4], s_base[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bu = __ballot(hu), bi = __ballot(hi);
    if (lane == 0) s_cnt[0][wv] = __popcll(bu), s_cnt[1][wv] = __popcll(bi);
    __syncthreads();
    if (threadIdx.x < 2) {
        const int tot = s_cnt[threadIdx.x][0] + s_cnt[threadIdx.x][1] + s_cnt[threadIdx.x][2] + s_cnt[threadIdx.x][3];
        s_base[threadIdx.x] = tot ? atomicAdd(d.counts + threadIdx.x, tot) : 0;
    }
    __syncthreads();
    if (!head) return;
    const int t = hu ? 0 : 1;
    int64_t e = s_base[t] + __popcll((hu ? bu : bi) & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) e += s_cnt[t][w];
    if (hu) {
        if (e < U) d.rows_u[e] = (int32_t)key;
    } else if (e < I) {
        d.rows_i[e] = (int32_t)(key - U);
    }
}

// finish of a complete row: delta = eps * normalize(g) (the row is on the list k_amf_list makes of the same sorted keys)
struct AmfFgsm {
    el_amf_delta d;
    int64_t U, I;
    int F;
    float eps;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t key, int sub, int lpt, const float (&gg)[CPL][VW], float) const {
        const float rn = amf_row_rnorm<CPL, VW>(gg, lpt);
        const bool user = key < U;
        float* dst = user ? d.dGu + key * F : d.dGi + (key - U) * F;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = (sub + q * lpt) * VW;
            if (e < F) {
                float v[VW];
#pragma unroll
                for (int x = 0; x < VW; ++x) v[x] = gg[q][x] * rn * eps;
                stv<VW>(dst + e, v);
            }
        }
    }
};

struct AmfSeg {
    const u32 *keys, *vals;                   // [n] sorted
    const float *coefT, *coefP;               // coefP == nullptr: no adversarial term
    const int32_t *u, *i, *j;
    const float *Gu, *Gi, *Bi, *dGu, *dGi;    // dGu == nullptr: plain rows
    int64_t n, U;
    int F, chunk, lpt;
    float l_w, l_b, l_adv;
    float *part, *part_b;
};

template <int VW, int CPL, typename FIN>
__global__ __launch_bounds__(256) void k_amf_seg(AmfSeg p, FIN fin) {
    const int F = p.F, lpt = p.lpt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t grp = gid / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t p0 = grp * p.chunk;
    if (p0 >= p.n) return;
    const int64_t p1 = (p0 + p.chunk < p.n) ? p0 + p.chunk : p.n;
    int64_t cur = -1;
    bool started_inside = false;
    float acc[CPL][VW];
    float bacc = 0.f, beta = 0.f;
    int cnt = 0;
    auto flush = [&](bool ends_inside) {
        const float w = (float)cnt * p.l_w;
        float v[CPL][VW];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = (sub + q * lpt) * VW;
#pragma unroll
            for (int x = 0; x < VW; ++x) v[q][x] = acc[q][x];
            if (e < F && w != 0.f) {
                const bool user = cur < p.U;
                const int64_t off = (user ? cur : cur - p.U) * F + e;
                float r[VW];
                ldv<VW>((user ? p.Gu : p.Gi) + off, r);
                if (p.dGu) {
                    float dd[VW];
                    ldv<VW>((user ? p.dGu : p.dGi) + off, dd);
#pragma unroll
                    for (int x = 0; x < VW; ++x) r[x] += dd[x];
                }
#pragma unroll
                for (int x = 0; x < VW; ++x) v[q][x] = fmaf(w, r[x], v[q][x]);
            }
        }
        if (started_inside && ends_inside) {
            fin(cur, sub, lpt, v, bacc);
            return;
        }
        // a cut piece: slot 2 grp + 1 when the segment starts in this chunk (the head piece), 2 grp otherwise
        const int64_t slot = 2 * grp + (started_inside ? 1 : 0);
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = (sub + q * lpt) * VW;
            if (e < F) stv<VW>(p.part + slot * F + e, v[q]);
        }
        if (sub == 0) p.part_b[slot] = bacc;
    };
    // the index chain of a position (sorted key, triplet -> coefficients and the other rows' ids) is staged in LDS for AMF_STG
    // positions at once, so that only the row gathers stay on the walk's critical path (as k_pw_seg does)
    __shared__ u32 s_key[32][AMF_STG];
    __shared__ int32_t s_o1[32][AMF_STG], s_o2[32][AMF_STG];
    __shared__ float s_cT[32][AMF_STG], s_cP[32][AMF_STG], s_bw[32][AMF_STG];
    const int gl = (int)(threadIdx.x / lpt);
    for (int64_t sbase = p0; sbase < p1; sbase += AMF_STG) {
        const int cs = (int)((p1 - sbase < AMF_STG) ? p1 - sbase : AMF_STG);
        for (int t = sub; t < cs; t += lpt) {
            const u32 key = p.keys[sbase + t], v = p.vals[sbase + t];
            const int64_t b = (int64_t)(v & ~AMF_NEG);
            const bool user = key < (u32)p.U, neg = (v & AMF_NEG) != 0u;
            const float sg = neg ? 1.0f : -1.0f;               // d/dx of the loss is -s; x falls with the negative item's row
            s_key[gl][t] = key;
            s_cT[gl][t] = sg * p.coefT[b];
            s_cP[gl][t] = p.coefP ? sg * p.l_adv * p.coefP[b] : 0.f;
            s_o1[gl][t] = user ? p.i[b] : p.u[b];
            s_o2[gl][t] = user ? p.j[b] : -1;
            s_bw[gl][t] = user ? 0.f : (neg ? 0.1f : 1.0f);
        }
        el_wave_lds_sync();
        for (int t = 0; t < cs; ++t) {
            const int64_t key = (int64_t)s_key[gl][t], pos = sbase + t;
            const float cT = s_cT[gl][t], cP = s_cP[gl][t], bw = s_bw[gl][t];
            const int64_t o1 = s_o1[gl][t], o2 = s_o2[gl][t];
            const bool user = key < p.U;
            const float* tb = user ? p.Gi : p.Gu;               // the other side's tables
            const float* td = user ? p.dGi : p.dGu;
            float a1[CPL][VW], d1[CPL][VW], a2[CPL][VW], d2[CPL][VW];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int e = (sub + q * lpt) * VW;
#pragma unroll
                for (int x = 0; x < VW; ++x) a1[q][x] = d1[q][x] = a2[q][x] = d2[q][x] = 0.f;
                if (e < F) {
                    ldv<VW>(tb + o1 * F + e, a1[q]);
                    if (p.dGu) ldv<VW>(td + o1 * F + e, d1[q]);
                    if (o2 >= 0) {
                        ldv<VW>(tb + o2 * F + e, a2[q]);
                        if (p.dGu) ldv<VW>(td + o2 * F + e, d2[q]);
                    }
                }
            }
            if (key != cur) {
                if (cur >= 0) flush(true);
                cur = key;
                started_inside = (pos > p0) || (pos == 0) || ((int64_t)p.keys[pos - 1] != key);
                cnt = 0;
                bacc = 0.f;
                beta = user ? 0.f : p.Bi[key - p.U];
#pragma unroll
                for (int q = 0; q < CPL; ++q)
#pragma unroll
                    for (int x = 0; x < VW; ++x) acc[q][x] = 0.f;
            }
#pragma unroll
            for (int q = 0; q < CPL; ++q)
#pragma unroll
                for (int x = 0; x < VW; ++x) {
                    acc[q][x] = fmaf(cT, (a1[q][x] + d1[q][x]) - (a2[q][x] + d2[q][x]), acc[q][x]);
                    if (p.coefP) acc[q][x] = fmaf(cP, a1[q][x] - a2[q][x], acc[q][x]);
                }
            bacc += (cT + cP) + p.l_b * beta * bw;
            ++cnt;
        }
        el_wave_lds_sync();
    }
    flush(p1 == p.n || (int64_t)p.keys[p1] != cur);
}

// one lane group per sorted position; the first position of a row's segment owns the row:
// delta = clip(delta + eps_iter * normalize(g), -eps, eps), g from the accumulators, which come back zero (AMF_model.py:190-197)
struct AmfRows {
    const u32* keys;
    int64_t n, U, I;
    float *gGu, *gGi, *gBi;
    el_amf_delta d;
    int F, lpt;
    float eps, eps_iter;
};

template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_amf_msap_rows(AmfRows p) {
    const int F = p.F, lpt = p.lpt;
    const int64_t pos = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    if (pos >= p.n) return;
    const int64_t key = (int64_t)p.keys[pos];
    if (pos > 0 && (int64_t)p.keys[pos - 1] == key) return;
    const bool user = key < p.U;
    const int64_t off = (user ? key : key - p.U) * F;
    float* g = (user ? p.gGu : p.gGi) + off;
    float* dl = (user ? p.d.dGu : p.d.dGi) + off;
    float gg[CPL][VW];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
#pragma unroll
        for (int x = 0; x < VW; ++x) gg[q][x] = 0.f;
        if (e < F) ldv<VW>(g + e, gg[q]);
    }
    const float rn = amf_row_rnorm<CPL, VW>(gg, lpt);
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int e = (sub + q * lpt) * VW;
        if (e < F) {
            float v[VW], z[VW];
            ldv<VW>(dl + e, v);
#pragma unroll
            for (int x = 0; x < VW; ++x) {
                v[x] = fminf(fmaxf(v[x] + gg[q][x] * rn * p.eps_iter, -p.eps), p.eps);
                z[x] = 0.f;
            }
            stv<VW>(dl + e, v);
            stv<VW>(g + e, z);
        }
    }
    if (sub == 0 && !user) p.gBi[key - p.U] = 0.f;
}

// zero the listed delta rows (the counts are reset by the caller, behind this kernel)
template <int VW, int CPL>
__global__ __launch_bounds__(256) void k_amf_clear(el_amf_delta d, int64_t U, int64_t I, int F, int lpt) {
    const int64_t nu = d.counts[0] < U ? d.counts[0] : U, ni = d.counts[1] < I ? d.counts[1] : I;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    float z[VW];
#pragma unroll
    for (int x = 0; x < VW; ++x) z[x] = 0.f;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / lpt; t < nu + ni; t += groups) {
        float* dst = t < nu ? d.dGu + (int64_t)d.rows_u[t] * F : d.dGi + (int64_t)d.rows_i[t - nu] * F;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = (sub + q * lpt) * VW;
            if (e < F) stv<VW>(dst + e, z);
        }
    }
}

// out = a + b in fp32 (predict(adversarial=True) adds before it multiplies, AMF_model.py:110-111)
__global__ __launch_bounds__(256) void k_amf_add(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                 int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) out[e] = a[e] + b[e];
}

struct AmfWs {
    u32 *key_in, *val_in, *key, *val;
    float *coefT, *coefP;
    void* tmp;
    size_t tmp_bytes, total;
    float *part, *part_b;
    int32_t* split_long;
};

// positions per lane group of the segment pass over the 3 B sorted pairs
int amf_chunk(int64_t n) {
    const int64_t c = n / 32768;
    return (int)(c < 8 ? 8 : (c > 64 ? 64 : c));
}

int amf_carve(int64_t B, int64_t U, int64_t I, int F, void* base, AmfWs* w) {
    ElCarve c{(char*)base};
    const int64_t n = 3 * B;
    w->key_in = c.take<u32>((size_t)n);
    w->val_in = c.take<u32>((size_t)n);
    w->key = c.take<u32>((size_t)n);
    w->val = c.take<u32>((size_t)n);
    w->coefT = c.take<float>((size_t)B);
    w->coefP = c.take<float>((size_t)B);
    size_t t1 = 0;
    u32* np = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (unsigned)n, 0, el_bits_for(U + I), (hipStream_t)0) != hipSuccess) return 1;
    w->tmp_bytes = t1;
    w->tmp = c.take<char>(t1);
    const int ch = amf_chunk(n);
    const int64_t groups = (n + ch - 1) / ch + 1;
    w->part = c.take<float>((size_t)2 * groups * (size_t)(F > 0 ? F : 1));
    w->part_b = c.take<float>((size_t)2 * groups);
    w->split_long = c.take<int32_t>((size_t)(2 * groups + 4));
    w->total = c.off;
    return 0;
}

bool amf_vec4(const el_bprmf_state& st, const el_amf_delta& d) {
    auto ok = [&](const void* p) { return ((uintptr_t)p % 16) == 0; };
    return st.F % 4 == 0 && ok(st.Gu) && ok(st.Gi) && ok(st.gGu) && ok(st.gGi) && ok(d.dGu) && ok(d.dGi);
}

struct AmfCall {
    el_bprmf_state st;
    el_amf_delta d;
    const int32_t *u, *i, *j;
    int64_t B;
    float l_w, l_b;
    AmfWs w;
    bool vec;
    int lpt, cpl;
    hipStream_t s;
};

#define AMF_BY_CPL(cpl, CALL)        \
    do {                             \
        if ((cpl) == 1) CALL(1);     \
        else if ((cpl) == 2) CALL(2);\
        else if ((cpl) == 4) CALL(4);\
        else CALL(8);                \
    } while (0)

template <int VW>
int amf_fwd_vw(const AmfCall& c, bool use_delta, bool plain_too, float l_adv, bool emit, double* loss_out) {
    AmfFwd p = {c.st.Gu, c.st.Gi, c.st.Bi, use_delta ? c.d.dGu : nullptr, use_delta ? c.d.dGi : nullptr, c.u, c.i, c.j, c.w.coefT,
                plain_too ? c.w.coefP : nullptr, emit ? c.w.key_in : nullptr, emit ? c.w.val_in : nullptr, c.B, (u32)c.st.U, c.st.F, c.lpt,
                c.l_w, c.l_b, l_adv, loss_out};
    const int64_t want = (c.B * c.lpt + 255) / 256, cap = (int64_t)g_el_cur_ctx->cus * 16;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
#define AMF_FWD(CPL_) EL_LAUNCH("k_amf_fwd", (k_amf_fwd<VW, CPL_>), dim3(grid), dim3(256), 0, c.s, p)
    AMF_BY_CPL(c.cpl, AMF_FWD);
#undef AMF_FWD
    EL_CHECK_LAUNCH();
    return 0;
}
int amf_fwd(const AmfCall& c, bool use_delta, bool plain_too, float l_adv, bool emit, double* loss_out) {
    return c.vec ? amf_fwd_vw<4>(c, use_delta, plain_too, l_adv, emit, loss_out) : amf_fwd_vw<1>(c, use_delta, plain_too, l_adv, emit, loss_out);
}

int amf_sort(const AmfCall& c) {
    ElKernelTimer t("rocprim_radix_sort_pairs", c.s);
    size_t tb = c.w.tmp_bytes;
    EL_CHECK_HIP(rocprim::radix_sort_pairs(c.w.tmp, tb, c.w.key_in, c.w.key, c.w.val_in, c.w.val, (unsigned)(3 * c.B), 0,
                                           el_bits_for(c.st.U + c.st.I), c.s));
    return 0;
}

template <int VW, typename FIN>
int amf_seg_vw(const AmfCall& c, bool use_delta, const float* coefA, const float* coefB, float l_adv, FIN fin, const char* nm) {
    const int64_t n = 3 * c.B;
    AmfSeg p = {c.w.key, c.w.val, coefA, coefB, c.u, c.i, c.j, c.st.Gu, c.st.Gi, c.st.Bi, use_delta ? c.d.dGu : nullptr,
                use_delta ? c.d.dGi : nullptr, n, c.st.U, c.st.F, amf_chunk(n), c.lpt, c.l_w, c.l_b, l_adv, c.w.part, c.w.part_b};
    const int64_t groups = (n + p.chunk - 1) / p.chunk;
    const unsigned grid = (unsigned)((groups * c.lpt + 255) / 256);
    EL_CHECK_HIP(hipMemsetAsync(c.w.split_long, 0, 4, c.s));
    SegParts sp = {c.w.key, 0u, n, p.chunk, c.lpt, c.st.F, c.w.split_long, c.w.part, c.w.part_b};
    const unsigned gl = (unsigned)(groups < 1024 ? groups : 1024);
#define AMF_SEG(CPL_)                                                                                             \
    do {                                                                                                          \
        EL_LAUNCH(nm, (k_amf_seg<VW, CPL_, FIN>), dim3(grid), dim3(256), 0, c.s, p, fin);                         \
        EL_LAUNCH("k_seg_combine", (k_seg_combine<VW, CPL_, FIN>), dim3(grid), dim3(256), 0, c.s, sp, fin);       \
        EL_LAUNCH("k_seg_combine_long", (k_seg_combine_long<VW, CPL_, FIN>), dim3(gl), dim3(256), 0, c.s, sp, fin); \
    } while (0)
    AMF_BY_CPL(c.cpl, AMF_SEG);
#undef AMF_SEG
    EL_CHECK_LAUNCH();
    return 0;
}
template <typename FIN>
int amf_seg(const AmfCall& c, bool use_delta, const float* coefA, const float* coefB, float l_adv, FIN fin, const char* nm) {
    return c.vec ? amf_seg_vw<4, FIN>(c, use_delta, coefA, coefB, l_adv, fin, nm) : amf_seg_vw<1, FIN>(c, use_delta, coefA, coefB, l_adv, fin, nm);
}

int amf_clear(el_ctx* ctx, hipStream_t s, const el_amf_delta& d, int64_t U, int64_t I, int F, bool vec, int lpt, int cpl) {
    const unsigned grid = el_stream_grid(ctx, (U + I) * lpt);
#define AMF_CLR(CPL_)                                                                                        \
    do {                                                                                                     \
        if (vec) EL_LAUNCH("k_amf_clear", (k_amf_clear<4, CPL_>), dim3(grid), dim3(256), 0, s, d, U, I, F, lpt); \
        else EL_LAUNCH("k_amf_clear", (k_amf_clear<1, CPL_>), dim3(grid), dim3(256), 0, s, d, U, I, F, lpt);     \
    } while (0)
    AMF_BY_CPL(cpl, AMF_CLR);
#undef AMF_CLR
    EL_CHECK_LAUNCH();
    EL_CHECK_HIP(hipMemsetAsync(d.counts, 0, 2 * sizeof(int32_t), s));
    return 0;
}

// the batch's distinct rows become the list of delta rows (the counts are zero: amf_clear ran)
int amf_list(const AmfCall& c) {
    const int64_t n = 3 * c.B;
    EL_LAUNCH("k_amf_list", k_amf_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.s, c.w.key, n, c.st.U, c.st.I, c.d);
    EL_CHECK_LAUNCH();
    return 0;
}

int amf_msap_rows(const AmfCall& c, float eps, float eps_iter) {
    const int64_t n = 3 * c.B;
    AmfRows p = {c.w.key, n, c.st.U, c.st.I, c.st.gGu, c.st.gGi, c.st.gBi, c.d, c.st.F, c.lpt, eps, eps_iter};
    const unsigned grid = (unsigned)((n * c.lpt + 255) / 256);
#define AMF_ROWS(CPL_)                                                                                      \
    do {                                                                                                    \
        if (c.vec) EL_LAUNCH("k_amf_msap_rows", (k_amf_msap_rows<4, CPL_>), dim3(grid), dim3(256), 0, c.s, p);  \
        else EL_LAUNCH("k_amf_msap_rows", (k_amf_msap_rows<1, CPL_>), dim3(grid), dim3(256), 0, c.s, p);        \
    } while (0)
    AMF_BY_CPL(c.cpl, AMF_ROWS);
#undef AMF_ROWS
    EL_CHECK_LAUNCH();
    return 0;
}

int amf_check_delta(const el_bprmf_state* st, const el_amf_delta* d, const char* who) {
    EL_REQUIRE(st != nullptr && d != nullptr, "%s: null state", who);
    EL_REQUIRE(st->U > 0 && st->I > 0, "%s: bad shape U=%lld I=%lld", who, (long long)st->U, (long long)st->I);
    EL_REQUIRE(st->F >= 1 && st->F <= 512, "%s: F=%d out of range (1 .. 512)", who, st->F);
    EL_REQUIRE(st->U + st->I < (1LL << 32), "%s: U + I must fit a 32-bit sort key", who);
    EL_REQUIRE(d->dGu && d->dGi && d->rows_u && d->rows_i && d->counts, "%s: null perturbation tables or row lists", who);
    return 0;
}

// everything a pass over a batch needs, checked before anything launches
int amf_prepare(const el_bprmf_state* st, const el_amf_delta* d, const int32_t* u, const int32_t* i, const int32_t* j, int64_t B, float l_w,
                float l_b, void* ws, size_t ws_bytes, void* stream, const char* who, AmfCall* c) {
    if (int rc = amf_check_delta(st, d, who)) return rc;
    EL_REQUIRE(st->Gu && st->Gi && st->Bi, "%s: null tables", who);
    EL_REQUIRE(st->gGu && st->gGi && st->gBi, "%s: needs the dense accumulators gGu / gGi / gBi", who);
    EL_REQUIRE(st->Gu_last == nullptr && st->Gi_last == nullptr, "%s: rows must be current (no deferred decay, no fused item side)", who);
    EL_REQUIRE(u && i && j, "%s: null triplets", who);
    EL_REQUIRE(B >= 1 && B < (1LL << 30), "%s: batch size %lld out of range", who, (long long)B);
    c->st = *st, c->d = *d, c->u = u, c->i = i, c->j = j, c->B = B, c->l_w = l_w, c->l_b = l_b, c->s = (hipStream_t)stream;
    EL_REQUIRE(amf_carve(B, st->U, st->I, st->F, ws, &c->w) == 0, "%s: rocprim size query failed", who);
    EL_REQUIRE(ws != nullptr && ws_bytes >= c->w.total, "%s: workspace too small (%zu < %zu)", who, ws_bytes, c->w.total);
    c->vec = amf_vec4(*st, *d);
    c->lpt = el_pick_lpt(st->F, c->vec ? 4 : 1, &c->cpl);
    EL_REQUIRE(c->cpl <= 8, "%s: F=%d too large", who, st->F);
    return 0;
}

}  // namespace

extern "C" size_t el_amf_ws_bytes(int64_t B, int64_t U, int64_t I, int32_t F) {
    if (B < 1 || B >= (1LL << 30) || U < 1 || I < 1 || F < 1) return 0;
    AmfWs w;
    if (amf_carve(B, U, I, F, nullptr, &w)) return 0;
    return w.total;
}

extern "C" int el_amf_grads(el_ctx* ctx, void* stream, const el_bprmf_state* st, const el_amf_delta* d, const int32_t* u,
                            const int32_t* i, const int32_t* j, int64_t B, float l_w, float l_b, float l_adv, float eps, int flags,
                            double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    AmfCall c;
    EL_REQUIRE(loss_out != nullptr, "el_amf_grads: null loss_out");
    EL_REQUIRE((flags & ~EL_AMF_ADVERSARIAL) == 0, "el_amf_grads: unknown flags %d", flags);
    if (int rc = amf_prepare(st, d, u, i, j, B, l_w, l_b, ws, ws_bytes, stream, "el_amf_grads", &c)) return rc;
    const bool adv = (flags & EL_AMF_ADVERSARIAL) != 0;
    if (int rc = amf_fwd(c, true, adv, adv ? l_adv : 0.f, true, loss_out)) return rc;
    if (int rc = amf_sort(c)) return rc;
    AmfStore store = {c.st.gGu, c.st.gGi, c.st.gBi, c.st.U, c.st.F};
    if (int rc = amf_seg(c, true, c.w.coefT, adv ? c.w.coefP : nullptr, l_adv, store, "k_amf_seg")) return rc;
    if (!adv) return 0;
    // build_perturbation on the plain rows (AMF_model.py:91, :133-161): the old rows leave, the batch's rows come
    if (int rc = amf_clear(ctx, c.s, c.d, c.st.U, c.st.I, c.st.F, c.vec, c.lpt, c.cpl)) return rc;
    if (int rc = amf_list(c)) return rc;
    AmfFgsm fg = {c.d, c.st.U, c.st.I, c.st.F, eps};
    return amf_seg(c, false, c.w.coefP, nullptr, 0.f, fg, "k_amf_seg_fgsm");
}

extern "C" int el_amf_perturb(el_ctx* ctx, void* stream, const el_bprmf_state* st, const el_amf_delta* d, const int32_t* u,
                              const int32_t* i, const int32_t* j, int64_t B, float l_w, float l_b, float eps, float eps_iter,
                              int32_t nb_iter, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    AmfCall c;
    EL_REQUIRE(nb_iter >= 0, "el_amf_perturb: nb_iter must be >= 0");
    if (int rc = amf_prepare(st, d, u, i, j, B, l_w, l_b, ws, ws_bytes, stream, "el_amf_perturb", &c)) return rc;
    if (int rc = amf_clear(ctx, c.s, c.d, c.st.U, c.st.I, c.st.F, c.vec, c.lpt, c.cpl)) return rc;
    if (nb_iter == 0) {                                       // FGSM (AMF_model.py:133-161)
        if (int rc = amf_fwd(c, false, false, 0.f, true, nullptr)) return rc;
        if (int rc = amf_sort(c)) return rc;
        if (int rc = amf_list(c)) return rc;
        AmfFgsm fg = {c.d, c.st.U, c.st.I, c.st.F, eps};
        return amf_seg(c, false, c.w.coefT, nullptr, 0.f, fg, "k_amf_seg_fgsm");
    }
    AmfStore store = {c.st.gGu, c.st.gGi, c.st.gBi, c.st.U, c.st.F};
    for (int32_t it = 0; it < nb_iter; ++it) {                // MSAP (AMF_model.py:163-197)
        if (int rc = amf_fwd(c, true, false, 0.f, it == 0, nullptr)) return rc;
        if (it == 0) {
            if (int rc = amf_sort(c)) return rc;
            if (int rc = amf_list(c)) return rc;
        }
        if (int rc = amf_seg(c, true, c.w.coefT, nullptr, 0.f, store, "k_amf_seg")) return rc;
        if (int rc = amf_msap_rows(c, eps, eps_iter)) return rc;
    }
    return 0;
}

extern "C" int el_amf_delta_clear(el_ctx* ctx, void* stream, const el_bprmf_state* st, const el_amf_delta* d) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = amf_check_delta(st, d, "el_amf_delta_clear")) return rc;
    const bool vec = st->F % 4 == 0 && ((uintptr_t)d->dGu % 16) == 0 && ((uintptr_t)d->dGi % 16) == 0;
    int cpl = 1;
    const int lpt = el_pick_lpt(st->F, vec ? 4 : 1, &cpl);
    return amf_clear(ctx, (hipStream_t)stream, *d, st->U, st->I, st->F, vec, lpt, cpl);
}

extern "C" int el_amf_perturbed_tables(el_ctx* ctx, void* stream, const el_bprmf_state* st, const el_amf_delta* d, float* Gu_out,
                                       float* Gi_out) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = amf_check_delta(st, d, "el_amf_perturbed_tables")) return rc;
    EL_REQUIRE(st->Gu && st->Gi && Gu_out && Gi_out, "el_amf_perturbed_tables: null tables");
    EL_REQUIRE(st->Gu_last == nullptr && st->Gi_last == nullptr, "el_amf_perturbed_tables: rows must be current");
    const int64_t nu = st->U * (int64_t)st->F, ni = st->I * (int64_t)st->F;
    EL_LAUNCH("k_amf_add", k_amf_add, dim3(el_stream_grid(ctx, nu)), dim3(256), 0, (hipStream_t)stream, st->Gu, d->dGu, Gu_out, nu);
    EL_LAUNCH("k_amf_add", k_amf_add, dim3(el_stream_grid(ctx, ni)), dim3(256), 0, (hipStream_t)stream, st->Gi, d->dGi, Gi_out, ni);
    EL_CHECK_LAUNCH();
    return 0;
}
