// VBPR (visual BPR, He & McAuley 2016) -- contract in include/elliot_hip.h; reference:
// elliot/recommender/visual_recommenders/VBPR/VBPR_model.py.
//
//   x(u, i) = Bi[i] + Gu[u] . Gi[i] + Tu[u] . (f_i E) + f_i . Bp            f_i: row i of the feature matrix Feat [I, D]
//
// E and Bp are ONE variable here, EB = [E | Bp] [D, Fd + 1], so both products of a step carry the bias column along.  The feature
// matrix enters a step only through the batch's DISTINCT items (n of them, in ascending item order):
//   forward    PB [n, Fd + 1] = Feat_rows EB           (P and Feat_rows . Bp)
//   backward   gEB [D, Fd + 1] = Feat_rows^T AB + l_e EB,   AB [n, Fd + 1] = [A | a]: per distinct item the signed sums of g_b Tu[u_b], g_b
// No [B, D] array exists.  One gradient pass:
//   1. k_vbpr_keys      the (row, triplet) sort pairs -- users as u, items as U + i; a negative occurrence carries bit 31 of its value
//   2. ONE rocprim radix sort of the 3 B pairs (stable -> a row's occurrences are summed in batch order)
//   3. k_vbpr_heads + rocprim exclusive scan + k_vbpr_fill: an item segment's head gets its slot = the number of item segments in
//      front of it; rows[slot] = item, slot_of[item] = slot, n = their count.  The host reads n (4 bytes, one stream synchronise):
//      the two products are launched with that M / K.
//   4. k_vbpr_gather    Feat_rows [n, D] (skipped when the batch touches every item: the rows are Feat itself); el_gemm_f32 -> PB
//   5. k_vbpr_fwd       one lane group per triplet over the widened rows [Gu | Tu][u], [Gi | P][i], [Gi | P][j]: x, the loss, s = sigma(-x)
//                       (0 where the clip blocks the gradient)
//   6. k_vbpr_seg       one lane group per chunk of sorted positions walks its segments over rows of F + Fd + 1 floats: a user
//                       occurrence adds -s ([Gi | P][i] - [Gi | P][j]), an item occurrence -+s [Gu | Tu | 1][u]; the L2 term is
//                       count * l_w * (the row) at the end of the piece -- on [Gu | Tu] for a user, on Gi alone for an item (P is no
//                       variable).  Cut segments go through k_seg_combine / k_seg_combine_long (el_segcombine.h): no floating-point
//                       atomics on any row, the same bytes on every run.  A finished user row goes to gGu / gTu, a finished item
//                       row to gGi / gBi and, its last Fd + 1 floats, to AB[slot].
//   7. el_gemm_f32 -> gEB, k_vbpr_reg adds l_e EB (once per step) and the regulariser's loss.
// The optimiser is el_bprmf_apply on (Gu, Gi, Bi), k_adam_dense (el_bpr.hip, the same el_adam_elem: Keras' sparse apply, every
// row moves) on Tu, and k_adam_apply_dense (el_vae.hip: TensorFlow's fused dense ApplyAdam) on EB.  No Adam arithmetic lives here.
#include "el_common.h"
#include "el_segcombine.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

#define VB_NEG 0x80000000u
#define VB_STG 32

// the widened rows: element e of [Gu | Tu | 1][u] and of [Gi | P | 0][i] (s = the item's slot in PB); e < F + Fd + 1
struct VbTabs {
    const float *Gu, *Tu, *Gi, *Bi, *PB;
    const int32_t* slot;
    int F, Fd;
};
__device__ __forceinline__ float vb_user_elem(const VbTabs& t, int64_t u, int e) {
    return e < t.F ? t.Gu[u * t.F + e] : (e < t.F + t.Fd ? t.Tu[u * t.Fd + (e - t.F)] : 1.0f);
}
__device__ __forceinline__ float vb_item_elem(const VbTabs& t, int64_t i, int64_t s, int e) {
    return e < t.F ? t.Gi[i * t.F + e] : (e < t.F + t.Fd ? t.PB[s * (t.Fd + 1) + (e - t.F)] : 0.0f);
}

__global__ __launch_bounds__(256) void k_vbpr_keys(const int32_t* __restrict__ u, const int32_t* __restrict__ i,
                                                   const int32_t* __restrict__ j, int64_t B, u32 U, u32* __restrict__ key,
                                                   u32* __restrict__ val) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    key[b] = (u32)u[b], val[b] = (u32)b;
    key[B + b] = U + (u32)i[b], val[B + b] = (u32)b;
    key[2 * B + b] = U + (u32)j[b], val[2 * B + b] = (u32)b | VB_NEG;
}

// 1 at the first sorted position of every ITEM segment
__global__ __launch_bounds__(256) void k_vbpr_heads(const u32* __restrict__ keys, int64_t n, u32 U, int32_t* __restrict__ hd) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    hd[p] = (keys[p] >= U && (p == 0 || keys[p - 1] != keys[p])) ? 1 : 0;
}

// hs = the exclusive scan of hd: the slot of the item whose segment starts at p (items ascending); the last position closes the count
__global__ __launch_bounds__(256) void k_vbpr_fill(const u32* __restrict__ keys, const int32_t* __restrict__ hd,
                                                   const int32_t* __restrict__ hs, int64_t n, u32 U, int64_t I, int64_t n_max,
                                                   int32_t* __restrict__ rows, int32_t* __restrict__ slot_of, int32_t* __restrict__ n_out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int64_t item = (int64_t)(keys[p] - U);
    if (hd[p] && hs[p] < n_max && item < I) {                  // (an id past the catalogue writes nothing outside the map)
        rows[hs[p]] = (int32_t)item;
        slot_of[item] = hs[p];
    }
    if (p == n - 1) *n_out = hs[p] + hd[p];
}

template <int VW>
__global__ __launch_bounds__(256) void k_vbpr_gather(const float* __restrict__ Feat, const int32_t* __restrict__ rows, int64_t n,
                                                     int64_t D, float* __restrict__ out) {
    const int64_t per = D / VW, total = n * per, stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t s = t / per, d = (t - s * per) * VW;
        float v[VW];
        ldv<VW>(Feat + (int64_t)rows[s] * D + d, v);
        stv<VW>(out + s * D + d, v);
    }
}

struct VbFwd {
    VbTabs t;
    const int32_t *u, *i, *j;
    float* coef;       // [B] s
    int64_t B;
    int lpt;
    float l_w, l_b;
    double* loss_out;
};

template <int CPL>
__global__ __launch_bounds__(256) void k_vbpr_fwd(VbFwd p) {
    const int F = p.t.F, W = p.t.F + p.t.Fd, lpt = p.lpt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    double lossv = 0.0;
    for (int64_t b = gid / lpt; b < p.B; b += groups) {
        const int64_t u = p.u[b], i = p.i[b], j = p.j[b];
        const int64_t si = p.t.slot[i], sj = p.t.slot[j];
        float di = 0.f, dj = 0.f, sq = 0.f;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = sub + q * lpt;
            if (e < W) {
                const float a = vb_user_elem(p.t, u, e), ri = vb_item_elem(p.t, i, si, e), rj = vb_item_elem(p.t, j, sj, e);
                di = fmaf(a, ri, di);
                dj = fmaf(a, rj, dj);
                sq += a * a;                                   // l2_loss of gamma_u and theta_u ...
                if (e < F) sq += ri * ri + rj * rj;            // ... and of gamma_i, gamma_j (VBPR_model.py:81-84)
            }
        }
        di = el_group_sum(di, lpt);
        dj = el_group_sum(dj, lpt);
        sq = el_group_sum(sq, lpt);
        if (sub == 0) {
            const float bi = p.t.Bi[i], bj = p.t.Bi[j];
            const float pi = p.t.PB[si * (p.t.Fd + 1) + p.t.Fd], pj = p.t.PB[sj * (p.t.Fd + 1) + p.t.Fd];
            const float x = ((bi + di) + pi) - ((bj + dj) + pj);
            const float c = fminf(fmaxf(x, -80.0f), 1e8f);
            p.coef[b] = (x >= -80.0f && x <= 1e8f) ? 1.0f / (1.0f + expf(c)) : 0.f;
            // (the terms of one triplet are added in double: a clipped triplet's 80 would otherwise round the small ones away)
            lossv += (double)el_softplus_tf(-c) + (double)(p.l_w * 0.5f * sq) + (double)(p.l_b * 0.5f * bi * bi) +
                     (double)(p.l_b * 0.5f * bj * bj / 10.0f);
        }
    }
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

// finish of a complete row (key < U: user row `key`, else item row key - U)
struct VbStore {
    float *gGu, *gTu, *gGi, *gBi, *AB;
    const int32_t* slot;
    int64_t U;
    int F, Fd;
    template <int CPL, int VW>
    __device__ __forceinline__ void operator()(int64_t key, int sub, int lpt, const float (&gg)[CPL][VW], float b) const {
        const bool user = key < U;
        const int64_t r = user ? key : key - U;
        const int64_t s = user ? 0 : (int64_t)slot[r];
        const int W = F + Fd;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = sub + q * lpt;
            if (e < F) {
                (user ? gGu : gGi)[r * F + e] = gg[q][0];
            } else if (e < W) {
                if (user) gTu[r * Fd + (e - F)] = gg[q][0];
                else AB[s * (Fd + 1) + (e - F)] = gg[q][0];
            } else if (e == W && !user) {
                AB[s * (Fd + 1) + Fd] = gg[q][0];
            }
        }
        if (sub == 0 && !user) gBi[r] = b;
    }
};

struct VbSeg {
    VbTabs t;
    const u32 *keys, *vals;   // [n] sorted
    const float* coef;
    const int32_t *u, *i, *j;
    int64_t n, U;
    int chunk, lpt;
    float l_w, l_b;
    float *part, *part_b;
};

template <int CPL>
__global__ __launch_bounds__(256) void k_vbpr_seg(VbSeg p, VbStore fin) {
    const int F = p.t.F, W = p.t.F + p.t.Fd, W1 = W + 1, lpt = p.lpt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t grp = gid / lpt;
    const int sub = (int)(threadIdx.x & (lpt - 1));
    const int64_t p0 = grp * p.chunk;
    if (p0 >= p.n) return;
    const int64_t p1 = (p0 + p.chunk < p.n) ? p0 + p.chunk : p.n;
    int64_t cur = -1;
    bool started_inside = false;
    float acc[CPL][1];
    float bacc = 0.f, beta = 0.f;
    int cnt = 0;
    auto flush = [&](bool ends_inside) {
        const float w = (float)cnt * p.l_w;
        const bool user = cur < p.U;
        const int64_t r = user ? cur : cur - p.U;
        float v[CPL][1];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = sub + q * lpt;
            v[q][0] = acc[q][0];
            if (w != 0.f && e < (user ? W : F)) v[q][0] = fmaf(w, user ? vb_user_elem(p.t, r, e) : p.t.Gi[r * F + e], v[q][0]);
        }
        if (started_inside && ends_inside) {
            fin(cur, sub, lpt, v, bacc);
            return;
        }
        // a cut piece: slot 2 grp + 1 when the segment starts in this chunk (the head piece), 2 grp otherwise
        const int64_t slot = 2 * grp + (started_inside ? 1 : 0);
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int e = sub + q * lpt;
            if (e < W1) p.part[slot * W1 + e] = v[q][0];
        }
        if (sub == 0) p.part_b[slot] = bacc;
    };
    // the index chain of a position is staged in LDS for VB_STG positions at once (as k_amf_seg does)
    __shared__ u32 s_key[32][VB_STG];
    __shared__ int32_t s_o1[32][VB_STG], s_o2[32][VB_STG], s_s1[32][VB_STG], s_s2[32][VB_STG];
    __shared__ float s_c[32][VB_STG], s_bw[32][VB_STG];
    const int gl = (int)(threadIdx.x / lpt);
    for (int64_t sbase = p0; sbase < p1; sbase += VB_STG) {
        const int cs = (int)((p1 - sbase < VB_STG) ? p1 - sbase : VB_STG);
        for (int t = sub; t < cs; t += lpt) {
            const u32 key = p.keys[sbase + t], v = p.vals[sbase + t];
            const int64_t b = (int64_t)(v & ~VB_NEG);
            const bool user = key < (u32)p.U, neg = (v & VB_NEG) != 0u;
            s_key[gl][t] = key;
            s_c[gl][t] = (neg ? 1.0f : -1.0f) * p.coef[b];     // d/dx of the loss is -s; x falls with the negative item's row
            const int32_t o1 = user ? p.i[b] : p.u[b], o2 = user ? p.j[b] : -1;
            s_o1[gl][t] = o1, s_o2[gl][t] = o2;
            s_s1[gl][t] = user ? p.t.slot[o1] : 0;
            s_s2[gl][t] = user ? p.t.slot[o2] : 0;
            s_bw[gl][t] = user ? 0.f : (neg ? 0.1f : 1.0f);
        }
        el_wave_lds_sync();
        for (int t = 0; t < cs; ++t) {
            const int64_t key = (int64_t)s_key[gl][t], pos = sbase + t;
            const float c = s_c[gl][t], bw = s_bw[gl][t];
            const int64_t o1 = s_o1[gl][t], o2 = s_o2[gl][t], s1 = s_s1[gl][t], s2 = s_s2[gl][t];
            const bool user = key < p.U;
            float d[CPL];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int e = sub + q * lpt;
                d[q] = 0.f;
                if (e < W1) d[q] = user ? vb_item_elem(p.t, o1, s1, e) - vb_item_elem(p.t, o2, s2, e) : vb_user_elem(p.t, o1, e);
            }
            if (key != cur) {
                if (cur >= 0) flush(true);
                cur = key;
                started_inside = (pos > p0) || (pos == 0) || ((int64_t)p.keys[pos - 1] != key);
                cnt = 0;
                bacc = 0.f;
                beta = user ? 0.f : p.t.Bi[key - p.U];
#pragma unroll
                for (int q = 0; q < CPL; ++q) acc[q][0] = 0.f;
            }
#pragma unroll
            for (int q = 0; q < CPL; ++q) acc[q][0] = fmaf(c, d[q], acc[q][0]);
            bacc += c + p.l_b * beta * bw;
            ++cnt;
        }
        el_wave_lds_sync();
    }
    flush(p1 == p.n || (int64_t)p.keys[p1] != cur);
}

// gEB += l_e EB (the regulariser of E and Bp enters once per step), loss += l_e / 2 * sum EB^2
__global__ __launch_bounds__(256) void k_vbpr_reg(const float* __restrict__ EB, float* __restrict__ gEB, int64_t n, float l_e,
                                                  double* loss_out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    double sq = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const float th = EB[e];
        gEB[e] = gEB[e] + l_e * th;
        sq += (double)(th * th);
    }
    __shared__ double part[4];
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) part[wv] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = (part[0] + part[1]) + (part[2] + part[3]);
        if (t != 0.0) atomicAdd(loss_out, (double)(l_e * 0.5f) * t);
    }
}

// Q [I, F + Fd] = [Gi | T[:, :Fd]], bq = Bi + T[:, Fd]   (T [I, Fd + 1] = Feat EB)
__global__ __launch_bounds__(256) void k_vbpr_image(const float* __restrict__ Gi, const float* __restrict__ Bi,
                                                    const float* __restrict__ T, int64_t I, int F, int Fd, float* __restrict__ Q,
                                                    float* __restrict__ bq) {
    const int W = F + Fd;
    const int64_t total = I * W, stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t r = t / W;
        const int e = (int)(t - r * W);
        Q[t] = e < F ? Gi[r * F + e] : T[r * (Fd + 1) + (e - F)];
        if (e == 0) bq[r] = Bi[r] + T[r * (Fd + 1) + Fd];
    }
}

// P [U, F + Fd] = [Gu | Tu]
__global__ __launch_bounds__(256) void k_vbpr_users(const float* __restrict__ Gu, const float* __restrict__ Tu, int64_t U, int F,
                                                    int Fd, float* __restrict__ P) {
    const int W = F + Fd;
    const int64_t total = U * W, stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t r = t / W;
        const int e = (int)(t - r * W);
        P[t] = e < F ? Gu[r * F + e] : Tu[r * Fd + (e - F)];
    }
}

struct VbWs {
    u32 *key_in, *val_in, *key, *val;
    float* coef;
    int32_t *hd, *hs, *rows, *slot_of, *n_dev;
    float *Fr, *PB, *AB;
    void *sort_tmp, *scan_tmp, *gemm_ws;
    size_t sort_bytes, scan_bytes, gemm_bytes, total;
    float *part, *part_b;
    int32_t* split_long;
    int64_t n_max;
};

// positions per lane group of the segment pass over the 3 B sorted pairs
int vb_chunk(int64_t n) {
    const int64_t c = n / 32768;
    return (int)(c < 8 ? 8 : (c > 64 ? 64 : c));
}

size_t vb_max(size_t a, size_t b) { return a > b ? a : b; }

int vb_carve(el_ctx* ctx, int64_t B, int64_t U, int64_t I, int F, int Fd, int64_t D, void* base, VbWs* w) {
    ElCarve c{(char*)base};
    const int64_t n = 3 * B, N = Fd + 1, W1 = F + Fd + 1;
    const int64_t n_max = 2 * B < I ? 2 * B : I;
    w->n_max = n_max;
    w->key_in = c.take<u32>((size_t)n);
    w->val_in = c.take<u32>((size_t)n);
    w->key = c.take<u32>((size_t)n);
    w->val = c.take<u32>((size_t)n);
    w->coef = c.take<float>((size_t)B);
    w->hd = c.take<int32_t>((size_t)n);
    w->hs = c.take<int32_t>((size_t)n);
    w->rows = c.take<int32_t>((size_t)n_max);
    w->slot_of = c.take<int32_t>((size_t)I);
    w->n_dev = c.take<int32_t>(1);
    w->Fr = c.take<float>((size_t)n_max * (size_t)D);
    w->PB = c.take<float>((size_t)n_max * (size_t)N);
    w->AB = c.take<float>((size_t)n_max * (size_t)N);
    size_t t1 = 0, t2 = 0;
    u32* np = nullptr;
    int32_t* ip = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (unsigned)n, 0, el_bits_for(U + I), (hipStream_t)0) != hipSuccess) return 1;
    if (rocprim::exclusive_scan(nullptr, t2, ip, ip, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), (hipStream_t)0) != hipSuccess) return 1;
    w->sort_bytes = t1, w->scan_bytes = t2;
    w->sort_tmp = c.take<char>(t1);
    w->scan_tmp = c.take<char>(t2);
    w->gemm_bytes = vb_max(el_gemm_ws_bytes(ctx, n_max, N, D), el_gemm_ws_bytes(ctx, D, N, n_max));
    w->gemm_ws = c.take<char>(w->gemm_bytes);
    const int ch = vb_chunk(n);
    const int64_t groups = (n + ch - 1) / ch + 1;
    w->part = c.take<float>((size_t)2 * groups * (size_t)W1);
    w->part_b = c.take<float>((size_t)2 * groups);
    w->split_long = c.take<int32_t>((size_t)(2 * groups + 4));
    w->total = c.off;
    return 0;
}

int vb_check_state(const el_vbpr_state* st, const char* who) {
    EL_REQUIRE(st != nullptr, "%s: null state", who);
    const el_bprmf_state& mf = st->mf;
    EL_REQUIRE(mf.U > 0 && mf.I > 0, "%s: bad shape U=%lld I=%lld", who, (long long)mf.U, (long long)mf.I);
    EL_REQUIRE(mf.F >= 1 && st->Fd >= 1 && mf.F + st->Fd + 1 <= 512, "%s: F=%d Fd=%d out of range (F, Fd >= 1, F + Fd <= 511)", who, mf.F,
               st->Fd);
    EL_REQUIRE(st->D >= 1, "%s: D=%lld out of range", who, (long long)st->D);
    EL_REQUIRE(mf.U + mf.I < (1LL << 31), "%s: U + I must fit a 31-bit sort key", who);
    EL_REQUIRE(mf.Gu && mf.Gi && mf.Bi && st->Tu && st->EB && st->Feat, "%s: null tables", who);
    EL_REQUIRE(mf.Gu_last == nullptr && mf.Gi_last == nullptr && mf.uslot == nullptr, "%s: rows must be current and the accumulators dense",
               who);
    return 0;
}

#define VB_BY_CPL(cpl, CALL)         \
    do {                             \
        if ((cpl) == 1) CALL(1);     \
        else if ((cpl) == 2) CALL(2);\
        else if ((cpl) == 4) CALL(4);\
        else CALL(8);                \
    } while (0)

bool vb_al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" size_t el_vbpr_ws_bytes(el_ctx* ctx, int64_t B, int64_t U, int64_t I, int32_t F, int32_t Fd, int64_t D) {
    if (!ctx || B < 1 || B >= (1LL << 30) || U < 1 || I < 1 || F < 1 || Fd < 1 || D < 1) return 0;
    VbWs w;
    if (vb_carve(ctx, B, U, I, F, Fd, D, nullptr, &w)) return 0;
    return w.total;
}

extern "C" int el_vbpr_grads(el_ctx* ctx, void* stream, const el_vbpr_state* st, const int32_t* u, const int32_t* i, const int32_t* j,
                             int64_t B, float l_w, float l_b, float l_e, double* loss_out, int64_t* n_items_out, void* ws,
                             size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = vb_check_state(st, "el_vbpr_grads")) return rc;
    const el_bprmf_state& mf = st->mf;
    EL_REQUIRE(mf.gGu && mf.gGi && mf.gBi && st->gTu && st->gEB, "el_vbpr_grads: needs the dense accumulators gGu / gGi / gBi / gTu / gEB");
    EL_REQUIRE(u && i && j, "el_vbpr_grads: null triplets");
    EL_REQUIRE(loss_out != nullptr, "el_vbpr_grads: null loss_out");
    EL_REQUIRE(B >= 1 && B < (1LL << 30), "el_vbpr_grads: batch size %lld out of range", (long long)B);
    VbWs w;
    const int F = mf.F, Fd = st->Fd;
    const int64_t U = mf.U, I = mf.I, D = st->D, N = Fd + 1, n = 3 * B;
    EL_REQUIRE(vb_carve(ctx, B, U, I, F, Fd, D, ws, &w) == 0, "el_vbpr_grads: rocprim size query failed");
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "el_vbpr_grads: workspace too small (%zu < %zu)", ws_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    int cpl = 1;
    const int lpt = el_pick_lpt(F + Fd + 1, 1, &cpl);

    // 1-3: the sorted (row, triplet) pairs and the batch's distinct items
    const unsigned gb = (unsigned)((B + 255) / 256), gn = (unsigned)((n + 255) / 256);
    EL_LAUNCH("k_vbpr_keys", k_vbpr_keys, dim3(gb), dim3(256), 0, s, u, i, j, B, (u32)U, w.key_in, w.val_in);
    {
        ElKernelTimer t("rocprim_radix_sort_pairs", s);
        size_t tb = w.sort_bytes;
        EL_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tb, w.key_in, w.key, w.val_in, w.val, (unsigned)n, 0, el_bits_for(U + I), s));
    }
    EL_LAUNCH("k_vbpr_heads", k_vbpr_heads, dim3(gn), dim3(256), 0, s, w.key, n, (u32)U, w.hd);
    {
        ElKernelTimer t("rocprim_exclusive_scan", s);
        size_t tb = w.scan_bytes;
        EL_CHECK_HIP(rocprim::exclusive_scan(w.scan_tmp, tb, w.hd, w.hs, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), s));
    }
    EL_LAUNCH("k_vbpr_fill", k_vbpr_fill, dim3(gn), dim3(256), 0, s, w.key, w.hd, w.hs, n, (u32)U, I, w.n_max, w.rows, w.slot_of, w.n_dev);
    EL_CHECK_LAUNCH();
    int32_t n_items = 0;
    EL_CHECK_HIP(hipMemcpyAsync(&n_items, w.n_dev, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EL_CHECK_HIP(hipStreamSynchronize(s));
    EL_REQUIRE(n_items >= 1 && n_items <= w.n_max, "el_vbpr_grads: %d distinct items for a batch of %lld over %lld items (item id out of range?)",
               n_items, (long long)B, (long long)I);
    if (n_items_out) *n_items_out = n_items;

    // 4: Feat_rows and PB = Feat_rows EB
    const float* Fr = st->Feat;
    if (n_items < I) {                                         // (all I items: rows[s] = s, the rows are Feat itself)
        const bool v4 = D % 4 == 0 && vb_al16(st->Feat) && vb_al16(w.Fr);
        const unsigned gg = el_stream_grid(ctx, (int64_t)n_items * (v4 ? D / 4 : D));
        if (v4) EL_LAUNCH("k_vbpr_gather", k_vbpr_gather<4>, dim3(gg), dim3(256), 0, s, st->Feat, w.rows, (int64_t)n_items, D, w.Fr);
        else EL_LAUNCH("k_vbpr_gather", k_vbpr_gather<1>, dim3(gg), dim3(256), 0, s, st->Feat, w.rows, (int64_t)n_items, D, w.Fr);
        EL_CHECK_LAUNCH();
        Fr = w.Fr;
    }
    if (int rc = el_gemm_f32(ctx, stream, 0, 0, n_items, N, D, Fr, D, st->EB, N, w.PB, N, nullptr, 0, w.gemm_ws, w.gemm_bytes)) return rc;

    // 5-6: scores, then the ordered row sums
    VbTabs tabs = {mf.Gu, st->Tu, mf.Gi, mf.Bi, w.PB, w.slot_of, F, Fd};
    {
        VbFwd p = {tabs, u, i, j, w.coef, B, lpt, l_w, l_b, loss_out};
        const int64_t want = (B * lpt + 255) / 256, cap = (int64_t)ctx->cus * 16;
        const unsigned grid = (unsigned)(want < cap ? want : cap);
#define VB_FWD(CPL_) EL_LAUNCH("k_vbpr_fwd", (k_vbpr_fwd<CPL_>), dim3(grid), dim3(256), 0, s, p)
        VB_BY_CPL(cpl, VB_FWD);
#undef VB_FWD
        EL_CHECK_LAUNCH();
    }
    {
        VbSeg p = {tabs, w.key, w.val, w.coef, u, i, j, n, U, vb_chunk(n), lpt, l_w, l_b, w.part, w.part_b};
        VbStore fin = {mf.gGu, st->gTu, mf.gGi, mf.gBi, w.AB, w.slot_of, U, F, Fd};
        const int64_t groups = (n + p.chunk - 1) / p.chunk;
        const unsigned grid = (unsigned)((groups * lpt + 255) / 256);
        EL_CHECK_HIP(hipMemsetAsync(w.split_long, 0, 4, s));
        SegParts sp = {w.key, 0u, n, p.chunk, lpt, F + Fd + 1, w.split_long, w.part, w.part_b};
        const unsigned gl = (unsigned)(groups < 1024 ? groups : 1024);
#define VB_SEG(CPL_)                                                                                                  \
    do {                                                                                                              \
        EL_LAUNCH("k_vbpr_seg", (k_vbpr_seg<CPL_>), dim3(grid), dim3(256), 0, s, p, fin);                             \
        EL_LAUNCH("k_seg_combine", (k_seg_combine<1, CPL_, VbStore>), dim3(grid), dim3(256), 0, s, sp, fin);          \
        EL_LAUNCH("k_seg_combine_long", (k_seg_combine_long<1, CPL_, VbStore>), dim3(gl), dim3(256), 0, s, sp, fin);  \
    } while (0)
        VB_BY_CPL(cpl, VB_SEG);
#undef VB_SEG
        EL_CHECK_LAUNCH();
    }

    // 7: gEB = Feat_rows^T AB + l_e EB
    if (int rc = el_gemm_f32(ctx, stream, 1, 0, D, N, n_items, Fr, D, w.AB, N, st->gEB, N, nullptr, 0, w.gemm_ws, w.gemm_bytes)) return rc;
    EL_LAUNCH("k_vbpr_reg", k_vbpr_reg, dim3(el_stream_grid(ctx, D * N)), dim3(256), 0, s, st->EB, st->gEB, D * N, l_e, loss_out);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_vbpr_apply(el_ctx* ctx, void* stream, const el_vbpr_state* st, float lr, int32_t step, float lr_t) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = vb_check_state(st, "el_vbpr_apply")) return rc;
    EL_REQUIRE(st->gTu && st->mTu && st->vTu && st->gEB && st->mEB && st->vEB, "el_vbpr_apply: accumulators or Adam slots of Tu / EB missing");
    if (int rc = el_bprmf_apply(ctx, stream, &st->mf, lr, EL_OPT_ADAM_TF_DENSE, step, lr_t)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nt = st->mf.U * (int64_t)st->Fd, ne = st->D * (int64_t)(st->Fd + 1);
    EL_LAUNCH("k_adam_dense_Tu", k_adam_dense, dim3(el_stream_grid(ctx, nt / 4 + 1)), dim3(256), 0, s, st->Tu, st->gTu, st->mTu, st->vTu, nt,
              lr_t, 0.9f, 0.999f, 1e-7f);
    // (E and Bp reach the optimiser as dense gradients: TensorFlow's fused ApplyAdam, the kernel of the Mult-VAE weights)
    EL_LAUNCH("k_adam_apply_dense_EB", k_adam_apply_dense, dim3(el_stream_grid(ctx, ne)), dim3(256), 0, s, st->EB, st->gEB, st->mEB, st->vEB,
              ne, lr_t, 0.9f, 0.999f, 1e-7f, 1);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t el_vbpr_image_ws_bytes(el_ctx* ctx, int64_t I, int32_t Fd, int64_t D) {
    if (!ctx || I < 1 || Fd < 1 || D < 1) return 0;
    return el_align256((size_t)I * (size_t)(Fd + 1) * 4) + el_gemm_ws_bytes(ctx, I, Fd + 1, D);
}

extern "C" int el_vbpr_item_image(el_ctx* ctx, void* stream, const el_vbpr_state* st, float* Q, float* bq, float* P, void* ws,
                                  size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = vb_check_state(st, "el_vbpr_item_image")) return rc;
    EL_REQUIRE(Q && bq, "el_vbpr_item_image: null output");
    const el_bprmf_state& mf = st->mf;
    const int64_t N = st->Fd + 1;
    const size_t tb = el_align256((size_t)mf.I * (size_t)N * 4), gbytes = el_gemm_ws_bytes(ctx, mf.I, N, st->D);
    EL_REQUIRE(ws != nullptr && ws_bytes >= tb + gbytes, "el_vbpr_item_image: workspace too small (%zu < %zu)", ws_bytes, tb + gbytes);
    float* T = (float*)ws;
    if (int rc = el_gemm_f32(ctx, stream, 0, 0, mf.I, N, st->D, st->Feat, st->D, st->EB, N, T, N, nullptr, 0, (char*)ws + tb, gbytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int W = mf.F + st->Fd;
    EL_LAUNCH("k_vbpr_image", k_vbpr_image, dim3(el_stream_grid(ctx, mf.I * W)), dim3(256), 0, s, mf.Gi, mf.Bi, T, mf.I, mf.F, st->Fd, Q, bq);
    if (P) EL_LAUNCH("k_vbpr_users", k_vbpr_users, dim3(el_stream_grid(ctx, mf.U * W)), dim3(256), 0, s, mf.Gu, st->Tu, mf.U, mf.F, st->Fd, P);
    EL_CHECK_LAUNCH();
    return 0;
}
