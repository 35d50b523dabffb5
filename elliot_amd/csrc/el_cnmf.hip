// ConvNeuMF (outer-product neural CF, He et al. 2018) -- contract in include/elliot_hip.h, DESIGN 3.33;
// reference: elliot/recommender/neural/ConvNeuMF/convolutional_neural_matrix_factorization_model.py.
//
// A pair (u, i) is the F x F map E[a, b] = p_u[a] q_i[b] pushed through L Conv2D + ReLU layers with k == s (disjoint patches), sum-pooled
// and sent through two linear Dense layers.  One workgroup (4 waves) serves one pair at a time and a contiguous range of pairs in all:
//   layer 1     never stored.  E has rank one, so  T_i[x, a, c] = sum_b W1[a, b, c] q_i[k x + b]  (per item; el_cnmf_item_image for
//               scoring) and  A_1[y, x, c] = relu(b1[c] + sum_a p_u[k y + a] T_i[x, a, c]):  k fma and a max where it is needed.
//   layer l>=2  the patch GEMM  [H_l^2 pixels] x [k^2 C_(l-1)] x [C_l]  on v_mfma_f32_32x32x2_f32 (cn_gemm): a wave owns 32 x 32 output
//               tiles, lane (col, hi) MAKES its A element (row col, k index hi) -- for l == 2 from p_u and T_i, so A_1 only ever exists
//               as fragment registers -- and reads its B element from W_l (W_2 staged in LDS once per workgroup where it fits).
//               Bias + ReLU on the accumulators; the last layer is pooled there: per lane in tile order, lane halves, then waves in order.
//   backward    recomputed, not stored: the forward is run again keeping A_2 .. A_L in the workgroup's workspace, dZ_l overwrites A_l,
//               dW_l = patches^T dZ_l (a row of ones appended gives db_l) and dA_(l-1) = dZ_l W_l^T are two more cn_gemm calls whose
//               epilogues add to the workgroup's gradient slot / mask and store to disjoint elements of the layer below.  Layer 1:
//               dZ_1 is masked by the recomputed z_1 and reduced to dW1, db1, dp, dq in fixed orders on the vector ALU.
// No floating-point atomics: a workgroup owns its slot (the same lane adds to the same element pair after pair), k_cnmf_finish adds the
// slots in workgroup order, and the per-pair dp / dq rows are added per distinct user / item in sorted order (stable radix sort).
#include "el_common.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

typedef float cn_f16 __attribute__((ext_vector_type(16)));

#define CN_MAXL 6
#define CN_W2_LDS 8192                    // floats of LDS for the staged W_2
#define CN_WG_BYTES (512ll << 20)         // the per-workgroup workspaces and slots of one call stay under this together

struct CnP {
    int L, F;
    int C[CN_MAXL + 1], k[CN_MAXL + 1], H[CN_MAXL + 1], Hc[CN_MAXL + 1];   // Hc[l]: side of the part of map l the layer above reads
    const float *P, *Q;
    const float *W[CN_MAXL + 1], *b[CN_MAXL + 1];                          // 1 .. L
    const float* D[4];                                                     // Wd1 [C, C], bd1 [C], Wd2 [C], bd2 [1]
    float rate;
    u64 seed;
    u32 step;
    float* wsf;                                                            // per-workgroup workspace
    int64_t ws_stride;
    int64_t oT, oS, oG, oD0, oZ1, oA[CN_MAXL + 1];
    double* slots;                                                         // per-workgroup gradient partials, in double
    int64_t slot_stride;
    int64_t oW[CN_MAXL + 1], ob[CN_MAXL + 1], oD[4];
};

struct CnLds {                                // the head is carried in double: a pair leaves ONE rounding behind, that of its score
    float *p, *q, *k0, *k1, *dz;
    double *pool, *z, *zd, *h, *hd, *dh, *x;
};

// Keras Dropout: the factor of unit `unit` of head layer `layer` (0: the pooled vector, 1: the first Dense output) of sample `sample`
// in call `call` (0: positive, 1: negative) of step `step`
__device__ __forceinline__ float cn_keep(float rate, u64 seed, u32 step, u32 call, u32 sample, u32 layer, u32 unit) {
    if (!(rate > 0.f)) return 1.f;
    const el_philox4 r = el_philox4x32_10(sample, unit >> 2, step, call * 2u + layer, (u32)seed, (u32)(seed >> 32));
    const u32 rv[4] = {r.x, r.y, r.z, r.w};
    const float uni = (float)(rv[unit & 3u] >> 8) * (1.0f / 16777216.0f);
    return uni < rate ? 0.f : 1.0f / (1.0f - rate);
}

// pre-activation of layer 1 at (Y, X, c)
__device__ __forceinline__ float cn_z1(const CnP& g, const float* sp, const float* T, int Y, int X, int c) {
    const int k = g.k[1], C1 = g.C[1];
    float z = g.b[1][c];
    const float* t = T + (int64_t)X * k * C1 + c;
    for (int a = 0; a < k; ++a) z = fmaf(sp[k * Y + a], t[a * C1], z);
    return z;
}

// the input of layer l >= 2: element (Y, X, ci) of A_(l-1)
struct CnIn {
    const CnP* g;
    const float *sp, *T, *act;
    int l;
    __device__ __forceinline__ float operator()(int Y, int X, int ci) const {
        if (l == 2) {
            const float z = cn_z1(*g, sp, T, Y, X, ci);
            return z > 0.f ? z : 0.f;
        }
        return act[((int64_t)Y * g->H[l - 1] + X) * g->C[l - 1] + ci];
    }
};
// where patch index kk of output pixel pix of layer l lies in the map below
__device__ __forceinline__ void cn_patch_at(const CnP& g, int l, int pix, int kk, int& Y, int& X, int& ci) {
    const int Hl = g.H[l], Cp = g.C[l - 1], k = g.k[l];
    const int y = pix / Hl, x = pix - y * Hl, pos = kk / Cp, dy = pos / k;
    ci = kk - pos * Cp;
    Y = y * k + dy;
    X = x * k + (pos - dy * k);
}
__device__ __forceinline__ float cn_patch(const CnIn& in, int pix, int kk) {
    int Y, X, ci;
    cn_patch_at(*in.g, in.l, pix, kk, Y, X, ci);
    return in(Y, X, ci);
}

// C[M, N] = sum_k A(m, k) B(k, n) by the workgroup's 4 waves: wave w owns the 32 x 32 tiles w, w + 4, ... (row-major over the tiles),
// lane (col = lane % 32, hi = lane / 32) supplies A(m0 + col, k0 + hi) and B(k0 + hi, n0 + col) of every k pair and receives rows
// (r % 4) + 8 (r / 4) + 4 hi of column col.  Rows, columns and k past the edge are zeros in the fragment, not padding in memory.
template <class AF, class BF, class EP>
__device__ __forceinline__ void cn_gemm(int M, int N, int K, AF af, BF bf, EP ep) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5, col = lane & 31;
    const int nt = (N + 31) >> 5, tiles = ((M + 31) >> 5) * nt;
    for (int t = wave; t < tiles; t += 4) {
        const int m0 = (t / nt) << 5, n0 = (t % nt) << 5, m = m0 + col, n = n0 + col;
        cn_f16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < K; k0 += 2) {
            const int k = k0 + hi;
            const float a = (m < M && k < K) ? af(m, k) : 0.f;
            const float b = (n < N && k < K) ? bf(k, n) : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        if (n < N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mm = m0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (mm < M) ep(mm, n, acc[r]);
            }
        }
    }
}

// T[x, a, c] = sum_b W1[a, b, c] src[k x + b] (src = q: the item image) -- and, with src = p, S_u[y, b, c] when `transposed`
__device__ __forceinline__ void cn_fill_T(const CnP& g, const float* src, float* T, bool transposed) {
    const int k = g.k[1], C1 = g.C[1], n = g.H[1] * k * C1;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int c = e % C1, xa = e / C1, a = xa % k, x = xa / k;
        float t = 0.f;
        for (int b = 0; b < k; ++b) t = fmaf(g.W[1][((transposed ? b * k + a : a * k + b)) * C1 + c], src[k * x + b], t);
        T[e] = t;
    }
}

// the conv tower of one pair: the pooled vector -> s.z.  A_2 .. A_(L-1) go to the workgroup's workspace, A_L too with store_last.
__device__ __forceinline__ void cn_forward(const CnP& g, float* wsb, const float* T, const CnLds& s, const float* w2, bool store_last) {
    const int L = g.L, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (L == 1) {
        const int H1 = g.H[1], C1 = g.C[1];
        float* D0 = wsb + g.oD0;
        for (int e = tid; e < H1 * C1; e += 256) {
            const int x = e / C1, c = e - x * C1;
            float a = 0.f;
            for (int y = 0; y < H1; ++y) {
                const float z = cn_z1(g, s.p, T, y, x, c);
                a += z > 0.f ? z : 0.f;
            }
            D0[e] = a;
        }
        __syncthreads();
        if (tid < C1) {
            double a = 0.0;
            for (int x = 0; x < H1; ++x) a += (double)D0[x * C1 + tid];
            s.z[tid] = a;
        }
        __syncthreads();
        return;
    }
    for (int l = 2; l <= L; ++l) {
        const CnIn in = {&g, s.p, T, l > 2 ? wsb + g.oA[l - 1] : nullptr, l};
        const float *Wl = l == 2 ? w2 : g.W[l], *bl = g.b[l];
        const int Cl = g.C[l];
        float* out = wsb + g.oA[l];
        const bool last = l == L, store = !last || store_last;
        double pool = 0.0;
        cn_gemm(
            g.H[l] * g.H[l], Cl, g.k[l] * g.k[l] * g.C[l - 1], [&](int m, int k) { return cn_patch(in, m, k); },
            [&](int k, int n) { return Wl[k * Cl + n]; },
            [&](int m, int n, float v) {
                v += bl[n];
                v = v > 0.f ? v : 0.f;
                if (store) out[(int64_t)m * Cl + n] = v;
                if (last) pool += (double)v;
            });
        if (last) {
            pool += __shfl_xor(pool, 32, 64);
            if (lane < 32) s.pool[wave * 32 + lane] = pool;
        }
        __syncthreads();
    }
    const int CL = g.C[L], nt = (CL + 31) >> 5;                        // a wave's tiles all lie in column tile wave % nt (nt = 1, 2)
    if (tid < CL) {
        double a = 0.0;
        for (int w = 0; w < 4; ++w)
            if (w % nt == (tid >> 5)) a += s.pool[w * 32 + (tid & 31)];
        s.z[tid] = a;
    }
    __syncthreads();
}

// Dropout, Dense(C, linear), Dropout, Dense(1, linear) on s.z -> s.x[0]
__device__ __forceinline__ void cn_head(const CnP& g, const CnLds& s, bool train, u32 call, u32 sample) {
    const int C = g.C[g.L], tid = threadIdx.x;
    if (tid < C) {
        s.k0[tid] = train ? cn_keep(g.rate, g.seed, g.step, call, sample, 0u, (u32)tid) : 1.f;
        s.k1[tid] = train ? cn_keep(g.rate, g.seed, g.step, call, sample, 1u, (u32)tid) : 1.f;
        s.zd[tid] = s.z[tid] * (double)s.k0[tid];
    }
    __syncthreads();
    if (tid < C) {
        double h = (double)g.D[1][tid];
        for (int c = 0; c < C; ++c) h = fma(s.zd[c], (double)g.D[0][c * C + tid], h);
        s.h[tid] = h;
        s.hd[tid] = h * (double)s.k1[tid];
    }
    __syncthreads();
    if (tid == 0) {
        double x = (double)g.D[3][0];
        for (int j = 0; j < C; ++j) x = fma(s.hd[j], (double)g.D[2][j], x);
        s.x[0] = x;
    }
    __syncthreads();
}

#define CN_LDS_DECL                                                                   \
    __shared__ __attribute__((aligned(16))) float s_w2[CN_W2_LDS];                    \
    __shared__ float s_pq[2][256], s_v[3][64];                                        \
    __shared__ double s_pool[128], s_d[5][64], s_x[1];                                \
    const CnLds s = {s_pq[0], s_pq[1], s_v[0], s_v[1], s_v[2], s_pool, s_d[0], s_d[1], s_d[2], s_d[3], s_d[4], s_x}

// W_2 into LDS once per workgroup where it fits
__device__ __forceinline__ const float* cn_stage_w2(const CnP& g, float* s_w2) {
    if (g.L < 2) return nullptr;
    const int n = g.k[2] * g.k[2] * g.C[1] * g.C[2];
    if (n > CN_W2_LDS) return g.W[2];
    for (int e = threadIdx.x; e < n; e += 256) s_w2[e] = g.W[2][e];
    __syncthreads();
    return s_w2;
}

__device__ __forceinline__ void cn_range(int64_t n, int64_t& e0, int64_t& e1) {
    const int64_t per = (n + gridDim.x - 1) / gridDim.x;
    e0 = (int64_t)blockIdx.x * per;
    e0 = e0 < n ? e0 : n;
    e1 = e0 + per < n ? e0 + per : n;
}

// p and q of a pair into LDS (zeros behind F), their squared norms (wave 0, a fixed tree) for the regulariser
__device__ __forceinline__ void cn_load_pq(const CnP& g, const CnLds& s, int64_t u, int64_t i, double* sqp, double* sqq) {
    const int tid = threadIdx.x;
    s.p[tid] = tid < g.F ? g.P[u * g.F + tid] : 0.f;
    s.q[tid] = tid < g.F ? g.Q[i * g.F + tid] : 0.f;
    __syncthreads();
    if (sqp && tid < 64) {
        double a = 0.0, b = 0.0;
        for (int f = tid; f < g.F; f += 64) a += (double)s.p[f] * (double)s.p[f], b += (double)s.q[f] * (double)s.q[f];
        a = el_group_sum(a, 64), b = el_group_sum(b, 64);
        if (tid == 0) *sqp = a, *sqq = b;
    }
}

// mode 0: pair e < B is (u[e], i[e]), pair e >= B is (u[e - B], j[e - B]); T_i is made per pair.  train: dropout of step g.step.
// mode 1: pair e is (u_start + e / I, e % I), T_i is row e % I of the item image, out[(e / I) ld + e % I].
__global__ __launch_bounds__(256) void k_cnmf_fwd(CnP g, const int32_t* __restrict__ u, const int32_t* __restrict__ i, const int32_t* __restrict__ j,
                                                  int64_t npairs, int64_t B, int mode, int train, const float* __restrict__ image, int64_t u_start,
                                                  int64_t I, float* __restrict__ out, int64_t ld, double* __restrict__ xd, double* __restrict__ sqp,
                                                  double* __restrict__ sqq) {
    CN_LDS_DECL;
    const float* w2 = cn_stage_w2(g, s_w2);
    float* wsb = g.wsf + (int64_t)blockIdx.x * g.ws_stride;
    const int64_t timg = (int64_t)g.H[1] * g.k[1] * g.C[1];
    int64_t e0, e1;
    cn_range(npairs, e0, e1);
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t smp = mode ? 0 : (e < B ? e : e - B);
        const int64_t uu = mode ? u_start + e / I : u[smp], ii = mode ? e % I : (e < B ? i[smp] : j[smp]);
        cn_load_pq(g, s, uu, ii, sqp ? sqp + e : nullptr, sqq ? sqq + e : nullptr);
        const float* T = mode ? image + ii * timg : wsb + g.oT;
        if (!mode) {
            cn_fill_T(g, s.q, wsb + g.oT, false);
            __syncthreads();
        }
        cn_forward(g, wsb, T, s, w2, false);
        cn_head(g, s, train != 0, e < B ? 0u : 1u, (u32)smp);
        if (threadIdx.x == 0) {
            if (xd) xd[e] = s.x[0];                                       // a step keeps the unrounded score for its loss
            else out[mode ? (e / I) * ld + e % I : e] = (float)s.x[0];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_cnmf_image(CnP g, int64_t I, float* __restrict__ image) {
    __shared__ float s_q[256];
    const int64_t timg = (int64_t)g.H[1] * g.k[1] * g.C[1];
    for (int64_t it = blockIdx.x; it < I; it += gridDim.x) {
        s_q[threadIdx.x] = (int)threadIdx.x < g.F ? g.Q[it * g.F + threadIdx.x] : 0.f;
        __syncthreads();
        cn_fill_T(g, s_q, image + it * timg, false);
        __syncthreads();
    }
}

// x = x_ui - x_uj -> the loss and dL/dx of both calls; one workgroup, samples strided over the threads, a fixed tree behind
__global__ __launch_bounds__(256) void k_cnmf_loss(const double* __restrict__ x, const double* __restrict__ sqp, const double* __restrict__ sqq,
                                                   int64_t B, float l_w, double* __restrict__ dx, double* loss_out) {
    __shared__ double red[256];
    double a = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += 256) {
        const double d = x[b] - x[B + b];
        const bool in = d >= -80.0 && d <= 1e8;
        const double dc = d < -80.0 ? -80.0 : (d > 1e8 ? 1e8 : d);
        a += (dc > 0.0 ? log1p(exp(-dc)) : -dc + log1p(exp(dc))) + (double)l_w * 0.5 * (sqp[b] + sqq[b] + sqq[B + b]);
        const double gd = in ? -1.0 / (1.0 + exp(dc)) : 0.0;
        dx[b] = gd;
        dx[B + b] = -gd;
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_out += red[0];
}

// dZ_l as the layers around it read it: zero outside the part of the map the layer above covers
__device__ __forceinline__ float cn_dz(const CnP& g, int l, const float* dZ, int pix, int n) {
    const int Hl = g.H[l], y = pix / Hl, x = pix - y * Hl;
    return (y < g.Hc[l] && x < g.Hc[l]) ? dZ[(int64_t)pix * g.C[l] + n] : 0.f;
}

__global__ __launch_bounds__(256) void k_cnmf_bwd(CnP g, const int32_t* __restrict__ u, const int32_t* __restrict__ i, const int32_t* __restrict__ j,
                                                  int64_t B, const double* __restrict__ dxs, float* __restrict__ dpr, float* __restrict__ dqr) {
    CN_LDS_DECL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* w2 = cn_stage_w2(g, s_w2);
    float* wsb = g.wsf + (int64_t)blockIdx.x * g.ws_stride;
    double* slot = g.slots + (int64_t)blockIdx.x * g.slot_stride;
    for (int64_t e = tid; e < g.slot_stride; e += 256) slot[e] = 0.0;
    __syncthreads();
    const int L = g.L, F = g.F, C = g.C[L], k1 = g.k[1], C1 = g.C[1], H1 = g.H[1], Hc1 = g.Hc[1];
    float *T = wsb + g.oT, *S = wsb + g.oS, *G = wsb + g.oG, *D0 = wsb + g.oD0, *Z1 = wsb + g.oZ1;
    int64_t e0, e1;
    cn_range(2 * B, e0, e1);
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t smp = e < B ? e : e - B;
        cn_load_pq(g, s, u[smp], e < B ? i[smp] : j[smp], nullptr, nullptr);
        cn_fill_T(g, s.q, T, false);
        cn_fill_T(g, s.p, S, true);
        __syncthreads();
        cn_forward(g, wsb, T, s, w2, true);
        cn_head(g, s, true, e < B ? 0u : 1u, (u32)smp);
        const double dx = dxs[e];

        // the head
        if (tid < C) {
            const double dh = dx * (double)g.D[2][tid] * (double)s.k1[tid];
            slot[g.oD[2] + tid] += dx * s.hd[tid];
            s.dh[tid] = dh;                                               // (the two head biases: k_cnmf_head_bias)
        }
        __syncthreads();
        if (tid < C) {
            double a = 0.0;
            for (int jj = 0; jj < C; ++jj) a = fma(s.dh[jj], (double)g.D[0][tid * C + jj], a);
            s.dz[tid] = (float)(a * (double)s.k0[tid]);
        }
        for (int t = tid; t < C * C; t += 256) slot[g.oD[0] + t] += s.zd[t / C] * s.dh[t % C];
        __syncthreads();

        // dZ_L
        if (L == 1) {
            for (int t = tid; t < H1 * H1 * C1; t += 256) {
                const int c = t % C1, yx = t / C1;
                Z1[t] = cn_z1(g, s.p, T, yx / H1, yx % H1, c) > 0.f ? s.dz[c] : 0.f;
            }
        } else {
            float* aL = wsb + g.oA[L];
            for (int t = tid; t < g.H[L] * g.H[L] * C; t += 256) aL[t] = aL[t] > 0.f ? s.dz[t % C] : 0.f;
        }
        __syncthreads();

        for (int l = L; l >= 2; --l) {
            const CnIn in = {&g, s.p, T, l > 2 ? wsb + g.oA[l - 1] : nullptr, l};
            const float *dZ = wsb + g.oA[l], *Wl = l == 2 ? w2 : g.W[l];
            const int Cl = g.C[l], Kl = g.k[l] * g.k[l] * g.C[l - 1], pix = g.H[l] * g.H[l];
            double *sW = slot + g.oW[l], *sb = slot + g.ob[l];
            cn_gemm(
                Kl + 1, Cl, pix, [&](int m, int p) { return m == Kl ? 1.f : cn_patch(in, p, m); },
                [&](int p, int n) { return cn_dz(g, l, dZ, p, n); },
                [&](int m, int n, float v) {
                    if (m == Kl) sb[n] += (double)v;
                    else sW[(int64_t)m * Cl + n] += (double)v;
                });
            __syncthreads();
            float* below = l > 2 ? wsb + g.oA[l - 1] : Z1;
            cn_gemm(
                pix, Kl, Cl, [&](int p, int n) { return cn_dz(g, l, dZ, p, n); }, [&](int n, int kk) { return Wl[kk * Cl + n]; },
                [&](int p, int kk, float v) {
                    int Y, X, ci;
                    cn_patch_at(g, l, p, kk, Y, X, ci);
                    const int64_t at = ((int64_t)Y * g.H[l - 1] + X) * g.C[l - 1] + ci;
                    const float zb = l > 2 ? below[at] : cn_z1(g, s.p, T, Y, X, ci);
                    below[at] = zb > 0.f ? v : 0.f;
                });
            __syncthreads();
        }

        // layer 1 from dZ_1 on [0, Hc1)^2: G[x, a, c] = sum_y p[k y + a] dZ_1[y, x, c], D0[x, c] = sum_y dZ_1[y, x, c]
        for (int t = tid; t < Hc1 * C1; t += 256) {
            const int x = t / C1, c = t - x * C1;
            double ga[4] = {0.0, 0.0, 0.0, 0.0}, d0 = 0.0;
            for (int y = 0; y < Hc1; ++y) {
                const double d = (double)Z1[((int64_t)y * H1 + x) * C1 + c];
                d0 += d;
                for (int a = 0; a < k1; ++a) ga[a] = fma((double)s.p[k1 * y + a], d, ga[a]);
            }
            D0[t] = (float)d0;
            for (int a = 0; a < k1; ++a) G[((int64_t)x * k1 + a) * C1 + c] = (float)ga[a];
        }
        __syncthreads();
        for (int t = tid; t < k1 * k1 * C1; t += 256) {                   // dW1[a, b, c] = sum_x q[k x + b] G[x, a, c]
            const int c = t % C1, ab = t / C1, a = ab / k1, b = ab % k1;
            double w = 0.0;
            for (int x = 0; x < Hc1; ++x) w = fma((double)s.q[k1 * x + b], (double)G[((int64_t)x * k1 + a) * C1 + c], w);
            slot[g.oW[1] + t] += w;
        }
        if (tid < C1) {
            double w = 0.0;
            for (int x = 0; x < Hc1; ++x) w += (double)D0[x * C1 + tid];
            slot[g.ob[1] + tid] += w;
        }
        // dp[k y + a] = sum_(x, c) dZ_1[y, x, c] T[x, a, c];  dq[k x + b] = sum_(y, c) dZ_1[y, x, c] S[y, b, c]: a wave per y / x
        float *dp = dpr + e * F, *dq = dqr + e * F;
        for (int f = k1 * Hc1 + tid; f < F; f += 256) dp[f] = 0.f, dq[f] = 0.f;
        for (int r = wave; r < 2 * Hc1; r += 4) {
            const bool qs = r >= Hc1;
            const int yx = qs ? r - Hc1 : r;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int t = lane; t < Hc1 * C1; t += 64) {
                const int o = t / C1, c = t - o * C1;                     // the other coordinate
                const double d = (double)Z1[(qs ? (int64_t)o * H1 + yx : (int64_t)yx * H1 + o) * C1 + c];
                const float* f = (qs ? S : T) + (int64_t)o * k1 * C1 + c;
                for (int a = 0; a < k1; ++a) acc[a] = fma(d, (double)f[a * C1], acc[a]);
            }
            for (int a = 0; a < k1; ++a) {
                const double v = el_group_sum(acc[a], 64);
                if (lane == 0) (qs ? dq : dp)[k1 * yx + a] = (float)v;
            }
        }
        __syncthreads();
    }
}

// The two head biases see x_ui and x_uj through the same weights: their gradients are the sums over the TRIPLETS, in sample order, of
// the triplet's own two terms -- which cancel exactly where the two calls share their masks (no dropout), as they do in the loss.
__global__ __launch_bounds__(128) void k_cnmf_head_bias(const double* __restrict__ dx, int64_t B, int C, const float* __restrict__ Wd2, float rate,
                                                        u64 seed, u32 step, float* __restrict__ gbd1, float* __restrict__ gbd2) {
    const int jj = threadIdx.x;
    if (jj > C) return;
    double a = 0.0;
    const double w = jj < C ? (double)Wd2[jj] : 0.0;
    for (int64_t b = 0; b < B; ++b) {
        if (jj == C) a += dx[b] + dx[B + b];
        else a += dx[b] * w * (double)cn_keep(rate, seed, step, 0u, (u32)b, 1u, (u32)jj) + dx[B + b] * w * (double)cn_keep(rate, seed, step, 1u, (u32)b, 1u, (u32)jj);
    }
    (jj == C ? gbd2 : gbd1 + jj)[0] = (float)a;
}

struct CnVars {
    float* dst[2 * CN_MAXL + 4];
    int64_t off[2 * CN_MAXL + 4], n[2 * CN_MAXL + 4];
    int nv;
};
// every conv and Dense gradient: the workgroups' slots added in workgroup order
__global__ __launch_bounds__(256) void k_cnmf_finish(CnVars v, const double* __restrict__ slots, int64_t slot_stride, int nwg) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= slot_stride) return;
    double a = 0.0;
    for (int w = 0; w < nwg; ++w) a += slots[(int64_t)w * slot_stride + t];
    for (int q = 0; q < v.nv; ++q)
        if (t >= v.off[q] && t < v.off[q] + v.n[q]) v.dst[q][t - v.off[q]] = (float)a;
}

__global__ __launch_bounds__(256) void k_cnmf_keys(const int32_t* __restrict__ u, const int32_t* __restrict__ i, const int32_t* __restrict__ j,
                                                   int64_t B, u32* __restrict__ ku, u32* __restrict__ vu, u32* __restrict__ ki, u32* __restrict__ vi) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    ku[b] = (u32)u[b], vu[b] = (u32)b;
    ki[b] = (u32)i[b], vi[b] = (u32)b;
    ki[B + b] = (u32)j[b], vi[B + b] = (u32)(B + b);
}

// one wave per sorted position that begins a segment: the row's gradient = its pairs' rows in ascending sample order, l_w * row added per
// occurrence.  user: sample b brings the rows of both its pairs (b, then B + b) and one l_w p_u.
__global__ __launch_bounds__(256) void k_cnmf_seg(const u32* __restrict__ keys, const u32* __restrict__ vals, int64_t n, int64_t B, int user,
                                                  const float* __restrict__ rows, const float* __restrict__ tab, float l_w, int F,
                                                  float* __restrict__ gtab) {
    const int64_t pos = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (pos >= n) return;
    const u32 row = keys[pos];
    if (pos > 0 && keys[pos - 1] == row) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, th[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) th[q] = lane + 64 * q < F ? (double)l_w * (double)tab[(int64_t)row * F + lane + 64 * q] : 0.0;
    for (int64_t p = pos; p < n && keys[p] == row; ++p) {
        const int64_t e = vals[p];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = lane + 64 * q;
            if (f >= F) continue;
            acc[q] += (double)rows[e * F + f];
            if (user) acc[q] += (double)rows[(B + e) * F + f];
            acc[q] += th[q];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (lane + 64 * q < F) gtab[(int64_t)row * F + lane + 64 * q] = (float)acc[q];
}

__global__ __launch_bounds__(256) void k_cnmf_zero(float* __restrict__ x, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) x[e] = 0.f;
}

// out[call, layer, b, c]: the factors cn_head applies in step `step`
__global__ __launch_bounds__(256) void k_cnmf_masks(float rate, u64 seed, u32 step, int64_t B, int C, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 4 * B * C) return;
    const int c = (int)(t % C);
    const int64_t b = (t / C) % B, cl = t / (C * B);
    out[t] = cn_keep(rate, seed, step, (u32)(cl >> 1), (u32)b, (u32)(cl & 1), (u32)c);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// the supported range, and the geometry of a state that lies in it
int cnmf_geom(const el_cnmf_state* st, const char* who, int level, CnP* g) {
    EL_REQUIRE(st != nullptr, "%s: null state", who);
    EL_REQUIRE(st->U > 0 && st->I > 0 && st->U < (1LL << 31) && st->I < (1LL << 31), "%s: bad shape U=%lld I=%lld", who, (long long)st->U,
               (long long)st->I);
    const int L = st->n_layers;
    EL_REQUIRE(L >= 1 && L <= CN_MAXL, "%s: %d conv layers (layers: 1 .. %d)", who, L, CN_MAXL);
    EL_REQUIRE(st->F >= 1 && st->F <= 256, "%s: embedding_size %d (1 .. 256)", who, st->F);
    EL_REQUIRE(st->channels[0] == 1, "%s: channels[0] = %d (the interaction map has one channel)", who, st->channels[0]);
    memset(g, 0, sizeof(*g));
    g->L = L, g->F = st->F, g->C[0] = 1, g->H[0] = st->F;
    for (int l = 1; l <= L; ++l) {
        const int C = st->channels[l], k = st->kernels[l - 1], sd = st->strides[l - 1];
        EL_REQUIRE(C >= 1 && C <= 64, "%s: channels[%d] = %d (1 .. 64)", who, l, C);
        EL_REQUIRE(sd == k, "%s: stride %d of layer %d differs from its kernel %d (only non-overlapping patches)", who, sd, l, k);
        EL_REQUIRE(k >= 1 && k <= 4, "%s: kernel %d of layer %d (1 .. 4)", who, k, l);
        EL_REQUIRE(g->H[l - 1] >= k, "%s: the map of side %d below layer %d is smaller than its kernel %d", who, g->H[l - 1], l, k);
        g->C[l] = C, g->k[l] = k, g->H[l] = (g->H[l - 1] - k) / k + 1;
        EL_REQUIRE(st->W[l - 1] && st->b[l - 1], "%s: conv layer %d has no kernel or bias", who, l);
        if (level >= 1) EL_REQUIRE(st->gW[l - 1] && st->gb[l - 1], "%s: conv layer %d has no gradient buffers", who, l);
        if (level >= 2) EL_REQUIRE(st->mW[l - 1] && st->vW[l - 1] && st->mb[l - 1] && st->vb[l - 1], "%s: conv layer %d: Adam slots missing", who, l);
        g->W[l] = st->W[l - 1], g->b[l] = st->b[l - 1];
    }
    for (int l = 1; l <= L; ++l) g->Hc[l] = l < L ? g->k[l + 1] * g->H[l + 1] : g->H[l];
    EL_REQUIRE(st->P && st->Q, "%s: needs the two tables", who);
    EL_REQUIRE(st->dropout >= 0.f && st->dropout < 1.f, "%s: dropout_prob %g (0 <= . < 1)", who, (double)st->dropout);
    for (int q = 0; q < 4; ++q) {
        EL_REQUIRE(st->D[q], "%s: a Dense kernel or bias is missing", who);
        if (level >= 1) EL_REQUIRE(st->gD[q], "%s: a Dense gradient buffer is missing", who);
        if (level >= 2) EL_REQUIRE(st->mD[q] && st->vD[q], "%s: Dense Adam slots missing", who);
        g->D[q] = st->D[q];
    }
    if (level >= 1) EL_REQUIRE(st->gP && st->gQ, "%s: needs gP and gQ", who);
    if (level >= 2) EL_REQUIRE(st->mP && st->vP && st->mQ && st->vQ, "%s: table Adam slots missing", who);
    g->P = st->P, g->Q = st->Q, g->rate = st->dropout, g->seed = st->seed;
    return 0;
}

int64_t cn_up64(int64_t x) { return (x + 63) & ~(int64_t)63; }

// the per-workgroup workspace (and, bwd, the gradient slot) of the geometry: offsets in floats
void cnmf_wg_layout(CnP* g, bool bwd) {
    const int64_t t = cn_up64((int64_t)g->H[1] * g->k[1] * g->C[1]);
    int64_t o = 0;
    g->oT = o, o += t;
    g->oD0 = o, o += cn_up64((int64_t)g->H[1] * g->C[1]);
    for (int l = 2; l <= g->L; ++l) g->oA[l] = o, o += cn_up64((int64_t)g->H[l] * g->H[l] * g->C[l]);
    if (bwd) {
        g->oS = o, o += t;
        g->oG = o, o += t;
        g->oZ1 = o, o += cn_up64((int64_t)g->H[1] * g->H[1] * g->C[1]);
    }
    g->ws_stride = o;
    o = 0;
    if (bwd) {
        const int C = g->C[g->L];
        for (int l = 1; l <= g->L; ++l) {
            g->oW[l] = o, o += (int64_t)g->k[l] * g->k[l] * g->C[l - 1] * g->C[l];
            g->ob[l] = o, o += g->C[l];
        }
        g->oD[0] = o, o += (int64_t)C * C;
        g->oD[1] = o, o += C;
        g->oD[2] = o, o += C;
        g->oD[3] = o, o += 1;
    }
    g->slot_stride = o;
}

// persistent workgroups of a call over npairs pairs
int cnmf_nwg(el_ctx* ctx, const CnP& g, int64_t npairs) {
    int64_t n = (int64_t)ctx->cus * 2;
    const int64_t per = (g.ws_stride + 2 * g.slot_stride) * (int64_t)sizeof(float), fit = CN_WG_BYTES / (per > 0 ? per : 1);
    n = n < fit ? n : fit;
    n = n < npairs ? n : npairs;
    return (int)(n < 1 ? 1 : n);
}

struct CnWs {
    float *dpr, *dqr, *wg;
    double *x, *dx, *slots, *sqp, *sqq;
    u32 *ku_in, *vu_in, *ku, *vu, *ki_in, *vi_in, *ki, *vi;
    void* sort_tmp;
    size_t sort_bytes, total;
    int nwg;
};

// which: EL_CNMF_WS_STEP (n = B), _FORWARD (n pairs), _SCORES (n users); g is laid out for it on return
int cnmf_carve(el_ctx* ctx, const el_cnmf_state* st, CnP* g, int64_t n, int which, void* base, CnWs* w) {
    ElCarve c{(char*)base};
    memset(w, 0, sizeof(*w));
    const bool step = which == EL_CNMF_WS_STEP;
    cnmf_wg_layout(g, step);
    const int64_t npairs = step ? 2 * n : (which == EL_CNMF_WS_SCORES ? n * st->I : n);
    w->nwg = cnmf_nwg(ctx, *g, npairs);
    w->wg = c.take<float>((size_t)w->nwg * (size_t)g->ws_stride);
    if (step) {
        const size_t B = (size_t)n, F = (size_t)st->F;
        w->slots = c.take<double>((size_t)w->nwg * (size_t)g->slot_stride);
        w->x = c.take<double>(2 * B);
        w->dx = c.take<double>(2 * B);
        w->sqp = c.take<double>(2 * B);
        w->sqq = c.take<double>(2 * B);
        w->dpr = c.take<float>(2 * B * F);
        w->dqr = c.take<float>(2 * B * F);
        w->ku_in = c.take<u32>(B), w->vu_in = c.take<u32>(B), w->ku = c.take<u32>(B), w->vu = c.take<u32>(B);
        w->ki_in = c.take<u32>(2 * B), w->vi_in = c.take<u32>(2 * B), w->ki = c.take<u32>(2 * B), w->vi = c.take<u32>(2 * B);
        size_t t = 0;
        u32* np = nullptr;
        if (rocprim::radix_sort_pairs(nullptr, t, np, np, np, np, (unsigned)(2 * B), 0, 32, (hipStream_t)0) != hipSuccess) return 1;
        w->sort_bytes = t;
        w->sort_tmp = c.take<char>(t);
    }
    w->total = c.off;
    g->wsf = w->wg, g->slots = w->slots;
    return 0;
}

int cnmf_grads(el_ctx* ctx, hipStream_t s, const el_cnmf_state* st, CnP g, const int32_t* u, const int32_t* i, const int32_t* j, int64_t B,
               int32_t step, double* loss_out, void* ws, size_t ws_bytes, const char* who) {
    EL_REQUIRE(u && i && j && loss_out, "%s: null argument", who);
    EL_REQUIRE(B >= 1 && B < (1LL << 29), "%s: batch size %lld out of range", who, (long long)B);
    CnWs w;
    EL_REQUIRE(cnmf_carve(ctx, st, &g, B, EL_CNMF_WS_STEP, ws, &w) == 0, "%s: rocprim size query failed", who);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    g.step = (u32)step;
    const int F = st->F;
    EL_LAUNCH("k_cnmf_fwd", k_cnmf_fwd, dim3((unsigned)w.nwg), dim3(256), 0, s, g, u, i, j, 2 * B, B, 0, 1, (const float*)nullptr, (int64_t)0, st->I,
              (float*)nullptr, (int64_t)0, w.x, w.sqp, w.sqq);
    EL_LAUNCH("k_cnmf_loss", k_cnmf_loss, dim3(1), dim3(256), 0, s, w.x, w.sqp, w.sqq, B, st->l_w, w.dx, loss_out);
    EL_LAUNCH("k_cnmf_bwd", k_cnmf_bwd, dim3((unsigned)w.nwg), dim3(256), 0, s, g, u, i, j, B, w.dx, w.dpr, w.dqr);
    CnVars v;
    v.nv = 0;
    for (int l = 1; l <= g.L; ++l) {
        v.dst[v.nv] = st->gW[l - 1], v.off[v.nv] = g.oW[l], v.n[v.nv++] = (int64_t)g.k[l] * g.k[l] * g.C[l - 1] * g.C[l];
        v.dst[v.nv] = st->gb[l - 1], v.off[v.nv] = g.ob[l], v.n[v.nv++] = g.C[l];
    }
    const int C = g.C[g.L];
    const int64_t nd[4] = {(int64_t)C * C, C, C, 1};
    for (int q = 0; q < 4; q += 2) v.dst[v.nv] = st->gD[q], v.off[v.nv] = g.oD[q], v.n[v.nv++] = nd[q];
    EL_LAUNCH("k_cnmf_head_bias", k_cnmf_head_bias, dim3(1), dim3(128), 0, s, w.dx, B, C, st->D[2], st->dropout, st->seed, (u32)step, st->gD[1],
              st->gD[3]);
    EL_LAUNCH("k_cnmf_finish", k_cnmf_finish, dim3((unsigned)((g.slot_stride + 255) / 256)), dim3(256), 0, s, v, w.slots, g.slot_stride, w.nwg);
    // the tables: zero, then the rows of the batch's distinct users and items
    EL_LAUNCH("k_cnmf_zero", k_cnmf_zero, dim3(el_stream_grid(ctx, st->U * F)), dim3(256), 0, s, st->gP, st->U * F);
    EL_LAUNCH("k_cnmf_zero", k_cnmf_zero, dim3(el_stream_grid(ctx, st->I * F)), dim3(256), 0, s, st->gQ, st->I * F);
    EL_LAUNCH("k_cnmf_keys", k_cnmf_keys, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, u, i, j, B, w.ku_in, w.vu_in, w.ki_in, w.vi_in);
    {
        ElKernelTimer t("rocprim_radix_sort_pairs", s);
        size_t tb = w.sort_bytes;
        EL_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tb, w.ku_in, w.ku, w.vu_in, w.vu, (unsigned)B, 0, el_bits_for(st->U), s));
        tb = w.sort_bytes;
        EL_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tb, w.ki_in, w.ki, w.vi_in, w.vi, (unsigned)(2 * B), 0, el_bits_for(st->I), s));
    }
    EL_LAUNCH("k_cnmf_seg_u", k_cnmf_seg, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, w.ku, w.vu, B, B, 1, w.dpr, st->P, st->l_w, F, st->gP);
    EL_LAUNCH("k_cnmf_seg_i", k_cnmf_seg, dim3((unsigned)((2 * B + 3) / 4)), dim3(256), 0, s, w.ki, w.vi, 2 * B, B, 0, w.dqr, st->Q, st->l_w, F,
              st->gQ);
    EL_CHECK_LAUNCH();
    return 0;
}

// Keras Adam: the sparse apply's arithmetic on every row of the two tables (k_adam_dense), TF's dense ApplyAdam on the rest
int cnmf_apply(el_ctx* ctx, hipStream_t s, const el_cnmf_state* st, const CnP& g, float lr_t) {
    const int64_t np = st->U * st->F, nq = st->I * st->F;
    EL_LAUNCH("k_adam_dense_P", k_adam_dense, dim3(el_stream_grid(ctx, np / 4 + 1)), dim3(256), 0, s, st->P, st->gP, st->mP, st->vP, np, lr_t, 0.9f,
              0.999f, 1e-7f);
    EL_LAUNCH("k_adam_dense_Q", k_adam_dense, dim3(el_stream_grid(ctx, nq / 4 + 1)), dim3(256), 0, s, st->Q, st->gQ, st->mQ, st->vQ, nq, lr_t, 0.9f,
              0.999f, 1e-7f);
    for (int l = 1; l <= g.L; ++l) {
        const int64_t nw = (int64_t)g.k[l] * g.k[l] * g.C[l - 1] * g.C[l];
        EL_LAUNCH("k_cnmf_opt_W", k_adam_apply_dense, dim3(el_stream_grid(ctx, nw)), dim3(256), 0, s, st->W[l - 1], st->gW[l - 1], st->mW[l - 1],
                  st->vW[l - 1], nw, lr_t, 0.9f, 0.999f, 1e-7f, 0);
        EL_LAUNCH("k_cnmf_opt_b", k_adam_apply_dense, dim3(1), dim3(256), 0, s, st->b[l - 1], st->gb[l - 1], st->mb[l - 1], st->vb[l - 1],
                  (int64_t)g.C[l], lr_t, 0.9f, 0.999f, 1e-7f, 0);
    }
    const int C = g.C[g.L];
    const int64_t nd[4] = {(int64_t)C * C, C, C, 1};
    for (int q = 0; q < 4; ++q)
        EL_LAUNCH("k_cnmf_opt_D", k_adam_apply_dense, dim3(el_stream_grid(ctx, nd[q])), dim3(256), 0, s, st->D[q], st->gD[q], st->mD[q], st->vD[q],
                  nd[q], lr_t, 0.9f, 0.999f, 1e-7f, 0);
    EL_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t el_cnmf_ws_bytes(el_ctx* ctx, const el_cnmf_state* st, int64_t n, int32_t which) {
    CnP g;
    if (!ctx || el_bind(ctx) || cnmf_geom(st, "el_cnmf_ws_bytes", 0, &g)) return 0;
    if (which != EL_CNMF_WS_STEP && which != EL_CNMF_WS_FORWARD && which != EL_CNMF_WS_SCORES) {
        el_set_error("el_cnmf_ws_bytes: unknown workspace %d", which);
        return 0;
    }
    if (n < 1 || n >= (1LL << 29)) {
        el_set_error("el_cnmf_ws_bytes: n = %lld out of range", (long long)n);
        return 0;
    }
    CnWs w;
    if (cnmf_carve(ctx, st, &g, n, which, nullptr, &w)) {
        el_set_error("el_cnmf_ws_bytes: rocprim size query failed");
        return 0;
    }
    return w.total > 0 ? w.total : 256;
}

extern "C" int el_cnmf_grads(el_ctx* ctx, void* stream, const el_cnmf_state* st, const int32_t* u, const int32_t* i, const int32_t* j, int64_t B,
                             int32_t step, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    CnP g;
    if (int rc = cnmf_geom(st, "el_cnmf_grads", 1, &g)) return rc;
    return cnmf_grads(ctx, (hipStream_t)stream, st, g, u, i, j, B, step, loss_out, ws, ws_bytes, "el_cnmf_grads");
}

extern "C" int el_cnmf_apply(el_ctx* ctx, void* stream, const el_cnmf_state* st, int32_t step, float lr_t) {
    if (int rc = el_bind(ctx)) return rc;
    CnP g;
    if (int rc = cnmf_geom(st, "el_cnmf_apply", 2, &g)) return rc;
    EL_REQUIRE(step >= 1, "el_cnmf_apply: step must be >= 1");
    return cnmf_apply(ctx, (hipStream_t)stream, st, g, lr_t);
}

extern "C" int el_cnmf_train_step(el_ctx* ctx, void* stream, const el_cnmf_state* st, const int32_t* u, const int32_t* i, const int32_t* j,
                                  int64_t B, int32_t step, float lr_t, double* loss_out, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    CnP g;
    if (int rc = cnmf_geom(st, "el_cnmf_train_step", 2, &g)) return rc;
    EL_REQUIRE(step >= 1, "el_cnmf_train_step: step must be >= 1");
    if (int rc = cnmf_grads(ctx, (hipStream_t)stream, st, g, u, i, j, B, step, loss_out, ws, ws_bytes, "el_cnmf_train_step")) return rc;
    return cnmf_apply(ctx, (hipStream_t)stream, st, g, lr_t);
}

extern "C" int el_cnmf_forward(el_ctx* ctx, void* stream, const el_cnmf_state* st, const int32_t* u, const int32_t* i, int64_t n, float* out,
                               void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    CnP g;
    if (int rc = cnmf_geom(st, "el_cnmf_forward", 0, &g)) return rc;
    if (n <= 0) return 0;
    EL_REQUIRE(u && i && out && n < (1LL << 29), "el_cnmf_forward: bad arguments");
    CnWs w;
    cnmf_carve(ctx, st, &g, n, EL_CNMF_WS_FORWARD, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "el_cnmf_forward: workspace too small (%zu < %zu)", ws_bytes, w.total);
    EL_LAUNCH("k_cnmf_fwd", k_cnmf_fwd, dim3((unsigned)w.nwg), dim3(256), 0, (hipStream_t)stream, g, u, i, (const int32_t*)nullptr, n, n, 0, 0,
              (const float*)nullptr, (int64_t)0, st->I, out, (int64_t)0, (double*)nullptr, (double*)nullptr, (double*)nullptr);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_cnmf_item_image(el_ctx* ctx, void* stream, const el_cnmf_state* st, float* image) {
    if (int rc = el_bind(ctx)) return rc;
    CnP g;
    if (int rc = cnmf_geom(st, "el_cnmf_item_image", 0, &g)) return rc;
    EL_REQUIRE(image, "el_cnmf_item_image: null image");
    const int64_t cap = (int64_t)ctx->cus * 8;
    EL_LAUNCH("k_cnmf_image", k_cnmf_image, dim3((unsigned)(st->I < cap ? st->I : cap)), dim3(256), 0, (hipStream_t)stream, g, st->I, image);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_cnmf_scores(el_ctx* ctx, void* stream, const el_cnmf_state* st, const float* image, int64_t u_start, int64_t u_stop, float* out,
                              int64_t ld, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    CnP g;
    if (int rc = cnmf_geom(st, "el_cnmf_scores", 0, &g)) return rc;
    EL_REQUIRE(image && out && u_start >= 0 && u_start < u_stop && u_stop <= st->U && ld >= st->I, "el_cnmf_scores: bad arguments");
    const int64_t n = u_stop - u_start;
    EL_REQUIRE(n < (1LL << 29), "el_cnmf_scores: chunk of %lld users out of range", (long long)n);
    CnWs w;
    cnmf_carve(ctx, st, &g, n, EL_CNMF_WS_SCORES, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "el_cnmf_scores: workspace too small (%zu < %zu)", ws_bytes, w.total);
    EL_LAUNCH("k_cnmf_scores", k_cnmf_fwd, dim3((unsigned)w.nwg), dim3(256), 0, (hipStream_t)stream, g, (const int32_t*)nullptr, (const int32_t*)nullptr,
              (const int32_t*)nullptr, n * st->I, n * st->I, 1, 0, image, u_start, st->I, out, ld, (double*)nullptr, (double*)nullptr,
              (double*)nullptr);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_cnmf_dropout_masks(el_ctx* ctx, void* stream, const el_cnmf_state* st, int32_t step, int64_t B, float* out) {
    if (int rc = el_bind(ctx)) return rc;
    CnP g;
    if (int rc = cnmf_geom(st, "el_cnmf_dropout_masks", 0, &g)) return rc;
    EL_REQUIRE(out && B >= 1 && B < (1LL << 29), "el_cnmf_dropout_masks: bad arguments");
    const int C = g.C[g.L];
    EL_LAUNCH("k_cnmf_masks", k_cnmf_masks, dim3((unsigned)((4 * B * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, st->dropout, st->seed,
              (u32)step, B, C, out);
    EL_CHECK_LAUNCH();
    return 0;
}
