// Full-catalog top-k, bf16-screened and fp32-exact (EL_TOPK_SCREEN).
//
// Same contract and the same answers as el_topk.hip (score = fp32 fma chain, order = score desc / item asc), but the
// 2*I*F flop per user run on the bf16 matrix cores (16x the fp32 MFMA rate) and only a handful of candidates per user
// are re-scored with the exact fp32 chain.  Exactness comes from a rigorous error bound, not from luck:
//
//   s   = exact fp32-chain score of (u, i)            s' = bf16 MFMA score  sum_f bf16(u_f) bf16(i_f)  (+ bias, fp32)
//   with u = u~ + du, i = i~ + di (u~, i~ the bf16 roundings; the residuals du, di are exact fp32 numbers):
//        u_f i_f - u~_f i~_f = du_f i~_f + u_f di_f      (identity)
//   |s - s'| <= E_u := ||du|| * max_i ||i~|| + ||u|| * max_i ||di|| + F * 2^-21 ||u|| max||i|| + 2^-21 (||u|| max||i|| + max|bias|)
//        (Cauchy-Schwarz on the two sums with the MEASURED residual norms -- ||du|| per user in k_screen_thr, max ||i~|| and
//         max ||di|| over the item shard in k_screen_prep, each with a 2^-10 margin for its own fp32 evaluation; round 1 used
//         the worst case 2^-8 per factor instead, ||u|| max||i|| 2^-7: 3x wider on real data, hence 3x more candidates;
//         fp32 accumulation of either chain: <= F 2^-24 sum|u_f i_f| each, taken with a 4x margin; bias add 2^-24 rel.)
//   If T is ANY value such that k unmasked items have s' >= T, every member of the exact top-k has s' >= T - 2 E_u.
//        (k items have s >= T - E_u, so the k-th exact score s_(k) >= T - E_u, and a member has s' >= s - E_u.)
//
// Selection in a stream is VALU work that the 16x faster matrix cores no longer hide, so the catalogue is passed twice:
//
//   pass 1  k_screen_pass<MODE 1>  s' for (user, item) pairs over every stride-th item tile; the only epilogue is a running
//           max per ACCUMULATOR POSITION: item tile row (64 of them) -> 64 disjoint item groups per user ("slot maxima").
//   thr     k_screen_thr           per user: slots whose maximum may belong to a masked (train) item are dropped -- the
//           masked items of the best slots are re-scored on the VALU and compared with a tolerance; T = kA-th largest
//           surviving slot maximum, thr = T - b E_u.  With stride 1 and kA = k, T is RIGOROUS (k distinct unmasked items
//           reach it) and b = 2; otherwise T is a GUESS aimed at rank ~5k that k_screen_final verifies (screen_policy below),
//           and b in [1, 1.5] follows the spacing of the user's top scores (see the kernel).
//   pass 2  k_screen_pass<MODE 2>  the GEMM over every tile (bit-identical s'), epilogue = max over the 16 accumulators of a
//           lane against thr; the rare hit appends one record (tile, row block, row mask) + its s' to the user's list
//           (surv + nnz_u slots, masked or not).
//   final   k_screen_final         per user: expand records, drop masked items, second-level screen on the recorded s',
//           exact fp32 chain for what is left, sort, VERIFY: k candidates with an exact score >= V = thr + E_u prove that no
//           non-candidate (s' < thr, hence exact < thr + E_u) belongs to the top-k; write.
//   Users that fail the verification, have fewer than kA clean slots, a non-finite bound, or more than `surv` unmasked hits
//   are flagged and recomputed exactly (el_topk_run_list in el_topk.hip), so the result is exact for every input.
//
// Geometry of a pass: 512 threads = 8 waves, 64 users per wave (2 MFMA column blocks; 1 above 128 factors) -> 512 users per
// workgroup share the staged 64-item bf16 tiles.  A operand (items): 16 B per lane straight out of an XOR-swizzled LDS
// image (conflict-free ds_read_b128); B operand (users): resident in VGPRs for the whole kernel; bias = C operand of the
// first MFMA of a chain; MFMA of one half tile is issued under the VALU epilogue of the other.
#include <stdio.h>
#include <stdlib.h>
#include "el_topk_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

#define SCR_TI 64        // items per tile == slots per user

__device__ __forceinline__ u32 el_f2bf(float x) {
    u32 b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    b += 0x7fffu + ((b >> 16) & 1u);
    return b >> 16;
}
__device__ __forceinline__ float el_bf2f(u32 h) { return __uint_as_float(h << 16); }

// E (screening error bound) and tol (bound on the difference of two fp32 evaluations of the same bf16 dot product)
// nu = ||u||, du = ||u - bf16(u)||, imax = max ||i||, imax_b = max ||bf16(i)||, dmax = max ||i - bf16(i)|| (all with their margins)
__device__ __forceinline__ void el_screen_bounds(float nu, float du, float imax, float imax_b, float dmax, float babs, int F, float& E,
                                                 float& tol) {
    tol = (float)F * 4.8e-7f * nu * imax + 4.8e-7f * (nu * imax + babs) + 1e-30f;
    E = du * imax_b + nu * dmax + tol;
}
#define SCR_STAT_IB 16   // stats[16] = max ||bf16(i)||, stats[17] = max ||i - bf16(i)||  (stats[0] = max ||i||, [1] = max |bias|)
#define SCR_STAT_ID 17

// accumulator position (tile row 0..63) -> slot id, the order pass 1 stores the maxima in
__device__ __forceinline__ int el_screen_slot(int row) {
    const int ib = row >> 5, r32 = row & 31;
    return ib * 32 + ((r32 >> 2) & 1) * 16 + (r32 & 3) + 4 * (r32 >> 3);
}

// ---- item side preparation: bf16 image [I][FP] (zero padded), max ||i||, max |bias| ------------------------------
// One thread per (item, 8-column chunk): 32 B in, 16 B out, the row norm is reduced over the SL = FP/8 lanes of the item.
template <int FP>
__global__ __launch_bounds__(256) void k_screen_prep(const float* __restrict__ Gi, const float* __restrict__ Bi, int64_t I,
                                                     int F, unsigned short* __restrict__ Gib, float* stats,
                                                     const unsigned long long* __restrict__ rebuild, float2* __restrict__ inorm) {
    constexpr int SL = FP / 8;
    if (*rebuild == 0ull) return;                         // the image in this workspace was built from these very tables
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t item = t / SL;
    const int sl = (int)(t % SL);
    float v[8];
    float ss = 0.f, sb = 0.f, sd = 0.f, amax = 0.f;
    const bool live = item < I;
    if (live) {
        const float* src = Gi + item * (int64_t)F + sl * 8;
        if ((F & 3) == 0 && sl * 8 + 8 <= F && ((reinterpret_cast<uintptr_t>(Gi) & 15) == 0)) {
            const float4 x = reinterpret_cast<const float4*>(src)[0], y = reinterpret_cast<const float4*>(src)[1];
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (sl * 8 + j < F) ? src[j] : 0.f;
        }
        uint4 o;
        o.x = el_f2bf(v[0]) | (el_f2bf(v[1]) << 16);
        o.y = el_f2bf(v[2]) | (el_f2bf(v[3]) << 16);
        o.z = el_f2bf(v[4]) | (el_f2bf(v[5]) << 16);
        o.w = el_f2bf(v[6]) | (el_f2bf(v[7]) << 16);
        *reinterpret_cast<uint4*>(Gib + item * FP + sl * 8) = o;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    }
    // The norms are taken SCALE-SAFELY: the squares of a row whose entries sit below ~1e-19 underflow to zero in fp32, the measured
    // residual norm would read 0 and the bound collapse below the true bf16 error (advisor, round 2).  Every entry is divided by the
    // row's largest magnitude first (a row maximum so small that its reciprocal overflows gives inf norms: every user falls back).
    for (int o = SL >> 1; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float rs = amax > 0.f ? 1.0f / amax : 0.f;
    if (live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float r = el_bf2f(el_f2bf(v[j])), d = v[j] - r;      // the residual of a bf16 rounding is an exact fp32 number
            const float vs = v[j] * rs, rr = r * rs, ds = d * rs;
            ss += vs * vs;
            sb += rr * rr;
            sd += ds * ds;
        }
    }
    ss = el_group_sum(ss, SL);                           // all SL lanes of an item hold its sum of squares
    sb = el_group_sum(sb, SL);
    sd = el_group_sum(sd, SL);
    float nrm = amax * sqrtf(ss) * 1.001f, nrb = amax * sqrtf(sb) * 1.001f, nrd = amax * sqrtf(sd) * 1.001f;
    if (!(nrm < INFINITY)) nrm = INFINITY;               // NaN / inf rows poison the bound -> every user falls back
    if (!(nrb < INFINITY)) nrb = INFINITY;
    if (!(nrd < INFINITY)) nrd = INFINITY;
    if (live && sl == 0) inorm[item] = make_float2(nrb, nrd);      // per-item norms: the second-level screen of k_screen_final
    u32 nmax = live ? __float_as_uint(nrm) : 0u;         // non-negative floats order as their bit patterns
    u32 nbmax = live ? __float_as_uint(nrb) : 0u, ndmax = live ? __float_as_uint(nrd) : 0u;
    u32 bmax = 0u;
    if (live && Bi && sl == 0) {
        float b = fabsf(Bi[item]);
        if (!(b < INFINITY)) b = INFINITY;
        bmax = __float_as_uint(b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nmax = max(nmax, (u32)__shfl_xor((int)nmax, o, 64));
        nbmax = max(nbmax, (u32)__shfl_xor((int)nbmax, o, 64));
        ndmax = max(ndmax, (u32)__shfl_xor((int)ndmax, o, 64));
        bmax = max(bmax, (u32)__shfl_xor((int)bmax, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {                       // same-address atomics serialise in L2: only raise, never re-assert
        unsigned int* st = reinterpret_cast<unsigned int*>(stats);
        if (nmax > __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st, nmax);
        if (bmax > __hip_atomic_load(st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st + 1, bmax);
        if (nbmax > __hip_atomic_load(st + SCR_STAT_IB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st + SCR_STAT_IB, nbmax);
        if (ndmax > __hip_atomic_load(st + SCR_STAT_ID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st + SCR_STAT_ID, ndmax);
    }
}

// ---- EL_TOPK_ITEMS_UNCHANGED is a claim the library checks -------------------------------------------------------
// A caller (any C host, not only the Python model classes with their weight-version counter) may update Gi / Bi IN PLACE
// between two blocks and still pass the flag: same pointers, same shape, stale bf16 image.  So the claim is verified on the
// device: k_items_hash folds every element of Gi and Bi (with its index) into an order-independent 64-bit sum -- a read-only
// pass over the table, about as long as building the image -- k_items_decide compares it with the hash the image in this
// workspace was built from, and k_screen_prep returns at once only when they agree.  No host synchronisation.
//   ctl[0] = hash the image was built from, ctl[1] = hash of the tables now, ctl[2] = 1: rebuild
__device__ __forceinline__ u64 el_mix_elem(u64 idx, u32 w) {
    u32 a = w + 0x9E3779B9u * (u32)(idx + 1), b = w ^ (0x85EBCA77u * (u32)((idx >> 7) + 3));
    a ^= a >> 16, a *= 0x85EBCA6Bu, a ^= a >> 13, a *= 0xC2B2AE35u, a ^= a >> 16;
    b ^= b >> 15, b *= 0x2C1B3C6Du, b ^= b >> 12, b *= 0x297A2D39u, b ^= b >> 15;
    return ((u64)a << 32) | (u64)b;
}

__global__ __launch_bounds__(256) void k_items_hash(const float* __restrict__ Gi, const float* __restrict__ Bi, int64_t n_g,
                                                    int64_t n_b, u64* ctl) {
    const u32* g = reinterpret_cast<const u32*>(Gi);
    const u32* b = reinterpret_cast<const u32*>(Bi);
    const int64_t stride = (int64_t)gridDim.x * 256, t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    u64 h = 0;
    if ((reinterpret_cast<uintptr_t>(Gi) & 15) == 0) {
        const uint4* g4 = reinterpret_cast<const uint4*>(Gi);
        const int64_t n4 = n_g >> 2;
        for (int64_t e = t; e < n4; e += stride) {
            const uint4 v = g4[e];
            h += el_mix_elem(4 * e, v.x) + el_mix_elem(4 * e + 1, v.y) + el_mix_elem(4 * e + 2, v.z) + el_mix_elem(4 * e + 3, v.w);
        }
        for (int64_t e = (n4 << 2) + t; e < n_g; e += stride) h += el_mix_elem(e, g[e]);
    } else {
        for (int64_t e = t; e < n_g; e += stride) h += el_mix_elem(e, g[e]);
    }
    if (Bi)
        for (int64_t e = t; e < n_b; e += stride) h += el_mix_elem(n_g + e, b[e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += (u64)__shfl_xor((long long)h, o, 64);
    __shared__ u64 part[4];                                // one atomic per workgroup: same-address atomics serialise in L2
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 tot = part[0] + part[1] + part[2] + part[3];
        if (tot != 0) atomicAdd(reinterpret_cast<unsigned long long*>(ctl + 1), (unsigned long long)tot);
    }
}

__global__ void k_items_decide(u64* ctl, float* stats, int force) {
    const bool stale = force || ctl[0] != ctl[1];
    ctl[0] = ctl[1];
    ctl[2] = stale ? 1ull : 0ull;
    if (stale) stats[0] = stats[1] = stats[SCR_STAT_IB] = stats[SCR_STAT_ID] = 0.f;   // the item-side maxima: re-derived by k_screen_prep
}

struct ScreenParams {
    TopkParams t;
    const unsigned short* Gib;   // [I_local][FP] bf16
    const float* stats;          // [0] max item norm, [1] max |bias|, [16] max norm of the bf16 image rows, [17] max residual norm
    float* smax;                 // [n_users][64] slot maxima (pass 1)
    float* thr;                  // [n_users] final threshold (+inf: user is flagged)
    int32_t* cnt;                // [n_users] hits appended in pass 2
    int32_t* ovf;                // [n_users] 1 = recompute with the exact wave kernel
    u64* lists;                  // user u: [64 * (u - u_start) + indptr[u] - indptr[u_start], +64 + nnz_u)
    float* lsc;                  // per record: the lane's best s' (exact for the record's item when its mask has one bit)
    int64_t list_cap;            // entries in `lists` / `lsc`
    int32_t* ulist;              // [n_users] flagged users (relative ids), filled by k_screen_flags
    int32_t* ulist_n;            // [1]
    const void* zeros;           // >= 16 bytes of zeros in device memory (LDS-DMA source of rows past the catalogue's end)
    float* Tg;                   // [n_users] V = thr + E: the level the k-th exact score must reach (k_screen_final verifies it)
    float* Eu;                   // [n_users] E_u
    float* nuv;                  // [n_users] ||u|| (with margin), k_screen_thr
    float* duv;                  // [n_users] ||u - bf16(u)||
    float2* inorm;               // [I_local] (||bf16(i)||, ||i - bf16(i)||) per item (with margins), k_screen_prep
    float band, band_min;        // thr = T - b E_u, b in [band_min, band] per user (k_screen_thr); 2 = the band a rigorous T needs
    int kA;                      // T = kA-th largest clean slot maximum (== k with stride 1: T is then rigorous)
    int surv;                    // unmasked hits a user may have before it is sent to the exact fallback (128 or 512)
    int stride;                  // pass 1 visits tiles t with t % stride == 0
    unsigned long long* prof;    // EL_SCREEN_PROF=1: [n_waves][8] cycle / event counters (developer tool)
    unsigned long long* prof2;   // EL_SCREEN_PROF=1: [16] sums over the users of k_screen_final: phase cycles and candidate counts
};

#define PROF_T() (PROF ? __builtin_amdgcn_s_memtime() : 0ull)

// v_max_f32 ignores a quiet NaN operand (MFMA results are quiet); fmaxf() would add a canonicalising v_max per call
__device__ __forceinline__ float el_vmax(float a, float b) {
    float d;
    asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ float el_vmax3(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// One pass over the catalogue.  Software pipeline per wave (acc[ub][ib]: ub = user column block, ib = item row block):
//
//     MFMA(t, ib1) || E(t, ib0)   ->   stage tile t+1, barrier   ->   MFMA(t+1, ib0) || E(t, ib1)
//
// the epilogue E of one half tile is VALU work issued while the matrix core runs the other half; the bias enters as the
// C operand of the first MFMA of a chain (s' = bias + sum, no VALU add).  LDS: two item tiles, a ring of four bias rows.
template <int FP, int MODE, int NW, int NSUB, int UB, bool PROF>
__global__ __launch_bounds__(NW * 64, 2) void k_screen_pass(ScreenParams sp) {
    constexpr int NT = NW * 64;
    constexpr int TI = SCR_TI;
    constexpr int ROWB = FP * 2;                // bytes per bf16 row
    constexpr int SL = FP / 8;                  // 16-byte slots per row
    constexpr int RPB = (256 / ROWB) ? (256 / ROWB) : 1;   // rows per 256 B (one sweep over the 64 LDS banks)
    constexpr int SWZ = (SL >= 16) ? 15 : (SL - 1);        // slot' = slot ^ ((row / RPB) & SWZ): 16 consecutive rows never collide
    constexpr int TILEB = TI * ROWB;
    constexpr int NPC = (TI * SL + NT - 1) / NT;  // 16-byte pieces per thread per tile
    constexpr int NKS = FP / 16;                // MFMA k-steps
    constexpr int UPB = NW * UB * 32;             // UB = 32-user column blocks per wave (2; 1 for FP = 256: register budget)
    const TopkParams& p = sp.t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tiles = smem;                                              // [2][NSUB][TILEB]: NSUB 64-item tiles per barrier
    float* Bs = reinterpret_cast<float*>(smem + 2 * NSUB * TILEB);   // [4][NSUB][TI] bias, -inf past the end of the catalogue

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, col = lane & 31;
    const int F = p.F;
    const int64_t I = p.I_local;
    const int64_t ublock = p.u_start + (int64_t)blockIdx.x * UPB + wave * (UB * 32);

    // ---- resident user fragments (bf16) ------------------------------------------------------------------------------
    bf16x8 bfr[UB][NKS];
    bool uvalid[UB];
    float thr[UB];
    int ucnt[UB], lcap[UB];
    int64_t lbase[UB];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
        thr[ub] = INFINITY;
        ucnt[ub] = lcap[ub] = 0;
        lbase[ub] = 0;
    }
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
        const int64_t user = ublock + ub * 32 + col;
        uvalid[ub] = user < p.u_stop;
        const float* gu = p.Gu + (uvalid[ub] ? user : p.u_start) * (int64_t)F;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int k0 = ks * 16 + hi * 8;
            union {
                u32 w[4];
                bf16x8 v;
            } pk;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ka = k0 + 2 * j, kb = ka + 1;
                const float a = (uvalid[ub] && ka < F) ? gu[ka] : 0.f;
                const float b = (uvalid[ub] && kb < F) ? gu[kb] : 0.f;
                pk.w[j] = el_f2bf(a) | (el_f2bf(b) << 16);
            }
            bfr[ub][ks] = pk.v;
        }
        if (MODE == 2 && uvalid[ub]) {
            const int64_t ur = user - p.u_start;
            thr[ub] = sp.thr[ur];
            int64_t nz = 0, zoff = 0;
            if (p.excl_indptr) {
                const int64_t z0 = p.excl_indptr[user];
                nz = p.excl_indptr[user + 1] - z0;
                zoff = z0 - p.excl_indptr[p.u_start];
            }
            lbase[ub] = ur * sp.surv + zoff;
            int64_t cap = sp.surv + nz;
            if (lbase[ub] + cap > sp.list_cap) cap = sp.list_cap - lbase[ub];     // undersized workspace: flag, never write OOB
            lcap[ub] = (int)(cap < 0 ? 0 : (cap > 0x3fffffff ? 0x3fffffff : cap));
        }
    }
    floatx16 mx[UB][2];
    if (MODE == 1) {
#pragma unroll
        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx[ub][ib][r] = -INFINITY;
    }

    // ---- item tile staging -------------------------------------------------------------------------------------------
    const int ntiles = (int)((I + TI - 1) / TI);
    const int step = (MODE == 1) ? sp.stride : 1;
    const int nv = (ntiles + step - 1) / step;              // tiles this pass visits: 0, step, 2 step, ...
    const int ng = (nv + NSUB - 1) / NSUB;                  // staged groups of NSUB visited tiles
    // The bf16 item tiles go from the image to LDS by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write;
    // round 1 staged them through 32 VGPRs).  The LDS side of a DMA is lane-linear (wave-uniform base + lane * 16 bytes), so the
    // XOR swizzle is applied to the SOURCE slot: the lane that lands at position `pos` of row r fetches slot pos ^ key(r).
    // Rows past the end of the catalogue read 16 bytes of zeros.  gload(x) is issued right after the barrier that retires
    // group x - 2 (its buffer is free), the barrier at the end of group x - 1 (vmcnt(0) + s_barrier) sees it landed.
    float pre_bias[NSUB];
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto gload = [&](int g) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int64_t tile = (int64_t)(g * NSUB + sub) * step;
            char* tbase = tiles + ((g & 1) * NSUB + sub) * TILEB;
#pragma unroll
            for (int q = 0; q < NPC; ++q) {
                const int i = q * NW + wave_u;                       // 1 KiB piece of the tile (wave-uniform)
                if (i * 64 < TI * SL) {
                    const int piece = i * 64 + lane;
                    const int r = piece / SL, pos = piece % SL;
                    const int64_t item = tile * TI + r;
                    const unsigned short* src = sp.Gib + item * FP + ((pos ^ ((r / RPB) & SWZ)) * 8);
                    if (!(item < I)) src = reinterpret_cast<const unsigned short*>(sp.zeros);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(tbase + i * 1024), 16, 0, 0);
                }
            }
            pre_bias[sub] = 0.f;
            if (tid < TI) {
                const int64_t item = tile * TI + tid;
                pre_bias[sub] = (item < I) ? (p.Bi ? p.Bi[item] : 0.f) : -INFINITY;
            }
        }
    };
    auto lstore = [&](int g) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            if (tid < TI) Bs[((g & 3) * NSUB + sub) * TI + tid] = pre_bias[sub];
        }
    };

    floatx16 acc[UB][2];
    // 2 x NKS MFMAs of item row block ib of sub-tile `sub` of staged group g
    auto mfma_half = [&](int g, int sub, int ib) {
        // bias of this lane's 16 accumulator rows: rows ib*32 + 8q + 4hi + {0..3} are r = 4q..4q+3
        const float* bb = Bs + ((g & 3) * NSUB + sub) * TI + ib * 32 + 4 * hi;
        floatx16 b16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const floatx4 v = *reinterpret_cast<const floatx4*>(bb + 8 * q);
            b16[4 * q + 0] = v[0];
            b16[4 * q + 1] = v[1];
            b16[4 * q + 2] = v[2];
            b16[4 * q + 3] = v[3];
        }
        const int row = ib * 32 + col;
        const char* rb = tiles + ((g & 1) * NSUB + sub) * TILEB + row * ROWB;
        const int key = (row / RPB) & SWZ;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(rb + (((ks * 2 + hi) ^ key) << 4));
#pragma unroll
            for (int ub = 0; ub < UB; ++ub)
                acc[ub][ib] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bfr[ub][ks], ks == 0 ? b16 : acc[ub][ib], 0, 0, 0);
        }
    };

    unsigned long long pn_enter = 0, pn_hits = 0, pn_blocks = 0;
    // epilogue of item row block ib of tile `tile` (scores in acc[.][ib])
    auto epi_half = [&](int tile, int ib) {
        if (PROF) pn_blocks += UB;
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const floatx16& sc = acc[ub][ib];                          // s' (a padded row carries -inf)
            if (MODE == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mx[ub][ib][r] = el_vmax(mx[ub][ib][r], sc[r]);
            } else {
                float m = el_vmax(sc[0], sc[1]);
#pragma unroll
                for (int r = 2; r < 16; r += 2) m = el_vmax3(m, sc[r], sc[r + 1]);
                if (__ballot(m >= thr[ub]) != 0ull) {
                    // rare: one RECORD per lane with a hit = (tile, row block, lane half, 16-bit mask of the rows that reach
                    // the threshold); k_screen_final expands it.  Lanes l and l+32 share the user's list counter.
                    if (PROF) pn_enter += 1;
                    u32 hm = 0u;
#pragma unroll
                    for (int r = 15; r >= 0; --r) hm = (hm << 1) | ((sc[r] >= thr[ub]) ? 1u : 0u);
                    const bool pend = hm != 0u;
                    const u32 pv = el_partner32(pend ? 1u : 0u, hi);
                    const int pos = ucnt[ub] + (hi ? (int)pv : 0);
                    if (pend && pos < lcap[ub]) {
                        sp.lists[lbase[ub] + pos] = ((u64)(u32)tile << 18) | ((u64)ib << 17) | ((u64)hi << 16) | (u64)hm;
                        sp.lsc[lbase[ub] + pos] = m;
                    }
                    ucnt[ub] += (pend ? 1 : 0) + (int)pv;
                    if (PROF) pn_hits += __popcll(__ballot(pend));
                }
            }
        }
    };

    const unsigned long long pt_begin = PROF_T();
    if (ng > 0) {
        gload(0);
        lstore(0);
        __syncthreads();
        if (1 < ng) gload(1);
        mfma_half(0, 0, 0);
    }
    for (int g = 0; g < ng; ++g) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int tile = (g * NSUB + sub) * step;            // (a tile past the end is all padding: bias -inf, no effect)
            mfma_half(g, sub, 1);
            epi_half(tile, 0);
            if (sub + 1 < NSUB) {
                mfma_half(g, sub + 1, 0);
                epi_half(tile, 1);
            }
        }
        if (g + 1 < ng) lstore(g + 1);
        __syncthreads();
        if (g + 2 < ng) gload(g + 2);
        mfma_half(g + 1, 0, 0);      // (past the last group this chews on a stale LDS slot; the result is never read)
        epi_half((g * NSUB + NSUB - 1) * step, 1);
    }

    if (MODE == 1) {
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int64_t user = ublock + ub * 32 + col;
            if (!uvalid[ub]) continue;
            float* o = sp.smax + (user - p.u_start) * SCR_TI + hi * 16;
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    floatx4 v;
                    v[0] = mx[ub][ib][4 * q + 0];
                    v[1] = mx[ub][ib][4 * q + 1];
                    v[2] = mx[ub][ib][4 * q + 2];
                    v[3] = mx[ub][ib][4 * q + 3];
                    *reinterpret_cast<floatx4*>(o + ib * 32 + 4 * q) = v;
                }
        }
    } else {
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int64_t user = ublock + ub * 32 + col;
            if (!uvalid[ub] || hi) continue;
            const int64_t ur = user - p.u_start;
            sp.cnt[ur] = ucnt[ub] < lcap[ub] ? ucnt[ub] : lcap[ub];
            if (ucnt[ub] > lcap[ub]) sp.ovf[ur] = 1;
        }
    }
    if (PROF && lane == 0) {
        unsigned long long* o = sp.prof + ((int64_t)blockIdx.x * NW + wave) * 8;
        o[0] = PROF_T() - pt_begin;
        o[1] = 0;
        o[2] = 0;
        o[3] = 0;
        o[4] = 0;
        o[5] = pn_blocks;
        o[6] = pn_enter;
        o[7] = pn_hits;
    }
}

// ---- per-user threshold from the slot maxima ---------------------------------------------------------------------
// One wave per user.  A masked item j contaminates its slot when it may be the slot's arg-max: its s' is recomputed
// here (same bf16 operands, fp32 fma chain) and compared with the slot maximum with the fp32 re-association tolerance.
// (If it is NOT flagged, the arg-max is another item, and that item is unmasked or it would have flagged the slot.)
// (occupancy knobs of the two latency-bound per-user kernels; -D overrides are for A/B builds, scripts/exp/build_variants.sh)
#ifndef EL_SCR_WPE
#define EL_SCR_WPE 6                 // 6 waves per SIMD (<= 80 VGPRs, 24 KB of LDS per workgroup): thr 0.357 -> 0.306 ms, final 1.25 -> 1.15 ms
#endif                               // per 131 072-user block on trained tables (gpurun_out r03c; 7 and 8 spill and lose it again)
#if EL_SCR_WPE > 0
#define SCR_LB __launch_bounds__(256, EL_SCR_WPE)
#else
#define SCR_LB __launch_bounds__(256)
#endif
#ifndef EL_SCR_XC
#define EL_SCR_XC 256
#endif
#ifndef EL_SCR_GUS
#define EL_SCR_GUS 256
#endif

template <int FP>
__global__ SCR_LB void k_screen_thr(ScreenParams sp) {
    const TopkParams& p = sp.t;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ur = (int64_t)blockIdx.x * 4 + wv, user = p.u_start + ur;     // one wave per user, 4 users per workgroup
    if (user >= p.u_stop) return;
    __shared__ float sm_[4][SCR_TI];
    __shared__ int inv_[4][SCR_TI];
    __shared__ __attribute__((aligned(16))) float ubf_[4][FP];
    __shared__ u64 keys_[4][SCR_TI];
    __shared__ int pos_of_[4][SCR_TI];
    int* pos_of = pos_of_[wv];
    float* sm = sm_[wv];
    int* inv = inv_[wv];
    float* ubf = ubf_[wv];
    u64* keys = keys_[wv];
    const float M = sp.smax[ur * SCR_TI + lane];
    sm[lane] = M;
    inv[lane] = 0;
    const float* gu = p.Gu + user * (int64_t)p.F;
    float ss = 0.f, sd = 0.f, amax = 0.f;
    for (int f = lane; f < FP; f += 64) amax = fmaxf(amax, (f < p.F) ? fabsf(gu[f]) : 0.f);
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float rs = amax > 0.f ? 1.0f / amax : 0.f;      // scale-safe norms: see k_screen_prep
    for (int f = lane; f < FP; f += 64) {
        const float v = (f < p.F) ? gu[f] : 0.f;
        const float r = el_bf2f(el_f2bf(v)), d = v - r;
        ubf[f] = r;
        const float vs = v * rs, ds = d * rs;
        ss += vs * vs;
        sd += ds * ds;
    }
    ss = el_group_sum(ss, 64);
    sd = el_group_sum(sd, 64);
    float nu = amax * sqrtf(ss) * 1.001f;
    if (!(nu < INFINITY)) nu = INFINITY;
    float du = amax * sqrtf(sd) * 1.001f;
    if (!(du < INFINITY)) du = INFINITY;                  // inf / NaN user row: the bound is infinite, the user falls back
    float E, tol;
    el_screen_bounds(nu, du, sp.stats[0], sp.stats[SCR_STAT_IB], sp.stats[SCR_STAT_ID], sp.stats[1], p.F, E, tol);
    // slots by descending maximum; only the slots near the top can decide T, so the masked items of the best k + 8 slots
    // are scored first and the rest only if those did not yield k clean slots (the rows are the kernel's HBM traffic)
    const bool fin = (M > -INFINITY) && (M < INFINITY);
    pos_of[lane] = -1;
    keys[lane] = fin ? el_make_key(M, lane) : 0ull;
    el_wave_lds_sync();
    el_wave_bitonic_desc(keys, SCR_TI, lane);
    const u64 mykey = keys[lane];
    const int myslot = mykey ? el_key_item(mykey) : 0;
    if (mykey) pos_of[myslot] = lane;
    el_wave_lds_sync();
    int64_t e0 = 0, e1 = 0;
    if (p.excl_indptr) {
        e0 = p.excl_indptr[user];
        e1 = p.excl_indptr[user + 1];
    }
    const int kA = sp.kA;
    int R = kA + 8 < SCR_TI ? kA + 8 : SCR_TI;
    bool good = false;
    float T = 0.f, D = INFINITY;
    for (int lo = 0; lo < SCR_TI && !good; lo = R, R = SCR_TI) {
        // one lane per masked item, 64 in flight: index (coalesced) -> slot -> is the slot in this round? -> bf16 row dot
        for (int64_t eb = e0; eb < e1; eb += 64) {
            const int64_t e = eb + lane;
            int64_t il = -1;
            int slot = 0;
            if (e < e1) {
                il = (int64_t)p.excl_indices[e] - p.item_offset;
                if (il < 0 || il >= p.I_local || ((il >> 6) % sp.stride) != 0) il = -1;   // other shard / tile not visited by pass 1
                if (il >= 0) {
                    slot = el_screen_slot((int)(il & 63));
                    const int ps = pos_of[slot];
                    if (ps < lo || ps >= R) il = -1;                                      // slot not in this round
                }
            }
            if (il >= 0) {
                const uint4* row = reinterpret_cast<const uint4*>(sp.Gib + il * FP);
                float a = 0.f;
#pragma unroll 4
                for (int c = 0; c < FP / 8; ++c) {
                    const uint4 v = row[c];
                    const float* uu = ubf + c * 8;
                    a = __builtin_fmaf(el_bf2f(v.x & 0xffffu), uu[0], a);
                    a = __builtin_fmaf(el_bf2f(v.x >> 16), uu[1], a);
                    a = __builtin_fmaf(el_bf2f(v.y & 0xffffu), uu[2], a);
                    a = __builtin_fmaf(el_bf2f(v.y >> 16), uu[3], a);
                    a = __builtin_fmaf(el_bf2f(v.z & 0xffffu), uu[4], a);
                    a = __builtin_fmaf(el_bf2f(v.z >> 16), uu[5], a);
                    a = __builtin_fmaf(el_bf2f(v.w & 0xffffu), uu[6], a);
                    a = __builtin_fmaf(el_bf2f(v.w >> 16), uu[7], a);
                }
                const float sc = a + (p.Bi ? p.Bi[il] : 0.f);
                if (!(sc < sm[slot] - tol)) inv[slot] = 1;               // NaN lands here too (conservative)
            }
        }
        el_wave_lds_sync();
        u64 clean = __ballot(mykey != 0ull && lane < R && inv[myslot] == 0);   // bit j: the j-th best slot is clean
        if (__popcll(clean) >= kA) {
            for (int q = 1; q < kA; ++q) clean &= clean - 1ull;
            T = el_key_score(keys[__ffsll((long long)clean) - 1]);
            good = true;
            // how far the guess may sit above the true k-th score is a matter of RANKS (the sample's kA-th maximum lands a few
            // ranks either side of its target), so the slack under it is sized by the local spacing of the top scores: D = the
            // drop over the next four clean slot maxima (~ 4 x stride ranks of the catalogue)
            u64 c3 = clean;
            for (int q = 0; q < 4; ++q) c3 &= c3 - 1ull;
            D = c3 ? T - el_key_score(keys[__ffsll((long long)c3) - 1]) : INFINITY;
        }
    }
    if (lane == 0) {
        good = good && (E < INFINITY);
        // thr = T - b E.  Every item outside the candidate list has s' < thr, hence an exact score < thr + E =: V, and
        // k_screen_final accepts the user iff its k-th exact score reaches V (the exact fallback takes the others).  b = 2 (V = T - E)
        // can never reject a RIGOROUS T.  A guessed T is aimed well below the k-th score (rank ~5 k of the catalogue), so the part of
        // the band beyond E -- slack for the guess -- is mostly unused, and E, a worst-case bound, is ~50 ranks wide at the top of a
        // trained table: b = 2 collects 212 records per user there, b = 0.75 (V = T + E / 4) 127 and still rejects nobody (4.76 ->
        // 4.22 ms per block).  On fresh tables E is a rank or two wide and V moves with it: 11 users of 131 072 rejected at b = 2 or
        // 1.5, 39 at 1, 86 at 0.75 (each costs the fallback ~5 us; b = 1.5 is the fastest there).  The regime shows in the data:
        // r = D / E, the drop over four slot maxima in units of E, is ~0.6 on the trained tables and >> 1 on fresh ones:
        // b = clamp(0.5 + 0.4 r, band_min, band) with band_min = 1 (V = T: the k-th exact score has to reach the guess itself;
        // 0.75 already sends a hundred users of the bench's lightly trained tables to the fallback: 4.49 against 4.26 ms).
        float bnd = sp.band;
        if (sp.band_min < sp.band && E > 0.f && D < INFINITY) bnd = fminf(sp.band, fmaxf(sp.band_min, 0.5f + 0.4f * (D / E)));
        sp.thr[ur] = good ? (T - bnd * E) : INFINITY;
        sp.Tg[ur] = T - (bnd - 1.0f) * E;                       // V
        sp.Eu[ur] = E;
        sp.nuv[ur] = nu;
        sp.duv[ur] = du;
        sp.ovf[ur] = good ? 0 : 1;
        sp.cnt[ur] = 0;
    }
}

// ---- exact re-scoring of the survivors + write-out -------------------------------------------------------------------
// exact fp32 score (fma chain over f = 0..F-1 from +0, + bias, + 0.0f); gu_s = the user's row staged in LDS.
// The item row is read 8 x 16 B at a time so that eight requests are in flight instead of one.
__device__ __forceinline__ float el_exact_score(const TopkParams& p, const float* gu_s, int64_t il, bool vec4) {
    const float* gi = p.Gi + il * (int64_t)p.F;
    float a = 0.f;
    int f = 0;
    if (vec4) {
        const float4* gi4 = reinterpret_cast<const float4*>(gi);
        for (; f + 32 <= p.F; f += 32) {
            float4 x[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) x[c] = gi4[(f >> 2) + c];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float4 y = *reinterpret_cast<const float4*>(gu_s + f + 4 * c);
                a = __builtin_fmaf(x[c].x, y.x, a);
                a = __builtin_fmaf(x[c].y, y.y, a);
                a = __builtin_fmaf(x[c].z, y.z, a);
                a = __builtin_fmaf(x[c].w, y.w, a);
            }
        }
        for (; f + 4 <= p.F; f += 4) {
            const float4 x = gi4[f >> 2];
            const float4 y = *reinterpret_cast<const float4*>(gu_s + f);
            a = __builtin_fmaf(x.x, y.x, a);
            a = __builtin_fmaf(x.y, y.y, a);
            a = __builtin_fmaf(x.z, y.z, a);
            a = __builtin_fmaf(x.w, y.w, a);
        }
    }
    for (; f < p.F; ++f) a = __builtin_fmaf(gi[f], gu_s[f], a);
    return (p.Bi ? a + p.Bi[il] : a) + 0.0f;
}

template <int SCR_SURV>
__global__ SCR_LB void k_screen_final(ScreenParams sp) {
    const TopkParams& p = sp.t;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ur = (int64_t)blockIdx.x * 4 + wv, user = p.u_start + ur;     // one wave per user, 4 users per workgroup
    if (user >= p.u_stop || sp.ovf[ur]) return;
    constexpr int XC = EL_SCR_XC;                    // exclusion rows up to this length are searched in LDS
    __shared__ u64 surv_[4][SCR_SURV];
    __shared__ int32_t xrow_[4][XC];
    __shared__ __attribute__((aligned(16))) float gus_[4][EL_SCR_GUS];   // F <= 256 (eligibility)
    u64* surv = surv_[wv];
    int32_t* xrow = xrow_[wv];
    float* gu_s = gus_[wv];
    const bool prf = sp.prof2 != nullptr;
    unsigned long long tp0 = prf ? __builtin_amdgcn_s_memtime() : 0ull, tp1 = 0, tp2 = 0, tp3 = 0;
    int pf_ns0 = 0, pf_ns1 = 0;
    for (int f = lane; f < p.F; f += 64) gu_s[f] = p.Gu[user * (int64_t)p.F + f];
    const int n = sp.cnt[ur];
    int64_t e0 = 0, e1 = 0, zoff = 0;
    if (p.excl_indptr) {
        e0 = p.excl_indptr[user];
        e1 = p.excl_indptr[user + 1];
        zoff = e0 - p.excl_indptr[p.u_start];
    }
    const u64* list = sp.lists + ur * SCR_SURV + zoff;
    const float* lsc = sp.lsc + ur * SCR_SURV + zoff;
    for (int t = lane; t < SCR_SURV; t += 64) surv[t] = 0ull;
    const int nx = (int)(e1 - e0);
    const bool xl = nx <= XC;
    if (xl)
        for (int t = lane; t < nx; t += 64) xrow[t] = p.excl_indices[e0 + t];
    el_wave_lds_sync();
    // ---- records -> unmasked candidates, keyed by s' (known exactly when the record holds one item, else +inf) ----------
    int ns = 0, nunk = 0;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        const u64 rec = (t < n) ? list[t] : 0ull;
        u32 hm = (u32)(rec & 0xffffu);
        const float sc = (t < n && __popc(hm) == 1) ? lsc[t] : INFINITY;
        const int64_t row0 = (int64_t)(rec >> 18) * SCR_TI + (int64_t)((rec >> 17) & 1u) * 32 + 4 * (int)((rec >> 16) & 1u);
        while (__ballot(hm != 0u) != 0ull) {
            bool keep = false;
            int32_t g = 0;
            if (hm != 0u) {
                const int r = __ffs((int)hm) - 1;
                hm &= hm - 1u;
                g = (int32_t)(p.item_offset + row0 + (r & 3) + 8 * (r >> 2));
                if (xl) {                                // lower bound in the LDS copy
                    int a = 0, bnd = nx;
                    while (a < bnd) {
                        const int mid = (a + bnd) >> 1;
                        if (xrow[mid] < g)
                            a = mid + 1;
                        else
                            bnd = mid;
                    }
                    keep = !(a < nx && xrow[a] == g);
                } else {
                    keep = !el_row_contains(p.excl_indices, e0, e1, g);
                }
            }
            const u64 b = __ballot(keep);
            const int pos = ns + __popcll(b & ((1ull << lane) - 1ull));
            if (keep && pos < SCR_SURV) surv[pos] = el_make_key(sc, g);
            ns += __popcll(b);
            nunk += __popcll(__ballot(keep && !(sc < INFINITY)));
        }
    }
    el_wave_lds_sync();
    if (prf) tp1 = __builtin_amdgcn_s_memtime();
    pf_ns0 = ns;
    if (ns > SCR_SURV || ns < p.k) {                 // window overflow / cannot happen unless flagged: exact fallback
        if (lane == 0) sp.ovf[ur] = 1;
        return;
    }
    // ---- second-level screen with PER-ITEM error radii.  For a candidate j whose s' is known, the exact score lies in
    // [s'_j - e_j, s'_j + e_j], e_j = ||du|| ||bf16(i_j)|| + ||u|| ||i_j - bf16(i_j)|| + tol (the Cauchy-Schwarz bound of the header with
    // THIS item's measured norms, k_screen_prep, instead of the maxima over the shard -- in a trained table a few popular items carry
    // norms several times the typical one, and E_u is sized for them).  With L = the k-th largest lower bound, k candidates have an
    // exact score >= L, so a candidate whose upper bound is below L is not in the top-k.  Candidates of unknown s' (records with
    // several rows) have no lower bound and always stay.  Round 2 cut at (k-th largest s') - 2 E_u: ~2x as many exact re-scorings,
    // i.e. random 4F-byte row reads, the bulk of this kernel's time on trained tables.
    {
        constexpr int NQ = SCR_SURV / 64;
        u64 mk[NQ];
        float ubd[NQ];
        const float nu = sp.nuv[ur], du = sp.duv[ur];
        float E_, tol;
        el_screen_bounds(nu, du, sp.stats[0], sp.stats[SCR_STAT_IB], sp.stats[SCR_STAT_ID], sp.stats[1], p.F, E_, tol);
        int n2 = 64;
        while (n2 < ns) n2 <<= 1;
        u64 lbk[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int t = q * 64 + lane;
            mk[q] = 0ull;
            ubd[q] = -INFINITY;
            lbk[q] = 0ull;
            if (q * 64 < ns && t < ns) {
                const u64 key = surv[t];
                mk[q] = key;
                const float s1 = el_key_score(key);
                if (s1 < INFINITY) {
                    const int32_t g = el_key_item(key);
                    const float2 nn = sp.inorm[(int64_t)g - p.item_offset];
                    const float e = du * nn.x + nu * nn.y + tol;
                    ubd[q] = s1 + e;
                    lbk[q] = el_make_key(s1 - e, g);
                } else {
                    ubd[q] = INFINITY;
                }
            }
        }
        el_wave_lds_sync();
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q * 64 < n2) surv[q * 64 + lane] = lbk[q];
        el_wave_lds_sync();
        el_wave_bitonic_desc(surv, n2, lane);
        const float L = (ns - nunk >= p.k) ? el_key_score(surv[p.k - 1]) : -INFINITY;
        el_wave_lds_sync();
        int ns2 = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (q * 64 < ns) {
                const bool kp = (q * 64 + lane < ns) && (ubd[q] >= L);
                const u64 b = __ballot(kp);
                const int pos = ns2 + __popcll(b & ((1ull << lane) - 1ull));
                if (kp) surv[pos] = mk[q];
                ns2 += __popcll(b);
            }
        }
        el_wave_lds_sync();
        ns = ns2;
    }
    if (prf) tp2 = __builtin_amdgcn_s_memtime();
    pf_ns1 = ns;
    const bool vec4 = (p.F % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.Gi) & 15) == 0);
    u64 nk[SCR_SURV / 64];
#pragma unroll
    for (int q = 0; q < SCR_SURV / 64; ++q) {
        const int t = q * 64 + lane;
        nk[q] = 0ull;
        if (q * 64 < ns && t < ns) {
            const int32_t g = el_key_item(surv[t]);
            const float s = el_exact_score(p, gu_s, (int64_t)g - p.item_offset, vec4);
            if (s == s) nk[q] = el_make_key(s, g);
        }
    }
    el_wave_lds_sync();
    if (prf) tp3 = __builtin_amdgcn_s_memtime();
#pragma unroll
    for (int q = 0; q < SCR_SURV / 64; ++q) surv[q * 64 + lane] = nk[q];
    el_wave_lds_sync();
    int n2 = 64;
    while (n2 < ns) n2 <<= 1;
    el_wave_bitonic_desc(surv, n2, lane);                           // keys beyond ns are 0 and sort last
    int nv = 0;
#pragma unroll
    for (int q = 0; q < SCR_SURV / 64; ++q) nv += __popcll(__ballot(surv[q * 64 + lane] != 0ull));
    if (nv < p.k) {                                  // exact score NaN where the screen was finite: let the fallback decide
        if (lane == 0) sp.ovf[ur] = 1;
        return;
    }
    // the threshold was a guess unless pass 1 saw every tile (kA == k): it was good enough iff k survivors have an exact
    // score >= V = thr + E, because every item that is NOT a survivor has s' < thr, hence an exact score < thr + E
    if (!(el_key_score(surv[p.k - 1]) >= sp.Tg[ur])) {            // Tg = V = thr + E (k_screen_thr)
        if (lane == 0) sp.ovf[ur] = 1;
        return;
    }
    const int64_t orow = ur * (int64_t)p.k;
    for (int t = lane; t < p.k; t += 64) {
        const u64 kk = surv[t];
        p.out_idx[orow + t] = el_key_item(kk);
        p.out_val[orow + t] = el_key_score(kk);
    }
    if (prf && lane == 0) {
        const unsigned long long tp4 = __builtin_amdgcn_s_memtime();
        atomicAdd(sp.prof2 + 0, 1ull);
        atomicAdd(sp.prof2 + 1, tp1 - tp0);          // records -> unmasked candidates
        atomicAdd(sp.prof2 + 2, tp2 - tp1);          // second-level screen
        atomicAdd(sp.prof2 + 3, tp3 - tp2);          // exact re-scoring
        atomicAdd(sp.prof2 + 4, tp4 - tp3);          // sort, verify, write
        atomicAdd(sp.prof2 + 5, (unsigned long long)n);
        atomicAdd(sp.prof2 + 6, (unsigned long long)pf_ns0);
        atomicAdd(sp.prof2 + 7, (unsigned long long)pf_ns1);
    }
}

// flagged users -> list for the fp32 MFMA kernel (order is irrelevant: rows are independent)
__global__ __launch_bounds__(256) void k_screen_flags(ScreenParams sp, int64_t n_users) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u < n_users && sp.ovf[u]) sp.ulist[atomicAdd(sp.ulist_n, 1)] = (int32_t)u;
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int screen_fp(int F) { return F <= 32 ? 32 : (F <= 64 ? 64 : (F <= 128 ? 128 : 256)); }

bool el_topk_screen_eligible(int F, int k, const void* cand) { return cand == nullptr && F >= 1 && F <= 256 && k >= 1 && k <= 128; }

// How the threshold T is obtained (see the header comment and DESIGN.md 3.1b):
//   small catalogue (< 192 tiles), k <= 12   pass 1 over every tile, T = k-th largest clean slot maximum: rigorous
//   k <= 12                                   a full pass 1 is half of the run time: every 4th (8th from 300 K items) tile, a GUESS
//   k  > 12                                   64 slots cannot yield k clean maxima: every stride-th tile (2..8), a GUESS
// A guess is the kA-th largest clean slot maximum of the sample, aimed at rank ~1.15 k (+ margin) of the catalogue;
// k_screen_final verifies it per user (exact fallback otherwise).  surv = unmasked hits a user may have.
struct ScreenPolicy {
    int stride, kA, surv;
    float band, band_min;
};

static ScreenPolicy screen_policy(int k, int64_t I_local) {
    const int ntiles = (int)((I_local + SCR_TI - 1) / SCR_TI);
    ScreenPolicy q;
    q.stride = 1;
    q.kA = k;
    q.surv = 128;
    q.band = q.band_min = 2.0f;
    if (k <= 12) {
        // every 8th tile from 60 K items (round 2: at I = 100 K pass 1 drops 0.66 -> 0.36 ms and the sample of 12.5 K items still
        // gives a usable guess: 4.52 -> 4.24 ms per 131 072-user block, nobody falls back; scripts/screen_sweep.sh), every 4th
        // for smaller catalogues of at least 192 tiles, every 16th from 500 K items (I = 1 M: pass 1 3.04 -> 1.54 ms of a 28.9 ms
        // block, the 62 K-item sample guesses as well as 12.5 K of 100 K do: 4.54 -> 4.77 M users/s, nobody falls back)
        const int sd = I_local >= 500000 ? 16 : (I_local >= 60000 ? 8 : (ntiles >= 192 ? 4 : 1));
        if (sd > 1) {
            q.stride = sd;
            q.kA = (int)((1.15 * k) / sd + 0.999) + (sd >= 8 ? 4 : 5);   // (+3 under the round-1 bound; the measured-residual bound verifies
            // the guess against a 3x narrower margin, so it is aimed one slot lower: 209 -> 19 fallback users per block on untrained weights)
        }
    } else {
        int sd = (int)(1.15 * k / 24.0 + 0.5);                  // kA ~ 20-30 of the 64 slots: a 1/sd sample has rank sd(kA + 1/2)
        sd = sd < 2 ? 2 : (sd > 8 ? 8 : sd);                    //   +- sd sqrt(kA (1 - 1/sd)) in the catalogue
        while (sd > 1 && ntiles < 48 * sd) --sd;                // small catalogues: sample more of it
        q.stride = sd;
        q.kA = (int)((1.15 * k) / sd + 0.999) + 2;
        if (q.kA > 40) q.kA = 40;                               // (tiny catalogues: the verification decides)
        q.surv = 512;
    }
    if (g_el_cur_ctx) {                                         // el_ctx_set_option("screen_stride" / "screen_ka"): the tests force guesses that fail
        const int sv = (int)g_el_cur_ctx->opt.screen_stride, kv = (int)g_el_cur_ctx->opt.screen_ka;
        if (sv >= 1 && sv <= 16) q.stride = sv;
        if (kv >= 1 && kv <= 56) q.kA = kv;
    }
    if (q.stride > 1 || q.kA != k) {
        q.surv = 512;
        q.band = 1.5f, q.band_min = 1.0f;                       // a guessed T: the band follows the spacing of the top scores (k_screen_thr)
    }
    return q;
}

struct ScreenWs {
    unsigned short* gib;       // ScreenParams::Gib and ::stats, writable
    float* stats;
    TopkListWs fb;             // scratch of the exact fallback (el_topk_run_list)
};

// The workspace of a screened call.  The item side comes first: its place does not depend on n_users, so the image survives
// from block to block (EL_TOPK_ITEMS_UNCHANGED).  The record lists come last: sp->lists is where they start, the caller
// shares whatever its workspace holds behind that between lists and lsc.
static size_t screen_carve(int64_t n_users, int64_t I_local, int F, int k, int64_t excl_nnz, void* base, ScreenParams* sp, ScreenWs* w) {
    const size_t nu = (size_t)n_users;
    ElCarve c{(char*)base};
    sp->Gib = w->gib = c.take<unsigned short>((size_t)I_local * screen_fp(F));
    sp->inorm = c.take<float2>((size_t)I_local);
    sp->stats = w->stats = c.take<float>(4);
    sp->smax = c.take<float>(nu * SCR_TI);
    sp->thr = c.take<float>(nu);
    sp->cnt = c.take<int32_t>(nu);
    sp->ovf = c.take<int32_t>(nu);
    sp->ulist = c.take<int32_t>(nu);
    sp->Tg = c.take<float>(nu);
    sp->Eu = c.take<float>(nu);
    sp->nuv = c.take<float>(nu);
    sp->duv = c.take<float>(nu);
    w->fb = el_topk_list_carve(c, n_users, I_local, k);
    sp->lists = (u64*)c.take<char>((nu * screen_policy(k, I_local).surv + (size_t)excl_nnz) * 12);     // surv * U + nnz records of 8 + 4 bytes
    return c.off;
}

size_t el_topk_screen_ws_bytes(int64_t n_users, int64_t I_local, int F, int k, int64_t excl_nnz) {
    ScreenParams sp;
    ScreenWs w;
    return screen_carve(n_users, I_local, F, k, excl_nnz < 0 ? 0 : excl_nnz, nullptr, &sp, &w);
}

template <int FP, int MODE, int NW, bool PROF>
static int launch_pass(const ScreenParams& sp, hipStream_t st) {
    constexpr int NSUB = (MODE == 2 && FP <= 128) ? 4 : 1;   // pass 2: four tiles per barrier average out the record path (-10 %)
    constexpr int UB = FP <= 128 ? 2 : 1;                    // FP = 256: the resident user fragments allow 32 users per wave
    constexpr size_t lds = (size_t)NSUB * (2 * SCR_TI * FP * 2 + 4 * SCR_TI * 4);
    auto kern = k_screen_pass<FP, MODE, NW, NSUB, UB, PROF>;
    if (lds > 65536) EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t n_users = sp.t.u_stop - sp.t.u_start;
    constexpr int UPB = NW * UB * 32;
    const int64_t n_wg = (n_users + UPB - 1) / UPB;
    // (Pace keeping of the workgroups that share an XCD's L2 -- progress counters + bounded naps so that they sweep the item image
    //  within ~2 MB of each other -- was measured in round 5 and removed in round 6: 26.1 against 25.9 ms per pass-2 launch at
    //  131 072 users x 1 M x 128, FETCH_SIZE unchanged at the 5 M x 256 shard: the pass is not bound by where its tiles come from.)
    const ScreenParams& q = sp;
    EL_LAUNCH(MODE == 1 ? "k_screen_pass1" : "k_screen_pass2", kern, dim3((unsigned)n_wg), dim3(NW * 64), lds, st, q);
    EL_CHECK_LAUNCH();
    return 0;
}

template <int FP, int NW, bool PROF>
static int run_passes(ScreenParams& sp, hipStream_t st) {
    const int64_t n_users = sp.t.u_stop - sp.t.u_start;
    constexpr int UPB_ = NW * (FP <= 128 ? 2 : 1) * 32;
    const int64_t nw = ((n_users + UPB_ - 1) / UPB_) * NW;
    unsigned long long* h = nullptr;
    if (PROF) {
        EL_CHECK_HIP(hipMalloc((void**)&sp.prof, (size_t)nw * 64));
        h = (unsigned long long*)malloc((size_t)nw * 64);
    }
    auto report = [&](const char* name) -> int {
        EL_CHECK_HIP(hipStreamSynchronize(st));
        EL_CHECK_HIP(hipMemcpy(h, sp.prof, (size_t)nw * 64, hipMemcpyDeviceToHost));
        double a[8] = {0};
        for (int64_t w = 0; w < nw; ++w)
            for (int q = 0; q < 8; ++q) a[q] += (double)h[w * 8 + q] / (double)nw;
        fprintf(stderr, "[screen prof] %s per wave: %.0f cycles | blocks %.0f entered %.0f hits %.0f\n", name, a[0], a[5], a[6], a[7]);
        return 0;
    };
    if (int rc = launch_pass<FP, 1, NW, PROF>(sp, st)) return rc;
    if (PROF) report("pass1");
    auto kthr = k_screen_thr<FP>;
    EL_LAUNCH("k_screen_thr", kthr, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, sp);
    if (int rc = launch_pass<FP, 2, NW, PROF>(sp, st)) return rc;
    if (PROF) {
        report("pass2");
        free(h);
        EL_CHECK_HIP(hipFree(sp.prof));
        sp.prof = nullptr;
        EL_CHECK_HIP(hipMalloc((void**)&sp.prof2, 16 * 8));
        EL_CHECK_HIP(hipMemsetAsync(sp.prof2, 0, 16 * 8, st));
    }
    if (sp.surv == 128)
        EL_LAUNCH("k_screen_final", k_screen_final<128>, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, sp);
    else
        EL_LAUNCH("k_screen_final", k_screen_final<512>, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, sp);
    EL_CHECK_LAUNCH();
    if (PROF) {
        unsigned long long a[16];
        EL_CHECK_HIP(hipStreamSynchronize(st));
        EL_CHECK_HIP(hipMemcpy(a, sp.prof2, sizeof(a), hipMemcpyDeviceToHost));
        EL_CHECK_HIP(hipFree(sp.prof2));
        sp.prof2 = nullptr;
        const double nu_ = a[0] ? (double)a[0] : 1.0;
        fprintf(stderr, "[screen prof] final per user (%llu users): expand %.0f | screen %.0f | rescore %.0f | sort+write %.0f cycles (100 MHz clock); "
                        "records %.1f -> unmasked %.1f -> after the second-level screen %.1f\n", a[0], a[1] / nu_, a[2] / nu_, a[3] / nu_, a[4] / nu_,
                a[5] / nu_, a[6] / nu_, a[7] / nu_);
    }
    return 0;
}

int el_topk_screen_run(const TopkParams& p, void* ws, size_t ws_bytes, hipStream_t st, bool items_unchanged) {
    const int64_t n_users = p.u_stop - p.u_start;
    if (n_users <= 0) return 0;
    const int FP = screen_fp(p.F);
    ScreenParams sp;
    ScreenWs w;
    const size_t fixed = screen_carve(n_users, p.I_local, p.F, p.k, 0, ws, &sp, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= fixed, "el_score_topk: screened top-k needs a workspace of el_score_topk_ws_bytes() bytes");
    sp.t = p;
    unsigned short* gib = w.gib;
    float* stats = w.stats;
    const ScreenPolicy pol = screen_policy(p.k, p.I_local);
    sp.surv = pol.surv;
    sp.stride = pol.stride;
    sp.zeros = g_el_cur_ctx->zeros;
    sp.kA = pol.kA;
    sp.band = pol.band;
    sp.band_min = pol.band_min;
    sp.ulist_n = (int32_t*)(stats + 2);
    sp.list_cap = (int64_t)(((char*)ws + ws_bytes - (char*)sp.lists) / 12) & ~(int64_t)31;   // whatever the caller provisioned for surv*U + nnz
    sp.lsc = (float*)((char*)sp.lists + (size_t)sp.list_cap * 8);
    sp.prof = nullptr;
    sp.prof2 = nullptr;
    // The item side (bf16 image, max norm, max |bias|) depends on Gi / Bi only.  A caller that scores block after block of
    // users against an unchanged table says so (EL_TOPK_ITEMS_UNCHANGED); the claim is honoured only if this context's
    // previous screened call used the same workspace, tables and shape.
    el_ctx* ctx = g_el_cur_ctx;
    const bool claim = items_unchanged && ctx->prep_ws == ws && ctx->prep_Gi == p.Gi && ctx->prep_Bi == p.Bi &&
                       ctx->prep_I == p.I_local && ctx->prep_F == p.F;
    ctx->prep_ws = ws, ctx->prep_Gi = p.Gi, ctx->prep_Bi = p.Bi, ctx->prep_I = p.I_local, ctx->prep_F = p.F;
    u64* ctl = reinterpret_cast<u64*>(reinterpret_cast<char*>(stats) + 32);     // inside the 256-byte control block
    EL_CHECK_HIP(hipMemsetAsync(stats + 2, 0, 8, st));                          // the flagged-user counter
    EL_CHECK_HIP(hipMemsetAsync(ctl + 1, 0, 8, st));                            // hash accumulator
    if (p.I_local > 0) {
        // the claim "items unchanged" is VERIFIED (in-place updates keep pointers and shapes): hash of the tables now against
        // the hash the image was built from; without the claim the image is rebuilt and its hash recorded
        const int64_t n_g = p.I_local * (int64_t)p.F;
        int64_t hb = (n_g / 4 + 255) / 256;
        const int64_t hcap = (int64_t)ctx->cus * 2;
        if (hb > hcap) hb = hcap;
        if (hb < 1) hb = 1;
        EL_LAUNCH("k_items_hash", k_items_hash, dim3((unsigned)hb), dim3(256), 0, st, p.Gi, p.Bi, n_g, p.I_local, ctl);
        EL_LAUNCH("k_items_decide", k_items_decide, dim3(1), dim3(1), 0, st, ctl, stats, claim ? 0 : 1);
        const unsigned long long* rebuild = reinterpret_cast<const unsigned long long*>(ctl + 2);
        const unsigned pg = (unsigned)((p.I_local * (FP / 8) + 255) / 256);
        if (FP == 32)
            EL_LAUNCH("k_screen_prep", k_screen_prep<32>, dim3(pg), dim3(256), 0, st, p.Gi, p.Bi, p.I_local, p.F, gib, stats, rebuild, sp.inorm);
        else if (FP == 64)
            EL_LAUNCH("k_screen_prep", k_screen_prep<64>, dim3(pg), dim3(256), 0, st, p.Gi, p.Bi, p.I_local, p.F, gib, stats, rebuild, sp.inorm);
        else if (FP == 128)
            EL_LAUNCH("k_screen_prep", k_screen_prep<128>, dim3(pg), dim3(256), 0, st, p.Gi, p.Bi, p.I_local, p.F, gib, stats, rebuild, sp.inorm);
        else
            EL_LAUNCH("k_screen_prep", k_screen_prep<256>, dim3(pg), dim3(256), 0, st, p.Gi, p.Bi, p.I_local, p.F, gib, stats, rebuild, sp.inorm);
    } else {
        EL_CHECK_HIP(hipMemsetAsync(stats, 0, 8, st));
        EL_CHECK_HIP(hipMemsetAsync(stats + SCR_STAT_IB, 0, 8, st));
    }
    const bool prof = ctx->opt.screen_prof != 0;
    int rc;
#define SCR_RUN(FPV) (prof ? run_passes<FPV, 8, true>(sp, st) : run_passes<FPV, 8, false>(sp, st))
    if (FP == 32)
        rc = SCR_RUN(32);
    else if (FP == 64)
        rc = SCR_RUN(64);
    else if (FP == 128)
        rc = SCR_RUN(128);
    else
        rc = SCR_RUN(256);
#undef SCR_RUN
    if (rc) return rc;
    // exact recomputation of the flagged users by the fp32 MFMA kernel (a grid of early exits when nothing is flagged)
    EL_LAUNCH("k_screen_flags", k_screen_flags, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0, st, sp, n_users);
    EL_CHECK_LAUNCH();
    if (prof) {
        int32_t nf = 0;
        EL_CHECK_HIP(hipStreamSynchronize(st));
        EL_CHECK_HIP(hipMemcpy(&nf, sp.ulist_n, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "[screen prof] flagged users: %d of %lld (stride %d)\n", nf, (long long)n_users, sp.stride);
    }
    TopkParams pw = p;
    pw.ulist = sp.ulist;
    pw.ulist_n = sp.ulist_n;
    ctx->scr_cnt = sp.cnt, ctx->scr_flagged = sp.ulist_n, ctx->scr_users = n_users;
    return el_topk_run_list(pw, w.fb, st);
}

// Diagnostics of the last screened el_score_topk call on this ctx (its workspace must still be alive): records pass 2 appended over
// all users of the block (one record = up to 16 candidate items of one user), users sent to the exact fallback.
__global__ __launch_bounds__(256) void k_screen_count(const int32_t* __restrict__ cnt, int64_t n, unsigned long long* out) {
    unsigned long long s = 0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) s += (unsigned long long)(cnt[t] > 0 ? cnt[t] : 0);
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

extern "C" int el_topk_screen_stats(el_ctx* ctx, void* stream, int64_t* users, int64_t* records, int64_t* flagged_users) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(users && records && flagged_users, "el_topk_screen_stats: null output");
    *users = *records = *flagged_users = 0;
    if (!ctx->scr_cnt || ctx->scr_users <= 0) return 0;               // no screened call yet
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* d = nullptr;
    EL_CHECK_HIP(hipMalloc((void**)&d, 8));
    unsigned long long h = 0;
    int32_t nf = 0;
    hipError_t e = hipMemsetAsync(d, 0, 8, s);
    if (e == hipSuccess) {
        int64_t g = (ctx->scr_users + 255) / 256;
        if (g > 1024) g = 1024;
        hipLaunchKernelGGL(k_screen_count, dim3((unsigned)g), dim3(256), 0, s, ctx->scr_cnt, ctx->scr_users, d);
        e = hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&nf, ctx->scr_flagged, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    EL_CHECK_HIP(e);
    *users = ctx->scr_users, *records = (int64_t)h, *flagged_users = nf;
    return 0;
}
