// Positions of held-out items in the user's complete ranking, and the AUC / GAUC / LAUC sums from them.
//
// Replaces, for the three rank metrics, the reference's full-length lists: an Evaluator that holds AUC or GAUC asks every model
// for num_items recommendations (evaluation/evaluator.py:149-159, needs_full_recommendations at metrics/accuracy/AUC/auc.py:92-95,
// gauc.py:106-109) and the metric classes then read the ranks of the relevant items off those lists:
//   neg_num   num_items - len(train_dict[u]) - len(user_relevant_items) + 1              auc.py:78, gauc.py:81, lauc.py:81
//   term      (neg_num - r_r + p_r) / neg_num for the p_r-th relevant item found, at 0-based rank r_r            auc.py:79-80
//   AUC       mean of all terms of all users (auc.py:86-89)    GAUC  mean over users of sum / len(rel) (gauc.py:83, 91-94)
//   LAUC      mean over users of the sum over ranks < cutoff, / min(cutoff, len(rel))                          lauc.py:81-83
//   users     those with a held-out row and >= 1 relevant item                                                 auc.py:88
// The list the reference ranks is top_k(where(mask, preds, -inf), k = num_items): (score desc, index asc), the masked items a
// -inf tail that never precedes a held-out item.  A [users, items] list is never built here.  For a block of users the kernel
// scores the whole catalogue exactly as the top-k kernels do (el_topk.hip: the k-ordered fma chain from +0, + Bi, + 0.0; the same
// mask protocols) and COUNTS, for each held-out item t of the user,
//   pos = #{ j in [0, I), j != t, j admissible : key(u, j) > key(u, t) }         key = el_make_key (fp32) / (el_d2ord, ~j) (fp64)
// -- the index of t in that list, by the very keys the selection kernels sort by, -0.0 canonicalised as there.  A target the
// model has no row for (id >= I) gets -1 and so does a target the mask removes: the project's splitters never produce the
// latter, and the reference would rank it somewhere in the -inf tail.  NaN scores are outside the contract.
//
// One wave per user (k_rank_wave<T, DENSE>: any F, both mask protocols, tables or a dense block, fp32 or fp64):
//   1. the wave scores up to RANK_CAP of the user's targets, one per lane, and sorts their keys in LDS (best first);
//   2. it streams the catalogue (or the candidate row), 64 items a pass; a lane finds by binary search how many target keys are
//      >= its item's key -- the first target the item ranks ahead of -- and adds 1 to that bucket's LDS counter: log T LDS reads
//      per score instead of T compares.  Under the exclusion protocol the membership test is not made per item: every item is
//      counted, then the user's excluded items are scored by the same chain and taken out again (nnz_u scores, not I log nnz_u
//      dependent loads);
//   3. a prefix sum over the buckets gives the positions; a key carries its item id, the (ascending) target row gives the entry.
// A row with more than RANK_CAP targets takes ceil(T / RANK_CAP) passes over the catalogue.  Integer LDS atomics only: the same
// input gives the same bytes.
//
// el_score_rank has a second route for F <= 256 without a candidate list, k_score_rank_mfma further down: the scores of 128 users
// per workgroup on the matrix cores, up to RANK_TCAP targets per user in LDS, users with more handed to k_rank_wave through a
// device-side list.  Its sums are the same fma chain, so both routes write the same bytes (profiles/rank_bench.md).
//
// el_rank_metrics turns the positions into the six sums (one thread per user, exact integer numerators, the fixed-shape tree of
// el_metrics_tree.h).
#include <type_traits>
#include "el_common.h"

#include "el_topk_common.h"
#include "el_metrics_row.h"
#include "el_metrics_tree.h"

#define RANK_CAP 512         // targets per pass of k_rank_wave: 512 keys (8 or 12 bytes) + 512 counters = 6 / 8 KB of LDS a wave
#define RANK_PER_LANE (RANK_CAP / 64)

template <class T>
struct RankParams {
    const T* Gu;
    const T* Gi;
    const T* Bi;
    const T* preds;
    int64_t ld;
    int64_t u_start, u_stop, I;
    int F;
    const int64_t* excl_indptr;
    const int32_t* excl_indices;
    const int64_t* cand_indptr;
    const int32_t* cand_indices;
    const int64_t* tgt_indptr;
    const int32_t* tgt_indices;
    int32_t* pos;
    // k_rank_wave: if set, the wave of workgroup b takes user u_start + ulist[b] (b < *ulist_n) -- the users k_score_rank_mfma
    // hands over; k_score_rank_mfma: where it writes them
    int32_t* ulist;
    int32_t* ulist_n;
};

__device__ __forceinline__ float el_rank_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double el_rank_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the score of item il for the wave's user: k_topk_wave's expression, term for term
template <class T, bool DENSE>
__device__ __forceinline__ T el_rank_score(const RankParams<T>& p, const T* gu, int64_t il) {
    if (DENSE) return p.preds[(int64_t)blockIdx.x * p.ld + il] + T(0);
    const T* gi = p.Gi + il * (int64_t)p.F;
    T acc = 0;
    for (int f = 0; f < p.F; ++f) acc = el_rank_fma(gi[f], gu[f], acc);
    return (p.Bi ? acc + p.Bi[il] : acc) + T(0);
}

// the sorted target keys of one pass: the key policies of the selection kernels own layout, sort and the empty slot
template <class T>
using RankKey = typename std::conditional<sizeof(T) == 4, ElPackedKey, ElPairKey<double>>::type;

// true when the key in slot t is >= the key of (v, index)
__device__ __forceinline__ bool el_rank_slot_ge(const ElPackedKey& k, int t, float v, int32_t index) { return k.a[t] >= el_make_key(v, index); }
__device__ __forceinline__ bool el_rank_slot_ge(const ElPairKey<double>& k, int t, double v, int32_t index) {
    const u64 x = k.prim[t], y = el_d2ord(v);
    const u32 sx = k.sec[t], sy = 0xffffffffu - (u32)index;
    return (x > y) | ((x == y) & (sx >= sy));
}

template <class T, bool DENSE>
__global__ __launch_bounds__(64) void k_rank_wave(RankParams<T> p) {
    typedef RankKey<T> Key;
    __shared__ __attribute__((aligned(16))) char ksm[RANK_CAP * 12];
    __shared__ int cnt[RANK_CAP];
    const Key keys(ksm, RANK_CAP);
    const int lane = threadIdx.x;
    int64_t urel = blockIdx.x;
    if (!DENSE && p.ulist) {                                     // (dense rows stay indexed by blockIdx.x)
        if ((int64_t)blockIdx.x >= (int64_t)*p.ulist_n) return;
        urel = p.ulist[blockIdx.x];
    }
    const int64_t user = p.u_start + urel;
    const T* gu = DENSE ? nullptr : p.Gu + user * (int64_t)p.F;
    const int64_t t0 = p.tgt_indptr[user], t1 = p.tgt_indptr[user + 1];
    if (t1 <= t0) return;
    const int64_t obase = p.tgt_indptr[p.u_start];
    int64_t e0 = 0, e1 = 0, c0 = 0, c1 = 0;
    if (p.excl_indptr) {
        e0 = p.excl_indptr[user];
        e1 = p.excl_indptr[user + 1];
    }
    if (p.cand_indptr) {
        c0 = p.cand_indptr[user];
        c1 = p.cand_indptr[user + 1];
    }
    const bool use_cand = p.cand_indptr != nullptr;
    const bool use_excl = p.excl_indptr != nullptr && !use_cand;

    for (int64_t s0 = t0; s0 < t1; s0 += RANK_CAP) {
        const int64_t s1 = s0 + RANK_CAP < t1 ? s0 + RANK_CAP : t1;
        // ---- 1. the slice's targets: score, key, sort ---------------------------------------------------------------------
        int nv = 0;
        for (int64_t b = s0; b < s1; b += 64) {
            const int64_t e = b + lane;
            bool ok = false;
            int32_t t = -1;
            T s = 0;
            if (e < s1) {
                t = p.tgt_indices[e];
                ok = t >= 0 && (int64_t)t < p.I;
                if (ok && use_cand) ok = el_row_contains(p.cand_indices, c0, c1, t);
                if (ok && use_excl) ok = !el_row_contains(p.excl_indices, e0, e1, t);
                if (ok)
                    s = el_rank_score<T, DENSE>(p, gu, t);
                else
                    p.pos[e - obase] = -1;
            }
            const u64 bal = __ballot(ok);
            if (ok) keys.put(nv + __popcll(bal & ((1ull << lane) - 1ull)), s, t);
            nv += __popcll(bal);
        }
        if (nv == 0) continue;                                   // (wave-uniform)
        int n2 = 64;
        while (n2 < nv) n2 <<= 1;
        for (int t = nv + lane; t < n2; t += 64) keys.clear(t);
        for (int t = lane; t < RANK_CAP; t += 64) cnt[t] = 0;
        el_wave_lds_sync();
        el_wave_bitonic_desc(keys, n2, lane);

        // ---- 2. the catalogue: bucket b = #{targets with key >= the item's key}; the item precedes targets b, b+1, ... ---------
        auto bucket = [&](T s, int32_t item, int delta) {
            int lo = 0, hi = nv;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (el_rank_slot_ge(keys, mid, s, item))
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < nv) atomicAdd(&cnt[lo], delta);
        };
        if (use_cand) {
            for (int64_t b = c0; b < c1; b += 64) {
                const int64_t e = b + lane;
                if (e < c1) {
                    const int32_t g = p.cand_indices[e];
                    if (g >= 0 && (int64_t)g < p.I) bucket(el_rank_score<T, DENSE>(p, gu, g), g, 1);
                }
            }
        } else {
            for (int64_t b = 0; b < p.I; b += 64) {
                const int64_t il = b + lane;
                if (il < p.I) bucket(el_rank_score<T, DENSE>(p, gu, il), (int32_t)il, 1);
            }
            if (use_excl) {                                      // take the excluded items out again (a repeated id counts once)
                for (int64_t b = e0; b < e1; b += 64) {
                    const int64_t e = b + lane;
                    if (e < e1) {
                        const int32_t g = p.excl_indices[e];
                        const bool dup = e > e0 && p.excl_indices[e - 1] == g;
                        if (!dup && g >= 0 && (int64_t)g < p.I) bucket(el_rank_score<T, DENSE>(p, gu, g), g, -1);
                    }
                }
            }
        }
        el_wave_lds_sync();

        // ---- 3. prefix sum over the buckets: target in slot s has cnt[0] + ... + cnt[s] items ahead of it --------------------
        int loc[RANK_PER_LANE];
        int tot = 0;
#pragma unroll
        for (int q = 0; q < RANK_PER_LANE; ++q) {
            tot += cnt[lane * RANK_PER_LANE + q];
            loc[q] = tot;
        }
        int inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        const int before = inc - tot;
#pragma unroll
        for (int q = 0; q < RANK_PER_LANE; ++q) {
            const int s = lane * RANK_PER_LANE + q;
            if (s < nv) {
                const int32_t item = keys.index(s);
                const int64_t e = el_lower_bound(p.tgt_indices, s0, s1, item);
                if (e < s1) p.pos[e - obase] = before + loc[q];
            }
        }
        el_wave_lds_sync();
    }
}

// =====================================================================================
// Fused fp32 route on the matrix cores (el_score_rank, F <= 256, no candidate list).  The tile loop is k_score_topk_mfma's
// (el_topk.hip, copied: that file's code objects stay as they are): 128 users per workgroup (4 waves x 32 users), the users'
// rows resident in VGPRs, items through LDS in tiles of 32 * NIB rows and K-chunks of 32, D[item][user] accumulated by
// v_mfma_f32_32x32x2_f32 -- bit for bit the k-ordered fma chain, so the positions equal the wave route's.
//   A operand (items): lane l supplies A[row = l&31][k = l>>5]    <- LDS (stride 33)
//   B operand (users): lane l supplies B[k = l>>5][col = l&31]    <- registers
//   D: lane l holds col (user) l&31, rows (items) (r&3) + 8*(r>>2) + 4*(l>>5), r = 0..15
// Lanes l and l+32 own the same user and every user belongs to one wave: all rank state is wave-private.
//   0. per user, up to RANK_TCAP targets are scored by the chain (a lane each), ranked among themselves and stored best
//      first in the user's LDS slice; a user with more targets goes to the device-side list the wave kernel takes afterwards
//   1. the epilogue of a tile buckets each of the lane's 16 * NIB scores against its user's sorted keys (six LDS reads, branch
//      free) and adds 1 to the bucket's counter.  The exclusion mask is NOT tested per item:
//   2. the wave gathers each user's exclusion row, scores it with the chain and takes those items out again (nnz_u scores)
//   3. prefix sums over the buckets, written out through the ascending target row
// LDS per workgroup: staging 2 * BI * 33 * 4 + bias 2 * BI * 4, keys 128 * RANK_TCAP * 8, counters 128 * RANK_TCAP * 4, 128 counts.
// =====================================================================================
#define RANK_AUTO_MFMA 1     // EL_TOPK_AUTO takes the fused route where it is eligible (profiles/rank_bench.md)
#define RANK_TCAP 63         // targets per user of the fused route (< 64: a lane each, and the six-step search covers [0, 63])

__device__ __forceinline__ int el_rank_bucket(const u64* __restrict__ uk, int nv, u64 key) {
    int lo = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const int mid = lo + step;
        const u64 kv = uk[(mid < RANK_TCAP ? mid : RANK_TCAP) - 1];
        lo = (mid <= nv && kv >= key) ? mid : lo;
    }
    return lo;                                                   // #{slots of [0, nv) with key >= `key`}
}

template <int FP, int NIB, int KC, int NW, int OCC>
__global__ __launch_bounds__(NW * 64, OCC) void k_score_rank_mfma(RankParams<float> p, int vec) {
    constexpr int LDA = KC + 1, BI = 32 * NIB, NCH = (FP + KC - 1) / KC, UPB = NW * 32, NT = NW * 64;
    constexpr int C4 = KC / 4;                      // float4 pieces per staged row
    constexpr int NLD = (BI * C4 + NT - 1) / NT;    // float4 loads per thread per chunk
    static_assert((BI * C4) % NT == 0, "staging must divide evenly");
    constexpr int A_FLOATS = 2 * BI * LDA + 2 * BI;
    static_assert(A_FLOATS % 2 == 0, "the keys behind the staging area are 8-byte aligned");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* As = reinterpret_cast<float*>(smem);                // [2][BI][LDA]
    float* Bs = As + 2 * BI * LDA;                             // [2][BI] bias
    u64* keys = reinterpret_cast<u64*>(smem + A_FLOATS * 4);   // [UPB][RANK_TCAP] sorted target keys
    int* cnt = reinterpret_cast<int*>(keys + UPB * RANK_TCAP); // [UPB][RANK_TCAP] bucket counters
    int* nvs = cnt + UPB * RANK_TCAP;                          // [UPB] valid targets

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, col = lane & 31;
    const int uslot = wave * 32 + col;
    const int64_t nlist = p.u_stop - p.u_start;
    const int64_t uidx = (int64_t)blockIdx.x * UPB + uslot;
    const bool uvalid = uidx < nlist;
    const int64_t user = p.u_start + (uvalid ? uidx : 0);
    const int F = p.F;
    const int64_t I = p.I;
    const int64_t obase = p.tgt_indptr[p.u_start];

    // resident user fragments
    float bfrag[FP / 2];
    {
        const float* gu = p.Gu + user * (int64_t)F;
#pragma unroll
        for (int s = 0; s < FP / 2; ++s) {
            int kk = 2 * s + hi;
            bfrag[s] = (uvalid && kk < F) ? gu[kk] : 0.f;
        }
    }
    int64_t e0 = 0, e1 = 0;
    if (p.excl_indptr && uvalid) {
        e0 = p.excl_indptr[user];
        e1 = p.excl_indptr[user + 1];
    }

    // ---- 0. the targets of the wave's 32 users ----------------------------------------------------------------------------
    for (int ul = 0; ul < 32; ++ul) {
        const int slot = wave * 32 + ul;
        int nv = 0;
        if ((int64_t)blockIdx.x * UPB + slot < nlist) {              // (wave-uniform)
            const int64_t uu = p.u_start + (int64_t)blockIdx.x * UPB + slot;
            const int64_t t0 = p.tgt_indptr[uu], t1 = p.tgt_indptr[uu + 1];
            const int64_t T = t1 - t0;
            if (T > RANK_TCAP) {
                if (lane == 0) p.ulist[atomicAdd(p.ulist_n, 1)] = (int32_t)(uu - p.u_start);
            } else if (T > 0) {
                const int64_t ue0 = __shfl(e0, ul, 64), ue1 = __shfl(e1, ul, 64);
                bool ok = false;
                int32_t t = -1;
                float s = 0.f;
                if (lane < T) {
                    t = p.tgt_indices[t0 + lane];
                    ok = t >= 0 && (int64_t)t < I;
                    if (ok && p.excl_indptr) ok = !el_row_contains(p.excl_indices, ue0, ue1, t);
                    if (ok)
                        s = el_rank_score<float, false>(p, p.Gu + uu * (int64_t)F, t);
                    else
                        p.pos[t0 + lane - obase] = -1;
                }
                const u64 key = ok ? el_make_key(s, t) : 0ull;       // (a valid key is never 0)
                int r = 0;
                for (int j = 0; j < (int)T; ++j) r += __shfl(key, j, 64) > key ? 1 : 0;
                if (ok) keys[slot * RANK_TCAP + r] = key;
                nv = __popcll(__ballot(ok));
                if (lane < RANK_TCAP) cnt[slot * RANK_TCAP + lane] = 0;
            }
        }
        if (lane == 0) nvs[slot] = nv;
    }
    el_wave_lds_sync();
    const int mynv = nvs[uslot];
    const u64* uk = keys + uslot * RANK_TCAP;
    int* uc = cnt + uslot * RANK_TCAP;

    const int ntiles = (int)((I + BI - 1) / BI);
    const int nch = (F + KC - 1) / KC;

    float4 pre[NLD];
    float pre_bias = 0.f;

    auto gload = [&](int tile, int ch) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            int f4 = q * NT + tid;
            int row = f4 / C4, c4 = f4 % C4;
            int64_t item = (int64_t)tile * BI + row;
            int kk = ch * KC + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (item < I && kk < F) {
                const float* src = p.Gi + item * (int64_t)F + kk;
                if (vec) {
                    v = *reinterpret_cast<const float4*>(src);
                } else {
                    v.x = src[0];
                    if (kk + 1 < F) v.y = src[1];
                    if (kk + 2 < F) v.z = src[2];
                    if (kk + 3 < F) v.w = src[3];
                }
            }
            pre[q] = v;
        }
        if (ch == 0 && tid < BI) {
            int64_t item = (int64_t)tile * BI + tid;
            pre_bias = (p.Bi && item < I) ? p.Bi[item] : 0.f;
        }
    };
    auto lstore = [&](int buf, int bias_buf) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            int f4 = q * NT + tid;
            int row = f4 / C4, c4 = f4 % C4;
            float* dst = As + (buf * BI + row) * LDA + c4 * 4;
            dst[0] = pre[q].x;
            dst[1] = pre[q].y;
            dst[2] = pre[q].z;
            dst[3] = pre[q].w;
        }
        if (bias_buf >= 0 && tid < BI) Bs[bias_buf * BI + tid] = pre_bias;
    };

    int buf = 0;
    if (ntiles > 0) gload(0, 0);
    for (int tile = 0; tile < ntiles; ++tile) {
        floatx16 acc[NIB];
#pragma unroll
        for (int b = 0; b < NIB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch < nch) {
                lstore(buf, ch == 0 ? (tile & 1) : -1);
                __syncthreads();
                int nt = tile, nc = ch + 1;
                if (nc >= nch) {
                    nt = tile + 1;
                    nc = 0;
                }
                if (nt < ntiles) gload(nt, nc);
                const float* Ab = As + buf * BI * LDA;
#pragma unroll
                for (int s = 0; s < KC / 2; ++s) {
                    if (ch * (KC / 2) + s >= FP / 2) break;   // compile-time (FP < KC * NCH)
                    float a[NIB];
#pragma unroll
                    for (int b = 0; b < NIB; ++b) a[b] = Ab[(b * 32 + col) * LDA + 2 * s + hi];
#pragma unroll
                    for (int b = 0; b < NIB; ++b)
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[b], bfrag[ch * (KC / 2) + s], acc[b], 0, 0, 0);
                }
                buf ^= 1;
            }
        }

        // ---- 1. bucket the tile's scores -------------------------------------------------------------------------------
        const float* bb = Bs + (tile & 1) * BI;
        if (__ballot(mynv > 0) != 0ull) {
#pragma unroll
            for (int b = 0; b < NIB; ++b) {
#pragma unroll
                for (int r0 = 0; r0 < 16; r0 += 4) {
                    int lo[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int r = r0 + q;
                        const int row = b * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        const int64_t il = (int64_t)tile * BI + row;
                        const float sc = (acc[b][r] + bb[row]) + 0.0f;
                        // an item past the catalogue takes key 0: below every valid key, bucket mynv, not counted
                        lo[q] = el_rank_bucket(uk, mynv, il < I ? el_make_key(sc, (int32_t)il) : 0ull);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (lo[q] < mynv) atomicAdd(&uc[lo[q]], 1);
                }
            }
        }
    }
    el_wave_lds_sync();

    // ---- 2. take each user's excluded items out again; 3. prefix sums, write-out ---------------------------------------------
    for (int ul = 0; ul < 32; ++ul) {
        const int slot = wave * 32 + ul;
        const int nv = __shfl(mynv, ul, 64);
        if (nv == 0) continue;                                       // (wave-uniform; covers slots past the user range)
        const int64_t uu = p.u_start + (int64_t)blockIdx.x * UPB + slot;
        const u64* k2 = keys + slot * RANK_TCAP;
        int* c2 = cnt + slot * RANK_TCAP;
        if (p.excl_indptr) {
            const int64_t ue0 = __shfl(e0, ul, 64), ue1 = __shfl(e1, ul, 64);
            const float* gu = p.Gu + uu * (int64_t)F;
            for (int64_t b = ue0; b < ue1; b += 64) {
                const int64_t e = b + lane;
                if (e < ue1) {
                    const int32_t g = p.excl_indices[e];
                    const bool dup = e > ue0 && p.excl_indices[e - 1] == g;      // (a repeated id counts once)
                    if (!dup && g >= 0 && (int64_t)g < I) {
                        const int lo = el_rank_bucket(k2, nv, el_make_key(el_rank_score<float, false>(p, gu, g), g));
                        if (lo < nv) atomicAdd(&c2[lo], -1);
                    }
                }
            }
            el_wave_lds_sync();
        }
        int inc = lane < nv ? c2[lane] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane < nv) {
            const int64_t t0 = p.tgt_indptr[uu], t1 = p.tgt_indptr[uu + 1];
            const int64_t e = el_lower_bound(p.tgt_indices, t0, t1, el_key_item(k2[lane]));
            if (e < t1) p.pos[e - obase] = inc;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static bool rank_mfma_eligible(int F, const void* cand) { return cand == nullptr && F >= 1 && F <= 256; }

// the fused route's workspace: the users it hands to the wave kernel, and their number
struct RankWs {
    int32_t* ulist;
    int32_t* ulist_n;
};
static size_t rank_carve(int64_t n_users, void* base, RankWs* w) {
    ElCarve c{(char*)base};
    w->ulist_n = c.take<int32_t>(1);
    w->ulist = c.take<int32_t>((size_t)n_users);
    return c.off;
}

template <int FP, int NIB, int KC, int NW, int OCC>
static int launch_rank_mfma(const RankParams<float>& p, int vec, hipStream_t st) {
    constexpr int LDA = KC + 1, BI = 32 * NIB, UPB = NW * 32;
    constexpr size_t lds = (size_t)(2 * BI * LDA + 2 * BI) * 4 + (size_t)UPB * RANK_TCAP * 12 + (size_t)UPB * 4;
    auto kern = k_score_rank_mfma<FP, NIB, KC, NW, OCC>;
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t n_users = p.u_stop - p.u_start;
    EL_LAUNCH("k_score_rank_mfma", kern, dim3((unsigned)((n_users + UPB - 1) / UPB)), dim3(NW * 64), lds, st, p, vec);
    EL_CHECK_LAUNCH();
    return 0;
}

static int check_rank_args(const char* fn, bool dense, const void* src0, const void* src1, int64_t ld, int64_t u_start, int64_t u_stop,
                           int64_t I, int F, const void* excl_indptr, const void* excl_indices, const void* cand_indptr,
                           const void* cand_indices, const void* tgt_indptr, const void* tgt_indices, const void* pos) {
    EL_REQUIRE(u_stop >= u_start && u_start >= 0, "%s: bad user range", fn);
    EL_REQUIRE(I >= 0 && I < 0x7fffffffLL, "%s: I out of range", fn);
    EL_REQUIRE(F >= 1, "%s: F must be >= 1", fn);
    EL_REQUIRE(u_stop == u_start || pos, "%s: null pos", fn);
    if (dense) {
        EL_REQUIRE(src0 && ld >= I, "%s: bad preds/ld", fn);
    } else {
        EL_REQUIRE(src0 && src1, "%s: null factor table", fn);
    }
    EL_REQUIRE(excl_indptr != nullptr || excl_indices == nullptr, "%s: excl_indices without excl_indptr", fn);
    EL_REQUIRE(excl_indptr == nullptr || excl_indices != nullptr, "%s: excl_indptr without excl_indices", fn);
    EL_REQUIRE((cand_indptr == nullptr) == (cand_indices == nullptr), "%s: cand CSR needs both arrays", fn);
    EL_REQUIRE(tgt_indptr && tgt_indices, "%s: target CSR needs both arrays", fn);
    return 0;
}

template <class T>
static RankParams<T> rank_params(const T* Gu, const T* Gi, const T* Bi, const T* preds, int64_t ld, int64_t u_start, int64_t u_stop, int64_t I,
                                 int F, const int64_t* excl_indptr, const int32_t* excl_indices, const int64_t* cand_indptr,
                                 const int32_t* cand_indices, const int64_t* tgt_indptr, const int32_t* tgt_indices, int32_t* pos) {
    RankParams<T> p;
    memset(&p, 0, sizeof(p));
    p.Gu = Gu, p.Gi = Gi, p.Bi = Bi, p.preds = preds, p.ld = ld;
    p.u_start = u_start, p.u_stop = u_stop, p.I = I, p.F = F;
    p.excl_indptr = excl_indptr, p.excl_indices = excl_indices, p.cand_indptr = cand_indptr, p.cand_indices = cand_indices;
    p.tgt_indptr = tgt_indptr, p.tgt_indices = tgt_indices, p.pos = pos;
    return p;
}

template <class T, bool DENSE>
static int run_rank_wave(const char* fn, el_ctx* ctx, void* stream, const T* Gu, const T* Gi, const T* Bi, const T* preds, int64_t ld,
                         int64_t u_start, int64_t u_stop, int64_t I, int F, const int64_t* excl_indptr, const int32_t* excl_indices,
                         const int64_t* cand_indptr, const int32_t* cand_indices, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                         int32_t* pos) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = check_rank_args(fn, DENSE, DENSE ? preds : Gu, Gi, ld, u_start, u_stop, I, F, excl_indptr, excl_indices, cand_indptr,
                                 cand_indices, tgt_indptr, tgt_indices, pos))
        return rc;
    if (u_stop == u_start) return 0;
    const RankParams<T> p = rank_params<T>(Gu, Gi, Bi, preds, ld, u_start, u_stop, I, F, excl_indptr, excl_indices, cand_indptr, cand_indices,
                                           tgt_indptr, tgt_indices, pos);
    EL_LAUNCH(sizeof(T) == 4 ? "k_rank_wave" : "k_rank_wave_f64", (k_rank_wave<T, DENSE>), dim3((unsigned)(u_stop - u_start)), dim3(64), 0,
              (hipStream_t)stream, p);
    EL_CHECK_LAUNCH();
    return 0;
}

// AUTO: the fused route where it is eligible and a workspace is given (profiles/rank_bench.md), else the wave kernel
static bool rank_use_mfma(int algo, int F, const void* cand, const void* ws) {
    return algo == EL_TOPK_MFMA || (algo == EL_TOPK_AUTO && RANK_AUTO_MFMA && rank_mfma_eligible(F, cand) && ws != nullptr);
}

extern "C" size_t el_score_rank_ws_bytes(int64_t n_users, int64_t I, int32_t F, int64_t tgt_nnz, int64_t excl_nnz, int algo) {
    (void)I, (void)tgt_nnz, (void)excl_nnz;
    algo &= 0xff;
    RankWs w;
    if (n_users > 0 && rank_mfma_eligible(F, nullptr) && (algo == EL_TOPK_MFMA || (algo == EL_TOPK_AUTO && RANK_AUTO_MFMA)))
        return rank_carve(n_users, nullptr, &w);
    return 0;                                                    // the wave route keeps its state in LDS
}

extern "C" int el_score_rank(el_ctx* ctx, void* stream, const float* Gu, const float* Gi, const float* Bi, int64_t u_start,
                             int64_t u_stop, int64_t I, int32_t F, const int64_t* excl_indptr, const int32_t* excl_indices,
                             const int64_t* cand_indptr, const int32_t* cand_indices, const int64_t* tgt_indptr,
                             const int32_t* tgt_indices, int32_t* pos, int algo, void* ws, size_t ws_bytes) {
    algo &= 0xff;
    EL_REQUIRE(algo == EL_TOPK_AUTO || algo == EL_TOPK_SIMPLE || algo == EL_TOPK_MFMA, "el_score_rank: algo %d unsupported (AUTO, MFMA, SIMPLE)",
               algo);
    if (!rank_use_mfma(algo, F, cand_indptr, ws))
        return run_rank_wave<float, false>("el_score_rank", ctx, stream, Gu, Gi, Bi, nullptr, 0, u_start, u_stop, I, F, excl_indptr,
                                           excl_indices, cand_indptr, cand_indices, tgt_indptr, tgt_indices, pos);
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = check_rank_args("el_score_rank", false, Gu, Gi, 0, u_start, u_stop, I, F, excl_indptr, excl_indices, cand_indptr,
                                 cand_indices, tgt_indptr, tgt_indices, pos))
        return rc;
    EL_REQUIRE(rank_mfma_eligible(F, cand_indptr), "el_score_rank: the MFMA route needs F<=256 and no candidate list");
    if (u_stop == u_start) return 0;
    RankWs w;
    EL_REQUIRE(ws != nullptr && ws_bytes >= rank_carve(u_stop - u_start, ws, &w), "el_score_rank: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    RankParams<float> p = rank_params<float>(Gu, Gi, Bi, nullptr, 0, u_start, u_stop, I, F, excl_indptr, excl_indices, nullptr, nullptr,
                                             tgt_indptr, tgt_indices, pos);
    p.ulist = w.ulist, p.ulist_n = w.ulist_n;
    EL_CHECK_HIP(hipMemsetAsync(w.ulist_n, 0, sizeof(int32_t), st));
    const int vec = (F % 4 == 0) && (((uintptr_t)Gi) % 16 == 0);
    int rc;
    if (F <= 32)
        rc = launch_rank_mfma<32, 4, 32, 4, 2>(p, vec, st);
    else if (F <= 64)
        rc = launch_rank_mfma<64, 4, 32, 4, 2>(p, vec, st);
    else if (F <= 128)
        rc = launch_rank_mfma<128, 4, 32, 4, 2>(p, vec, st);
    else
        rc = launch_rank_mfma<256, 2, 32, 4, 1>(p, vec, st);
    if (rc) return rc;
    // the users over RANK_TCAP targets: one wave each (the list length lives on the device; surplus workgroups exit at once)
    EL_LAUNCH("k_rank_wave", (k_rank_wave<float, false>), dim3((unsigned)(u_stop - u_start)), dim3(64), 0, st, p);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_score_rank_f64(el_ctx* ctx, void* stream, const double* P, const double* Q, const double* b, int64_t u_start,
                                 int64_t u_stop, int64_t I, int32_t F, const int64_t* excl_indptr, const int32_t* excl_indices,
                                 const int64_t* cand_indptr, const int32_t* cand_indices, const int64_t* tgt_indptr,
                                 const int32_t* tgt_indices, int32_t* pos) {
    return run_rank_wave<double, false>("el_score_rank_f64", ctx, stream, P, Q, b, nullptr, 0, u_start, u_stop, I, F, excl_indptr,
                                        excl_indices, cand_indptr, cand_indices, tgt_indptr, tgt_indices, pos);
}

extern "C" int el_dense_rank(el_ctx* ctx, void* stream, const float* preds, int64_t ld, int64_t u_start, int64_t u_stop, int64_t I,
                             const int64_t* excl_indptr, const int32_t* excl_indices, const int64_t* cand_indptr,
                             const int32_t* cand_indices, const int64_t* tgt_indptr, const int32_t* tgt_indices, int32_t* pos) {
    return run_rank_wave<float, true>("el_dense_rank", ctx, stream, nullptr, nullptr, nullptr, preds, ld, u_start, u_stop, I, 1,
                                      excl_indptr, excl_indices, cand_indptr, cand_indices, tgt_indptr, tgt_indices, pos);
}

extern "C" int el_dense_rank_f64(el_ctx* ctx, void* stream, const double* preds, int64_t ld, int64_t u_start, int64_t u_stop, int64_t I,
                                 const int64_t* excl_indptr, const int32_t* excl_indices, const int64_t* cand_indptr,
                                 const int32_t* cand_indices, const int64_t* tgt_indptr, const int32_t* tgt_indices, int32_t* pos) {
    return run_rank_wave<double, true>("el_dense_rank_f64", ctx, stream, nullptr, nullptr, nullptr, preds, ld, u_start, u_stop, I, 1,
                                       excl_indptr, excl_indices, cand_indptr, cand_indices, tgt_indptr, tgt_indices, pos);
}

// =====================================================================================================
// The metric sums.  Per user, over the relevant entries (rating >= threshold) of the held-out row:
//   nrel = their number (ids >= n_items included, like len(user_relevant_items));  neg = n_items - train_len - nrel + 1
//   m, P = number and position sum of those with pos >= 0;   mc, Pc = the same over 0 <= pos < cutoff
//   S = (m neg - P + m (m - 1) / 2) / neg: the found items taken in list order are p = 0 .. m-1, so sum(neg - r_p + p) has this
//   integer numerator; S^c likewise (the items at ranks < cutoff are the first mc found)
// row = S, m, S / nrel, S^c / min(cutoff, nrel), [nrel > 0], [nrel > 0 and neg <= 0]; a user with neg <= 0 adds to the last only.
// =====================================================================================================
#define RANKMET_N 6

__global__ __launch_bounds__(256) void k_rank_metrics(const int32_t* __restrict__ pos, int64_t u_start, int64_t n,
                                                      const int64_t* __restrict__ tp, const float* __restrict__ tr, double thr,
                                                      const int64_t* __restrict__ train_indptr, int64_t n_items, int cutoff,
                                                      double* __restrict__ rows, double* __restrict__ per_user) {
    const int64_t ur = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ur >= n) return;
    const int64_t user = u_start + ur, base = tp[u_start];
    int64_t nrel = 0, m = 0, P = 0, mc = 0, Pc = 0;
    for (int64_t e = tp[user]; e < tp[user + 1]; ++e) {
        if (!(met_rating(tr, e) >= thr)) continue;
        ++nrel;
        const int64_t q = pos[e - base];
        if (q >= 0) {
            ++m;
            P += q;
            if (q < cutoff) {
                ++mc;
                Pc += q;
            }
        }
    }
    const int64_t neg = n_items - (train_indptr[user + 1] - train_indptr[user]) - nrel + 1;
    double o[RANKMET_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (nrel > 0 && neg <= 0) {
        o[5] = 1.0;
    } else if (nrel > 0) {
        const double S = (double)(m * neg - P + m * (m - 1) / 2) / (double)neg;
        const double Sc = (double)(mc * neg - Pc + mc * (mc - 1) / 2) / (double)neg;
        o[0] = S;
        o[1] = (double)m;
        o[2] = S / (double)nrel;
        o[3] = Sc / (double)(nrel < cutoff ? nrel : (int64_t)cutoff);
        o[4] = 1.0;
    }
#pragma unroll
    for (int c = 0; c < RANKMET_N; ++c) rows[ur * RANKMET_N + c] = o[c];
    if (per_user) {
#pragma unroll
        for (int c = 0; c < 4; ++c) per_user[ur * 4 + c] = o[c];
    }
}

extern "C" size_t el_rank_metrics_ws_bytes(int64_t n_users) {
    MetWs w;
    return n_users <= 0 ? 0 : met_carve(n_users, RANKMET_N, nullptr, &w);
}

extern "C" int el_rank_metrics(el_ctx* ctx, void* stream, const int32_t* pos, int64_t u_start, int64_t u_stop, const int64_t* test_indptr,
                               const int32_t* test_indices, const float* test_ratings, double threshold, const int64_t* train_indptr,
                               int64_t n_items, int32_t cutoff, double* sums, double* per_user, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(u_stop >= u_start && u_start >= 0, "el_rank_metrics: bad user range");
    const int64_t n = u_stop - u_start;
    if (n == 0) return 0;
    EL_REQUIRE(pos && test_indptr && test_indices && train_indptr && sums, "el_rank_metrics: null pointer");
    EL_REQUIRE(cutoff >= 1 && n_items >= 0, "el_rank_metrics: bad cutoff / n_items");
    MetWs w;
    EL_REQUIRE(ws != nullptr && ws_bytes >= met_carve(n, RANKMET_N, ws, &w), "el_rank_metrics: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    EL_LAUNCH("k_rank_metrics", k_rank_metrics, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pos, u_start, n, test_indptr, test_ratings,
              threshold, train_indptr, n_items, (int)cutoff, w.rows, per_user);
    met_tree_sum<RANKMET_N, -1>(st, w.rows, n, w.part, sums);
    EL_CHECK_LAUNCH();
    return 0;
}
