// ItemAutoRec / UserAutoRec train step on the batch's nonzeros, encoder for prediction.
//
// Replaces UserAutoRecModel / ItemAutoRecModel.call / train_step (userautorec_model.py:86-107, itemautorec_model.py:83-104) and the
// dense-row sampler feeding them (sparse_sampler.py:19-25).  N is the layer width (items for the user variant, users for the item
// variant), a batch is B rows of a binary CSR (sp_i_train, or its transpose):
//
//   h = sigmoid(x W1 + b1);  r = act(h W2 + b2), act linear (User) or sigmoid (Item);  loss = (1/B) sum_b sum_{j in row b} (1 - r_bj)^2
//
// The reference multiplies the reconstruction by sign(batch) before it takes the error (:96 / :99): the decoder's output gradient is
// zero outside the batch's nonzeros, so the step needs the decoder at the observed entries only.  No [B, N] array is formed:
//   k_ar_boff         boff[b] = number of entries in the batch rows before position b (where row b's d values live)
//   k_ar_enc          h[b] = sigmoid(sum_{j in row b} W1[j] + b1): gather-sum, the 16 wave partials added in wave order
//   k_ar_dec          per entry: pre = h[b].W2T[j] + b2[j], r, err = 1 - r, d = -2 err / B_global (x r (1 - r) for the sigmoid head);
//                     dh[b] = sum_j d W2T[j] (wave w takes the row's entries w, w + 16, ..., the partials added in wave order: an
//                     order the row alone fixes); dpre1 = dh h (1 - h); the loss partial is ADDED to a device double
//   k_vae_w1_count / _scan (el_vae.hip), k_ar_fill   the batch transposed on the fly: per item the list of batch positions that hold it
//   k_ar_item_light / k_ar_item_heavy   per item j, over its batch positions ASCENDING: gW1[j] = sum dpre1[b], gW2T[j] = sum d_bj h[b],
//                     gb2[j] = sum d_bj; d_bj is found by a search for j in the sorted CSR row of position b.  Every row is written
//                     exactly once per step (zeros for the items the batch does not touch), nothing depends on the order atomics landed in.
//   el_colsum_finish  gb1 = ordered column sum of dpre1
//   k_ar_adam         Keras' dense Adam on the four variables, TF's ApplyAdam arithmetic (el_vae.hip:14), eps 1e-7: every element
//                     moves every step
// W2 is held transposed, W2T [N, H]: the decoder dot, dh and the decoder's weight gradient are row gathers.
// The L2 kernel_regularizers the reference declares never reach its loss (train_step does not add self.losses): l_w is a no-op here too.
#include "el_common.h"

// (el_vae.hip) per-item counts of a batch, their exclusive scan + the list of items in more than W1_LIGHT batch rows
__global__ void k_vae_w1_count(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                               int32_t* __restrict__ cnt);
__global__ void k_vae_w1_scan(const int32_t* __restrict__ cnt, int64_t I, int32_t* __restrict__ off, int32_t* __restrict__ cursor,
                              int32_t* __restrict__ heavy);

namespace {

constexpr int AR_LIGHT = 16;            // = W1_LIGHT of k_vae_w1_scan: an item in more batch rows than this is on the heavy list
constexpr int AR_ACT_SIGMOID = 3;       // el_gemm_f32's code
constexpr int64_t AR_MAX_B = 262144;    // batch rows of one step: the heavy kernel's presence bits (32 KiB) beside its partial tables

__device__ __forceinline__ float ar_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- boff[0..B] = exclusive scan of the batch rows' lengths; status <- 1 when the batch holds more than nnz_max entries ----
__global__ __launch_bounds__(1024) void k_ar_boff(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr, int64_t B,
                                                  int64_t nnz_max, int32_t* __restrict__ boff, int32_t* __restrict__ status,
                                                  double* loss_out) {
    __shared__ long long tot[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = ((B + 15) / 16 + 63) / 64 * 64, i0 = wave * chunk, i1 = (i0 + chunk < B) ? i0 + chunk : B;
    long long s = 0;
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        const int32_t r = rows[i];
        s += indptr[r + 1] - indptr[r];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) tot[wave] = s;
    __syncthreads();
    long long carry = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) carry += tot[w];
        all += tot[w];
    }
    const bool over = all > nnz_max;                                 // (then nothing downstream runs: the offsets are not used)
    for (int64_t base = i0; base < i1; base += 64) {
        const int64_t i = base + lane;
        long long v = 0;
        if (i < i1) {
            const int32_t r = rows[i];
            v = indptr[r + 1] - indptr[r];
        }
        long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (i < i1) boff[i] = over ? 0 : (int32_t)(carry + inc - v);
        carry += __shfl(inc, 63, 64);
    }
    if (threadIdx.x == 0) {
        boff[B] = over ? -1 : (int32_t)all;                          // -1: the kernels behind this one return at once
        if (over) status[0] = 1, loss_out[0] = NAN;                  // (loud on both channels: the gradients are NOT computed)
    }
}

// pairs[off[j] ..) = the batch positions that hold item j, in the order the atomics land (k_vae_w1_fill behind the entry guard)
__global__ __launch_bounds__(256) void k_ar_fill(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                                 const int32_t* __restrict__ indices, const int32_t* __restrict__ boff, int64_t B,
                                                 int32_t* __restrict__ cursor, int32_t* __restrict__ pairs) {
    if (boff[B] < 0) return;
    const int32_t b = blockIdx.x, row = rows[b];
    const int64_t r0 = indptr[row], r1 = indptr[row + 1];
    for (int64_t e = r0 + threadIdx.x; e < r1; e += 256) pairs[atomicAdd(cursor + indices[e], 1)] = b;
}

// ---- encoder: one workgroup (16 waves) per batch row, as k_vae_enc1 without normalisation and dropout ----
constexpr int AR_NW = 16;
template <int CPL>
__global__ __launch_bounds__(AR_NW * 64) void k_ar_enc(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ indices, const float* __restrict__ W1,
                                                       const float* __restrict__ b1, int H, float* __restrict__ h) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* part = reinterpret_cast<float4*>(smem);   // [AR_NW][H/4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const int32_t row = rows[b];
    const int64_t r0 = indptr[row], r1 = indptr[row + 1];
    const int H4 = H >> 2;
    float4 acc[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    // U entries of a wave are in flight together, and the column ids of the wave's NEXT U entries are fetched while their rows are
    // read: a long row (a popular item's, in the item variant) is a chain of dependent id -> W1-row round trips, and with one
    // workgroup per batch row that chain is the kernel's duration
    constexpr int U = CPL <= 2 ? 8 : 4;
    int32_t jn[U];
#pragma unroll
    for (int t = 0; t < U; ++t) jn[t] = r0 + wave * U + t < r1 ? indices[r0 + wave * U + t] : 0;
    for (int64_t e0 = r0 + wave * U; e0 < r1; e0 += AR_NW * U) {
        float4 tv[U][CPL];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int64_t e = e0 + t;
            const float4* wr = reinterpret_cast<const float4*>(W1 + (int64_t)jn[t] * H);
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int c = lane + q * 64;
                tv[t][q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < r1 && c < H4) tv[t][q] = wr[c];
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int64_t e = e0 + AR_NW * U + t;
            jn[t] = e < r1 ? indices[e] : 0;
        }
#pragma unroll
        for (int t = 0; t < U; ++t)                    // same summation order as one entry at a time
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                acc[q].x += tv[t][q].x;
                acc[q].y += tv[t][q].y;
                acc[q].z += tv[t][q].z;
                acc[q].w += tv[t][q].w;
            }
    }
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int c = lane + q * 64;
        if (c < H4) part[wave * H4 + c] = acc[q];
    }
    __syncthreads();
    float* hb = h + b * (int64_t)H;
    for (int c = threadIdx.x; c < H4; c += AR_NW * 64) {
        float4 t = part[c];
#pragma unroll
        for (int w = 1; w < AR_NW; ++w) {              // fixed order: run-to-run identical sums
            const float4 q = part[w * H4 + c];
            t.x += q.x;
            t.y += q.y;
            t.z += q.z;
            t.w += q.w;
        }
        const float4 bb = reinterpret_cast<const float4*>(b1)[c];
        reinterpret_cast<float4*>(hb)[c] =
            make_float4(ar_sigmoid(t.x + bb.x), ar_sigmoid(t.y + bb.y), ar_sigmoid(t.z + bb.z), ar_sigmoid(t.w + bb.w));
    }
}

// ---- decoder at the observed entries: one workgroup (16 waves) per batch row ----
// wave w takes the row's entries w, w + 16, ...; a lane owns float4 chunks lane, lane + 64, ... of the H hidden units.  The W2T row
// read for the dot is the row dh needs: it stays in registers.  dent[boff[b] + t] = d of the row's t-th entry.
template <int CPL>
__global__ __launch_bounds__(AR_NW * 64) void k_ar_dec(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ indices, const int32_t* __restrict__ boff,
                                                       const float* __restrict__ W2T, const float* __restrict__ b2,
                                                       const float* __restrict__ h, int64_t B, int H, int act, float Bd,
                                                       float* __restrict__ dent, float* __restrict__ dh, double* loss_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (boff[B] < 0) return;                                         // more entries than dent holds (k_ar_boff raised the status)
    const int H4 = H >> 2;
    float4* part = reinterpret_cast<float4*>(smem);                  // [AR_NW][H4]
    double* lred = reinterpret_cast<double*>(part + (size_t)AR_NW * H4);   // [AR_NW]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const int32_t row = rows[b];
    const int64_t r0 = indptr[row], r1 = indptr[row + 1];
    float* drow = dent + boff[b];
    const float4* hb4 = reinterpret_cast<const float4*>(h + b * (int64_t)H);
    float4 hv[CPL], acc[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int c = lane + q * 64;
        hv[q] = c < H4 ? hb4[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double lsum = 0.0;
    constexpr int U = CPL <= 2 ? 4 : 2;                              // entries of a wave in flight together; next ids fetched ahead (k_ar_enc)
    int32_t jn[U];
#pragma unroll
    for (int t = 0; t < U; ++t) jn[t] = r0 + wave * U + t < r1 ? indices[r0 + wave * U + t] : 0;
    for (int64_t e0 = r0 + wave * U; e0 < r1; e0 += AR_NW * U) {
        float4 wv[U][CPL];
        float bj[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int64_t e = e0 + t;
            const int32_t j = jn[t];
            bj[t] = e < r1 ? b2[j] : 0.f;
            const float4* wr = reinterpret_cast<const float4*>(W2T + (int64_t)j * H);
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int c = lane + q * 64;
                wv[t][q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < r1 && c < H4) wv[t][q] = wr[c];
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int64_t e = e0 + AR_NW * U + t;
            jn[t] = e < r1 ? indices[e] : 0;
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (e0 + t >= r1) break;                                 // (wave-uniform)
            float p = 0.f;
#pragma unroll
            for (int q = 0; q < CPL; ++q) p += (wv[t][q].x * hv[q].x + wv[t][q].y * hv[q].y) + (wv[t][q].z * hv[q].z + wv[t][q].w * hv[q].w);
            p = el_group_sum(p, 64);                                 // butterfly: the same bits in every lane
            const float pre = p + bj[t];
            const float r = act == AR_ACT_SIGMOID ? ar_sigmoid(pre) : pre;
            const float err = 1.0f - r;
            float d = (-2.0f * err) / Bd;
            if (act == AR_ACT_SIGMOID) d *= r * (1.0f - r);
            lsum += (double)err * (double)err;
            if (lane == 0) drow[e0 + t - r0] = d;
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                acc[q].x += d * wv[t][q].x;
                acc[q].y += d * wv[t][q].y;
                acc[q].z += d * wv[t][q].z;
                acc[q].w += d * wv[t][q].w;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int c = lane + q * 64;
        if (c < H4) part[wave * H4 + c] = acc[q];
    }
    if (lane == 0) lred[wave] = lsum;
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(dh + b * (int64_t)H);
    for (int c = threadIdx.x; c < H4; c += AR_NW * 64) {
        float4 t = part[c];
#pragma unroll
        for (int w = 1; w < AR_NW; ++w) {
            const float4 q = part[w * H4 + c];
            t.x += q.x;
            t.y += q.y;
            t.z += q.z;
            t.w += q.w;
        }
        const float4 y = hb4[c];
        dst[c] = make_float4(t.x * (y.x * (1.0f - y.x)), t.y * (y.y * (1.0f - y.y)), t.z * (y.z * (1.0f - y.z)), t.w * (y.w * (1.0f - y.w)));
    }
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < AR_NW; ++w) tot += lred[w];
        if (tot != 0.0) atomicAdd(loss_out, tot / (double)Bd);
    }
}

// d of (batch position b, item j): the entry's place in the sorted CSR row of b gives its place in dent
__device__ __forceinline__ float ar_d_of(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                         const int32_t* __restrict__ indices, const int32_t* __restrict__ boff,
                                         const float* __restrict__ dent, int b, int32_t j) {
    const int32_t row = rows[b];
    const int64_t r0 = indptr[row], r1 = indptr[row + 1];
    const int64_t p = el_lower_bound(indices, r0, r1, j);
    return (p < r1 && indices[p] == j) ? dent[boff[b] + (p - r0)] : 0.f;
}

// up to U batch positions bb[] (-1: none) with their d values: acc1 += dpre1[bb], acc2 += dd h[bb], accb += dd, in the order given
template <int CPL, int U>
__device__ __forceinline__ void ar_item_add(const int (&bb)[U], const float (&dd)[U], const float* __restrict__ h,
                                            const float* __restrict__ dpre1, int H, int lane, float4 (&acc1)[CPL], float4 (&acc2)[CPL],
                                            float& accb) {
    const int H4 = H >> 2;
    float4 v1[U][CPL], v2[U][CPL];
#pragma unroll
    for (int t = 0; t < U; ++t)
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = lane + q * 64;
            v1[t][q] = v2[t][q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (bb[t] >= 0 && c < H4) {
                v1[t][q] = reinterpret_cast<const float4*>(dpre1 + (int64_t)bb[t] * H)[c];
                v2[t][q] = reinterpret_cast<const float4*>(h + (int64_t)bb[t] * H)[c];
            }
        }
#pragma unroll
    for (int t = 0; t < U; ++t) {
        if (bb[t] < 0) continue;                                     // (wave-uniform)
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            acc1[q].x += v1[t][q].x;
            acc1[q].y += v1[t][q].y;
            acc1[q].z += v1[t][q].z;
            acc1[q].w += v1[t][q].w;
            acc2[q].x += dd[t] * v2[t][q].x;
            acc2[q].y += dd[t] * v2[t][q].y;
            acc2[q].z += dd[t] * v2[t][q].z;
            acc2[q].w += dd[t] * v2[t][q].w;
        }
        accb += dd[t];
    }
}

// ---- item side, LIGHT items (at most AR_LIGHT batch rows): one wave per item, four items per workgroup, no LDS ----
// lane t < n holds list entry t and finds its d; the entry's rank among the positions gives the ascending order
template <int CPL>
__global__ __launch_bounds__(256) void k_ar_item_light(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ indices, const int32_t* __restrict__ boff,
                                                       const int32_t* __restrict__ off, const int32_t* __restrict__ pairs,
                                                       const float* __restrict__ dent, const float* __restrict__ h,
                                                       const float* __restrict__ dpre1, int64_t N, int H, int64_t B,
                                                       float* __restrict__ gW1, float* __restrict__ gW2T, float* __restrict__ gb2) {
    if (boff[B] < 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= N) return;
    const int o0 = off[item], n = off[item + 1] - o0;
    if (n > AR_LIGHT) return;                                        // k_ar_item_heavy writes this row
    const int H4 = H >> 2;
    float4 acc1[CPL], acc2[CPL];
    float accb = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) acc1[q] = acc2[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) {
        const int myb = lane < n ? pairs[o0 + lane] : 0x7fffffff;
        const float myd = lane < n ? ar_d_of(rows, indptr, indices, boff, dent, myb, (int32_t)item) : 0.f;
        int rank = 0;
        for (int t = 0; t < n; ++t) rank += (__shfl(myb, t, 64) < myb) ? 1 : 0;      // batch positions are distinct
        constexpr int U = CPL <= 2 ? 4 : 2;
        for (int k0 = 0; k0 < n; k0 += U) {
            int bb[U];
            float dd[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const u64 who = __ballot(lane < n && rank == k0 + t);
                const int src = who ? __ffsll((long long)who) - 1 : 0;
                bb[t] = who ? __shfl(myb, src, 64) : -1;
                dd[t] = who ? __shfl(myd, src, 64) : 0.f;
            }
            ar_item_add<CPL, U>(bb, dd, h, dpre1, H, lane, acc1, acc2, accb);
        }
    }
    float4* d1 = reinterpret_cast<float4*>(gW1 + item * (int64_t)H);
    float4* d2 = reinterpret_cast<float4*>(gW2T + item * (int64_t)H);
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int c = lane + q * 64;
        if (c < H4) d1[c] = acc1[q], d2[c] = acc2[q];
    }
    if (lane == 0) gb2[item] = accb;
}

// ---- item side, HEAVY items (listed by k_vae_w1_scan): a fixed grid walks the list, one workgroup (8 waves) per item ----
// The item's batch positions become presence BITS in LDS; wave w walks its contiguous range of positions ascending, 64 at a time:
// the lanes of the present positions find their d side by side, then the rows are added one after the other (U in flight).  The 8
// partial rows of both tables are combined in wave order.  LDS at H = 1024: 2 tables x 8 waves x 4 KiB = 64 KiB, + B / 8 bytes of
// presence bits (32 KiB at the largest batch) -- 16 waves would ask for 128 KiB + bits, more than the 160 KiB of a CU leave room for.
constexpr int AR_HNW = 8;
template <int CPL>
__global__ __launch_bounds__(AR_HNW * 64) void k_ar_item_heavy(const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr,
                                                               const int32_t* __restrict__ indices, const int32_t* __restrict__ boff,
                                                               const int32_t* __restrict__ off, const int32_t* __restrict__ pairs,
                                                               const float* __restrict__ dent, const float* __restrict__ h,
                                                               const float* __restrict__ dpre1, int H, int64_t B, int nwords,
                                                               float* __restrict__ gW1, float* __restrict__ gW2T, float* __restrict__ gb2,
                                                               const int32_t* __restrict__ heavy) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (boff[B] < 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H4 = H >> 2;
    float4* p1 = reinterpret_cast<float4*>(smem);                    // [AR_HNW][H4]
    float4* p2 = p1 + (size_t)AR_HNW * H4;                           // [AR_HNW][H4]
    float* pb = reinterpret_cast<float*>(p2 + (size_t)AR_HNW * H4);  // [AR_HNW]
    u32* bits = reinterpret_cast<u32*>(pb + AR_HNW);                 // [2 nwords]: positions 64 w .. 64 w + 63 in words 2 w, 2 w + 1
    const int nh = heavy[0];
    const int wpw = (nwords + AR_HNW - 1) / AR_HNW;                  // 64-position words per wave
    for (int hi = blockIdx.x; hi < nh; hi += gridDim.x) {
        const int64_t item = heavy[1 + hi];
        const int o0 = off[item], n = off[item + 1] - o0;
        __syncthreads();                                             // (the previous item's partials and bits have been read)
        for (int t = tid; t < 2 * nwords; t += AR_HNW * 64) bits[t] = 0u;
        __syncthreads();
        for (int t = tid; t < n; t += AR_HNW * 64) {
            const int b = pairs[o0 + t];
            atomicOr(&bits[b >> 5], 1u << (b & 31));
        }
        __syncthreads();
        float4 acc1[CPL], acc2[CPL];
        float accb = 0.f;
#pragma unroll
        for (int q = 0; q < CPL; ++q) acc1[q] = acc2[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int w1 = (wave + 1) * wpw < nwords ? (wave + 1) * wpw : nwords;
        for (int w = wave * wpw; w < w1; ++w) {
            const int b = w * 64 + lane;
            const bool here = ((bits[b >> 5] >> (b & 31)) & 1u) != 0u;
            u64 m = __ballot(here);
            if (!m) continue;
            const float myd = here ? ar_d_of(rows, indptr, indices, boff, dent, b, (int32_t)item) : 0.f;
            constexpr int U = CPL <= 2 ? 4 : 2;
            while (m) {
                int bb[U];
                float dd[U];
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    bb[t] = -1;
                    dd[t] = 0.f;
                    if (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        bb[t] = w * 64 + src;
                        dd[t] = __shfl(myd, src, 64);
                    }
                }
                ar_item_add<CPL, U>(bb, dd, h, dpre1, H, lane, acc1, acc2, accb);
            }
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = lane + q * 64;
            if (c < H4) p1[wave * H4 + c] = acc1[q], p2[wave * H4 + c] = acc2[q];
        }
        if (lane == 0) pb[wave] = accb;
        __syncthreads();
        float4* d1 = reinterpret_cast<float4*>(gW1 + item * (int64_t)H);
        float4* d2 = reinterpret_cast<float4*>(gW2T + item * (int64_t)H);
        for (int c = tid; c < 2 * H4; c += AR_HNW * 64) {
            const float4* src = c < H4 ? p1 + c : p2 + (c - H4);
            float4 t = src[0];
#pragma unroll
            for (int w = 1; w < AR_HNW; ++w) {
                const float4 q = src[w * H4];
                t.x += q.x;
                t.y += q.y;
                t.z += q.z;
                t.w += q.w;
            }
            if (c < H4) d1[c] = t;
            else d2[c - H4] = t;
        }
        if (tid == 0) {
            float t = pb[0];
            for (int w = 1; w < AR_HNW; ++w) t += pb[w];
            gb2[item] = t;
        }
    }
}

// ---- Keras dense Adam on the four variables from one launch (k_adam_apply_oct's arithmetic and access pattern) ----
struct ArAdam {
    float* th[4];
    float* g[4];
    float* m[4];
    float* v[4];
    int64_t n[4];
};
__global__ __launch_bounds__(256) void k_ar_adam(ArAdam t, float alpha, float b1, float b2, float eps) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        float *th = t.th[k], *g = t.g[k], *m = t.m[k], *v = t.v[k];
        const int64_t n = t.n[k];
        int64_t done = 0;
        if ((((uintptr_t)th | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
            f4 *th4 = reinterpret_cast<f4*>(th), *m4 = reinterpret_cast<f4*>(m), *v4 = reinterpret_cast<f4*>(v);
            const f4* g4 = reinterpret_cast<const f4*>(g);
            const int64_t n4 = n >> 2;
            for (int64_t e = tid; e < n4; e += stride) {
                f4 a = __builtin_nontemporal_load(th4 + e), mm = __builtin_nontemporal_load(m4 + e), vv = __builtin_nontemporal_load(v4 + e);
                const f4 gg = __builtin_nontemporal_load(g4 + e);
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    mm[x] = mm[x] + (gg[x] - mm[x]) * omb1;
                    vv[x] = vv[x] + (gg[x] * gg[x] - vv[x]) * omb2;
                    a[x] = a[x] - (mm[x] * alpha) / (sqrtf(vv[x]) + eps);
                }
                __builtin_nontemporal_store(a, th4 + e);
                __builtin_nontemporal_store(mm, m4 + e);
                __builtin_nontemporal_store(vv, v4 + e);
            }
            done = n4 << 2;
        }
        for (int64_t e = done + tid; e < n; e += stride) {
            const float gg = g[e];
            float mm = m[e], vv = v[e];
            mm = mm + (gg - mm) * omb1;
            vv = vv + (gg * gg - vv) * omb2;
            th[e] = th[e] - (mm * alpha) / (sqrtf(vv) + eps);
            m[e] = mm;
            v[e] = vv;
        }
    }
}

// ---- C[r, c] <- act(C[r, c] + bias[r]): the item variant's block of scores W2T[u] . h[i] gets the decoder bias of its ROW ----
__global__ __launch_bounds__(256) void k_ar_rowbias_act(float* __restrict__ C, int64_t M, int64_t N, int64_t ldc,
                                                        const float* __restrict__ bias, int act) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, total = M * N;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t r = t / N, c = t - r * N;
        const float x = C[r * ldc + c] + bias[r];
        C[r * ldc + c] = act == AR_ACT_SIGMOID ? ar_sigmoid(x) : x;
    }
}

// ---- host ----
struct ArWs {           // status word; per-item counts, offsets, cursors, the heavy list; the batch rows' offsets; the transposed lists
    int32_t *status, *cnt, *off, *cursor, *heavy, *boff, *pairs;
};
size_t ar_carve(int64_t N, int64_t Bmax, int64_t nnz_max, void* base, ArWs* w) {
    ElCarve c{(char*)base};
    w->status = c.take<int32_t>(1);
    w->cnt = c.take<int32_t>((size_t)N + 1);
    w->off = c.take<int32_t>((size_t)N + 1);
    w->cursor = c.take<int32_t>((size_t)N + 1);
    w->heavy = c.take<int32_t>((size_t)N + 1);
    w->boff = c.take<int32_t>((size_t)Bmax + 1);
    w->pairs = c.take<int32_t>((size_t)(nnz_max > 0 ? nnz_max : 1));
    return c.off;
}

int ar_check(const el_autorec_state* st, int64_t B) {
    EL_REQUIRE(st != nullptr, "el_autorec: null state");
    EL_REQUIRE(st->N >= 1 && st->N < 0x7fffffffLL && st->H >= 4 && st->H % 4 == 0, "el_autorec: bad dims (H must be a multiple of 4)");
    EL_REQUIRE(st->H <= 1024, "el_autorec: hidden_neuron > 1024 unsupported in this build");
    EL_REQUIRE(st->out_act == 0 || st->out_act == AR_ACT_SIGMOID, "el_autorec: out_act must be 0 (linear) or 3 (sigmoid)");
    EL_REQUIRE(st->Bmax >= 1 && st->Bmax <= AR_MAX_B, "el_autorec: Bmax %lld exceeds the limit of %lld batch rows", (long long)st->Bmax,
               (long long)AR_MAX_B);
    EL_REQUIRE(B >= 1 && B <= st->Bmax, "el_autorec: batch %lld exceeds Bmax %lld", (long long)B, (long long)st->Bmax);
    EL_REQUIRE(st->nnz_max >= 0 && st->nnz_max < 0x7fffffffLL, "el_autorec: bad nnz_max");
    for (int t = 0; t < 4; ++t) EL_REQUIRE(st->w[t] != nullptr, "el_autorec: null variable %d", t);
    EL_REQUIRE((((uintptr_t)st->w[0] | (uintptr_t)st->w[1] | (uintptr_t)st->w[2]) & 15) == 0, "el_autorec: variables must be 16-byte aligned");
    return 0;
}

template <class K>
int ar_lds(K kern, size_t lds) {
    if (lds > 48 * 1024) EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return 0;
}

#define AR_BY_CPL(H_, CALL)                      \
    do {                                         \
        const int cpl_ = ((H_) / 4 + 63) / 64;   \
        if (cpl_ <= 1) { CALL(1); }              \
        else if (cpl_ <= 2) { CALL(2); }         \
        else if (cpl_ <= 3) { CALL(3); }         \
        else { CALL(4); }                        \
    } while (0)

int ar_encode(hipStream_t s, const el_autorec_state* st, const int64_t* indptr, const int32_t* indices, const int32_t* rows, int64_t B,
              float* out) {
    const size_t lds = (size_t)st->H * 4 * AR_NW;
#define AR_ENC(C_)                                                                                                            \
    if (int rc = ar_lds(k_ar_enc<C_>, lds)) return rc;                                                                       \
    EL_LAUNCH("k_ar_enc", (k_ar_enc<C_>), dim3((unsigned)B), dim3(AR_NW * 64), lds, s, rows, indptr, indices, st->w[0], st->w[1], st->H, out)
    AR_BY_CPL(st->H, AR_ENC);
#undef AR_ENC
    return 0;
}

int ar_grads(el_ctx* ctx, hipStream_t s, const el_autorec_state* st, const int64_t* indptr, const int32_t* indices, const int32_t* rows,
             int64_t B, int64_t Bd, double* loss_out) {
    if (int rc = ar_check(st, B)) return rc;
    EL_REQUIRE(indptr && indices && rows && loss_out && Bd >= B, "el_autorec: bad arguments");
    for (int t = 0; t < 4; ++t) EL_REQUIRE(st->g[t], "el_autorec: gradient buffers missing");
    EL_REQUIRE(st->h && st->dh && st->d, "el_autorec: activation buffers missing");
    EL_REQUIRE((((uintptr_t)st->h | (uintptr_t)st->dh | (uintptr_t)st->g[0] | (uintptr_t)st->g[2]) & 15) == 0,
               "el_autorec: buffers must be 16-byte aligned");
    ArWs w;
    const size_t need = ar_carve(st->N, st->Bmax, st->nnz_max, nullptr, &w);
    EL_REQUIRE(st->ws && st->ws_bytes >= need, "el_autorec: workspace of %zu bytes, %zu needed (el_autorec_ws_bytes)", st->ws_bytes, need);
    ar_carve(st->N, st->Bmax, st->nnz_max, st->ws, &w);
    const int H = st->H;
    const int64_t N = st->N;
    EL_LAUNCH("k_ar_boff", k_ar_boff, dim3(1), dim3(1024), 0, s, rows, indptr, B, st->nnz_max, w.boff, w.status, loss_out);
    if (int rc = ar_encode(s, st, indptr, indices, rows, B, st->h)) return rc;
    {
        const size_t lds = (size_t)H * 4 * AR_NW + AR_NW * sizeof(double);
#define AR_DEC(C_)                                                                                                                  \
    if (int rc = ar_lds(k_ar_dec<C_>, lds)) return rc;                                                                              \
    EL_LAUNCH("k_ar_dec", (k_ar_dec<C_>), dim3((unsigned)B), dim3(AR_NW * 64), lds, s, rows, indptr, indices, w.boff, st->w[2], st->w[3], \
              st->h, B, H, st->out_act, (float)Bd, st->d, st->dh, loss_out)
        AR_BY_CPL(H, AR_DEC);
#undef AR_DEC
    }
    if (int rc = el_colsum_finish(s, st->dh, (int)B, H, st->g[1])) return rc;
    // the batch transposed: per item the batch positions that hold it (any order; the item kernels put them in ascending order)
    EL_CHECK_HIP(hipMemsetAsync(w.cnt, 0, (size_t)(N + 1) * 4, s));
    EL_LAUNCH("k_vae_w1_count", k_vae_w1_count, dim3((unsigned)B), dim3(256), 0, s, rows, indptr, indices, w.cnt);
    EL_LAUNCH("k_vae_w1_scan", k_vae_w1_scan, dim3(1), dim3(1024), 0, s, w.cnt, N, w.off, w.cursor, w.heavy);
    EL_LAUNCH("k_ar_fill", k_ar_fill, dim3((unsigned)B), dim3(256), 0, s, rows, indptr, indices, w.boff, B, w.cursor, w.pairs);
    const int nwords = (int)((B + 63) / 64);
    const size_t ldsh = (size_t)2 * AR_HNW * H * 4 + AR_HNW * 4 + (size_t)nwords * 8;
    const unsigned gl = (unsigned)((N + 3) / 4), gh = (unsigned)(ctx->cus * 2);
#define AR_ITEM(C_)                                                                                                                  \
    EL_LAUNCH("k_ar_item_light", (k_ar_item_light<C_>), dim3(gl), dim3(256), 0, s, rows, indptr, indices, w.boff, w.off, w.pairs, st->d, \
              st->h, st->dh, N, H, B, st->g[0], st->g[2], st->g[3]);                                                                 \
    if (int rc = ar_lds(k_ar_item_heavy<C_>, ldsh)) return rc;                                                                       \
    EL_LAUNCH("k_ar_item_heavy", (k_ar_item_heavy<C_>), dim3(gh), dim3(AR_HNW * 64), ldsh, s, rows, indptr, indices, w.boff, w.off,   \
              w.pairs, st->d, st->h, st->dh, H, B, nwords, st->g[0], st->g[2], st->g[3], w.heavy)
    AR_BY_CPL(H, AR_ITEM);
#undef AR_ITEM
    EL_CHECK_LAUNCH();
    return 0;
}

int ar_apply(el_ctx* ctx, hipStream_t s, const el_autorec_state* st, float lr_t) {
    if (int rc = ar_check(st, 1)) return rc;
    for (int t = 0; t < 4; ++t) EL_REQUIRE(st->g[t] && st->m[t] && st->v[t], "el_autorec: optimiser buffers missing");
    const int64_t sizes[4] = {st->N * st->H, st->H, st->N * st->H, st->N};
    ArAdam t;
    for (int k = 0; k < 4; ++k) t.th[k] = st->w[k], t.g[k] = st->g[k], t.m[k] = st->m[k], t.v[k] = st->v[k], t.n[k] = sizes[k];
    int64_t blocks = (sizes[0] / 4 + 1 + 255) / 256;
    const int64_t cap = (int64_t)ctx->cus * 16;
    if (blocks > cap) blocks = cap;
    EL_LAUNCH("k_ar_adam", k_ar_adam, dim3((unsigned)blocks), dim3(256), 0, s, t, lr_t, 0.9f, 0.999f, 1e-7f);
    EL_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t el_autorec_ws_bytes(int64_t N, int64_t Bmax, int64_t nnz_max) {
    if (N < 1 || Bmax < 1 || nnz_max < 0) return 0;
    ArWs w;
    return ar_carve(N, Bmax, nnz_max, nullptr, &w);
}

extern "C" int el_autorec_grads(el_ctx* ctx, void* stream, const el_autorec_state* st, const int64_t* indptr, const int32_t* indices,
                                const int32_t* rows, int64_t B, int64_t B_global, double* loss_out) {
    if (int rc = el_bind(ctx)) return rc;
    return ar_grads(ctx, (hipStream_t)stream, st, indptr, indices, rows, B, B_global, loss_out);
}

extern "C" int el_autorec_apply(el_ctx* ctx, void* stream, const el_autorec_state* st, float lr_t) {
    if (int rc = el_bind(ctx)) return rc;
    return ar_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_autorec_train_step(el_ctx* ctx, void* stream, const el_autorec_state* st, const int64_t* indptr, const int32_t* indices,
                                     const int32_t* rows, int64_t B, float lr_t, double* loss_out) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = ar_grads(ctx, (hipStream_t)stream, st, indptr, indices, rows, B, B, loss_out)) return rc;
    return ar_apply(ctx, (hipStream_t)stream, st, lr_t);
}

extern "C" int el_autorec_encode(el_ctx* ctx, void* stream, const el_autorec_state* st, const int64_t* indptr, const int32_t* indices,
                                 const int32_t* rows, int64_t B, float* out) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = ar_check(st, 1)) return rc;
    EL_REQUIRE(indptr && indices && rows && out && B >= 1 && B < 0x7fffffffLL, "el_autorec_encode: bad arguments");
    EL_REQUIRE(((uintptr_t)out & 15) == 0, "el_autorec_encode: out must be 16-byte aligned");
    if (int rc = ar_encode((hipStream_t)stream, st, indptr, indices, rows, B, out)) return rc;
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_autorec_rowbias_act(el_ctx* ctx, void* stream, float* C, int64_t M, int64_t N, int64_t ldc, const float* bias, int act) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(C && bias && M >= 1 && N >= 1 && ldc >= N, "el_autorec_rowbias_act: bad arguments");
    EL_REQUIRE(act == 0 || act == AR_ACT_SIGMOID, "el_autorec_rowbias_act: act must be 0 (none) or 3 (sigmoid)");
    EL_LAUNCH("k_ar_rowbias_act", k_ar_rowbias_act, dim3(el_stream_grid(ctx, M * N)), dim3(256), 0, (hipStream_t)stream, C, M, N, ldc, bias, act);
    EL_CHECK_LAUNCH();
    return 0;
}
