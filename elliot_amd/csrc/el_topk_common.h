// Shared pieces of the top-k kernels (el_topk.hip, el_topk_screen.hip, el_nmf_score.hip) and the ONE one-wave selection of the
// project: the running best k of a stream of (value, index) pairs, ordered (value desc, index asc).  ElWaveSelect<Key> appends
// what its caller's predicate lets in to a cap-slot LDS buffer, 64 lanes a pass, and whenever a further pass might not fit it
// sorts the buffer (one-wave bitonic network), keeps the best k and hands back the value of the k-th as the new threshold.
// The count lives in registers (it is wave-uniform).  Two key policies own the LDS layout, the empty slot, compare-and-swap and
// the threshold:
//   ElPackedKey      one u64 per slot, el_make_key(fp32 value, index); empty = 0.  k_topk_wave<float>, k_knn_score, the SLIM
//                    cut, k_rp3_coltop.
//   ElPairKey<V>     a u64 primary array and a u32 secondary (~index) behind it; empty = (0, 0).  V = double: primary =
//                    el_d2ord(value), threshold a double (k_topk_wave<double>); V = u64: the caller's ready-made primary,
//                    threshold that key, 0 while fewer than k are held (k_rp3_slice, k_rp3_merge).
// Keys of distinct indices are distinct, so the sorted buffer does not depend on the network.
#pragma once
#include "el_common.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

// T = float: every top-k route; T = double: the wave kernel alone (the fp64 entry points leave the list and split fields zero)
template <class T>
struct TopkParamsT {
    const T* Gu;
    const T* Gi;
    const T* Bi;
    int64_t u_start, u_stop, item_offset, I_local;
    int F;
    const int64_t* excl_indptr;
    const int32_t* excl_indices;
    const int64_t* cand_indptr;
    const int32_t* cand_indices;
    int k;
    int32_t* out_idx;
    T* out_val;
    // dense-preds variant
    const T* preds;
    int64_t ld;
    int dbg;  // experiment switches (EL_TOPK_DEBUG): 1 = skip the fused selection (GEMM-only timing)
    const int32_t* ulist;         // MFMA kernel: if set, process users u_start + ulist[skip .. min(*ulist_n, max)) instead of the range
    const int32_t* ulist_n;
    int ulist_skip, ulist_max;    // (ulist_max == 0: no upper limit)
    // MFMA kernel, item-split mode (gridDim.y = nsplit > 1): split s scores its slice of the item tiles and writes the
    // partial list of list entry e to row s * part_stride + e of out_idx / out_val (merged by k_topk_merge afterwards)
    int nsplit;
    int64_t part_stride;
};
typedef TopkParamsT<float> TopkParams;

// defined in el_topk.hip: fp32 MFMA kernel (must be eligible: F <= 256, k <= 40, no candidate list); honours p.ulist
int el_topk_launch_mfma(const TopkParams& p, hipStream_t st);
// defined in el_topk.hip: exact top-k of the users in p.ulist (device list, *p.ulist_n entries), parallel over users AND
// item slices so that a handful of users does not serialise on one workgroup.  Its scratch is nested in the caller's workspace.
struct TopkListWs {
    int32_t* part_idx;     // [LIST_SPLIT, list cap, k] partial lists of the item slices
    float* part_val;
    float* preds;          // [LIST_DENSE, I_local] scores of the dense tier
};
TopkListWs el_topk_list_carve(ElCarve& c, int64_t n_users, int64_t I_local, int k);
int el_topk_run_list(const TopkParams& p, const TopkListWs& scratch, hipStream_t st);
// defined in el_topk_screen.hip: the bf16-screened route of el_score_topk
bool el_topk_screen_eligible(int F, int k, const void* cand);
size_t el_topk_screen_ws_bytes(int64_t n_users, int64_t I_local, int F, int k, int64_t excl_nnz);
int el_topk_screen_run(const TopkParams& p, void* ws, size_t ws_bytes, hipStream_t st, bool items_unchanged);

// ---- key policies ---------------------------------------------------------------------
struct ElPackedKey {
    typedef float Value;
    u64* a;                                                     // [cap]
    __device__ __forceinline__ ElPackedKey(u64* a_) : a(a_) {}
    __device__ __forceinline__ ElPackedKey(void* lds, int) : a(reinterpret_cast<u64*>(lds)) {}
    static size_t lds_bytes(int cap) { return (size_t)cap * 8; }
    static __device__ __forceinline__ float lowest() { return -INFINITY; }
    __device__ __forceinline__ void put(int t, float v, int32_t index) const { a[t] = el_make_key(v, index); }
    __device__ __forceinline__ void clear(int t) const { a[t] = 0ull; }
    __device__ __forceinline__ float value(int t) const { return el_key_score(a[t]); }
    __device__ __forceinline__ int32_t index(int t) const { return el_key_item(a[t]); }
    // slots i < j of a bitonic step: the larger key goes to i (desc) or to j.  Both compares first, then the choice: with the
    // choice around the compares the sort's inner loop compiles to branches (profiles/topk_select_refactor.md)
    __device__ __forceinline__ void cas(int i, int j, bool desc) const {
        const u64 x = a[i], y = a[j];
        const bool lt = x < y, gt = x > y;
        if (desc ? lt : gt) {
            a[i] = y;
            a[j] = x;
        }
    }
};

// what a pair key's primary is made of: ord(double), or the caller's u64 as it is; lowest() = the threshold below every value
template <class V>
struct ElPairValue;
template <>
struct ElPairValue<double> {
    static __device__ __forceinline__ u64 prim(double v) { return el_d2ord(v); }
    static __device__ __forceinline__ double value(u64 p) { return el_ord2d(p); }
    static __device__ __forceinline__ double lowest() { return -INFINITY; }
};
template <>
struct ElPairValue<u64> {
    static __device__ __forceinline__ u64 prim(u64 v) { return v; }
    static __device__ __forceinline__ u64 value(u64 p) { return p; }
    static __device__ __forceinline__ u64 lowest() { return 0ull; }
};

template <class V>
struct ElPairKey {
    typedef V Value;
    u64* prim;                                                  // [cap]
    u32* sec;                                                   // [cap] ~index
    __device__ __forceinline__ ElPairKey(void* lds, int cap) : prim(reinterpret_cast<u64*>(lds)), sec(reinterpret_cast<u32*>(prim + cap)) {}
    static size_t lds_bytes(int cap) { return (size_t)cap * 12; }
    static __device__ __forceinline__ V lowest() { return ElPairValue<V>::lowest(); }
    __device__ __forceinline__ void put(int t, V v, int32_t index) const {
        prim[t] = ElPairValue<V>::prim(v);
        sec[t] = 0xffffffffu - (u32)index;
    }
    __device__ __forceinline__ void clear(int t) const {
        prim[t] = 0ull;
        sec[t] = 0u;
    }
    __device__ __forceinline__ V value(int t) const { return ElPairValue<V>::value(prim[t]); }
    __device__ __forceinline__ int32_t index(int t) const { return (int32_t)(0xffffffffu - sec[t]); }
    __device__ __forceinline__ void cas(int i, int j, bool desc) const {
        const u64 x = prim[i], y = prim[j];
        const u32 sx = sec[i], sy = sec[j];
        const bool eq = x == y;                                 // (no short circuit: compares and masks, not branches)
        const bool lt = (x < y) | (eq & (sx < sy)), gt = (y < x) | (eq & (sy < sx));
        if (desc ? lt : gt) {
            prim[i] = y;
            prim[j] = x;
            sec[i] = sy;
            sec[j] = sx;
        }
    }
};

// ---- one-wave bitonic sort (best first) of n = 2^m keys held in LDS -------------------
template <class Key>
__device__ __forceinline__ void el_wave_bitonic_desc(const Key& a, int n, int lane) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (n >> 1); t += 64) {
                const int i = 2 * t - (t & (stride - 1));
                a.cas(i, i + stride, (i & size) == 0);
            }
            el_wave_lds_sync();
        }
    }
}
__device__ __forceinline__ void el_wave_bitonic_desc(u64* a, int n, int lane) { el_wave_bitonic_desc(ElPackedKey(a), n, lane); }

// Sort one candidate list (n valid keys in a cap-slot LDS buffer), keep the best k.
// Whole wave participates, all arguments wave-uniform. Returns the new threshold.
template <class Key>
__device__ __forceinline__ typename Key::Value el_wave_compact(const Key& a, int n, int cap, int k, int lane) {
    for (int t = n + lane; t < cap; t += 64) a.clear(t);
    el_wave_lds_sync();
    el_wave_bitonic_desc(a, cap, lane);
    const typename Key::Value nt = (n >= k) ? a.value(k - 1) : Key::lowest();
    el_wave_lds_sync();
    return nt;
}
// The same with the count handed over and back in LDS: the selection epilogues of el_nmf_score.hip, which flush at cap - 32
// inside register-bound MFMA kernels and keep this form instruction for instruction.
__device__ __forceinline__ float el_wave_compact(u64* kb, int* cp, int cap, int k, int lane) {
    el_wave_lds_sync();
    int n = *cp;
    for (int t = n + lane; t < cap; t += 64) kb[t] = 0ull;
    el_wave_lds_sync();
    el_wave_bitonic_desc(kb, cap, lane);
    int nn = n < k ? n : k;
    if (lane == 0) *cp = nn;
    float nt = (nn >= k) ? el_key_score(kb[k - 1]) : -INFINITY;
    el_wave_lds_sync();
    return nt;
}

// The running best k of a stream of (value, index) pairs in one wave: cap slots of Key in LDS, cnt and tau in registers
// (cap = el_select_cap(k) or any power of two >= k + 64).  The caller's hit predicate decides what enters and should refuse
// what falls below tau; every lane calls push in every pass, all members but the pushed pair wave-uniform.
template <class Key>
struct ElWaveSelect {
    Key keys;
    int cap, k;
    int cnt;
    typename Key::Value tau;

    __device__ __forceinline__ ElWaveSelect(Key keys_, int cap_, int k_) : keys(keys_), cap(cap_), k(k_), cnt(0), tau(Key::lowest()) {}

    __device__ __forceinline__ void push(bool hit, typename Key::Value v, int32_t index, int lane) {
        const u64 bal = __ballot(hit);
        if (bal) {
            const int offp = __popcll(bal & ((1ull << lane) - 1ull));
            if (hit) keys.put(cnt + offp, v, index);
            cnt += __popcll(bal);
        }
        if (cnt > cap - 64) {
            tau = el_wave_compact(keys, cnt, cap, k, lane);
            cnt = cnt < k ? cnt : k;
        }
    }

    // sorts what is left: slots [0 .. returned count) are the best, (value desc, index asc)
    __device__ __forceinline__ int finish(int lane) {
        el_wave_compact(keys, cnt, cap, k, lane);
        return cnt = cnt < k ? cnt : k;
    }
};

// Same, but first drops keys whose item is in the (sorted) exclusion row idx[e0,e1): the MFMA kernel
// inserts candidates unchecked and pays the membership test (a chain of dependent global loads) once
// per compaction for the whole buffer instead of once per insertion.  cap <= 64 here.
__device__ __forceinline__ float el_wave_compact_excl(u64* kb, int n, int& n_out, int cap, int k, int lane,
                                                      const int32_t* __restrict__ idx, int64_t e0, int64_t e1) {
    el_wave_lds_sync();
    bool drop = false;
    if (lane < cap) {
        if (lane < n) {
            if (e1 > e0) drop = el_row_contains(idx, e0, e1, el_key_item(kb[lane]));
            if (drop) kb[lane] = 0ull;
        } else {
            kb[lane] = 0ull;
        }
    }
    const int removed = __popcll(__ballot(drop));
    el_wave_lds_sync();
    el_wave_bitonic_desc(kb, cap, lane);
    n -= removed;
    int nn = n < k ? n : k;
    n_out = nn;
    float nt = (nn >= k) ? el_key_score(kb[k - 1]) : -INFINITY;
    el_wave_lds_sync();
    return nt;
}

// value held by the partner lane (l <-> l+32) -- v_permlane32_swap_b32, no LDS round trip
__device__ __forceinline__ u32 el_partner32(u32 x, int hi) {
    auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return hi ? r[0] : r[1];
}

// The r-th (0-based) masked item of a row, ascending, inside the local shard
// [off, off+I_local): what tf.where(mask, preds, -inf) + top_k pads with.
// (reads the shard and the two mask CSRs of p only)
template <class T>
__device__ __forceinline__ int32_t el_fill_masked_range(const TopkParamsT<T>& p, int64_t off, int64_t end, int64_t e0, int64_t e1,
                                                        int64_t c0, int64_t c1, int64_t r) {
    if (p.cand_indptr) {
        // masked = NOT candidate.  q* = #candidates (inside the range) with
        // cand[q] - off - q <= r ; answer = off + r + q*.
        int64_t lo = el_lower_bound(p.cand_indices, c0, c1, (int32_t)off);
        int64_t hi = el_lower_bound(p.cand_indices, c0, c1, (int32_t)(end > 0x7fffffffLL ? 0x7fffffffLL : end));
        int64_t a = lo, b = hi;
        while (a < b) {
            int64_t mid = (a + b) >> 1;
            int64_t f = (int64_t)p.cand_indices[mid] - off - (mid - lo);
            if (f <= r)
                a = mid + 1;
            else
                b = mid;
        }
        int64_t g = off + r + (a - lo);
        return g < end ? (int32_t)g : -1;
    }
    if (p.excl_indptr) {
        int64_t lo = el_lower_bound(p.excl_indices, e0, e1, (int32_t)off);
        int64_t hi = el_lower_bound(p.excl_indices, e0, e1, (int32_t)(end > 0x7fffffffLL ? 0x7fffffffLL : end));
        return (lo + r < hi) ? p.excl_indices[lo + r] : -1;
    }
    return -1;
}

template <class T>
__device__ __forceinline__ int32_t el_fill_masked(const TopkParamsT<T>& p, int64_t e0, int64_t e1, int64_t c0,
                                                  int64_t c1, int64_t r) {
    return el_fill_masked_range(p, p.item_offset, p.item_offset + p.I_local, e0, e1, c0, c1, r);
}
