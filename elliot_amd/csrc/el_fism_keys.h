// The sorted sample keys of the item-similarity steps (el_fism.hip, el_nais.hip): users as u, items as U + i in ONE stable radix sort,
// the head of every user segment, the slot of every distinct user of the batch, the piece count of a cut list and the length of a
// sorted segment.  Included inside the anonymous namespace of the file that uses it.
#pragma once

// pieces of a list of len positions as the scanned count: low word pieces, high word the same where there is more than one
__device__ __forceinline__ u64 fi_plen(int64_t len, int piece) {
    const u64 np = len <= piece ? 1ull : (u64)((len + piece - 1) / piece);
    return np | (np > 1 ? np << 32 : 0ull);
}
__device__ __forceinline__ int64_t fi_lo(u64 v) { return (int64_t)(u32)v; }

// users as u, items as U + i; the counters of the two combine passes and the piece counts of the slots start at zero
__global__ __launch_bounds__(256) void k_fism_keys(const int32_t* __restrict__ u, const int32_t* __restrict__ i, int64_t B, u32 U,
                                                   u32* __restrict__ key, u32* __restrict__ val, int32_t* split_u, int32_t* split_i,
                                                   u64* __restrict__ plen, int64_t n_max) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b == 0) split_u[0] = 0, split_i[0] = 0;
    for (int64_t t = b; t <= n_max; t += (int64_t)gridDim.x * 256) plen[t] = 0ull;
    if (b >= B) return;
    key[b] = (u32)u[b], val[b] = (u32)b;
    key[B + b] = U + (u32)i[b], val[B + b] = (u32)b;
}

__global__ __launch_bounds__(256) void k_fism_heads(const u32* __restrict__ keys, int64_t n, int32_t* __restrict__ hd) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    hd[p] = (p == 0 || keys[p - 1] != keys[p]) ? 1 : 0;
}

// the head of every user segment: the user's slot (hs = the exclusive scan of hd), the slot's user and its pieces
__global__ __launch_bounds__(256) void k_fism_users(const u32* __restrict__ keys, const int32_t* __restrict__ hd, const int32_t* __restrict__ hs,
                                                    int64_t B, int64_t U, int64_t n_max, const int64_t* __restrict__ h_indptr, int piece,
                                                    int32_t* __restrict__ rows, int32_t* __restrict__ slot, u64* __restrict__ plen,
                                                    int32_t* __restrict__ n_out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= B) return;
    if (p == B - 1) *n_out = hs[p] + hd[p];
    if (!hd[p]) return;
    const int64_t user = (int64_t)keys[p], sl = hs[p];
    if (user >= U || sl >= n_max) return;                        // (an id past the table writes nothing outside the map)
    rows[sl] = (int32_t)user;
    slot[user] = (int32_t)sl;
    plen[sl] = fi_plen(h_indptr[user + 1] - h_indptr[user], piece);
}

// first position of `key` in the sorted keys (n where it is absent and larger than all)
__device__ __forceinline__ int64_t fi_first(const u32* __restrict__ keys, int64_t n, u32 key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// samples of one row: the positions of its key in the sorted keys of its side
__device__ __forceinline__ int fi_count(const u32* __restrict__ keys, int64_t n, u32 key) {
    int64_t lo = fi_first(keys, n, key), hi = n;
    const int64_t first = lo;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return (int)(lo - first);
}
