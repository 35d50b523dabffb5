// KaHFM (knowledge-aware hybrid factorisation machine): the start tables of KAHFMModel.initialize (kahfm_model.py:47-72) as dense
// fp64 matrices on the device.  Training is el_bprsgd_apply (el_bpr.hip / el_bprsgd_wide.hip), scoring el_score_topk_f64.
//
//   el_kahfm_init   Q0[i, f] = w(i, f); P0[u, f] = w(last item of row u that carries f, f) / len(row u)
//
// Numerics contract (tests/helpers/kahfm_ref.py restates it in NumPy):
//   Q0   the weight as it is where the item carries the feature, +0.0 elsewhere
//   P0   the user's items in stored order (train_dict order), one write per cell per item (an item's features are distinct), a
//        workgroup barrier between items: the last writer wins, as in TFIDF.get_profiles; then __ddiv_rn(cell, len) for every
//        cell of the row (an untouched cell is +0.0 / len = +0.0); a user with an empty row gets +0.0 everywhere
// No atomics: every cell is written by one lane per step, so the same input gives the same bytes on every run.
#include "el_common.h"

#define KAHFM_TILE 8192                           // fp64 cells per LDS tile (64 KiB)
#define KAHFM_THREADS 256

namespace {

struct KahfmInit {
    const int64_t* rp;   // users -> items, stored (train_dict) order
    const int32_t* ri;
    const int64_t* fp;   // items -> features (distinct inside an item, any order)
    const int32_t* fi;
    const double* fv;
    int64_t n_items, n_features;
    int tile;
    double *P0, *Q0;
};

// One workgroup per item: its lanes across the item's features.  Q0 was zeroed before.
__global__ __launch_bounds__(KAHFM_THREADS) void k_kahfm_items(KahfmInit p) {
    const int64_t i = blockIdx.x;
    double* row = p.Q0 + i * p.n_features;
    for (int64_t a = p.fp[i] + threadIdx.x; a < p.fp[i + 1]; a += KAHFM_THREADS) {
        const int64_t f = p.fi[a];
        if (f >= 0 && f < p.n_features) row[f] = p.fv[a];
    }
}

// One workgroup per user, one tile of the feature range at a time: the user's items sequentially, lanes across the item's
// features, then the whole tile divided by the row length and written out (every cell of the row is written exactly once).
__global__ __launch_bounds__(KAHFM_THREADS) void k_kahfm_users(KahfmInit p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* cell = reinterpret_cast<double*>(smem);                // [tile]
    const int tid = threadIdx.x;
    const int64_t u = blockIdx.x;
    const int64_t r0 = p.rp[u], r1 = p.rp[u + 1];
    const double len = (double)(r1 - r0);
    double* row = p.P0 + u * p.n_features;
    for (int64_t f0 = 0; f0 < p.n_features; f0 += p.tile) {
        const int64_t f1 = f0 + p.tile < p.n_features ? f0 + p.tile : p.n_features;
        const int wd = (int)(f1 - f0);
        for (int c = tid; c < wd; c += KAHFM_THREADS) cell[c] = 0.0;
        __syncthreads();
        for (int64_t e = r0; e < r1; ++e) {
            const int32_t item = p.ri[e];
            if (item < 0 || item >= p.n_items) continue;           // (workgroup-uniform)
            for (int64_t a = p.fp[item] + tid; a < p.fp[item + 1]; a += KAHFM_THREADS) {
                const int64_t f = p.fi[a];
                if (f >= f0 && f < f1) cell[f - f0] = p.fv[a];
            }
            __syncthreads();
        }
        for (int c = tid; c < wd; c += KAHFM_THREADS) row[f0 + c] = r1 > r0 ? __ddiv_rn(cell[c], len) : 0.0;
        __syncthreads();
    }
}

}  // namespace

extern "C" int el_kahfm_init(el_ctx* ctx, void* stream, const int64_t* r_indptr, const int32_t* r_indices, const int64_t* f_indptr,
                             const int32_t* f_indices, const double* f_vals, int64_t n_users, int64_t n_items, int64_t n_features,
                             double* P0, double* Q0) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(r_indptr && r_indices && f_indptr && f_indices && f_vals, "el_kahfm_init: null input pointer");
    EL_REQUIRE(P0 && Q0, "el_kahfm_init: null output pointer");
    EL_REQUIRE(n_users >= 1 && n_users < 0x7fffffffLL && n_items >= 1 && n_items < 0x7fffffffLL && n_features >= 1 &&
                   n_features < 0x7fffffffLL,
               "el_kahfm_init: bad sizes users=%lld items=%lld features=%lld", (long long)n_users, (long long)n_items,
               (long long)n_features);
    hipStream_t st = (hipStream_t)stream;
    KahfmInit p;
    p.rp = r_indptr, p.ri = r_indices, p.fp = f_indptr, p.fi = f_indices, p.fv = f_vals;
    p.n_items = n_items, p.n_features = n_features, p.P0 = P0, p.Q0 = Q0;
    p.tile = (int)(n_features < KAHFM_TILE ? n_features : KAHFM_TILE);
    EL_CHECK_HIP(hipMemsetAsync(Q0, 0, (size_t)n_items * (size_t)n_features * sizeof(double), st));
    EL_LAUNCH("k_kahfm_items", k_kahfm_items, dim3((unsigned)n_items), dim3(KAHFM_THREADS), 0, st, p);
    EL_CHECK_LAUNCH();
    const size_t lds = (size_t)p.tile * sizeof(double);
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_kahfm_users), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    EL_LAUNCH("k_kahfm_users", k_kahfm_users, dim3((unsigned)n_users), dim3(KAHFM_THREADS), lds, st, p);
    EL_CHECK_LAUNCH();
    return 0;
}
