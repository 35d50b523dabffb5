// Attribute-aware baselines (AttributeItemKNN / AttributeUserKNN / VSM): what they need beside el_knn.hip (whose el_knn_build_f32
// turns the profile rows into W).
//
//   el_profile_build   user profiles over item features -- the reference's Python dict loops (compute_binary_profile of
//                      attribute_user_knn.py / vector_space_model.py, TFIDF.get_profiles of both tfidf_utils.py) -- as a CSR
//
// Numerics contract (tests/helpers/attr_ref.py restates it in NumPy):
//   profile  one fp64 cell per (user, feature); the user's items are taken in stored order (train_dict order);
//            ADD:  cell = __dadd_rn(cell, w) from +0 per item that carries the feature, w = __ddiv_rn(1, len) (or 1);
//            LAST: cell = weight of the feature in the last item that carries it, then __ddiv_rn(cell, len) (or as it is);
//            an entry for every feature touched (zeros kept), columns ascending, value rounded once to float
// No float atomics: every cell is written by one lane per step and the steps are ordered by the wave's own LDS order, so the
// same input gives the same bytes on every run.
#include "el_common.h"

#include "el_knn_csr.h"

#define ATTR_TILE 8192                            // fp64 cells per LDS tile (64 KiB)

namespace {

struct Profile {
    const int64_t* rp;   // users -> items, stored (train_dict) order
    const int32_t* ri;
    const int64_t* fp;   // items -> features (distinct inside an item, any order)
    const int32_t* fi;
    const double* fv;    // weights (LAST)
    int64_t n_items, n_features;
    int mode, by_len, tile;
    int32_t* rowcnt;         // count pass: entries per user
    const int64_t* indptr;   // fill pass
    int64_t cap;
    int32_t* out_idx;
    float* out_val;
};

// One wave per user, one tile of the feature range at a time: the user's items sequentially, lanes across the item's features
// (distinct: one write per cell per item), a bitmap of the cells touched.  FILL = false only counts the touched cells.
template <bool FILL>
__global__ __launch_bounds__(64) void k_profile(Profile p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* cell = reinterpret_cast<double*>(smem);                                          // [tile] (FILL)
    u32* bits = reinterpret_cast<u32*>(smem + (FILL ? (size_t)p.tile * 8 : 0));              // [tile / 32]
    const int lane = threadIdx.x;
    const int64_t u = blockIdx.x;
    const int64_t r0 = p.rp[u], r1 = p.rp[u + 1];
    const double len = (double)(r1 - r0);
    const double w = p.by_len ? __ddiv_rn(1.0, len) : 1.0;
    const int nwd_max = p.tile >> 5;
    int64_t base = FILL ? p.indptr[u] : 0;
    const bool room = !FILL || p.indptr[u + 1] <= p.cap;          // a caller that sized the output too small gets no stray write
    int total = 0;
    for (int64_t f0 = 0; f0 < p.n_features; f0 += p.tile) {
        const int64_t f1 = f0 + p.tile < p.n_features ? f0 + p.tile : p.n_features;
        const int wd = (int)(f1 - f0);
        const int nwd = (wd + 31) >> 5;
        for (int i = lane; i < nwd_max; i += 64) bits[i] = 0u;
        if (FILL)
            for (int i = lane; i < wd; i += 64) cell[i] = 0.0;
        el_wave_lds_sync();
        for (int64_t e = r0; e < r1; ++e) {
            const int32_t item = p.ri[e];
            if (item < 0 || item >= p.n_items) continue;          // (wave-uniform)
            const int64_t a0 = p.fp[item], a1 = p.fp[item + 1];
            for (int64_t a = a0 + lane; a < a1; a += 64) {
                const int64_t f = p.fi[a];
                if (f < f0 || f >= f1) continue;
                const int j = (int)(f - f0);
                atomicOr(&bits[j >> 5], 1u << (j & 31));
                if (FILL) cell[j] = p.mode == EL_PROFILE_ADD ? __dadd_rn(cell[j], w) : p.fv[a];
            }
            el_wave_lds_sync();
        }
        // lane l ranks the words [l * per, (l + 1) * per) of the bitmap behind the words of the lanes before it
        const int per = (nwd + 63) >> 6;
        const int w0 = lane * per < nwd ? lane * per : nwd, w1 = w0 + per < nwd ? w0 + per : nwd;
        int s = 0;
        for (int x = w0; x < w1; ++x) s += __popc(bits[x]);
        int incl = s;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const int tile_total = __shfl(incl, 63, 64);
        if (FILL && room) {
            int64_t pos = base + incl - s;
            for (int x = w0; x < w1; ++x) {
                u32 b = bits[x];
                while (b) {
                    const int j = (x << 5) + __builtin_ctz(b);
                    b &= b - 1u;
                    const double v = cell[j];
                    p.out_idx[pos] = (int32_t)(f0 + j);
                    p.out_val[pos] = (float)((p.mode == EL_PROFILE_LAST && p.by_len) ? __ddiv_rn(v, len) : v);
                    ++pos;
                }
            }
        }
        base += tile_total;
        total += tile_total;
        el_wave_lds_sync();
    }
    if (!FILL && lane == 0) p.rowcnt[u] = total;
}

struct ProfileWs {      // entries per user, and the cursor array k_knn_scan fills beside the indptr
    int32_t* rowcnt;
    int64_t* cursor;
};
size_t profile_carve(int64_t U, void* base, ProfileWs* w) {
    ElCarve c{(char*)base};
    w->rowcnt = c.take<int32_t>((size_t)U);
    w->cursor = c.take<int64_t>((size_t)U);
    return c.off;
}

int attr_tile(int64_t n) { return (int)(n < ATTR_TILE ? ((n + 63) / 64) * 64 : ATTR_TILE); }

}  // namespace

extern "C" size_t el_profile_ws_bytes(int64_t n_users) {
    if (n_users <= 0) return 0;
    ProfileWs w;
    return profile_carve(n_users, nullptr, &w);
}

extern "C" int el_profile_build(el_ctx* ctx, void* stream, const int64_t* r_indptr, const int32_t* r_indices, const int64_t* f_indptr,
                                const int32_t* f_indices, const double* f_vals, int64_t n_users, int64_t n_items, int64_t n_features,
                                int mode, int by_len, int64_t* out_indptr, int32_t* out_indices, float* out_vals, int64_t out_cap,
                                void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(r_indptr && r_indices && f_indptr && f_indices, "el_profile_build: null input pointer");
    EL_REQUIRE(mode == EL_PROFILE_ADD || mode == EL_PROFILE_LAST, "el_profile_build: mode %d unsupported (EL_PROFILE_ADD, EL_PROFILE_LAST)",
               mode);
    EL_REQUIRE(mode == EL_PROFILE_ADD || f_vals, "el_profile_build: EL_PROFILE_LAST needs the feature weights");
    EL_REQUIRE(out_indptr && out_indices && out_vals, "el_profile_build: null output pointer");
    EL_REQUIRE(n_users >= 1 && n_users < 0x7fffffffLL && n_items >= 1 && n_items < 0x7fffffffLL && n_features >= 1 &&
                   n_features < 0x7fffffffLL,
               "el_profile_build: bad sizes users=%lld items=%lld features=%lld", (long long)n_users, (long long)n_items,
               (long long)n_features);
    EL_REQUIRE(out_cap >= 0, "el_profile_build: bad output capacity");
    ProfileWs w;
    const size_t need = profile_carve(n_users, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_profile_build: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    Profile p;
    p.rp = r_indptr, p.ri = r_indices, p.fp = f_indptr, p.fi = f_indices, p.fv = f_vals;
    p.n_items = n_items, p.n_features = n_features, p.mode = mode, p.by_len = by_len ? 1 : 0;
    p.tile = attr_tile(n_features);
    p.rowcnt = w.rowcnt, p.indptr = out_indptr, p.cap = out_cap, p.out_idx = out_indices, p.out_val = out_vals;
    const size_t lds_bits = (size_t)(p.tile >> 5) * 4, lds_fill = (size_t)p.tile * 8 + lds_bits;
    EL_LAUNCH("k_profile_count", k_profile<false>, dim3((unsigned)n_users), dim3(64), lds_bits, st, p);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_knn_scan", k_knn_scan, dim3(1), dim3(1024), 0, st, (const int32_t*)w.rowcnt, n_users, out_indptr, w.cursor);
    EL_CHECK_LAUNCH();
    EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_profile<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_fill));
    EL_LAUNCH("k_profile_fill", k_profile<true>, dim3((unsigned)n_users), dim3(64), lds_fill, st, p);
    EL_CHECK_LAUNCH();
    return 0;
}
