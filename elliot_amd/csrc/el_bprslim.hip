// BPRSlim (Ning & Karypis' SLIM trained with the BPR criterion): per-triplet SGD on a dense fp64 item-item matrix, ordered scoring.
//
// Replaces BPRSlimModel.train_step and predict (bprslim_model.py:36-84):
//   el_bprslim_levels_host   dependency levels of a triplet sequence: a triplet reads and writes rows i and j of S, nothing else
//   el_bprslim_apply         x = sum over the seen items s of user u of (S[i, s] - S[j, s]), g = 1 / (1 + exp(x)), then
//                            S[i, s] += lr (g - li_reg S[i, s]) for s != i and S[j, s] -= lr (g - lj_reg S[j, s]) for s != j
//   el_bprslim_apply_levels  one launch of el_bprslim_apply per level, in stream order
//   el_bprslim_table         St[s, i] = S[i, s]: the scoring kernel reads one contiguous row of St per seen item
//   el_bprslim_scores        P[u, i] = +0 + St[s, i] over row u in stored order, one __dadd_rn each (predict, bit for bit)
//
// Numerics contract of el_bprslim_apply (the library is built with -ffp-contract=off: no multiply below meets an add in an fma):
//   mapping  one wave of 64 lanes per triplet, SLIM_WAVES triplets per workgroup; position p of row u belongs to lane p mod 64
//   sum      a lane adds its rounded differences S[i, s] - S[j, s] in ascending position order from +0; the 64 lane sums go
//            through the xor shuffle tree (32, 16, ..., 1).  The shape depends on the row length alone: the same input gives
//            the same bytes on every run.  No float atomics.
//   update   every lane updates the cells of its own positions with the reference's operations in its order: multiply,
//            subtract, multiply, add for row i (skipping s == i), then multiply, subtract, multiply, subtract for row j
//            (skipping s == j).  With i == j the second statement works on the value the first one stored, as the reference's.
//   loads    a lane takes its positions in chunks of SLIM_KEEP: the column ids, then the cells of both rows, side by side, so
//            a long row costs one gather latency per chunk, not per position.  The first chunk (rows up to 64 * SLIM_KEEP
//            entries: all of them) stays in registers for the update; later chunks are read again -- cells that no other lane
//            and, in a conflict-free launch, no other triplet writes.
//   edges    a row of length 0: x = +0, g = 0.5, no store.  No cell outside the seen columns of rows i and j is touched.  A
//            triplet or a column out of range is skipped (x_out = g_out = NaN for the triplet).
#include "el_common.h"
#include "el_levels.h"
#include "el_rowscore.h"

#define SLIM_WAVES 4             // triplets per workgroup of k_bprslim_apply
#define SLIM_KEEP 4              // positions per lane that k_bprslim_apply keeps in registers between the sum and the update

namespace {

struct SlimApply {
    const int32_t* u;
    const int32_t* i;
    const int32_t* j;
    const int64_t* indptr;
    const int32_t* indices;
    int64_t U, I;
    double* S;              // not restrict: rows i and j are read and written through it
    int64_t lds;
    double lr, li_reg, lj_reg;
    double* x_out;          // may be null
    double* g_out;          // may be null
};

// The SLIM_KEEP positions lane + 64 q of the chunk that starts at entry `base`: the column ids, then the cells of both rows,
// loaded side by side, not one dependent gather after the other.  sc[q] = -1 beyond the row; true when a column is out of range.
__device__ __forceinline__ bool slim_load_chunk(const SlimApply& p, int64_t base, int64_t e1, const double* si, const double* sj,
                                                int32_t* sc, double* vi, double* vj) {
    bool bad = false;
#pragma unroll
    for (int q = 0; q < SLIM_KEEP; ++q) {
        const int64_t e = base + 64 * q;
        sc[q] = -1;
        if (e < e1) {
            const int32_t s = p.indices[e];
            if (s < 0 || s >= p.I) bad = true;
            else sc[q] = s;
        }
    }
#pragma unroll
    for (int q = 0; q < SLIM_KEEP; ++q) {
        vi[q] = vj[q] = 0.0;
        if (sc[q] >= 0) {
            vi[q] = si[sc[q]];
            vj[q] = sj[sc[q]];
        }
    }
    return bad;
}

// bprslim_model.py:62 and :65 on the cells of one chunk, from the values slim_load_chunk read
__device__ __forceinline__ void slim_update_chunk(const SlimApply& p, int64_t ii, int64_t jj, double g, double* si, double* sj,
                                                  const int32_t* sc, const double* vi, const double* vj) {
#pragma unroll
    for (int q = 0; q < SLIM_KEEP; ++q) {
        const int64_t s = sc[q];
        if (s < 0) continue;
        double ni = vi[q];
        if (s != ii) {
            ni = __dadd_rn(vi[q], __dmul_rn(p.lr, __dsub_rn(g, __dmul_rn(p.li_reg, vi[q]))));
            si[s] = ni;
        }
        if (s != jj) {
            const double v = ii == jj ? ni : vj[q];             // i == j: the second statement reads what the first stored
            sj[s] = __dsub_rn(v, __dmul_rn(p.lr, __dsub_rn(g, __dmul_rn(p.lj_reg, v))));
        }
    }
}

__global__ __launch_bounds__(SLIM_WAVES * 64) void k_bprslim_apply(SlimApply p, int64_t first, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * SLIM_WAVES + (threadIdx.x >> 6);
    if (w >= n) return;                                         // whole waves leave: the shuffles below stay complete
    const int64_t t = first + w;
    const int64_t uu = p.u[t], ii = p.i[t], jj = p.j[t];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (uu < 0 || uu >= p.U || ii < 0 || ii >= p.I || jj < 0 || jj >= p.I) {
        if (lane == 0) {
            if (p.x_out) p.x_out[t] = nan;
            if (p.g_out) p.g_out[t] = nan;
        }
        return;
    }
    const int64_t e0 = p.indptr[uu] + lane, e1 = p.indptr[uu + 1];
    double* si = p.S + ii * p.lds;
    double* sj = p.S + jj * p.lds;
    // the row in chunks of 64 * SLIM_KEEP entries; the first chunk (most rows: all of them) stays in registers for the update
    int32_t sc0[SLIM_KEEP], sc[SLIM_KEEP];
    double vi0[SLIM_KEEP], vj0[SLIM_KEEP], vi[SLIM_KEEP], vj[SLIM_KEEP];
    double x = 0.0;
    bool bad = slim_load_chunk(p, e0, e1, si, sj, sc0, vi0, vj0);
#pragma unroll
    for (int q = 0; q < SLIM_KEEP; ++q)
        if (sc0[q] >= 0) x = __dadd_rn(x, __dsub_rn(vi0[q], vj0[q]));          // bprslim_model.py:50, ascending positions
    for (int64_t base = e0 + 64 * SLIM_KEEP; base < e1; base += 64 * SLIM_KEEP) {
        bad |= slim_load_chunk(p, base, e1, si, sj, sc, vi, vj);
#pragma unroll
        for (int q = 0; q < SLIM_KEEP; ++q)
            if (sc[q] >= 0) x = __dadd_rn(x, __dsub_rn(vi[q], vj[q]));
    }
    bad = el_group_any(bad, 64);
    x = el_group_sum(x, 64);
    const double g = bad ? nan : __ddiv_rn(1.0, __dadd_rn(1.0, exp(x)));        // :52
    if (lane == 0) {
        if (p.x_out) p.x_out[t] = bad ? nan : x;
        if (p.g_out) p.g_out[t] = g;
    }
    if (bad) return;
    slim_update_chunk(p, ii, jj, g, si, sj, sc0, vi0, vj0);
    for (int64_t base = e0 + 64 * SLIM_KEEP; base < e1; base += 64 * SLIM_KEEP) {
        slim_load_chunk(p, base, e1, si, sj, sc, vi, vj);      // a lane reads again only cells that it alone writes
        slim_update_chunk(p, ii, jj, g, si, sj, sc, vi, vj);
    }
}

// St[s, i] = S[i, s] on k_transpose_f64 (el_rowscore.h)
struct SlimTableLoad {
    const double* S;
    int64_t lds;
    __device__ double operator()(int64_t i, int64_t s) const { return S[i * lds + s]; }
};

// bprslim_model.py:82 on k_row_scores: a plain sum; a column out of range is no cell of St
struct SlimScoreOp : RowScoreOp<double> {
    static constexpr bool CHECK_COLS = true;
    __device__ void step(double& a, int, double v) const { a = __dadd_rn(a, v); }
};

int check_slim_apply(const char* who, const int32_t* u, const int32_t* i, const int32_t* j, const int64_t* indptr,
                     const int32_t* indices, int64_t U, const double* S, int64_t lds, int64_t I) {
    EL_REQUIRE(u && i && j && indptr && indices && S, "%s: null pointer", who);
    EL_REQUIRE(U >= 1 && U < 0x7fffffffLL && I >= 1 && I < 0x7fffffffLL, "%s: bad sizes U=%lld I=%lld", who, (long long)U,
               (long long)I);
    EL_REQUIRE(lds >= I, "%s: leading dimension %lld below I=%lld", who, (long long)lds, (long long)I);
    return 0;
}

int launch_slim_apply(const SlimApply& p, int64_t first, int64_t n, hipStream_t s) {
    EL_REQUIRE(first >= 0 && n >= 1 && (n + SLIM_WAVES - 1) / SLIM_WAVES < 0x7fffffffLL,
               "el_bprslim_apply: %lld triplets from %lld in one call unsupported", (long long)n, (long long)first);
    EL_LAUNCH("k_bprslim_apply", k_bprslim_apply, dim3((unsigned)((n + SLIM_WAVES - 1) / SLIM_WAVES)), dim3(SLIM_WAVES * 64), 0, s,
              p, first, n);
    EL_CHECK_LAUNCH();
    return 0;
}

SlimApply slim_args(const int32_t* u, const int32_t* i, const int32_t* j, const int64_t* indptr, const int32_t* indices, int64_t U,
                    double* S, int64_t lds, int64_t I, double lr, double li_reg, double lj_reg, double* x_out, double* g_out) {
    SlimApply p;
    p.u = u, p.i = i, p.j = j, p.indptr = indptr, p.indices = indices, p.U = U, p.I = I, p.S = S, p.lds = lds;
    p.lr = lr, p.li_reg = li_reg, p.lj_reg = lj_reg, p.x_out = x_out, p.g_out = g_out;
    return p;
}

}  // namespace

extern "C" int el_bprslim_apply(el_ctx* ctx, void* stream, const int32_t* u, const int32_t* i, const int32_t* j, int64_t first,
                                int64_t n, const int64_t* indptr, const int32_t* indices, int64_t U, double* S, int64_t lds,
                                int64_t I, double lr, double li_reg, double lj_reg, double* x_out, double* g_out) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = check_slim_apply("el_bprslim_apply", u, i, j, indptr, indices, U, S, lds, I)) return rc;
    EL_REQUIRE(first >= 0, "el_bprslim_apply: negative first triplet");
    if (n <= 0) return 0;
    return launch_slim_apply(slim_args(u, i, j, indptr, indices, U, S, lds, I, lr, li_reg, lj_reg, x_out, g_out), first, n,
                             (hipStream_t)stream);
}

extern "C" int el_bprslim_apply_levels(el_ctx* ctx, void* stream, const int32_t* u, const int32_t* i, const int32_t* j,
                                       const int64_t* level_start_host, int64_t n_levels, const int64_t* indptr,
                                       const int32_t* indices, int64_t U, double* S, int64_t lds, int64_t I, double lr,
                                       double li_reg, double lj_reg, double* x_out, double* g_out) {
    if (int rc = el_bind(ctx)) return rc;
    if (int rc = check_slim_apply("el_bprslim_apply_levels", u, i, j, indptr, indices, U, S, lds, I)) return rc;
    EL_REQUIRE(level_start_host && n_levels >= 0, "el_bprslim_apply_levels: bad level table");
    const SlimApply p = slim_args(u, i, j, indptr, indices, U, S, lds, I, lr, li_reg, lj_reg, x_out, g_out);
    int64_t bad = 0;
    const int rc = el_levels_apply(level_start_host, n_levels, &bad, [&](int64_t first, int64_t n) {
        return launch_slim_apply(p, first, n, (hipStream_t)stream);
    });
    EL_REQUIRE(rc != EL_LEVELS_BAD_TABLE, "el_bprslim_apply_levels: level %lld is [%lld, %lld)", (long long)bad,
               (long long)level_start_host[bad], (long long)level_start_host[bad + 1]);
    return rc;
}

// Host-only scheduling helper: rows i and j of S are all a triplet reads or writes, so the user is no dependency.
extern "C" int el_bprslim_levels_host(const int32_t* i, const int32_t* j, int64_t n, int64_t I, int32_t* order, int64_t* level_start,
                                      int64_t level_start_cap, int64_t* n_levels) {
    EL_REQUIRE(i && j && order && level_start && n_levels, "el_bprslim_levels_host: null pointer");
    EL_REQUIRE(n >= 0 && n < 0x7fffffffLL && I >= 1, "el_bprslim_levels_host: n or I out of range");
    EL_REQUIRE(level_start_cap >= 1, "el_bprslim_levels_host: no room for the level table");
    int64_t bad = 0;
    const int rc = el_levels_build<0, 0>({i, j}, {I}, n, order, level_start, level_start_cap, n_levels, &bad);
    EL_REQUIRE(rc != EL_LEVELS_BAD_ID, "el_bprslim_levels_host: triplet %lld out of range", (long long)bad);
    EL_REQUIRE(rc != EL_LEVELS_NO_ROOM, "el_bprslim_levels_host: %d levels exceed capacity %lld", (int)bad,
               (long long)level_start_cap);
    return 0;
}

extern "C" int el_bprslim_table(el_ctx* ctx, void* stream, const double* S, int64_t lds, int64_t I, double* St, int64_t ldt) {
    return el_transpose_f64("el_bprslim_table", "k_bprslim_table", ctx, stream, S && St, lds >= I && ldt >= I,
                            SlimTableLoad{S, lds}, I, St, ldt);
}

extern "C" int el_bprslim_scores(el_ctx* ctx, void* stream, const int64_t* indptr, const int32_t* indices, int64_t u_start,
                                 int64_t u_stop, const double* St, int64_t ldt, int64_t I, double* P, int64_t ldp) {
    return el_row_scores("el_bprslim_scores", "k_bprslim_scores", ctx, stream, indptr && indices && St && P, indptr, indices,
                         u_start, u_stop, SlimScoreOp{{St, ldt}}, I, P, ldp);
}
