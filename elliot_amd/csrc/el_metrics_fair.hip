// Fairness metrics on the device, from the same [users, k] top-k tensors as el_metrics.hip / el_metrics_beyond.hip.
//
// Replaces the per-user set algebra of evaluation/metrics/fairness/ (Evaluator._process_test_data, evaluation/evaluator.py:117-147):
//   RSP, REO                     rsp/rsp.py, reo/reo.py           exposure / hit probability per ITEM group, std / mean over the groups
//   BiasDisparityBR / BS / BD    BiasDisparity/*.py               (user group, item group) counts of the lists / of the train rows
//   UserMADranking / rating      MAD/UserMAD*.py                  mean nDCG / mean list score per USER group, mean pairwise |difference|
//   ItemMADranking / rating      MAD/ItemMAD*.py                  per item the mean gain / score over the lists that hold it, mean per group
// PopRSP / PopREO of el_metrics_beyond.hip are the two-group special case of RSP / REO; here the groups come from label tables
// (item_group int32[I], user_group int32[U], -1 = no label, up to FAIR_MAXG groups each).
//
// Populations: A = users with a non-empty held-out row, R = users of A with an item rated >= threshold.
// Passes:
//   1. k_fair_users        one wave per user, FAIR_UPW users per wave one after the other.  Integers (RSP / REO numerators and
//                          denominators, the BR count matrix) are added into an LDS table per workgroup and flushed with one 64-bit
//                          integer add per non-zero cell: with two or three groups every list entry of the block lands on the same
//                          few words.
//                          Per user: label, nDCG (k_rec_metrics' own IDCG pass and lookup, el_metrics_row.h), mean list score, flags.
//                          Per relevant held-out entry found in the list: its column and its score (arrays aligned with the CSR).
//      k_beyond_hist<true> the lists of the users of R into an int32[I] histogram (el_metrics_hist.h)
//      el_group_sums       the per-user rows summed by user label in a fixed shape
//   2. k_fair_items        after the last block, one thread per item: the item's column of the held-out set (item-major copy of the
//                          CSR), gains and scores of the hit entries added in ascending user order, divided by the histogram count;
//                          then the per-item rows summed by item label in the same fixed shape.
// No float atomics anywhere: integer adds do not depend on their order, every fp64 sum has a shape fixed by the sizes alone, and an
// item's sum runs in user order whatever the block cut was.
#include "el_common.h"
#include "el_metrics_row.h"
#include "el_metrics_tree.h"
#include "el_metrics_hist.h"

#define FAIR_MAXG 64
#define FAIR_UPW 8          // users per wave: 32 per workgroup share one LDS table
#define FAIR_ROW 4          // per-user row: nDCG, in R, mean list score, has a score

struct FairArgs {
    const int32_t* rec;
    const float* val;
    int64_t ld, u_start, n;
    const int64_t* tp;
    const int32_t* ti;
    const float* tr;
    double thr;
    int cutoff;
    const int64_t* qp;
    const int32_t* qi;
    int32_t I;
    const int32_t *item_group, *user_group;
    const int64_t* item_size;
    int Gi, Gu;
    const double* disc;
    u64 *item_tab, *br;       // [4][Gi]: RSP num, RSP den, REO num, REO den;  [Gu][Gi]
    int32_t* label;
    double* rows;
    int32_t* hit_pos;
    float* hit_score;
};

__device__ __forceinline__ int fair_label(const int32_t* __restrict__ tab, int64_t i, int G) {
    const int g = tab[i];
    return (g >= 0 && g < G) ? g : -1;
}

// tab[key] += 1 in the workgroup's LDS table (-1: nothing).  A list chunk holds a handful of entries, so a plain LDS add per lane
// (lanes on one word serialise inside the LDS, one cycle each) beats electing one lane per distinct key.
__device__ __forceinline__ void fair_lds_add(int* tab, int key) {
    if (key >= 0) atomicAdd(tab + key, 1);
}

__global__ __launch_bounds__(256) void k_fair_users(FairArgs a) {
    __shared__ u64 gb_[4][MET_BUF];
    extern __shared__ int tab[];                               // fair_tab_ints(Gu, Gi) ints: the table is as large as the groups need
    const int Gi = a.Gi, Gu = a.Gu, cutoff = a.cutoff;
    int *rspn = tab, *tcnt = tab + FAIR_MAXG, *reon = tab + 2 * FAIR_MAXG, *reod = tab + 3 * FAIR_MAXG, *br = tab + 4 * FAIR_MAXG;
    int* nA = br + Gu * Gi;
    for (int t = threadIdx.x; t < 4 * FAIR_MAXG + Gu * Gi + 1; t += 256) tab[t] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u64* gb = gb_[wv];
    const double thr = a.thr;
    for (int s = 0; s < FAIR_UPW; ++s) {
        const int64_t ur = ((int64_t)blockIdx.x * 4 + wv) * FAIR_UPW + s;
        if (ur >= a.n) break;                                    // wave-uniform
        const int64_t user = a.u_start + ur;
        const int64_t t0 = a.tp[user], t1 = a.tp[user + 1];
        const int h = fair_label(a.user_group, user, Gu);
        double* o = a.rows + ur * FAIR_ROW;
        if (lane == 0) a.label[ur] = h;
        if (t1 <= t0) {                                          // not in A
            if (lane < FAIR_ROW) o[lane] = 0.0;
            continue;
        }
        const int64_t q0 = a.qp[user], q1 = a.qp[user + 1];

        // ---- held-out row: relevant items, the `cutoff` largest gains (IDCG), REO denominators ----------------------------------------
        const MetRow row = met_row_idcg(gb, a.tr, t0, t1, thr, cutoff, a.disc, lane, [&](int64_t e, bool relv) {
            int dg = -1;
            if (relv) {
                const int32_t item = a.ti[e];
                if (item >= 0 && item < a.I && !el_row_contains(a.qi, q0, q1, item)) dg = fair_label(a.item_group, item, Gi);
            }
            fair_lds_add(reod, dg);
        });
        const bool inR = row.nrel > 0.0;

        // ---- train row: what it holds of every item group (RSP denominators) ----------------------------------------------------------
        for (int64_t b = q0; b < q1; b += 64) {
            const int64_t e = b + lane;
            int g = -1;
            if (e < q1) {
                const int32_t item = a.qi[e];
                if (item >= 0 && item < a.I) g = fair_label(a.item_group, item, Gi);
            }
            fair_lds_add(tcnt, g);
        }
        if (lane == 0) atomicAdd(nA, 1);

        // ---- the recommendation list -------------------------------------------------------------------------------------------------
        double dcg = 0.0, ss = 0.0;
        int nu = 0;
        for (int c0 = 0; c0 < cutoff; c0 += 64) {
            const int c = c0 + lane;
            bool valid = false, hit = false;
            double g = 0.0;
            int ig = -1;
            if (c < cutoff) {
                const int32_t item = a.rec[ur * a.ld + c];
                if (item >= 0) {
                    const MetEntry m = met_lookup(a.ti, a.tr, t0, t1, item, thr);
                    hit = m.rel && item < a.I;
                    g = m.gain;
                    if (item < a.I) {
                        valid = true;
                        ig = fair_label(a.item_group, item, Gi);
                        const float sc = a.val ? a.val[ur * a.ld + c] : 0.0f;
                        ss += (double)sc;
                        if (hit) {
                            a.hit_pos[m.pos] = c;
                            a.hit_score[m.pos] = sc;
                        }
                    }
                }
                dcg += g * a.disc[c];
            }
            nu += __popcll(__ballot(valid));
            fair_lds_add(rspn, ig);
            fair_lds_add(br, (h >= 0 && ig >= 0) ? h * Gi + ig : -1);
            fair_lds_add(reon, hit ? ig : -1);
        }
        dcg = el_group_sum(dcg, 64);
        ss = el_group_sum(ss, 64);
        if (lane == 0) {
            const bool scored = inR && a.val != nullptr && nu > 0;
            o[0] = (inR && dcg > 0.0 && row.idcg > 0.0) ? dcg / row.idcg : 0.0;
            o[1] = inR ? 1.0 : 0.0;
            o[2] = scored ? ss / (double)nu : 0.0;
            o[3] = scored ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    const long long na = (long long)*nA;
    for (int t = threadIdx.x; t < Gi; t += 256) {
        if (rspn[t]) atomicAdd(a.item_tab + t, (u64)rspn[t]);
        const long long d = na * (long long)a.item_size[t] - (long long)tcnt[t];
        if (d) atomicAdd(a.item_tab + Gi + t, (u64)d);
        if (reon[t]) atomicAdd(a.item_tab + 2 * Gi + t, (u64)reon[t]);
        if (reod[t]) atomicAdd(a.item_tab + 3 * Gi + t, (u64)reod[t]);
    }
    for (int t = threadIdx.x; t < Gu * Gi; t += 256)
        if (br[t]) atomicAdd(a.br + t, (u64)br[t]);
}

// counts[h][g] += entries of the rows [0, n_rows) of a CSR whose row has label h and whose column has label g
__global__ __launch_bounds__(256) void k_fair_group_counts(const int64_t* __restrict__ rp, const int32_t* __restrict__ ci, int64_t n_rows,
                                                           int32_t I, const int32_t* __restrict__ item_group, int Gi,
                                                           const int32_t* __restrict__ user_group, int Gu, u64* __restrict__ counts) {
    __shared__ u64 tab[FAIR_MAXG * FAIR_MAXG];                 // a train row can be long: 64-bit cells
    for (int t = threadIdx.x; t < Gu * Gi; t += 256) tab[t] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int s = 0; s < FAIR_UPW; ++s) {
        const int64_t row = ((int64_t)blockIdx.x * 4 + wv) * FAIR_UPW + s;
        if (row >= n_rows) break;
        const int h = fair_label(user_group, row, Gu);
        if (h < 0) continue;
        const int64_t p0 = rp[row], p1 = rp[row + 1];
        for (int64_t b = p0; b < p1; b += 64) {
            const int64_t e = b + lane;
            int key = -1;
            if (e < p1) {
                const int32_t item = ci[e];
                if (item >= 0 && item < I) {
                    const int g = fair_label(item_group, item, Gi);
                    if (g >= 0) key = h * Gi + g;
                }
            }
            if (key >= 0) atomicAdd(tab + key, 1ull);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < Gu * Gi; t += 256)
        if (tab[t]) atomicAdd(counts + t, tab[t]);
}

// ---- rows [n, W] (W <= 4) summed by label in a fixed shape: the grouped sibling of met_tree_sum ------------------------------------
// grid (met_groups(n), n_groups): workgroup (b, g) adds the rows of its contiguous range whose label is g -> part[b][g][4]; then one
// thread per (g, column) adds the partial rows in order.  The shape depends on n alone.
__global__ __launch_bounds__(256) void k_fair_group_partial(const double* __restrict__ rows, int W, const int32_t* __restrict__ labels, int64_t n,
                                                            int64_t per, double* __restrict__ part, u64* __restrict__ counts) {
    __shared__ double sh[256];
    __shared__ int shc[256];
    const int g = blockIdx.y, G = gridDim.y;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = (lo + per < n) ? lo + per : n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int c = 0;
    for (int64_t r = lo + threadIdx.x; r < hi; r += 256) {
        if (labels[r] == g) {
            ++c;
            for (int m = 0; m < W; ++m) acc[m] += rows[r * W + m];
        }
    }
    shc[threadIdx.x] = c;
    for (int m = 0; m < 4; ++m) {
        sh[threadIdx.x] = acc[m];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                sh[threadIdx.x] += sh[threadIdx.x + s];
                if (m == 0) shc[threadIdx.x] += shc[threadIdx.x + s];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) part[((int64_t)blockIdx.x * G + g) * 4 + m] = sh[0];
        __syncthreads();
    }
    if (threadIdx.x == 0 && shc[0]) atomicAdd(counts + g, (u64)shc[0]);
}

__global__ __launch_bounds__(256) void k_fair_group_final(const double* __restrict__ part, int B, int G, int W, double* __restrict__ sums) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= G * W) return;
    const int g = t / W, m = t - g * W;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc += part[((int64_t)b * G + g) * 4 + m];
    sums[t] += acc;
}

// per item: rows[i] = (sum of the gains, sum of the scores) of its hit entries in ascending user order / hist[i]; lab[i] = the item's
// group when a list of R holds it, else -1
__global__ __launch_bounds__(256) void k_fair_items(const int64_t* __restrict__ cp, const int64_t* __restrict__ ce, const float* __restrict__ tr,
                                                    double thr, const int32_t* __restrict__ hit_pos, const float* __restrict__ hit_score,
                                                    const int32_t* __restrict__ hist, int64_t I, const int32_t* __restrict__ item_group, int Gi,
                                                    double* __restrict__ rows, int32_t* __restrict__ lab) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= I) return;
    const int32_t c = hist[i];
    double sg = 0.0, ss = 0.0;
    if (c > 0) {
        for (int64_t j = cp[i]; j < cp[i + 1]; ++j) {
            const int64_t e = ce[j];
            if (hit_pos[e] >= 0) {
                sg += met_gain(met_rating(tr, e), thr);
                ss += (double)hit_score[e];
            }
        }
    }
    rows[i * 2] = c > 0 ? sg / (double)c : 0.0;
    rows[i * 2 + 1] = c > 0 ? ss / (double)c : 0.0;
    lab[i] = c > 0 ? fair_label(item_group, i, Gi) : -1;
}

namespace {

size_t fair_sum_carve(int64_t n, int n_groups, ElCarve& c, double** part) {
    *part = c.take<double>((size_t)met_groups(n) * n_groups * 4);
    return c.off;
}

int fair_group_sums(hipStream_t st, const double* rows, int W, const int32_t* labels, int64_t n, int n_groups, double* sums, int64_t* counts,
                    double* part) {
    const int B = met_groups(n);
    const int64_t per = (n + B - 1) / B;
    EL_LAUNCH("k_fair_group_partial", k_fair_group_partial, dim3(B, n_groups), dim3(256), 0, st, rows, W, labels, n, per, part,
              reinterpret_cast<u64*>(counts));
    EL_LAUNCH("k_fair_group_final", k_fair_group_final, dim3((n_groups * W + 255) / 256), dim3(256), 0, st, (const double*)part, B, n_groups, W,
              sums);
    return 0;
}

struct FairItemWs {
    double *rows, *part;
    int32_t* lab;
};
size_t fair_item_carve(int64_t I, int n_groups, void* base, FairItemWs* w) {
    ElCarve c{(char*)base};
    w->rows = c.take<double>((size_t)I * 2);
    w->lab = c.take<int32_t>((size_t)I);
    return fair_sum_carve(I, n_groups, c, &w->part);
}

bool fair_groups_ok(int32_t g) { return g >= 1 && g <= FAIR_MAXG; }

// k_fair_users' dynamic LDS: four item-group rows, the pair matrix, the count of users of A
size_t fair_tab_ints(int Gu, int Gi) { return (size_t)4 * FAIR_MAXG + (size_t)Gu * Gi + 1; }

}  // namespace

extern "C" int el_fair_metrics(el_ctx* ctx, void* stream, const int32_t* rec_idx, const float* rec_val, int64_t ld, int64_t u_start,
                               int64_t u_stop, const int64_t* test_indptr, const int32_t* test_indices, const float* test_ratings,
                               double threshold, int32_t cutoff, const int64_t* train_indptr, const int32_t* train_indices, int64_t n_items,
                               const int32_t* item_group, int32_t n_item_groups, const int64_t* item_group_size, const int32_t* user_group,
                               int32_t n_user_groups, const double* discount, int64_t* item_counts, int64_t* pair_counts,
                               int32_t* user_label, double* user_rows, int32_t* hit_pos, float* hit_score, int32_t* hist) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(u_stop >= u_start, "el_fair_metrics: u_stop < u_start");
    const int64_t n = u_stop - u_start;
    if (n == 0) return 0;
    EL_REQUIRE(rec_idx && test_indptr && test_indices && train_indptr && train_indices && item_group && item_group_size && user_group &&
                   discount && item_counts && pair_counts && user_label && user_rows && hit_pos && hit_score && hist,
               "el_fair_metrics: null pointer");
    MET_REQUIRE_CUTOFF("el_fair_metrics", cutoff, ld);
    EL_REQUIRE(fair_groups_ok(n_item_groups) && fair_groups_ok(n_user_groups), "el_fair_metrics: %d item / %d user groups (1..%d each)",
               n_item_groups, n_user_groups, FAIR_MAXG);
    EL_REQUIRE(n_items >= 1 && n_items < (1LL << 31), "el_fair_metrics: bad item count");
    EL_REQUIRE(n < (1LL << 31), "el_fair_metrics: more than 2^31 users in one block");
    hipStream_t st = (hipStream_t)stream;
    FairArgs a;
    a.rec = rec_idx, a.val = rec_val, a.ld = ld, a.u_start = u_start, a.n = n;
    a.tp = test_indptr, a.ti = test_indices, a.tr = test_ratings, a.thr = threshold, a.cutoff = (int)cutoff;
    a.qp = train_indptr, a.qi = train_indices, a.I = (int32_t)n_items;
    a.item_group = item_group, a.user_group = user_group, a.item_size = item_group_size, a.Gi = n_item_groups, a.Gu = n_user_groups;
    a.disc = discount, a.item_tab = reinterpret_cast<u64*>(item_counts), a.br = reinterpret_cast<u64*>(pair_counts);
    a.label = user_label, a.rows = user_rows, a.hit_pos = hit_pos, a.hit_score = hit_score;
    const int64_t per_wg = 4 * FAIR_UPW;
    EL_LAUNCH("k_fair_users", k_fair_users, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(256),
              fair_tab_ints(n_user_groups, n_item_groups) * sizeof(int), st, a);
    const int64_t tiles = (n * cutoff + BEY_TILE - 1) / BEY_TILE;
    EL_LAUNCH("k_fair_hist", k_beyond_hist<true>, dim3((unsigned)tiles), dim3(256), 0, st, rec_idx, ld, u_start, n, test_indptr,
              (const double*)(user_rows + 1), FAIR_ROW, (int)cutoff, (int32_t)n_items, hist);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_group_counts(el_ctx* ctx, void* stream, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_items,
                               const int32_t* item_group, int32_t n_item_groups, const int32_t* user_group, int32_t n_user_groups,
                               int64_t* pair_counts) {
    if (int rc = el_bind(ctx)) return rc;
    if (n_rows == 0) return 0;
    EL_REQUIRE(indptr && indices && item_group && user_group && pair_counts, "el_group_counts: null pointer");
    EL_REQUIRE(fair_groups_ok(n_item_groups) && fair_groups_ok(n_user_groups), "el_group_counts: %d item / %d user groups (1..%d each)",
               n_item_groups, n_user_groups, FAIR_MAXG);
    EL_REQUIRE(n_rows > 0 && n_rows < (1LL << 31) * 4 * FAIR_UPW && n_items >= 1 && n_items < (1LL << 31), "el_group_counts: bad sizes");
    const int64_t per_wg = 4 * FAIR_UPW;
    EL_LAUNCH("k_fair_group_counts", k_fair_group_counts, dim3((unsigned)((n_rows + per_wg - 1) / per_wg)), dim3(256), 0, (hipStream_t)stream,
              indptr, indices, n_rows, (int32_t)n_items, item_group, (int)n_item_groups, user_group, (int)n_user_groups,
              reinterpret_cast<u64*>(pair_counts));
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t el_group_sums_ws_bytes(int64_t n, int32_t n_groups) {
    if (n <= 0 || !fair_groups_ok(n_groups)) return 0;
    ElCarve c{nullptr};
    double* part;
    return fair_sum_carve(n, n_groups, c, &part);
}

extern "C" int el_group_sums(el_ctx* ctx, void* stream, const double* rows, int32_t width, const int32_t* labels, int64_t n, int32_t n_groups,
                             double* sums, int64_t* counts, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    if (n == 0) return 0;
    EL_REQUIRE(rows && labels && sums && counts, "el_group_sums: null pointer");
    EL_REQUIRE(n > 0 && width >= 1 && width <= 4, "el_group_sums: rows of 1..4 columns (got %d)", width);
    EL_REQUIRE(fair_groups_ok(n_groups), "el_group_sums: %d groups (1..%d)", n_groups, FAIR_MAXG);
    ElCarve c{(char*)ws};
    double* part;
    EL_REQUIRE(ws != nullptr && ws_bytes >= fair_sum_carve(n, n_groups, c, &part), "el_group_sums: workspace too small");
    fair_group_sums((hipStream_t)stream, rows, (int)width, labels, n, (int)n_groups, sums, counts, part);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t el_fair_item_finish_ws_bytes(int64_t n_items, int32_t n_item_groups) {
    if (n_items <= 0 || !fair_groups_ok(n_item_groups)) return 0;
    FairItemWs w;
    return fair_item_carve(n_items, n_item_groups, nullptr, &w);
}

extern "C" int el_fair_item_finish(el_ctx* ctx, void* stream, const int64_t* col_indptr, const int64_t* col_entry, const float* test_ratings,
                                   double threshold, const int32_t* hit_pos, const float* hit_score, const int32_t* hist, int64_t n_items,
                                   const int32_t* item_group, int32_t n_item_groups, double* sums, int64_t* counts, double* per_item, void* ws,
                                   size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(col_indptr && col_entry && hit_pos && hit_score && hist && item_group && sums && counts, "el_fair_item_finish: null pointer");
    EL_REQUIRE(n_items >= 1 && n_items < (1LL << 31), "el_fair_item_finish: bad item count");
    EL_REQUIRE(fair_groups_ok(n_item_groups), "el_fair_item_finish: %d item groups (1..%d)", n_item_groups, FAIR_MAXG);
    FairItemWs w;
    EL_REQUIRE(ws != nullptr && ws_bytes >= fair_item_carve(n_items, n_item_groups, ws, &w), "el_fair_item_finish: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double* rows = per_item ? per_item : w.rows;
    EL_LAUNCH("k_fair_items", k_fair_items, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st, col_indptr, col_entry, test_ratings,
              threshold, hit_pos, hit_score, hist, n_items, item_group, (int)n_item_groups, rows, w.lab);
    fair_group_sums(st, rows, 2, w.lab, n_items, (int)n_item_groups, sums, counts, w.part);
    EL_CHECK_LAUNCH();
    return 0;
}
