// Beyond-accuracy metrics on the device, from the same [users, k] top-k index tensor as el_metrics.hip:
// coverage, concentration, novelty and popularity bias.
//
// Replaces the reference's per-user Python of evaluation/evaluator.py:117-147 (_process_test_data) for
//   ItemCoverage  #items in any list                                     metrics/coverage/item_coverage/item_coverage.py
//   UserCoverage  #users with a non-empty list                           metrics/coverage/user_coverage/user_coverage.py
//   NumRetrieved  list length, over the users with a relevant item       metrics/coverage/num_retrieved/num_retrieved.py
//   Gini          1 - sum_j (2(j + I - n + 1) - I - 1) c_(j)/free / (I-1) metrics/diversity/gini_index/gini_index.py
//   SEntropy      sum_i w_i nov_i / #users, nov_i = -log2(c_i / free)    metrics/diversity/shannon_entropy/shannon_entropy.py
//   EFD, EPC      rank-discounted novelty of the relevant hits           metrics/novelty/EFD/efd.py, metrics/novelty/EPC/epc.py
//   ARP, APLT, ACLT   popularity / long-tail share of the lists          metrics/bias/{arp,aplt,aclt}
//   PopREO, PopRSP    head / tail hit and exposure ratios                metrics/bias/pop_reo/pop_reo.py, pop_rsp/pop_rsp.py
// with the item tables of popularity_utils/popularity.py (popularity, short head) built once on the host.
//
// Two populations: A = users with a non-empty held-out row (evaluator.py:121), R = users of A with an item rated >= threshold.
// Three passes:
//   1. k_beyond_users  one wave per user: a row of BEY_N fp64 terms (flags, list length, ARP / APLT / ACLT / EFD / EPC terms, the eight
//                      PopRSP / PopREO integers -- exact in fp64: each is below 2^31 and their sums stay below 2^53), summed over the block
//                      of users by the fixed-shape tree of el_metrics_tree.h; the lists of the users of A are added to the item histogram
//   2. el_beyond_hist_finish   radix sort of the counts -> n, free and the exact integer G = sum_p (2p + 1 - I) sorted[p]
//                      (= the Gini numerator: the n non-zero counts sit at p = I - n + j), and nov[i]
//   3. k_beyond_entropy        (1/n_u) sum of nov over each list, fixed-shape sum
// No float atomics: the histogram and the three integers of pass 2 use integer adds, whose result does not depend on their order.
//
// Histogram: one popular item can sit in most lists of a block, and adds on one word serialise.  k_beyond_hist therefore sorts a tile
// of BEY_TILE list entries in LDS and issues one add per DISTINCT id of the tile (guideline: aggregate inside the workgroup before
// touching memory).  EL_BEYOND_HIST_DIRECT keeps the plain form (one add per list entry from k_beyond_users).  Measured per block of
// 131 072 x 10 at I = 1 M (profiles/metrics_beyond_bench.md, scripts/metrics_bench.py), whole el_beyond_metrics call: tile-aggregated
// 0.29 / 0.28 / 0.24 ms on uniform / Zipf / identical lists, direct 0.20 / 1.11 / 1.56 ms -- the default is the aggregated form.
#include "el_common.h"
#include "el_metrics_row.h"          // relevance and the list-entry lookup, shared with the accuracy and fairness kernels
#include "el_metrics_tree.h"
#include "el_metrics_hist.h"

#include <rocprim/device/device_radix_sort.hpp>

#define BEY_N 18

struct BeyArgs {
    const int32_t* rec;
    int64_t ld, u_start, n;
    const int64_t* tp;
    const int32_t* ti;
    const float* tr;
    double thr;
    int cutoff;
    const int64_t* qp;      // train CSR
    const int32_t* qi;
    int64_t I, n_head;
    const int32_t* pop;
    const unsigned char* head;
    const double *efd, *epc, *disc;
    int32_t* hist;
    double* rows;
};

template <bool DIRECT>
__global__ __launch_bounds__(256) void k_beyond_users(BeyArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ur = (int64_t)blockIdx.x * 4 + wv;
    if (ur >= a.n) return;
    const int64_t user = a.u_start + ur;
    const int64_t t0 = a.tp[user], t1 = a.tp[user + 1];
    double* o = a.rows + ur * BEY_N;
    if (t1 <= t0) {                                          // not in A: the row adds nothing
        if (lane < BEY_N) o[lane] = 0.0;
        return;
    }
    const int64_t q0 = a.qp[user], q1 = a.qp[user + 1];
    const int32_t I = (int32_t)a.I;

    // ---- held-out row: relevant items, and those outside the train row by head / tail (PopREO denominators) ---------------------
    int nrel = 0, rdh = 0, rdt = 0;
    for (int64_t b = t0; b < t1; b += 64) {
        const int64_t e = b + lane;
        bool relv = false;
        int h = -1;
        if (e < t1) {
            relv = met_rating(a.tr, e) >= a.thr;
            const int32_t item = a.ti[e];
            if (relv && item >= 0 && item < I && !el_row_contains(a.qi, q0, q1, item)) h = a.head[item] ? 1 : 0;
        }
        nrel += __popcll(__ballot(relv));
        rdh += __popcll(__ballot(h == 1));
        rdt += __popcll(__ballot(h == 0));
    }
    const bool inR = nrel > 0;

    // ---- train row: how much of the head it holds (PopRSP denominators) ------------------------------------------------------------
    int th = 0;
    for (int64_t b = q0; b < q1; b += 64) {
        const int64_t e = b + lane;
        bool hh = false;
        if (e < q1) {
            const int32_t item = a.qi[e];
            hh = item >= 0 && item < I && a.head[item] != 0;
        }
        th += __popcll(__ballot(hh));
    }
    const double sdh = (double)(a.n_head - th);
    const double sdt = (double)((a.I - a.n_head) - ((q1 - q0) - th));

    // ---- the recommendation list --------------------------------------------------------------------------------------------------
    int nu = 0, nt = 0, rnh = 0, rnt = 0;
    double ps = 0.0, fe = 0.0, fp = 0.0, norm = 0.0;
    for (int c0 = 0; c0 < a.cutoff; c0 += 64) {
        const int c = c0 + lane;
        bool valid = false, tail = false, hit = false;
        if (c < a.cutoff) {
            const int32_t item = a.rec[ur * a.ld + c];
            if (item >= 0 && item < I) {
                valid = true;
                tail = a.head[item] == 0;
                ps += (double)a.pop[item];
                const double d = a.disc[c];
                norm += d;
                if (met_lookup(a.ti, a.tr, t0, t1, item, a.thr).rel) {
                    hit = true;
                    fe += d * a.efd[item];
                    fp += d * a.epc[item];
                }
                if (DIRECT) atomicAdd(a.hist + item, 1);
            }
        }
        nu += __popcll(__ballot(valid));
        nt += __popcll(__ballot(valid && tail));
        rnh += __popcll(__ballot(hit && !tail));
        rnt += __popcll(__ballot(hit && tail));
    }
    ps = el_group_sum(ps, 64);
    fe = el_group_sum(fe, 64);
    fp = el_group_sum(fp, 64);
    norm = el_group_sum(norm, 64);
    if (lane == 0) {
        const double dn = (double)nu;
        const bool nov = inR && norm > 0.0;
        o[0] = 1.0;
        o[1] = inR ? 1.0 : 0.0;
        o[2] = nu > 0 ? 1.0 : 0.0;
        o[3] = dn;
        o[4] = nu > 0 ? ps / dn : 0.0;
        o[5] = nu > 0 ? (double)nt / dn : 0.0;
        o[6] = (double)nt;
        o[7] = inR ? dn : 0.0;
        o[8] = nov ? fe / norm : 0.0;
        o[9] = nov ? fp / norm : 0.0;
        o[10] = (double)(nu - nt);
        o[11] = (double)nt;
        o[12] = sdh;
        o[13] = sdt;
        o[14] = inR ? (double)rnh : 0.0;
        o[15] = inR ? (double)rnt : 0.0;
        o[16] = inR ? (double)rdh : 0.0;
        o[17] = inR ? (double)rdt : 0.0;
    }
}

// stats[0] += #non-zero counts, stats[1] += sum of the counts, stats[2] += sum_p (2p + 1 - I) sorted[p]   (64-bit integer adds)
__global__ __launch_bounds__(256) void k_beyond_hist_stats(const u32* __restrict__ sorted, int64_t I, unsigned long long* __restrict__ stats) {
    __shared__ long long sh[3][256];
    long long nz = 0, fr = 0, g = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < I; p += (int64_t)gridDim.x * 256) {
        const long long c = (long long)sorted[p];
        nz += c > 0 ? 1 : 0;
        fr += c;
        g += (2 * p + 1 - I) * c;
    }
    sh[0][threadIdx.x] = nz, sh[1][threadIdx.x] = fr, sh[2][threadIdx.x] = g;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int m = 0; m < 3; ++m) sh[m][threadIdx.x] += sh[m][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) atomicAdd(stats + threadIdx.x, (unsigned long long)sh[threadIdx.x][0]);
}

// nov[i] = -log(cnt[i] / free) / log 2 (shannon_entropy.py: __sales_novelty), 0 for an item no list holds
__global__ __launch_bounds__(256) void k_beyond_nov(const int32_t* __restrict__ hist, int64_t I, const unsigned long long* __restrict__ stats,
                                                    double* __restrict__ nov) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= I) return;
    const int32_t c = hist[i];
    const double fr = (double)(long long)stats[1];
    nov[i] = c > 0 ? -log((double)c / fr) / log(2.0) : 0.0;
}

__global__ __launch_bounds__(256) void k_beyond_entropy(const int32_t* __restrict__ rec, int64_t ld, int64_t u_start, int64_t n,
                                                        const int64_t* __restrict__ tp, int cutoff, int32_t I,
                                                        const double* __restrict__ nov, double* __restrict__ rows) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ur = (int64_t)blockIdx.x * 4 + wv;
    if (ur >= n) return;
    const int64_t user = u_start + ur;
    double s = 0.0;
    int nu = 0;
    if (tp[user + 1] > tp[user]) {
        for (int c0 = 0; c0 < cutoff; c0 += 64) {
            const int c = c0 + lane;
            bool valid = false;
            if (c < cutoff) {
                const int32_t item = rec[ur * ld + c];
                if (item >= 0 && item < I) {
                    valid = true;
                    s += nov[item];
                }
            }
            nu += __popcll(__ballot(valid));
        }
        s = el_group_sum(s, 64);
    }
    if (lane == 0) rows[ur] = nu > 0 ? s / (double)nu : 0.0;
}

namespace {

struct BeyWs {
    u32* sorted;
    void* tmp;
    size_t tmp_bytes, total;
};

int bey_carve(int64_t I, void* base, BeyWs* w) {
    ElCarve c{(char*)base};
    w->sorted = c.take<u32>((size_t)I);
    size_t t = 0;
    u32* np = nullptr;
    if (rocprim::radix_sort_keys(nullptr, t, np, np, (unsigned)I, 0, 32, (hipStream_t)0) != hipSuccess) return 1;
    w->tmp_bytes = t;
    w->tmp = c.take<char>(t);
    w->total = c.off;
    return 0;
}

}  // namespace

extern "C" size_t el_beyond_ws_bytes(int64_t n_users, int64_t n_items) {
    MetWs m;
    size_t need = n_users <= 0 ? 0 : met_carve(n_users, BEY_N, nullptr, &m);
    if (n_items > 0 && n_items < (1LL << 31)) {
        BeyWs w;
        if (bey_carve(n_items, nullptr, &w)) return 0;
        if (w.total > need) need = w.total;
    }
    return need;
}

extern "C" int el_beyond_metrics(el_ctx* ctx, void* stream, const int32_t* rec_idx, int64_t ld, int64_t u_start, int64_t u_stop,
                                 const int64_t* test_indptr, const int32_t* test_indices, const float* test_ratings, double threshold,
                                 int32_t cutoff, const int64_t* train_indptr, const int32_t* train_indices, int64_t n_items,
                                 int64_t n_head, const int32_t* pop, const unsigned char* head, const double* efd, const double* epc,
                                 const double* discount, int32_t* hist, double* sums, double* per_user, int32_t flags, void* ws,
                                 size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(u_stop >= u_start, "el_beyond_metrics: u_stop < u_start");
    const int64_t n = u_stop - u_start;
    if (n == 0) return 0;
    EL_REQUIRE(rec_idx && test_indptr && test_indices && train_indptr && train_indices && pop && head && efd && epc && discount && hist &&
                   sums,
               "el_beyond_metrics: null pointer");
    MET_REQUIRE_CUTOFF("el_beyond_metrics", cutoff, ld);
    EL_REQUIRE(n_items >= 1 && n_items < (1LL << 31) && n_head >= 0 && n_head <= n_items, "el_beyond_metrics: bad item counts");
    EL_REQUIRE(n < (1LL << 31), "el_beyond_metrics: more than 2^31 users in one block");
    MetWs m;
    EL_REQUIRE(ws != nullptr && ws_bytes >= met_carve(n, BEY_N, ws, &m), "el_beyond_metrics: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    BeyArgs a;
    a.rec = rec_idx, a.ld = ld, a.u_start = u_start, a.n = n;
    a.tp = test_indptr, a.ti = test_indices, a.tr = test_ratings, a.thr = threshold, a.cutoff = (int)cutoff;
    a.qp = train_indptr, a.qi = train_indices, a.I = n_items, a.n_head = n_head;
    a.pop = pop, a.head = head, a.efd = efd, a.epc = epc, a.disc = discount, a.hist = hist;
    a.rows = per_user ? per_user : m.rows;
    const dim3 grid((unsigned)((n + 3) / 4));
    if (flags & EL_BEYOND_HIST_DIRECT) {
        EL_LAUNCH("k_beyond_users", (k_beyond_users<true>), grid, dim3(256), 0, st, a);
    } else {
        EL_LAUNCH("k_beyond_users", (k_beyond_users<false>), grid, dim3(256), 0, st, a);
        const int64_t tiles = (n * cutoff + BEY_TILE - 1) / BEY_TILE;
        EL_LAUNCH("k_beyond_hist", k_beyond_hist<false>, dim3((unsigned)tiles), dim3(256), 0, st, rec_idx, ld, u_start, n, test_indptr,
                  (const double*)nullptr, 0, (int)cutoff, (int32_t)n_items, hist);
    }
    met_tree_sum<BEY_N, -1>(st, a.rows, n, m.part, sums);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_beyond_hist_finish(el_ctx* ctx, void* stream, const int32_t* hist, int64_t n_items, int64_t* stats, double* nov, void* ws,
                                     size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(hist && stats && nov, "el_beyond_hist_finish: null pointer");
    EL_REQUIRE(n_items >= 1 && n_items < (1LL << 31), "el_beyond_hist_finish: bad item count");
    BeyWs w;
    EL_REQUIRE(bey_carve(n_items, ws, &w) == 0, "el_beyond_hist_finish: rocprim size query failed");
    EL_REQUIRE(ws != nullptr && ws_bytes >= w.total, "el_beyond_hist_finish: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    EL_CHECK_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st));
    {
        ElKernelTimer t("rocprim_radix_sort_keys", st);
        size_t tb = w.tmp_bytes;
        EL_CHECK_HIP(rocprim::radix_sort_keys(w.tmp, tb, reinterpret_cast<const u32*>(hist), w.sorted, (unsigned)n_items, 0, 32, st));
    }
    const int64_t want = (n_items + 255) / 256;
    EL_LAUNCH("k_beyond_hist_stats", k_beyond_hist_stats, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, st, (const u32*)w.sorted,
              n_items, reinterpret_cast<unsigned long long*>(stats));
    EL_LAUNCH("k_beyond_nov", k_beyond_nov, dim3((unsigned)want), dim3(256), 0, st, hist, n_items,
              reinterpret_cast<const unsigned long long*>(stats), nov);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_beyond_entropy(el_ctx* ctx, void* stream, const int32_t* rec_idx, int64_t ld, int64_t u_start, int64_t u_stop,
                                 const int64_t* test_indptr, int32_t cutoff, int64_t n_items, const double* nov, double* sum, void* ws,
                                 size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(u_stop >= u_start, "el_beyond_entropy: u_stop < u_start");
    const int64_t n = u_stop - u_start;
    if (n == 0) return 0;
    EL_REQUIRE(rec_idx && test_indptr && nov && sum, "el_beyond_entropy: null pointer");
    MET_REQUIRE_CUTOFF("el_beyond_entropy", cutoff, ld);
    EL_REQUIRE(n_items >= 1 && n_items < (1LL << 31), "el_beyond_entropy: bad item count");
    MetWs m;
    EL_REQUIRE(ws != nullptr && ws_bytes >= met_carve(n, 1, ws, &m), "el_beyond_entropy: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double *rows = m.rows, *part = m.part;
    EL_LAUNCH("k_beyond_entropy", k_beyond_entropy, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, rec_idx, ld, u_start, n, test_indptr,
              (int)cutoff, (int32_t)n_items, nov, rows);
    met_tree_sum<1, -1>(st, rows, n, part, sum);
    EL_CHECK_LAUNCH();
    return 0;
}
