// A user's held-out row as the metric kernels read it: relevance, gain, the lookup of a list entry and the IDCG pass, once for the
// accuracy (el_metrics.hip), beyond-accuracy (el_metrics_beyond.hip), fairness (el_metrics_fair.hip) and rank (el_rank.hip) kernels.
// The nDCG of k_rec_metrics and of k_fair_users agree bit for bit because both run met_row_idcg and met_lookup.
//
// The reference's definitions (evaluation/):
//   relevance   test items with rating >= threshold                         relevance/relevance.py:87-96
//   gain        2^(rating - threshold + 1) - 1, discount ln2 / ln(rank + 2)  relevance/relevance.py:49-55,71-82
//   IDCG        the user's gains sorted descending, the first `cutoff` discounted   metrics/accuracy/ndcg/ndcg.py:68-125
// Arithmetic in fp64 like the reference; the discount table comes from the host (Python's math.log values).  A held-out CSR without
// ratings (tr == nullptr) rates every entry 1.
#pragma once
#include "el_common.h"
#include "el_topk_common.h"

#define MET_MAXCUT 512   // largest cutoff of every metric entry point
#define MET_BUF 1024     // LDS gain buffer per wave (kept <= MET_MAXCUT + incoming)

// the cutoff and list-width check of an entry point; `who` is its name, a string literal
#define MET_REQUIRE_CUTOFF(who, cutoff, ld)                                                                                          \
    EL_REQUIRE((cutoff) >= 1 && (cutoff) <= MET_MAXCUT && (int64_t)(cutoff) <= (ld), who ": cutoff %d unsupported (1..%d, <= ld)", \
               cutoff, MET_MAXCUT)

__device__ __forceinline__ double met_rating(const float* __restrict__ tr, int64_t e) { return tr ? (double)tr[e] : 1.0; }
__device__ __forceinline__ double met_gain(double r, double thr) { return exp2(r - thr + 1.0) - 1.0; }

// A list entry against the held-out row [t0, t1) (ids ascending): is it there (found, at pos), and is it relevant (rel, with its gain)
struct MetEntry {
    bool found, rel;
    int64_t pos;
    double gain;
};
__device__ __forceinline__ MetEntry met_lookup(const int32_t* __restrict__ ti, const float* __restrict__ tr, int64_t t0, int64_t t1,
                                               int32_t item, double thr) {
    MetEntry m{false, false, el_lower_bound(ti, t0, t1, item), 0.0};
    if (m.pos < t1 && ti[m.pos] == item) {
        m.found = true;
        const double r = met_rating(tr, m.pos);
        if (r >= thr) {
            m.rel = true;
            m.gain = met_gain(r, thr);
        }
    }
    return m;
}

// One wave over the held-out row [t0, t1) in chunks of 64: the number of relevant entries, and the IDCG of the `cutoff` largest gains.
// The gains are compacted into gb (MET_BUF slots of this wave's LDS); when fewer than 64 slots are free the buffer is sorted and cut
// to the best `cutoff`.  hook(e, relevant) runs in every lane of every chunk (e >= t1 in the lanes behind the row's end).
struct MetRow {
    double nrel, idcg;
};
template <class Hook>
__device__ __forceinline__ MetRow met_row_idcg(u64* gb, const float* __restrict__ tr, int64_t t0, int64_t t1, double thr, int cutoff,
                                               const double* __restrict__ disc, int lane, Hook hook) {
    int cnt = 0;
    double nrel = 0.0;
    auto sort_keep = [&]() {
        int n2 = 64;
        while (n2 < cnt) n2 <<= 1;
        for (int t = cnt + lane; t < n2; t += 64) gb[t] = 0ull;
        el_wave_lds_sync();
        el_wave_bitonic_desc(gb, n2, lane);               // positive doubles order as their bit patterns
        cnt = cnt < cutoff ? cnt : cutoff;
    };
    for (int64_t b = t0; b < t1; b += 64) {
        const int64_t e = b + lane;
        bool relv = false;
        double g = 0.0;
        if (e < t1) {
            const double r = met_rating(tr, e);
            relv = r >= thr;
            if (relv) g = met_gain(r, thr);
        }
        const u64 bal = __ballot(relv);
        if (relv) gb[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = (u64)__double_as_longlong(g);
        cnt += __popcll(bal);
        nrel += (double)__popcll(bal);
        el_wave_lds_sync();
        if (cnt > MET_BUF - 64) sort_keep();
        hook(e, relv);
    }
    sort_keep();
    double idcg = 0.0;
    for (int t = lane; t < cnt; t += 64) idcg += __longlong_as_double((long long)gb[t]) * disc[t];
    return MetRow{nrel, el_group_sum(idcg, 64)};
}
