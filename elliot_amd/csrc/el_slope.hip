// SlopeOne (Lemire & Maclachlan 2005): exact deviation build, scoring table, ordered fp64 scoring.
//
// Replaces SlopeOneModel.initialize and predict (slope_one_model.py:19-47):
//   el_slope_build    freq[c, x] = users who rated both, S[c, x] = sum_u (r_uc - r_ux): integer counts in LDS, then
//                     dev = S / freq on the upper triangle, its exact negation below, +0 on the diagonal
//   el_slope_table    T[j, i] = dev[i, j] where freq[i, j] > 0, a quiet NaN elsewhere: the scoring kernel's one 8-byte stream
//   el_slope_scores   P[u, i] = mean_u + (sum over row u in dict order of T[j, i], NaN cells skipped) / (cells added)
//
// Every sum of the build is an integer (ratings times 1 or 2) and every order gives the same counts; the scoring sum is one
// __dadd_rn per cell in the stored order of the row, from +0.  Nothing floating-point is added with atomics and there is no
// fma: with integer or half-step ratings freq, dev and every prediction equal the reference's bit for bit.
#include "el_common.h"
#include "el_rowscore.h"

#define SLOPE_THREADS 256
#define SLOPE_TILE 8192          // LDS cells per pass over the catalogue (a freq and an S counter each)

namespace {

struct SlopeBuild {
    const int64_t* tp;      // R^T: item c -> users, int64[I + 1]
    const int32_t* ti;
    const int32_t* tv;      // integer ratings (ratings * scale)
    const int64_t* rp;      // R: user -> items, rows ascending
    const int32_t* ri;
    const int32_t* rv;
    int64_t I;
    double inv_s;           // 1 / scale (exact)
    int tile;
    int32_t* freq;
    int64_t ldf;
    double* dev;
    int64_t ldd;
    double* T;              // may be null
    int64_t ldt;
};

__device__ __forceinline__ double slope_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// one workgroup per row c of freq / dev: the two counters of every column of one tile at a time, written densely
template <typename ACC>
__global__ __launch_bounds__(SLOPE_THREADS) void k_slope_build(SlopeBuild p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ACC* sacc = reinterpret_cast<ACC*>(smem);                                  // [tile]
    int* facc = reinterpret_cast<int*>(sacc + p.tile);                         // [tile]
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int64_t p0 = p.tp[c], p1 = p.tp[c + 1];
    const bool tiled = p.tile < p.I;
    for (int64_t x0 = 0; x0 < p.I; x0 += p.tile) {
        const int64_t x1 = (x0 + p.tile < p.I) ? x0 + p.tile : p.I;
        const int w = (int)(x1 - x0);
        for (int i = tid; i < w; i += SLOPE_THREADS) {
            sacc[i] = 0;
            facc[i] = 0;
        }
        __syncthreads();
        el_count_diff_expand<SLOPE_THREADS / 64>(facc, sacc, p.ti, p.tv, p0, p1, p.rp, p.ri, p.rv, x0, x1, tiled);
        __syncthreads();
        int32_t* fr = p.freq + c * p.ldf + x0;
        double* dv = p.dev + c * p.ldd + x0;
        double* tb = p.T ? p.T + c * p.ldt + x0 : nullptr;
        for (int i = tid; i < w; i += SLOPE_THREADS) {
            const int64_t x = x0 + i;
            const int f = facc[i];
            const int64_t s = (int64_t)sacc[i];                                // S[c, x]; S[x, c] = -s exactly
            const double fd = (double)f;
            // slope_one_model.py:30-34: the upper cell is the quotient (or +0), the lower one its negation, the diagonal +0
            const double up_cx = f ? __ddiv_rn(__dmul_rn((double)s, p.inv_s), fd) : 0.0;       // dev[c, x] if c < x
            const double up_xc = f ? __ddiv_rn(__dmul_rn((double)(-s), p.inv_s), fd) : 0.0;    // dev[x, c] if x < c
            fr[i] = f;
            dv[i] = x == c ? 0.0 : (x > c ? up_cx : -up_xc);
            if (tb) tb[i] = !f ? slope_nan() : (x == c ? 0.0 : (x < c ? up_xc : -up_cx));      // T[c, x] = dev[x, c]
        }
        __syncthreads();                                  // every counter is read before the next tile clears it
    }
}

// T[j, i] = dev[i, j] where freq[i, j] > 0, on k_transpose_f64 (el_rowscore.h)
struct SlopeTableLoad {
    const int32_t* freq;
    int64_t ldf;
    const double* dev;
    int64_t ldd;
    __device__ double operator()(int64_t i, int64_t j) const { return freq[i * ldf + j] > 0 ? dev[i * ldd + j] : slope_nan(); }
};

// slope_one_model.py:42-47 on k_row_scores: a NaN cell (freq[c, j] == 0) is not part of Ri
struct SlopeScoreOp : RowScoreOp<double> {
    struct Acc { double a; int n; };
    const double* mean;
    __device__ void step(Acc& s, int, double v) const {
        if (v == v) {
            s.a = __dadd_rn(s.a, v);
            ++s.n;
        }
    }
    __device__ double base(int64_t u) const { return mean[u]; }
    __device__ double finish(const Acc& s, double m) const { return s.n ? __dadd_rn(m, __ddiv_rn(s.a, (double)s.n)) : m; }
};

}  // namespace

extern "C" int el_slope_build(el_ctx* ctx, void* stream, const int64_t* t_indptr, const int32_t* t_indices, const int32_t* t_vals,
                              const int64_t* r_indptr, const int32_t* r_indices, const int32_t* r_vals, int64_t I, int64_t U,
                              int32_t scale, int64_t max_deg, int32_t max_abs, int32_t* freq, int64_t ldf, double* dev,
                              int64_t ldd, double* T, int64_t ldt) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(t_indptr && t_indices && t_vals && r_indptr && r_indices && r_vals && freq && dev, "el_slope_build: null pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && U >= 0 && U < 0x7fffffffLL, "el_slope_build: bad sizes I=%lld U=%lld", (long long)I,
               (long long)U);
    EL_REQUIRE(ldf >= I && ldd >= I && (T == nullptr || ldt >= I), "el_slope_build: leading dimensions below I=%lld", (long long)I);
    EL_REQUIRE(scale == 1 || scale == 2, "el_slope_build: scale=%d unsupported (1 or 2)", scale);
    EL_REQUIRE(max_deg >= 0 && max_deg < 0x7fffffffLL && max_abs >= 0, "el_slope_build: bad max_deg / max_abs");
    const double bound = 2.0 * (double)max_deg * (double)max_abs;
    EL_REQUIRE(bound < 9.0e15, "el_slope_build: sums up to %.3g do not fit the exact range", bound);
    SlopeBuild p;
    p.tp = t_indptr, p.ti = t_indices, p.tv = t_vals;
    p.rp = r_indptr, p.ri = r_indices, p.rv = r_vals;
    p.I = I, p.inv_s = scale == 2 ? 0.5 : 1.0;
    p.tile = (int)(I < SLOPE_TILE ? I : SLOPE_TILE);
    p.freq = freq, p.ldf = ldf, p.dev = dev, p.ldd = ldd, p.T = T, p.ldt = ldt;
    hipStream_t st = (hipStream_t)stream;
    if (bound < 2147483647.0) {
        const size_t lds = (size_t)p.tile * (sizeof(int) + sizeof(int));
        EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_slope_build<int>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
        EL_LAUNCH("k_slope_build", k_slope_build<int>, dim3((unsigned)I), dim3(SLOPE_THREADS), lds, st, p);
    } else {
        const size_t lds = (size_t)p.tile * (sizeof(unsigned long long) + sizeof(int));
        EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_slope_build<unsigned long long>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        EL_LAUNCH("k_slope_build", k_slope_build<unsigned long long>, dim3((unsigned)I), dim3(SLOPE_THREADS), lds, st, p);
    }
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_slope_table(el_ctx* ctx, void* stream, const int32_t* freq, int64_t ldf, const double* dev, int64_t ldd,
                              int64_t I, double* T, int64_t ldt) {
    return el_transpose_f64("el_slope_table", "k_slope_table", ctx, stream, freq && dev && T, ldf >= I && ldd >= I && ldt >= I,
                            SlopeTableLoad{freq, ldf, dev, ldd}, I, T, ldt);
}

extern "C" int el_slope_scores(el_ctx* ctx, void* stream, const int64_t* indptr, const int32_t* indices, const double* user_mean,
                               int64_t u_start, int64_t u_stop, const double* T, int64_t ldt, int64_t I, double* P, int64_t ldp) {
    return el_row_scores("el_slope_scores", "k_slope_scores", ctx, stream, indptr && indices && user_mean && T && P, indptr,
                         indices, u_start, u_stop, SlopeScoreOp{{T, ldt}, user_mean}, I, P, ldp);
}
