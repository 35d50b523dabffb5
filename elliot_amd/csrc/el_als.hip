// Alternating least squares (iALS / WRMF).
//
// Replaces the per-row Python loops of iALS_model.py:43-72 (np.linalg.inv) and wrmf_model.py:40-58 (spsolve):
//   el_als_gram   G = Y^T Y                        fixed row slots, slot sums added in slot order, lower triangle mirrored
//   el_als_solve  for every row r of a CSR pattern over the rows of Y:
//                   A_r = G + w_A * S_r + lambda I,   S_r = sum_{j in r} y_j y_j^T   (ascending CSR position)
//                   b_r = w_b * s_r,                  s_r = sum_{j in r} y_j
//                   x_r = A_r^{-1} b_r                Cholesky A = L L^T with the forward solve fused, then L^T x = z
//
// Everything is fp64 and nothing is added with atomics: each sum has one owner and a fixed order, so the same input gives the same
// bits on every run.  Layout:
//   * a row is solved by a lane group of T lanes (T = 16 for F <= 16, 64 for F <= 64, 256 for F <= 128), 256 / T rows per
//     workgroup; lane l of a group owns the entries p = l + m T of the packed lower triangle of A (p = i (i + 1) / 2 + j, j <= i)
//     in registers through the whole build, factorisation and back substitution; LDS holds the staged y rows and three F-vectors
//   * rows longer than piece_len are listed by the caller (long_rows, long_first): each piece of piece_len positions is summed by
//     one workgroup into its own slot (S, s unweighted), and the row's solve adds its slots in piece order
#include "el_common.h"

#define ALS_MAX_F 128
#define ALS_TILE 16            // y rows staged per pass (solve, pieces)
#define ALS_GRAM_TILE 32       // y rows staged per pass (Gram)
#define ALS_GRAM_MIN_ROWS 256  // rows per Gram slot, at least
#define ALS_GRAM_MAX_SLOTS 512
#define ALS_NONE 0x7fffffff

namespace {

__device__ __forceinline__ int als_tri(int i) { return i * (i + 1) / 2; }

// packed lower-triangle index p -> (i << 8) | j
__device__ __forceinline__ int als_pair(int p) {
    int r = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (als_tri(r + 1) <= p) ++r;
    while (als_tri(r) > p) --r;
    return (r << 8) | (p - als_tri(r));
}

int64_t als_gram_rows_per_slot(int64_t n) {
    int64_t c = (n + ALS_GRAM_MAX_SLOTS - 1) / ALS_GRAM_MAX_SLOTS;
    return c < ALS_GRAM_MIN_ROWS ? ALS_GRAM_MIN_ROWS : c;
}

// ---- Gram ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_als_gram_part(const double* __restrict__ Y, int64_t n, int F, int64_t chunk,
                                                       double* __restrict__ part) {
    extern __shared__ double sy[];                       // [ALS_GRAM_TILE][F]
    constexpr int MAXP = 33;                             // ceil(128 * 129 / 2 / 256)
    const int P = als_tri(F);
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
    int pij[MAXP];
    double acc[MAXP];
#pragma unroll
    for (int m = 0; m < MAXP; ++m) {
        const int p = threadIdx.x + m * 256;
        pij[m] = p < P ? als_pair(p) : 0;
        acc[m] = 0.0;
    }
    for (int64_t t0 = r0; t0 < r1; t0 += ALS_GRAM_TILE) {
        const int rows = (int)(r1 - t0 < ALS_GRAM_TILE ? r1 - t0 : ALS_GRAM_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * F; e += 256) sy[e] = Y[t0 * F + e];
        __syncthreads();
        for (int q = 0; q < rows; ++q) {
            const double* y = sy + q * F;
#pragma unroll
            for (int m = 0; m < MAXP; ++m)
                if ((int)threadIdx.x + m * 256 < P) acc[m] = __fma_rn(y[pij[m] >> 8], y[pij[m] & 255], acc[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < MAXP; ++m) {
        const int p = threadIdx.x + m * 256;
        if (p < P) part[(int64_t)blockIdx.x * P + p] = acc[m];
    }
}

__global__ __launch_bounds__(256) void k_als_gram_sum(const double* __restrict__ part, int nslots, int F, double* __restrict__ G) {
    const int P = als_tri(F);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int q = 0; q < nslots; ++q) s = __dadd_rn(s, part[(int64_t)q * P + p]);
    const int ij = als_pair(p), i = ij >> 8, j = ij & 255;
    G[i * F + j] = s;
    G[j * F + i] = s;
}

// ---- solve ---------------------------------------------------------------------------------------------------------------------
struct AlsSolve {
    const int64_t* indptr;
    const int32_t* indices;
    int64_t n_rows;
    const double* Y;          // [n_other, F]
    int F;
    const double* G;          // [F, F]
    double wA, wB, lambda;
    int flags;
    const int32_t* long_rows; // [n_long] ascending
    const int64_t* long_first;// [n_long + 1] first piece of each long row
    int64_t n_long;
    int64_t piece_len;
    double* slots;            // [n_pieces][P + F]
    double* X;                // [n_rows, F]
    int32_t* status;          // [0] smallest row with a non-positive pivot, [1] smallest long row the plan does not match
};

__global__ void k_als_status_init(int32_t* status) {
    if (threadIdx.x < 2) status[threadIdx.x] = ALS_NONE;
}

// one workgroup per piece of a long row: unweighted (S, s) over the piece's positions, in ascending order
__global__ __launch_bounds__(256) void k_als_piece(AlsSolve a) {
    extern __shared__ double sy[];                       // [ALS_TILE][F]
    constexpr int MAXP = 33;
    const int F = a.F, P = als_tri(F);
    const int64_t piece = blockIdx.x;
    int64_t lo = 0, hi = a.n_long - 1;                   // last long row whose first piece <= piece
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.long_first[mid] <= piece) lo = mid;
        else hi = mid - 1;
    }
    const int64_t row = a.long_rows[lo];
    const int64_t q = piece - a.long_first[lo];
    bool ok = row >= 0 && row < a.n_rows && q >= 0;
    int64_t p0 = 0, p1 = 0;
    if (ok) {
        const int64_t s = a.indptr[row], e = a.indptr[row + 1];
        p0 = s + q * a.piece_len;
        p1 = p0 + a.piece_len < e ? p0 + a.piece_len : e;
        ok = e - s > a.piece_len && p0 < e && a.long_first[lo + 1] - a.long_first[lo] == (e - s + a.piece_len - 1) / a.piece_len;
    }
    if (!ok) {                                           // the caller's plan does not describe this CSR (uniform: whole workgroup)
        if (threadIdx.x == 0) atomicMin(a.status + 1, (int32_t)(row >= 0 && row < a.n_rows ? row : 0));
        return;
    }
    int pij[MAXP];
    double acc[MAXP];
    double sb = 0.0;
#pragma unroll
    for (int m = 0; m < MAXP; ++m) {
        const int p = threadIdx.x + m * 256;
        pij[m] = p < P ? als_pair(p) : 0;
        acc[m] = 0.0;
    }
    for (int64_t t0 = p0; t0 < p1; t0 += ALS_TILE) {
        const int rows = (int)(p1 - t0 < ALS_TILE ? p1 - t0 : ALS_TILE);
        __syncthreads();
        for (int x = threadIdx.x; x < rows * F; x += 256) {
            const int r = x / F, c = x - r * F;
            sy[x] = a.Y[(int64_t)a.indices[t0 + r] * F + c];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const double* y = sy + r * F;
#pragma unroll
            for (int m = 0; m < MAXP; ++m)
                if ((int)threadIdx.x + m * 256 < P) acc[m] = __fma_rn(y[pij[m] >> 8], y[pij[m] & 255], acc[m]);
            if ((int)threadIdx.x < F) sb = __dadd_rn(sb, y[threadIdx.x]);
        }
    }
    double* out = a.slots + piece * (P + F);
#pragma unroll
    for (int m = 0; m < MAXP; ++m) {
        const int p = threadIdx.x + m * 256;
        if (p < P) out[p] = acc[m];
    }
    if ((int)threadIdx.x < F) out[P + threadIdx.x] = sb;
}

template <int T, int MAXP>
__global__ __launch_bounds__(256) void k_als_solve(AlsSolve a) {
    constexpr int NG = 256 / T;                          // rows per workgroup
    extern __shared__ double lds[];
    __shared__ int64_t glen[NG];
    const int F = a.F, P = als_tri(F);
    const int g = threadIdx.x / T, lane = threadIdx.x % T;
    double* tile = lds + (size_t)g * (ALS_TILE * F + 3 * F);   // [ALS_TILE][F]
    double* col = tile + ALS_TILE * F;                   // column k of the trailing matrix; later x
    double* lcol = col + F;                              // column k of L
    double* v = lcol + F;                                // b, then z
    const int64_t row = (int64_t)blockIdx.x * NG + g;
    const bool live = row < a.n_rows;
    const int64_t s = live ? a.indptr[row] : 0;
    const int64_t len = live ? a.indptr[row + 1] - s : 0;
    const bool skip = live && len == 0 && (a.flags & EL_ALS_SKIP_EMPTY);
    const bool is_long = live && len > a.piece_len;
    const int64_t mylen = (live && !is_long) ? len : 0;

    int pij[MAXP];
    double acc[MAXP];
    double sb = 0.0;
#pragma unroll
    for (int m = 0; m < MAXP; ++m) {
        const int p = lane + m * T;
        pij[m] = p < P ? als_pair(p) : 0;
        acc[m] = 0.0;
    }
    if (lane == 0) glen[g] = mylen;
    __syncthreads();
    int64_t maxlen = 0;
#pragma unroll
    for (int x = 0; x < NG; ++x) maxlen = glen[x] > maxlen ? glen[x] : maxlen;

    // S and s of a short row, ascending CSR position (the trip count is the workgroup's longest row: barriers stay uniform)
    for (int64_t t0 = 0; t0 < maxlen; t0 += ALS_TILE) {
        const int rows = mylen > t0 ? (int)(mylen - t0 < ALS_TILE ? mylen - t0 : ALS_TILE) : 0;
        __syncthreads();
        for (int x = lane; x < rows * F; x += T) {
            const int r = x / F, c = x - r * F;
            tile[x] = a.Y[(int64_t)a.indices[s + t0 + r] * F + c];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const double* y = tile + r * F;
#pragma unroll
            for (int m = 0; m < MAXP; ++m)
                if (lane + m * T < P) acc[m] = __fma_rn(y[pij[m] >> 8], y[pij[m] & 255], acc[m]);
            if (lane < F) sb = __dadd_rn(sb, y[lane]);
        }
    }
    // a long row: its pieces' slots in piece order
    if (is_long) {
        int64_t lo = 0, hi = a.n_long - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)a.long_rows[mid] < row) lo = mid + 1;
            else hi = mid;
        }
        if (a.n_long > 0 && (int64_t)a.long_rows[lo] == row) {
            const int64_t q0 = a.long_first[lo], q1 = a.long_first[lo + 1];
            for (int64_t q = q0; q < q1; ++q) {
                const double* in = a.slots + q * (P + F);
#pragma unroll
                for (int m = 0; m < MAXP; ++m)
                    if (lane + m * T < P) acc[m] = q == q0 ? in[lane + m * T] : __dadd_rn(acc[m], in[lane + m * T]);
                if (lane < F) sb = q == q0 ? in[P + lane] : __dadd_rn(sb, in[P + lane]);
            }
        } else if (lane == 0) {
            atomicMin(a.status + 1, (int32_t)row);
        }
    }
    // A = G + w_A S + lambda I (packed lower triangle, in registers), b = w_b s
#pragma unroll
    for (int m = 0; m < MAXP; ++m) {
        if (lane + m * T < P) {
            const int i = pij[m] >> 8, j = pij[m] & 255;
            double x = __dadd_rn(a.G[i * F + j], __dmul_rn(a.wA, acc[m]));
            if (i == j) x = __dadd_rn(x, a.lambda);
            acc[m] = x;
        }
    }
    if (lane < F) v[lane] = __dmul_rn(a.wB, sb);

    // right-looking Cholesky; the forward solve L z = b rides along (z_k = v_k / L_kk, then v_i -= L_ik z_k)
    bool bad = false;
    for (int k = 0; k < F; ++k) {
#pragma unroll
        for (int m = 0; m < MAXP; ++m)
            if (lane + m * T < P && (pij[m] & 255) == k) col[pij[m] >> 8] = acc[m];
        __syncthreads();
        const double d = col[k];
        bad = bad || !(d > 0.0);
        const double sq = __dsqrt_rn(d);
        const double z = __ddiv_rn(v[k], sq);
        if (lane > k && lane < F) {
            const double l = __ddiv_rn(col[lane], sq);
            lcol[lane] = l;
            v[lane] = __fma_rn(-l, z, v[lane]);
        }
        __syncthreads();
        if (lane == k) v[k] = z;
#pragma unroll
        for (int m = 0; m < MAXP; ++m) {
            if (lane + m * T < P) {
                const int i = pij[m] >> 8, j = pij[m] & 255;
                if (j == k) acc[m] = i == k ? sq : lcol[i];
                else if (j > k) acc[m] = __fma_rn(-lcol[i], lcol[j], acc[m]);
            }
        }
    }
    __syncthreads();
    // back substitution L^T x = z: x_k = z_k / L_kk, then z_j -= L_kj x_k (j < k); x goes to col
    for (int k = F - 1; k >= 0; --k) {
#pragma unroll
        for (int m = 0; m < MAXP; ++m)
            if (lane + m * T < P && pij[m] == ((k << 8) | k)) col[k] = __ddiv_rn(v[k], acc[m]);
        __syncthreads();
        const double xk = col[k];
#pragma unroll
        for (int m = 0; m < MAXP; ++m)
            if (lane + m * T < P && (pij[m] >> 8) == k && (pij[m] & 255) < k) {
                const int j = pij[m] & 255;
                v[j] = __fma_rn(-acc[m], xk, v[j]);
            }
        __syncthreads();
    }
    if (!live || skip) return;
    if (bad) {
        if (lane == 0) atomicMin(a.status, (int32_t)row);
        return;
    }
    if (lane < F) a.X[row * F + lane] = col[lane];
}

template <int T, int MAXP>
int als_launch_solve(const AlsSolve& a, hipStream_t st) {
    constexpr int NG = 256 / T;
    const size_t lds = (size_t)NG * (ALS_TILE * a.F + 3 * a.F) * sizeof(double);
    const int64_t blocks = (a.n_rows + NG - 1) / NG;
    EL_LAUNCH("k_als_solve", (k_als_solve<T, MAXP>), dim3((unsigned)blocks), dim3(256), lds, st, a);
    EL_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t el_als_gram_ws_bytes(int64_t n, int32_t F) {
    if (n <= 0 || F <= 0 || F > ALS_MAX_F) return 0;
    const int64_t chunk = als_gram_rows_per_slot(n);
    const int64_t nslots = (n + chunk - 1) / chunk;
    return el_align256((size_t)nslots * (size_t)(F * (F + 1) / 2) * sizeof(double));
}

extern "C" int el_als_gram(el_ctx* ctx, void* stream, const double* Y, int64_t n, int32_t F, double* G, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(F >= 1 && F <= ALS_MAX_F, "el_als_gram: factors=%d unsupported (1..%d)", F, ALS_MAX_F);
    EL_REQUIRE(n >= 0 && n < 0x7fffffffLL, "el_als_gram: bad row count %lld", (long long)n);
    EL_REQUIRE(G != nullptr && (n == 0 || Y != nullptr), "el_als_gram: null pointer");
    const size_t need = el_als_gram_ws_bytes(n, F);
    EL_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need), "el_als_gram: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t chunk = als_gram_rows_per_slot(n > 0 ? n : 1);
    const int nslots = n > 0 ? (int)((n + chunk - 1) / chunk) : 0;
    double* part = (double*)ws;
    if (nslots > 0) {
        const size_t lds = (size_t)ALS_GRAM_TILE * F * sizeof(double);
        EL_LAUNCH("k_als_gram_part", k_als_gram_part, dim3(nslots), dim3(256), lds, st, Y, n, (int)F, chunk, part);
        EL_CHECK_LAUNCH();
    }
    const int P = F * (F + 1) / 2;
    EL_LAUNCH("k_als_gram_sum", k_als_gram_sum, dim3((P + 255) / 256), dim3(256), 0, st, part, nslots, (int)F, G);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t el_als_solve_ws_bytes(int64_t n_pieces, int32_t F) {
    if (n_pieces <= 0 || F <= 0 || F > ALS_MAX_F) return 0;
    return el_align256((size_t)n_pieces * (size_t)(F * (F + 1) / 2 + F) * sizeof(double));
}

extern "C" int el_als_solve(el_ctx* ctx, void* stream, const int64_t* indptr, const int32_t* indices, int64_t n_rows,
                            const double* Y, int64_t n_other, int32_t F, const double* G, double w_A, double w_b, double lambda,
                            int flags, const int32_t* long_rows, const int64_t* long_first, int64_t n_long, int64_t n_pieces,
                            int64_t piece_len, double* X, int32_t* status, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(F >= 1 && F <= ALS_MAX_F, "el_als_solve: factors=%d unsupported (1..%d)", F, ALS_MAX_F);
    EL_REQUIRE(indptr && indices && Y && G && X && status, "el_als_solve: null pointer");
    EL_REQUIRE(n_rows >= 0 && n_rows < 0x7fffffffLL && n_other >= 1 && n_other < 0x7fffffffLL,
               "el_als_solve: bad sizes n_rows=%lld n_other=%lld", (long long)n_rows, (long long)n_other);
    EL_REQUIRE((flags & ~EL_ALS_SKIP_EMPTY) == 0, "el_als_solve: unknown flags 0x%x", flags);
    EL_REQUIRE(piece_len >= 1, "el_als_solve: piece_len must be >= 1");
    EL_REQUIRE(n_long >= 0 && (n_long == 0 || (long_rows && long_first)), "el_als_solve: long-row plan needs both arrays");
    EL_REQUIRE(n_pieces <= 0 || n_long > 0, "el_als_solve: bad long-row plan (%lld pieces but no long row)", (long long)n_pieces);
    hipStream_t st = (hipStream_t)stream;
    EL_LAUNCH("k_als_status_init", k_als_status_init, dim3(1), dim3(64), 0, st, status);
    EL_CHECK_LAUNCH();
    if (n_rows == 0) return 0;
    EL_REQUIRE(n_pieces >= n_long && n_pieces < 0x7fffffffLL, "el_als_solve: bad long-row plan (%lld rows, %lld pieces)",
               (long long)n_long, (long long)n_pieces);
    const size_t need = el_als_solve_ws_bytes(n_pieces, F);
    EL_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need), "el_als_solve: workspace too small (need %zu bytes)", need);
    AlsSolve a;
    a.indptr = indptr, a.indices = indices, a.n_rows = n_rows;
    a.Y = Y, a.F = F, a.G = G;
    a.wA = w_A, a.wB = w_b, a.lambda = lambda, a.flags = flags;
    a.long_rows = long_rows, a.long_first = long_first, a.n_long = n_long, a.piece_len = piece_len;
    a.slots = (double*)ws, a.X = X, a.status = status;
    if (n_pieces > 0) {
        const size_t lds = (size_t)ALS_TILE * F * sizeof(double);
        EL_LAUNCH("k_als_piece", k_als_piece, dim3((unsigned)n_pieces), dim3(256), lds, st, a);
        EL_CHECK_LAUNCH();
    }
    if (F <= 16) return als_launch_solve<16, 9>(a, st);
    if (F <= 64) return als_launch_solve<64, 33>(a, st);
    return als_launch_solve<256, 33>(a, st);
}
