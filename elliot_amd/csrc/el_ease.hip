// EASE^R (Steck 2019): Gram, dense fp64 inverse, weights and CSR x dense scoring.
//
// Replaces EASER.train (ease_r.py:76-93):
//   el_ease_gram         G = R^T R with the diagonal replaced by (float)(n_i + l2_norm)   exact integer counts in LDS
//   el_inv_f64           A <- A^-1 by LU with partial pivoting, then triangular solves against the identity
//   el_ease_weights      B[j][i] = (float)(-P[j][i] / P[i][i]), B[i][i] = 0                 correctly rounded fp64 division
//   el_csr_dense_scores  S[u, :] = sum over row u of R, stored order, of R[u, a] * B[a, :]   scipy's csr_matvecs order
//
// The inverse is a right-looking blocked LU on the augmented matrix [A | I] with panels of INV_NB columns:
//   per column j    k_lu_pivot  (one workgroup): largest |a| of column j on rows >= j, ties to the smallest row (LAPACK idamax),
//                               swap of the two full rows of A and of the right-hand sides, division of the column below j
//                   k_lu_panel: rank-1 update of the panel's remaining columns
//   per panel       k_inv_trsm: U12 = L11^-1 A12 and the same for the right-hand sides; k_inv_update: the trailing update
//                   A22 -= L21 U12 and Y2 -= L21 Y1 on v_mfma_f64_16x16x4_f64
// then the backward solve U X = Y by block rows from the bottom (k_inv_trsm + k_inv_update) and X is copied into A.  Every sum has
// one owner and a fixed order and nothing floating-point is added with atomics: the same input gives the same bits on every run.
// Kernel boundaries are the only grid-wide synchronisation.
#include "el_common.h"
#include "el_rowscore.h"

#define EASE_GRAM_THREADS 256
#define EASE_GRAM_TILE 16384     // LDS counters per pass over the catalogue
#define INV_NB 64                // panel width of the LU (the inner dimension of every MFMA update)
#define INV_TILE 64              // rows and columns of C per workgroup of k_inv_update
#define INV_NONE 0x7fffffff

typedef double el_d4 __attribute__((ext_vector_type(4)));

namespace {

// ---- Gram -------------------------------------------------------------------------------------------------------------------
struct EaseGram {
    const int64_t* tp;      // R^T: item c -> users, int64[I + 1]
    const int32_t* ti;
    const int32_t* tv;      // integer ratings (ratings * scale)
    const int64_t* rp;      // R: user -> items, rows ascending
    const int32_t* ri;
    const int32_t* rv;
    int64_t I;
    double l2;
    double inv_s2;          // 1 / scale^2 (exact)
    int tile;
    double* G;
    int64_t ldg;
};

// one workgroup per row c of G: counters of the co-rated sums over one tile of columns at a time, written densely
template <typename ACC>
__global__ __launch_bounds__(EASE_GRAM_THREADS) void k_ease_gram(EaseGram p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ACC* acc = reinterpret_cast<ACC*>(smem);                                   // [tile]
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int64_t p0 = p.tp[c], p1 = p.tp[c + 1];
    // ease_r.py:80-82: the stored-entry count plus l2_norm, a double, assigned into the float32 matrix
    const double diag = (double)__double2float_rn(__dadd_rn((double)(p1 - p0), p.l2));
    const bool tiled = p.tile < p.I;
    for (int64_t x0 = 0; x0 < p.I; x0 += p.tile) {
        const int64_t x1 = (x0 + p.tile < p.I) ? x0 + p.tile : p.I;
        const int w = (int)(x1 - x0);
        for (int i = tid; i < w; i += EASE_GRAM_THREADS) acc[i] = 0;
        __syncthreads();
        el_count_expand<EASE_GRAM_THREADS / 64>(acc, p.ti, p.tv, p0, p1, p.rp, p.ri, p.rv, x0, x1, tiled);
        __syncthreads();
        double* g = p.G + c * p.ldg + x0;
        for (int i = tid; i < w; i += EASE_GRAM_THREADS)
            g[i] = (x0 + i == c) ? diag : __dmul_rn((double)(int64_t)acc[i], p.inv_s2);
        __syncthreads();                                  // every counter is read before the next tile clears it
    }
}

// ---- inverse ----------------------------------------------------------------------------------------------------------------
__global__ void k_inv_init(double* Y, int64_t n, int32_t* status) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) status[0] = INV_NONE;
    if (e < n * n) Y[e] = (e / n == e % n) ? 1.0 : 0.0;
}

// pivot of column j: one workgroup of 1024 threads; a deterministic (|a| desc, row asc) reduction, NaN ranks as +inf
__global__ __launch_bounds__(1024) void k_lu_pivot(double* A, int64_t lda, int64_t n, int64_t j, double* Y, int64_t ldy,
                                                   int32_t* ipiv, int32_t* status) {
    __shared__ double s_v[16];
    __shared__ int s_r[16];
    __shared__ int s_p;
    __shared__ double s_piv;
    if (*status != INV_NONE) return;                      // an earlier column was singular (uniform)
    const int tid = threadIdx.x;
    double bv = -1.0;
    int br = (int)n;
    for (int64_t r = j + tid; r < n; r += 1024) {         // rows ascending per thread: the first maximum stays
        const double a = A[r * lda + j];
        const double v = a != a ? (double)INFINITY : fabs(a);
        if (v > bv) {
            bv = v;
            br = (int)r;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int orr = __shfl_xor(br, o);
        if (ov > bv || (ov == bv && orr < br)) {
            bv = ov;
            br = orr;
        }
    }
    if ((tid & 63) == 0) {
        s_v[tid >> 6] = bv;
        s_r[tid >> 6] = br;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (s_v[w] > bv || (s_v[w] == bv && s_r[w] < br)) {
                bv = s_v[w];
                br = s_r[w];
            }
        const double piv = A[(int64_t)br * lda + j];
        s_p = br;
        s_piv = piv;
        ipiv[j] = br;
        if (piv == 0.0 || piv != piv) atomicMin(status, (int32_t)j);
    }
    __syncthreads();
    const int64_t p = s_p;
    const double piv = s_piv;
    if (piv == 0.0 || piv != piv) return;                 // uniform
    if (p != j) {                                         // full rows: the L columns, the panel, the trailing part, the rhs
        for (int64_t c = tid; c < n; c += 1024) {
            const double a = A[j * lda + c];
            A[j * lda + c] = A[p * lda + c];
            A[p * lda + c] = a;
            if (Y != nullptr) {
                const double y = Y[j * ldy + c];
                Y[j * ldy + c] = Y[p * ldy + c];
                Y[p * ldy + c] = y;
            }
        }
        __syncthreads();
    }
    for (int64_t r = j + 1 + tid; r < n; r += 1024) A[r * lda + j] = __ddiv_rn(A[r * lda + j], piv);
}

// rank-1 update of the panel columns (j, kend) on the rows below j; 4 rows x 64 columns per workgroup
__global__ __launch_bounds__(256) void k_lu_panel(double* A, int64_t lda, int64_t n, int64_t j, int64_t kend,
                                                  const int32_t* status) {
    if (*status != INV_NONE) return;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t i = j + 1 + (int64_t)blockIdx.x * 4 + ty;
    const int64_t c = j + 1 + tx;
    if (i >= n || c >= kend) return;
    A[i * lda + c] = __fma_rn(-A[i * lda + j], A[j * lda + c], A[i * lda + c]);
}

// M[0:nb, c] <- D^-1 M[0:nb, c] for c in [c0, c1): D = the nb x nb diagonal block, unit lower (forward) or upper (backward);
// one column per lane, its solved entries in LDS, terms in ascending column order of D
template <bool UPPER>
__global__ __launch_bounds__(64) void k_inv_trsm(const double* __restrict__ D, int64_t ldd, int nb, double* M, int64_t ldm,
                                                 int64_t c0, int64_t c1, const int32_t* status) {
    __shared__ double sd[INV_NB][INV_NB];
    __shared__ double sx[INV_NB][64];
    if (*status != INV_NONE) return;
    const int tid = threadIdx.x;
    for (int e = tid; e < nb * nb; e += 64) sd[e / nb][e % nb] = D[(e / nb) * ldd + e % nb];
    __syncthreads();
    const int64_t c = c0 + (int64_t)blockIdx.x * 64 + tid;
    if (c >= c1) return;                                  // no barrier below: each lane reads back only its own column
    for (int s = 0; s < nb; ++s) {
        const int i = UPPER ? nb - 1 - s : s;
        double x = M[i * ldm + c];
        for (int t = UPPER ? i + 1 : 0; t < (UPPER ? nb : i); ++t) x = __fma_rn(-sd[i][t], sx[t][tid], x);
        if (UPPER) x = __ddiv_rn(x, sd[i][i]);
        sx[i][tid] = x;
        M[i * ldm + c] = x;
    }
}

// C[r, c] -= sum_{t < nb} L[r * ldl + t] * R[t * ldr + c] for r in [r0, r1), c in [c0, c1): a 64 x 64 tile per workgroup, wave w
// owns rows 16 w .. 16 w + 15 as four 16 x 16 v_mfma_f64_16x16x4_f64 tiles.  Lane l: A operand (-L)[row l & 15][k l >> 4],
// B operand R[k l >> 4][col l & 15]; C/D col = l & 15, row = (l >> 4) + 4 reg (the f64 map, not the f32 one).  The written rows
// never overlap the rows of R nor the columns of L that the call reads.
__global__ __launch_bounds__(256) void k_inv_update(const double* __restrict__ L, int64_t ldl, const double* __restrict__ R,
                                                    int64_t ldr, double* C, int64_t ldc, int64_t r0, int64_t r1, int64_t c0,
                                                    int64_t c1, int nb, const int32_t* status) {
    __shared__ double sl[INV_NB][INV_TILE];               // sl[t][row] = -L
    __shared__ double sr[INV_NB][INV_TILE];               // sr[t][col] = R
    if (*status != INV_NONE) return;
    const int tid = threadIdx.x;
    const int64_t rb = r0 + (int64_t)blockIdx.y * INV_TILE, cb = c0 + (int64_t)blockIdx.x * INV_TILE;
    for (int e = tid; e < INV_TILE * INV_NB; e += 256) {
        const int row = e / INV_NB, t = e % INV_NB;       // t fastest: L rows are read along their length
        const int64_t r = rb + row;
        sl[t][row] = (r < r1 && t < nb) ? -L[r * ldl + t] : 0.0;
        const int tt = e / INV_TILE, col = e % INV_TILE;
        const int64_t cc = cb + col;
        sr[tt][col] = (cc < c1 && tt < nb) ? R[tt * ldr + cc] : 0.0;
    }
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    el_d4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t r = rb + 16 * w + lk + 4 * g, cc = cb + 16 * s + lr;
            acc[s][g] = (r < r1 && cc < c1) ? C[r * ldc + cc] : 0.0;
        }
    for (int k = 0; k < nb; k += 4) {                     // sl / sr are zero from nb up to INV_NB
        const double a = sl[k + lk][16 * w + lr];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sr[k + lk][16 * s + lr], acc[s], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t r = rb + 16 * w + lk + 4 * g, cc = cb + 16 * s + lr;
            if (r < r1 && cc < c1) C[r * ldc + cc] = acc[s][g];
        }
}

int inv_update(double* L, int64_t ldl, const double* R, int64_t ldr, double* C, int64_t ldc, int64_t r0, int64_t r1, int64_t c0,
               int64_t c1, int nb, const int32_t* status, hipStream_t st) {
    if (r1 <= r0 || c1 <= c0) return 0;
    const dim3 grid((unsigned)((c1 - c0 + INV_TILE - 1) / INV_TILE), (unsigned)((r1 - r0 + INV_TILE - 1) / INV_TILE));
    EL_LAUNCH("k_inv_update", k_inv_update, grid, dim3(256), 0, st, (const double*)L, ldl, R, ldr, C, ldc, r0, r1, c0, c1, nb,
              status);
    EL_CHECK_LAUNCH();
    return 0;
}

template <bool UPPER>
int inv_trsm(const double* D, int64_t ldd, int nb, double* M, int64_t ldm, int64_t c0, int64_t c1, const int32_t* status,
             hipStream_t st) {
    if (c1 <= c0) return 0;
    EL_LAUNCH("k_inv_trsm", k_inv_trsm<UPPER>, dim3((unsigned)((c1 - c0 + 63) / 64)), dim3(64), 0, st, D, ldd, nb, M, ldm, c0, c1,
              status);
    EL_CHECK_LAUNCH();
    return 0;
}

// ---- weights and scores -----------------------------------------------------------------------------------------------------
__global__ void k_ease_diag(const double* __restrict__ P, int64_t ldp, int64_t I, double* __restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < I) d[i] = P[i * ldp + i];
}

// row j per blockIdx.x, 256 columns per blockIdx.y
__global__ __launch_bounds__(256) void k_ease_weights(const double* __restrict__ P, int64_t ldp, int64_t I,
                                                      const double* __restrict__ d, float* __restrict__ B, int64_t ldb) {
    const int64_t j = blockIdx.x, i = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (i >= I) return;
    B[j * ldb + i] = i == j ? 0.0f : __double2float_rn(__ddiv_rn(-P[j * ldp + i], d[i]));
}

// scipy's csr_matvecs on k_row_scores (el_rowscore.h): fp32, one rounded product and one rounded sum per entry
struct EaseScoreOp : RowScoreOp<float> {
    const float* vals;
    __device__ float weight(int64_t e) const { return vals[e]; }
    __device__ void step(float& a, float w, float x) const { a = __fadd_rn(a, __fmul_rn(w, x)); }
};

}  // namespace

extern "C" int el_ease_gram(el_ctx* ctx, void* stream, const int64_t* t_indptr, const int32_t* t_indices, const int32_t* t_vals,
                            const int64_t* r_indptr, const int32_t* r_indices, const int32_t* r_vals, int64_t I, int64_t U,
                            int32_t scale, int64_t max_deg, int32_t max_abs, double l2_norm, double* G, int64_t ldg) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(t_indptr && t_indices && t_vals && r_indptr && r_indices && r_vals && G, "el_ease_gram: null pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && U >= 0 && U < 0x7fffffffLL, "el_ease_gram: bad sizes I=%lld U=%lld", (long long)I,
               (long long)U);
    EL_REQUIRE(ldg >= I, "el_ease_gram: ldg=%lld < I=%lld", (long long)ldg, (long long)I);
    EL_REQUIRE(scale == 1 || scale == 2, "el_ease_gram: scale=%d unsupported (1 or 2)", scale);
    EL_REQUIRE(max_deg >= 0 && max_abs >= 0, "el_ease_gram: bad max_deg / max_abs");
    const double bound = (double)max_deg * (double)max_abs * (double)max_abs;
    EL_REQUIRE(bound < 9.0e15, "el_ease_gram: counts up to %.3g do not fit the exact range", bound);
    EaseGram p;
    p.tp = t_indptr, p.ti = t_indices, p.tv = t_vals;
    p.rp = r_indptr, p.ri = r_indices, p.rv = r_vals;
    p.I = I, p.l2 = l2_norm, p.inv_s2 = scale == 2 ? 0.25 : 1.0;
    p.tile = (int)(I < EASE_GRAM_TILE ? I : EASE_GRAM_TILE);
    p.G = G, p.ldg = ldg;
    hipStream_t st = (hipStream_t)stream;
    if (bound < 2147483647.0) {
        const size_t lds = (size_t)p.tile * sizeof(int);
        EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ease_gram<int>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
        EL_LAUNCH("k_ease_gram", k_ease_gram<int>, dim3((unsigned)I), dim3(EASE_GRAM_THREADS), lds, st, p);
    } else {
        const size_t lds = (size_t)p.tile * sizeof(unsigned long long);
        EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ease_gram<unsigned long long>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        EL_LAUNCH("k_ease_gram", k_ease_gram<unsigned long long>, dim3((unsigned)I), dim3(EASE_GRAM_THREADS), lds, st, p);
    }
    EL_CHECK_LAUNCH();
    return 0;
}

namespace {

// the blocked LU of A; with Y (ld n, the identity on entry) the same row operations turn Y into L^-1 P
int lu_f64(double* A, int64_t lda, int64_t n, double* Y, int32_t* ipiv, int32_t* status, hipStream_t st) {
    const int64_t ldy = n;
    for (int64_t k0 = 0; k0 < n; k0 += INV_NB) {
        const int nb = (int)(n - k0 < INV_NB ? n - k0 : INV_NB);
        const int64_t kend = k0 + nb;
        for (int64_t j = k0; j < kend; ++j) {
            EL_LAUNCH("k_lu_pivot", k_lu_pivot, dim3(1), dim3(1024), 0, st, A, lda, n, j, Y, ldy, ipiv, status);
            EL_CHECK_LAUNCH();
            if (j + 1 < kend && j + 1 < n) {
                EL_LAUNCH("k_lu_panel", k_lu_panel, dim3((unsigned)((n - j - 1 + 3) / 4)), dim3(256), 0, st, A, lda, n, j, kend,
                          (const int32_t*)status);
                EL_CHECK_LAUNCH();
            }
        }
        const double* D = A + k0 * lda + k0;
        if (int rc = inv_trsm<false>(D, lda, nb, A + k0 * lda, lda, kend, n, status, st)) return rc;      // U12 = L11^-1 A12
        if (int rc = inv_update(A + k0, lda, A + k0 * lda, lda, A, lda, kend, n, kend, n, nb, status, st)) return rc;
        if (Y != nullptr) {
            if (int rc = inv_trsm<false>(D, lda, nb, Y + k0 * ldy, ldy, 0, n, status, st)) return rc;     // Y1 = L11^-1 Y1
            if (int rc = inv_update(A + k0, lda, Y + k0 * ldy, ldy, Y, ldy, kend, n, 0, n, nb, status, st)) return rc;
        }
    }
    return 0;
}

__global__ void k_status_init(int32_t* status) {
    if (threadIdx.x == 0) status[0] = INV_NONE;
}

}  // namespace

extern "C" int el_lu_f64(el_ctx* ctx, void* stream, double* A, int64_t lda, int64_t n, int32_t* ipiv, int32_t* status) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(A && ipiv && status, "el_lu_f64: null pointer");
    EL_REQUIRE(n >= 1 && n < 0x7fffffffLL, "el_lu_f64: bad order n=%lld", (long long)n);
    EL_REQUIRE(lda >= n, "el_lu_f64: lda=%lld < n=%lld", (long long)lda, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    EL_LAUNCH("k_status_init", k_status_init, dim3(1), dim3(64), 0, st, status);
    EL_CHECK_LAUNCH();
    return lu_f64(A, lda, n, nullptr, ipiv, status, st);
}

extern "C" size_t el_inv_f64_ws_bytes(int64_t n) {
    if (n <= 0) return 0;
    return el_align256((size_t)n * (size_t)n * sizeof(double));
}

extern "C" int el_inv_f64(el_ctx* ctx, void* stream, double* A, int64_t lda, int64_t n, int32_t* ipiv, int32_t* status, void* ws,
                          size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(A && ipiv && status, "el_inv_f64: null pointer");
    EL_REQUIRE(n >= 1 && n < 0x7fffffffLL && (double)n * (double)n < 4.0e18, "el_inv_f64: bad order n=%lld", (long long)n);
    EL_REQUIRE(lda >= n, "el_inv_f64: lda=%lld < n=%lld", (long long)lda, (long long)n);
    const size_t need = el_inv_f64_ws_bytes(n);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_inv_f64: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    double* Y = (double*)ws;                               // the right-hand sides, n x n, ld n: I, then L^-1 P I, then A^-1
    const int64_t ldy = n;
    EL_LAUNCH("k_inv_init", k_inv_init, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, Y, n, status);
    EL_CHECK_LAUNCH();
    if (int rc = lu_f64(A, lda, n, Y, ipiv, status, st)) return rc;
    // U X = Y by block rows from the bottom: X1 = U11^-1 Y1, then Y0 -= U01 X1
    const int64_t last = ((n - 1) / INV_NB) * INV_NB;
    for (int64_t k0 = last; k0 >= 0; k0 -= INV_NB) {
        const int nb = (int)(n - k0 < INV_NB ? n - k0 : INV_NB);
        if (int rc = inv_trsm<true>(A + k0 * lda + k0, lda, nb, Y + k0 * ldy, ldy, 0, n, status, st)) return rc;
        if (int rc = inv_update(A + k0, lda, Y + k0 * ldy, ldy, Y, ldy, 0, k0, 0, n, nb, status, st)) return rc;
    }
    EL_CHECK_HIP(hipMemcpy2DAsync(A, (size_t)lda * sizeof(double), Y, (size_t)ldy * sizeof(double), (size_t)n * sizeof(double),
                                  (size_t)n, hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" size_t el_ease_weights_ws_bytes(int64_t I) {
    if (I <= 0) return 0;
    return el_align256((size_t)I * sizeof(double));
}

extern "C" int el_ease_weights(el_ctx* ctx, void* stream, const double* P, int64_t ldp, int64_t I, float* B, int64_t ldb, void* ws,
                               size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(P && B, "el_ease_weights: null pointer");
    EL_REQUIRE(I >= 1 && I < 0x7fffffffLL && (I + 255) / 256 < 65536, "el_ease_weights: bad size I=%lld", (long long)I);
    EL_REQUIRE(ldp >= I && ldb >= I, "el_ease_weights: leading dimensions below I");
    const size_t need = el_ease_weights_ws_bytes(I);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_ease_weights: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    double* d = (double*)ws;
    EL_LAUNCH("k_ease_diag", k_ease_diag, dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st, P, ldp, I, d);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_ease_weights", k_ease_weights, dim3((unsigned)I, (unsigned)((I + 255) / 256)), dim3(256), 0, st, P, ldp, I,
              (const double*)d, B, ldb);
    EL_CHECK_LAUNCH();
    return 0;
}

extern "C" int el_csr_dense_scores(el_ctx* ctx, void* stream, const int64_t* indptr, const int32_t* indices, const float* vals,
                                   int64_t u_start, int64_t u_stop, const float* B, int64_t ldb, int64_t I, float* S, int64_t lds) {
    return el_row_scores("el_csr_dense_scores", "k_csr_dense_scores", ctx, stream, indptr && indices && vals && B && S, indptr,
                         indices, u_start, u_stop, EaseScoreOp{{B, ldb}, vals}, I, S, lds);
}
