// PureSVD (Cremonesi et al. 2010): the tall-skinny fp64 layer under sklearn's randomized_svd.
//
// Replaces the device-side work of PureSVDModel.train_step (pure_svd_model.py:36-43):
//   el_spmm_csr_f64   Y = A X, CSR x dense fp64, stored order inside a row, long rows in pieces          (A @ Q, A.T @ Q)
//   el_gram_f64       G = Y^T Y on v_mfma_f64_16x16x4_f64, fixed slots of rows, symmetric bit for bit
//   el_psvd_orth      Cholesky-QR twice: Gram, Cholesky, W = L^-T, Y <- Y W                               (the LU / QR normalisers)
//   el_psvd_project   T = (Y W) diag(s) on the same matrix instruction, fp64 and / or float output        (Q U^, Z U^)
//   el_psvd_signs     sign of every column's entry of largest magnitude, first row among equals         (svd_flip)
// The R x R eigenproblem stays on the host.  Every sum has one owner and a fixed order and nothing
// floating-point is added with atomics: the same input gives the same bits on every run.
#include "el_common.h"

#define PSVD_NONE 0x7fffffff
#define PSVD_GRAM_SLOT_ROWS 1024     // rows per slot of the Gram sum while the slots stay below PSVD_GRAM_MAX_SLOTS
#define PSVD_GRAM_MAX_SLOTS 256
#define PSVD_KC 32                   // rows of Y staged per step of k_gram_f64
#define PSVD_LDS_ROW 80              // doubles per staged row: 64 + 16, so that the two k of a half wave use disjoint banks
#define PSVD_CHOL_LDS_R 96           // the Cholesky works in LDS up to this order (2 R^2 doubles <= 147 456 bytes)
#define PSVD_SIGN_ROWS 512           // rows per workgroup of k_psvd_colmax

typedef double el_d4 __attribute__((ext_vector_type(4)));
typedef double el_d2 __attribute__((ext_vector_type(2)));

namespace {

// ---- CSR x dense --------------------------------------------------------------------------------------------------------------
struct Spmm {
    const int64_t* indptr;
    const int32_t* indices;
    const float* vals;
    int64_t n_rows, n_cols;
    const double* X;
    int64_t ldx;
    int R;
    double* Y;
    int64_t ldy;
    const int32_t* long_rows;
    const int64_t* long_first;
    int64_t n_long, n_pieces, piece_len;
    double* part;                    // [n_pieces, R]
    int32_t* status;                 // [0] plan, [1] column index
};

__global__ void k_psvd_status_init(int32_t* status, int n) {
    if ((int)threadIdx.x < n) status[threadIdx.x] = PSVD_NONE;
}

// the plan's entry of long row `row` (len entries), -1 when the plan does not describe it
__device__ __forceinline__ int64_t spmm_plan_entry(const Spmm& p, int64_t row, int64_t len) {
    int64_t lo = 0, hi = p.n_long;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)p.long_rows[mid] < row)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= p.n_long || (int64_t)p.long_rows[lo] != row) return -1;
    const int64_t f0 = p.long_first[lo], f1 = p.long_first[lo + 1];
    if (f0 < 0 || f1 > p.n_pieces || f1 - f0 != (len + p.piece_len - 1) / p.piece_len) return -1;
    return lo;
}

// One group of G lanes per row (PIECES: per piece of a long row); a lane owns the column pairs 2 g + 2 G s, s < NP, read with one
// 16-byte load each (VEC: X 16-byte aligned, ldx even).  Four entries' gathers are in flight before their terms are added in
// stored order.
template <int G, int NP, bool VEC, bool PIECES>
__global__ __launch_bounds__(256) void k_spmm_f64(Spmm p) {
    const int tid = threadIdx.x, g = tid & (G - 1);
    const int64_t item = ((int64_t)blockIdx.x * 256 + tid) / G;
    const int R = p.R;
    int64_t row, e0, e1;
    double* out;
    if (PIECES) {
        if (item >= p.n_pieces) return;
        int64_t lo = 0, hi = p.n_long;                    // the last entry whose first slot is <= item
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (p.long_first[mid] <= item)
                lo = mid;
            else
                hi = mid;
        }
        out = p.part + item * R;
        row = p.long_rows[lo];
        e0 = e1 = 0;
        if (row >= 0 && row < p.n_rows && p.long_first[lo] <= item && item < p.long_first[lo + 1]) {
            const int64_t r0 = p.indptr[row], r1 = p.indptr[row + 1];
            if (spmm_plan_entry(p, row, r1 - r0) == lo) {     // a slot the plan gets wrong stays zero; the row reports it
                e0 = r0 + (item - p.long_first[lo]) * p.piece_len;
                e1 = e0 + p.piece_len < r1 ? e0 + p.piece_len : r1;
            }
        }
    } else {
        if (item >= p.n_rows) return;
        row = item;
        e0 = p.indptr[row], e1 = p.indptr[row + 1];
        out = p.Y + row * p.ldy;
        if (e1 - e0 > p.piece_len) {                      // summed by its pieces; k_spmm_combine writes the row
            if (g == 0 && spmm_plan_entry(p, row, e1 - e0) < 0) atomicMin(&p.status[0], (int32_t)row);
            return;
        }
    }
    double acc[NP][2];
#pragma unroll
    for (int s = 0; s < NP; ++s) acc[s][0] = acc[s][1] = 0.0;
    bool bad = false;
    for (int64_t e = e0; e < e1; e += 4) {
        int32_t ci[4];
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t ee = e + q < e1 ? e + q : e;
            ci[q] = p.indices[ee];
            v[q] = p.vals != nullptr ? (double)p.vals[ee] : 1.0;
            if ((uint32_t)ci[q] >= (uint64_t)p.n_cols) {
                bad = true;
                ci[q] = 0;
            }
        }
        double x[4][NP][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double* xr = p.X + (int64_t)ci[q] * p.ldx;
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                const int c = 2 * g + 2 * G * s;
                if (VEC && c + 1 < R) {
                    const el_d2 t = *reinterpret_cast<const el_d2*>(xr + c);
                    x[q][s][0] = t.x, x[q][s][1] = t.y;
                } else {
                    x[q][s][0] = c < R ? xr[c] : 0.0;
                    x[q][s][1] = c + 1 < R ? xr[c + 1] : 0.0;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (e + q < e1) {
#pragma unroll
                for (int s = 0; s < NP; ++s) {
                    acc[s][0] = __dadd_rn(acc[s][0], __dmul_rn(v[q], x[q][s][0]));
                    acc[s][1] = __dadd_rn(acc[s][1], __dmul_rn(v[q], x[q][s][1]));
                }
            }
        }
    }
    if (bad && g == 0) atomicMin(&p.status[1], (int32_t)row);
#pragma unroll
    for (int s = 0; s < NP; ++s) {
        const int c = 2 * g + 2 * G * s;
        if (c < R) out[c] = acc[s][0];
        if (c + 1 < R) out[c + 1] = acc[s][1];
    }
}

// one workgroup per long row: its slots added in piece order from +0
__global__ __launch_bounds__(256) void k_spmm_combine(Spmm p) {
    const int64_t j = blockIdx.x;
    const int64_t row = p.long_rows[j];
    if (row < 0 || row >= p.n_rows) return;
    if (spmm_plan_entry(p, row, p.indptr[row + 1] - p.indptr[row]) != j) return;
    const int64_t f0 = p.long_first[j], f1 = p.long_first[j + 1];
    for (int c = threadIdx.x; c < p.R; c += 256) {
        double acc = 0.0;
        for (int64_t s = f0; s < f1; ++s) acc = __dadd_rn(acc, p.part[s * p.R + c]);
        p.Y[row * p.ldy + c] = acc;
    }
}

template <int G, int NP, bool VEC>
int spmm_launch(const Spmm& p, hipStream_t st) {
    const int64_t per = 256 / G;
    EL_LAUNCH("k_spmm_f64", (k_spmm_f64<G, NP, VEC, false>), dim3((unsigned)((p.n_rows + per - 1) / per)), dim3(256), 0, st, p);
    EL_CHECK_LAUNCH();
    if (p.n_long > 0 && p.n_pieces > 0) {
        EL_LAUNCH("k_spmm_f64_pieces", (k_spmm_f64<G, NP, VEC, true>), dim3((unsigned)((p.n_pieces + per - 1) / per)), dim3(256), 0,
                  st, p);
        EL_CHECK_LAUNCH();
        EL_LAUNCH("k_spmm_combine", k_spmm_combine, dim3((unsigned)p.n_long), dim3(256), 0, st, p);
        EL_CHECK_LAUNCH();
    }
    return 0;
}

template <bool VEC>
int spmm_dispatch(const Spmm& p, hipStream_t st) {
    if (p.R > 128) return spmm_launch<64, 2, VEC>(p, st);
    if (p.R > 64) return spmm_launch<64, 1, VEC>(p, st);
    if (p.R > 32) return spmm_launch<32, 1, VEC>(p, st);
    if (p.R > 16) return spmm_launch<16, 1, VEC>(p, st);
    return spmm_launch<8, 1, VEC>(p, st);
}

// ---- Gram ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int64_t gram_slots(int64_t n) {
    const int64_t s = (n + PSVD_GRAM_SLOT_ROWS - 1) / PSVD_GRAM_SLOT_ROWS;
    return s < 1 ? 1 : (s > PSVD_GRAM_MAX_SLOTS ? PSVD_GRAM_MAX_SLOTS : s);
}
__host__ __device__ inline int64_t gram_slot_rows(int64_t n) {
    const int64_t s = gram_slots(n);
    return ((n + s - 1) / s + 3) / 4 * 4;
}

// part[slot][i][j] for one 64 x 64 block (bi <= bj) of G and one slot of rows: wave w owns rows 16 w .. 16 w + 15 of the block as
// four 16 x 16 tiles.  Lane l: A operand Y[k = l >> 4][column i = l & 15], B operand Y[k][column j]; C/D col = l & 15,
// row = (l >> 4) + 4 reg (the f64 map).
__global__ __launch_bounds__(256) void k_gram_f64(const double* __restrict__ Y, int64_t ldy, int64_t n, int R, int64_t slot_rows,
                                                  double* __restrict__ part, int nb, const int32_t* status) {
    __shared__ double sa[PSVD_KC][PSVD_LDS_ROW];
    __shared__ double sb[PSVD_KC][PSVD_LDS_ROW];
    if (status != nullptr && *status != PSVD_NONE) return;
    const int tid = threadIdx.x;
    int bi = 0, rem = blockIdx.x;
    while (rem >= nb - bi) {
        rem -= nb - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const int64_t r_lo = (int64_t)blockIdx.y * slot_rows;
    const int64_t r_hi = r_lo + slot_rows < n ? r_lo + slot_rows : n;
    const int w = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    el_d4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = (el_d4){0.0, 0.0, 0.0, 0.0};
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += PSVD_KC) {
        for (int e = tid; e < PSVD_KC * 64; e += 256) {
            const int t = e >> 6, c = e & 63;
            const int64_t r = r0 + t;
            const int ca = bi * 64 + c, cb = bj * 64 + c;
            sa[t][c] = (r < r_hi && ca < R) ? Y[r * ldy + ca] : 0.0;
            sb[t][c] = (r < r_hi && cb < R) ? Y[r * ldy + cb] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PSVD_KC; k += 4) {
            const double a = sa[k + lk][16 * w + lr];
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sb[k + lk][16 * s + lr], acc[s], 0, 0, 0);
        }
        __syncthreads();
    }
    double* out = part + (int64_t)blockIdx.y * R * R;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = bi * 64 + 16 * w + lk + 4 * g, j = bj * 64 + 16 * s + lr;
            if (i < R && j < R) out[(int64_t)i * R + j] = acc[s][g];
        }
}

// G[i][j] = G[j][i] = the slots of part[.][i][j], i <= j, added in slot order from +0
__global__ __launch_bounds__(256) void k_gram_reduce(const double* __restrict__ part, int64_t n_slots, int R, double* __restrict__ G,
                                                     int64_t ldg, const int32_t* status) {
    if (status != nullptr && *status != PSVD_NONE) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = e / R, j = e % R;
    if (i >= R || j < i) return;
    double acc = 0.0;
    for (int64_t s = 0; s < n_slots; ++s) acc = __dadd_rn(acc, part[s * R * R + i * R + j]);
    G[i * ldg + j] = acc;
    G[j * ldg + i] = acc;
}

int gram_run(const double* Y, int64_t ldy, int64_t n, int R, double* G, int64_t ldg, double* part, const int32_t* status,
             hipStream_t st) {
    const int nb = (R + 63) / 64;
    const int64_t slots = gram_slots(n);
    EL_LAUNCH("k_gram_f64", k_gram_f64, dim3((unsigned)(nb * (nb + 1) / 2), (unsigned)slots), dim3(256), 0, st, Y, ldy, n, R,
              gram_slot_rows(n), part, nb, status);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_gram_reduce", k_gram_reduce, dim3((unsigned)(((int64_t)R * R + 255) / 256)), dim3(256), 0, st, (const double*)part,
              slots, R, G, ldg, status);
    EL_CHECK_LAUNCH();
    return 0;
}

// ---- Cholesky and W = L^-T (one workgroup) ------------------------------------------------------------------------------------
// G (ld R) -> L in its lower triangle by the right-looking form: column j's pivot, its division, the rank-1 update of the
// trailing lower triangle; then column c of L^-1 by forward substitution, one thread per column, terms in ascending order; then
// W[k][j] = L^-1[j][k].  Up to PSVD_CHOL_LDS_R the two matrices live in LDS (lds = 1).
__global__ __launch_bounds__(1024) void k_psvd_chol(double* Gg, int R, double rel, double* W, double* Xg, int32_t* status, int lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double s_diag[EL_PSVD_MAX_R];
    __shared__ double s_d;
    __shared__ int s_bad;
    if (*status != PSVD_NONE) return;                     // an earlier pass refused a pivot (uniform)
    const int tid = threadIdx.x;
    double* G = Gg;
    double* X = Xg;
    if (lds) {
        G = reinterpret_cast<double*>(smem);
        X = G + R * R;
        for (int e = tid; e < R * R; e += 1024) G[e] = Gg[e];
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (tid < R) s_diag[tid] = G[tid * R + tid];
    __syncthreads();
    for (int j = 0; j < R; ++j) {
        if (tid == 0) {
            const double d = G[j * R + j];
            if (!(d > 0.0) || !(d > __dmul_rn(rel, s_diag[j]))) {
                s_bad = 1;
                atomicMin(status, (int32_t)j);
            } else {
                s_d = __dsqrt_rn(d);
                G[j * R + j] = s_d;
            }
        }
        __syncthreads();
        if (s_bad) return;                                // uniform
        const double d = s_d;
        for (int i = j + 1 + tid; i < R; i += 1024) G[i * R + j] = __ddiv_rn(G[i * R + j], d);
        __syncthreads();
        const int m = R - j - 1;
        for (int e = tid; e < m * m; e += 1024) {
            const int ii = e / m, kk = e % m;
            if (kk <= ii) {
                const int i = j + 1 + ii, k = j + 1 + kk;
                G[i * R + k] = __fma_rn(-G[i * R + j], G[k * R + j], G[i * R + k]);
            }
        }
        __syncthreads();
    }
    if (tid < R) {
        const int c = tid;
        for (int i = c; i < R; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s = __fma_rn(-G[i * R + k], X[k * R + c], s);
            X[i * R + c] = __ddiv_rn(s, G[i * R + i]);
        }
    }
    __syncthreads();
    for (int e = tid; e < R * R; e += 1024) {
        const int k = e / R, j = e % R;
        W[e] = j >= k ? X[j * R + k] : 0.0;
    }
}

// ---- T = (Y W) diag(s) ----------------------------------------------------------------------------------------------------------
// 64 rows per workgroup, 16 per wave, every column tile of the output in the wave's accumulators: a wave reads its rows of Y whole
// (the A operand straight from memory, lane l: Y[row l & 15][k = l >> 4]) before it writes them, so T64 may be Y.  W is staged 16
// rows at a time.
template <int NT>
__global__ __launch_bounds__(256) void k_psvd_project(const double* Y, int64_t ldy, int64_t n, int R, const double* __restrict__ W,
                                                      int64_t ldw, int k, const double* __restrict__ scale, double* T64,
                                                      int64_t ldt64, float* T32, int64_t ldt32, const int32_t* status) {
    constexpr int LW = NT * 16 + ((NT & 1) ? 0 : 16);     // an odd multiple of 16 doubles: the two k of a half wave on disjoint banks
    __shared__ double sw[16][LW];
    if (status != nullptr && *status != PSVD_NONE) return;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int64_t rb = (int64_t)blockIdx.x * 64 + 16 * w;
    el_d4 acc[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc[s] = (el_d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < R; k0 += 16) {
        for (int e = tid; e < 16 * NT * 16; e += 256) {
            const int t = e / (NT * 16), c = e % (NT * 16);
            sw[t][c] = (k0 + t < R && c < k) ? W[(int64_t)(k0 + t) * ldw + c] : 0.0;
        }
        __syncthreads();
        double a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = rb + lr;
            const int kk = k0 + 4 * q + lk;
            a[q] = (r < n && kk < R) ? Y[r * ldy + kk] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int s = 0; s < NT; ++s)
                acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], sw[4 * q + lk][16 * s + lr], acc[s], 0, 0, 0);
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < NT; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t r = rb + lk + 4 * g;
            const int c = 16 * s + lr;
            if (r < n && c < k) {
                const double v = scale != nullptr ? __dmul_rn(acc[s][g], scale[c]) : acc[s][g];
                if (T64 != nullptr) T64[r * ldt64 + c] = v;
                if (T32 != nullptr) T32[r * ldt32 + c] = __double2float_rn(v);
            }
        }
}

int project_run(const double* Y, int64_t ldy, int64_t n, int R, const double* W, int64_t ldw, int k, const double* scale, double* T64,
                int64_t ldt64, float* T32, int64_t ldt32, const int32_t* status, hipStream_t st) {
    const dim3 grid((unsigned)((n + 63) / 64));
    const int nt = (k + 15) / 16;
#define PSVD_PROJECT(NT)                                                                                                       \
    EL_LAUNCH("k_psvd_project", k_psvd_project<NT>, grid, dim3(256), 0, st, Y, ldy, n, R, W, ldw, k, scale, T64, ldt64, T32, ldt32, \
              status)
    if (nt <= 1)
        PSVD_PROJECT(1);
    else if (nt <= 2)
        PSVD_PROJECT(2);
    else if (nt <= 3)
        PSVD_PROJECT(3);
    else if (nt <= 4)
        PSVD_PROJECT(4);
    else if (nt <= 5)
        PSVD_PROJECT(5);
    else if (nt <= 7)
        PSVD_PROJECT(7);
    else if (nt <= 9)
        PSVD_PROJECT(9);
    else if (nt <= 12)
        PSVD_PROJECT(12);
    else
        PSVD_PROJECT(16);
#undef PSVD_PROJECT
    EL_CHECK_LAUNCH();
    return 0;
}

// ---- svd_flip ---------------------------------------------------------------------------------------------------------------------
// thread c walks column c over PSVD_SIGN_ROWS rows (the threads of a workgroup read consecutive columns of a row): the entry of
// largest magnitude, the first one among equals
__global__ __launch_bounds__(256) void k_psvd_colmax(const double* __restrict__ T, int64_t ldt, int64_t n, int k,
                                                     double* __restrict__ part) {
    const int c = threadIdx.x;
    if (c >= k) return;
    const int64_t r0 = (int64_t)blockIdx.x * PSVD_SIGN_ROWS;
    const int64_t r1 = r0 + PSVD_SIGN_ROWS < n ? r0 + PSVD_SIGN_ROWS : n;
    double best = 0.0, mag = -1.0;
    for (int64_t r = r0; r < r1; ++r) {
        const double x = T[r * ldt + c];
        if (fabs(x) > mag) {
            mag = fabs(x);
            best = x;
        }
    }
    part[(int64_t)blockIdx.x * k + c] = best;
}

__global__ __launch_bounds__(256) void k_psvd_signs(const double* __restrict__ part, int64_t n_blocks, int k,
                                                    double* __restrict__ signs) {
    const int c = threadIdx.x;
    if (c >= k) return;
    double best = 0.0, mag = -1.0;
    for (int64_t b = 0; b < n_blocks; ++b) {
        const double x = part[b * k + c];
        if (fabs(x) > mag) {
            mag = fabs(x);
            best = x;
        }
    }
    signs[c] = best < 0.0 ? -1.0 : 1.0;
}

size_t gram_part_bytes(int64_t n, int R) { return el_align256((size_t)gram_slots(n) * (size_t)R * (size_t)R * sizeof(double)); }

struct OrthWs {
    double* part;          // the Gram partial sums of gram_run
    double *G, *X, *W;     // [R, R] each
};

size_t orth_carve(int64_t n, int R, void* base, OrthWs* w) {
    ElCarve c{(char*)base};
    w->part = (double*)c.take<char>(gram_part_bytes(n, R));
    w->G = c.take<double>((size_t)R * R);
    w->X = c.take<double>((size_t)R * R);
    w->W = c.take<double>((size_t)R * R);
    return c.off;
}

}  // namespace

extern "C" size_t el_spmm_csr_f64_ws_bytes(int64_t n_pieces, int32_t R) {
    if (n_pieces <= 0 || R <= 0) return 0;
    return el_align256((size_t)n_pieces * (size_t)R * sizeof(double));
}

extern "C" int el_spmm_csr_f64(el_ctx* ctx, void* stream, const int64_t* indptr, const int32_t* indices, const float* vals,
                               int64_t n_rows, int64_t n_cols, const double* X, int64_t ldx, int32_t R, double* Y, int64_t ldy,
                               const int32_t* long_rows, const int64_t* long_first, int64_t n_long, int64_t n_pieces,
                               int64_t piece_len, int32_t* status, void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(indptr && indices && X && Y && status, "el_spmm_csr_f64: null pointer");
    EL_REQUIRE(n_rows >= 0 && n_rows < 0x7fffffffLL && n_cols >= 1 && n_cols < 0x7fffffffLL, "el_spmm_csr_f64: bad shape %lld x %lld",
               (long long)n_rows, (long long)n_cols);
    EL_REQUIRE(R >= 1 && R <= EL_PSVD_MAX_R, "el_spmm_csr_f64: R=%d unsupported (1 .. %d)", R, EL_PSVD_MAX_R);
    EL_REQUIRE(ldx >= R && ldy >= R, "el_spmm_csr_f64: leading dimensions below R");
    EL_REQUIRE(piece_len >= 1 && n_long >= 0 && n_pieces >= 0 && n_long <= n_rows, "el_spmm_csr_f64: bad plan sizes");
    EL_REQUIRE(n_long == 0 || (long_rows && long_first), "el_spmm_csr_f64: the plan's arrays are missing");
    const size_t need = n_long > 0 ? el_spmm_csr_f64_ws_bytes(n_pieces, R) : 0;
    EL_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need), "el_spmm_csr_f64: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    EL_LAUNCH("k_psvd_status_init", k_psvd_status_init, dim3(1), dim3(64), 0, st, status, 2);
    EL_CHECK_LAUNCH();
    if (n_rows == 0) return 0;
    Spmm p;
    p.indptr = indptr, p.indices = indices, p.vals = vals;
    p.n_rows = n_rows, p.n_cols = n_cols;
    p.X = X, p.ldx = ldx, p.R = R, p.Y = Y, p.ldy = ldy;
    p.long_rows = long_rows, p.long_first = long_first, p.n_long = n_long, p.n_pieces = n_pieces, p.piece_len = piece_len;
    p.part = (double*)ws, p.status = status;
    const bool vec = (ldx % 2 == 0) && ((uintptr_t)X % 16 == 0);
    return vec ? spmm_dispatch<true>(p, st) : spmm_dispatch<false>(p, st);
}

extern "C" int64_t el_gram_f64_slots(int64_t n) { return gram_slots(n); }

extern "C" size_t el_gram_f64_ws_bytes(int64_t n, int32_t R) {
    if (n < 0 || R <= 0) return 0;
    return gram_part_bytes(n, R);
}

extern "C" int el_gram_f64(el_ctx* ctx, void* stream, const double* Y, int64_t ldy, int64_t n, int32_t R, double* G, int64_t ldg,
                           void* ws, size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(Y && G, "el_gram_f64: null pointer");
    EL_REQUIRE(n >= 0 && n < 0x7fffffffLL, "el_gram_f64: bad row count %lld", (long long)n);
    EL_REQUIRE(R >= 1 && R <= EL_PSVD_MAX_R, "el_gram_f64: R=%d unsupported (1 .. %d)", R, EL_PSVD_MAX_R);
    EL_REQUIRE(ldy >= R && ldg >= R, "el_gram_f64: leading dimensions below R");
    const size_t need = el_gram_f64_ws_bytes(n, R);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_gram_f64: workspace too small (need %zu bytes)", need);
    return gram_run(Y, ldy, n, R, G, ldg, (double*)ws, nullptr, (hipStream_t)stream);
}

extern "C" size_t el_psvd_orth_ws_bytes(int64_t n, int32_t R) {
    if (n < 0 || R <= 0) return 0;
    OrthWs w;
    return orth_carve(n, R, nullptr, &w);
}

extern "C" int el_psvd_orth(el_ctx* ctx, void* stream, double* Y, int64_t ldy, int64_t n, int32_t R, int32_t* status, void* ws,
                            size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(Y && status, "el_psvd_orth: null pointer");
    EL_REQUIRE(n >= 1 && n < 0x7fffffffLL, "el_psvd_orth: bad row count %lld", (long long)n);
    EL_REQUIRE(R >= 1 && R <= EL_PSVD_MAX_R, "el_psvd_orth: R=%d unsupported (1 .. %d)", R, EL_PSVD_MAX_R);
    EL_REQUIRE(ldy >= R, "el_psvd_orth: ldy=%lld < R=%d", (long long)ldy, R);
    OrthWs w;
    const size_t need = orth_carve(n, R, ws, &w);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_psvd_orth: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    const double rel = 8.0 * ((double)n * R + (double)R * (R + 1)) * 1.1102230246251565e-16;
    const int lds = R <= PSVD_CHOL_LDS_R;
    const size_t dyn = lds ? 2 * (size_t)R * R * sizeof(double) : 0;
    if (lds)
        EL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_psvd_chol), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)dyn));
    EL_LAUNCH("k_psvd_status_init", k_psvd_status_init, dim3(1), dim3(64), 0, st, status, 1);
    EL_CHECK_LAUNCH();
    for (int pass = 0; pass < 2; ++pass) {
        if (int rc = gram_run(Y, ldy, n, R, w.G, R, w.part, status, st)) return rc;
        EL_LAUNCH("k_psvd_chol", k_psvd_chol, dim3(1), dim3(1024), dyn, st, w.G, (int)R, rel, w.W, w.X, status, lds);
        EL_CHECK_LAUNCH();
        if (int rc = project_run(Y, ldy, n, R, w.W, R, R, nullptr, Y, ldy, nullptr, 0, status, st)) return rc;
    }
    return 0;
}

extern "C" int el_psvd_project(el_ctx* ctx, void* stream, const double* Y, int64_t ldy, int64_t n, int32_t R, const double* W,
                               int64_t ldw, int32_t k, const double* col_scale, double* T64, int64_t ldt64, float* T32,
                               int64_t ldt32) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(Y && W && (T64 || T32), "el_psvd_project: null pointer");
    EL_REQUIRE(n >= 0 && n < 0x7fffffffLL, "el_psvd_project: bad row count %lld", (long long)n);
    EL_REQUIRE(R >= 1 && R <= EL_PSVD_MAX_R && k >= 1 && k <= R, "el_psvd_project: R=%d, k=%d unsupported (1 <= k <= R <= %d)", R, k,
               EL_PSVD_MAX_R);
    EL_REQUIRE(ldy >= R && ldw >= k && (!T64 || ldt64 >= k) && (!T32 || ldt32 >= k), "el_psvd_project: leading dimensions too small");
    EL_REQUIRE((const double*)T64 != Y || (k == R && ldt64 == ldy), "el_psvd_project: in place needs k == R and ldt64 == ldy");
    if (n == 0) return 0;
    return project_run(Y, ldy, n, R, W, ldw, k, col_scale, T64, ldt64, T32, ldt32, nullptr, (hipStream_t)stream);
}

extern "C" size_t el_psvd_signs_ws_bytes(int64_t n, int32_t k) {
    if (n <= 0 || k <= 0) return 0;
    return el_align256((size_t)((n + PSVD_SIGN_ROWS - 1) / PSVD_SIGN_ROWS) * (size_t)k * sizeof(double));
}

extern "C" int el_psvd_signs(el_ctx* ctx, void* stream, const double* T, int64_t ldt, int64_t n, int32_t k, double* signs, void* ws,
                             size_t ws_bytes) {
    if (int rc = el_bind(ctx)) return rc;
    EL_REQUIRE(T && signs, "el_psvd_signs: null pointer");
    EL_REQUIRE(n >= 1 && n < 0x7fffffffLL, "el_psvd_signs: bad row count %lld", (long long)n);
    EL_REQUIRE(k >= 1 && k <= EL_PSVD_MAX_R && ldt >= k, "el_psvd_signs: k=%d, ldt=%lld unsupported", k, (long long)ldt);
    const size_t need = el_psvd_signs_ws_bytes(n, k);
    EL_REQUIRE(ws != nullptr && ws_bytes >= need, "el_psvd_signs: workspace too small (need %zu bytes)", need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (n + PSVD_SIGN_ROWS - 1) / PSVD_SIGN_ROWS;
    EL_LAUNCH("k_psvd_colmax", k_psvd_colmax, dim3((unsigned)nb), dim3(256), 0, st, T, ldt, n, (int)k, (double*)ws);
    EL_CHECK_LAUNCH();
    EL_LAUNCH("k_psvd_signs", k_psvd_signs, dim3(1), dim3(256), 0, st, (const double*)ws, nb, (int)k, signs);
    EL_CHECK_LAUNCH();
    return 0;
}
