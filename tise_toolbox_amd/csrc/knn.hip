// k-nearest-neighbour manifold passes of improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et
// al. 2020) on fp32 feature rows that stay on the device.  Squared distances come from the expansion
//     d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)
// in fp64 (rows_tile.h's rows_d2): a.b from the gathered-row fp64 MFMA tile (every fp32 x fp32 product is exact in fp64), the norms
// from rows_norm2_kernel (exact squares, fixed order; NaN for a row that holds a NaN or an infinity, and the clamp keeps a NaN --
// rows_tile.h: such a row is nobody's neighbour, lies in no ball, and its own r2 is NaN).  No N x N matrix is written: a
// workgroup turns the accumulators of one 64 x 64 tile into d2 and consumes them on the spot.
//
// One value per pair, whatever the pass.  a.b is accumulated over k in the tile's fixed order, and a step fma(a_k, b_k, acc) does
// not care which operand is which; |a|^2 + |b|^2 commutes; so d2(x_i, x_j) of the within-set pass, d2(x_j, x_i) of the same pass
// and d2 of the same two rows in the cross pass are the same bits.  The strict `<` of the counts therefore resolves the exact
// ties of a set compared with itself the same way in every run.
//
// Grid of both tile kernels: (row tiles of 64) x (S column splits); workgroup (tm, s) walks column tiles [s T / S, (s + 1) T / S).
//
// Kernels
//   rows_norm2_kernel      (rows_tile.h) one wave per row; bound: HBM (reads the rows once)
//   knn_radius2_kernel     within-set pass; after each tile's K loop the 64 x 64 d2 values are staged in the slab buffer (free after
//                          the K loop's last barrier) and thread t < 64 folds row t's 64 values into its running k-smallest list;
//                          k candidates per (row, split) at the end.  bound: fp64 MFMA for d in the thousands (64 * 64 * 2 * d flop
//                          per tile against 2 * 64 * d * 4 bytes fetched, mostly from L2); the scan is 64 LDS reads per row and tile
//   knn_merge_kernel       one thread per row: the k-th smallest of its S * k candidates.  bound: latency
//   prdc_counts_kernel     cross pass R x F; compares on the accumulator registers, row-side results accumulate in registers over
//                          the walk and leave through integer LDS / global atomics, the column-side flag through atomicOr.
//                          bound: fp64 MFMA, as above
//   nn_argmin_kernel       cross pass Q x B (or a set against itself without the diagonal): the nearest base row of every query
//                          row WITH ITS INDEX (authenticity.py).  The lexicographic minimum of (d2, index) stays in the registers
//                          of the thread that owns the accumulator rows over the whole walk; the 32 threads that share a row meet
//                          once per workgroup in the slab buffer; one candidate per (row, split).  bound: fp64 MFMA, as above
//   nn_merge_kernel        one thread per row: the minimum of its S candidates.  bound: latency
//
// Reproducible by construction: the only cross-workgroup combination is integer add / or (order-independent) and a minimum
// selection over candidates (order-independent); there are no floating-point atomics.
#include "common.h"
#include "rows_tile.h"

#define KNN_MAX_K 16
#define KNN_MAX_ROWS ((int64_t)1 << 24)
#define KNN_MAX_SPLITS 1024
#define KNN_TP 65        // pitch in doubles of the staged d2 tile: 64 * 65 * 8 = 33 280 bytes <= the 34 816 of the slab buffer

static_assert(64 * KNN_TP * sizeof(double) <= GT_ROWS_LDS_FLOATS * sizeof(float), "the staged tile must fit the slab buffer");

// ascending list of the KL smallest values met
template <int KL>
__device__ __forceinline__ void knn_insert(double (&best)[KL], double v) {
    if (v < best[KL - 1]) {
        best[KL - 1] = v;
#pragma unroll
        for (int j = KL - 1; j > 0; --j) {
            const double lo = fmin(best[j - 1], best[j]), hi = fmax(best[j - 1], best[j]);
            best[j - 1] = lo;
            best[j] = hi;
        }
    }
}

template <int KL>
__global__ __launch_bounds__(256, 2) void knn_radius2_kernel(const float* __restrict__ X, int64_t ld, int n, int d, int k,
                                                             const double* __restrict__ norm, double* __restrict__ cand) {
    __shared__ __attribute__((aligned(16))) float lds[GT_ROWS_LDS_FLOATS];
    const int tm = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int T = (n + 63) >> 6;
    const int t0 = (int)((int64_t)s * T / S), t1 = (int)((int64_t)(s + 1) * T / S);
    const int tid = threadIdx.x;
    const GtAccLanes at;
    GtRowFetch fa, fb;
    fa.bind(X, ld, nullptr, 0, tm * 64, n, tid);
    double na[2][4];
    gt_rows_load(na, norm, tm * 64, n, at);
    double best[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) best[j] = __builtin_inf();
    double* tile = reinterpret_cast<double*>(lds);
    for (int tn = t0; tn < t1; ++tn) {
        fb.bind(X, ld, nullptr, 0, tn * 64, n, tid);
        double4_t acc[2][2];
        gt_acc_zero(acc);
        gemm_tile_64x64_rows_f32(fa, fb, d, acc, lds);
        // every wave is past the K loop's last barrier: the slab buffer is free.  i == j and columns past n become +inf
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int cl = at.col(b), col = tn * 64 + cl;
            const double nb = norm[col < n ? col : n - 1];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rl = at.row(a, r), row = tm * 64 + rl;
                    const double v = rows_d2(na[a][r], nb, acc[a][b][r]);
                    tile[rl * KNN_TP + cl] = (col < n && row != col) ? v : __builtin_inf();
                }
        }
        __syncthreads();
        if (tid < 64) {
#pragma unroll 8
            for (int c = 0; c < 64; ++c) knn_insert<KL>(best, tile[tid * KNN_TP + c]);
        }
        __syncthreads();                                      // the next tile's first slab store overwrites the staged values
    }
    const int row = tm * 64 + tid;
    if (tid < 64 && row < n) {
        double* out = cand + ((int64_t)row * S + s) * k;
#pragma unroll
        for (int j = 0; j < KL; ++j)
            if (j < k) out[j] = best[j];
    }
}

// r2[row] = the k-th smallest of the row's S * k candidates (+inf entries: a split that held fewer than k other rows); NaN for a
// row that holds a non-finite value (its norm is NaN, and no pair with it was a candidate anywhere)
__global__ __launch_bounds__(256) void knn_merge_kernel(const double* __restrict__ cand, const double* __restrict__ norm, int n,
                                                        int S, int k, double* __restrict__ r2) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    double best[KNN_MAX_K];
#pragma unroll
    for (int j = 0; j < KNN_MAX_K; ++j) best[j] = __builtin_inf();
    const double* p = cand + (int64_t)row * S * k;
    for (int i = 0; i < S * k; ++i) knn_insert<KNN_MAX_K>(best, p[i]);
    double v = best[0];
#pragma unroll
    for (int j = 1; j < KNN_MAX_K; ++j)
        if (j == k - 1) v = best[j];
    const double nr = norm[row];
    r2[row] = nr == nr ? v : nr;
}

__global__ __launch_bounds__(256, 2) void prdc_counts_kernel(const float* __restrict__ R, int64_t ldr, int n,
                                                             const double* __restrict__ r2r, const float* __restrict__ F,
                                                             int64_t ldf, int m, const double* __restrict__ r2f, int d,
                                                             const double* __restrict__ norm_r, const double* __restrict__ norm_f,
                                                             int* __restrict__ cnt, int* __restrict__ rec, int* __restrict__ prec) {
    __shared__ __attribute__((aligned(16))) float lds[GT_ROWS_LDS_FLOATS];
    __shared__ int row_cnt[64], row_rec[64];
    const int tm = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int T = (m + 63) >> 6;
    const int t0 = (int)((int64_t)s * T / S), t1 = (int)((int64_t)(s + 1) * T / S);
    const int tid = threadIdx.x, lane = tid & 63;
    const GtAccLanes at;
    if (tid < 64) row_cnt[tid] = row_rec[tid] = 0;
    __syncthreads();
    GtRowFetch fa, fb;
    fa.bind(R, ldr, nullptr, 0, tm * 64, n, tid);
    double na[2][4], ra[2][4];
    int c_cnt[2][4] = {}, c_rec[2][4] = {};
    gt_rows_load(na, norm_r, tm * 64, n, at);
    gt_rows_load(ra, r2r, tm * 64, n, at);
    for (int tn = t0; tn < t1; ++tn) {
        fb.bind(F, ldf, nullptr, 0, tn * 64, m, tid);
        double4_t acc[2][2];
        gt_acc_zero(acc);
        gemm_tile_64x64_rows_f32(fa, fb, d, acc, lds);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = tn * 64 + at.col(b);
            const bool col_on = col < m;
            const double nb = norm_f[col_on ? col : m - 1], rb = r2f[col_on ? col : m - 1];
            int hit = 0;                                      // some real row of this thread has the column inside its ball
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tm * 64 + at.row(a, r);
                    const double v = rows_d2(na[a][r], nb, acc[a][b][r]);
                    const bool on = col_on && row < n;
                    const int in_r = (on && v < ra[a][r]) ? 1 : 0, in_f = (on && v < rb) ? 1 : 0;
                    c_cnt[a][r] += in_r;
                    c_rec[a][r] |= in_f;
                    hit |= in_r;
                }
            hit |= __shfl_xor(hit, 16, 64);                   // the four lane groups of a wave hold the same column
            hit |= __shfl_xor(hit, 32, 64);
            if (hit && lane < 16) atomicOr(&prec[col], 1);
        }
    }
    // the walk's last barrier lies behind every wave: fold the 32 threads that share a row through LDS, then one global
    // integer atomic per row and workgroup
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = at.row(a, r);
            if (c_cnt[a][r]) atomicAdd(&row_cnt[rl], c_cnt[a][r]);
            if (c_rec[a][r]) atomicOr(&row_rec[rl], 1);
        }
    __syncthreads();
    const int row = tm * 64 + tid;
    if (tid < 64 && row < n) {
        if (row_cnt[tid]) atomicAdd(&cnt[row], row_cnt[tid]);
        if (row_rec[tid]) atomicOr(&rec[row], 1);
    }
}

// ---- nearest row of another set, with its index ------------------------------------------------------------------------------
// The only combination, in a thread, in a workgroup and across the splits: the lexicographic minimum of (d2, index).  It is
// order-independent, so the result does not depend on the walk, on the lane map or on col_splits.  A NaN d2 (a non-finite row
// on either side) fails both comparisons and is never a candidate.
#define NN_NONE 0x7fffffff   // the index of "no candidate": it sorts after every real index, and d2 = +inf with it
#define NN_TP 33             // pitch of the end-of-walk staging: 64 rows x 32 threads that share a row

static_assert(64 * NN_TP * (sizeof(double) + sizeof(int)) <= GT_ROWS_LDS_FLOATS * sizeof(float), "the staged candidates must fit the slab buffer");

__device__ __forceinline__ void nn_take(double& best, int& bestj, double v, int j) {
    if (v < best || (v == best && j < bestj)) {
        best = v;
        bestj = j;
    }
}

// Q x B pass.  Every thread keeps one (d2, index) for each of its eight accumulator rows over the whole walk -- the first
// minimum is taken on the accumulator registers, nothing is staged per tile -- and the 32 threads that share a row meet once,
// after the walk, in the slab buffer.  bound: fp64 MFMA, as knn_radius2_kernel, without its per-tile scan
__global__ __launch_bounds__(256, 2) void nn_argmin_kernel(const float* __restrict__ Q, int64_t ldq, int n, const float* __restrict__ B,
                                                           int64_t ldb, int m, int d, int exclude_diagonal,
                                                           const double* __restrict__ norm_q, const double* __restrict__ norm_b,
                                                           double* __restrict__ cand_d2, int* __restrict__ cand_idx) {
    __shared__ __attribute__((aligned(16))) float lds[GT_ROWS_LDS_FLOATS];
    const int tm = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int T = (m + 63) >> 6;
    const int t0 = (int)((int64_t)s * T / S), t1 = (int)((int64_t)(s + 1) * T / S);
    const int tid = threadIdx.x;
    const GtAccLanes at;
    GtRowFetch fa, fb;
    fa.bind(Q, ldq, nullptr, 0, tm * 64, n, tid);
    double na[2][4], best[2][4];
    int bestj[2][4];
    gt_rows_load(na, norm_q, tm * 64, n, at);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            best[a][r] = __builtin_inf();
            bestj[a][r] = NN_NONE;
        }
    for (int tn = t0; tn < t1; ++tn) {
        fb.bind(B, ldb, nullptr, 0, tn * 64, m, tid);
        double4_t acc[2][2];
        gt_acc_zero(acc);
        gemm_tile_64x64_rows_f32(fa, fb, d, acc, lds);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = tn * 64 + at.col(b);
            const bool col_on = col < m;
            const double nb = norm_b[col_on ? col : m - 1];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tm * 64 + at.row(a, r);
                    const double v = rows_d2(na[a][r], nb, acc[a][b][r]);
                    if (col_on && !(exclude_diagonal && row == col)) nn_take(best[a][r], bestj[a][r], v, col);
                }
        }
    }
    // the walk's last barrier lies behind every wave: the slab buffer is free.  Slot = this thread's place among the 32 that hold
    // the same rows (2 wave columns x 16 lanes)
    double* sd = reinterpret_cast<double*>(lds);
    int* sj = reinterpret_cast<int*>(sd + 64 * NN_TP);
    const int slot = ((tid >> 6) & 1) * 16 + (tid & 15);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sd[at.row(a, r) * NN_TP + slot] = best[a][r];
            sj[at.row(a, r) * NN_TP + slot] = bestj[a][r];
        }
    __syncthreads();
    const int row = tm * 64 + tid;
    if (tid < 64 && row < n) {
        double v = __builtin_inf();
        int j = NN_NONE;
#pragma unroll 8
        for (int c = 0; c < 32; ++c) nn_take(v, j, sd[tid * NN_TP + c], sj[tid * NN_TP + c]);
        cand_d2[(int64_t)row * S + s] = v;
        cand_idx[(int64_t)row * S + s] = j;
    }
}

// one thread per query row: the minimum over its S candidates.  A query row with a non-finite value (norm NaN; no pair with it
// was a candidate) gets (NaN, -1); a row without any candidate (+inf, -1).  bound: latency
__global__ __launch_bounds__(256) void nn_merge_kernel(const double* __restrict__ cand_d2, const int* __restrict__ cand_idx,
                                                       const double* __restrict__ norm_q, int n, int S, double* __restrict__ d2,
                                                       int* __restrict__ idx) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    double v = __builtin_inf();
    int j = NN_NONE;
    for (int i = 0; i < S; ++i) nn_take(v, j, cand_d2[(int64_t)row * S + i], cand_idx[(int64_t)row * S + i]);
    const double nq = norm_q[row];
    d2[row] = nq == nq ? v : nq;
    idx[row] = (nq == nq && j != NN_NONE) ? j : -1;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// column splits of a (rows x cols) pass: the caller's value, or enough to put about four workgroups on each of 256 compute
// units when there are few row tiles; never more than there are column tiles.  A function of the sizes alone (no device query),
// so that tise_knn_workspace_bytes is one too.
static int knn_splits(int64_t rows, int64_t cols, int col_splits) {
    const int64_t tr = (rows + 63) / 64, tc = (cols + 63) / 64;
    int64_t s = col_splits > 0 ? col_splits : (1024 + tr - 1) / tr;
    if (s > tc) s = tc;
    if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
    return (int)(s < 1 ? 1 : s);
}

static int knn_side_check(const float* p, int64_t rows, int64_t ld, int d, int64_t min_rows) {
    if (!p || rows < min_rows) return TISE_ERR_INVALID_ARG;
    const int rc = rows_layout_check(p, rows, ld, d);
    if (rc != TISE_OK) return rc;
    return rows > KNN_MAX_ROWS ? TISE_ERR_UNSUPPORTED : TISE_OK;
}

extern "C" {

int tise_knn_workspace_bytes(int64_t rows, int k, int col_splits, size_t* bytes) {
    if (!bytes || k < 1 || k > KNN_MAX_K || rows < (int64_t)k + 1 || col_splits < 0 || col_splits > KNN_MAX_SPLITS) return TISE_ERR_INVALID_ARG;
    if (rows > KNN_MAX_ROWS) return TISE_ERR_UNSUPPORTED;
    *bytes = sizeof(double) * (size_t)rows * ((size_t)knn_splits(rows, rows, col_splits) * (size_t)k + 1);
    return TISE_OK;
}

int tise_knn_radius2(const float* x_dev, int64_t rows, int64_t ld, int d, int k, int col_splits, double* r2_dev, void* ws_dev,
                     size_t ws_bytes, void* stream) {
    if (k < 1 || k > KNN_MAX_K || col_splits < 0 || col_splits > KNN_MAX_SPLITS) return TISE_ERR_INVALID_ARG;
    int rc = knn_side_check(x_dev, rows, ld, d, (int64_t)k + 1);
    if (rc != TISE_OK) return rc;
    if (!r2_dev || (reinterpret_cast<uintptr_t>(r2_dev) & 7)) return TISE_ERR_INVALID_ARG;
    size_t need = 0;
    rc = tise_knn_workspace_bytes(rows, k, col_splits, &need);
    if (rc != TISE_OK) return rc;
    if (!ws_dev || (reinterpret_cast<uintptr_t>(ws_dev) & 7) || ws_bytes < need) return TISE_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int S = knn_splits(rows, rows, col_splits), n = (int)rows;
    double* norm = reinterpret_cast<double*>(ws_dev);
    double* cand = norm + rows;
    rc = rows_norm2(x_dev, ld, nullptr, 0, rows, nullptr, 0, nullptr, 0, 0, d, norm, st);
    if (rc != TISE_OK) return rc;
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)S);
    if (k <= 4) hipLaunchKernelGGL(knn_radius2_kernel<4>, grid, dim3(256), 0, st, x_dev, ld, n, d, k, norm, cand);
    else if (k <= 8) hipLaunchKernelGGL(knn_radius2_kernel<8>, grid, dim3(256), 0, st, x_dev, ld, n, d, k, norm, cand);
    else hipLaunchKernelGGL(knn_radius2_kernel<KNN_MAX_K>, grid, dim3(256), 0, st, x_dev, ld, n, d, k, norm, cand);
    TISE_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cand, norm, n, S, k, r2_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_prdc_counts(const float* r_dev, int64_t rows_r, int64_t ld_r, const double* r2_r_dev, const float* f_dev, int64_t rows_f,
                     int64_t ld_f, const double* r2_f_dev, int d, int col_splits, int32_t* cnt_dev, int32_t* rec_dev,
                     int32_t* prec_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    if (col_splits < 0 || col_splits > KNN_MAX_SPLITS) return TISE_ERR_INVALID_ARG;
    int rc = knn_side_check(r_dev, rows_r, ld_r, d, 1);
    if (rc != TISE_OK) return rc;
    rc = knn_side_check(f_dev, rows_f, ld_f, d, 1);
    if (rc != TISE_OK) return rc;
    if (!r2_r_dev || !r2_f_dev || ((reinterpret_cast<uintptr_t>(r2_r_dev) | reinterpret_cast<uintptr_t>(r2_f_dev)) & 7)) return TISE_ERR_INVALID_ARG;
    if (!cnt_dev || !rec_dev || !prec_dev) return TISE_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(cnt_dev) | reinterpret_cast<uintptr_t>(rec_dev) | reinterpret_cast<uintptr_t>(prec_dev)) & 3) return TISE_ERR_INVALID_ARG;
    if (!ws_dev || (reinterpret_cast<uintptr_t>(ws_dev) & 7) || ws_bytes < sizeof(double) * (size_t)(rows_r + rows_f)) return TISE_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)rows_r, m = (int)rows_f;
    double* norm_r = reinterpret_cast<double*>(ws_dev);
    double* norm_f = norm_r + rows_r;
    TISE_HIP_CHECK(hipMemsetAsync(cnt_dev, 0, sizeof(int32_t) * (size_t)n, st));
    TISE_HIP_CHECK(hipMemsetAsync(rec_dev, 0, sizeof(int32_t) * (size_t)n, st));
    TISE_HIP_CHECK(hipMemsetAsync(prec_dev, 0, sizeof(int32_t) * (size_t)m, st));
    rc = rows_norm2(r_dev, ld_r, nullptr, 0, rows_r, f_dev, ld_f, nullptr, 0, rows_f, d, norm_r, st);   // norm_f = norm_r + rows_r
    if (rc != TISE_OK) return rc;
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)knn_splits(rows_r, rows_f, col_splits));
    hipLaunchKernelGGL(prdc_counts_kernel, grid, dim3(256), 0, st, r_dev, ld_r, n, r2_r_dev, f_dev, ld_f, m, r2_f_dev, d, norm_r,
                       norm_f, cnt_dev, rec_dev, prec_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_nn_workspace_bytes(int64_t rows_q, int64_t rows_b, int col_splits, size_t* bytes) {
    if (!bytes || rows_q < 1 || rows_b < 1 || col_splits < 0 || col_splits > KNN_MAX_SPLITS) return TISE_ERR_INVALID_ARG;
    if (rows_q > KNN_MAX_ROWS || rows_b > KNN_MAX_ROWS) return TISE_ERR_UNSUPPORTED;
    const size_t S = (size_t)knn_splits(rows_q, rows_b, col_splits);
    *bytes = sizeof(double) * (size_t)(rows_q + rows_b) + (sizeof(double) + sizeof(int32_t)) * (size_t)rows_q * S;
    return TISE_OK;
}

int tise_nn_argmin(const float* q_dev, int64_t rows_q, int64_t ld_q, const float* b_dev, int64_t rows_b, int64_t ld_b, int d,
                   int exclude_diagonal, int col_splits, double* d2_dev, int32_t* idx_dev, void* ws_dev, size_t ws_bytes,
                   void* stream) {
    if (col_splits < 0 || col_splits > KNN_MAX_SPLITS || (exclude_diagonal != 0 && exclude_diagonal != 1)) return TISE_ERR_INVALID_ARG;
    int rc = knn_side_check(q_dev, rows_q, ld_q, d, 1);
    if (rc != TISE_OK) return rc;
    rc = knn_side_check(b_dev, rows_b, ld_b, d, 1);
    if (rc != TISE_OK) return rc;
    if (exclude_diagonal && rows_q != rows_b) return TISE_ERR_INVALID_ARG;
    if (!d2_dev || !idx_dev || (reinterpret_cast<uintptr_t>(d2_dev) & 7) || (reinterpret_cast<uintptr_t>(idx_dev) & 3)) return TISE_ERR_INVALID_ARG;
    size_t need = 0;
    rc = tise_nn_workspace_bytes(rows_q, rows_b, col_splits, &need);
    if (rc != TISE_OK) return rc;
    if (!ws_dev || (reinterpret_cast<uintptr_t>(ws_dev) & 7) || ws_bytes < need) return TISE_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int S = knn_splits(rows_q, rows_b, col_splits), n = (int)rows_q, m = (int)rows_b;
    double* norm_q = reinterpret_cast<double*>(ws_dev);
    double* norm_b = norm_q + rows_q;
    double* cand_d2 = norm_b + rows_b;
    int* cand_idx = reinterpret_cast<int*>(cand_d2 + (size_t)rows_q * S);
    rc = rows_norm2(q_dev, ld_q, nullptr, 0, rows_q, b_dev, ld_b, nullptr, 0, rows_b, d, norm_q, st);   // norm_b = norm_q + rows_q
    if (rc != TISE_OK) return rc;
    hipLaunchKernelGGL(nn_argmin_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)S), dim3(256), 0, st, q_dev, ld_q, n, b_dev, ld_b,
                       m, d, exclude_diagonal, norm_q, norm_b, cand_d2, cand_idx);
    TISE_LAUNCH_CHECK();
    hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cand_d2, cand_idx, norm_q, n, S, d2_dev,
                       idx_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

}  // extern "C"
