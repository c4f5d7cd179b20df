// 64x64 fp64 output tile on v_mfma_f64_16x16x4_f64 (gfx950), shared by the covariance
// accumulator (fp32 feature rows in) and the Frechet-distance GEMMs (fp64 in).
//
// Workgroup = 256 threads = 4 waves in a 2x2 grid, each wave owns a 32x32 sub-tile
// (2x2 MFMA tiles, 4 x double4 accumulators).  K is walked in steps of 16 through LDS:
// the next K-slab is fetched into registers while the current one feeds the MFMAs.
//
// Operand addressing is by strides so the same tile serves A^T A (feature rows, m
// contiguous), row-major NN and NT products:
//     A(m,k) = A[m*sam + k*sak]      B(k,n) = B[k*sbk + n*sbn]
// The global->LDS fetch picks the lane order that is contiguous in memory for each operand.
//
// MFMA lane maps (cdna_hip_programming.md section 3, f64 form): A[i = lane&15][k = lane>>4],
// B[k = lane>>4][j = lane&15]; D: col = lane&15, row = (lane>>4) + 4*reg.
#pragma once
#include "common.h"

#define GT_BM 64
#define GT_BN 64
#define GT_BK 16
// LDS row pitch in doubles: 80 = 64 + 16 puts the two k-rows a 32-lane half reads with one
// ds_read_b64 on disjoint banks ((a/4) % 64 banking for b64 reads).
#define GT_PITCH 80
#define GT_LDS_DOUBLES (2 * GT_BK * GT_PITCH)

template <typename T>
struct GtFetch {
    double v[4];
    // lim = number of valid entries along the 64-wide (m or n) dimension starting at x0
    __device__ __forceinline__ void load(const T* __restrict__ p, int64_t sx, int64_t sk, int x0, int xlim,
                                         int k0, int klim, int tid) {
        if (sx == 1) {  // contiguous along the 64-wide dimension: 64 consecutive lanes per k row
            const int x = tid & 63;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = (tid >> 6) + 4 * q;
                v[q] = (x0 + x < xlim && k0 + k < klim) ? (double)p[(int64_t)(x0 + x) * sx + (int64_t)(k0 + k) * sk] : 0.0;
            }
        } else {        // contiguous along k: 16 consecutive lanes per row
            const int k = tid & 15;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int x = (tid >> 4) + 16 * q;
                v[q] = (x0 + x < xlim && k0 + k < klim) ? (double)p[(int64_t)(x0 + x) * sx + (int64_t)(k0 + k) * sk] : 0.0;
            }
        }
    }
    __device__ __forceinline__ void store(double* __restrict__ lds, int64_t sx, int tid) const {
        if (sx == 1) {
            const int x = tid & 63;
#pragma unroll
            for (int q = 0; q < 4; ++q) lds[((tid >> 6) + 4 * q) * GT_PITCH + x] = v[q];
        } else {
            const int k = tid & 15;
#pragma unroll
            for (int q = 0; q < 4; ++q) lds[k * GT_PITCH + (tid >> 4) + 16 * q] = v[q];
        }
    }
};

// acc[tm][tn] += A(m0.., :) * B(:, n0..)  over k in [0, K)
template <typename TA, typename TB>
__device__ __forceinline__ void gemm_tile_64x64(const TA* __restrict__ A, int64_t sam, int64_t sak,
                                                const TB* __restrict__ B, int64_t sbk, int64_t sbn, int M, int N,
                                                int K, int m0, int n0, double4_t (&acc)[2][2], double* lds) {
    double* As = lds;
    double* Bs = lds + GT_BK * GT_PITCH;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int fi = lane & 15, fk = lane >> 4;

    GtFetch<TA> fa;
    GtFetch<TB> fb;
    fa.load(A, sam, sak, m0, M, 0, K, tid);
    fb.load(B, sbn, sbk, n0, N, 0, K, tid);
    for (int k0 = 0; k0 < K; k0 += GT_BK) {
        fa.store(As, sam, tid);
        fb.store(Bs, sbn, tid);
        __syncthreads();
        if (k0 + GT_BK < K) {
            fa.load(A, sam, sak, m0, M, k0 + GT_BK, K, tid);
            fb.load(B, sbn, sbk, n0, N, k0 + GT_BK, K, tid);
        }
#pragma unroll
        for (int kk = 0; kk < GT_BK; kk += 4) {
            const double a0 = As[(kk + fk) * GT_PITCH + wr * 32 + fi];
            const double a1 = As[(kk + fk) * GT_PITCH + wr * 32 + 16 + fi];
            const double b0 = Bs[(kk + fk) * GT_PITCH + wc * 32 + fi];
            const double b1 = Bs[(kk + fk) * GT_PITCH + wc * 32 + 16 + fi];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}

// write / accumulate the wave's 32x32 sub-tile.  MODE 0: C = acc, 1 (true): C += acc, 2: C -= acc.
template <int MODE>
__device__ __forceinline__ void gemm_tile_store(double* __restrict__ C, int64_t ldc, int M, int N, int m0, int n0,
                                                const double4_t (&acc)[2][2]) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wr * 32 + tm * 16 + (lane >> 4) + 4 * r;
                const int col = n0 + wc * 32 + tn * 16 + (lane & 15);
                if (row < M && col < N) {
                    double* p = C + (int64_t)row * ldc + col;
                    if (MODE == 1) *p += acc[tm][tn][r];
                    else if (MODE == 2) *p -= acc[tm][tn][r];
                    else *p = acc[tm][tn][r];
                }
            }
}

// ---- NT form on GATHERED fp32 rows (csrc/mmd.hip): acc += A B^T, tile row m of A = an arbitrary row of a feature matrix.
// Both operands are contiguous along k, so a slab is 64 rows x GT_RK k-values per operand, fetched as float4 (8 in flight per
// thread under 64 MFMAs per wave on the previous slab -- the depth the covariance kernel's fast path needs, stats.hip) and kept
// fp32 in LDS as [row][k]; the widening to fp64 is exact and happens in registers.  Pitch 68 floats: the ds_read_b32 of a
// fragment (row = lane & 15, k = lane >> 4) lands on bank (4 row + k) mod 64 -- all 64 lanes on different banks -- and a row
// stays 16-byte aligned for the float4 stores.  The existing tile above is untouched.
#define GT_RK 64
#define GT_RP 68
#define GT_ROWS_LDS_FLOATS (2 * 64 * GT_RP)

struct GtRowFetch {
    float4 v[4];
    const float* row[4];          // tile rows (tid >> 4) + 16 q, already advanced to this thread's k offset (tid & 15) * 4
    // rows x0 .. x0 + 63 of a group of n >= 1 rows that starts at r0: row r0 + m of `base` (index == nullptr) or row
    // index[r0 + m].  Rows past the group are fetched from its last row: the caller masks them in its epilogue.
    __device__ __forceinline__ void bind(const float* __restrict__ base, int64_t ld, const int64_t* __restrict__ index,
                                         int64_t r0, int x0, int n, int tid) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int m = x0 + (tid >> 4) + 16 * q;
            m = m < n ? m : n - 1;
            const int64_t r = index ? index[r0 + m] : r0 + m;
            row[q] = base + r * ld + (tid & 15) * 4;
        }
    }
    // k0 % 4 == 0, rows 16-byte aligned (ld % 4 == 0): a float4 that lies inside [0, d) is one load, the tail of a row whose d
    // is not a multiple of 4 is read element by element, nothing at or beyond column d is touched
    __device__ __forceinline__ void load(int k0, int d, int tid) {
        const int k = k0 + (tid & 15) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (k + 3 < d) {
                v[q] = *reinterpret_cast<const float4*>(row[q] + k0);
            } else {
                v[q].x = k < d ? row[q][k0] : 0.f;
                v[q].y = k + 1 < d ? row[q][k0 + 1] : 0.f;
                v[q].z = k + 2 < d ? row[q][k0 + 2] : 0.f;
                v[q].w = 0.f;
            }
        }
    }
    __device__ __forceinline__ void store(float* __restrict__ lds, int tid) const {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(lds + ((tid >> 4) + 16 * q) * GT_RP + (tid & 15) * 4) = v[q];
    }
};

// The squared distance the callers form from the tile, d2 = max(0, (|a|^2 + |b|^2) - 2 a.b), must not hide a row that holds a
// NaN or an infinity: fmax returns the operand that is not NaN and would turn such a pair into d2 = 0, the nearest neighbour of
// every row.  The rule (include/tise_hip.h, "Non-finite feature rows"): the norm pre-pass writes NaN for a row whose sum of
// squares is not finite, and the clamp keeps a NaN, so d2 of every pair with such a row is NaN and every comparison with it is
// false.  For finite operands both functions return the bits they were given (the difference is never -0: the norms are sums
// of squares from +0 and the accumulators start at +0).
__device__ __forceinline__ double rows_norm2_or_nan(double s) { return __builtin_isfinite(s) ? s : __builtin_nan(""); }
__device__ __forceinline__ double rows_clamp_d2(double x) { return x < 0.0 ? 0.0 : x; }

// acc[tm][tn] += sum_k A(m, k) B(n, k) over k in [0, d); same wave grid and accumulator layout as gemm_tile_64x64
__device__ __forceinline__ void gemm_tile_64x64_rows_f32(GtRowFetch& fa, GtRowFetch& fb, int d, double4_t (&acc)[2][2],
                                                         float* lds) {
    float* As = lds;
    float* Bs = lds + 64 * GT_RP;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int fi = lane & 15, fk = lane >> 4;
    fa.load(0, d, tid);
    fb.load(0, d, tid);
    for (int k0 = 0; k0 < d; k0 += GT_RK) {
        fa.store(As, tid);
        fb.store(Bs, tid);
        __syncthreads();
        if (k0 + GT_RK < d) {
            fa.load(k0 + GT_RK, d, tid);
            fb.load(k0 + GT_RK, d, tid);
        }
#pragma unroll
        for (int kk = 0; kk < GT_RK; kk += 4) {
            const double a0 = (double)As[(wr * 32 + fi) * GT_RP + kk + fk];
            const double a1 = (double)As[(wr * 32 + 16 + fi) * GT_RP + kk + fk];
            const double b0 = (double)Bs[(wc * 32 + fi) * GT_RP + kk + fk];
            const double b1 = (double)Bs[(wc * 32 + 16 + fi) * GT_RP + kk + fk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}
