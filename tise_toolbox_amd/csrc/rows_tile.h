// 64x64 fp64 output tile on v_mfma_f64_16x16x4_f64 (gfx950) in NT form on GATHERED fp32 rows: acc += A B^T, tile row m of an operand
// = an arbitrary row of a feature matrix.  The primitive of csrc/mmd.hip (KID, CMMD) and csrc/knn.hip (PRDC), with everything those
// kernels must do the same way to give the same bits for the same pair of rows: the fetch and its layout contract, the accumulator
// lane map, the row norms and the squared distance formed from them.  NOT here, on purpose: a walker over a thread's sixteen
// accumulator elements -- the order in which a kernel adds or stages them is part of its result and stays written out there.
//
// 256 threads = 4 waves in a 2x2 grid, each wave owns a 32x32 sub-tile (2x2 MFMA tiles, 4 x double4 accumulators), as gemm_tile.h,
// with which this file shares no code.  Both operands are contiguous along k, so a slab is 64 rows x GT_RK k-values per operand,
// fetched as float4 (8 in flight per thread under 64 MFMAs per wave on the previous slab -- the depth the covariance kernel's
// fast path needs, stats.hip) and kept fp32 in LDS as [row][k]; the widening to fp64 is exact and happens in registers.  Pitch 68
// floats: the ds_read_b32 of a fragment (row = lane & 15, k = lane >> 4) lands on bank (4 row + k) mod 64 -- all 64 lanes on
// different banks -- and a row stays 16-byte aligned for the float4 stores.
#pragma once
#include "common.h"

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

// The fetch's layout contract, host side: d in [1, 2^20], rows >= 0, a row pitch ld >= d that is a multiple of 4 floats, a
// 16-byte aligned base (null passes: whether there may be no rows is the entry point's business), rows * ld <= 2^40.
static inline bool rows_width_ok(int d) { return d > 0 && d <= (1 << 20); }
static inline int rows_layout_check(const float* p, int64_t rows, int64_t ld, int d) {
    if (!rows_width_ok(d) || rows < 0 || ld < d || (ld & 3) || (reinterpret_cast<uintptr_t>(p) & 15)) return TISE_ERR_INVALID_ARG;
    return rows > ((int64_t)1 << 40) / ld ? TISE_ERR_UNSUPPORTED : TISE_OK;
}

// acc[a][b][r] of this thread is the tile's local row row(a, r), local column col(b) (MFMA D: col = lane & 15, row = (lane >> 4) + 4 reg)
struct GtAccLanes {
    int r0, c0;
    __device__ __forceinline__ GtAccLanes() {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        r0 = (wave >> 1) * 32 + (lane >> 4);
        c0 = (wave & 1) * 32 + (lane & 15);
    }
    __device__ __forceinline__ int row(int a, int r) const { return r0 + a * 16 + 4 * r; }
    __device__ __forceinline__ int col(int b) const { return c0 + b * 16; }
};

__device__ __forceinline__ void gt_acc_zero(double4_t (&acc)[2][2]) {
    acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = (double4_t){0.0, 0.0, 0.0, 0.0};
}

// v[a][r] = x[first + row(a, r)] of n >= 1 per-row values; a row past the last reads the last (as the fetch does), the caller masks it
template <typename T>
__device__ __forceinline__ void gt_rows_load(T (&v)[2][4], const T* __restrict__ x, int first, int n, const GtAccLanes& at) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[a][r] = x[min(first + at.row(a, r), n - 1)];
}

// The squared distance the callers form from the tile, d2 = max(0, (|a|^2 + |b|^2) - 2 a.b), must not hide a row that holds a
// NaN or an infinity: fmax returns the operand that is not NaN and would turn such a pair into d2 = 0, the nearest neighbour of
// every row.  The rule (include/tise_hip.h, "Non-finite feature rows"): the norm pre-pass writes NaN for a row whose sum of squares
// is not finite, and the clamp keeps a NaN, so d2 of every pair with such a row is NaN and every comparison with it is false.  For
// finite operands both return the bits they were given (never -0: the norms are sums of squares and the accumulators start at +0).
__device__ __forceinline__ double rows_norm2_or_nan(double s) { return __builtin_isfinite(s) ? s : __builtin_nan(""); }
__device__ __forceinline__ double rows_clamp_d2(double x) { return x < 0.0 ? 0.0 : x; }
// one value per pair, whichever kernel asks and whichever side each row is on; the parentheses are the contract
__device__ __forceinline__ double rows_d2(double na, double nb, double dot) { return rows_clamp_d2((na + nb) - 2.0 * dot); }

// fp64 |row|^2 of cx + cy rows: wave w takes position x0 + w of the x side, or y0 + (w - cx) of the y side (a count of 0 switches
// a side off); position p is row p of the side's matrix, or row index[p].  Lane l adds the exact squares of columns l, l + 64,
// ... in order, then the fixed butterfly; out[0 .. cx) = the x side's norms, out[cx .. cx + cy) = the y side's.  static: the
// kernel is compiled into every object that includes this header.
static __global__ __launch_bounds__(256) void rows_norm2_kernel(const float* __restrict__ X, int64_t ldx, const int64_t* __restrict__ ix,
                                                                int64_t x0, int64_t cx, const float* __restrict__ Y, int64_t ldy,
                                                                const int64_t* __restrict__ iy, int64_t y0, int64_t cy, int d,
                                                                double* __restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= cx + cy) return;                                 // wave-uniform
    const bool y = w >= cx;
    const int64_t p = y ? y0 + (w - cx) : x0 + w;
    const int64_t* idx = y ? iy : ix;
    const int64_t r = idx ? idx[p] : p;
    const float* row = (y ? Y : X) + r * (y ? ldy : ldx);
    double s = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double v = (double)row[c];
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) out[w] = rows_norm2_or_nan(s);
}

static inline int rows_norm2(const float* X, int64_t ldx, const int64_t* ix, int64_t x0, int64_t cx, const float* Y, int64_t ldy,
                             const int64_t* iy, int64_t y0, int64_t cy, int d, double* out, hipStream_t st) {
    hipLaunchKernelGGL(rows_norm2_kernel, dim3((unsigned)((cx + cy + 3) / 4)), dim3(256), 0, st, X, ldx, ix, x0, cx, Y, ldy, iy, y0,
                       cy, d, out);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

// acc[a][b] += sum_k A(m, k) B(n, k) over k in [0, d)
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
