// PSNR, SSIM and MS-SSIM of image PAIRS (tise_toolbox_amd/paired.py): the exact squared error, the Gaussian-window moments in
// fp64 and the 2 x 2 mean of the five-scale pyramid.  No counterpart in the reference toolbox; the definitions are restated
// from Wang, Bovik, Sheikh & Simoncelli 2004 (SSIM) and Wang, Simoncelli & Bovik 2003 (MS-SSIM) in include/tise_hip.h and
// tests/_ssim_ref.py is the numpy fp64 restatement every kernel here is pinned to.
//
// All three entry points are RAGGED: a device table of tise_pair_t {x, y, h, w}, one record per pair, one launch for any list
// of pairs of any sizes (a uniform batch builds the same table).  The host knows the table's largest h and w (max_h, max_w: it
// sizes the grid and the workspace by them); a workgroup whose tile lies outside its own pair's size leaves at once.  Nothing a
// pair's result is formed from depends on max_h, max_w or on the other pairs of the launch.
//
// ssim_tile_kernel.  The image pair is taken CHANNEL-INTERLEAVED as it lies in memory: an (h, 3w) matrix whose output column
// j = 3 * pixel + channel has its eleven horizontal taps at j, j + 3, ..., j + 30.  One workgroup of 192 threads (three waves)
// owns an output tile of 64 rows x 192 interleaved columns (64 pixels) and walks DOWN it: per source row it stages the 222
// values of x and of y that the tile's columns need in LDS as fp32 (a byte and a pyramid level are both exact in fp32, so the
// uint8 and the fp32 input take ONE path from there on: the same bits), two buffers, one barrier per row, the next row's
// global loads in flight over the arithmetic.  Lane stride in LDS is one dword and a tap is 3 dwords further: no bank conflict
// (the 3-byte pixel stride never reaches LDS).  A thread forms the five horizontal moments of its column
//     sum_k g[k] x_k, sum_k g[k] y_k, sum_k g[k] (x_k x_k), sum_k g[k] (y_k y_k), sum_k g[k] (x_k y_k)
// through ONE function in ONE order (products of two values of <= 16 bits are exact in fp64, then fma(g[k], p, acc) from k = 0
// up), keeps the last eleven rows of them in a REGISTER RING (5 x 11 doubles; the loop over rows is unrolled by 11 so every
// ring index is a compile-time constant) and combines the ring vertically in the same way.  With x == y the three second
// moments are therefore bit-equal, as are the two means.  l and cs are formed without contraction, every product once:
//     cs = (2 sxy + C2) / (sxx + syy + C2),  l = (2 mx my + C1) / (mx mx + my my + C1),  ssim = l * cs
// so an identical pair gives numerator == denominator: exactly 1.0 at every position and 1.0 as the mean.
// Reduction: a thread adds its column's values down the tile (row order), six threads add the 64 columns of each channel in
// column order from LDS, and the tile's six sums {ssim, cs} x {R, G, B} go to the workspace slot of (pair, tile).
// ssim_finish_kernel (one wave per pair) adds a pair's tiles, lane l the tiles l, l + 64, ... in order, then the fixed xor
// butterfly, and divides by the count.  No floating-point atomics; the tile cut depends on the pair's own size only.
// Source traffic: every byte is read (1 + 10/64)(1 + 30/192) = 1.34 times, mostly from L2, and never written back.
//
// The window g[i] = exp(-(i - 5)^2 / 4.5) / sum is six distinct doubles, given as LITERALS (numpy's fp64 values, 17 digits).
#include <math.h>
#include "common.h"

namespace {

constexpr int kTaps = TISE_SSIM_TAPS;                  // 11
constexpr int kTileRows = TISE_SSIM_TILE;              // output rows of a tile
constexpr int kTilePix = TISE_SSIM_TILE;               // output pixels of a tile row
constexpr int kThreads = 3 * kTilePix;                 // one thread per interleaved output column
constexpr int kStage = kThreads + 3 * (kTaps - 1);     // staged values of one source row
constexpr int kMaxSide = TISE_SSIM_MAX_SIDE;
constexpr int64_t kMaxPairs = TISE_SSIM_MAX_PAIRS;
constexpr int64_t kMaxTiles = (int64_t)1 << 22;        // tile slots of one launch (n * tiles of the largest pair)
constexpr int kSseChunk = 256 * 64;                    // bytes of a pair that one workgroup of the squared-error kernel takes

__device__ constexpr double kG[kTaps] = {0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
                                         0.2130055377112537,  0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
                                         0.03600077212843083, 0.007598758135239185, 0.00102838008447911};
constexpr double kC1 = (0.01 * 255.0) * (0.01 * 255.0);
constexpr double kC2 = (0.03 * 255.0) * (0.03 * 255.0);

__host__ __device__ inline int tiles_of(int side) { return (side - (kTaps - 1) + kTileRows - 1) / kTileRows; }

__device__ __forceinline__ bool usable(const tise_pair_t& e, int min_side, int max_h, int max_w) {
    return e.x != nullptr && e.y != nullptr && e.h >= min_side && e.w >= min_side && e.h <= max_h && e.w <= max_w;
}

template <bool F32>
__device__ __forceinline__ float load_value(const void* p, int64_t i) {
    return F32 ? static_cast<const float*>(p)[i] : (float)static_cast<const uint8_t*>(p)[i];
}

template <bool F32>
__global__ __launch_bounds__(kThreads) void ssim_tile_kernel(const tise_pair_t* __restrict__ table, int max_h, int max_w,
                                                             double* __restrict__ ws, int64_t slots_per_pair) {
#pragma clang fp contract(off)
    __shared__ float sx[2][kStage];
    __shared__ float sy[2][kStage];
    __shared__ double red[2][kThreads];
    const tise_pair_t e = table[blockIdx.z];
    if (!usable(e, kTaps, max_h, max_w)) return;
    const int tx = blockIdx.x, ty = blockIdx.y;
    const int own_tx = tiles_of(e.w), own_ty = tiles_of(e.h);
    if (tx >= own_tx || ty >= own_ty) return;
    const int tid = threadIdx.x;
    const int in_cols = 3 * e.w;                                     // interleaved source columns
    const int out_cols = in_cols - 3 * (kTaps - 1);
    const int col0 = tx * kThreads;
    const bool live = col0 + tid < out_cols;
    const int row0 = ty * kTileRows;
    const int out_rows = min(kTileRows, e.h - (kTaps - 1) - row0);
    const int src_rows = out_rows + kTaps - 1;
    // a thread stages the values tid and tid + kThreads of a source row (the second one: the 30 columns of the halo)
    const int ca = col0 + tid, cb = col0 + kThreads + tid;
    const bool has_a = ca < in_cols, has_b = tid < kStage - kThreads && cb < in_cols;
    const int64_t pitch = in_cols;
    int64_t off = (int64_t)row0 * pitch;
    float xa = 0.0f, ya = 0.0f, xb = 0.0f, yb = 0.0f;
    if (has_a) { xa = load_value<F32>(e.x, off + ca); ya = load_value<F32>(e.y, off + ca); }
    if (has_b) { xb = load_value<F32>(e.x, off + cb); yb = load_value<F32>(e.y, off + cb); }

    double ring[5][kTaps];
    double sum_ssim = 0.0, sum_cs = 0.0;
    for (int i0 = 0; i0 < src_rows; i0 += kTaps) {
#pragma unroll
        for (int s = 0; s < kTaps; ++s) {
            const int i = i0 + s;
            if (i >= src_rows) continue;                             // uniform over the workgroup
            const int buf = i & 1;
            sx[buf][tid] = xa;
            sy[buf][tid] = ya;
            if (tid < kStage - kThreads) {
                sx[buf][kThreads + tid] = xb;
                sy[buf][kThreads + tid] = yb;
            }
            if (i + 1 < src_rows) {                                  // the next row's loads fly over this row's arithmetic
                off += pitch;
                if (has_a) { xa = load_value<F32>(e.x, off + ca); ya = load_value<F32>(e.y, off + ca); }
                if (has_b) { xb = load_value<F32>(e.x, off + cb); yb = load_value<F32>(e.y, off + cb); }
            }
            __syncthreads();
            {
                const double x0 = (double)sx[buf][tid], y0 = (double)sy[buf][tid];
                double hx = kG[0] * x0, hy = kG[0] * y0;
                double hxx = kG[0] * (x0 * x0), hyy = kG[0] * (y0 * y0), hxy = kG[0] * (x0 * y0);
#pragma unroll
                for (int k = 1; k < kTaps; ++k) {
                    const double xk = (double)sx[buf][tid + 3 * k], yk = (double)sy[buf][tid + 3 * k];
                    hx = fma(kG[k], xk, hx);
                    hy = fma(kG[k], yk, hy);
                    hxx = fma(kG[k], xk * xk, hxx);
                    hyy = fma(kG[k], yk * yk, hyy);
                    hxy = fma(kG[k], xk * yk, hxy);
                }
                ring[0][s] = hx;
                ring[1][s] = hy;
                ring[2][s] = hxx;
                ring[3][s] = hyy;
                ring[4][s] = hxy;
            }
            if (i >= kTaps - 1) {                                    // rows i - 10 .. i are in the ring: slot of row i - 10 + k is (s + 1 + k) % 11
                double m[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    double v = kG[0] * ring[q][(s + 1) % kTaps];
#pragma unroll
                    for (int k = 1; k < kTaps; ++k) v = fma(kG[k], ring[q][(s + 1 + k) % kTaps], v);
                    m[q] = v;
                }
                const double mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
                const double vxx = m[2] - mxx, vyy = m[3] - myy, vxy = m[4] - mxy;
                const double cs = (2.0 * vxy + kC2) / (vxx + vyy + kC2);
                const double l = (2.0 * mxy + kC1) / (mxx + myy + kC1);
                if (live) {
                    sum_ssim += l * cs;
                    sum_cs += cs;
                }
            }
        }
    }
    red[0][tid] = sum_ssim;
    red[1][tid] = sum_cs;
    __syncthreads();
    if (tid < 6) {                                                   // thread 2 c + which: channel c's columns c, c + 3, ... in order
        const int c = tid >> 1, which = tid & 1;
        double acc = 0.0;
        for (int p = 0; p < kTilePix; ++p) acc += red[which][3 * p + c];
        const int64_t slot = (int64_t)blockIdx.z * slots_per_pair + (int64_t)ty * own_tx + tx;
        ws[slot * 6 + tid] = acc;
    }
}

// one wave per pair: out[pair][c][which] = (sum of the pair's tile sums, fixed order) / ((h - 10) (w - 10)); NaN for a skipped record
__global__ __launch_bounds__(64) void ssim_finish_kernel(const tise_pair_t* __restrict__ table, int max_h, int max_w,
                                                         const double* __restrict__ ws, int64_t slots_per_pair,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
    const tise_pair_t e = table[blockIdx.x];
    const int lane = threadIdx.x;
    if (!usable(e, kTaps, max_h, max_w)) {
        if (lane < 6) out[(int64_t)blockIdx.x * 6 + lane] = __builtin_nan("");
        return;
    }
    const int tiles = tiles_of(e.w) * tiles_of(e.h);
    const double count = (double)(e.h - (kTaps - 1)) * (double)(e.w - (kTaps - 1));
    const double* base = ws + (int64_t)blockIdx.x * slots_per_pair * 6;
    for (int q = 0; q < 6; ++q) {
        double acc = 0.0;
        for (int t = lane; t < tiles; t += 64) acc += base[(int64_t)t * 6 + q];
        acc = wave_sum(acc);
        if (lane == 0) out[(int64_t)blockIdx.x * 6 + q] = acc / count;
    }
}

// sum over a chunk of a pair's bytes of (x - y)^2: exact integers, so the integer atomic's order is immaterial
__global__ __launch_bounds__(256) void pair_sse_kernel(const tise_pair_t* __restrict__ table, int max_h, int max_w,
                                                       unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[4];
    const tise_pair_t e = table[blockIdx.y];
    if (!usable(e, 1, max_h, max_w)) return;
    const int64_t bytes = (int64_t)e.h * e.w * 3;
    const int64_t base = (int64_t)blockIdx.x * kSseChunk;
    if (base >= bytes) return;
    const uint8_t* x = static_cast<const uint8_t*>(e.x);
    const uint8_t* y = static_cast<const uint8_t*>(e.y);
    unsigned acc = 0;                                                // 64 terms <= 255^2 each
#pragma unroll 8
    for (int k = 0; k < kSseChunk / 256; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        if (i < bytes) {
            const int d = (int)x[i] - (int)y[i];
            acc += (unsigned)(d * d);
        }
    }
    unsigned long long v = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&out[blockIdx.y], part[0] + part[1] + part[2] + part[3]);
}

// (a + b + c + d) * 0.25 of every whole 2 x 2 block, both images of every pair; a last odd row or column is dropped
template <bool F32>
__global__ __launch_bounds__(256) void pool2x2_kernel(const tise_pair_t* __restrict__ table, const tise_pair_t* __restrict__ out_table,
                                                      int max_h, int max_w) {
#pragma clang fp contract(off)
    const tise_pair_t e = table[blockIdx.y];
    const tise_pair_t o = out_table[blockIdx.y];
    if (!usable(e, 2, max_h, max_w) || o.x == nullptr || o.y == nullptr || o.h != e.h / 2 || o.w != e.w / 2) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int orow = 3 * o.w;
    if (i >= (int64_t)o.h * orow) return;
    const int oy = (int)(i / orow);
    const int r = (int)(i - (int64_t)oy * orow);                     // 3 * ox + c
    const int ox = r / 3;
    const int64_t pitch = 3 * (int64_t)e.w;
    const int64_t s = 2 * (int64_t)oy * pitch + 3 * ox + r;          // 6 * ox + c
    const void* src = blockIdx.z ? e.y : e.x;
    float* dst = static_cast<float*>(const_cast<void*>(blockIdx.z ? o.y : o.x));
    const float a = load_value<F32>(src, s), b = load_value<F32>(src, s + 3);
    const float c = load_value<F32>(src, s + pitch), d = load_value<F32>(src, s + pitch + 3);
    dst[i] = (a + b + c + d) * 0.25f;
}

int check_common(const void* table, int64_t n, int max_h, int max_w, int min_side) {
    if (!table || n < 0 || max_h < min_side || max_w < min_side) return TISE_ERR_INVALID_ARG;
    if (max_h > kMaxSide || max_w > kMaxSide || n > kMaxPairs) return TISE_ERR_UNSUPPORTED;
    return TISE_OK;
}

}  // namespace

extern "C" int tise_ssim_workspace_bytes(int64_t n, int max_h, int max_w, size_t* bytes) {
    if (!bytes || n < 0 || max_h < kTaps || max_w < kTaps) return TISE_ERR_INVALID_ARG;
    if (max_h > kMaxSide || max_w > kMaxSide || n > kMaxPairs) return TISE_ERR_UNSUPPORTED;
    const int64_t slots = n * tiles_of(max_h) * tiles_of(max_w);
    if (slots > kMaxTiles) return TISE_ERR_UNSUPPORTED;
    *bytes = (size_t)slots * 6 * sizeof(double);
    return TISE_OK;
}

extern "C" int tise_ssim_pairs(const tise_pair_t* table_dev, int64_t n, int max_h, int max_w, int is_f32, double* out_dev,
                               void* ws_dev, size_t ws_bytes, void* stream) {
    int st = check_common(table_dev, n, max_h, max_w, kTaps);
    if (st != TISE_OK) return st;
    if (!out_dev || !ws_dev || (is_f32 != 0 && is_f32 != 1) || ((uintptr_t)out_dev & 7) || ((uintptr_t)ws_dev & 7) ||
        ((uintptr_t)table_dev & 7))
        return TISE_ERR_INVALID_ARG;
    size_t need = 0;
    st = tise_ssim_workspace_bytes(n, max_h, max_w, &need);
    if (st != TISE_OK) return st;
    if (ws_bytes < need) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    const int txs = tiles_of(max_w), tys = tiles_of(max_h);
    const int64_t slots = (int64_t)txs * tys;
    const dim3 grid((unsigned)txs, (unsigned)tys, (unsigned)n);
    hipStream_t s = (hipStream_t)stream;
    if (is_f32)
        hipLaunchKernelGGL(ssim_tile_kernel<true>, grid, dim3(kThreads), 0, s, table_dev, max_h, max_w, (double*)ws_dev, slots);
    else
        hipLaunchKernelGGL(ssim_tile_kernel<false>, grid, dim3(kThreads), 0, s, table_dev, max_h, max_w, (double*)ws_dev, slots);
    TISE_LAUNCH_CHECK();
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)n), dim3(64), 0, s, table_dev, max_h, max_w, (const double*)ws_dev, slots,
                       out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

extern "C" int tise_pair_sse_u8(const tise_pair_t* table_dev, int64_t n, int max_h, int max_w, uint64_t* out_dev, void* stream) {
    int st = check_common(table_dev, n, max_h, max_w, 1);
    if (st != TISE_OK) return st;
    if (!out_dev || ((uintptr_t)out_dev & 7) || ((uintptr_t)table_dev & 7)) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    hipStream_t s = (hipStream_t)stream;
    TISE_HIP_CHECK(hipMemsetAsync(out_dev, 0, (size_t)n * sizeof(uint64_t), s));
    const int64_t chunks = ceil_div64((int64_t)max_h * max_w * 3, kSseChunk);
    hipLaunchKernelGGL(pair_sse_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, s, table_dev, max_h, max_w,
                       (unsigned long long*)out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

extern "C" int tise_pool2x2_pairs(const tise_pair_t* table_dev, const tise_pair_t* out_table_dev, int64_t n, int max_h, int max_w,
                                  int is_f32, void* stream) {
    int st = check_common(table_dev, n, max_h, max_w, 2);
    if (st != TISE_OK) return st;
    if (!out_table_dev || (is_f32 != 0 && is_f32 != 1) || ((uintptr_t)table_dev & 7) || ((uintptr_t)out_table_dev & 7))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    const int64_t blocks = ceil_div64((int64_t)(max_h / 2) * (max_w / 2) * 3, 256);
    const dim3 grid((unsigned)blocks, (unsigned)n, 2);
    hipStream_t s = (hipStream_t)stream;
    if (is_f32)
        hipLaunchKernelGGL(pool2x2_kernel<true>, grid, dim3(256), 0, s, table_dev, out_table_dev, max_h, max_w);
    else
        hipLaunchKernelGGL(pool2x2_kernel<false>, grid, dim3(256), 0, s, table_dev, out_table_dev, max_h, max_w);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}
