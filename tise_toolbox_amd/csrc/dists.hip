// DISTS of image PAIRS around the split-precision convolutions (tise_toolbox_amd/dists_hip.py): the L2 (Hanning) pool between
// VGG's blocks, the per-stage moment head and the exact integer sums of stage 0.  No counterpart in the reference toolbox; the
// definition is restated from Ding, Ma, Wang & Simoncelli 2020 in include/tise_hip.h, and tise_toolbox_amd/dists_model.py is the
// plain torch module the whole route is compared against.  The network input is lpips.hip's tise_lpips_input_split with DISTS's
// table, the thirteen convolutions are conv_split.hip's.
//
// l2pool3s2_split_kernel.  y = sqrt(sum_taps g (hi + lo 2^-11)^2 + 1e-12), g = [[1,2,1],[2,4,2],[1,2,1]] / 16, stride 2, zero
// padding 1: the output is ceil(H/2) x ceil(W/2).  thread = (pooled pixel, 8 channels) as in maxpool2s2_split_kernel, so a pixel's
// row is read as whole 16-byte pieces.  A value is formed in fp64 (exact), its square is exact (at most 48 significant bits), the
// weights are powers of two; the nine terms are added in row-major tap order (a tap outside the image is skipped: it would add
// +0.0), then + 1e-12, the fp64 square root, ONE rounding to fp32, and the split of conv_split.split.
//
// tise_dists_layer: four launches for one stage (2n, h, w, C).  A workgroup of 256 threads owns kWgPix consecutive pixels of ONE
// pair (the cut depends on h w only, not on n).  With G8 = C / 8 lanes across a pixel's channels (a lane owns 8 channels: two
// 16-byte loads per side) and P = 256 / G8 pixel slots, slot g adds the pixels q0 + g, q0 + g + P, .. in order; the P slots of a
// channel are then added in order through LDS, and the workgroup's partial goes to its own place in the workspace.
//   dists_sum_kernel     per side and channel: sum of the values, and the COUNT of pixels that differ from the image's first pixel.
//   dists_mean_kernel    adds a pair's partials in slot order; mean = the first pixel's value if no pixel differs from it (a
//                        constant channel's mean is exact, so its variance and covariance terms below are exactly 0), else sum / hw.
//   dists_center_kernel  sum (x - mx)^2, sum (y - my)^2, sum (x - mx)(y - my): the centered second moments, second read of the stage.
//   dists_finish_kernel  one workgroup per pair: per channel the partials in slot order, S1 = (2 mx my + c1) / (mx^2 + my^2 + c1),
//                        S2 = (2 cxy + c2) / (vx + vy + c2), t_c = alpha_c (1 - S1) + beta_c (1 - S2); thread t adds t_c of channels
//                        t and t + 256, then the butterfly, the four waves in order, and out[pair] += the sum.
// Everything after the exact hi + lo 2^-11 is fp64 with contraction off, in a fixed order, no floating-point atomics.  An identical
// pair runs the same operations on the same bits on both sides: mx == my gives 2 mx my == mx^2 + my^2 bit for bit, cxy == vx == vy
// gives 2 cxy == vx + vy, so S1 = S2 = 1 and the pair adds exactly 0.0; a channel that is zero on both sides gives c / c = 1 twice.
// A NaN or an inf stays in its pair's partials.
//
// dists_image_sums_kernel.  Stage 0 on the bytes: per pair and colour the five integer sums of bx, by, bx^2, by^2, bx by (a thread
// adds at most 16 pixels in 32 bits, then 64-bit butterflies and one integer atomic per workgroup and sum: exact, order-free).
//
// Range guard (csrc/common.h): the pool's weights are non-negative and sum to 1, so its output never exceeds the largest stored
// input magnitude (plus 1e-6) -- the guard cannot fire here and this file keeps no flag word; the convolutions keep theirs.
#include <math.h>
#include "common.h"
#include "split_px.h"

namespace {

constexpr int kMaxSide = TISE_DISTS_MAX_SIDE;
constexpr int64_t kMaxPairs = TISE_DISTS_MAX_PAIRS;
constexpr int kWgPix = TISE_DISTS_WG_PIXELS;           // pixels of one pair that one workgroup of the head sums
constexpr int kMaxC = TISE_DISTS_MAX_CHANNELS;         // two channels per thread of the finish kernel
constexpr int kSumPix = TISE_DISTS_SUM_PIXELS;         // pixels of one pair per workgroup of the stage-0 sums
constexpr double kC1 = 1e-6, kC2 = 1e-6;

__global__ __launch_bounds__(256) void l2pool3s2_split_kernel(const _Float16* __restrict__ x, int x_C, int x_off,
                                                              int N, int H, int W, int C8,
                                                              _Float16* __restrict__ out, int out_C, int out_off) {
#pragma clang fp contract(off)
    const SplitPoolThread t = split_pool_thread((H + 1) / 2, (W + 1) / 2, C8, x_C, x_off);
    if (!t.live) return;
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0;
#pragma unroll
    for (int dh = 0; dh < 3; ++dh)
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
            const int ih = 2 * t.oh - 1 + dh, iw = 2 * t.ow - 1 + dw;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;            // zero padding: the tap contributes 0
            const double g = (dh == 1 ? 0.5 : 0.25) * (dw == 1 ? 0.5 : 0.25);
            double v[8];
            split_load8_f64(x + ((t.n * H + ih) * W + iw) * t.x_px + t.xo, t.xs, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += g * (v[i] * v[i]);
        }
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)sqrt(acc[i] + 1e-12);
    t.store8(f, out, out_C, out_off);
}

// Adds the 8 values of every thread over the P pixel slots of a chunk, slot 0 first, and writes the C sums to dst[0..C).
// red: 256 * 8 doubles of LDS.  Called by all 256 threads; ends with a barrier, so it can be called again at once.
__device__ __forceinline__ void slot_sum(const double v[8], bool active, double* red, int C, int G8, int P, double* __restrict__ dst) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[tid * 8 + i] = v[i];
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const int j = c >> 3, i = c & 7;
        double s = 0.0;
        for (int g = 0; g < P; ++g) s += red[(g * G8 + j) * 8 + i];
        dst[c] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void dists_sum_kernel(const _Float16* __restrict__ feat, int n, int64_t hw, int C,
                                                        double* __restrict__ part, int64_t slots) {
#pragma clang fp contract(off)
    __shared__ double red[256 * 8];
    const int tid = threadIdx.x;
    const int G8 = C / 8, P = 256 / G8;
    const int j = tid % G8, g = tid / G8;
    const bool active = g < P;
    const int64_t pair = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * kWgPix;
    const int64_t q1 = min(q0 + (int64_t)kWgPix, hw);
    double* dst = part + (pair * slots + blockIdx.x) * 4 * (int64_t)C;
    for (int side = 0; side < 2; ++side) {
        const _Float16* f = feat + ((int64_t)side * n + pair) * hw * (2 * (int64_t)C);
        double p[8], sum[8], nd[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = sum[i] = nd[i] = 0.0;
        if (active) {
            split_chunk_f64(f, C, j, p);                                      // the image's first pixel
            for (int64_t q = q0 + g; q < q1; q += P) {
                double v[8];
                split_chunk_f64(f + q * (2 * (int64_t)C), C, j, v);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    sum[i] += v[i];
                    nd[i] += v[i] != p[i] ? 1.0 : 0.0;                   // (a NaN differs from everything)
                }
            }
        }
        slot_sum(sum, active, red, C, G8, P, dst + (2 * side) * (int64_t)C);
        slot_sum(nd, active, red, C, G8, P, dst + (2 * side + 1) * (int64_t)C);
    }
}

__global__ __launch_bounds__(256) void dists_mean_kernel(const _Float16* __restrict__ feat, int n, int64_t hw, int C,
                                                         const double* __restrict__ part, int64_t slots, double* __restrict__ mean) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * C) return;
    const int side = e / C, c = e - side * C;
    const int64_t pair = blockIdx.y;
    const double* base = part + pair * slots * 4 * (int64_t)C + (2 * side) * (int64_t)C + c;
    double s = 0.0, nd = 0.0;
    for (int64_t t = 0; t < slots; ++t) {
        s += base[t * 4 * (int64_t)C];
        nd += base[t * 4 * (int64_t)C + C];
    }
    const _Float16* f = feat + ((int64_t)side * n + pair) * hw * (2 * (int64_t)C) + tise_ilv_off(c, C);
    const double p = (double)(float)f[0] + (double)(float)f[tise_ilv_second(c, C)] * (1.0 / 2048.0);
    mean[pair * 2 * (int64_t)C + e] = nd == 0.0 ? p : s / (double)hw;
}

__global__ __launch_bounds__(256) void dists_center_kernel(const _Float16* __restrict__ feat, int n, int64_t hw, int C,
                                                           const double* __restrict__ mean, double* __restrict__ part,
                                                           int64_t slots) {
#pragma clang fp contract(off)
    __shared__ double red[256 * 8];
    const int tid = threadIdx.x;
    const int G8 = C / 8, P = 256 / G8;
    const int j = tid % G8, g = tid / G8;
    const bool active = g < P;
    const int64_t pair = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * kWgPix;
    const int64_t q1 = min(q0 + (int64_t)kWgPix, hw);
    const _Float16* fa = feat + pair * hw * (2 * (int64_t)C);
    const _Float16* fb = feat + ((int64_t)n + pair) * hw * (2 * (int64_t)C);
    double* dst = part + (pair * slots + blockIdx.x) * 3 * (int64_t)C;
    double mx[8], my[8], sxx[8], syy[8], sxy[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) mx[i] = my[i] = sxx[i] = syy[i] = sxy[i] = 0.0;
    if (active) {
        const double* m = mean + pair * 2 * (int64_t)C + 8 * j;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            mx[i] = m[i];
            my[i] = m[C + i];
        }
        for (int64_t q = q0 + g; q < q1; q += P) {
            double a[8], b[8];
            split_chunk_f64(fa + q * (2 * (int64_t)C), C, j, a);
            split_chunk_f64(fb + q * (2 * (int64_t)C), C, j, b);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double dx = a[i] - mx[i], dy = b[i] - my[i];
                sxx[i] += dx * dx;
                syy[i] += dy * dy;
                sxy[i] += dx * dy;
            }
        }
    }
    slot_sum(sxx, active, red, C, G8, P, dst);
    slot_sum(syy, active, red, C, G8, P, dst + C);
    slot_sum(sxy, active, red, C, G8, P, dst + 2 * (int64_t)C);
}

__global__ __launch_bounds__(256) void dists_finish_kernel(const double* __restrict__ part, int64_t slots, int64_t hw, int C,
                                                           const double* __restrict__ mean, const double* __restrict__ alpha,
                                                           const double* __restrict__ beta, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pair = blockIdx.x;
    const double n = (double)hw;
    double acc = 0.0;
    for (int c = tid; c < C; c += 256) {
        const double* base = part + pair * slots * 3 * (int64_t)C + c;
        double sxx = 0.0, syy = 0.0, sxy = 0.0;
        for (int64_t t = 0; t < slots; ++t) {
            sxx += base[t * 3 * (int64_t)C];
            syy += base[t * 3 * (int64_t)C + C];
            sxy += base[t * 3 * (int64_t)C + 2 * (int64_t)C];
        }
        const double mx = mean[pair * 2 * (int64_t)C + c], my = mean[pair * 2 * (int64_t)C + C + c];
        const double vx = sxx / n, vy = syy / n, cxy = sxy / n;
        const double s1 = (2.0 * mx * my + kC1) / (mx * mx + my * my + kC1);
        const double s2 = (2.0 * cxy + kC2) / (vx + vy + kC2);
        acc += alpha[c] * (1.0 - s1) + beta[c] * (1.0 - s2);
    }
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) out[pair] += ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void dists_image_sums_kernel(const tise_pair_t* __restrict__ table, int H, int W,
                                                               unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[4][15];
    const tise_pair_t rec = table[blockIdx.y];
    if (rec.x == nullptr || rec.y == nullptr || rec.h != H || rec.w != W) return;      // a record of another size: its sums stay 0
    const int64_t npix = (int64_t)H * W;
    const int64_t base = (int64_t)blockIdx.x * kSumPix;
    const uint8_t* x = static_cast<const uint8_t*>(rec.x);
    const uint8_t* y = static_cast<const uint8_t*>(rec.y);
    unsigned acc[15];                                                  // 16 terms <= 255^2 each
#pragma unroll
    for (int k = 0; k < 15; ++k) acc[k] = 0u;
#pragma unroll 4
    for (int k = 0; k < kSumPix / 256; ++k) {
        const int64_t q = base + k * 256 + threadIdx.x;
        if (q < npix) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned bx = x[q * 3 + c], by = y[q * 3 + c];
                acc[5 * c + 0] += bx;
                acc[5 * c + 1] += by;
                acc[5 * c + 2] += bx * bx;
                acc[5 * c + 3] += by * by;
                acc[5 * c + 4] += bx * by;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 15; ++k) {
        unsigned long long v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 15) {
        const int k = threadIdx.x;
        atomicAdd(&out[(int64_t)blockIdx.y * 15 + k], part[0][k] + part[1][k] + part[2][k] + part[3][k]);
    }
}

}  // namespace

extern "C" int tise_l2pool3s2_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C, void* out_dev,
                                         int64_t out_ld, int out_off, void* stream) {
    if (!split_pool_args_ok(x_dev, x_ld, x_off, n, h, w, 1, C, out_dev, out_ld, out_off)) return TISE_ERR_INVALID_ARG;
    const int oh = (int)(((int64_t)h + 1) / 2), ow = (int)(((int64_t)w + 1) / 2);
    return split_pool_launch(l2pool3s2_split_kernel, oh, ow, x_dev, x_ld, x_off, n, h, w, C, out_dev, out_ld, out_off, stream);
}

extern "C" int tise_dists_workspace_bytes(int64_t n, int h, int w, int C, size_t* bytes) {
    if (!bytes || C < 16 || C % 16) return TISE_ERR_INVALID_ARG;
    const int st = check_sizes(n, h, w, kMaxSide, kMaxPairs);
    if (st != TISE_OK) return st;
    if (C > kMaxC) return TISE_ERR_UNSUPPORTED;
    const int64_t slots = ceil_div64((int64_t)h * w, kWgPix);
    *bytes = (size_t)(n * C * (7 * slots + 2)) * sizeof(double);
    return TISE_OK;
}

extern "C" int tise_dists_layer(const void* feat_dev, int64_t n, int h, int w, int C, const double* alpha_dev, const double* beta_dev,
                                double* out_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    if (!feat_dev || !alpha_dev || !beta_dev || !out_dev || !ws_dev || C < 16 || C % 16 || ((uintptr_t)feat_dev & 15) ||
        ((uintptr_t)alpha_dev & 7) || ((uintptr_t)beta_dev & 7) || ((uintptr_t)out_dev & 7) || ((uintptr_t)ws_dev & 7))
        return TISE_ERR_INVALID_ARG;
    size_t need = 0;
    const int st = tise_dists_workspace_bytes(n, h, w, C, &need);
    if (st != TISE_OK) return st;
    if (ws_bytes < need) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    const int64_t hw = (int64_t)h * w;
    const int64_t slots = ceil_div64(hw, kWgPix);
    double* part1 = (double*)ws_dev;                                   // (n, slots, {sum x, differ x, sum y, differ y}, C)
    double* mean = part1 + n * slots * 4 * C;                          // (n, {x, y}, C)
    double* part2 = mean + n * 2 * C;                                  // (n, slots, {xx, yy, xy}, C)
    const _Float16* feat = reinterpret_cast<const _Float16*>(feat_dev);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)slots, (unsigned)n);
    hipLaunchKernelGGL(dists_sum_kernel, grid, dim3(256), 0, s, feat, (int)n, hw, C, part1, slots);
    TISE_LAUNCH_CHECK();
    hipLaunchKernelGGL(dists_mean_kernel, dim3((unsigned)ceil_div(2 * C, 256), (unsigned)n), dim3(256), 0, s, feat, (int)n, hw, C,
                       (const double*)part1, slots, mean);
    TISE_LAUNCH_CHECK();
    hipLaunchKernelGGL(dists_center_kernel, grid, dim3(256), 0, s, feat, (int)n, hw, C, (const double*)mean, part2, slots);
    TISE_LAUNCH_CHECK();
    hipLaunchKernelGGL(dists_finish_kernel, dim3((unsigned)n), dim3(256), 0, s, (const double*)part2, slots, hw, C, (const double*)mean,
                       alpha_dev, beta_dev, out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

extern "C" int tise_dists_image_sums_u8(const tise_pair_t* table_dev, int64_t n, int h, int w, int64_t* out_dev, void* stream) {
    if (!table_dev || !out_dev || ((uintptr_t)table_dev & 7) || ((uintptr_t)out_dev & 7)) return TISE_ERR_INVALID_ARG;
    const int st = check_sizes(n, h, w, kMaxSide, kMaxPairs);
    if (st != TISE_OK) return st;
    if (n == 0) return TISE_OK;
    hipStream_t s = (hipStream_t)stream;
    TISE_HIP_CHECK(hipMemsetAsync(out_dev, 0, (size_t)n * 15 * sizeof(int64_t), s));
    const int64_t chunks = ceil_div64((int64_t)h * w, kSumPix);
    hipLaunchKernelGGL(dists_image_sums_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, s, table_dev, h, w,
                       (unsigned long long*)out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}
