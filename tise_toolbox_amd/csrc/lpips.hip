// LPIPS (VGG-16) of image PAIRS around the split-precision convolutions (tise_toolbox_amd/lpips_hip.py): the network input, the
// 2 x 2 max-pool between VGG's blocks and the per-tap distance head.  No counterpart in the reference toolbox; the definition is
// restated from Zhang, Isola, Efros, Shechtman & Wang 2018 in include/tise_hip.h, and tise_toolbox_amd/lpips_model.py is the
// plain torch module the whole route is compared against.  The thirteen convolutions themselves are conv_split.hip's.
//
// lpips_input_kernel.  Bytes -> the split tensor conv1_1 reads.  A pixel of the destination is ONE 128-byte line
// [hi c0..c31 | lo c0..c31] (csrc/common.h); eight threads write its eight 16-byte chunks, so a wave stores eight whole lines.
// Only chunk 0 (hi of channels 0..7) and chunk 4 (their lo) carry values: channels 0..2 are table[c][byte], split as
// conv_split.split does (hi = fp16(v), lo = fp16((v - hi) 2^11)); everything else is zero in both halves, so conv1_1 runs as a
// 32-channel layer whose weight columns 3..31 are zero.  The source is read byte by byte: an image may start at any address.
//
// maxpool2s2_split_kernel.  maxpool3s2_split_kernel's (trunk_ops.hip) value arithmetic on a 2 x 2 / stride 2 window: the maximum
// of the exact fp32 values hi + lo 2^-11, split again; thread = (pooled pixel, 8 channels), a last odd row or column is dropped.
//
// lpips_head_kernel.  One tap (2n, h, w, C) -> per pair the SUM over the pixels of d = sum_c w_c (a_c / n(a) - b_c / n(b))^2,
// n(v) = sqrt(sum_c v_c^2) + 1e-10.  A value is hi + lo 2^-11, formed in fp64 (exact); everything after it is fp64 in a fixed
// order.  A lane owns 8 channels of a pixel (two 16-byte loads per side: the hi and the lo chunk of one line), G = the power of
// two >= C / 8 (at most 64) neighbouring lanes own one pixel -- together they read that pixel's 128-byte lines -- and a wave
// works on 64 / G pixels at once, so the widest tap (64 channels, half of all the bytes) keeps every lane busy; C <= 512 = one
// chunk per lane of a wave, kept in registers between the two passes (VGG's widest tap; more is refused).  The two channel sums are
// fma chains over a lane's channels in order and then the xor butterfly over the G lanes, which leaves the SAME bits in every
// lane of the group; an identical pair therefore has n(a) == n(b) and a_c / n(a) == b_c / n(b): d is exactly 0.  A pixel that is
// zero on both sides gives 0 / 1e-10 - 0 / 1e-10 = 0.  A workgroup of 256 threads owns kHeadPix consecutive pixels of ONE pair
// (the cut depends on h w only, not on n), a group adds its pixels in order, the leaders of a wave are added by the butterfly,
// the four waves in order, and the sum goes to the workspace slot of (pair, workgroup).  lpips_finish_kernel (one wave per pair)
// adds a pair's slots -- lane l the slots l, l + 64, ... in order, then the butterfly -- divides by h w and ADDS the tap's value
// to out[pair].  No floating-point atomics; a NaN or an inf in a pair's features stays in that pair's slots.
//
// Range guard (csrc/common.h): neither writer of split tensors here can leave the fp16 range -- the input kernel converts values
// of a table the host has checked (finite, |v| <= 65504; lpips_hip.py), the pool stores maxima of values that are stored already
// -- so this file keeps no flag word; the convolutions between them keep theirs.
#include <math.h>
#include "common.h"
#include "split_px.h"

namespace {

constexpr int kMaxSide = TISE_LPIPS_MAX_SIDE;
constexpr int64_t kMaxPairs = TISE_LPIPS_MAX_PAIRS;
constexpr int kHeadPix = TISE_LPIPS_WG_PIXELS;         // pixels of one pair that one workgroup of the head sums
constexpr int kMaxC = TISE_LPIPS_MAX_CHANNELS;         // one 8-channel chunk per lane of a wave

__global__ __launch_bounds__(256) void lpips_input_kernel(const tise_pair_t* __restrict__ table, int n, int H, int W,
                                                          const float* __restrict__ lut, _Float16* __restrict__ out) {
    const unsigned per_img = (unsigned)H * (unsigned)W * 8u;                 // <= 2^31
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= per_img) return;
    const unsigned pix = e >> 3;
    const int chunk = (int)(e & 7u);
    const int img = blockIdx.y;
    const tise_pair_t rec = table[img < n ? img : img - n];
    const uint8_t* src = static_cast<const uint8_t*>(img < n ? rec.x : rec.y);
    half8v v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (_Float16)0.0f;
    if ((chunk & 3) == 0 && src != nullptr && rec.h == H && rec.w == W) {    // a record of another size is written as zeros
        const uint8_t* q = src + (int64_t)pix * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = lut[c * 256 + q[c]];
            const _Float16 hi = (_Float16)f;
            v[c] = chunk == 0 ? hi : (_Float16)((f - (float)hi) * 2048.f);
        }
    }
    *reinterpret_cast<half8v*>(out + ((int64_t)img * H * W + pix) * 64 + chunk * 8) = v;
}

__global__ __launch_bounds__(256) void maxpool2s2_split_kernel(const _Float16* __restrict__ x, int x_C, int x_off,
                                                               int N, int H, int W, int C8,
                                                               _Float16* __restrict__ out, int out_C, int out_off) {
    const SplitPoolThread t = split_pool_thread(H / 2, W / 2, C8, x_C, x_off);
    if (!t.live) return;
    float bv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bv[i] = -INFINITY;
#pragma unroll
    for (int dh = 0; dh < 2; ++dh)
#pragma unroll
        for (int dw = 0; dw < 2; ++dw) {
            float v[8];
            split_load8_f32(x + ((t.n * H + 2 * t.oh + dh) * W + 2 * t.ow + dw) * t.x_px + t.xo, t.xs, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) bv[i] = fmaxf(bv[i], v[i]);
        }
    t.store8(bv, out, out_C, out_off);
}

// sum over the G lanes of a group (G a power of two, groups aligned): the same bits in every lane of the group
__device__ __forceinline__ double group_sum(double v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void lpips_head_kernel(const _Float16* __restrict__ feat, int n, int64_t hw, int C, int G,
                                                         const float* __restrict__ wlin, double* __restrict__ ws, int64_t slots) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = 64 / G;                                            // pixels a wave works on at once
    const int j = lane & (G - 1), g = lane / G;
    const bool has_chunk = j < C / 8;                                // C / 8 = 6 (C = 48): two lanes of a group of 8 idle
    const int64_t pair = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * kHeadPix;
    const int64_t q1 = min(q0 + (int64_t)kHeadPix, hw);
    const _Float16* fa = feat + pair * hw * (2 * (int64_t)C);
    const _Float16* fb = feat + ((int64_t)n + pair) * hw * (2 * (int64_t)C);
    double w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = has_chunk ? (double)wlin[8 * j + i] : 0.0;
    double acc = 0.0;
    for (int64_t q = q0 + wave * P + g; q < q0 + kHeadPix; q += 4 * P) {     // the same trip count in every lane of the workgroup
        const bool live = q < q1;
        double a[8], b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = b[i] = 0.0;
        if (live && has_chunk) {
            split_chunk_f64(fa + q * (2 * (int64_t)C), C, j, a);
            split_chunk_f64(fb + q * (2 * (int64_t)C), C, j, b);
        }
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sa = fma(a[i], a[i], sa);
            sb = fma(b[i], b[i], sb);
        }
        const double na = sqrt(group_sum(sa, G)) + 1e-10, nb = sqrt(group_sum(sb, G)) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double t = a[i] / na - b[i] / nb;
            d = fma(w[i], t * t, d);
        }
        d = group_sum(d, G);
        if (live) acc += d;
    }
    acc = wave_sum(j == 0 ? acc : 0.0);                              // the leaders of the wave's groups
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) ws[pair * slots + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ ws, int64_t slots, int64_t hw,
                                                          double* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const double* base = ws + (int64_t)blockIdx.x * slots;
    double acc = 0.0;
    for (int64_t t = lane; t < slots; t += 64) acc += base[t];
    acc = wave_sum(acc);
    if (lane == 0) out[blockIdx.x] += acc / (double)hw;
}

}  // namespace

extern "C" int tise_lpips_input_split(const tise_pair_t* table_dev, int64_t n, int h, int w, const float* lut_dev, void* out_dev,
                                      void* stream) {
    if (!table_dev || !lut_dev || !out_dev || ((uintptr_t)table_dev & 7) || ((uintptr_t)lut_dev & 3) || ((uintptr_t)out_dev & 15))
        return TISE_ERR_INVALID_ARG;
    const int st = check_sizes(n, h, w, kMaxSide, kMaxPairs);
    if (st != TISE_OK) return st;
    if (n == 0) return TISE_OK;
    const int64_t blocks = ceil_div64((int64_t)h * w * 8, 256);
    hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)blocks, (unsigned)(2 * n)), dim3(256), 0, (hipStream_t)stream, table_dev,
                       (int)n, h, w, lut_dev, reinterpret_cast<_Float16*>(out_dev));
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

extern "C" int tise_maxpool2s2_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C, void* out_dev,
                                          int64_t out_ld, int out_off, void* stream) {
    if (!split_pool_args_ok(x_dev, x_ld, x_off, n, h, w, 2, C, out_dev, out_ld, out_off)) return TISE_ERR_INVALID_ARG;
    return split_pool_launch(maxpool2s2_split_kernel, h / 2, w / 2, x_dev, x_ld, x_off, n, h, w, C, out_dev, out_ld, out_off, stream);
}

extern "C" int tise_lpips_workspace_bytes(int64_t n, int h, int w, size_t* bytes) {
    if (!bytes) return TISE_ERR_INVALID_ARG;
    const int st = check_sizes(n, h, w, kMaxSide, kMaxPairs);
    if (st != TISE_OK) return st;
    *bytes = (size_t)(n * ceil_div64((int64_t)h * w, kHeadPix)) * sizeof(double);
    return TISE_OK;
}

extern "C" int tise_lpips_layer(const void* feat_dev, int64_t n, int h, int w, int C, const float* w_dev, double* out_dev,
                                void* ws_dev, size_t ws_bytes, void* stream) {
    if (!feat_dev || !w_dev || !out_dev || !ws_dev || C < 16 || C % 16 || ((uintptr_t)feat_dev & 15) || ((uintptr_t)w_dev & 3) ||
        ((uintptr_t)out_dev & 7) || ((uintptr_t)ws_dev & 7))
        return TISE_ERR_INVALID_ARG;
    size_t need = 0;
    const int st = tise_lpips_workspace_bytes(n, h, w, &need);
    if (st != TISE_OK) return st;
    if (C > kMaxC) return TISE_ERR_UNSUPPORTED;
    if (ws_bytes < need) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    const int64_t hw = (int64_t)h * w;
    const int64_t slots = ceil_div64(hw, kHeadPix);
    int G = 2;
    while (G < 64 && G < C / 8) G <<= 1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)slots, (unsigned)n);
    hipLaunchKernelGGL(lpips_head_kernel, grid, dim3(256), 0, s, reinterpret_cast<const _Float16*>(feat_dev), (int)n, hw, C, G, w_dev,
                       (double*)ws_dev, slots);
    TISE_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)n), dim3(64), 0, s, (const double*)ws_dev, slots, hw, out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}
