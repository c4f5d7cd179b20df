// What a ResNet needs around the split-precision convolutions (tise_toolbox_amd/resnet_hip.py; tise_toolbox_amd/resnet_model.py is
// the plain torch module the whole route is compared against).  No counterpart in the reference toolbox, which has no ResNet.
//
// resnet_input_kernel.  Bytes -> the 32-channel split tensor the stem reads when it runs as a 32-channel SplitConv (route "padded"
// of resnet_hip.py): lpips.hip's lpips_input_kernel on ONE contiguous (n, h, w, 3) batch.  A pixel of the destination is one
// 128-byte line; eight threads write its eight 16-byte chunks; chunk 0 carries hi of channels 0..2 = table[c][byte], chunk 4 their
// lo, everything else is zero.  The source is read byte by byte: a batch may start at any address.
//
// maxpool3s2p1_split_kernel.  3 x 3 / stride 2 / padding 1 max-pool, padding ignored (a tap outside the map is skipped, i.e. -inf;
// the centre tap always lies inside): maxpool3s2_split_kernel's (trunk_ops.hip) value arithmetic -- the maximum of the exact fp32
// values hi + lo 2^-11, split again -- on split_px.h's thread map, (pooled pixel, 8 channels) per thread.  It stores maxima of
// values that are stored already, so it cannot leave the fp16 range and raises no guard.
//
// residual_relu_split_kernel.  The end of a bottleneck block: out = split(max((raw + bias) + identity, 0)).  raw is conv3's fp32
// result (scale * conv, tise_conv_split_f16 mode 1), the identity either a split tensor (u = hi + lo 2^-11, exact) or the
// downsample convolution's fp32 result with its own bias (u = id_raw + id_bias).  Three fp32 additions in that order, contraction
// off.  thread = (pixel, 8 channels): two 16-byte loads of raw, two of the identity, two 16-byte stores -- 12 C bytes per pixel
// and nothing else, so the kernel is a copy with arithmetic; its rate is the memory system's.
// Range guard (csrc/common.h): raised where v is NaN or |v| > 65504, tested on v itself BEFORE the max, so a NaN or a -inf cannot
// leave as 0 unseen.  One atomicOr per thread that saw one; no floating-point atomics.
#include <math.h>
#include "common.h"
#include "split_px.h"

namespace {

__global__ __launch_bounds__(256) void resnet_input_kernel(const uint8_t* __restrict__ x, int H, int W, const float* __restrict__ lut,
                                                           _Float16* __restrict__ out) {
    const unsigned per_img = (unsigned)H * (unsigned)W * 8u;                 // <= 2^31 (checked by the entry point)
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= per_img) return;
    const unsigned pix = e >> 3;
    const int chunk = (int)(e & 7u);
    const int64_t p = (int64_t)blockIdx.y * H * W + pix;
    half8v v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (_Float16)0.0f;
    if ((chunk & 3) == 0) {
        const uint8_t* q = x + p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = lut[c * 256 + q[c]];
            const _Float16 hi = (_Float16)f;
            v[c] = chunk == 0 ? hi : (_Float16)((f - (float)hi) * 2048.f);
        }
    }
    *reinterpret_cast<half8v*>(out + p * 64 + chunk * 8) = v;
}

__global__ __launch_bounds__(256) void maxpool3s2p1_split_kernel(const _Float16* __restrict__ x, int x_C, int x_off,
                                                                 int N, int H, int W, int C8,
                                                                 _Float16* __restrict__ out, int out_C, int out_off) {
    const SplitPoolThread t = split_pool_thread((H - 1) / 2 + 1, (W - 1) / 2 + 1, C8, x_C, x_off);
    if (!t.live) return;
    float bv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bv[i] = -INFINITY;
#pragma unroll
    for (int dh = 0; dh < 3; ++dh)
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
            const int ih = 2 * t.oh - 1 + dh, iw = 2 * t.ow - 1 + dw;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;            // padding: the tap does not take part
            float v[8];
            split_load8_f32(x + ((t.n * H + ih) * W + iw) * t.x_px + t.xo, t.xs, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) bv[i] = fmaxf(bv[i], v[i]);
        }
    t.store8(bv, out, out_C, out_off);
}

template <bool ID_SPLIT>
__global__ __launch_bounds__(256) void residual_relu_split_kernel(const float* __restrict__ raw, int64_t raw_ld, int raw_off,
                                                                  const float* __restrict__ bias,
                                                                  const _Float16* __restrict__ id_split, int id_C, int id_off,
                                                                  const float* __restrict__ id_raw, int64_t id_raw_ld, int id_raw_off,
                                                                  const float* __restrict__ id_bias, int64_t total, int C8,
                                                                  _Float16* __restrict__ out, int out_C, int out_off) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t p = e / C8;
    const int c = 8 * (int)(e - p * C8);
    float t[8], u[8];
    {
        const float* q = raw + p * raw_ld + raw_off + c;
        const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
        const float4 ba = *reinterpret_cast<const float4*>(bias + c), bb = *reinterpret_cast<const float4*>(bias + c + 4);
        t[0] = a.x + ba.x; t[1] = a.y + ba.y; t[2] = a.z + ba.z; t[3] = a.w + ba.w;
        t[4] = b.x + bb.x; t[5] = b.y + bb.y; t[6] = b.z + bb.z; t[7] = b.w + bb.w;
    }
    if (ID_SPLIT) {
        const int ch = id_off + c;
        split_load8_f32(id_split + p * (2 * (int64_t)id_C) + tise_ilv_off(ch, id_C), tise_ilv_second(ch, id_C), u);
    } else {
        const float* q = id_raw + p * id_raw_ld + id_raw_off + c;
        const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
        const float4 ba = *reinterpret_cast<const float4*>(id_bias + c), bb = *reinterpret_cast<const float4*>(id_bias + c + 4);
        u[0] = a.x + ba.x; u[1] = a.y + ba.y; u[2] = a.z + ba.z; u[3] = a.w + ba.w;
        u[4] = b.x + bb.x; u[5] = b.y + bb.y; u[6] = b.z + bb.z; u[7] = b.w + bb.w;
    }
    bool bad = false;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float s = t[i] + u[i];
        bad |= !(fabsf(s) <= TISE_F16_MAX);                                  // a NaN fails the comparison too
        v[i] = fmaxf(s, 0.f);
    }
    const int ch = out_off + c;
    split_store8(v, out + p * (2 * (int64_t)out_C) + tise_ilv_off(ch, out_C), tise_ilv_second(ch, out_C));
    if (bad) tise_flag_split_overflow(INFINITY);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int tise_resnet_input_split(const uint8_t* x_dev, const float* lut_dev, int n, int h, int w, void* out_dev, void* stream) {
    if (!x_dev || !lut_dev || !out_dev || n < 0 || h < 1 || w < 1 || ((uintptr_t)lut_dev & 3) || !aligned16(out_dev))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if (n > 65535 || (int64_t)h * w > (1LL << 27)) return TISE_ERR_UNSUPPORTED;
    const int64_t blocks = ceil_div64((int64_t)h * w * 8, 256);
    hipLaunchKernelGGL(resnet_input_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, x_dev, h, w, lut_dev,
                       reinterpret_cast<_Float16*>(out_dev));
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

extern "C" int tise_maxpool3s2p1_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C, void* out_dev,
                                            int64_t out_ld, int out_off, void* stream) {
    if (!split_pool_args_ok(x_dev, x_ld, x_off, n, h, w, 1, C, out_dev, out_ld, out_off) || x_dev == out_dev) return TISE_ERR_INVALID_ARG;
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    return split_pool_launch(maxpool3s2p1_split_kernel, oh, ow, x_dev, x_ld, x_off, n, h, w, C, out_dev, out_ld, out_off, stream);
}

extern "C" int tise_residual_relu_split_nhwc(const float* raw_dev, int64_t raw_ld, int raw_off, const float* bias_dev,
                                             const void* id_split_dev, int64_t id_ld, int id_off, const float* id_raw_dev,
                                             int64_t id_raw_ld, int id_raw_off, const float* id_bias_dev, int64_t pixels, int C,
                                             void* out_dev, int64_t out_ld, int out_off, void* stream) {
    if (!raw_dev || !bias_dev || !out_dev || pixels < 0 || C <= 0 || C % 8) return TISE_ERR_INVALID_ARG;
    if ((id_split_dev != nullptr) == (id_raw_dev != nullptr)) return TISE_ERR_INVALID_ARG;          // exactly one identity
    if (raw_ld % 4 || raw_off % 4 || raw_off < 0 || raw_off + (int64_t)C > raw_ld || !aligned16(raw_dev) || !aligned16(bias_dev))
        return TISE_ERR_INVALID_ARG;
    if (out_ld % 16 || out_off % 8 || out_off < 0 || out_off + (int64_t)C > out_ld || out_ld > 0x7fffffff || !aligned16(out_dev))
        return TISE_ERR_INVALID_ARG;
    if (id_split_dev) {
        if (id_ld % 16 || id_off % 8 || id_off < 0 || id_off + (int64_t)C > id_ld || id_ld > 0x7fffffff || !aligned16(id_split_dev))
            return TISE_ERR_INVALID_ARG;
    } else {
        if (!id_bias_dev || id_raw_ld % 4 || id_raw_off % 4 || id_raw_off < 0 || id_raw_off + (int64_t)C > id_raw_ld ||
            !aligned16(id_raw_dev) || !aligned16(id_bias_dev))
            return TISE_ERR_INVALID_ARG;
    }
    if (out_dev == (const void*)raw_dev || out_dev == id_split_dev || out_dev == (const void*)id_raw_dev) return TISE_ERR_INVALID_ARG;
    if (pixels == 0) return TISE_OK;
    const int C8 = C / 8;
    if (pixels > (0x7fffff00LL * 256) / C8) return TISE_ERR_UNSUPPORTED;                          // one thread per (pixel, 8 channels)
    const int64_t total = pixels * C8;
    const dim3 grid((unsigned)ceil_div64(total, 256));
    hipStream_t s = (hipStream_t)stream;
    _Float16* out = reinterpret_cast<_Float16*>(out_dev);
    if (id_split_dev)
        hipLaunchKernelGGL(residual_relu_split_kernel<true>, grid, dim3(256), 0, s, raw_dev, raw_ld, raw_off, bias_dev,
                           reinterpret_cast<const _Float16*>(id_split_dev), (int)id_ld, id_off, (const float*)nullptr, (int64_t)0, 0,
                           (const float*)nullptr, total, C8, out, (int)out_ld, out_off);
    else
        hipLaunchKernelGGL(residual_relu_split_kernel<false>, grid, dim3(256), 0, s, raw_dev, raw_ld, raw_off, bias_dev,
                           (const _Float16*)nullptr, 0, 0, id_raw_dev, id_raw_ld, id_raw_off, id_bias_dev, total, C8, out, (int)out_ld,
                           out_off);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

TISE_DEFINE_SPLIT_FLAG_READER(tise_internal_split_flag_resnet)
