// Pixel access to split tensors for the kernels around the VGG-16 pair trunk (lpips.hip, dists.hip): 8 channels of a pixel as
// exact values, the split of 8 fp32 values back into the two halves, the thread map and the launch of a pool kernel, and the
// size check of the pair-batch entry points.  The layout itself -- [hi | lo] interleaved per 32 channels, tise_ilv_off /
// tise_ilv_second -- is csrc/common.h's.
//
// Contraction.  `#pragma clang fp contract(off)` is lexical: it does not follow code into these helpers.  What they compute does
// not need it: hi + lo 2^-11 is exact in fp32 and in fp64 (two 11-bit significands 11 binary places apart), fused or not, and the
// split (f - hi) 2^11 has no add after its multiply.  Any other arithmetic stays in the kernel that owns its rounding.
#pragma once
#include "common.h"

namespace {

typedef _Float16 half8v __attribute__((ext_vector_type(8)));

// q: the hi half of 8 channels of a pixel, their lo half `second` elements further -> the exact values
__device__ __forceinline__ void split_load8_f32(const _Float16* __restrict__ q, int second, float v[8]) {
    const half8v vh = *reinterpret_cast<const half8v*>(q);
    const half8v vl = *reinterpret_cast<const half8v*>(q + second);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)vh[i] + (float)vl[i] * (1.f / 2048.f);
}

__device__ __forceinline__ void split_load8_f64(const _Float16* __restrict__ q, int second, double v[8]) {
    const half8v vh = *reinterpret_cast<const half8v*>(q);
    const half8v vl = *reinterpret_cast<const half8v*>(q + second);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (double)(float)vh[i] + (double)(float)vl[i] * (1.0 / 2048.0);
}

// the 8 channels of chunk `ch8` of a C-channel pixel as exact doubles
__device__ __forceinline__ void split_chunk_f64(const _Float16* __restrict__ pixel, int C, int ch8, double v[8]) {
    split_load8_f64(pixel + tise_ilv_off(8 * ch8, C), tise_ilv_second(8 * ch8, C), v);
}

// 8 fp32 values -> hi = fp16(v), lo = fp16((v - hi) 2^11) (conv_split.split), two 16-byte stores
__device__ __forceinline__ void split_store8(const float v[8], _Float16* __restrict__ d, int second) {
    half8v bh, bl;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        bh[i] = (_Float16)v[i];
        bl[i] = (_Float16)((v[i] - (float)bh[i]) * 2048.f);
    }
    *reinterpret_cast<half8v*>(d) = bh;
    *reinterpret_cast<half8v*>(d + second) = bl;
}

// The thread map of a pool kernel: grid (ceil(OH OW C8 / 256), N), 256 threads; thread = (pooled pixel, 8 channels) of image n,
// so a pixel's row is read and written as whole 16-byte pieces.
struct SplitPoolThread {
    bool live;              // false: past the last element of the image, the thread returns
    int oh, ow;             // the pooled pixel
    int64_t n;              // the image
    int64_t x_px;           // fp16 elements of an input pixel
    int xo, xs;             // this thread's hi chunk inside an input pixel, and the distance to its lo chunk
    int64_t p;              // the output pixel, counted over the images
    int c8;                 // this thread's 8-channel chunk

    // splits 8 fp32 values into this thread's chunk of its output pixel (the address is formed here, after the loads)
    __device__ __forceinline__ void store8(const float v[8], _Float16* __restrict__ out, int out_C, int out_off) const {
        const int ch = out_off + 8 * c8;
        split_store8(v, out + p * (2 * (int64_t)out_C) + tise_ilv_off(ch, out_C), tise_ilv_second(ch, out_C));
    }
};

__device__ __forceinline__ SplitPoolThread split_pool_thread(int OH, int OW, int C8, int x_C, int x_off) {
    SplitPoolThread t;
    const unsigned per_img = (unsigned)OH * (unsigned)OW * (unsigned)C8;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    t.live = e < per_img;
    const unsigned pix = e / (unsigned)C8;
    t.c8 = (int)(e - pix * (unsigned)C8);
    t.oh = (int)(pix / (unsigned)OW);
    t.ow = (int)(pix - (unsigned)t.oh * (unsigned)OW);
    t.n = blockIdx.y;
    t.x_px = 2 * (int64_t)x_C;
    t.p = t.n * OH * OW + pix;
    t.xo = tise_ilv_off(x_off + 8 * t.c8, x_C);
    t.xs = tise_ilv_second(x_off + 8 * t.c8, x_C);
    return t;
}

// the arguments of a *_split_nhwc pool entry point, sides at least min_side
inline bool split_pool_args_ok(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int min_side, int C,
                               const void* out_dev, int64_t out_ld, int out_off) {
    return x_dev && out_dev && n >= 0 && h >= min_side && w >= min_side && C > 0 && C % 8 == 0 && x_ld % 16 == 0 && x_off % 8 == 0 &&
           out_ld % 16 == 0 && out_off % 8 == 0 && x_off >= 0 && out_off >= 0 && x_off + C <= x_ld && out_off + C <= out_ld &&
           x_ld <= 0x7fffffff && out_ld <= 0x7fffffff && !((uintptr_t)x_dev & 15) && !((uintptr_t)out_dev & 15);
}

// launches a pool kernel (x, x_C, x_off, N, H, W, C8, out, out_C, out_off) with SplitPoolThread's grid for an oh x ow output
template <typename Kernel>
int split_pool_launch(Kernel kernel, int oh, int ow, const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C,
                      void* out_dev, int64_t out_ld, int out_off, void* stream) {
    if (n == 0) return TISE_OK;
    if (n > 65535 || (int64_t)oh * ow * (C / 8) >= 0x7fffff00LL) return TISE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((int64_t)oh * ow * (C / 8) + 255) / 256), (unsigned)n), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const _Float16*>(x_dev), (int)x_ld, x_off, n, h, w, C / 8,
                       reinterpret_cast<_Float16*>(out_dev), (int)out_ld, out_off);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

// n pairs of h x w images against an entry point's limits
inline int check_sizes(int64_t n, int h, int w, int max_side, int64_t max_pairs) {
    if (n < 0 || h < 1 || w < 1) return TISE_ERR_INVALID_ARG;
    if (h > max_side || w > max_side || n > max_pairs) return TISE_ERR_UNSUPPORTED;
    return TISE_OK;
}

}  // namespace
