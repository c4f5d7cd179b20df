// torch's float bilinear interpolation fused with ToTensor and the input affine: the input route of pytorch-fid.
//
// pytorch-fid (Seitzer 2020, fid_score.py + inception.py) reads an image with Pillow, ToTensor() divides every byte by 255, and
// its InceptionV3 wrapper resizes with F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) -- half-pixel
// centres, no antialiasing -- and maps 2 * x - 1.  What this kernel writes is what the CPU build of torch computes with its
// generic kernel (aten/src/ATen/native/cpu/UpSampleKernel.cpp, upsample_generic_Nd_kernel_impl: the one torch takes for
// 299 x 299 outputs on more than one thread; on one thread and at small outputs it takes a channels-last kernel with another
// rounding), bit for bit; tests/_torch_resize_ref.py is the restatement and tests/test_torch_resize_host.py
// holds it to the installed torch.  Per axis, all in float32,
//     scale = (float)in / (float)out;  s = max(fmaf(scale, (float)o + 0.5f, -0.5f), 0);  i0 = min((int)s, in - 1);
//     i1 = min(i0 + 1, in - 1);  l1 = s - (float)i0;  l0 = 1 - l1
// (the source index IS a fused multiply-add: separate operations are off by up to 1.5e-5), and per output value, with a, b the
// upper and c, d the lower pair of source bytes and p(byte) = (float)byte / 255.0f,
//     top = fmaf(wx0, p(a), wx1 * p(b));  bot = fmaf(wx0, p(c), wx1 * p(d));  v = fmaf(hy0, top, hy1 * bot);  out = v * mul - sub
// -- in each line the SECOND product is rounded on its own and the first is fused into the add; every other choice differs from
// torch in about a third of the values.  So the three fmaf calls are written out and contraction is off for everything else in
// the kernel body.  p() is a table of 256 floats divided at compile time (IEEE division, the bits of the host's), copied from
// constant memory into LDS by every workgroup: no division per tap.
//
// A gather without LDS staging of source pixels: a workgroup of 256 threads takes a tile of 1024 consecutive output pixels of
// the flat (n, oh, ow) index in four rounds, thread t the pixels t, t + 256, t + 512, t + 768 of the tile -- the lanes of a wave
// work on ADJACENT pixels, so a wave's four 3-byte taps come from one or two cache lines of a source row (a first form gave each
// thread four consecutive pixels: the lanes then sat 4 pixels apart, every tap load touched three times as many lines, and the
// launch took 0.71 ms per 1000 images against 0.57 ms for resize_tf1_f32_kernel, the table look-ups measured to cost nothing).
// The three floats of a pixel go into a 12 KB LDS image of the tile (lane stride 3 words: no bank conflict), and the tile leaves
// as 16-byte stores, 4 KB contiguous per store instruction, when it is whole, every image of it is usable and the destination
// is 16-byte aligned; otherwise every thread stores its own pixels, dword by dword.  One 64-bit and one 32-bit division per
// pixel; 64-bit offsets, a grid capped at 4096 workgroups and a grid-stride loop over the tiles, so any batch is one launch.
// The ragged entry point runs the same kernel body with (pointer, h, w) read from a device table per image instead of from
// the arguments: the same bits image by image, one launch for the list.
// Algorithmic bytes per image: h * w * 3 read + oh * ow * 12 written (256 x 256 -> 299 x 299: 1 269 420 B, as resize_tf1.hip).
#include <math.h>
#include "common.h"

namespace {

struct UnitTable {
    float v[256];
    constexpr UnitTable() : v() {
        for (int i = 0; i < 256; ++i) v[i] = (float)i / 255.0f;
    }
};
__constant__ UnitTable k_unit = UnitTable();

constexpr int64_t kMaxBlocks = 4096;       // 16 workgroups per CU; the grid-stride loop takes the rest
constexpr int kTile = 1024;                // output pixels per workgroup and trip: four per thread

template <bool RAGGED>
__global__ __launch_bounds__(256) void resize_torch_f32_kernel(const uint8_t* __restrict__ src,
                                                               const tise_torch_image_t* __restrict__ table, int64_t pixels, int h,
                                                               int w, float* __restrict__ dst, int oh, int ow, float sy_arg,
                                                               float sx_arg, float mul, float sub, int wide) {
#pragma clang fp contract(off)
    __shared__ float unit[256];
    __shared__ float4 stage4[kTile * 3 / 4];
    float* stage = reinterpret_cast<float*>(stage4);
    const int tid = threadIdx.x;
    unit[tid] = k_unit.v[tid];
    __syncthreads();
    const int64_t per_image = (int64_t)oh * ow;
    const int64_t tiles = (pixels + kTile - 1) / kTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kTile;
        unsigned live = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t p = base + k * 256 + tid;
            if (p < pixels) {
                const int64_t img = p / per_image;
                const int rem = (int)(p - img * per_image);
                const int oy = rem / ow;
                const int ox = rem - oy * ow;
                const uint8_t* image;
                int ih = h, iw = w;
                float sy = sy_arg, sx = sx_arg;
                bool ok = true;
                if (RAGGED) {
                    const tise_torch_image_t e = table[img];
                    image = e.src;
                    ih = e.h;
                    iw = e.w;
                    ok = image != nullptr && ih > 0 && iw > 0;
                    sy = __fdiv_rn((float)ih, (float)oh);
                    sx = __fdiv_rn((float)iw, (float)ow);
                } else {
                    image = src + img * ((int64_t)h * w * 3);
                }
                if (ok) {
                    const float fy = fmaxf(fmaf(sy, (float)oy + 0.5f, -0.5f), 0.0f);
                    int y0 = (int)fy;
                    y0 = y0 < ih - 1 ? y0 : ih - 1;
                    const int y1 = y0 + 1 < ih - 1 ? y0 + 1 : ih - 1;
                    const float hy1 = fy - (float)y0;
                    const float hy0 = 1.0f - hy1;
                    const float fx = fmaxf(fmaf(sx, (float)ox + 0.5f, -0.5f), 0.0f);
                    int x0 = (int)fx;
                    x0 = x0 < iw - 1 ? x0 : iw - 1;
                    const int x1 = x0 + 1 < iw - 1 ? x0 + 1 : iw - 1;
                    const float wx1 = fx - (float)x0;
                    const float wx0 = 1.0f - wx1;
                    const uint8_t* top = image + (int64_t)y0 * iw * 3;
                    const uint8_t* bot = image + (int64_t)y1 * iw * 3;
                    const int64_t o0 = (int64_t)x0 * 3, o1 = (int64_t)x1 * 3;
                    float* out = stage + (k * 256 + tid) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float pa = unit[top[o0 + c]], pb = unit[top[o1 + c]];
                        const float pc = unit[bot[o0 + c]], pd = unit[bot[o1 + c]];
                        const float t = fmaf(wx0, pa, wx1 * pb);
                        const float b = fmaf(wx0, pc, wx1 * pd);
                        const float v = fmaf(hy0, t, hy1 * b);
                        out[c] = v * mul - sub;
                    }
                    live |= 1u << k;
                }
            }
        }
        // (the barrier behind the staging writes, and the vote: a whole tile of usable pixels?)
        const int whole = __syncthreads_and(live == 15u);
        float* d = dst + base * 3;
        if (whole && wide) {
            float4* d4 = reinterpret_cast<float4*>(d);
#pragma unroll
            for (int j = 0; j < 3; ++j) d4[j * 256 + tid] = stage4[j * 256 + tid];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (live >> k & 1) {
                    const int i = (k * 256 + tid) * 3;
                    d[i + 0] = stage[i + 0];
                    d[i + 1] = stage[i + 1];
                    d[i + 2] = stage[i + 2];
                }
            }
        }
        __syncthreads();                                             // the next trip writes the staging image again
    }
}

int launch(bool ragged, const uint8_t* src, const tise_torch_image_t* table, int64_t n, int h, int w, float* dst, int oh, int ow,
           float mul, float sub, hipStream_t stream) {
    const int64_t per_image = (int64_t)oh * ow;
    if (per_image > 0x7fffffff || n > INT64_MAX / per_image / 3) return TISE_ERR_UNSUPPORTED;
    const int64_t pixels = n * per_image;
    int64_t blocks = (pixels + kTile - 1) / kTile;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    const int wide = ((uintptr_t)dst & 15) == 0;
    if (ragged)
        hipLaunchKernelGGL(resize_torch_f32_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, src, table, pixels, 1, 1, dst,
                           oh, ow, 0.0f, 0.0f, mul, sub, wide);
    else
        hipLaunchKernelGGL(resize_torch_f32_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, src, table, pixels, h, w, dst,
                           oh, ow, (float)h / (float)oh, (float)w / (float)ow, mul, sub, wide);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

}  // namespace

extern "C" int tise_resize_torch_f32(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, float mul,
                                     float sub, void* stream) {
    if (n < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || !src_dev || !dst_dev || !isfinite(mul) || !isfinite(sub))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    return launch(false, src_dev, nullptr, n, h, w, dst_dev, oh, ow, mul, sub, (hipStream_t)stream);
}

extern "C" int tise_resize_ragged_torch_f32(const tise_torch_image_t* table_dev, int64_t n, float* dst_dev, int oh, int ow,
                                            float mul, float sub, void* stream) {
    if (n < 0 || oh <= 0 || ow <= 0 || !table_dev || !dst_dev || !isfinite(mul) || !isfinite(sub)) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    return launch(true, nullptr, table_dev, n, 1, 1, dst_dev, oh, ow, mul, sub, (hipStream_t)stream);
}
