// TensorFlow 1's legacy ResizeBilinear fused with the input affine: the input route of the guided-diffusion ("ADM") evaluator.
//
// The evaluator (Dhariwal & Nichol 2021, "Diffusion Models Beat GANs on Image Synthesis", evaluations/evaluator.py) feeds uint8
// images at their own size into classify_image_graph_def.pb, whose first nodes are Cast -> ResizeBilinear(299, 299) ->
// Sub(128) -> Mul(1/128).  That ResizeBilinear is TF1's legacy kernel (resize_bilinear_op.cc with LegacyScaler):
// align_corners=False, no half-pixel centres, no antialiasing.  Per axis, in float32,
//     scale = (float)in / (float)out;  x = (float)o * scale;  lo = floorf(x);  hi = min(ceilf(x), in - 1);  t = x - floorf(x)
// and per output value, with tl, tr, bl, br the four source bytes as floats (compute_lerp),
//     top = tl + (tr - tl) * tx;  bot = bl + (br - bl) * tx;  v = top + (bot - top) * ty;  out = (v - sub) * mul.
// TensorFlow's CPU kernel compiles these as separate fp32 multiplies and adds; so does this kernel: device code is built with
// contraction on, the pragma in the kernel body switches it off (as mac() of resize_f32.hip does), and the numpy restatement
// tests/_tf1_resize_ref.py is the pin, bit for bit.  lo is clamped to in - 1 too: TensorFlow does not (it would read out of
// bounds), and tests/test_tf1_resize_host.py shows that the unclamped lo never exceeds in - 1 at the sizes served.
//
// A gather: one thread per output pixel, all three channels (four 3-byte taps out of L2, three fp32 stores that the lanes of a
// wave lay side by side: 768 contiguous bytes per wave), no LDS; 64-bit indices, a capped grid and a grid-stride loop, so
// 5000 images are one launch.  Algorithmic bytes per image: h*w*3 read + oh*ow*12 written (256 x 256 -> 299 x 299: 1 269 420 B).
// Measured: 0.576 ms per 1000 such images, 2.2 TB/s of algorithmic bytes, a little over a quarter of HBM's peak
// (profiles/r14a_adm_probe.txt); 1.4 % of a step's kernel time.
#include <math.h>
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void resize_tf1_f32_kernel(const uint8_t* __restrict__ src, int64_t pixels, int h, int w,
                                                             float* __restrict__ dst, int oh, int ow, float sy, float sx,
                                                             float sub, float mul) {
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += stride) {
        const int ox = (int)(i % ow);
        const int64_t r = i / ow;
        const int oy = (int)(r % oh);
        const int64_t img = r / oh;
        const float fy = (float)oy * sy, fx = (float)ox * sx;
        const float fly = floorf(fy), flx = floorf(fx);
        const float ty = fy - fly, tx = fx - flx;
        int y0 = (int)fly, x0 = (int)flx, y1 = (int)ceilf(fy), x1 = (int)ceilf(fx);
        y0 = y0 < h - 1 ? y0 : h - 1;
        y1 = y1 < h - 1 ? y1 : h - 1;
        x0 = x0 < w - 1 ? x0 : w - 1;
        x1 = x1 < w - 1 ? x1 : w - 1;
        const uint8_t* top = src + ((img * h + y0) * (int64_t)w) * 3;
        const uint8_t* bot = src + ((img * h + y1) * (int64_t)w) * 3;
        float* d = dst + i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float tl = (float)top[x0 * 3 + c], tr = (float)top[x1 * 3 + c];
            const float bl = (float)bot[x0 * 3 + c], br = (float)bot[x1 * 3 + c];
            const float t = tl + (tr - tl) * tx;
            const float b = bl + (br - bl) * tx;
            const float v = t + (b - t) * ty;
            d[c] = (v - sub) * mul;
        }
    }
}

}  // namespace

extern "C" int tise_resize_tf1_f32(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, float sub,
                                   float mul, void* stream) {
    if (n < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || !src_dev || !dst_dev || !isfinite(sub) || !isfinite(mul))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    const int64_t pixels = (int64_t)n * oh * ow;
    int64_t blocks = (pixels + 255) / 256;
    if (blocks > 16384) blocks = 16384;                          // 64 workgroups per CU: the loop takes the rest
    const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
    hipLaunchKernelGGL(resize_tf1_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src_dev, pixels, h, w,
                       dst_dev, oh, ow, sy, sx, sub, mul);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}
