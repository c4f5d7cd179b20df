// The head of counting alignment (CA; tise_toolbox_amd/countseg_hip.py): CountSeg's two branches and peak stimulation on the raw
// result of the mix convolution.  The definition is restated in include/tise_hip.h (Cholakkal, Sun, Khan & Shao 2019; the PRM
// package of Zhou et al. 2018) and tise_toolbox_amd/countseg_model.py is the plain torch module the route is compared against.
//
// countseg_head_kernel.  One workgroup of 256 threads owns kG = 4 consecutive classes of ONE image, and the maps of those classes
// never leave the CU: kG class maps and kG density maps of at most 1024 pixels, 64 KiB of LDS in fp64.
//   maps    thread = pixel (p = tid, tid + 256, ..).  T_k = fp32(mix_k + b_mix_k); M_c = b_cls[c] + sum_k W_cls[c][k] T_k and D_c =
//           b_den[c] + sum_k W_den[c][k] T_{P+k} in fp64 with k ascending.  A product of two fp32 values is exact in fp64, so the
//           sum has one rounding per term whether the compiler contracts it or not.  The pixel's row is read as 16-byte pieces, the
//           weights have a wave-uniform address.  A class past C (a partial group) repeats class C - 1 and is never stored.
//   peaks   thread = pixel again: the 8 neighbours from LDS (q before p in row-major order must be smaller, q after p not larger:
//           the first maximum of a 3 x 3 window wins its tie, as max_pool2d's indices say), and the pixel's rank by counting over all
//           hw values: the value with #(x < v) <= k < #(x <= v), k = (hw - 1) / 2, is the lower median.  A NaN raises the class's flag.
//   sums    one thread per class adds the peaks M(p) >= median in row-major order and counts them; another (in a second wave) adds
//           the density map in row-major order.  conf = sum / count (NaN and count 0 under the flag), den = sum / hw.
// Every comparison is on the fp64 values.  No floating-point atomics, no library call; an (image, class) result is a function of that
// image's pixels and that class's weights alone, in a fixed order: the same bits in any batch, position or call.
#include "common.h"

namespace {

constexpr int kG = TISE_COUNTSEG_CLASS_GROUP;
constexpr int kMaxPix = TISE_COUNTSEG_MAX_PIXELS;
constexpr int kMaxP = TISE_COUNTSEG_MAX_WIDTH;
constexpr int kMaxC = TISE_COUNTSEG_MAX_CLASSES;
constexpr int64_t kMaxN = TISE_COUNTSEG_MAX_IMAGES;

__global__ __launch_bounds__(256) void countseg_head_kernel(const float* __restrict__ mix, int64_t ld, int off,
                                                            const float* __restrict__ b_mix, const float* __restrict__ w_cls,
                                                            const float* __restrict__ b_cls, const float* __restrict__ w_den,
                                                            const float* __restrict__ b_den, int h, int w, int P, int C,
                                                            double* __restrict__ conf, double* __restrict__ den,
                                                            int* __restrict__ peaks, double* __restrict__ maps) {
#pragma clang fp contract(off)
    __shared__ double sm[kG][kMaxPix];                                  // class maps
    __shared__ double sd[kG][kMaxPix];                                  // density maps
    __shared__ unsigned char lmax[kG][kMaxPix];                         // 1 = local maximum
    __shared__ double med[kG];
    __shared__ int has_nan[kG];
    const int tid = threadIdx.x;
    const int hw = h * w;
    const int64_t img = blockIdx.y;
    const int c0 = blockIdx.x * kG;
    int cls[kG];
#pragma unroll
    for (int j = 0; j < kG; ++j) cls[j] = min(c0 + j, C - 1);
    if (tid < kG) has_nan[tid] = 0;

    for (int p = tid; p < hw; p += 256) {
        const float* row = mix + (img * hw + p) * ld + off;
        double m[kG], d[kG];
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            m[j] = (double)b_cls[cls[j]];
            d[j] = (double)b_den[cls[j]];
        }
        for (int k = 0; k < P; k += 4) {
            const float4 a = *reinterpret_cast<const float4*>(row + k);
            const float4 b = *reinterpret_cast<const float4*>(row + P + k);
            const float ta[4] = {a.x + b_mix[k], a.y + b_mix[k + 1], a.z + b_mix[k + 2], a.w + b_mix[k + 3]};
            const float tb[4] = {b.x + b_mix[P + k], b.y + b_mix[P + k + 1], b.z + b_mix[P + k + 2], b.w + b_mix[P + k + 3]};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < kG; ++j) {
                    m[j] += (double)w_cls[cls[j] * P + k + e] * (double)ta[e];
                    d[j] += (double)w_den[cls[j] * P + k + e] * (double)tb[e];
                }
        }
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            sm[j][p] = m[j];
            sd[j][p] = d[j];
            if (maps != nullptr && c0 + j < C) {
                maps[((img * 2 * C) + c0 + j) * hw + p] = m[j];
                maps[((img * 2 * C) + C + c0 + j) * hw + p] = d[j];
            }
        }
    }
    __syncthreads();

    const int kth = (hw - 1) / 2;
    for (int p = tid; p < hw; p += 256) {
        const int y = p / w, x = p - y * w;
        double v[kG];
        int lt[kG], le[kG];
        bool top[kG];
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            v[j] = sm[j][p];
            lt[j] = le[j] = 0;
            top[j] = true;
        }
        for (int q = 0; q < hw; ++q)
#pragma unroll
            for (int j = 0; j < kG; ++j) {
                const double u = sm[j][q];
                lt[j] += u < v[j] ? 1 : 0;
                le[j] += u <= v[j] ? 1 : 0;
            }
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const int yy = y + dy, xx = x + dx;
                if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
                const int q = yy * w + xx;
                const bool before = dy < 0 || (dy == 0 && dx < 0);
#pragma unroll
                for (int j = 0; j < kG; ++j) {
                    const double u = sm[j][q];
                    top[j] = top[j] && (before ? u < v[j] : u <= v[j]);
                }
            }
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            lmax[j][p] = top[j] ? 1 : 0;
            if (v[j] != v[j])
                has_nan[j] = 1;
            else if (lt[j] <= kth && kth < le[j])
                med[j] = v[j];                                             // equal values: every writer stores the same number
        }
    }
    __syncthreads();

    if (tid < kG && c0 + tid < C) {
        const int j = tid;
        const int64_t o = img * C + c0 + j;
        if (has_nan[j]) {
            conf[o] = __builtin_nan("");
            peaks[o] = 0;
        } else {
            const double md = med[j];
            double s = 0.0;
            int cnt = 0;
            for (int p = 0; p < hw; ++p) {
                const double u = sm[j][p];
                if (lmax[j][p] && u >= md) {
                    s += u;
                    ++cnt;
                }
            }
            conf[o] = s / (double)cnt;
            peaks[o] = cnt;
        }
    } else if (tid >= 64 && tid < 64 + kG && c0 + tid - 64 < C) {
        const int j = tid - 64;
        double s = 0.0;
        for (int p = 0; p < hw; ++p) s += sd[j][p];
        den[img * C + c0 + j] = s / (double)hw;
    }
}

}  // namespace

extern "C" int tise_countseg_head(const float* mix_dev, int64_t ld, int off, const float* b_mix_dev, const float* w_cls_dev,
                                  const float* b_cls_dev, const float* w_den_dev, const float* b_den_dev, int64_t n, int h, int w,
                                  int P, int C, double* conf_dev, double* den_dev, int* peaks_dev, double* maps_dev, void* stream) {
    if (!mix_dev || !b_mix_dev || !w_cls_dev || !b_cls_dev || !w_den_dev || !b_den_dev || !conf_dev || !den_dev || !peaks_dev ||
        n < 0 || h < 1 || w < 1 || P < 4 || P % 4 || C < 1 || off < 0 || off % 4 || ld < 4 || ld % 4 || ld > 0x7fffffff ||
        ((uintptr_t)mix_dev & 15) || ((uintptr_t)b_mix_dev & 3) || ((uintptr_t)w_cls_dev & 3) || ((uintptr_t)b_cls_dev & 3) ||
        ((uintptr_t)w_den_dev & 3) || ((uintptr_t)b_den_dev & 3) || ((uintptr_t)conf_dev & 7) || ((uintptr_t)den_dev & 7) ||
        ((uintptr_t)peaks_dev & 3) || ((uintptr_t)maps_dev & 7))
        return TISE_ERR_INVALID_ARG;
    if (P > kMaxP || C > kMaxC || n > kMaxN || (int64_t)h * w > kMaxPix) return TISE_ERR_UNSUPPORTED;
    if ((int64_t)off + 2 * (int64_t)P > ld) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    hipLaunchKernelGGL(countseg_head_kernel, dim3((unsigned)ceil_div(C, kG), (unsigned)n), dim3(256), 0, (hipStream_t)stream, mix_dev,
                       ld, off, b_mix_dev, w_cls_dev, b_cls_dev, w_den_dev, b_den_dev, h, w, P, C, conf_dev, den_dev, peaks_dev,
                       maps_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}
