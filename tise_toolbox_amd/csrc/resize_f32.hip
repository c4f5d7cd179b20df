// Pillow-exact float32 resize ("F" mode images) fused with clip + input affine: the resize of clean-fid.
//
// clean-fid (Parmar et al. 2022, "On Aliased Resizing and Surprising Subtleties in GAN Evaluation") resizes every channel as a
// float32 image with Pillow's antialiased bicubic filter -- Image.fromarray(x.astype(np.float32), mode="F").resize(size, BICUBIC)
// -- does NOT quantise the result, clips it to [0, 255] and feeds (x - 128) / 128 to Inception-2015.  Pillow's algorithm for
// 32-bit pixels (Resample.c, ImagingResampleHorizontal_32bpc / Vertical_32bpc): the double-precision coefficients of
// precompute_coeffs (no 22-bit rounding); per output
//     double ss = 0.0;  for x ascending: ss += (double)pixel * k[x];  out = (float)ss;
// with a separate multiply and add (the host compiler does not contract them), the horizontal pass first, its result stored as
// float32, then the vertical pass on that float32 image; a pass whose size does not change is skipped.  Image.resize itself
// runs the vertical pass first, as a resize of its own, for a source more than 100 times taller than wide whose height
// shrinks (device.pillow_vertical_first): `order` = 1 states that order, the caller applies the rule.
//
// IEEE double multiply and add are the same on the host and on gfx950, so the kernel is exact bit for bit as long as the
// multiply and the add stay two instructions: device code is compiled with contraction on, mac() below switches it off.
//
// One workgroup produces RT output rows of one image (resize_f32_tile; the row tiles, their plans and the staging are
// resize_plan.h's, shared with resize.hip): it stages the uint8 source rows those output rows depend on in LDS (16-byte
// coalesced loads), runs the first pass LDS -> LDS (float32 intermediate rows), then the second pass LDS -> registers, clips,
// applies (v - sub) / div as two fp32 operations and stores fp32 rows coalesced, planar NCHW or interleaved NHWC.
//
// Algorithmic bytes per image: h*w*3 read + oh*ow*3*4 written (256x256 -> 299x299: 1 269 420 B).  HBM is the floor, not yet the
// bound: measured 1.69 ms per 1000 such images, 753 GB/s (profiles/r13a_clean_resize_probe.txt) -- two workgroups of 78 KB LDS
// per CU, fp64 multiply/add pairs behind byte-wide LDS reads; 4 % of a trunk pass.
#include "resize_plan.h"

namespace {

// How a workgroup runs its tile (`exec`): H_FIRST / V_FIRST are the caller's `order` 0 / 1; H_STREAMED is order 0 for sizes whose
// float32 rows do not fit LDS beside the staged source rows (a strong vertical reduction: hundreds of source rows per output
// row): one output row per workgroup, every lane recomputes the horizontal pass of its element row by row and feeds the rounded
// float32 straight into the vertical sum -- the same operations in the same order, no intermediate rows.
enum { H_FIRST = 0, V_FIRST = 1, H_STREAMED = 2 };

// LDS bytes of a workgroup: `span` staged uint8 source rows, then the float32 rows of the first pass -- H_FIRST: one row of
// ow*3 floats per staged source row; V_FIRST: one row of w*3 floats per output row of the tile; H_STREAMED: none
size_t lds_bytes(int w, int ow, int span, int rt, int exec) {
    const size_t stage = (size_t)span * (size_t)((w * 3 + 15) & ~15);
    if (exec == H_STREAMED) return stage;
    return stage + (exec == V_FIRST ? (size_t)rt * (size_t)w * 12 : (size_t)span * (size_t)ow * 12);
}

PlanCache<7> g_plans;            // key: device, h, w, oh, ow, filter, order

// The row tile of (h -> oh) beside (w -> ow): the largest of 16, 8, 4, 2, 1 output rows whose staged rows fit LDS; order 0 with
// no such tile: one row per workgroup, streamed.
bool pick_exec(const Coeffs& ty, int w, int oh, int ow, int order, ResizeTile* t) {
    t->exec = order ? V_FIRST : H_FIRST;
    if (pick_row_tile(ty, oh, [&](int span, int rt) { return lds_bytes(w, ow, span, rt, t->exec); }, &t->rt, &t->span)) return true;
    t->exec = H_STREAMED;
    return order == 0 && lds_bytes(w, ow, t->span, 1, H_STREAMED) <= LDS_BUDGET;
}

// plan table: kx[ow*ksx] | ky[oh*ksy] doubles (off_ky, in doubles), then from off_int (in doubles) ints:
// bounds_x[ow*2] | bounds_y[oh*2] | tile_y0[ntiles] (off_by, off_t0: in ints, from the int part)
int get_plan_f(int h, int w, int oh, int ow, int filter, int order, ResizePlan* out) {
    int device = 0;
    TISE_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(g_plans.mu);
    const PlanCache<7>::Key key{device, h, w, oh, ow, filter, order};
    if (g_plans.find(key, out)) return TISE_OK;
    const Coeffs tx = precompute_coeffs(w, ow, filter), ty = precompute_coeffs(h, oh, filter);
    ResizePlan p{};
    ResizeTile& t = p.tile;
    t.h = h; t.w = w; t.ksx = tx.ksize; t.ksy = ty.ksize;
    if (!pick_exec(ty, w, oh, ow, order, &t)) return TISE_ERR_UNSUPPORTED;
    p.ntiles = (oh + t.rt - 1) / t.rt;
    t.off_ky = (int)tx.kk.size();
    t.off_int = (int)(tx.kk.size() + ty.kk.size());
    std::vector<int> ints(tx.bounds);
    t.off_by = (int)ints.size();
    ints.insert(ints.end(), ty.bounds.begin(), ty.bounds.end());
    t.off_t0 = (int)ints.size();
    append_tile_starts(ty, oh, t.rt, ints);
    std::vector<unsigned char> host((size_t)t.off_int * 8 + ints.size() * 4);
    memcpy(host.data(), tx.kk.data(), tx.kk.size() * 8);
    memcpy(host.data() + tx.kk.size() * 8, ty.kk.data(), ty.kk.size() * 8);
    memcpy(host.data() + (size_t)t.off_int * 8, ints.data(), ints.size() * 4);
    return g_plans.insert(key, p, host.data(), host.size(), 8192, out);
}

// Pillow's `ss += pixel * k`: an IEEE double multiply, then an IEEE double add -- never one fused multiply-add, which rounds
// once where Pillow rounds twice (a last-bit difference in the float32 result)
__device__ __forceinline__ double mac(double ss, double pix, double k) {
#pragma clang fp contract(off)
    const double p = pix * k;
    return ss + p;
}

struct EpilogueF {
    float* dst;
    int oh, ow, nhwc;
    float lo, hi, sub, div;
};

// clip, affine, store: element e = ox*3 + c of output row y of image img
__device__ __forceinline__ void put(const EpilogueF& o, size_t img, int y, int e, float v) {
    v = v < o.lo ? o.lo : v;                                  // np.clip: max with lo, then min with hi
    v = v > o.hi ? o.hi : v;
    v = (v - o.sub) / o.div;                                  // two fp32 operations, in this order
    if (o.nhwc) {
        o.dst[(img * o.oh + y) * (size_t)o.ow * 3 + e] = v;
    } else {
        const int ox = e / 3, c = e - 3 * ox;
        o.dst[((img * 3 + c) * o.oh + y) * (size_t)o.ow + ox] = v;
    }
}

// One window of one row: cnt taps, 3 elements apart (interleaved channels), ascending
template <typename T>
__device__ __forceinline__ float hdot(const T* p, const double* k, int cnt) {
    double ss = 0.0;
    for (int x = 0; x < cnt; ++x) ss = mac(ss, (double)p[3 * x], k[x]);
    return (float)ss;
}

// Horizontal pass over `nrows` rows of `in` (pitch ip elements, w*3 used) -> ow*3 elements per row: to `out` (pitch op), or,
// FINAL, through the epilogue as output rows y0, y0+1, ...  Thread t owns the elements t, t+256, ... of EVERY row, so the
// window and -- for up to 5 taps: any up-scale -- the coefficients are read once per element, not once per pixel.  A tap
// beyond the window's count carries a zero coefficient and a clamped address: ss + pixel * 0.0 = ss exactly (ss is never -0.0).
template <typename T, bool FINAL>
__device__ __forceinline__ void hpass(const T* in, int ip, float* out, int op, int nrows, int w, int ow, const int* bx, const double* kx,
                                      int ksx, const EpilogueF& o, size_t img, int y0) {
    const int rowlen = ow * 3;
    for (int e = threadIdx.x; e < rowlen; e += 256) {
        const int ox = e / 3, c = e - 3 * ox;
        if (w == ow) {                                                        // Pillow skips the pass
            for (int r = 0; r < nrows; ++r) {
                const float v = (float)in[(size_t)r * ip + e];
                if (FINAL) put(o, img, y0 + r, e, v); else out[(size_t)r * op + e] = v;
            }
            continue;
        }
        const int xmin = bx[2 * ox], cnt = bx[2 * ox + 1];
        const double* k = kx + (size_t)ox * ksx;
        const T* p = in + xmin * 3 + c;
        if (ksx <= 5) {
            double kr[5];
            int off[5];
#pragma unroll
            for (int x = 0; x < 5; ++x) { kr[x] = x < cnt ? k[x] : 0.0; off[x] = x < cnt ? 3 * x : 0; }
            for (int r = 0; r < nrows; ++r) {
                const T* pr = p + (size_t)r * ip;
                double ss = 0.0;
#pragma unroll
                for (int x = 0; x < 5; ++x) ss = mac(ss, (double)pr[off[x]], kr[x]);
                const float v = (float)ss;
                if (FINAL) put(o, img, y0 + r, e, v); else out[(size_t)r * op + e] = v;
            }
        } else {
            for (int r = 0; r < nrows; ++r) {
                const float v = hdot(p + (size_t)r * ip, k, cnt);
                if (FINAL) put(o, img, y0 + r, e, v); else out[(size_t)r * op + e] = v;
            }
        }
    }
}

// Vertical pass: output rows [oy0, oy1) from the rows of `in` (pitch ip, row 0 = source row ys0, `len` elements per row): to
// `out` rows 0, 1, ... (pitch op), or, FINAL, through the epilogue.  Row parameters and coefficients are wave-uniform.
template <typename T, bool FINAL>
__device__ __forceinline__ void vpass(const T* in, int ip, float* out, int op, int len, int h, int oh, int oy0, int oy1, int ys0,
                                      const int* by, const double* ky, int ksy, const EpilogueF& o, size_t img) {
    for (int y = oy0; y < oy1; ++y) {
        const int ymin = (h == oh) ? y : by[2 * y];                           // h == oh: Pillow skips the pass
        const int cnt = (h == oh) ? 1 : by[2 * y + 1];
        const double* k = ky + (size_t)y * ksy;
        const T* base = in + (size_t)(ymin - ys0) * ip;
        for (int e = threadIdx.x; e < len; e += 256) {
            float v;
            if (h == oh) {
                v = (float)base[e];
            } else {
                double ss = 0.0;
                for (int yy = 0; yy < cnt; ++yy) ss = mac(ss, (double)base[(size_t)yy * ip + e], k[yy]);
                v = (float)ss;
            }
            if (FINAL) put(o, img, y, e, v); else out[(size_t)(y - oy0) * op + e] = v;
        }
    }
}

// RT output rows of one image: the work of one workgroup, shared by the batch kernel and the ragged kernel.
__device__ __forceinline__ void resize_f32_tile(const ResizeTile& d, size_t img, int tile, const EpilogueF& o, unsigned char* smem) {
    const int h = d.h, w = d.w, oh = o.oh, ow = o.ow;
    const int src_pitch = (w * 3 + 15) & ~15;
    unsigned char* srow = smem;                                                        // span x src_pitch bytes
    float* trow = reinterpret_cast<float*>(smem + (size_t)d.span * src_pitch);         // first-pass rows (16-byte aligned: src_pitch is)
    const double* kx = static_cast<const double*>(d.plan);
    const double* ky = kx + d.off_ky;
    const int* ints = reinterpret_cast<const int*>(kx + d.off_int);
    const int* bx = ints;
    const int* by = ints + d.off_by;

    const int oy0 = tile * d.rt;
    const int oy1 = min(oy0 + d.rt, oh);
    const int ys0 = ints[d.off_t0 + tile];
    int ys1 = 0;                                                                       // end of the source rows this tile needs
    for (int y = oy0; y < oy1; ++y) ys1 = max(ys1, by[2 * y] + by[2 * y + 1]);
    const int nrows = ys1 - ys0;
    const int tid = threadIdx.x;

    stage_rows(srow, src_pitch, d.src + (size_t)ys0 * (size_t)w * 3, w * 3, nrows);      // source rows [ys0, ys1)
    __syncthreads();

    if (d.exec == H_STREAMED) {
        // one output row (rt = 1): per element, the horizontal window of each source row of the vertical window, rounded to
        // float32 and summed in ascending row order
        const int y = oy0;
        const int ymin = (h == oh) ? y : by[2 * y];
        const int cnt = (h == oh) ? 1 : by[2 * y + 1];
        const double* k = ky + (size_t)y * d.ksy;
        const unsigned char* base = srow + (size_t)(ymin - ys0) * src_pitch;
        for (int e = tid; e < ow * 3; e += 256) {
            const int ox = e / 3, c = e - 3 * ox;
            const int xmin = (w == ow) ? ox : bx[2 * ox], cntx = (w == ow) ? 1 : bx[2 * ox + 1];
            const double* kxe = kx + (size_t)ox * d.ksx;
            const unsigned char* p = base + xmin * 3 + c;
            double ss = 0.0;
            float t = 0.0f;
            for (int yy = 0; yy < cnt; ++yy) {
                t = (w == ow) ? (float)p[(size_t)yy * src_pitch] : hdot(p + (size_t)yy * src_pitch, kxe, cntx);
                ss = mac(ss, (double)t, k[yy]);
            }
            put(o, img, y, e, (h == oh) ? t : (float)ss);
        }
    } else if (d.exec == H_FIRST) {
        // horizontal pass on every staged row, then the vertical pass on its float32 rows
        hpass<unsigned char, false>(srow, src_pitch, trow, ow * 3, nrows, w, ow, bx, kx, d.ksx, o, img, 0);
        __syncthreads();
        vpass<float, true>(trow, ow * 3, nullptr, 0, ow * 3, h, oh, oy0, oy1, ys0, by, ky, d.ksy, o, img);
    } else {
        // vertical pass to the tile's rows at the source width, then the horizontal pass on those float32 rows
        vpass<unsigned char, false>(srow, src_pitch, trow, w * 3, w * 3, h, oh, oy0, oy1, ys0, by, ky, d.ksy, o, img);
        __syncthreads();
        hpass<float, true>(trow, w * 3, nullptr, 0, oy1 - oy0, w, ow, bx, kx, d.ksx, o, img, oy0);
    }
}

__global__ __launch_bounds__(256) void resize_f32_kernel(ResizeTile d, size_t img_bytes, EpilogueF o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d.src += (size_t)blockIdx.y * img_bytes;
    resize_f32_tile(d, blockIdx.y, blockIdx.x, o, smem);
}

__global__ __launch_bounds__(256) void resize_ragged_f32_kernel(const ResizeTile* __restrict__ descs, const int* __restrict__ tile_img,
                                                                 EpilogueF o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int img = tile_img[blockIdx.x];
    const ResizeTile d = descs[img];
    resize_f32_tile(d, (size_t)img, (int)blockIdx.x - d.tile0, o, smem);
}

bool affine_ok(float clip_lo, float clip_hi, float sub, float div) {
    return clip_lo <= clip_hi && isfinite(sub) && isfinite(div) && div != 0.0f;        // (NaN bounds fail the comparison)
}

}  // namespace

extern "C" int tise_resize_f32(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, int nhwc, int filter,
                               float clip_lo, float clip_hi, float sub, float div, int order, void* stream) {
    if (n < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || (n > 0 && (!src_dev || !dst_dev)) || (filter != 0 && filter != 1) ||
        (order != 0 && order != 1) || !affine_ok(clip_lo, clip_hi, sub, div))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if (n > 65535 || h > (1 << 20) || w > (1 << 20) || oh > (1 << 20) || ow > (1 << 20)) return TISE_ERR_UNSUPPORTED;
    ResizePlan p;
    const int rc = get_plan_f(h, w, oh, ow, filter, order, &p);
    if (rc != TISE_OK) return rc;
    ResizeTile d = p.tile;
    d.src = src_dev;
    const size_t lds = lds_bytes(w, ow, d.span, d.rt, d.exec);
    if (lds > 48 * 1024)
        TISE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resize_f32_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const EpilogueF o{dst_dev, oh, ow, nhwc, clip_lo, clip_hi, sub, div};
    hipLaunchKernelGGL(resize_f32_kernel, dim3(p.ntiles, n), dim3(256), lds, (hipStream_t)stream, d,
                       (size_t)h * (size_t)w * 3, o);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

extern "C" int tise_resize_ragged_f32(const uint8_t* const* src_ptrs_host, const int32_t* h_host, const int32_t* w_host,
                                      const int32_t* order_host, int64_t n, float* dst_dev, int oh, int ow, int nhwc, int filter,
                                      float clip_lo, float clip_hi, float sub, float div, uint8_t* ws_dev, int64_t ws_bytes,
                                      uint8_t* table_host_pinned, int64_t* bad_index, void* stream) {
    const RaggedArgs a{src_ptrs_host, h_host, w_host, order_host, true, n, dst_dev, oh, ow, filter, ws_dev, ws_bytes, table_host_pinned,
                       bad_index, (hipStream_t)stream};
    return resize_ragged(
        a, affine_ok(clip_lo, clip_hi, sub, div), 1 << 20, reinterpret_cast<const void*>(resize_ragged_f32_kernel),
        [&](int h, int w, int order) {
            return plan_refused(h, oh, filter, [&](int span) { return lds_bytes(w, ow, span, 1, order ? V_FIRST : H_STREAMED) <= LDS_BUDGET; });
        },
        [&](int h, int w, int order, ResizePlan* p, size_t* lds) {
            const int rc = get_plan_f(h, w, oh, ow, filter, order, p);
            if (rc == TISE_OK) *lds = lds_bytes(w, ow, p->tile.span, p->tile.rt, p->tile.exec);
            return rc;
        },
        [&](const ResizeTile* descs, const int* tile_img, unsigned ntiles, size_t lds, int64_t c0, hipStream_t st) {
            const EpilogueF o{dst_dev + (size_t)c0 * (size_t)oh * (size_t)ow * 3, oh, ow, nhwc, clip_lo, clip_hi, sub, div};
            hipLaunchKernelGGL(resize_ragged_f32_kernel, dim3(ntiles), dim3(256), lds, st, descs, tile_img, o);
        });
}
