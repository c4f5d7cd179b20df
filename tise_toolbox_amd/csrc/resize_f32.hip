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
// One workgroup produces RT output rows of one image, as resize_bilinear_u8_kernel (resize.hip) does: it stages the uint8
// source rows those output rows depend on in LDS (16-byte coalesced loads), runs the first pass LDS -> LDS (float32
// intermediate rows), then the second pass LDS -> registers, clips, applies (v - sub) / div as two fp32 operations and stores
// fp32 rows coalesced, planar NCHW or interleaved NHWC.
//
// Algorithmic bytes per image: h*w*3 read + oh*ow*3*4 written (256x256 -> 299x299: 1 269 420 B).  HBM is the floor, not yet the
// bound: measured 1.69 ms per 1000 such images, 753 GB/s (profiles/r13a_clean_resize_probe.txt) -- two workgroups of 78 KB LDS
// per CU, fp64 multiply/add pairs behind byte-wide LDS reads; 4 % of a trunk pass.
#include <math.h>
#include <string.h>
#include <list>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "common.h"

namespace {

double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// Resample.c bicubic_filter (a = -0.5, support 2)
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct CoeffTableF {
    int ksize;
    std::vector<int> bounds;     // out_size * 2 : (min, count)
    std::vector<double> kk;      // out_size * ksize, normalised, NOT rounded
};

// Resample.c precompute_coeffs(); filter 0 = BILINEAR (support 1), 1 = BICUBIC (support 2)
void precompute_coeffs_f(int in_size, int out_size, CoeffTableF& t, int filter) {
    double scale = (double)in_size / out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    double support = (filter == 1 ? 2.0 : 1.0) * filterscale;
    int ksize = (int)ceil(support) * 2 + 1;
    t.ksize = ksize;
    t.bounds.assign((size_t)out_size * 2, 0);
    t.kk.assign((size_t)out_size * ksize, 0.0);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double* k = &t.kk[(size_t)xx * ksize];
        for (int x = 0; x < xmax; ++x) {
            double w = filter == 1 ? bicubic_filter((x + xmin - center + 0.5) * ss) : bilinear_filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        t.bounds[xx * 2 + 0] = xmin;
        t.bounds[xx * 2 + 1] = xmax;
    }
}

constexpr size_t LDS_BUDGET = 144 * 1024;

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

struct DevPlanF {
    int device;
    int h, w, oh, ow, filter, order;
    int exec;        // H_FIRST | V_FIRST | H_STREAMED
    int ksx, ksy;
    int rt;          // output rows per workgroup
    int span;        // max source rows any row tile needs
    double* dev;     // kx[ow*ksx] | ky[oh*ksy] doubles, then ints: bounds_x[ow*2] | bounds_y[oh*2] | tile_y0[ntiles]
    size_t cap;      // bytes allocated at dev
    int off_ky;      // in doubles
    int off_int;     // in doubles: where the int part begins
    int off_by, off_t0, ntiles;   // in ints, from the int part
};

// Plan cache, as resize.hip's: least-recently-used list + hash index, 8192 plans, an evicted plan's buffer reused.
struct PlanKeyF {
    int device, h, w, oh, ow, filter, order;
    bool operator==(const PlanKeyF& o) const {
        return device == o.device && h == o.h && w == o.w && oh == o.oh && ow == o.ow && filter == o.filter && order == o.order;
    }
};
struct PlanKeyFHash {
    size_t operator()(const PlanKeyF& k) const {
        size_t x = (size_t)k.device;
        for (int v : {k.h, k.w, k.oh, k.ow, k.filter, k.order}) x = x * 1000003u ^ (size_t)v;
        return x;
    }
};
constexpr size_t PLAN_CACHE_CAP = 8192;
std::mutex g_plan_mu;
std::list<DevPlanF> g_plans;                                                   // front = most recently used
std::unordered_map<PlanKeyF, std::list<DevPlanF>::iterator, PlanKeyFHash> g_plan_index;

// The row tile of (h -> oh) beside (w -> ow): the largest of 16, 8, 4, 2, 1 output rows whose staged rows fit LDS; order 0 with
// no such tile: one row per workgroup, streamed.
bool pick_row_tile(const CoeffTableF& ty, int w, int oh, int ow, int order, int* rt_out, int* span_out, int* exec_out) {
    *exec_out = order ? V_FIRST : H_FIRST;
    for (int rt = 16; rt >= 1; rt >>= 1) {
        int span = 0;
        for (int y0 = 0; y0 < oh; y0 += rt) {
            int y1 = (y0 + rt < oh) ? y0 + rt : oh;
            int lo = ty.bounds[y0 * 2], hi = 0;
            for (int y = y0; y < y1; ++y) {
                int e = ty.bounds[y * 2] + ty.bounds[y * 2 + 1];
                if (e > hi) hi = e;
                if (ty.bounds[y * 2] < lo) lo = ty.bounds[y * 2];
            }
            if (hi - lo > span) span = hi - lo;
        }
        if (lds_bytes(w, ow, span, rt, *exec_out) <= LDS_BUDGET) { *rt_out = rt; *span_out = span; return true; }
        if (rt == 1 && order == 0 && lds_bytes(w, ow, span, 1, H_STREAMED) <= LDS_BUDGET) {
            *rt_out = 1; *span_out = span; *exec_out = H_STREAMED;
            return true;
        }
    }
    return false;
}

int get_plan_f(int h, int w, int oh, int ow, int filter, int order, DevPlanF* out) {
    int device = 0;
    TISE_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(g_plan_mu);
    const PlanKeyF key{device, h, w, oh, ow, filter, order};
    auto hit = g_plan_index.find(key);
    if (hit != g_plan_index.end()) {
        g_plans.splice(g_plans.begin(), g_plans, hit->second);
        *out = g_plans.front();
        return TISE_OK;
    }
    CoeffTableF tx, ty;
    precompute_coeffs_f(w, ow, tx, filter);
    precompute_coeffs_f(h, oh, ty, filter);
    DevPlanF p;
    p.device = device;
    p.h = h; p.w = w; p.oh = oh; p.ow = ow; p.filter = filter; p.order = order; p.ksx = tx.ksize; p.ksy = ty.ksize;
    if (!pick_row_tile(ty, w, oh, ow, order, &p.rt, &p.span, &p.exec)) return TISE_ERR_UNSUPPORTED;
    const int rt = p.rt;
    p.ntiles = (oh + rt - 1) / rt;
    p.off_ky = (int)tx.kk.size();
    p.off_int = (int)(tx.kk.size() + ty.kk.size());
    std::vector<int> ints;
    ints.insert(ints.end(), tx.bounds.begin(), tx.bounds.end());
    p.off_by = (int)ints.size();
    ints.insert(ints.end(), ty.bounds.begin(), ty.bounds.end());
    p.off_t0 = (int)ints.size();
    for (int t = 0; t < p.ntiles; ++t) {
        int lo = ty.bounds[(t * rt) * 2];
        int y1 = (t * rt + rt < oh) ? t * rt + rt : oh;
        for (int y = t * rt; y < y1; ++y) if (ty.bounds[y * 2] < lo) lo = ty.bounds[y * 2];
        ints.push_back(lo);
    }
    std::vector<unsigned char> host((size_t)p.off_int * 8 + ints.size() * 4);
    memcpy(host.data(), tx.kk.data(), tx.kk.size() * 8);
    memcpy(host.data() + tx.kk.size() * 8, ty.kk.data(), ty.kk.size() * 8);
    memcpy(host.data() + (size_t)p.off_int * 8, ints.data(), ints.size() * 4);
    p.dev = nullptr;
    p.cap = 0;
    if (g_plans.size() >= PLAN_CACHE_CAP) {
        // evict the least recently used plan; a kernel still reading its table was enqueued before this call: order the
        // overwrite behind it with a device synchronisation, only in this (rare: > 8192 live sizes) case
        DevPlanF victim = g_plans.back();
        g_plan_index.erase(PlanKeyF{victim.device, victim.h, victim.w, victim.oh, victim.ow, victim.filter, victim.order});
        g_plans.pop_back();
        TISE_HIP_CHECK(hipDeviceSynchronize());
        if (victim.device == device && victim.cap >= host.size()) { p.dev = victim.dev; p.cap = victim.cap; }
        else (void)hipFree(victim.dev);
    }
    if (!p.dev) {
        p.cap = host.size() + 8192;                                          // slack so a later, larger plan can reuse it
        TISE_HIP_CHECK(hipMalloc((void**)&p.dev, p.cap));
    }
    TISE_HIP_CHECK(hipMemcpy(p.dev, host.data(), host.size(), hipMemcpyHostToDevice));
    g_plans.push_front(p);
    g_plan_index[key] = g_plans.begin();
    *out = p;
    return TISE_OK;
}

// Pillow's `ss += pixel * k`: an IEEE double multiply, then an IEEE double add -- never one fused multiply-add, which rounds
// once where Pillow rounds twice (a last-bit difference in the float32 result)
__device__ __forceinline__ double mac(double ss, double pix, double k) {
#pragma clang fp contract(off)
    const double p = pix * k;
    return ss + p;
}

struct TileF {                   // one image of a launch: what a workgroup needs beyond its tile index
    const uint8_t* src;          // (h, w, 3) uint8, any alignment
    const double* plan;          // DevPlanF table
    int h, w, ksx, ksy;
    int off_ky, off_int, off_by, off_t0;
    int rt, span, exec, tile0;   // exec: H_FIRST | V_FIRST | H_STREAMED; tile0: the image's first workgroup in a ragged grid
};
static_assert(sizeof(TileF) == 64, "descriptor layout");

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
__device__ __forceinline__ void resize_f32_tile(const TileF& d, size_t img, int tile, const EpilogueF& o, unsigned char* smem) {
    const int h = d.h, w = d.w, oh = o.oh, ow = o.ow;
    const int src_pitch = (w * 3 + 15) & ~15;
    unsigned char* srow = smem;                                                        // span x src_pitch bytes
    float* trow = reinterpret_cast<float*>(smem + (size_t)d.span * src_pitch);         // first-pass rows (16-byte aligned: src_pitch is)
    const double* kx = d.plan;
    const double* ky = d.plan + d.off_ky;
    const int* ints = reinterpret_cast<const int*>(d.plan + d.off_int);
    const int* bx = ints;
    const int* by = ints + d.off_by;

    const int oy0 = tile * d.rt;
    const int oy1 = min(oy0 + d.rt, oh);
    const int ys0 = ints[d.off_t0 + tile];
    int ys1 = 0;                                                                       // end of the source rows this tile needs
    for (int y = oy0; y < oy1; ++y) ys1 = max(ys1, by[2 * y] + by[2 * y + 1]);
    const int nrows = ys1 - ys0;
    const int tid = threadIdx.x;

    // stage source rows [ys0, ys1): contiguous in memory (w*3 bytes each); the byte loop takes what the 16-byte loop cannot
    const uint8_t* sbase = d.src + (size_t)ys0 * (size_t)w * 3;
    const int row_bytes = w * 3;
    if ((((uintptr_t)sbase) & 15) == 0 && (row_bytes & 15) == 0) {
        const int vec_per_row = row_bytes >> 4;
        for (int i = tid; i < nrows * vec_per_row; i += 256) {
            const int r = i / vec_per_row, c = i - r * vec_per_row;
            *reinterpret_cast<uint4*>(srow + (size_t)r * src_pitch + c * 16) =
                *reinterpret_cast<const uint4*>(sbase + (size_t)r * row_bytes + c * 16);
        }
    } else {
        const size_t tot = (size_t)nrows * row_bytes;
        for (size_t i = tid; i < tot; i += 256) {
            const int r = (int)(i / row_bytes), c = (int)(i - (size_t)r * row_bytes);
            srow[(size_t)r * src_pitch + c] = sbase[i];
        }
    }
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

__global__ __launch_bounds__(256) void resize_f32_kernel(TileF d, size_t img_bytes, EpilogueF o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    d.src += (size_t)blockIdx.y * img_bytes;
    resize_f32_tile(d, blockIdx.y, blockIdx.x, o, smem);
}

__global__ __launch_bounds__(256) void resize_ragged_f32_kernel(const TileF* __restrict__ descs, const int* __restrict__ tile_img,
                                                                 EpilogueF o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int img = tile_img[blockIdx.x];
    const TileF d = descs[img];
    resize_f32_tile(d, (size_t)img, (int)blockIdx.x - d.tile0, o, smem);
}

TileF tile_of(const DevPlanF& p, const uint8_t* src) {
    TileF d;
    d.src = src; d.plan = p.dev; d.h = p.h; d.w = p.w; d.ksx = p.ksx; d.ksy = p.ksy;
    d.off_ky = p.off_ky; d.off_int = p.off_int; d.off_by = p.off_by; d.off_t0 = p.off_t0;
    d.rt = p.rt; d.span = p.span; d.exec = p.exec; d.tile0 = 0;
    return d;
}

bool affine_ok(float clip_lo, float clip_hi, float sub, float div) {
    return clip_lo <= clip_hi && isfinite(sub) && isfinite(div) && div != 0.0f;        // (NaN bounds fail the comparison)
}

constexpr int64_t RAGGED_CHUNK = 4096;   // images per launch: at most half of PLAN_CACHE_CAP distinct sizes, so gathering a
                                         // launch's plans can never evict a plan gathered for the same launch
static_assert(RAGGED_CHUNK * 2 <= (int64_t)PLAN_CACHE_CAP, "a launch's plans must fit the plan cache twice");

// Would get_plan_f refuse?  span at one output row per workgroup is at most ksy, a closed form: only sizes that fail THAT
// bound pay for the exact answer (the coefficient table of the vertical pass).
bool plan_refused(int h, int w, int oh, int ow, int filter, int order) {
    const double scale = (double)h / oh, fs = scale < 1.0 ? 1.0 : scale;
    const int ksy = (int)ceil((filter == 1 ? 2.0 : 1.0) * fs) * 2 + 1;
    if (lds_bytes(w, ow, ksy, 1, order ? V_FIRST : H_STREAMED) <= LDS_BUDGET) return false;
    CoeffTableF ty;
    precompute_coeffs_f(h, oh, ty, filter);
    int rt, span, exec;
    return !pick_row_tile(ty, w, oh, ow, order, &rt, &span, &exec);
}

}  // namespace

extern "C" int tise_resize_f32(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, int nhwc, int filter,
                               float clip_lo, float clip_hi, float sub, float div, int order, void* stream) {
    if (n < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || (n > 0 && (!src_dev || !dst_dev)) || (filter != 0 && filter != 1) ||
        (order != 0 && order != 1) || !affine_ok(clip_lo, clip_hi, sub, div))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if (n > 65535 || h > (1 << 20) || w > (1 << 20) || oh > (1 << 20) || ow > (1 << 20)) return TISE_ERR_UNSUPPORTED;
    DevPlanF p;
    const int rc = get_plan_f(h, w, oh, ow, filter, order, &p);
    if (rc != TISE_OK) return rc;
    const size_t lds = lds_bytes(w, ow, p.span, p.rt, p.exec);
    if (lds > 48 * 1024)
        TISE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resize_f32_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const EpilogueF o{dst_dev, oh, ow, nhwc, clip_lo, clip_hi, sub, div};
    hipLaunchKernelGGL(resize_f32_kernel, dim3(p.ntiles, n), dim3(256), lds, (hipStream_t)stream, tile_of(p, src_dev),
                       (size_t)h * (size_t)w * 3, o);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

extern "C" int tise_resize_ragged_f32(const uint8_t* const* src_ptrs_host, const int32_t* h_host, const int32_t* w_host,
                                      const int32_t* order_host, int64_t n, float* dst_dev, int oh, int ow, int nhwc, int filter,
                                      float clip_lo, float clip_hi, float sub, float div, uint8_t* ws_dev, int64_t ws_bytes,
                                      uint8_t* table_host_pinned, int64_t* bad_index, void* stream) {
    if (bad_index) *bad_index = -1;
    if (n < 0 || oh <= 0 || ow <= 0 || ws_bytes < 0 || (filter != 0 && filter != 1) || !affine_ok(clip_lo, clip_hi, sub, div))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if (!src_ptrs_host || !h_host || !w_host || !order_host || !dst_dev || !ws_dev) return TISE_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(ws_dev) & 15) || (reinterpret_cast<uintptr_t>(table_host_pinned) & 15)) return TISE_ERR_INVALID_ARG;
    if (oh > 65535 || ow > (1 << 20)) return TISE_ERR_UNSUPPORTED;
    if (n > (1 << 24)) return TISE_ERR_UNSUPPORTED;
    // table: n descriptors, then one int per workgroup (at most oh row tiles per image); each launch's part ends on 16 bytes
    const int64_t need = n * (int64_t)sizeof(TileF) + n * (int64_t)oh * 4 + 16 * ((n + RAGGED_CHUNK - 1) / RAGGED_CHUNK);
    if (ws_bytes < need) return TISE_ERR_INVALID_ARG;
    // everything that can be refused is refused here, before anything is enqueued
    for (int64_t i = 0; i < n; ++i) {
        const int h = h_host[i], w = w_host[i], order = order_host[i];
        if (!src_ptrs_host[i] || h <= 0 || w <= 0 || (order != 0 && order != 1)) { if (bad_index) *bad_index = i; return TISE_ERR_INVALID_ARG; }
        if (h > (1 << 20) || w > (1 << 20) || plan_refused(h, w, oh, ow, filter, order)) { if (bad_index) *bad_index = i; return TISE_ERR_UNSUPPORTED; }
    }
    std::vector<unsigned char> own;
    unsigned char* host = table_host_pinned;
    if (!host) {
        own.resize((size_t)need);
        host = own.data();
    }
    hipStream_t st = (hipStream_t)stream;
    int64_t pos = 0;                                           // bytes of the table used by the launches so far
    for (int64_t c0 = 0; c0 < n; c0 += RAGGED_CHUNK) {
        const int64_t cn = (n - c0 < RAGGED_CHUNK) ? n - c0 : RAGGED_CHUNK;
        TileF* descs = reinterpret_cast<TileF*>(host + pos);
        int* tiles = reinterpret_cast<int*>(host + pos + cn * (int64_t)sizeof(TileF));
        int64_t ntiles = 0;
        size_t lds = 0;
        for (int64_t i = 0; i < cn; ++i) {
            const int h = h_host[c0 + i], w = w_host[c0 + i], order = order_host[c0 + i];
            DevPlanF p;
            const int rc = get_plan_f(h, w, oh, ow, filter, order, &p);
            if (rc != TISE_OK) { if (bad_index) *bad_index = c0 + i; return rc; }
            descs[i] = tile_of(p, src_ptrs_host[c0 + i]);
            descs[i].tile0 = (int)ntiles;
            for (int t = 0; t < p.ntiles; ++t) tiles[ntiles + t] = (int)i;
            ntiles += p.ntiles;
            const size_t l = lds_bytes(w, ow, p.span, p.rt, p.exec);
            lds = l > lds ? l : lds;
        }
        const int64_t bytes = ((cn * (int64_t)sizeof(TileF) + ntiles * 4) + 15) & ~(int64_t)15;
        if (table_host_pinned) {
            TISE_HIP_CHECK(hipMemcpyAsync(ws_dev + pos, host + pos, (size_t)bytes, hipMemcpyHostToDevice, st));
        } else {
            TISE_HIP_CHECK(hipMemcpyWithStream(ws_dev + pos, host + pos, (size_t)bytes, hipMemcpyHostToDevice, st));
        }
        if (lds > 48 * 1024)
            TISE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resize_ragged_f32_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const EpilogueF o{dst_dev + (size_t)c0 * (size_t)oh * (size_t)ow * 3, oh, ow, nhwc, clip_lo, clip_hi, sub, div};
        hipLaunchKernelGGL(resize_ragged_f32_kernel, dim3((unsigned)ntiles), dim3(256), lds, st,
                           reinterpret_cast<const TileF*>(ws_dev + pos),
                           reinterpret_cast<const int*>(ws_dev + pos + cn * (int64_t)sizeof(TileF)), o);
        TISE_LAUNCH_CHECK();
        pos += bytes;
    }
    return TISE_OK;
}
