// What the two Pillow-exact resize kernels share (resize.hip: 8 bits per channel; resize_f32.hip: float32 "F" mode): Resample.c's
// filters and coefficient windows, the row-tile search, the plan cache, the staging of source rows in LDS, the per-image
// descriptor and the host driver of a ragged entry point.  The two passes themselves are each file's own: they do different
// arithmetic on purpose (22-bit integers there, double multiply and add here).
#pragma once
#include <math.h>
#include <string.h>
#include <array>
#include <list>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "common.h"

namespace {

// ---- filters and coefficients (Resample.c) -------------------------------------------------------------------------------
double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// Resample.c bicubic_filter (a = -0.5, support 2): the filter of clip._transform's Resize(224, BICUBIC)
// (text_relevance/RP_coco.py:31,64 and positional_alignment/PA.py:30,34 through clip.load's preprocess) and of clean-fid
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct Coeffs {
    int ksize;
    std::vector<int> bounds;     // out_size * 2 : (min, count)
    std::vector<double> kk;      // out_size * ksize, normalised, NOT rounded (resize.hip rounds them to 22 bits itself)
};

// window size of in_size -> out_size: a closed form of the scale
int coeff_ksize(int in_size, int out_size, int filter) {
    const double scale = (double)in_size / out_size;
    return (int)ceil((filter == 1 ? 2.0 : 1.0) * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

// Resample.c precompute_coeffs(); filter 0 = BILINEAR (support 1), 1 = BICUBIC (support 2)
Coeffs precompute_coeffs(int in_size, int out_size, int filter) {
    double scale = (double)in_size / out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    double support = (filter == 1 ? 2.0 : 1.0) * filterscale;
    Coeffs t;
    const int ksize = t.ksize = (int)ceil(support) * 2 + 1;
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
    return t;
}

// ---- row tiles: one workgroup makes `rt` output rows of one image from the source rows they depend on -----------------------
constexpr size_t LDS_BUDGET = 144 * 1024;

// first source row of the output rows [y0, y0 + rt), and how many source rows they span
void tile_rows(const Coeffs& ty, int oh, int y0, int rt, int* lo_out, int* span_out) {
    const int y1 = (y0 + rt < oh) ? y0 + rt : oh;
    int lo = ty.bounds[y0 * 2], hi = 0;
    for (int y = y0; y < y1; ++y) {
        int e = ty.bounds[y * 2] + ty.bounds[y * 2 + 1];
        if (e > hi) hi = e;
        if (ty.bounds[y * 2] < lo) lo = ty.bounds[y * 2];
    }
    *lo_out = lo;
    *span_out = hi - lo;
}

// The largest of 16, 8, 4, 2, 1 output rows per workgroup whose LDS need, lds_bytes(span, rt), is within the budget; span: the
// most source rows any row tile of that height needs.  false: none fits, and *span_out is the span at one row per workgroup.
template <typename LdsBytes>
bool pick_row_tile(const Coeffs& ty, int oh, LdsBytes lds_bytes, int* rt_out, int* span_out) {
    for (int rt = 16; rt >= 1; rt >>= 1) {
        int span = 0;
        for (int y0 = 0; y0 < oh; y0 += rt) {
            int lo, s;
            tile_rows(ty, oh, y0, rt, &lo, &s);
            if (s > span) span = s;
        }
        *rt_out = rt; *span_out = span;
        if (lds_bytes(span, rt) <= LDS_BUDGET) return true;
    }
    return false;
}

// the tile_y0 table of a plan: the first staged source row of every row tile
template <typename T>
void append_tile_starts(const Coeffs& ty, int oh, int rt, std::vector<T>& out) {
    for (int y0 = 0; y0 < oh; y0 += rt) {
        int lo, s;
        tile_rows(ty, oh, y0, rt, &lo, &s);
        out.push_back(lo);
    }
}

// Would the plan of (h -> oh) be refused, i.e. does not even one output row per workgroup fit (fits_one_row(span))?  span at
// one row per workgroup is at most the window size, a closed form: only sizes that fail THAT bound pay for the exact answer
// (the coefficient table of the vertical pass), so the check costs nothing for crops.
template <typename Fits>
bool plan_refused(int h, int oh, int filter, Fits fits_one_row) {
    if (fits_one_row(coeff_ksize(h, oh, filter))) return false;
    const Coeffs ty = precompute_coeffs(h, oh, filter);
    int span = 0;
    for (int y = 0; y < oh; ++y) span = ty.bounds[y * 2 + 1] > span ? ty.bounds[y * 2 + 1] : span;
    return !fits_one_row(span);
}

// ---- one image of a launch: what a workgroup needs beyond its tile index ----------------------------------------------------
struct ResizeTile {              // 64 bytes; built on the host, read-only in the kernels
    const uint8_t* src;          // (h, w, 3) uint8, any alignment
    const void* plan;            // the size's plan table on the device: ints (resize.hip), doubles then ints (resize_f32.hip)
    int h, w, ksx, ksy;
    int off_ky;                           // where the table's parts begin: each file names its layout at its get_plan
    union { int off_kx; int off_int; };
    int off_by, off_t0;
    int rt, span;                // output rows per workgroup; the most source rows any row tile needs
    int exec;                    // resize_f32.hip: H_FIRST | V_FIRST | H_STREAMED
    int tile0;                   // the image's first workgroup in a ragged grid
};
static_assert(sizeof(ResizeTile) == 64, "descriptor layout");

struct ResizePlan {
    ResizeTile tile;             // src and tile0 unset
    int ntiles;
    void* dev;                   // = tile.plan
    size_t cap;                  // bytes allocated at dev
};

// ---- plan cache -------------------------------------------------------------------------------------------------------------
// Least-recently-used list + hash index, keyed by N ints that begin with the HIP device (one process may drive several GPUs).
// Object crops (O-FID / O-IS) arrive in thousands of distinct sizes: the cache holds 8192 plans (~12 KB each) and an evicted
// plan's device buffer is REUSED for the new plan when it is large enough, so steady state does no hipMalloc / hipFree (hipFree
// is a device-wide synchronisation).  The caller holds `mu` from find() to insert().
constexpr size_t PLAN_CACHE_CAP = 8192;

template <size_t N>
struct PlanCache {
    using Key = std::array<int, N>;
    struct Hash {
        size_t operator()(const Key& k) const {
            size_t x = (size_t)k[0];
            for (size_t i = 1; i < N; ++i) x = x * 1000003u ^ (size_t)k[i];
            return x;
        }
    };
    using List = std::list<std::pair<Key, ResizePlan>>;
    std::mutex mu;
    List plans;                                                               // front = most recently used
    std::unordered_map<Key, typename List::iterator, Hash> index;

    bool find(const Key& key, ResizePlan* out) {
        auto hit = index.find(key);
        if (hit == index.end()) return false;
        plans.splice(plans.begin(), plans, hit->second);
        *out = plans.front().second;
        return true;
    }

    // uploads the table and caches the plan; `slack` bytes more are allocated so that a later, larger plan can reuse the buffer
    int insert(const Key& key, ResizePlan p, const void* table, size_t bytes, size_t slack, ResizePlan* out) {
        p.dev = nullptr;
        p.cap = 0;
        if (plans.size() >= PLAN_CACHE_CAP) {
            // evict the least recently used plan; any kernel still reading its table was enqueued before this call on
            // the caller's stream(s) -- order the overwrite behind them with a device synchronisation only in this
            // (rare: > 8192 live sizes) case
            const int victim_device = plans.back().first[0];
            const ResizePlan victim = plans.back().second;
            index.erase(plans.back().first);
            plans.pop_back();
            TISE_HIP_CHECK(hipDeviceSynchronize());
            if (victim_device == key[0] && victim.cap >= bytes) { p.dev = victim.dev; p.cap = victim.cap; }
            else (void)hipFree(victim.dev);
        }
        if (!p.dev) {
            p.cap = bytes + slack;
            TISE_HIP_CHECK(hipMalloc(&p.dev, p.cap));
        }
        TISE_HIP_CHECK(hipMemcpy(p.dev, table, bytes, hipMemcpyHostToDevice));
        p.tile.plan = p.dev;
        plans.emplace_front(key, p);
        index[key] = plans.begin();
        *out = p;
        return TISE_OK;
    }
};

// ---- device: source rows -> LDS ---------------------------------------------------------------------------------------------
// `nrows` rows of row_bytes bytes, contiguous from sbase, to srow (pitch src_pitch, a multiple of 16), by the 256 threads of the
// workgroup.  A crop that is a view into a feed's output buffer starts wherever its offset says: the byte loop takes what the
// 16-byte loop cannot.
__device__ __forceinline__ void stage_rows(unsigned char* srow, int src_pitch, const uint8_t* sbase, int row_bytes, int nrows) {
    const int tid = threadIdx.x;
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
}

// ---- host driver of a ragged entry point: images of DIFFERENT sizes to one output size, one launch per RAGGED_CHUNK images --
constexpr int64_t RAGGED_CHUNK = 4096;   // images per launch: at most half of PLAN_CACHE_CAP distinct sizes, so gathering a
                                         // launch's plans (each use moves a plan to the cache's front, eviction takes the back)
                                         // can never evict a plan gathered for the same launch
static_assert(RAGGED_CHUNK * 2 <= (int64_t)PLAN_CACHE_CAP, "a launch's plans must fit the plan cache twice");

struct RaggedArgs {                      // the arguments the ragged entry points share (include/tise_hip.h)
    const uint8_t* const* src_ptrs_host;
    const int32_t* h_host;
    const int32_t* w_host;
    const int32_t* order_host;           // per image 0 | 1 (resize_f32.hip); an entry without it: has_order = false, order 0
    bool has_order;
    int64_t n;
    const void* dst_dev;
    int oh, ow, filter;
    uint8_t* ws_dev;                     // the table on the device: n descriptors, then one int per workgroup (at most oh row
    int64_t ws_bytes;                    // tiles per image); each launch's part ends on 16 bytes
    uint8_t* table_host_pinned;          // the same table in page-locked memory (copied asynchronously), or null
    int64_t* bad_index;
    hipStream_t stream;
};

// scalars_ok: the entry's own scalar arguments are valid; ow_max: the widest output its kernel takes.
//   refused(h, w, order) -> bool                      would the plan builder refuse the size?
//   plan(h, w, order, ResizePlan*, size_t* lds) -> status   the size's plan and the LDS bytes of its workgroups
//   launch(descs_dev, tile_img_dev, ntiles, lds, first_image, stream)     enqueue `kernel` for one chunk
// Everything that can be refused is refused before anything is enqueued, *bad_index naming the image.
template <typename Refused, typename Plan, typename Launch>
int resize_ragged(const RaggedArgs& a, bool scalars_ok, int ow_max, const void* kernel, Refused refused, Plan plan, Launch launch) {
    auto fail = [&a](int64_t i, int rc) { if (a.bad_index) *a.bad_index = i; return rc; };
    const int64_t n = a.n;
    if (a.bad_index) *a.bad_index = -1;
    if (n < 0 || a.oh <= 0 || a.ow <= 0 || a.ws_bytes < 0 || (a.filter != 0 && a.filter != 1) || !scalars_ok) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if (!a.src_ptrs_host || !a.h_host || !a.w_host || (a.has_order && !a.order_host) || !a.dst_dev || !a.ws_dev) return TISE_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(a.ws_dev) & 15) || (reinterpret_cast<uintptr_t>(a.table_host_pinned) & 15)) return TISE_ERR_INVALID_ARG;
    if (a.oh > 65535 || a.ow > ow_max) return TISE_ERR_UNSUPPORTED;
    if (n > (1 << 24)) return TISE_ERR_UNSUPPORTED;
    const int64_t need = n * (int64_t)sizeof(ResizeTile) + n * (int64_t)a.oh * 4 + 16 * ((n + RAGGED_CHUNK - 1) / RAGGED_CHUNK);
    if (a.ws_bytes < need) return TISE_ERR_INVALID_ARG;
    auto order_of = [&a](int64_t i) { return a.has_order ? a.order_host[i] : 0; };
    for (int64_t i = 0; i < n; ++i) {
        const int h = a.h_host[i], w = a.w_host[i], order = order_of(i);
        if (!a.src_ptrs_host[i] || h <= 0 || w <= 0 || (order != 0 && order != 1)) return fail(i, TISE_ERR_INVALID_ARG);
        if (h > (1 << 20) || w > (1 << 20) || refused(h, w, order)) return fail(i, TISE_ERR_UNSUPPORTED);
    }
    std::vector<unsigned char> own;
    unsigned char* host = a.table_host_pinned;
    if (!host) {
        own.resize((size_t)need);
        host = own.data();
    }
    int64_t pos = 0;                                           // bytes of the table used by the launches so far
    for (int64_t c0 = 0; c0 < n; c0 += RAGGED_CHUNK) {
        const int64_t cn = (n - c0 < RAGGED_CHUNK) ? n - c0 : RAGGED_CHUNK;
        ResizeTile* descs = reinterpret_cast<ResizeTile*>(host + pos);
        int* tiles = reinterpret_cast<int*>(host + pos + cn * (int64_t)sizeof(ResizeTile));
        int64_t ntiles = 0;
        size_t lds = 0;
        for (int64_t i = 0; i < cn; ++i) {
            ResizePlan p;
            size_t l = 0;
            const int rc = plan(a.h_host[c0 + i], a.w_host[c0 + i], order_of(c0 + i), &p, &l);
            if (rc != TISE_OK) return fail(c0 + i, rc);
            if (p.ntiles > a.oh) return fail(c0 + i, TISE_ERR_UNSUPPORTED);            // (rt >= 1: cannot happen)
            descs[i] = p.tile;
            descs[i].src = a.src_ptrs_host[c0 + i];
            descs[i].tile0 = (int)ntiles;
            for (int t = 0; t < p.ntiles; ++t) tiles[ntiles + t] = (int)i;
            ntiles += p.ntiles;
            lds = l > lds ? l : lds;
        }
        const int64_t bytes = ((cn * (int64_t)sizeof(ResizeTile) + ntiles * 4) + 15) & ~(int64_t)15;
        if (a.table_host_pinned) {
            TISE_HIP_CHECK(hipMemcpyAsync(a.ws_dev + pos, host + pos, (size_t)bytes, hipMemcpyHostToDevice, a.stream));
        } else {
            TISE_HIP_CHECK(hipMemcpyWithStream(a.ws_dev + pos, host + pos, (size_t)bytes, hipMemcpyHostToDevice, a.stream));
        }
        if (lds > 48 * 1024)
            TISE_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        launch(reinterpret_cast<const ResizeTile*>(a.ws_dev + pos),
               reinterpret_cast<const int*>(a.ws_dev + pos + cn * (int64_t)sizeof(ResizeTile)), (unsigned)ntiles, lds, c0, a.stream);
        TISE_LAUNCH_CHECK();
        pos += bytes;
    }
    return TISE_OK;
}

}  // namespace
