// PIL-exact uint8 bilinear resize fused with ToTensor() and the InceptionV3 input affine.
//
// Replaces transforms.Resize((299, 299)) + transforms.ToTensor() (reference
// image_realism/FID/fid_score.py:208-213 -> Pillow Image.resize(BILINEAR), 8 bits per channel) and the
// per-channel affine of image_realism/FID/inception.py:120-124.  Pillow's algorithm (Resample.c):
// per output coordinate a window [xmin, xmin+cnt) of normalised triangle weights rounded to 22-bit
// integers; out = clip8((sum src*k + 2^21) >> 22); horizontal pass first, stored as uint8, then
// the vertical pass on that uint8 image.  Integer arithmetic => the kernel is bit-exact.
//
// One workgroup produces RT output rows of one image (resize_u8_tile): it stages the source rows those
// output rows depend on in LDS (16-byte coalesced loads), runs the horizontal pass LDS->LDS, then the
// vertical pass LDS->registers, maps each byte through a 3x256 fp32 table (v/255 then the affine,
// tabulated on the host with the reference's own op order) and stores fp32 rows coalesced, either
// planar NCHW or interleaved NHWC (torch.channels_last storage).  resize_bilinear_u8_kernel runs that
// tile for a batch of one size, resize_ragged_u8_kernel for images of different sizes (uint8 out only).
// Coefficient windows, row-tile search, plan cache, staging and the ragged driver: resize_plan.h.
//
// Bound: HBM.  Algorithmic bytes per image: h*w*3 read + oh*ow*3*4 written
// (256x256 -> 299x299: 196 608 + 1 072 812 = 1 269 420 B).
#include "resize_plan.h"

#define PRECISION_BITS 22
#define RS_MAXE 8     // elements per thread per row kept in registers: supports ow*3 <= 2048

namespace {

// LDS bytes of a workgroup: the 3x256 fp32 table, then `span` staged source rows and as many horizontal-pass rows.  The table
// counts for the row-tile search of every plan, also for launches that do not stage it (lds_table = false).
size_t lds_bytes(int w, int ow, int span, bool lds_table = true) {
    return (size_t)span * ((size_t)((w * 3 + 15) & ~15) + (size_t)((ow * 3 + 3) & ~3)) + (lds_table ? 3 * 256 * 4 : 0);
}

// Resample.c normalize_coeffs_8bpc()
int round22(double v) { return v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS)); }

PlanCache<6> g_plans;            // key: device, h, w, oh, ow, filter

// plan table, ints: bounds_x[ow*2] | kx[ow*ksx] | bounds_y[oh*2] | ky[oh*ksy] | tile_y0[ntiles]
int get_plan(int h, int w, int oh, int ow, int filter, ResizePlan* out) {
    int device = 0;
    TISE_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(g_plans.mu);
    const PlanCache<6>::Key key{device, h, w, oh, ow, filter};
    if (g_plans.find(key, out)) return TISE_OK;
    const Coeffs tx = precompute_coeffs(w, ow, filter), ty = precompute_coeffs(h, oh, filter);
    ResizePlan p{};
    ResizeTile& t = p.tile;
    t.h = h; t.w = w; t.ksx = tx.ksize; t.ksy = ty.ksize;
    // pick the row tile so staged source rows + horizontal-pass rows fit comfortably in LDS
    if (!pick_row_tile(ty, oh, [&](int span, int) { return lds_bytes(w, ow, span); }, &t.rt, &t.span)) return TISE_ERR_UNSUPPORTED;
    p.ntiles = (oh + t.rt - 1) / t.rt;
    std::vector<int> host(tx.bounds);
    t.off_kx = (int)host.size();
    for (double v : tx.kk) host.push_back(round22(v));
    t.off_by = (int)host.size();
    host.insert(host.end(), ty.bounds.begin(), ty.bounds.end());
    t.off_ky = (int)host.size();
    for (double v : ty.kk) host.push_back(round22(v));
    t.off_t0 = (int)host.size();
    append_tile_starts(ty, oh, t.rt, host);
    return g_plans.insert(key, p, host.data(), host.size() * sizeof(int), 1024 * sizeof(int), out);
}

// device copies of the 3x256 fp32 byte->value tables, keyed by content (a run uses one or two)
struct LutEntry { int device; float host[3 * 256]; float* dev; };
std::mutex g_lut_mu;
std::vector<LutEntry*> g_luts;

int get_lut(const float* lut, float** dev) {
    int device = 0;
    TISE_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(g_lut_mu);
    for (LutEntry* e : g_luts)
        if (e->device == device && memcmp(e->host, lut, sizeof(e->host)) == 0) { *dev = e->dev; return TISE_OK; }
    LutEntry* e = new LutEntry;
    e->device = device;
    memcpy(e->host, lut, sizeof(e->host));
    e->dev = nullptr;
    hipError_t err = hipMalloc((void**)&e->dev, sizeof(e->host));
    if (err == hipSuccess) err = hipMemcpy(e->dev, e->host, sizeof(e->host), hipMemcpyHostToDevice);
    if (err != hipSuccess) { tise_set_last_hip_error((int)err); if (e->dev) hipFree(e->dev); delete e; return TISE_ERR_HIP; }
    g_luts.push_back(e);
    *dev = e->dev;
    return TISE_OK;
}

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// RT output rows of one image: the work of one workgroup, shared by the batch kernel and the ragged kernel.  The source is image
// `src_img` of the dense (h, w, 3) batch at d.src (a ragged list: 0, every image has its own d.src), the destination image `img`
// of the output batch.  TABLE: the 3x256 table `lut` is staged in LDS in front of the rows and `dst`, when not null, takes the
// float output; without it (the ragged kernel: uint8 out only) neither is looked at and the kernel pays for neither.  `u8_out`
// may be null when `dst` is not.
// SMALLK: every horizontal window has <= 3 taps (any up-scale): the thread keeps its taps in registers.
// Thread t owns the row elements e = t, t+256, ... (e = ox*3 + c) for EVERY row of the tile, so the
// per-element table look-ups (window start, taps, table row) are done once per thread, not per pixel,
// and the inner loops contain no integer division.
template <bool SMALLK, bool TABLE>
__device__ __forceinline__ void resize_u8_tile(const ResizeTile& d, int src_img, int img, int tile, int oh, int ow,
                                               const float* __restrict__ lut, float* __restrict__ dst, int nhwc,
                                               uint8_t* __restrict__ u8_out, unsigned char* smem) {
    const int h = d.h, w = d.w, ksx = d.ksx, ksy = d.ksy, rt = d.rt, span = d.span;
    const int src_pitch = (w * 3 + 15) & ~15;
    const int tmp_pitch = (ow * 3 + 3) & ~3;
    float* lut_s = reinterpret_cast<float*>(smem);                       // 3*256 floats (TABLE)
    unsigned char* srow = smem + (TABLE ? 3 * 256 * 4 : 0);              // span x src_pitch
    unsigned char* trow = srow + (size_t)span * src_pitch;               // span x tmp_pitch
    const uint8_t* __restrict__ src = d.src;
    const int* __restrict__ plan = static_cast<const int*>(d.plan);
    const int* bx = plan;
    const int* kx = plan + d.off_kx;
    const int* by = plan + d.off_by;
    const int* ky = plan + d.off_ky;

    const int oy0 = tile * rt;
    const int oy1 = min(oy0 + rt, oh);
    const int ys0 = plan[d.off_t0 + tile];
    int ys1 = 0;                                                         // last source row needed by this tile
    for (int y = oy0; y < oy1; ++y) ys1 = max(ys1, by[2 * y] + by[2 * y + 1]);
    const int nrows = ys1 - ys0;
    const int tid = threadIdx.x;
    const int rowlen = ow * 3;

    if (TABLE)
        for (int i = tid; i < 3 * 256; i += 256) lut_s[i] = lut[i];

    // stage source rows [ys0, ys1): rows are contiguous in memory (w*3 bytes each)
    stage_rows(srow, src_pitch, src + ((size_t)src_img * h + ys0) * (size_t)w * 3, w * 3, nrows);

    // per-thread element descriptors
    int e_off[RS_MAXE];          // byte offset of the first tap inside a staged source row
    int e_k[RS_MAXE][3];         // taps (SMALLK)
    int e_cnt[RS_MAXE];
    int e_lut[RS_MAXE];          // c * 256
    int e_dst[RS_MAXE];          // offset of (ox, c) inside an output row (nhwc) / inside a plane row (nchw: ox)
    int ne = 0;
#pragma unroll
    for (int j = 0; j < RS_MAXE; ++j) {
        const int e = tid + 256 * j;
        e_off[j] = 0; e_cnt[j] = 0; e_lut[j] = 0; e_dst[j] = 0;
        e_k[j][0] = e_k[j][1] = e_k[j][2] = 0;
        if (e < rowlen) {
            ne = j + 1;
            const int ox = e / 3, c = e - 3 * ox;
            const int xmin = (w == ow) ? ox : bx[2 * ox];
            e_off[j] = xmin * 3 + c;
            e_cnt[j] = (w == ow) ? 1 : bx[2 * ox + 1];
            e_lut[j] = c * 256;
            e_dst[j] = nhwc ? e : ox;
            if (SMALLK && w != ow) {
                const int* k = kx + ox * ksx;
                e_k[j][0] = k[0];
                e_k[j][1] = e_cnt[j] > 1 ? k[1] : 0;
                e_k[j][2] = e_cnt[j] > 2 ? k[2] : 0;
            }
        }
    }
    __syncthreads();

    // horizontal pass LDS -> LDS (uint8 intermediate, as Pillow).  When w == ow Pillow skips this pass.
    for (int r = 0; r < nrows; ++r) {
        const unsigned char* sr = srow + (size_t)r * src_pitch;
        unsigned char* tr = trow + (size_t)r * tmp_pitch;
#pragma unroll
        for (int j = 0; j < RS_MAXE; ++j) {
            if (j >= ne) break;
            const int e = tid + 256 * j;
            if (e >= rowlen) break;
            const unsigned char* sp = sr + e_off[j];
            if (w == ow) {
                tr[e] = sp[0];
            } else if (SMALLK) {
                // taps beyond cnt carry a zero coefficient; clamp their address to stay inside the staged row
                const int c1 = e_cnt[j] > 1 ? 3 : 0, c2 = e_cnt[j] > 2 ? 6 : 0;
                // 24-bit multiplies (a byte x a weight <= 2^22): full-rate v_mad_u32_u24 instead of quarter-rate 32-bit multiplies
                const int ss = (1 << (PRECISION_BITS - 1)) + __mul24((int)sp[0], e_k[j][0]) + __mul24((int)sp[c1], e_k[j][1]) +
                               __mul24((int)sp[c2], e_k[j][2]);
                tr[e] = clip8(ss);
            } else {
                const int ox = e / 3;
                const int* k = kx + ox * ksx;
                int ss = 1 << (PRECISION_BITS - 1);
                for (int x = 0; x < e_cnt[j]; ++x) ss += __mul24((int)sp[x * 3], k[x]);
                tr[e] = clip8(ss);
            }
        }
    }
    __syncthreads();

    // uint8-only output (the product path: the stem convolution applies the table) with <= 3 vertical taps: FOUR output bytes
    // per lane -- three aligned dword reads of the horizontal-pass rows instead of twelve byte reads, one (unaligned: a row is
    // ow * 3 bytes) dword store instead of four byte stores.  Same integer arithmetic per byte.
    if (!(TABLE && dst) && u8_out && h != oh && ksy <= 3) {
        const int nd = (rowlen + 3) >> 2;
        for (int y = oy0; y < oy1; ++y) {
            const int ymin = by[2 * y], cnt = by[2 * y + 1];
            const int* k = ky + y * ksy;
            const int k0 = k[0], k1 = cnt > 1 ? k[1] : 0, k2 = cnt > 2 ? k[2] : 0;
            const unsigned char* tbase = trow + (size_t)(ymin - ys0) * tmp_pitch;
            const int p1 = cnt > 1 ? tmp_pitch : 0, p2 = cnt > 2 ? 2 * tmp_pitch : 0;
            uint8_t* urow = u8_out + ((size_t)img * oh + y) * (size_t)rowlen;
            for (int dw = tid; dw < nd; dw += 256) {
                const unsigned t0 = *reinterpret_cast<const unsigned*>(tbase + 4 * dw);
                const unsigned t1 = *reinterpret_cast<const unsigned*>(tbase + p1 + 4 * dw);
                const unsigned t2 = *reinterpret_cast<const unsigned*>(tbase + p2 + 4 * dw);
                unsigned outw = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int ss = (1 << (PRECISION_BITS - 1)) + __mul24((int)((t0 >> (8 * b)) & 255u), k0) +
                                   __mul24((int)((t1 >> (8 * b)) & 255u), k1) + __mul24((int)((t2 >> (8 * b)) & 255u), k2);
                    outw |= (unsigned)clip8(ss) << (8 * b);
                }
                if (4 * dw + 3 < rowlen) {
                    __builtin_memcpy(urow + 4 * dw, &outw, 4);
                } else {
                    for (int b = 0; b < 4; ++b)
                        if (4 * dw + b < rowlen) urow[4 * dw + b] = (uint8_t)(outw >> (8 * b));
                }
            }
        }
        return;
    }

    // vertical pass + table + store, one output row at a time (row parameters are wave-uniform)
    for (int y = oy0; y < oy1; ++y) {
        const int ymin = (h == oh) ? y : by[2 * y];
        const int cnt = (h == oh) ? 1 : by[2 * y + 1];
        const int* k = ky + y * ksy;
        const unsigned char* tbase = trow + (size_t)(ymin - ys0) * tmp_pitch;
        int k0 = 0, k1 = 0, k2 = 0;
        if (h != oh && cnt <= 3) { k0 = k[0]; k1 = cnt > 1 ? k[1] : 0; k2 = cnt > 2 ? k[2] : 0; }
        const int p1 = cnt > 1 ? tmp_pitch : 0, p2 = cnt > 2 ? 2 * tmp_pitch : 0;
        float* drow_nhwc = TABLE && dst ? dst + ((size_t)img * oh + y) * (size_t)rowlen : nullptr;
        uint8_t* urow = u8_out ? u8_out + ((size_t)img * oh + y) * (size_t)rowlen : nullptr;
#pragma unroll
        for (int j = 0; j < RS_MAXE; ++j) {
            if (j >= ne) break;
            const int e = tid + 256 * j;
            if (e >= rowlen) break;
            const unsigned char* tp = tbase + e;
            uint8_t v;
            if (h == oh) {
                v = tp[0];
            } else if (cnt <= 3) {
                const int ss = (1 << (PRECISION_BITS - 1)) + __mul24((int)tp[0], k0) + __mul24((int)tp[p1], k1) + __mul24((int)tp[p2], k2);
                v = clip8(ss);
            } else {
                int ss = 1 << (PRECISION_BITS - 1);
                for (int yy = 0; yy < cnt; ++yy) ss += __mul24((int)tp[(size_t)yy * tmp_pitch], k[yy]);
                v = clip8(ss);
            }
            if (TABLE && dst) {                             // dst == nullptr: uint8 result only (the stem conv applies the table)
                const float f = lut_s[e_lut[j] + v];
                if (nhwc) drow_nhwc[e] = f;
                else dst[(((size_t)img * 3 + (e_lut[j] >> 8)) * oh + y) * ow + e_dst[j]] = f;
            }
            if (urow) urow[e] = v;
        }
    }
}

template <bool SMALLK>
__global__ __launch_bounds__(256) void resize_bilinear_u8_kernel(ResizeTile d, float* __restrict__ dst, int oh, int ow, int nhwc,
                                                                  const float* __restrict__ lut, uint8_t* __restrict__ u8_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    resize_u8_tile<SMALLK, true>(d, blockIdx.y, blockIdx.y, blockIdx.x, oh, ow, lut, dst, nhwc, u8_out, smem);
}

// Images of DIFFERENT sizes into one (n, oh, ow, 3) uint8 batch, one launch (object crops: O-FID / O-IS; one launch per crop was
// ~1000 launches of ~19 workgroups in front of one trunk pass).  A workgroup learns which image and which row tile from a
// tile -> image map and a per-image descriptor, so any mix of sizes is one grid.  uint8 output only (the stem convolution applies
// the input table).
__global__ __launch_bounds__(256) void resize_ragged_u8_kernel(const ResizeTile* __restrict__ descs, const int* __restrict__ tile_img,
                                                                uint8_t* __restrict__ u8_out, int oh, int ow) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int img = tile_img[blockIdx.x];
    const ResizeTile d = descs[img];
    const int tile = (int)blockIdx.x - d.tile0;
    if (d.ksx <= 3) resize_u8_tile<true, false>(d, 0, img, tile, oh, ow, nullptr, nullptr, 1, u8_out, smem);       // workgroup-uniform
    else resize_u8_tile<false, false>(d, 0, img, tile, oh, ow, nullptr, nullptr, 1, u8_out, smem);
}

template <bool SMALLK>
int launch_batch(const ResizePlan& p, const uint8_t* src_dev, int n, float* dst_dev, int oh, int ow, int nhwc, const float* lut_dev,
                 uint8_t* u8_out_dev, hipStream_t st) {
    const size_t lds = lds_bytes(p.tile.w, ow, p.tile.span);
    if (lds > 48 * 1024)
        TISE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resize_bilinear_u8_kernel<SMALLK>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ResizeTile d = p.tile;
    d.src = src_dev;
    hipLaunchKernelGGL(resize_bilinear_u8_kernel<SMALLK>, dim3(p.ntiles, n), dim3(256), lds, st, d, dst_dev, oh, ow, nhwc, lut_dev,
                       u8_out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

}  // namespace

static int resize_u8_impl(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow,
                          int nhwc, const float* lut, uint8_t* u8_out_dev, int filter, void* stream) {
    if (n < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || !lut || (n > 0 && (!src_dev || (!dst_dev && !u8_out_dev))) || (filter != 0 && filter != 1))
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if (n > 65535) return TISE_ERR_UNSUPPORTED;
    ResizePlan p;
    int rc = get_plan(h, w, oh, ow, filter, &p);
    if (rc != TISE_OK) return rc;
    float* lut_dev = nullptr;
    rc = get_lut(lut, &lut_dev);
    if (rc != TISE_OK) return rc;
    if (ow * 3 > 256 * RS_MAXE) return TISE_ERR_UNSUPPORTED;
    return p.tile.ksx <= 3 ? launch_batch<true>(p, src_dev, n, dst_dev, oh, ow, nhwc, lut_dev, u8_out_dev, (hipStream_t)stream)
                           : launch_batch<false>(p, src_dev, n, dst_dev, oh, ow, nhwc, lut_dev, u8_out_dev, (hipStream_t)stream);
}

extern "C" int tise_resize_bilinear_u8(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow,
                                       int nhwc, const float* lut, uint8_t* u8_out_dev, void* stream) {
    return resize_u8_impl(src_dev, n, h, w, dst_dev, oh, ow, nhwc, lut, u8_out_dev, 0, stream);
}

// The same two-pass 8-bit resample with Pillow's BICUBIC filter (filter = 1; 0 = BILINEAR): clip._transform's
// Resize(224, interpolation=BICUBIC) + ToTensor + Normalize through the table (RP_coco.py:64, PA.py:34).
extern "C" int tise_resize_u8(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, int nhwc,
                              const float* lut, uint8_t* u8_out_dev, int filter, void* stream) {
    return resize_u8_impl(src_dev, n, h, w, dst_dev, oh, ow, nhwc, lut, u8_out_dev, filter, stream);
}

extern "C" int tise_resize_ragged_u8(const uint8_t* const* src_ptrs_host, const int32_t* h_host, const int32_t* w_host, int64_t n,
                                     uint8_t* dst_dev, int oh, int ow, int filter, uint8_t* ws_dev, int64_t ws_bytes,
                                     uint8_t* table_host_pinned, int64_t* bad_index, void* stream) {
    const RaggedArgs a{src_ptrs_host, h_host, w_host, nullptr, false, n, dst_dev, oh, ow, filter, ws_dev, ws_bytes, table_host_pinned,
                       bad_index, (hipStream_t)stream};
    return resize_ragged(
        a, true, 256 * RS_MAXE / 3, reinterpret_cast<const void*>(resize_ragged_u8_kernel),
        [&](int h, int w, int) { return plan_refused(h, oh, filter, [&](int span) { return lds_bytes(w, ow, span) <= LDS_BUDGET; }); },
        [&](int h, int w, int, ResizePlan* p, size_t* lds) {
            const int rc = get_plan(h, w, oh, ow, filter, p);
            if (rc == TISE_OK) *lds = lds_bytes(w, ow, p->tile.span, false);
            return rc;
        },
        [&](const ResizeTile* descs, const int* tile_img, unsigned ntiles, size_t lds, int64_t c0, hipStream_t st) {
            hipLaunchKernelGGL(resize_ragged_u8_kernel, dim3(ntiles), dim3(256), lds, st, descs, tile_img,
                               dst_dev + (size_t)c0 * (size_t)oh * (size_t)ow * 3, oh, ow);
        });
}
