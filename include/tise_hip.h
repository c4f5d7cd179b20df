/*
 * libtise_hip.so -- C ABI of the MI355X (gfx950) image-realism hot path of the TISE toolbox.
 *
 * The reference (VinAIResearch/tise-toolbox) has no native code and no FFI: its statistics
 * layer is numpy/scipy called from Python.  Each entry point below replaces the numpy/scipy
 * (or Pillow) call cited next to it; the Python shims in tise_toolbox_amd/ (same function
 * names as the reference) are the only callers and bind these symbols with ctypes
 * (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer named *_dev is DEVICE memory (hipMalloc or a torch CUDA tensor's
 *     data_ptr()); everything else is host memory.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  All work is enqueued
 *     on it; nothing synchronises unless the comment says so.
 *   - return value: 0 = TISE_OK, negative = error (tise_status_string() names it).  No C++
 *     exception crosses the boundary.  Data-dependent conditions (rank deficiency, non-finite
 *     input) are reported through device-side flag words, not through the return code.
 *   - no hidden allocation of caller-visible memory: scratch lives in handles created and
 *     destroyed explicitly.
 */
#ifndef TISE_HIP_H
#define TISE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TISE_OK 0
#define TISE_ERR_INVALID_ARG (-1)   /* -> AssertionError / ValueError in the Python mirror   */
#define TISE_ERR_HIP (-2)           /* a HIP runtime call failed (tise_last_hip_error())     */
#define TISE_ERR_NO_DEVICE (-3)     /* no gfx950 device visible                              */
#define TISE_ERR_UNSUPPORTED (-4)   /* size outside what the kernels are built for          */

const char* tise_status_string(int status);
int tise_last_hip_error(void);                 /* hipError_t of the last failing HIP call    */
int tise_version(void);                        /* ABI version, currently 1                   */
int tise_device_info(int* cu_count, int* gcn_arch_is_gfx950, size_t* total_mem);

/* ------------------------------------------------------------------------------------------
 * (a2) Host feed.  The reference hands decoded images from 8 DataLoader worker processes to the main process through
 * pickling queues as fp32 tensors (image_realism/FID/fid_score.py:215-217, img_data.py:19-25).  Here the decode workers
 * write uint8 pixels into one shared-memory ring owned by the caller (tise_toolbox_amd/png_ring.py); these three calls
 * page-lock that ring once and enqueue host->device copies straight from it.
 *   tise_host_register    hipHostRegister of caller-owned host memory (the memory stays the caller's)
 *   tise_host_unregister  before the caller unmaps it
 *   tise_memcpy_h2d_async enqueue on `stream`; asynchronous when src_host is page-locked (registered)
 * ------------------------------------------------------------------------------------------ */
int tise_host_register(void* host_ptr, size_t bytes);
int tise_host_unregister(void* host_ptr);
int tise_memcpy_h2d_async(void* dst_dev, const void* src_host, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a2) PNG row filters on the device.  Replaces the second half of ``Image.open(f).convert("RGB")`` of
 * Dataset.__getitem__ (image_realism/FID/img_data.py:19-25; third-party Pillow: zlib inflate, then the five row filters
 * of RFC 2083 section 6).  The feed's decode processes only inflate a file into a ring slot (libtise_png.so,
 * csrc/png_decode.c: tise_png_inflate_slot); the slots are copied to HBM as they are and this call reconstructs the
 * pixels.  Slot = [64-byte header | payload]; header byte 0: 0 = payload is h*w*3 RGB pixels (decoded on the host: copied),
 * 3 / 4 = payload is h rows of (1 filter-type byte + w*3 / w*4 filtered bytes) -- None, Sub, Up, Average, Paeth are
 * reversed and the alpha byte of RGBA is dropped (Pillow's convert("RGB") of an RGBA PNG: no blending).
 *   slots_dev    n slots, slot_stride bytes apart (multiple of 4, 4-byte aligned base)
 *   dst_dev      (n, h, w, 3) uint8, the layout tise_resize_u8 reads
 * Bit-exact against Pillow (tests/test_gpu_png.py).  The filter-type bytes are trusted to be <= 4 (the host checks).
 * ------------------------------------------------------------------------------------------ */
int tise_png_unfilter_rgb8(const uint8_t* slots_dev, int64_t n, int64_t slot_stride, int h, int w, uint8_t* dst_dev,
                           void* stream);

/* The same reconstruction for n images of DIFFERENT sizes in one launch (object crops, O-FID / O-IS:
 * tise_toolbox_amd/crop_feed.py).  The slots -- RGB, RGBA and mode-0 ones mixed freely -- sit at per-image offsets in one device
 * arena, the pixels go to per-image offsets in one device buffer as (h_i, w_i, 3) uint8.  One wave per image; LDS is sized
 * for the largest image of the launch.
 *   arena_dev         the arena (4-byte aligned), arena_bytes long
 *   slot_offsets_host n byte offsets of the slots in the arena, multiples of 4
 *   hwm_host          n x 3 int32: height, width and mode (0, 3 or 4) of every slot, as the HOST knows them (what
 *                     tise_png_inflate_slot reported); the slot's own header is not read
 *   out_offsets_host  n byte offsets into dst_dev (dst_bytes long)
 *   table_dev         table_bytes >= 48 * n of device scratch, 8-byte aligned: the call writes the kernel's table there
 *   table_host_pinned NULL, or 48 * n bytes of PAGE-LOCKED host scratch (8-byte aligned) the table is built in and copied from
 *                     asynchronously (the caller leaves it alone until the stream has passed this call); NULL: the call waits
 *                     for its own copy
 * Every value the kernel indexes with comes from these host arrays and is checked here, before any HIP call
 * (TISE_ERR_INVALID_ARG): a NULL pointer, n < 0, a misaligned base or offset, h or w outside 1..65535, a mode other than
 * 0 / 3 / 4, a filtered row above 8192 bytes (such a file must arrive as mode 0), a slot -- payload plus the 8 bytes the dword
 * staging may read past it -- beyond arena_bytes, pixels beyond dst_bytes, a table too small.  The LDS row pitch and the rows
 * per block of every image are computed here, rows >= 1. */
int tise_png_unfilter_ragged_rgb8(const uint8_t* arena_dev, int64_t arena_bytes, int64_t n, const int64_t* slot_offsets_host,
                                  const int32_t* hwm_host, const int64_t* out_offsets_host, uint8_t* dst_dev, int64_t dst_bytes,
                                  uint8_t* table_dev, int64_t table_bytes, uint8_t* table_host_pinned, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a2) JPEG reconstruction on the device.  Replaces the second half of ``Image.open(f).convert("RGB")`` of
 * Dataset.__getitem__ (image_realism/FID/img_data.py:19-25; third-party Pillow -> libjpeg-turbo: dequantisation, the accurate
 * integer IDCT, "fancy" chroma upsampling, YCbCr -> RGB) for JPEG files.  The feed's decode threads only parse markers and
 * Huffman-decode a file into a slot (libtise_jpeg.so, csrc/jpeg_decode.c: tise_jpeg_entropy_decode; slot layout in
 * include/tise_jpeg.h); the slots are copied to HBM as they are and this call reconstructs the pixels of n images of
 * DIFFERENT sizes in one launch pair (csrc/jpeg_idct.hip).  A slot of mode 0 holds pixels decoded on the host: copied.
 *   slots_dev         n slots, slot_stride bytes apart (multiple of 16, 16-byte aligned base)
 *   headers_host      the same n slot headers in HOST memory, header_stride bytes apart (the feed's pinned arena: stride =
 *                     slot_stride).  Every size the kernels index with is taken from here and checked here -- against
 *                     each other, slot_stride, dst_bytes and ws_bytes -- and reaches the kernels in a device table this
 *                     call writes to the head of ws_dev (a stream-ordered copy the call waits for).
 *   out_offsets_host  n byte offsets into dst_dev: image i is written as (h_i, w_i, 3) uint8 at dst_dev + offset, the layout
 *                     tise_resize_u8 reads (offsets i * h * w * 3 give a dense (n, h, w, 3) tensor)
 *   ws_dev            ws_bytes >= tise_jpeg_workspace_bytes(n, slot_stride) of device scratch, 16-byte aligned
 *   table_host_pinned NULL, or 64 * n bytes of PAGE-LOCKED host scratch (8-byte aligned) the call builds the device table in and
 *                     copies from asynchronously: the caller leaves it alone until the stream has passed this call.  NULL: the
 *                     table is copied from a buffer of the call, which then waits for the stream to reach that copy.
 * Bit-exact against Pillow (tests/test_gpu_jpeg.py).  Rejected before any HIP call (TISE_ERR_INVALID_ARG): a NULL pointer,
 * n < 0, a misaligned base or stride, a header whose sampling, block counts or payload length disagree with its size, a slot
 * beyond slot_stride, an output beyond dst_bytes, a workspace too small.  n > 65535: TISE_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
int tise_jpeg_workspace_bytes(int64_t n, int64_t slot_stride, size_t* bytes);
int tise_jpeg_reconstruct_rgb8(const uint8_t* slots_dev, int64_t n, int64_t slot_stride, const uint8_t* headers_host,
                               int64_t header_stride, const int64_t* out_offsets_host, uint8_t* dst_dev, int64_t dst_bytes,
                               uint8_t* ws_dev, int64_t ws_bytes, uint8_t* table_host_pinned, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a3) PIL-exact uint8 bilinear resize + ToTensor + input affine, fused.
 * Replaces transforms.Resize((299,299)) + ToTensor()   image_realism/FID/fid_score.py:208-213
 * (Pillow ImagingResample, 8bpc: 22-bit fixed-point coefficients, horizontal pass -> u8 ->
 * vertical pass -> u8) and the per-channel affine of image_realism/FID/inception.py:120-124.
 *
 *   src_dev   n images, HWC uint8, contiguous (n, h, w, 3)
 *   dst_dev   fp32, (n, 3, oh, ow) when nhwc == 0, (n, oh, ow, 3) when nhwc != 0; NULL: only u8_out_dev is produced
 *             (the latter is torch.channels_last storage of an NCHW tensor)
 *   lut       host pointer, 3*256 floats: lut[c*256 + v] = value written for channel c and
 *             resized byte v (the shim fills it with fp32(v)/255 then the inception.py affine,
 *             evaluated with the reference's own op order, so the kernel is exact by table).
 *   u8_out_dev optional (may be NULL): the resized uint8 image (n, oh, ow, 3), for parity tests.
 * ------------------------------------------------------------------------------------------ */
int tise_resize_bilinear_u8(const uint8_t* src_dev, int n, int h, int w,
                            float* dst_dev, int oh, int ow, int nhwc,
                            const float* lut, uint8_t* u8_out_dev, void* stream);
/* The same kernel with Pillow's BICUBIC filter (filter = 1; 0 = BILINEAR): replaces, for the CLIP metrics, the
 * Resize(224, interpolation=BICUBIC) + ToTensor + Normalize of clip.load's preprocess (third-party `clip`,
 * text_relevance/RP_coco.py:31,64; positional_alignment/PA.py:30,34) -- the table carries (v/255 - mean)/std;
 * dst_dev planar (n, 3, oh, ow) with nhwc == 0.  Square inputs need no CenterCrop. */
int tise_resize_u8(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, int nhwc,
                   const float* lut, uint8_t* u8_out_dev, int filter, void* stream);

/* The uint8 result of the same resample for n images of DIFFERENT sizes, written into one (n, oh, ow, 3) uint8 batch by one
 * launch per 4096 images (RealismEngine.features_from_u8_list: object crops).  Byte for byte what tise_resize_u8 writes to
 * u8_out_dev image by image; plans come from the same per-size cache (a launch's plans cannot evict each other).
 *   src_ptrs_host     n DEVICE pointers in a host array: image i is (h_host[i], w_host[i], 3) uint8, contiguous, any alignment
 *   ws_dev            ws_bytes >= 64 * n + 4 * n * oh + 16 * ceil(n / 4096) of device scratch, 16-byte aligned (descriptors and
 *                     the workgroup -> image map)
 *   table_host_pinned NULL, or as many bytes of PAGE-LOCKED host scratch (16-byte aligned) the table is built in and copied from
 *                     asynchronously; NULL: the call waits for its own copies
 *   bad_index         optional: receives the index of the image a refusal is about, else -1
 * Checked before anything is enqueued: a NULL pointer or a size <= 0 (TISE_ERR_INVALID_ARG), a size the plan builder
 * refuses -- no row tile of it fits LDS -- or ow * 3 > 2048 (TISE_ERR_UNSUPPORTED). */
int tise_resize_ragged_u8(const uint8_t* const* src_ptrs_host, const int32_t* h_host, const int32_t* w_host, int64_t n,
                          uint8_t* dst_dev, int oh, int ow, int filter, uint8_t* ws_dev, int64_t ws_bytes,
                          uint8_t* table_host_pinned, int64_t* bad_index, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a3f) Pillow-exact FLOAT32 resize + clip + input affine, fused: clean-fid's resize (csrc/resize_f32.hip).
 * Every channel of the uint8 image is resampled as Pillow resamples a mode "F" image -- double coefficients (Resample.c
 * precompute_coeffs, no 22-bit rounding), per output `double ss = 0; ss += (double)pixel * k[x]` in ascending x with a
 * separate multiply and add, the result of each pass rounded to float32, a pass whose size does not change skipped -- and is
 * NOT quantised; then min(max(v, clip_lo), clip_hi) and (v - sub) / div, two fp32 operations in that order.
 *
 *   src_dev   n images, HWC uint8, contiguous (n, h, w, 3), any alignment
 *   dst_dev   fp32, (n, 3, oh, ow) when nhwc == 0, (n, oh, ow, 3) when nhwc != 0
 *   filter    0 = BILINEAR, 1 = BICUBIC
 *   order     0: horizontal pass first (Pillow's ImagingResample); 1: vertical pass first (what Image.resize does for a
 *             source more than 100 times taller than wide whose height shrinks: the caller applies that rule)
 * clip_lo > clip_hi, a non-finite sub or div, div == 0: TISE_ERR_INVALID_ARG.  A size of which no row tile fits LDS, n > 65535:
 * TISE_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
int tise_resize_f32(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, int nhwc, int filter,
                    float clip_lo, float clip_hi, float sub, float div, int order, void* stream);

/* The same for n images of DIFFERENT sizes into one fp32 batch ((n, oh, ow, 3) when nhwc != 0, (n, 3, oh, ow) otherwise), one
 * launch per 4096 images: image by image exactly the bits tise_resize_f32 writes.  Arguments, workspace size, pinned table and
 * refusals as tise_resize_ragged_u8; order_host: per image, 0 or 1 as above. */
int tise_resize_ragged_f32(const uint8_t* const* src_ptrs_host, const int32_t* h_host, const int32_t* w_host,
                           const int32_t* order_host, int64_t n, float* dst_dev, int oh, int ow, int nhwc, int filter,
                           float clip_lo, float clip_hi, float sub, float div, uint8_t* ws_dev, int64_t ws_bytes,
                           uint8_t* table_host_pinned, int64_t* bad_index, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a3t) TensorFlow 1's legacy ResizeBilinear (align_corners=False, no half-pixel centres, no antialiasing) + input affine,
 * fused: the input route of the guided-diffusion ("ADM") evaluator's Inception graph (csrc/resize_tf1.hip).  Per axis, all in
 * float32: scale = (float)in / (float)out, x = (float)o * scale, lo = floorf(x), hi = min(ceilf(x), in - 1), t = x - floorf(x)
 * (lo is clamped to in - 1 as well: TensorFlow does not, and the clamp is never active at any size tested in
 * tests/test_tf1_resize_host.py).  Per value: top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx, v = top + (bot - top) * ty,
 * out = (v - sub) * mul -- every multiply and every add a separate fp32 operation, never a fused multiply-add.
 *
 *   src_dev   n images, HWC uint8, contiguous (n, h, w, 3), any alignment
 *   dst_dev   fp32 (n, oh, ow, 3), what tise_stem_conv3x3s2_split reads
 * A non-positive size, n < 0, a null pointer, a non-finite sub or mul: TISE_ERR_INVALID_ARG.  One launch for any n (grid-stride).
 * ------------------------------------------------------------------------------------------ */
int tise_resize_tf1_f32(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, float sub, float mul,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * (a3p) torch's float bilinear interpolation (F.interpolate(x, size, mode="bilinear", align_corners=False): half-pixel centres,
 * no antialiasing) on ToTensor's byte / 255, + input affine, fused: the input route of pytorch-fid (csrc/resize_torch.hip).
 * What the CPU build of torch computes, bit for bit (tests/_torch_resize_ref.py).  Per axis, all in float32:
 * scale = (float)in / (float)out, s = max(fmaf(scale, (float)o + 0.5f, -0.5f), 0), i0 = min((int)s, in - 1),
 * i1 = min(i0 + 1, in - 1), l1 = s - (float)i0, l0 = 1 - l1.  Per value, p(byte) = (float)byte / 255.0f:
 * top = fmaf(wx0, p(a), wx1 * p(b)), bot = fmaf(wx0, p(c), wx1 * p(d)), v = fmaf(hy0, top, hy1 * bot), out = v * mul - sub
 * (a separate multiply and subtract).
 *
 *   src_dev   n images, HWC uint8, contiguous (n, h, w, 3), any alignment
 *   dst_dev   fp32 (n, oh, ow, 3), what tise_stem_conv3x3s2_split reads; any 4-byte alignment (16-byte: wider stores, same bits)
 * A non-positive size, n < 0, a null pointer, a non-finite mul or sub: TISE_ERR_INVALID_ARG.  oh * ow >= 2^31:
 * TISE_ERR_UNSUPPORTED.  n == 0: TISE_OK, no launch.  One launch for any n (grid-stride).
 * ------------------------------------------------------------------------------------------ */
int tise_resize_torch_f32(const uint8_t* src_dev, int n, int h, int w, float* dst_dev, int oh, int ow, float mul, float sub,
                          void* stream);

/* One image of a ragged batch: an (h, w, 3) uint8 image in device memory, contiguous, any alignment. */
typedef struct tise_torch_image {
    const uint8_t* src;
    int32_t h, w;
} tise_torch_image_t;

/* The same for n images of DIFFERENT sizes into one fp32 batch (n, oh, ow, 3), ONE launch for any n: image by image exactly the
 * bits tise_resize_torch_f32 writes.  table_dev: n entries in DEVICE memory, read by the kernel (the caller copies them there,
 * on ``stream`` or before); an entry with a null pointer or a non-positive size is skipped and its output left unwritten.
 * Refusals as above (the table's contents cannot be checked on the host: the caller checks the sizes). */
int tise_resize_ragged_torch_f32(const tise_torch_image_t* table_dev, int64_t n, float* dst_dev, int oh, int ow, float mul,
                                 float sub, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a7) Streaming activation statistics: n, s = sum_i x_i, S = sum_i x_i x_i^T in fp64 from
 * fp32 feature rows that never leave the device.
 * Replaces pred_arr[start:end] = pred.cpu()...  + np.mean(act, 0) + np.cov(act, rowvar=False)
 *                                           image_realism/FID/fid_score.py:98,113,194-195
 * ------------------------------------------------------------------------------------------ */
typedef struct tise_stats tise_stats_t;

int tise_stats_create(int d, tise_stats_t** h);           /* allocates (d*d + d + 2) doubles, zeroed */
int tise_stats_destroy(tise_stats_t* h);
int tise_stats_reset(tise_stats_t* h, void* stream);
/* accumulate `rows` feature rows: feats_dev[r*ld + c], c < d.  Callable once per batch.  ONE launch when d % 64 == 0
 * and the rows are 16-byte aligned (the covariance kernel's diagonal-tile workgroups also fold the column sums and
 * the row count); otherwise the two halves below, one after the other. */
int tise_stats_update(tise_stats_t* h, const float* feats_dev, int64_t rows, int64_t ld, void* stream);
/* the two halves of tise_stats_update, separately launchable:
 * _cov: S += X^T X (fp64 MFMA)   _sum: s += column sums, n += rows (column tiles x 8 row slices, fixed-order merge) */
int tise_stats_update_cov(tise_stats_t* h, const float* feats_dev, int64_t rows, int64_t ld, void* stream);
int tise_stats_update_sum(tise_stats_t* h, const float* feats_dev, int64_t rows, int64_t ld, void* stream);
/* GROUPED accumulation (per-class O-FID, BASELINE configs[4]): feats_dev holds rows sorted by group; group g = rows
 * [row_offsets[g], row_offsets[g + 1]) (HOST array of n_groups + 1 offsets) is folded into handles[g] -- all groups in ONE
 * launch (grid.y = group), so every class's S is read-modify-written once per call instead of once per class and batch. */
int tise_stats_update_grouped(tise_stats_t* const* handles, int n_groups, const float* feats_dev, const int64_t* row_offsets,
                              int64_t ld, void* stream);
/* the contiguous fp64 buffer [S (d*d, upper triangle by 64x64 tile) | s (d) | n | pad] that a
 * data-parallel caller hands to RCCL / torch.distributed.all_reduce(SUM). */
int tise_stats_buffer(tise_stats_t* h, double** buf_dev, size_t* n_doubles);
/* mu = s/n ; sigma = (S - s s^T / n) / (n - 1)   (np.cov ddof = 1).  mu_dev: d, sigma_dev: d*d */
int tise_stats_finalize(tise_stats_t* h, double* mu_dev, double* sigma_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Kernel Inception Distance: grouped sums of the polynomial kernel k(a, b) = (a.b / d + 1)^3 (csrc/mmd.hip).
 * No counterpart in the reference (it has FID only); the estimator is the one of Binkowski et al. 2018 as torch-fidelity,
 * the StyleGAN2-ADA metrics and clean-fid compute it on the host with numpy.  For every group g, from fp32 rows on the device:
 *     out_dev[3 g + 0] = Sxx = sum_{i != j} k(x_i, x_j)     out_dev[3 g + 1] = Syy = sum_{i != j} k(y_i, y_j)
 *     out_dev[3 g + 2] = Sxy = sum_{i, j} k(x_i, y_j)
 * with the dot products in fp64 on the matrix cores; no Gram matrix is materialised.  All groups, the three blocks of each and
 * all their 64 x 64 tiles go in ONE launch (a work list of exactly the tiles that exist), followed by one small launch that
 * adds the tiles' partial sums in a fixed order: no floating-point atomics, two calls on the same inputs give the same bits.
 *   x_dev, y_dev        fp32 feature matrices, rows_* rows of ld_* floats, d columns used (ld >= d, ld % 4 == 0, 16-byte
 *                       aligned base; NULL only with rows == 0)
 *   offsets_*_host      HOST arrays of n_groups + 1 ascending entries, per side (as tise_stats_update_grouped's row_offsets)
 *   index_*_dev         NULL: group g of that side is the contiguous rows offsets[g] .. offsets[g + 1] - 1;
 *                       else n_index_* int64 row numbers on the DEVICE and group g is the rows index[offsets[g] .. offsets[g + 1] - 1]
 *   A group may have different sizes on the two sides; a side with 0 rows yields zeros for the sums it enters.
 *   out_dev             3 * n_groups doubles
 *   ws_dev              ws_bytes >= tise_mmd_poly3_workspace_bytes(...) of device scratch, 8-byte aligned (segment table + one
 *                       double per tile); the call copies its table there and waits for that copy before it launches
 * Rejected before any HIP call (TISE_ERR_INVALID_ARG): a NULL pointer, d <= 0, ld < d, ld % 4 != 0 or a base that is not 16-byte
 * aligned, negative counts, descending offsets, a group that reaches past the rows (or past the index), a workspace too small.
 * TISE_ERR_UNSUPPORTED: a group above 2^24 rows or more than 2^31 - 1 tiles in all.
 * The VALUES of a device index array are NOT checked here and are trusted to lie in [0, rows): the caller validates them on
 * the host before it uploads them (tise_toolbox_amd.device.PolynomialMMD does).
 * ------------------------------------------------------------------------------------------ */
int tise_mmd_poly3_workspace_bytes(const int64_t* offsets_x_host, const int64_t* offsets_y_host, int n_groups, size_t* bytes);
int tise_mmd_poly3_grouped(const float* x_dev, int64_t rows_x, int64_t ld_x, const int64_t* index_x_dev, int64_t n_index_x,
                           const int64_t* offsets_x_host, const float* y_dev, int64_t rows_y, int64_t ld_y,
                           const int64_t* index_y_dev, int64_t n_index_y, const int64_t* offsets_y_host, int n_groups, int d,
                           double* out_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CLIP maximum mean discrepancy (CMMD; Jayasumana et al. 2024, "Rethinking FID"): grouped sums of the Gaussian kernel (csrc/mmd.hip)
 *     k(a, b) = exp(-gamma d2(a, b)),      d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)      (NaN stays NaN: "Non-finite feature rows" below)
 * No counterpart in the reference; the published implementation forms the three n x n kernel matrices in fp32.  The interface is
 * tise_mmd_poly3_grouped's, argument for argument, plus gamma, and so are the outputs (Sxx and Syy over i != j, Sxy over all pairs),
 * the single launch over exactly the 64 x 64 tiles that exist, the fixed-order reduction launch after it, and the guarantee: no
 * floating-point atomics, no n x n matrix, two calls on the same inputs give the same bits.  Numerics: a.b in fp64 on the matrix
 * cores; |.|^2 from a pre-pass (one more small launch) into the workspace as a fixed-order sum of exact squares, as
 * tise_knn_radius2 forms it -- with the parentheses above, d2 of a pair is the same bits whichever side each row is on; exp is the
 * fp64 library function.  The cost of that exp beside the tile's matrix work has NOT been measured.
 *   gamma               finite and >= 0 (CMMD: 1 / (2 sigma^2), sigma = 10, on L2-normalised rows)
 *   ws_dev              ws_bytes >= tise_mmd_rbf_workspace_bytes(...) = tise_mmd_poly3_workspace_bytes(...) + 8 bytes for every
 *                       row that enters a group, per side: 8 * ((offsets_x[n_groups] - offsets_x[0]) + (offsets_y[n_groups] -
 *                       offsets_y[0]))
 * Rejected before any HIP call: whatever tise_mmd_poly3_grouped rejects, with the same codes, and a gamma that is NaN, infinite
 * or negative (TISE_ERR_INVALID_ARG).  Index values are trusted as there (tise_toolbox_amd.device.GaussianMMD validates them).
 * ------------------------------------------------------------------------------------------ */
int tise_mmd_rbf_workspace_bytes(const int64_t* offsets_x_host, const int64_t* offsets_y_host, int n_groups, size_t* bytes);
int tise_mmd_rbf_grouped(const float* x_dev, int64_t rows_x, int64_t ld_x, const int64_t* index_x_dev, int64_t n_index_x,
                         const int64_t* offsets_x_host, const float* y_dev, int64_t rows_y, int64_t ld_y,
                         const int64_t* index_y_dev, int64_t n_index_y, const int64_t* offsets_y_host, int n_groups, int d,
                         double gamma, double* out_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * k-nearest-neighbour manifold metrics: improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et
 * al. 2020) (csrc/knn.hip).  No counterpart in the reference; the definitions are those of the `prdc` package, which computes
 * them on the host with sklearn.  From fp32 rows on the device, with
 *     d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)     in fp64: a.b on the matrix cores, |.|^2 a fixed-order sum of exact squares
 * tise_knn_radius2 writes, for every row i of one set, r2[i] = the k-th smallest d2(x_i, x_j) over j != i, and tise_prdc_counts,
 * for rows R (n, the real side) and F (m, the generated side) with their radii, with strict comparisons on the squared values,
 *     cnt[i] = #{ j : d2(R_i, F_j) < r2_r[i] }    rec[i] = 1 if some j has d2(R_i, F_j) < r2_f[j], else 0
 *     prec[j] = 1 if some i has d2(R_i, F_j) < r2_r[i], else 0
 * No rows x rows matrix is written; the grid is (row tiles of 64) x (S column splits).  d2 of a pair is the same bits in both
 * calls and for either order of the two rows.  Results combine across workgroups through a selection among candidates and
 * integer add / or only: two calls on the same inputs give the same bits.
 *   x_dev, r_dev, f_dev   fp32 feature matrices, rows of ld floats, d columns used (ld >= d, ld % 4 == 0, 16-byte aligned base)
 *   k                     1 .. 16; rows >= k + 1 (tise_prdc_counts: rows >= 1 per side); rows <= 2^24
 *   col_splits            S: 0 = ceil(1024 / row tiles) (about four workgroups per compute unit of a 256-unit device when the
 *                         rows are few), 1 .. 1024 = the caller's value; either is capped at the number of column tiles
 *   r2_dev                rows doubles (out); r2_r_dev, r2_f_dev: n and m doubles (in)
 *   cnt_dev, rec_dev      n int32 each (out);  prec_dev: m int32 (out); the call zeroes them first
 *   ws_dev                device scratch, 8-byte aligned.  tise_knn_radius2: ws_bytes >= tise_knn_workspace_bytes(rows, k,
 *                         col_splits) = 8 * rows * (S * k + 1) (k candidates per row and split, and the norms);
 *                         tise_prdc_counts: ws_bytes >= 8 * (rows_r + rows_f) (the norms)
 * Rejected before any HIP call (TISE_ERR_INVALID_ARG): a NULL pointer, k outside 1 .. 16, rows < k + 1, d <= 0, ld < d,
 * ld % 4 != 0, a feature base that is not 16-byte aligned, col_splits outside 0 .. 1024, a workspace too small or misaligned.
 * TISE_ERR_UNSUPPORTED: more than 2^24 rows.
 * Non-finite feature rows (this block and tise_mmd_rbf_grouped / tise_mmd_poly3_grouped above).  A row that holds a NaN or an
 * infinity is a legal input with a defined result; nothing is rejected and nothing is clamped away.  Its |.|^2 is stored as NaN
 * and the clamp of d2 keeps a NaN (max(0, NaN) is NaN here, not 0), so d2 of every pair with such a row is NaN (one function
 * each for every kernel of the block: rows_norm2_or_nan and rows_d2 in csrc/rows_tile.h):
 *   tise_knn_radius2 / tise_prdc_counts: every IEEE comparison with NaN is false, so the pair is never a neighbour candidate and
 *     never inside a ball.  The row itself gets r2 = NaN, cnt = 0, rec = 0, prec = 0; every other row gets exactly the results
 *     of the same call on the sets WITHOUT that row (the caller must leave k + 1 finite rows for them to be meaningful;
 *     r2 = +inf where fewer than k finite other rows exist).  A NaN in r2_r_dev / r2_f_dev is a ball that holds nothing.
 *   tise_mmd_rbf_grouped: k = exp(-gamma NaN) = NaN for the pair, at every gamma including 0.  tise_mmd_poly3_grouped forms no
 *     d2: a.b, hence k, is NaN or +-inf by IEEE arithmetic.  In both, every sum of a group that has a pair with the row is
 *     non-finite -- Sxx and Sxy when the row is in X, Syy and Sxy when it is in Y -- while the group's third sum and EVERY other
 *     group of the launch have the bits of the same launch on finite rows (rows past a group's end are fetched from its last
 *     row and masked by selection, never by multiplication).
 * For finite rows neither rule changes a bit.  tise_toolbox_amd.prdc.prdc_from_features turns the NaN radii into a ValueError
 * (as the prdc package refuses such input); cmmd and kid return the NaN, as their reference implementations do.
 * ------------------------------------------------------------------------------------------ */
int tise_knn_workspace_bytes(int64_t rows, int k, int col_splits, size_t* bytes);
int tise_knn_radius2(const float* x_dev, int64_t rows, int64_t ld, int d, int k, int col_splits, double* r2_dev, void* ws_dev,
                     size_t ws_bytes, void* stream);
int tise_prdc_counts(const float* r_dev, int64_t rows_r, int64_t ld_r, const double* r2_r_dev, const float* f_dev, int64_t rows_f,
                     int64_t ld_f, const double* r2_f_dev, int d, int col_splits, int32_t* cnt_dev, int32_t* rec_dev,
                     int32_t* prec_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Nearest row of another set, with its index (csrc/knn.hip): the primitive of authenticity (AuthPct; Alaa et al. 2022, as the
 * `dgm-eval` package of Stein et al. 2023 states it) and of "which training image is this sample closest to".  No counterpart in
 * the reference; dgm-eval writes the whole n x m fp32 torch.cdist matrix.  For every query row i, over the base rows j, with the
 * d2 of the block above (the same bits for the same pair as in tise_knn_radius2 and tise_prdc_counts):
 *     d2[i]  = min_j d2(Q_i, B_j)          idx[i] = the SMALLEST j that attains it
 * exclude_diagonal = 1 skips the pair j == i by row number (the within-set pass; it requires rows_q == rows_b, and q_dev may be
 * b_dev): d2 then has the bits of tise_knn_radius2 at k = 1.  The grid is that block's, (query row tiles of 64) x (S column
 * splits) with the same col_splits rule; a workgroup writes one (d2, index) candidate per (row, split) and a merge launch takes
 * the minimum of the S candidates.  The ONLY combination anywhere is the lexicographic minimum of (d2, index),
 * v < best || (v == best && j < bestj), which is order-independent: the result is bitwise reproducible and does not depend on
 * col_splits.  No floating-point atomics, no n x m matrix.
 *   q_dev, b_dev          fp32 feature matrices, rows of ld floats, d columns used (ld >= d, ld % 4 == 0, 16-byte aligned base)
 *   rows_q, rows_b        1 .. 2^24 each
 *   d2_dev, idx_dev       rows_q doubles (8-byte aligned) and rows_q int32 (out)
 *   ws_dev                device scratch, 8-byte aligned, ws_bytes >= tise_nn_workspace_bytes(rows_q, rows_b, col_splits)
 *                         = 8 * (rows_q + rows_b) + (8 + 4) * rows_q * S: the norms of both sides, then one double and one int32
 *                         candidate per query row and split, S = min(col_splits or ceil(1024 / query row tiles), base row tiles)
 * Non-finite feature rows (the rule of the block above, extended): a base row that holds a NaN or an infinity is nobody's
 * nearest row -- d2 of every pair with it is NaN and both comparisons of the rule are false -- so every query row gets the bits
 * of the same call without that base row (its index shifted accordingly).  A query row that holds one gets d2 = NaN, idx = -1.
 * A query row with no candidate at all -- every base row non-finite, or rows_b == 1 under exclude_diagonal -- gets d2 = +inf,
 * idx = -1.
 * Rejected before any HIP call (TISE_ERR_INVALID_ARG): a NULL pointer, rows_q < 1 or rows_b < 1, d <= 0, ld < d, ld % 4 != 0, a
 * feature base that is not 16-byte aligned, col_splits outside 0 .. 1024, exclude_diagonal outside {0, 1} or set while rows_q !=
 * rows_b, a misaligned output, a workspace too small or misaligned.  TISE_ERR_UNSUPPORTED: more than 2^24 rows on either side.
 * ------------------------------------------------------------------------------------------ */
int tise_nn_workspace_bytes(int64_t rows_q, int64_t rows_b, int col_splits, size_t* bytes);
int tise_nn_argmin(const float* q_dev, int64_t rows_q, int64_t ld_q, const float* b_dev, int64_t rows_b, int64_t ld_b, int d,
                   int exclude_diagonal, int col_splits, double* d2_dev, int32_t* idx_dev, void* ws_dev, size_t ws_bytes,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * PSNR, SSIM and MS-SSIM of image PAIRS (csrc/ssim.hip; tise_toolbox_amd/paired.py).  No counterpart in the reference.  Images
 * are 8-bit RGB, HWC, L = 255; every quantity is formed per channel and the caller averages the three channels.
 *   PSNR     SSE = sum (x - y)^2 over the h w 3 bytes (an exact integer; tise_pair_sse_u8), MSE = SSE / (3 h w),
 *            PSNR = 10 log10(255^2 / MSE) -- the caller's fp64.
 *   SSIM     Wang, Bovik, Sheikh & Simoncelli 2004: window g[i] ~ exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, normalised to sum 1,
 *            applied as g g^T at the (h - 10)(w - 10) VALID positions (no padding): mx, my, E[xx], E[yy], E[xy];
 *            sxx = E[xx] - mx mx, syy = E[yy] - my my, sxy = E[xy] - mx my (biased, weighted); C1 = (0.01 255)^2,
 *            C2 = (0.03 255)^2; cs = (2 sxy + C2) / (sxx + syy + C2), l = (2 mx my + C1) / (mx mx + my my + C1), ssim = l cs.
 *            tise_ssim_pairs gives, per pair and channel, the mean of the ssim map and the mean of the cs map.
 *   MS-SSIM  Wang, Simoncelli & Bovik 2003: five scales, between scales the 2 x 2 mean with stride 2, a last odd row or column
 *            DROPPED (tise_pool2x2_pairs); the caller forms prod_s max(m_s, 0)^w_s from the cs means of scales 1..4 and the
 *            ssim mean of scale 5.  A level holds multiples of 4^-s that are <= 255: exact in fp32.
 * All arithmetic after the byte or float load is fp64, in a fixed order: the five moments go through one function (with x == y
 * E[xx], E[yy] and E[xy] are bit-equal, as are mx and my), l and cs are formed without contraction, so an IDENTICAL pair gives
 * exactly 1.0 for both means.  Map means: fixed-order sums inside a workgroup, one partial per (pair, tile) in the workspace, a
 * second fixed-order pass; no floating-point atomics.  A pair's result depends on its own size and values only -- not on max_h,
 * max_w, the other pairs of the launch or the run.  The uint8 and the fp32 form of the same values give the same bits.
 *
 * RAGGED launches: every entry point takes a table of n records in DEVICE memory (the caller copies it there, on ``stream`` or
 * before), one record per pair, and is one launch (tise_ssim_pairs: two) for any n.  max_h, max_w: the largest h and w of the
 * table, which size the grid and the workspace.  The table's contents cannot be checked on the host: the caller checks them.  A
 * record with a null pointer, a side below the entry point's minimum or above max_h / max_w is SKIPPED: nothing of it is read,
 * tise_ssim_pairs writes NaN for it, tise_pair_sse_u8 writes 0, tise_pool2x2_pairs writes nothing.
 * LIMITS: 1 <= h, w <= TISE_SSIM_MAX_SIDE, n <= TISE_SSIM_MAX_PAIRS pairs per launch, n * tiles(max_h) * tiles(max_w) <= 2^22
 * with tiles(s) = ceil((s - 10) / TISE_SSIM_TILE); uint8 images at any address, fp32 levels 4-byte aligned, both contiguous.
 * ------------------------------------------------------------------------------------------ */
#define TISE_SSIM_TAPS 11
#define TISE_SSIM_TILE 64            /* output rows and output pixels per row of one workgroup's tile */
#define TISE_SSIM_MAX_SIDE 16384
#define TISE_SSIM_MAX_PAIRS 65535

/* One pair of a ragged launch: two (h, w, 3) images in device memory, contiguous, uint8 or fp32 as the call's is_f32 says (the
 * output table of tise_pool2x2_pairs: the two fp32 destinations and THEIR size).  24 bytes, 8-byte aligned. */
typedef struct tise_pair {
    const void* x;
    const void* y;
    int32_t h, w;
} tise_pair_t;

/* out_dev[i] = sum over the h w 3 bytes of (x - y)^2 of pair i (uint64, 8-byte aligned; zeroed by the call, then exact integer
 * atomics).  uint8 images; minimum side 1.
 * TISE_ERR_INVALID_ARG: a NULL or misaligned table or output, n < 0, max_h or max_w < 1.  TISE_ERR_UNSUPPORTED: max_h or max_w
 * above TISE_SSIM_MAX_SIDE, n above TISE_SSIM_MAX_PAIRS.  n == 0: TISE_OK, no HIP call. */
int tise_pair_sse_u8(const tise_pair_t* table_dev, int64_t n, int max_h, int max_w, uint64_t* out_dev, void* stream);

/* bytes = 48 * n * tiles(max_h) * tiles(max_w): six doubles ({ssim, cs} x {R, G, B}) per pair and tile of the largest pair.
 * TISE_ERR_INVALID_ARG: NULL bytes, n < 0, max_h or max_w < 11.  TISE_ERR_UNSUPPORTED: the limits above. */
int tise_ssim_workspace_bytes(int64_t n, int max_h, int max_w, size_t* bytes);

/* out_dev: (n, 3, 2) doubles, [pair][channel] = {mean of the ssim map, mean of the cs map}.  is_f32 = 0: uint8 images (scale
 * 1); 1: fp32 images (the pyramid levels).  Minimum side 11.  ws_dev: 8-byte aligned scratch of at least
 * tise_ssim_workspace_bytes(n, max_h, max_w).
 * TISE_ERR_INVALID_ARG: a NULL or misaligned (8 bytes) table, output or workspace, n < 0, max_h or max_w < 11, is_f32 outside
 * {0, 1}, a workspace too small.  TISE_ERR_UNSUPPORTED: the limits above.  n == 0: TISE_OK, no HIP call. */
int tise_ssim_pairs(const tise_pair_t* table_dev, int64_t n, int max_h, int max_w, int is_f32, double* out_dev, void* ws_dev,
                    size_t ws_bytes, void* stream);

/* Both images of every pair -> fp32 (h / 2, w / 2, 3), value (a + b + c + d) * 0.25 of each whole 2 x 2 block (exact).
 * out_table_dev[i]: the two destinations of pair i and their size, which must be (h / 2, w / 2) of table_dev[i] (otherwise the
 * pair is skipped); it can be the input table of the next level's calls.  Minimum side 2.
 * TISE_ERR_INVALID_ARG: a NULL or misaligned table, n < 0, max_h or max_w < 2, is_f32 outside {0, 1}.  TISE_ERR_UNSUPPORTED: the
 * limits above.  n == 0: TISE_OK, no HIP call. */
int tise_pool2x2_pairs(const tise_pair_t* table_dev, const tise_pair_t* out_table_dev, int64_t n, int max_h, int max_w, int is_f32,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * LPIPS (VGG-16) of image PAIRS (csrc/lpips.hip, csrc/split_px.h; tise_toolbox_amd/lpips_hip.py on vgg_pairs_hip.py).  No counterpart in the reference; restated from
 * Zhang, Isola, Efros, Shechtman & Wang 2018 (the `lpips` package v0.1, net = vgg):
 *   input    8-bit RGB; x = b / 127.5 - 1, then (x - shift_c) / scale_c, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448,
 *            0.450): a 3 x 256 fp32 table the caller forms.
 *   network  torchvision VGG-16 `features`: thirteen 3 x 3 / stride 1 / padding 1 convolutions with ReLU (tise_conv_split_f16),
 *            MaxPool2d(2, 2) (floor) after blocks 1..4; taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (64, 128, 256, 512, 512
 *            channels).
 *   head     per tap and pixel n(a) = sqrt(sum_c a_c^2) + 1e-10, d = sum_c w_c (a_c / n(a) - b_c / n(b))^2; the tap's value is the
 *            mean of d over the pixels; LPIPS is the sum over the five taps.
 * The three kernels here are what stands around the convolutions.  All take n PAIRS as 2n images: 0..n-1 side one, n..2n-1 side
 * two.  LIMITS: 1 <= h, w <= TISE_LPIPS_MAX_SIDE, n <= TISE_LPIPS_MAX_PAIRS.
 * ------------------------------------------------------------------------------------------ */
#define TISE_LPIPS_MAX_SIDE 16384
#define TISE_LPIPS_MAX_PAIRS 32767
#define TISE_LPIPS_WG_PIXELS 256     /* pixels of one pair that one workgroup of the head sums */
#define TISE_LPIPS_MAX_CHANNELS 512  /* of a tap: one 8-channel chunk per lane of a wave */

/* table_dev: n records {x, y, h, w} of uint8 (h, w, 3) images at any address, ALL of the size (h, w) given here (a record of
 * another size or with a NULL image is written as zeros).  lut_dev: 3 x 256 fp32 (4-byte aligned).  out_dev: split tensor
 * (2n, h, w, 32), 16-byte aligned: channels 0..2 = lut[c][byte] in split form, channels 3..31 zero in both halves.
 * TISE_ERR_INVALID_ARG: a NULL or misaligned pointer, n < 0, h or w < 1.  TISE_ERR_UNSUPPORTED: the limits above.  n == 0: TISE_OK,
 * no HIP call. */
int tise_lpips_input_split(const tise_pair_t* table_dev, int64_t n, int h, int w, const float* lut_dev, void* out_dev, void* stream);

/* 2 x 2 / stride 2 max-pool (floor: a last odd row or column is dropped) of a channel slice of a split tensor into a channel slice
 * of another; arguments and value arithmetic as tise_maxpool3s2_split_nhwc (the maximum of the exact fp32 values hi + lo 2^-11,
 * split again).  C % 8 == 0, h, w >= 2, both tensors 16-byte aligned. */
int tise_maxpool2s2_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C, void* out_dev, int64_t out_ld,
                               int out_off, void* stream);

/* bytes = 8 * n * ceil(h w / TISE_LPIPS_WG_PIXELS): one double per pair and workgroup.
 * TISE_ERR_INVALID_ARG: NULL bytes, n < 0, h or w < 1.  TISE_ERR_UNSUPPORTED: the limits above. */
int tise_lpips_workspace_bytes(int64_t n, int h, int w, size_t* bytes);

/* One tap.  feat_dev: split tensor (2n, h, w, C), 16 <= C <= TISE_LPIPS_MAX_CHANNELS, C % 16 == 0, 16-byte aligned; w_dev: C fp32;
 * out_dev[i] += mean over the pixels of d (pair i; n doubles, 8-byte aligned: the caller zeroes them before the first tap);
 * ws_dev: 8-byte aligned scratch of at least tise_lpips_workspace_bytes(n, h, w).  hi + lo 2^-11 is formed exactly, everything
 * after it is fp64 in a fixed order, no floating-point atomics: two calls give the same bits, a pair's bits depend on its own
 * features only, an identical pair adds exactly 0.0, a pixel that is zero on both sides contributes exactly 0.
 * TISE_ERR_INVALID_ARG: a NULL or misaligned pointer, n < 0, h or w < 1, C < 16 or C % 16, a workspace too small.
 * TISE_ERR_UNSUPPORTED: the limits above, C > TISE_LPIPS_MAX_CHANNELS.  n == 0: TISE_OK, no HIP call. */
int tise_lpips_layer(const void* feat_dev, int64_t n, int h, int w, int C, const float* w_dev, double* out_dev, void* ws_dev,
                     size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * DISTS of image PAIRS (csrc/dists.hip, csrc/split_px.h; tise_toolbox_amd/dists_hip.py on vgg_pairs_hip.py).  No counterpart in the reference; restated from Ding, Ma,
 * Wang & Simoncelli 2020, "Image Quality Assessment: Unifying Structure and Texture Similarity" (the DISTS_pytorch package from
 * memory; parity with its numbers is unpinned):
 *   stage 0  the image itself, x = b / 255, 3 channels.
 *   input    (x - mean_c) / std_c, mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225): a 3 x 256 fp32 table the caller
 *            forms; tise_lpips_input_split turns the bytes into the split tensor conv1_1 reads.
 *   network  torchvision VGG-16 `features`: thirteen 3 x 3 / stride 1 / padding 1 convolutions with ReLU (tise_conv_split_f16);
 *            each of the four max-pools replaced by the L2 pool y = sqrt(conv(x^2, g, stride 2, padding 1, depthwise) + 1e-12),
 *            g = [[1,2,1],[2,4,2],[1,2,1]] / 16, zero padding, output ceil(H/2) x ceil(W/2); taps relu1_2, relu2_2, relu3_3,
 *            relu4_3, relu5_3.  Channels of the six stages: 3, 64, 128, 256, 512, 512.
 *   head     per stage, pair and channel over the h w pixels: mx, my the means, vx, vy = mean (x - mx)^2, cxy = mean (x - mx)(y - my);
 *            S1 = (2 mx my + c1) / (mx^2 + my^2 + c1), S2 = (2 cxy + c2) / (vx + vy + c2), c1 = c2 = 1e-6.
 *   score    sum over stages and channels of alpha_c (1 - S1_c) + beta_c (1 - S2_c), alpha and beta divided by (sum alpha + sum beta).
 * All calls take n PAIRS as 2n images: 0..n-1 side one, n..2n-1 side two.  LIMITS: 1 <= h, w <= TISE_DISTS_MAX_SIDE,
 * n <= TISE_DISTS_MAX_PAIRS.
 * ------------------------------------------------------------------------------------------ */
#define TISE_DISTS_MAX_SIDE 16384
#define TISE_DISTS_MAX_PAIRS 32767
#define TISE_DISTS_WG_PIXELS 512     /* pixels of one pair that one workgroup of the head sums */
#define TISE_DISTS_MAX_CHANNELS 512  /* of a stage: two channels per thread of the finishing workgroup */
#define TISE_DISTS_SUM_PIXELS 4096   /* pixels of one pair per workgroup of tise_dists_image_sums_u8 */

/* L2 (Hanning) pool, 3 x 3 / stride 2 / zero padding 1, of a channel slice of a split tensor into a channel slice of another;
 * arguments as tise_maxpool2s2_split_nhwc / tise_maxpool3s2_split_nhwc.  out = sqrt(sum over the nine taps of g (hi + lo 2^-11)^2 +
 * 1e-12): the value, its square and the weighted terms are exact in fp64, the nine terms are added in row-major tap order (a tap
 * outside the image contributes 0), then the fp64 square root, one rounding to fp32 and the split hi = fp16(v), lo = fp16((v - hi)
 * 2^11).  The output is (n, ceil(h/2), ceil(w/2), ..).  C % 8 == 0, h, w >= 1, both tensors 16-byte aligned.  The output never
 * exceeds the largest input magnitude (+ 1e-6), so the range guard of the split format is not involved. */
int tise_l2pool3s2_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C, void* out_dev, int64_t out_ld,
                              int out_off, void* stream);

/* bytes = 8 * n * C * (7 * ceil(h w / TISE_DISTS_WG_PIXELS) + 2): per pair, workgroup and channel four doubles of the first pass
 * (sum and count of pixels differing from the first, both sides) and three of the second (xx, yy, xy), per pair and channel the two means.
 * TISE_ERR_INVALID_ARG: NULL bytes, n < 0, h or w < 1, C < 16 or C % 16.  TISE_ERR_UNSUPPORTED: the limits above,
 * C > TISE_DISTS_MAX_CHANNELS. */
int tise_dists_workspace_bytes(int64_t n, int h, int w, int C, size_t* bytes);

/* One stage.  feat_dev: split tensor (2n, h, w, C), 16 <= C <= TISE_DISTS_MAX_CHANNELS, C % 16 == 0, 16-byte aligned; alpha_dev,
 * beta_dev: C doubles each, already divided by (sum alpha + sum beta); out_dev[i] += sum_c alpha_c (1 - S1_c) + beta_c (1 - S2_c) of
 * pair i (n doubles, 8-byte aligned: the caller zeroes them before the first stage); ws_dev: 8-byte aligned scratch of at least
 * tise_dists_workspace_bytes(n, h, w, C).  hi + lo 2^-11 is formed exactly, everything after it is fp64 in a fixed order, two passes
 * (the means, then the centered second moments), no floating-point atomics: two calls give the same bits, a pair's bits depend on
 * its own features only, an identical pair adds exactly 0.0, a channel that is constant over the pixels has variance and
 * covariance exactly 0, a channel that is zero on both sides adds exactly 0.
 * TISE_ERR_INVALID_ARG: a NULL or misaligned pointer, n < 0, h or w < 1, C < 16 or C % 16, a workspace too small.
 * TISE_ERR_UNSUPPORTED: the limits above, C > TISE_DISTS_MAX_CHANNELS.  n == 0: TISE_OK, no HIP call. */
int tise_dists_layer(const void* feat_dev, int64_t n, int h, int w, int C, const double* alpha_dev, const double* beta_dev,
                     double* out_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Stage 0 on the bytes.  table_dev as for tise_lpips_input_split (a record of another size or with a NULL image leaves zeros).
 * out_dev: (n, 3, 5) int64, 8-byte aligned, zeroed by the call: per pair and colour the sums over the pixels of bx, by, bx^2, by^2,
 * bx by (exact integer atomics, order-free).  The host forms S1 and S2 of the three colours from them.
 * TISE_ERR_INVALID_ARG: a NULL or misaligned pointer, n < 0, h or w < 1.  TISE_ERR_UNSUPPORTED: the limits above.  n == 0: TISE_OK,
 * no HIP call. */
int tise_dists_image_sums_u8(const tise_pair_t* table_dev, int64_t n, int h, int w, int64_t* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a6) Frechet distance.
 * Replaces calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps)
 *                                           image_realism/FID/fid_score.py:121-171
 * Tr sqrtm(S1 S2) is evaluated as sum_i sqrt(lambda_i(L^T S2 L)), S1 = L L^T: an unpivoted blocked
 * Cholesky factor when every pivot is safely positive, otherwise the diagonally pivoted one
 * (rank-revealing, runs to the last positive pivot); L^T S2 L reduced to tridiagonal form by
 * Householder reflections, eigenvalues by Sturm bisection; all fp64.
 *
 *   out_dev[0] = fid            out_dev[1] = tr sqrt(S1 S2)     out_dev[2] = |mu1-mu2|^2
 *   out_dev[3] = tr S1          out_dev[4] = tr S2              out_dev[5] = rank(L) as double
 *   out_dev[6] = number of negative eigenvalues clipped         out_dev[7] = flags as double
 *   flags: bit0 = non-finite value met (the reference's "singular product" branch, :156-160,
 *          is taken by the Python mirror on this bit), bit1 = sigma1 numerically rank deficient.
 * ------------------------------------------------------------------------------------------ */
typedef struct tise_frechet tise_frechet_t;

#define TISE_FRECHET_OUT_DOUBLES 8
#define TISE_FLAG_NONFINITE 1
#define TISE_FLAG_RANK_DEFICIENT 2

int tise_frechet_create(int d, tise_frechet_t** h);       /* allocates ~4 d*d doubles of scratch */
int tise_frechet_destroy(tise_frechet_t* h);
/* Synchronises `stream` once (to read the numerical rank back). */
int tise_frechet_distance(tise_frechet_t* h, const double* mu1_dev, const double* sigma1_dev,
                          const double* mu2_dev, const double* sigma2_dev, double diag_offset,
                          double* out_dev, void* stream);
/* Two-step form.  Tr sqrtm(S1 S2) is symmetric in its arguments and the factor of ONE covariance does not depend on
 * the other: when one side's statistics are known early -- the reference .npz of fid_score.py:200-203 -- its pivoted
 * Cholesky (tise_frechet_prefactor, any stream; synchronises THAT stream to read the rank) can overlap the network
 * passes of the other side, and tise_frechet_distance_prefactored (which waits for the factor through an event) leaves
 * only GEMM + tridiagonalisation + bisection after the last batch.  (mu_f, sigma_f) = the factored side, sigma_f the
 * same matrix that was given to tise_frechet_prefactor.  No diag_offset: on TISE_FLAG_NONFINITE the caller falls back
 * to tise_frechet_distance with the reference's eps (fid_score.py:156-160). */
int tise_frechet_prefactor(tise_frechet_t* h, const double* sigma_dev, void* stream);
int tise_frechet_distance_prefactored(tise_frechet_t* h, const double* mu_f_dev, const double* sigma_f_dev,
                                      const double* mu_o_dev, const double* sigma_o_dev, double* out_dev, void* stream);
int tise_frechet_prefactor_ms(tise_frechet_t* h, double* ms_host);   /* HIP-event duration of the last prefactor */
/* Optional phase timing of tise_frechet_distance with HIP events on the caller's stream.
 * ms_host[5] = Cholesky | GEMMs | tridiagonalisation | bisection | final reduction.
 * tise_frechet_phase_ms waits for the last recorded call to finish. */
int tise_frechet_set_profiling(tise_frechet_t* h, int on);
int tise_frechet_phase_ms(tise_frechet_t* h, double* ms_host, int* rank_host);
/* Test hook: eigenvalues (ascending, n of them) of the symmetric n x n matrix a_dev (ld = n),
 * through the same tridiagonalisation + bisection kernels.  a_dev is not modified. */
int tise_eigvalsh(tise_frechet_t* h, const double* a_dev, int n, double* w_dev, void* stream);
/* Test hook: pivoted Cholesky of sigma_dev (d x d).  lt_dev receives L^T (d x d, row k = column k
 * of L, rows >= rank zero); rank_host receives the numerical rank.  Synchronises the stream. */
int tise_pivoted_cholesky(tise_frechet_t* h, const double* sigma_dev, double* lt_dev,
                          int* rank_host, void* stream);
/* Test hook: the factor tise_frechet_prefactor left (whichever factorisation produced it).  lt_dev receives
 * L^T (d x d, row k = column k of L, rows >= rank zero); rank_host the numerical rank; unpivoted_host 1 when
 * the unpivoted factorisation produced it (L^T upper triangular, natural order), 0 for the pivoted one.
 * TISE_ERR_INVALID_ARG when nothing is prefactored.  Synchronises the stream. */
int tise_frechet_factor(tise_frechet_t* h, double* lt_dev, int* rank_host, int* unpivoted_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a8, a8', a8'') IS* reduction with temperature.
 * Replaces tf.div(logits, T); tf.nn.softmax            IS/coco/inception_score_star_coco.py:107-108
 *      and the split / KL / exp loop                    IS/coco/inception_score_star_coco.py:52-60
 *          (same loop: IS/bird/inception_score_star_bird.py:97-108, slice+T :189-194;
 *           per-row entropy form: O-IS/object_centric_inception_score.py:69-81)
 * One-pass additive form: per split k keep A_k = sum_i sum_c p_ic log p_ic and
 * B_kc = sum_i p_ic; score_k = exp(A_k/n_k - sum_c pbar_c log pbar_c).
 *
 *   split_rule 0: split k = [k*N/splits, (k+1)*N/splits)          (coco, bird)
 *   split_rule 1: split k = [k*(N/splits), (k+1)*(N/splits)), the tail is dropped   (O-IS)
 *   drop_first != 0: class 0 is discarded before the softmax       (bird, :189)
 *   acc_dev: splits * (1 + C_eff) doubles, [A_0..A_{splits-1} | B row-major]; C_eff = C - drop.
 *            Additive across calls and across GPUs (all_reduce SUM).  Caller zeroes it.
 *   ws_dev:  scratch, at least 2*rows doubles.
 *   Rows carry global indices idx_base .. idx_base + rows - 1 of an N_total-image set.
 * ------------------------------------------------------------------------------------------ */
int tise_is_update(const float* logits_dev, int64_t rows, int64_t ld, int C, double temperature,
                   int drop_first, int64_t idx_base, int64_t n_total, int splits, int split_rule,
                   double* acc_dev, double* ws_dev, void* stream);
/* out_dev: 2 + splits doubles = [mean, std (ddof 0), score_0 .. score_{splits-1}] */
int tise_is_finalize(const double* acc_dev, int C_eff, int64_t n_total, int splits, int split_rule,
                     double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * IS* temperature calibration (csrc/calibrate.hip).  One evaluation of the reference's
 * CrossEntropyLoss(logits / T, labels), its derivative in T and _ECELoss's bins on cached logits
 * (classifier_calibration/temperature_scaling.py:41,64-67,80-119); the LBFGS loop is the caller's.
 *   logits_dev  rows x ld fp32; the classes of row i are logits_dev[i*ld + c0 .. i*ld + c0 + C)
 *               (c0 = 1: the bird rule's dropped background class)
 *   labels_dev  rows int32 class indices in [0, C)
 *   edges_dev   n_bins + 1 ascending fp32 bin edges (torch.linspace(0, 1, n_bins + 1)); 1 <= n_bins <= 64
 *   out_dev     4 + 3 n_bins doubles: [sum nll, sum dnll/dT, rows with a non-finite logit, rows with a label
 *               outside [0, C), count[b], sum confidence[b], sum correct[b] (b < n_bins)]; flagged rows enter
 *               no sum.  Bitwise reproducible (fixed summation order, no atomics).
 *   ws_dev      ws_bytes >= tise_calib_workspace_bytes(rows, C, n_bins) of device scratch
 * Rejected before any HIP call (TISE_ERR_INVALID_ARG): a NULL pointer, rows < 0, C < 1, c0 < 0,
 * ld < c0 + C, n_bins outside 1..64, T <= 0 or not finite, T so small that 1 / T is not finite
 * (below 5.56e-309), T > 2^100 (the kernel's column padding relies on it), a workspace too small.
 * ------------------------------------------------------------------------------------------ */
int tise_calib_workspace_bytes(int64_t rows, int C, int n_bins, size_t* bytes);
int tise_calib_eval(const float* logits_dev, int64_t rows, int64_t ld, int c0, int C, const int32_t* labels_dev,
                    double temperature, const float* edges_dev, int n_bins, double* out_dev, void* ws_dev,
                    size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a5, epilogues) Fused channels-last fp32 epilogues around the MIOpen convolutions of the
 * InceptionV3 trunk (image_realism/FID/inception.py:59-95 via torchvision BasicConv2d = conv ->
 * BatchNorm(eval) -> ReLU, InceptionA/C/E branch_pool = avg_pool2d(3,1,1) -> 1x1 conv,
 * InceptionB/D branch_pool and the stem = max_pool2d(3,2), torch.cat of the branches).
 * BatchNorm is folded into the conv weights and the per-channel bias by the caller.
 * All tensors are NHWC fp32; x is addressed as x[pixel*x_ld + x_off + c] and out as
 * out[pixel*out_ld + out_off + c], c < C, so a kernel can read a channel slice of a fused 1x1
 * conv output and write straight into the channel slice of a block's concatenated output.
 * C, offsets and leading dimensions must be multiples of 4.
 * ------------------------------------------------------------------------------------------ */
/* out = max(x + bias, 0); may run in place (out == x, same ld/off). */
int tise_bias_relu_nhwc(const float* x_dev, int64_t x_ld, int x_off, int64_t pixels, int C,
                        const float* bias_dev, float* out_dev, int64_t out_ld, int out_off, void* stream);
/* out = max(avgpool3x3(stride 1, pad 1, count_include_pad)(x) + bias, 0) over an (n,h,w) grid. */
int tise_avgpool3_bias_relu_nhwc(const float* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C,
                                 const float* bias_dev, float* out_dev, int64_t out_ld, int out_off, void* stream);
/* out (n, (h-3)/2+1, (w-3)/2+1) = maxpool3x3(stride 2)(x); with bias_dev != NULL the input is a raw
 * conv output and max(. + bias, 0) is applied (ReLU and max commute). */
int tise_maxpool3s2_nhwc(const float* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C,
                         const float* bias_dev, float* out_dev, int64_t out_ld, int out_off, void* stream);
/* Inception-2015 graph (TensorFlow SAME pools): as tise_avgpool3_bias_relu_nhwc with count_include_pad=False -- the
 * divisor is the number of taps inside the map (4 at corners, 6 on edges, 9 inside). */
int tise_avgpool3_excl_bias_relu_nhwc(const float* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C,
                                      const float* bias_dev, float* out_dev, int64_t out_ld, int out_off, void* stream);
/* out (n, h, w) = maxpool3x3(stride 1, pad 1)(x), padding acting as -inf (Inception-2015 Mixed_7c pool branch). */
int tise_maxpool3s1p1_nhwc(const float* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C, float* out_dev,
                           int64_t out_ld, int out_off, void* stream);

/* Split-fp16 activations (v ~= hi + lo * 2^-11, the format tise_conv_split_f16 consumes and produces).
 * LAYOUT of a split tensor of C channels (C % 16 == 0): NHWC; inside a pixel the channels come in blocks of 32 with
 * the two halves of a block side by side -- [hi c0..c31 | lo c0..c31][hi c32..c63 | lo c32..c63]... (128 bytes per
 * block) -- followed, when C % 32 == 16, by one 64-byte block [hi x16 | lo x16].  A pixel is 4*C bytes, the same as
 * fp32.  `ld` arguments of split tensors are the tensor's channel count C, `off` the first channel of a slice.
 *
 * out = split(max(avgpool3x3(stride 1, pad 1, count_include_pad)(x) + bias, 0)): x is raw fp32 (n, h, w, x_ld);
 * C % 8 == 0, x_ld / x_off multiples of 4 floats, bias_dev 16-byte aligned. */
int tise_avgpool3_bias_relu_split_nhwc(const float* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C,
                                       const float* bias_dev, void* out_dev, int64_t out_ld, int out_off,
                                       void* stream);
/* 3x3 / stride 2 max pool, split tensor -> split tensor (channel slice [out_off, out_off + C) of out; C % 8 == 0). */
int tise_maxpool3s2_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w,
                               int C, void* out_dev, int64_t out_ld, int out_off, void* stream);
/* tise_avgpool3_bias_relu_split_nhwc with count_include_pad=False (divisor = taps inside the map). */
int tise_avgpool3_excl_bias_relu_split_nhwc(const float* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C,
                                            const float* bias_dev, void* out_dev, int64_t out_ld, int out_off,
                                            void* stream);
/* 3x3 / stride 1 / pad 1 max pool (padding = -inf), split tensor -> split tensor slice (n, h, w); C % 8 == 0. */
int tise_maxpool3s1p1_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w,
                                 int C, void* out_dev, int64_t out_ld, int out_off, void* stream);

/* Stem layer Conv2d_1a_3x3 (3 -> 32, 3x3, stride 2) from the fp32 NHWC input (n, h, w, 3), folded bias +
 * ReLU + fp16 split fused: out = split tensor (n, oh, ow, 32).  w_dev: [kh][kw][cin][cout] fp32 (27 x 32). */
int tise_stem_conv3x3s2_split(const float* x_dev, int n, int h, int w, const float* w_dev, const float* bias_dev,
                              void* out_dev, void* stream);
/* The same layer from the uint8 NHWC result of tise_resize_bilinear_u8 (called with dst_dev = NULL and u8_out_dev set):
 * lut_dev is the 3 x 256 fp32 table (device copy) that ToTensor + the inception.py:120-124 affine tabulate, applied
 * while loading; bit-identical to the fp32 entry point on the table's values. */
int tise_stem_conv3x3s2_split_u8(const uint8_t* x_dev, const float* lut_dev, int n, int h, int w, const float* w_dev,
                                 const float* bias_dev, void* out_dev, void* stream);
/* Round 3: the same layer on the matrix cores (K = 27 padded to 32 = one K-step of the split-precision scheme).
 * wsplit_dev: fp16 [2][32 couts][32 k] (hi plane, lo plane) of the BatchNorm-folded weights, each cout pre-scaled by a
 * power of two, in the kernel's K order: k = 16 (u / 8) + 8 h + u % 8 for half h in {0, 1} and slot u in 0..15, where
 * (h = 0, u < 9) = tap (kh 0, t = u), (0, u >= 9) = (kh 1, t = u - 9), (1, u < 9) = (kh 2, t = u), (1, u = 9, 10) = (kh 1,
 * t = 7, 8), all other slots zero; t = 3 kw + cin.  scale_dev[32] undoes the pre-scaling, bias_dev[32]; w >= 5, x_dev
 * 4-byte aligned.  Same values as the entry point above to split-precision accuracy (not the same bits). */
int tise_stem_conv3x3s2_split_u8_mfma(const uint8_t* x_dev, const float* lut_dev, int n, int h, int w, const void* wsplit_dev,
                                      const float* scale_dev, const float* bias_dev, void* out_dev, void* stream);
/* ResNet (csrc/resnet.hip, csrc/conv_pipe.hip; tise_toolbox_amd/resnet_hip.py).  No counterpart in the reference, which has no
 * residual network; tise_toolbox_amd/resnet_model.py is the definition.
 *
 * The stem: 3 -> 64 channels, 7 x 7, stride 2, ZERO padding 3 of the normalised input, on the matrix cores straight from the
 * uint8 NHWC image (n, h, w, 3) and the 3 x 256 fp32 table lut_dev.  out_dev: split tensor (n, (h-1)/2+1, (w-1)/2+1, 64) =
 * split(max(scale * conv + bias, 0)) with the range guard and ReLU of every other layer.  A tap outside the image contributes
 * exactly 0 (not lut[c][0]); no byte outside [x_dev, x_dev + n h w 3) is read; x_dev may sit at any address.
 * wsplit_dev: 28672 fp16 = [7 kh][2 s2][2 planes hi, lo][2 cout tiles t][64 lanes][8 j] of the BatchNorm-folded weights, each cout
 * pre-scaled by a power of two: entry (kh, s2, plane, t, lane, j) is the weight of cout 32 t + lane % 32 at slot
 * s = 16 s2 + 8 (lane / 32) + j of filter row kh, where slot s < 21 is tap (kw = s / 3, c = s % 3) and slots 21..31 are zero
 * (K = 7 x 32 = 224).  scale_dev[64] undoes the pre-scaling, bias_dev[64]; wsplit / scale / bias / out 16-byte aligned.
 * Three-term split scheme of tise_stem_conv3x3s2_split_u8_mfma; a fixed summation order per output element: the bits do not
 * depend on the batch position or on a second call.
 * TISE_ERR_INVALID_ARG: a NULL or misaligned pointer, n < 0, h or w < 1 (the entry's minimum is one pixel).
 * TISE_ERR_UNSUPPORTED: n oh ow >= 2^31 - 256.  n == 0: TISE_OK, no HIP call. */
int tise_stem_conv7x7s2_split_u8_mfma(const uint8_t* x_dev, const float* lut_dev, int n, int h, int w, const void* wsplit_dev,
                                      const float* scale_dev, const float* bias_dev, void* out_dev, void* stream);
/* The input of the same layer when it runs as a 32-channel tise_conv_split_f16 layer instead: (n, h, w, 3) uint8 at any address
 * -> split tensor (n, h, w, 32), 16-byte aligned: channels 0..2 = lut[c][byte] in split form, channels 3..31 zero in both halves
 * (tise_lpips_input_split on one contiguous batch).  TISE_ERR_INVALID_ARG: a NULL or misaligned pointer, n < 0, h or w < 1.
 * TISE_ERR_UNSUPPORTED: n > 65535, h w > 2^27. */
int tise_resnet_input_split(const uint8_t* x_dev, const float* lut_dev, int n, int h, int w, void* out_dev, void* stream);
/* The end of a bottleneck block, split(max((raw + bias) + identity, 0)) on `pixels` pixels of C channels:
 *   t = raw + bias                  raw_dev: fp32 NHWC (pixels, raw_ld), channels [raw_off, raw_off + C): tise_conv_split_f16's
 *                                   mode-1 output (scale * conv, no bias); bias_dev: C fp32
 *   u = hi + lo 2^-11 (exact)       id_split_dev: split tensor (pixels, id_ld), channels from id_off;  OR
 *   u = id_raw + id_bias            id_raw_dev: fp32 NHWC (pixels, id_raw_ld) from id_raw_off, id_bias_dev: C fp32 (the downsample
 *                                   convolution's mode-1 output).  Exactly one of id_split_dev / id_raw_dev is non-NULL.
 *   v = t + u                       fp32, in this order, nothing fused
 *   out = split(max(v, 0))          out_dev: split tensor (pixels, out_ld), channels from out_off
 * The range guard is raised where v is NaN or |v| > 65504, tested before the max (a non-finite input cannot leave as 0 unseen).
 * C % 8 == 0; split ld % 16 == 0, off % 8 == 0; fp32 ld % 4 == 0, off % 4 == 0; off + C <= ld; all pointers 16-byte aligned;
 * out_dev equal to an input pointer is refused.  No atomics on values; the bits do not depend on the position in the batch.
 * TISE_ERR_INVALID_ARG: any of the above.  TISE_ERR_UNSUPPORTED: pixels C / 8 >= 2^39.  pixels == 0: TISE_OK, no HIP call. */
int tise_residual_relu_split_nhwc(const float* raw_dev, int64_t raw_ld, int raw_off, const float* bias_dev, const void* id_split_dev,
                                  int64_t id_ld, int id_off, const float* id_raw_dev, int64_t id_raw_ld, int id_raw_off,
                                  const float* id_bias_dev, int64_t pixels, int C, void* out_dev, int64_t out_ld, int out_off,
                                  void* stream);
/* 3 x 3 / stride 2 / padding 1 max-pool, padding ignored (-inf), of a channel slice of a split tensor into a channel slice of
 * another: (n, h, w) -> (n, (h-1)/2+1, (w-1)/2+1).  Arguments and value arithmetic as tise_maxpool3s2_split_nhwc (the maximum of
 * the exact fp32 values hi + lo 2^-11, split again).  C % 8 == 0, h, w >= 1, both tensors 16-byte aligned and distinct. */
int tise_maxpool3s2p1_split_nhwc(const void* x_dev, int64_t x_ld, int x_off, int n, int h, int w, int C, void* out_dev,
                                 int64_t out_ld, int out_off, void* stream);
/* Global average of a split tensor (n, hw, C), C % 32 == 0 -> fp32 (n, C): AdaptiveAvgPool2d((1,1)) of the last block. */
int tise_split_mean_nhwc(const void* x_dev, int n, int hw, int C, float* out_dev, void* stream);
/* the same mean, also written as a split row (n, 2C) fp16 (layout above): the operand of the classifier layer, which runs
 * as a 1x1 split-precision convolution on it (the IS* logits: pool3 x W, inception_score_star_coco.py:104-105) */
int tise_split_mean_both_nhwc(const void* x_dev, int n, int hw, int C, float* out_dev, void* out_split_dev, void* stream);
/* A channel slice of a split tensor (n, hw, C) (layout above; C % 16 == 0) as fp32 rows: the only way a feature MAP leaves
 * the split trunk (sFID's 17 x 17 x 7 tap of Mixed_6d).  out[i, p * nc + j] = float(hi) + float(lo) * 2^-11 of channel
 * c0 + j of pixel p -- exact in fp32, the value conv_split.merge gives -- in h, w, c order; columns [hw * nc, ld) of every
 * row are written as 0.  The slice may cross a 32-channel block boundary and reach into the 16-wide tail.
 * ld < hw * nc, c0 < 0, nc <= 0, c0 + nc > C: TISE_ERR_INVALID_ARG. */
int tise_split_tap_rows(const void* x_dev, int n, int hw, int C, int c0, int nc, float* out_dev, int64_t ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * The head of counting alignment, CA (csrc/countseg.hip; tise_toolbox_amd/countseg_hip.py).  counting_alignment/CA.py:120-128 and
 * :150-187 define the metric; its network (nest.modules.fc_resnet50(channels=240) under peak_response_mapping with the median
 * filter) is restated from Cholakkal, Sun, Khan & Shao 2019, "Object Counting and Instance Segmentation with Image-level
 * Supervision", and the PRM package of Zhou et al. 2018; tise_toolbox_amd/countseg_model.py is the plain torch module.
 *
 * mix_dev: the RAW fp32 result of the 1 x 1 mix convolution (tise_conv_split_f16 mode 1: scale * conv, no bias), NHWC
 * (n, h, w, ld), channels [off, off + 2 P).  With T_k = fp32(mix_k + b_mix[k]), k < 2 P, per image, class c < C and pixel p:
 *   M_c(p) = b_cls[c] + sum_{k < P} W_cls[c][k] T_k(p)          the class map          fp64, k ascending (each product is exact)
 *   D_c(p) = b_den[c] + sum_{k < P} W_den[c][k] T_{P+k}(p)      the density map
 *   p is a local maximum of M_c iff M_c(q) < M_c(p) for every 8-neighbour q inside the map before p in row-major order and
 *     M_c(q) <= M_c(p) for every one after it (max_pool2d(3, stride 1, padding -inf) returns p's own index)
 *   med = the value of ascending rank (h w - 1) / 2 of M_c (the lower median, torch.median); peaks = the local maxima >= med
 *   conf[i][c]  = (sum over the peaks of M_c(p), row-major) / #peaks;  peaks[i][c] = #peaks (>= 1)
 *   den[i][c]   = (sum_p D_c(p), row-major) / (h w)
 *   a NaN anywhere in M_c: conf[i][c] = NaN, peaks[i][c] = 0; nothing else is touched.
 * maps_dev: NULL, or fp64 (n, 2 C, h w): M_0 .. M_{C-1}, D_0 .. D_{C-1} of every image.  All comparisons on the fp64 values; no
 * floating-point atomics; the same bits in any batch, position or call.  One launch; no workspace.
 * b_mix_dev: 2 P fp32; w_cls_dev, w_den_dev: (C, P) fp32; b_cls_dev, b_den_dev: C fp32; conf_dev, den_dev: (n, C) fp64;
 * peaks_dev: (n, C) int32.  mix_dev 16-byte aligned, ld % 4 == 0, off % 4 == 0, P % 4 == 0, off + 2 P <= ld; fp32 and int32 arrays
 * 4-byte, fp64 arrays 8-byte aligned.
 * TISE_ERR_INVALID_ARG: a NULL (but maps_dev) or misaligned pointer, n < 0, h or w < 1, P < 4, C < 1, the rules above.
 * TISE_ERR_UNSUPPORTED, before any HIP call: h w > TISE_COUNTSEG_MAX_PIXELS (the maps of a class group stay in the LDS of one
 * CU), P > TISE_COUNTSEG_MAX_WIDTH, C > TISE_COUNTSEG_MAX_CLASSES, n > TISE_COUNTSEG_MAX_IMAGES.  n == 0: TISE_OK, no HIP call. */
#define TISE_COUNTSEG_MAX_PIXELS 1024
#define TISE_COUNTSEG_MAX_WIDTH 1024
#define TISE_COUNTSEG_MAX_CLASSES 4096
#define TISE_COUNTSEG_MAX_IMAGES 65535
#define TISE_COUNTSEG_CLASS_GROUP 4   /* classes of one image per workgroup */
int tise_countseg_head(const float* mix_dev, int64_t ld, int off, const float* b_mix_dev, const float* w_cls_dev,
                       const float* b_cls_dev, const float* w_den_dev, const float* b_den_dev, int64_t n, int h, int w, int P, int C,
                       double* conf_dev, double* den_dev, int* peaks_dev, double* maps_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a11, section 8 f3) Top-1 text retrieval for R-precision and the 2-way softmax test of PA.
 * Replaces the tail of the per-item loop of text_relevance/RP_coco.py:72-78 (logits_per_image ->
 * softmax -> argmax == 0) and positional_alignment/PA.py:37-42 (softmax[0] > 0.6) for n items at once.
 * img_emb: (n, d); txt_emb: a table of DISTINCT caption embeddings (rows, d); txt_index: (n, c) int32 rows of
 * that table, candidate 0 = the true caption (NULL: item i's candidates are table rows i*c .. i*c+c-1).
 * dtype 0 = fp32, 1 = fp16 embeddings; normalize != 0 divides by both norms (cosine), 0 takes the dot product
 * of already normalised features as CLIP.forward does.  Every intermediate CLIP.forward stores (normalised and
 * scaled image features, logits) and the softmax output are rounded to the embeddings' dtype, fp32 arithmetic
 * inside, as torch does for the fp16 model clip.load serves on a GPU: top1_out[i] = FIRST maximum of the rounded
 * softmax (np.argmax of the reference: near-ties go to candidate 0), p0_out (nullable) = its entry 0.  c <= 1024.
 * ------------------------------------------------------------------------------------------ */
int tise_cosine_top1(const void* img_emb_dev, const void* txt_emb_dev, const int32_t* txt_index_dev, int64_t n, int c,
                     int d, int dtype, int normalize, float logit_scale, int32_t* top1_out_dev, float* p0_out_dev,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * (a11, section 8 f3) The CLIP ViT-B/32 towers (third-party `clip`, called per item by text_relevance/RP_coco.py:56-80
 * and positional_alignment/PA.py:33-43), batched: fp16 tensors, fp32 accumulation and statistics -- the arithmetic of
 * the fp16 model `clip.load` serves on a GPU.  Row-major matrices with explicit leading dimensions (elements).
 *   tise_gemm_f16        out[m][n] = act(sum_k a[m][k] w[n][k] + bias[n]) + residual[m][n]     (nn.Linear layout of w;
 *                        act 0 = none, 1 = QuickGELU x*sigmoid(1.702x); bias / residual nullable; k % 64 == 0,
 *                        n % 8 == 0, leading dimensions % 8 == 0, lda / ldw >= k, ldo / ldr >= n; a / w / residual / out
 *                        16-byte aligned, bias 8-byte aligned)
 *   tise_layernorm_f16   per row over C <= 1024 columns (C, ldx, ldo multiples of 8, ldx / ldo >= C; 16-byte aligned pointers), fp32 mean / variance (clip.model.LayerNorm)
 *   tise_attention_f16   qkv [batch*seq][3*heads*64] (q | k | v) -> out [batch*seq][heads*64], softmax(q k^T / 8) v per
 *                        (sequence, head), optional causal mask (text tower); seq <= 96, head_dim == 64, qkv / out
 *                        16-byte aligned
 *   tise_patchify_f16    image (batch, 3, res, res) NCHW -> [batch*(res/patch)^2][3*patch*patch], columns in the order of
 *                        conv1.weight.flatten(1): the patch embedding becomes one tise_gemm_f16 (patch % 8 == 0; image /
 *                        out 16-byte aligned)
 *   tise_attention_long_f16  the same layout and result for ANY seq >= 1, non-causal: keys stream in tiles of
 *                        tise_attention_long_key_tile() under an online softmax with the exact running maximum; a workgroup
 *                        of 4 waves serves 128 consecutive queries of one (sequence, head) and stages each K / V tile once
 *                        in LDS (the image tower of ViT-L/14@336: 577 tokens); head_dim == 64, or 80 (open_clip ViT-H/14: five
 *                        K-steps of 16, the fp32 scale nearest 1 / sqrt(80), a third output tile whose columns >= 80 are never
 *                        stored), any other head_dim is refused; qkv / out 16-byte aligned (then so is every head's q, k and v)
 *   tise_patchify_pad_f16  tise_patchify_f16's matrix for any patch >= 1 with res % patch == 0, rows padded to kpad columns
 *                        (kpad >= 3*patch*patch, kpad % 64 == 0: tise_gemm_f16's K-step), the padding written as +0;
 *                        image 2-byte, out 16-byte aligned
 *   tise_vit_tokens_f16  x[b][0] = class_emb + pos[0]; x[b][1+p] = patch_out[b*n_patches+p] + pos[1+p]
 *   tise_text_tokens_f16 x[r] = table[tokens[r]] + pos[r % seq]
 *   tise_gather_rows_f16 out[i] = x[index[i]]   (class token of every image / end-of-text token of every caption)
 * ------------------------------------------------------------------------------------------ */
int tise_gemm_f16(const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, const void* res_dev,
                  int64_t ldr, void* out_dev, int64_t ldo, int m, int n, int k, int act, void* stream);
int tise_layernorm_f16(const void* x_dev, int64_t ldx, const void* gamma_dev, const void* beta_dev, void* out_dev, int64_t ldo,
                       int64_t rows, int C, float eps, void* stream);
int tise_attention_f16(const void* qkv_dev, int batch, int seq, int heads, int head_dim, int causal, void* out_dev, void* stream);
int tise_patchify_f16(const void* img_dev, int batch, int res, int patch, void* out_dev, void* stream);
int tise_attention_long_key_tile(void);
int tise_attention_long_f16(const void* qkv_dev, int batch, int seq, int heads, int head_dim, void* out_dev, void* stream);
int tise_patchify_pad_f16(const void* img_dev, int batch, int res, int patch, int kpad, void* out_dev, void* stream);
int tise_vit_tokens_f16(const void* patch_out_dev, const void* class_emb_dev, const void* pos_emb_dev, int batch, int n_patches,
                        int width, void* x_dev, void* stream);
int tise_text_tokens_f16(const int32_t* tokens_dev, const void* table_dev, const void* pos_emb_dev, int64_t rows, int seq, int width,
                         void* x_dev, void* stream);
int tise_gather_rows_f16(const void* x_dev, const int64_t* index_dev, int64_t n, int width, void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * The DINOv2 ViT tower (FD-DINOv2, tise_toolbox_amd/dinov2_hip.py): what torch.autocast(fp16) computes -- fp16 operands on the
 * matrix cores, fp32 accumulation, an FP32 RESIDUAL STREAM, LayerNorm from fp32, fp32 features.  Attention, the patch matrix
 * and the fp16 GEMMs are the entries above.
 *   tise_gemm_f16_act    tise_gemm_f16 -- the same kernels, arguments and refusals -- with one more activation: act 2 = exact
 *                        GELU 0.5 v (1 + erff(v / sqrt 2)), applied in fp32 before the one fp16 rounding as QuickGELU is
 *                        (-inf gives -0, +inf +inf, NaN NaN); act 0 and 1 give tise_gemm_f16's bits.  tise_gemm_f16 itself
 *                        keeps refusing every act but 0 and 1.  Under the default instance rule an act 2 launch stays on a
 *                        128 x 128 kernel (the erff epilogue needs the second workgroup of a CU to hide under).
 *   tise_gemm_f16_res32  out32[m][n] = res32[m][n] + scale[n] * (sum_k a[m][k] w[n][k] + bias[n]): the kernels, main loops and
 *                        instance rule of tise_gemm_f16 (TISE_GEMM_BIG / TISE_GEMM_SHAPE included) with another epilogue;
 *                        everything after the fp32 accumulator stays fp32 (one add for the bias, one multiply, one add, each
 *                        rounded once, no fma).  a / w / bias as tise_gemm_f16 (fp16; bias nullable); scale fp32 [n],
 *                        nullable (= 1); res32 / out32 fp32, never null, leading dimensions in elements, % 4 == 0 and >= n.
 *                        out32 == res32 with ldo == ldr is allowed (the tower updates its stream in place); any other
 *                        overlap is undefined.  k % 64 == 0, n % 8 == 0; a / w / scale / res32 / out32 16-byte aligned,
 *                        bias 8-byte aligned.
 *   tise_layernorm_f32   tise_layernorm_f16 on an fp32 row with fp32 gamma / beta, eps inside the square root;
 *                        out_f32 0: fp16 rows (ldo % 8 == 0) for the next GEMM, 1: fp32 rows (ldo % 4 == 0), the features.
 *                        C <= 1024, C % 8 == 0, ldx % 4 == 0, ldx / ldo >= C, 16-byte aligned pointers.
 *   tise_vit_tokens_f32  x[b][0] = class_tok + pos[0]; x[b][1+p] = float(patch_out[b*n_patches+p]) + pos[1+p]: fp16 rows of
 *                        the patch GEMM, fp32 class row and position table, fp32 tokens (one fp32 add per element)
 *   tise_gather_rows_f32 out[i] = x[index[i]], fp32 rows (the class token of every image)
 * ------------------------------------------------------------------------------------------ */
int tise_gemm_f16_act(const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, const void* res_dev,
                      int64_t ldr, void* out_dev, int64_t ldo, int m, int n, int k, int act, void* stream);
int tise_gemm_f16_res32(const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, const void* scale_dev,
                        const void* res32_dev, int64_t ldr, void* out32_dev, int64_t ldo, int m, int n, int k, void* stream);
int tise_layernorm_f32(const void* x_dev, int64_t ldx, const void* gamma_dev, const void* beta_dev, void* out_dev, int64_t ldo,
                       int64_t rows, int C, float eps, int out_f32, void* stream);
int tise_vit_tokens_f32(const void* patch_out_dev, const void* class_tok_dev, const void* pos_emb_dev, int batch, int n_patches,
                        int width, void* x_dev, void* stream);
int tise_gather_rows_f32(const void* x_dev, const int64_t* index_dev, int64_t n, int width, void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * CLIPScore on an open_clip ViT-H/14 tower (tise_toolbox_amd/clip_score.py, openclip_model.py): head width 80 is
 * tise_attention_long_f16 above, exact GELU is tise_gemm_f16_act; the two entries the tower and the score add:
 *   tise_layernorm_wide_f16  tise_layernorm_f16 -- the same parameters, two-pass fp32 statistics and rsqrtf -- for rows of up to
 *                        2048 columns (C % 8 == 0; ViT-H/14: 1280): four 16-byte groups per lane instead of two.
 *                        tise_layernorm_f16 / _f32 keep refusing C > 1024.
 *   tise_paired_cosine   out_cos[i] = (a_i . b_i) / sqrt((a_i . a_i)(b_i . b_i)) of row i of two contiguous (n, d) tables, fp16
 *                        (is_f16 1) or fp32 (0): fp64 products and sums in a fixed order (lane-strided partial sums, then a
 *                        butterfly), one wave per row, no atomics -- two launches give the same bits.  A zero row gives NaN.
 *                        n >= 0, d >= 1; tables aligned to their element, out_cos (n doubles) to 8 bytes.
 * ------------------------------------------------------------------------------------------ */
int tise_layernorm_wide_f16(const void* x_dev, int64_t ldx, const void* gamma_dev, const void* beta_dev, void* out_dev, int64_t ldo,
                            int64_t rows, int C, float eps, void* stream);
int tise_paired_cosine(const void* img_dev, const void* txt_dev, int64_t n, int d, int is_f16, double* out_cos_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a5, convolution) Implicit-GEMM convolution on fp16 MFMA with 3-term split-precision operands.
 * Replaces the Conv2d + BatchNorm(eval) + ReLU of torchvision's BasicConv2d for split tensors (layout above;
 * v ~= hi + lo * 2^-11): D = max(scale * conv(x, w) + bias, 0), re-split and written
 * into up to four destination channel slices (mode 0), or raw fp32 scale*conv (mode 1, pool branch).
 * `args` points to a host-side tise_conv_args (copied into the launch).  `tn` = tile width | kernel variant:
 * the low four bits give the output tile, 128 pixels x 32*tn channels with tn in {1..5}; weights and
 * scale/bias must be padded to a multiple of 32*tn rows and of 32 in K.
 * Variant bits (same arithmetic; 16 and 128 give bit-identical results when Cin % 32 == 0):
 *   16   direct-to-LDS DMA, two stages, addresses recomputed per K-step (generic form: the reference kernel of
 *        the tests, also serves M >= 2^31); weights fp16 [2][Cout_pad][Kpad] (hi plane, lo plane w_plane further)
 *        K = (kh, kw, cin) with cin fastest.
 *   128  DMA with the address arithmetic hoisted out of the K loop (the default of the Python layer; M < 2^31,
 *        H, W < 16128); weights fp16 [Cout_pad][Kpad / 32][hi x32 | lo x32], K order (tap, 32-channel block) for
 *        all taps, then -- Cin % 32 == 16 -- the 16-channel tails two taps per 32-wide step.
 *   64   row-window kernel for stride-1 layers with KW in 2..8 (the kw taps of a filter row share one fetch of the
 *        pixel operand); tn in {2, 3, 4}; weights fp16 [Cout_pad][Kpad / 32][hi x32 | lo x32] in the K order
 *        (kh, 32-channel block, kw), and per kh -- Cin % 32 == 16 -- the 16-channel tails two taps per 32-wide step
 *        last.  Same accuracy as 16 / 128, not the same bits (fp32 summation order).
 *   512  | 34: conv_pipe.hip configuration 34, register-resident-weights sliding-window kernel for Cin = 32, 3x3,
 *        stride 1, Cout = 32 or 64; weights as for 16.
 *   256  (round 3) POOLED INPUT: the convolution (1x1, stride 1, no padding, Cin % 32 == 0, weights as for 128) reads
 *        max_pool2d(x, 3, stride 2): args->H, W describe the UN-pooled tensor x, args->OH, OW the pooled grid
 *        ((H - 3) / 2 + 1), which is also the output grid; M = N * OH * OW; the low bits of tn are ignored (tiles of 64 pixels x 128 couts when
 *        Cout <= 128, else x 256 couts; weights, scale and bias zero-padded to that many rows).  The pool is taken while
 *        the pixel operand is loaded (torchvision's MaxPool2d(3, 2) before Conv2d_3b_1x1 and before Mixed_5b,
 *        image_realism/FID/inception.py:61-71); bit-identical to tise_maxpool3s2_split_nhwc followed by variant 128.
 *   Round 4 modifiers (OR-ed into `tn`):
 *   1024 with 512 | 34 (64 couts, unpadded: Conv2d_2b on its zero-bordered input): max_pool2d(3, stride 2) of the RESULT is
 *        taken in the epilogue (image_realism/FID/inception.py:63-65) and only the pooled split tensor
 *        N x ((OH - 3) / 2 + 1) x ((OW - 3) / 2 + 1) is written; split segments only; 128 <= W, LDS-bounded (~W <= 152).
 *   2048 with 64 (tile width 3): the HORIZONTAL half of that pool in the row-window kernel's epilogue -- destinations
 *        N x OH x ((OW - 3) / 2 + 1) (Conv2d_4a, inception.py:69-70); with 256: the pooled-input kernel takes the three
 *        VERTICAL taps of such an input (H = the producer's rows, W = OW = its pooled columns).  Both halves together are
 *        bit-identical to tise_maxpool3s2_split_nhwc of the stored result.
 *   4096 with 128: K order (32-channel block, tap) instead of (tap, block); unpadded layers with Cin % 32 == 0 and more
 *        than one tap, weights packed in that order (the stride-2 3x3 layers of Mixed_6a / 7a: their tap-shifted re-reads
 *        hit L2).  Same products, another summation order than variant 16 / 128.
 *   (Round 1's variants 0 / 32 and the other pipe configurations tied with 128 and were removed.)
 * Bits 8..13 of args->nseg are measurement switches (tools/conv_ablate.py, tools/conv_stamps.py; 0x2000: the epilogue
 * converts and stages but does not store) and must be zero in product calls.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int c0, c1;             /* output-channel range [c0, c1) of this segment (c0 % 8 == 0)             */
    void* dst;              /* mode 0: split tensor (layout above); mode 1: float*                     */
    long long ld;           /* mode 0: channel count C of the destination tensor (a pixel is 4*C bytes);
                               mode 1: destination floats per pixel                                    */
    int off;                /* first destination channel (mode 0: % 8 == 0, mode 1: % 4 == 0)          */
    int mode;
} tise_conv_seg;

typedef struct {
    const void* x;          /* split tensor [N][H][W][Cin], layout above                               */
    const void* w;          /* fp16 weights, K = (kh, kw, cin) in the order described above            */
    long long w_plane;      /* variants 16 / 512: elements between the hi and lo weight planes         */
    const float* scale;     /* [Cout_pad] un-scaling of the (power-of-two pre-scaled) weights          */
    const float* bias;      /* [Cout_pad]                                                              */
    int N, H, W, Cin, KH, KW, SH, SW, PH, PW, OH, OW;
    int Cout, K, Kpad;
    long long M;            /* N*OH*OW                                                                 */
    int nseg;
    tise_conv_seg seg[4];
    /* Variant 512|34 only (the one configuration tise_conv_pipe_launch accepts; 0 everywhere else): write the (OH, OW) result INTO a larger
     * destination image of out_hp x out_wp pixels per image at offset (out_y0, out_x0) -- Conv2d_2a writes into the
     * interior of a zero-bordered 149 x 149 buffer so that the padded Conv2d_2b runs as a valid convolution with no
     * per-lane tap masks.  out_hp = 0: the destination is the plain (OH, OW) image. */
    int out_hp, out_wp, out_y0, out_x0;
} tise_conv_args;

int tise_conv_split_f16(const tise_conv_args* args, int tn, void* stream);

/* Range guard of the split format: every kernel that writes split tensors (the convolution epilogues, the stem
 * convolution, the average-pool tail) raises a per-device flag when a value it converts exceeds the fp16 range
 * (65504; it would become +inf in the hi half) or is NaN.  Reads the flag into *flag_host (0 / 1), clears it and
 * synchronises `stream`.  The Python mirror calls it once per image set and raises FloatingPointError. */
int tise_split_overflow_check(int* flag_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp64 GEMM building block (MFMA v_mfma_f64_16x16x4_f64), exported for tests/bench only:
 * C[m][n] (ldc) = sum_k A(m,k) * B(k,n) with A(m,k) = a[m*sam + k*sak], B(k,n) = b[k*sbk + n*sbn].
 * ------------------------------------------------------------------------------------------ */
int tise_gemm_f64(const double* a_dev, int64_t sam, int64_t sak, const double* b_dev, int64_t sbk,
                  int64_t sbn, double* c_dev, int64_t ldc, int m, int n, int k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TISE_HIP_H */
