// (a2) JPEG reconstruction on the device: the second half of ``Image.open(f).convert("RGB")`` of the reference's
// Dataset.__getitem__ (image_realism/FID/img_data.py:19-25; third-party Pillow -> libjpeg-turbo) for JPEG files.  The feed's
// decode threads only parse markers and Huffman-decode a file into a slot (csrc/jpeg_decode.c: tise_jpeg_entropy_decode,
// layout in include/tise_jpeg.h); the slots travel to HBM as they are and the two kernels below do what is data-parallel:
//
//   A  jpeg_idct_kernel: dequantise + the accurate integer IDCT (13-bit constants, 2 extra bits between the passes,
//      columns then rows, +128, clamp).  ONE 8x8 BLOCK PER GROUP OF 8 LANES: lane r loads row r of the coefficients as one
//      16-byte vector, the transposes before and after the column pass go through LDS (rows padded to 9 words: the 8 lanes
//      of a group and the 8 groups of a wave fall on different banks), and lane r writes the 8 samples of row r of the block
//      into its component plane as one 8-byte store.
//   B  jpeg_colour_kernel: chroma upsampling ("fancy" triangle filter for 2x1 and 2x2 luma sampling, edges at the
//      component's DOWNSAMPLED size, replication for planes at most 2 samples wide), YCbCr -> RGB in 16-bit fixed point,
//      crop to w x h; one thread per 4 output pixels, 12 bytes written as three dwords where the address allows it.
//
// All integer, so the result equals Pillow's byte for byte (tests/test_gpu_jpeg.py); csrc/jpeg_decode.c holds the scalar
// restatement (tise_jpeg_reconstruct_slot_rgb8) and the notes on where the vectorised libjpeg-turbo is followed.
// Images of different sizes share one launch: blockIdx.y is the image, blockIdx.x walks the largest image's work and
// blocks beyond an image's own work leave at once.  HBM-bound: 2 bytes of coefficients in, 1 byte of plane out and in
// again, at most 3 bytes out per sample.  Measured (tools/jpeg_kernel_probe.py, profiles/r07b_jpeg_kernel_stats.txt): 0.418 ms per
// 1000 images of 256 x 256 = 1.41 TB/s, 0.27 of a device-to-device copy; B takes 3.5 x the time of A (its per-pixel byte loads of
// the chroma neighbours) -- 0.036 ms per loader batch of 50 beside a trunk that needs 1.9 ms for them.
//
// The kernels index with what the HOST validated: tise_jpeg_reconstruct_rgb8 checks every slot header (in the caller's
// host copy) against the slot size, the output buffer and the workspace, and hands the geometry over in a device table of
// its own -- the kernels never read a size from a slot.  Only the quantisation tables (any byte is harmless) come from
// the slot in HBM.
#include "common.h"

#include <vector>

namespace {

constexpr int HDR = 256;                  // include/tise_jpeg.h: TISE_JPEG_SLOT_HDR

struct JpegImg {                          // one image of a launch (device table, 64 bytes)
    int64_t slot_off;                     // byte offset of the slot in slots_dev
    int64_t out_off;                      // byte offset of the image in dst_dev
    int64_t plane_off;                    // byte offset of its component planes in the workspace
    int32_t mode, w, h, ncomp, hs, vs;
    int32_t bw0, bh0, bwc, bhc;           // blocks per row / column: luma, chroma
};
static_assert(sizeof(JpegImg) == 64, "device table entry");

constexpr int C_0_298 = 2446, C_0_390 = 3196, C_0_541 = 4433, C_0_765 = 6270, C_0_899 = 7373, C_1_175 = 9633, C_1_501 = 12299,
              C_1_847 = 15137, C_1_961 = 16069, C_2_053 = 16819, C_2_562 = 20995, C_3_072 = 25172;

// a sum the vectorised libjpeg-turbo keeps in a 16-bit lane (v_bfe_i32; csrc/jpeg_decode.c says where and why)
__device__ __forceinline__ int w16(int x) { return (int)(short)(x & 0xffff); }

// One 1-D pass.  The sums are formed in UNSIGNED arithmetic (two's-complement wrap is defined there; the host restatement
// is compiled with -fwrapv): outside the encoder's range the row pass can exceed 32 bits, and byte-identity with the
// restatement must not rest on what the compiler does with signed overflow.  The shifts are arithmetic, on the signed value.
template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int (&in)[8], int (&out)[8]) {
    typedef unsigned U;
    const U i0 = (U)in[0], i1 = (U)in[1], i2 = (U)in[2], i3 = (U)in[3], i4 = (U)in[4], i5 = (U)in[5], i6 = (U)in[6], i7 = (U)in[7];
    U z1 = (i2 + i6) * (U)C_0_541;
    U tmp2 = z1 - i6 * (U)C_1_847, tmp3 = z1 + i2 * (U)C_0_765;
    U tmp0 = (U)w16((int)(i0 + i4)) * 8192u, tmp1 = (U)w16((int)(i0 - i4)) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = i7;
    tmp1 = i5;
    tmp2 = i3;
    tmp3 = i1;
    z1 = tmp0 + tmp3;
    U z2 = tmp1 + tmp2;
    U z3 = (U)w16((int)(tmp0 + tmp2));
    U z4 = (U)w16((int)(tmp1 + tmp3));
    const U z5 = (z3 + z4) * (U)C_1_175;
    tmp0 *= (U)C_0_298;
    tmp1 *= (U)C_2_053;
    tmp2 *= (U)C_3_072;
    tmp3 *= (U)C_1_501;
    z1 *= (U)(-C_0_899);
    z2 *= (U)(-C_2_562);
    z3 = z3 * (U)(-C_1_961) + z5;
    z4 = z4 * (U)(-C_0_390) + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr U R = 1u << (SHIFT - 1);
    out[0] = (int)(tmp10 + tmp3 + R) >> SHIFT;
    out[7] = (int)(tmp10 - tmp3 + R) >> SHIFT;
    out[1] = (int)(tmp11 + tmp2 + R) >> SHIFT;
    out[6] = (int)(tmp11 - tmp2 + R) >> SHIFT;
    out[2] = (int)(tmp12 + tmp1 + R) >> SHIFT;
    out[5] = (int)(tmp12 - tmp1 + R) >> SHIFT;
    out[3] = (int)(tmp13 + tmp0 + R) >> SHIFT;
    out[4] = (int)(tmp13 - tmp0 + R) >> SHIFT;
}

constexpr int BLOCKS_PER_WG = 32;         // 256 threads, 8 lanes per 8x8 block

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* __restrict__ slots, const JpegImg* __restrict__ table,
                                                         uint8_t* __restrict__ ws) {
    __shared__ int tile[BLOCKS_PER_WG][8][9];
    const JpegImg im = table[blockIdx.y];
    if (im.mode != 1) return;
    const int nb0 = im.bw0 * im.bh0, nbc = im.bwc * im.bhc;
    const int total = nb0 + (im.ncomp == 3 ? 2 * nbc : 0);
    if ((int)blockIdx.x * BLOCKS_PER_WG >= total) return;                 // uniform per workgroup: no barrier is skipped by a part of it
    const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int blk = blockIdx.x * BLOCKS_PER_WG + g;
    const bool live = blk < total;
    const int b = live ? blk : total - 1;                                  // lanes beyond the image shadow its last block (no store)
    const int comp = b < nb0 ? 0 : (b < nb0 + nbc ? 1 : 2);
    const int local = b - (comp == 0 ? 0 : (comp == 1 ? nb0 : nb0 + nbc));
    const int bw = comp == 0 ? im.bw0 : im.bwc;
    const uint8_t* slot = slots + im.slot_off;
    // row r of the block: 8 int16 = one 16-byte load; the quantiser row: 8 bytes
    const int4 cv = *reinterpret_cast<const int4*>(slot + HDR + (int64_t)b * 128 + r * 16);
    const uint2 qv = *reinterpret_cast<const uint2*>(slot + 64 + comp * 64 + r * 8);
    int row[8];
    {
        const int c32[4] = {cv.x, cv.y, cv.z, cv.w};
        const unsigned q32[2] = {qv.x, qv.y};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = (int)(short)((c32[i >> 1] >> ((i & 1) * 16)) & 0xffff);
            const int q = (int)((q32[i >> 2] >> ((i & 3) * 8)) & 0xffu);
            row[i] = c * q;
        }
    }
    // does the block have a coefficient outside row 0?  (the 16-bit form of the column pass differs for such blocks only
    // outside the encoder's range: csrc/jpeg_decode.c)
    const bool mine = r != 0 && (cv.x | cv.y | cv.z | cv.w) != 0;
    const unsigned long long bal = __ballot(mine);
    const int lane = threadIdx.x & 63;
    const bool ac_rows = ((bal >> (lane & ~7)) & 0xffull) != 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) tile[g][r][i] = row[i];
    __syncthreads();
    int col[8], res[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) col[i] = tile[g][i][r];                   // lane r now owns column r
    idct_1d<11>(col, res);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int sat = min(max(res[i], -32768), 32767);
        res[i] = ac_rows ? sat : (int)(short)(res[i] & 0xffff);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) tile[g][i][r] = res[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) col[i] = tile[g][r][i];                   // row r of the column pass's result
    idct_1d<18>(col, res);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lo |= (unsigned)min(max(res[i] + 128, 0), 255) << (8 * i);
        hi |= (unsigned)min(max(res[i + 4] + 128, 0), 255) << (8 * i);
    }
    if (live) {
        const int by = local / bw, bx = local - by * bw;
        uint8_t* plane = ws + im.plane_off + (int64_t)(comp == 0 ? 0 : (comp == 1 ? nb0 : nb0 + nbc)) * 64;
        *reinterpret_cast<uint2*>(plane + ((int64_t)(by * 8 + r) * bw + bx) * 8) = make_uint2(lo, hi);
    }
}

// chroma sample for output pixel (x, y); dsw / dsh: the component's downsampled size
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ pl, int pitch, int dsw, int dsh, int hs, int vs, int x, int y) {
    if (hs == 1) return pl[(int64_t)y * pitch + x];
    const int i = x >> 1;
    if (vs == 1) {
        const uint8_t* r = pl + (int64_t)y * pitch;
        if (dsw <= 2) return r[i];
        if (x & 1) return i == dsw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
        return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    if (dsw <= 2) return pl[(int64_t)cy * pitch + i];
    const int oy = min(max((y & 1) ? cy + 1 : cy - 1, 0), dsh - 1);
    const uint8_t* r0 = pl + (int64_t)cy * pitch;
    const uint8_t* r1 = pl + (int64_t)oy * pitch;
    const int cur = 3 * r0[i] + r1[i];
    if (x & 1) return i == dsw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

__device__ __forceinline__ int clamp8(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ slots, const JpegImg* __restrict__ table,
                                                           const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst) {
    const JpegImg im = table[blockIdx.y];
    const int quads = (im.w + 3) >> 2;                                     // groups of 4 pixels in a row
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= (int64_t)quads * im.h) return;
    const int y = (int)(unit / quads), x0 = (int)(unit - (int64_t)y * quads) * 4;
    const int npx = min(4, im.w - x0);
    uint8_t px[12];
    if (im.mode == 0) {                                                     // pixels decoded on the host: copied
        const uint8_t* src = slots + im.slot_off + HDR + ((int64_t)y * im.w + x0) * 3;
        for (int i = 0; i < npx * 3; ++i) px[i] = src[i];
    } else {
        const int nb0 = im.bw0 * im.bh0, nbc = im.bwc * im.bhc;
        const uint8_t* yp = ws + im.plane_off;
        const uint8_t* cbp = yp + (int64_t)nb0 * 64;
        const uint8_t* crp = cbp + (int64_t)nbc * 64;
        const int dsw = (im.w + im.hs - 1) / im.hs, dsh = (im.h + im.vs - 1) / im.vs;
        for (int i = 0; i < npx; ++i) {
            const int x = x0 + i;
            const int yv = yp[(int64_t)y * (im.bw0 * 8) + x];
            if (im.ncomp == 1) {
                px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint8_t)yv;
            } else {
                const int cb = chroma_at(cbp, im.bwc * 8, dsw, dsh, im.hs, im.vs, x, y) - 128;
                const int cr = chroma_at(crp, im.bwc * 8, dsw, dsh, im.hs, im.vs, x, y) - 128;
                px[3 * i] = (uint8_t)clamp8(yv + ((91881 * cr + 32768) >> 16));
                px[3 * i + 1] = (uint8_t)clamp8(yv + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                px[3 * i + 2] = (uint8_t)clamp8(yv + ((116130 * cb + 32768) >> 16));
            }
        }
    }
    uint8_t* o = dst + im.out_off + ((int64_t)y * im.w + x0) * 3;
    if (npx == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            o32[i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) | ((uint32_t)px[4 * i + 3] << 24);
    } else {
        for (int i = 0; i < npx * 3; ++i) o[i] = px[i];
    }
}

int rd32(const uint8_t* p) { return (int)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); }

int64_t table_bytes(int64_t n) { return (n * (int64_t)sizeof(JpegImg) + 255) & ~(int64_t)255; }

}  // namespace

extern "C" int tise_jpeg_workspace_bytes(int64_t n, int64_t slot_stride, size_t* bytes) {
    if (!bytes || n < 0 || slot_stride < HDR || (slot_stride & 15) || n > 65535) return TISE_ERR_INVALID_ARG;
    // the device table + the component planes: 64 bytes per block, a slot holds at most (slot_stride - HDR) / 128 blocks
    *bytes = (size_t)(table_bytes(n) + n * ((slot_stride - HDR) / 128) * 64);
    return TISE_OK;
}

extern "C" int tise_jpeg_reconstruct_rgb8(const uint8_t* slots_dev, int64_t n, int64_t slot_stride, const uint8_t* headers_host,
                                          int64_t header_stride, const int64_t* out_offsets_host, uint8_t* dst_dev, int64_t dst_bytes,
                                          uint8_t* ws_dev, int64_t ws_bytes, uint8_t* table_host_pinned, void* stream) {
    if (n < 0 || slot_stride < HDR || (slot_stride & 15) || header_stride < HDR || dst_bytes < 0 || ws_bytes < 0) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if (!slots_dev || !headers_host || !out_offsets_host || !dst_dev || !ws_dev) return TISE_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(slots_dev) & 15) || (reinterpret_cast<uintptr_t>(ws_dev) & 15)) return TISE_ERR_INVALID_ARG;   // 16-byte loads, 8-byte stores
    if (n > 65535) return TISE_ERR_UNSUPPORTED;                                    // grid y
    // the device table is built in the caller's page-locked scratch when there is one (an asynchronous copy: the calling
    // thread does not wait for the stream), else in a buffer of this call (a stream-ordered copy the call waits for)
    std::vector<JpegImg> own;
    JpegImg* table = reinterpret_cast<JpegImg*>(table_host_pinned);
    if (!table) {
        own.resize((size_t)n);
        table = own.data();
    } else if (reinterpret_cast<uintptr_t>(table_host_pinned) & 7) {
        return TISE_ERR_INVALID_ARG;
    }
    int64_t plane_pos = table_bytes(n);
    int64_t max_blocks = 0, max_units = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* hd = headers_host + i * header_stride;
        JpegImg& t = table[(size_t)i];
        t.mode = rd32(hd);
        t.w = rd32(hd + 4);
        t.h = rd32(hd + 8);
        t.ncomp = rd32(hd + 12);
        t.hs = rd32(hd + 16);
        t.vs = rd32(hd + 20);
        t.bw0 = rd32(hd + 24);
        t.bwc = rd32(hd + 28);
        t.bh0 = rd32(hd + 36);
        t.bhc = rd32(hd + 40);
        const int64_t payload = (int64_t)(uint32_t)rd32(hd + 48);
        if (t.w < 1 || t.h < 1 || t.w > 65535 || t.h > 65535) return TISE_ERR_INVALID_ARG;
        const int64_t pixels = (int64_t)t.w * t.h * 3;
        int64_t blocks = 0;
        if (t.mode == 0) {
            if (payload != pixels) return TISE_ERR_INVALID_ARG;
            t.ncomp = 0;
            t.hs = t.vs = 1;
            t.bw0 = t.bh0 = t.bwc = t.bhc = 0;
        } else if (t.mode == 1) {
            const bool gray = t.ncomp == 1 && t.hs == 1 && t.vs == 1;
            const bool colour = t.ncomp == 3 && ((t.hs == 1 && t.vs == 1) || (t.hs == 2 && t.vs == 1) || (t.hs == 2 && t.vs == 2));
            if (!gray && !colour) return TISE_ERR_INVALID_ARG;
            const int mx = (t.w + 8 * t.hs - 1) / (8 * t.hs), my = (t.h + 8 * t.vs - 1) / (8 * t.vs);
            if (t.bw0 != mx * t.hs || t.bh0 != my * t.vs) return TISE_ERR_INVALID_ARG;
            if (gray) {
                if (t.bwc != 0 || t.bhc != 0 || rd32(hd + 32) != 0 || rd32(hd + 44) != 0) return TISE_ERR_INVALID_ARG;
            } else if (t.bwc != mx || t.bhc != my || rd32(hd + 32) != mx || rd32(hd + 44) != my) {
                return TISE_ERR_INVALID_ARG;
            }
            blocks = (int64_t)t.bw0 * t.bh0 + (gray ? 0 : 2 * (int64_t)t.bwc * t.bhc);
            if (payload != blocks * 128 || blocks > 0x7fffffff / 128) return TISE_ERR_INVALID_ARG;
        } else {
            return TISE_ERR_INVALID_ARG;
        }
        if (HDR + payload > slot_stride) return TISE_ERR_INVALID_ARG;
        const int64_t off = out_offsets_host[i];
        if (off < 0 || off > dst_bytes || pixels > dst_bytes - off) return TISE_ERR_INVALID_ARG;
        t.slot_off = i * slot_stride;
        t.out_off = off;
        t.plane_off = plane_pos;
        plane_pos += blocks * 64;
        if (plane_pos > ws_bytes) return TISE_ERR_INVALID_ARG;
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        const int64_t units = (int64_t)((t.w + 3) / 4) * t.h;
        max_units = units > max_units ? units : max_units;
    }
    if (table_bytes(n) > ws_bytes) return TISE_ERR_INVALID_ARG;
    const int64_t gx_a = (max_blocks + BLOCKS_PER_WG - 1) / BLOCKS_PER_WG, gx_b = (max_units + 255) / 256;
    if (gx_a > 0x7fffffff || gx_b > 0x7fffffff) return TISE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (table_host_pinned) {
        TISE_HIP_CHECK(hipMemcpyAsync(ws_dev, table, (size_t)n * sizeof(JpegImg), hipMemcpyHostToDevice, st));
    } else {
        TISE_HIP_CHECK(hipMemcpyWithStream(ws_dev, table, (size_t)n * sizeof(JpegImg), hipMemcpyHostToDevice, st));
    }
    const JpegImg* table_dev = reinterpret_cast<const JpegImg*>(ws_dev);
    if (gx_a > 0) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)gx_a, (unsigned)n), dim3(256), 0, st, slots_dev, table_dev, ws_dev);
        TISE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)gx_b, (unsigned)n), dim3(256), 0, st, slots_dev, table_dev, ws_dev, dst_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}
