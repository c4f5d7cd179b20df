/*
 * libtise_jpeg.so -- host side of the JPEG image feed (plain C, gcc; no HIP, no libjpeg): marker parsing and Huffman
 * decoding of baseline / extended-sequential JPEG files (csrc/jpeg_decode.c), bound with ctypes by
 * tise_toolbox_amd/jpeg_feed.py.
 *
 * Replaces ``Image.open(f).convert("RGB")`` of the reference's Dataset.__getitem__ (image_realism/FID/img_data.py:19-25;
 * third-party Pillow -> libjpeg-turbo) for the subset below, byte for byte (tests/test_jpeg_host.py compares with the
 * installed Pillow).  Every other file gets a non-zero code and is decoded by Pillow itself.
 *
 * Subset: 8-bit Huffman SOF0 / SOF1, ONE scan holding all components; 1 component (1x1) or 3 components YCbCr (JFIF
 * marker, or Adobe marker with transform 1, or neither marker and component ids 1, 2, 3) with luma sampling 1x1, 2x1
 * or 2x2 and chroma 1x1; 8-bit quantisation tables; every |coefficient * quantiser| <= 16383; width and height at most
 * 65500 (TISE_JPEG_MAX_DIMENSION: libjpeg refuses a larger file, Pillow raises OSError for it, and so must the feed).
 */
#ifndef TISE_JPEG_H
#define TISE_JPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TISE_JPEG_OK 0
#define TISE_JPEG_UNSUPPORTED 1   /* outside the subset (progressive, arithmetic, 12-bit, CMYK, RGB ids, 4:4:0, 4:1:1, several
                                     scans, 16-bit tables, a product beyond the guard, not a JPEG): use Pillow */
#define TISE_JPEG_CORRUPT 2       /* malformed, or ANY doubt: a bad Huffman code, a coefficient index beyond 63, a missing or
                                     out-of-order restart marker, data ending early, a missing EOI -- Pillow decides or raises */
#define TISE_JPEG_SIZE 3          /* a decodable file that does not fit the slot / destination (size reported through w / h) */

/* layouts reported by tise_jpeg_probe */
#define TISE_JPEG_GRAY 0
#define TISE_JPEG_444 1
#define TISE_JPEG_422 2           /* luma 2x1 */
#define TISE_JPEG_420 3           /* luma 2x2 */

/* ---- the slot: what the host hands to tise_jpeg_reconstruct_rgb8 (libtise_hip.so, include/tise_hip.h) -------------------
 * [256-byte header | payload].  Header, little-endian int32 at byte offset:
 *    0 mode (1: payload = quantised coefficients; 0: payload = h*w*3 RGB pixels decoded on the host)
 *    4 width    8 height    12 components (1 or 3)    16 / 20 luma sampling h / v (1x1, 2x1, 2x2)
 *   24 / 28 / 32 blocks per row of component 0 / 1 / 2     36 / 40 / 44 blocks per column of component 0 / 1 / 2
 *   48 payload bytes
 *   64 + 64 c: the quantisation table of component c, 8-bit, natural (row-major) order
 * Payload (mode 1): int16[blocks][64] per component in natural (de-zigzagged) order, NOT dequantised, component planes
 * one after the other, block rows padded to whole MCUs (component c: blocks-per-column x blocks-per-row blocks, row-major). */
#define TISE_JPEG_SLOT_HDR 256
#define TISE_JPEG_MAX_PRODUCT 16383
/* libjpeg's JPEG_MAX_DIMENSION: probe / entropy_decode / decode_rgb8 answer TISE_JPEG_UNSUPPORTED above it.  (Mode-0 slots carry
 * Pillow's pixels of any file Pillow opened; tise_jpeg_reconstruct_rgb8 keeps its own bound of 65535, which is about indexing.) */
#define TISE_JPEG_MAX_DIMENSION 65500

/* slot bytes (header + coefficients, a multiple of 16) of a w x h image of `layout` */
size_t tise_jpeg_slot_bytes(int w, int h, int layout);
/* marker parse only: width, height, layout; TISE_JPEG_OK only for the subset decoded here */
int tise_jpeg_probe(const uint8_t* file, size_t len, int* w, int* h, int* layout);
/* parse + Huffman-decode `file` into `slot` (header + coefficients); *w / *h receive the size whenever the headers parse */
int tise_jpeg_entropy_decode(const uint8_t* file, size_t len, uint8_t* slot, size_t slot_bytes, int* w, int* h);
/* the scalar restatement of the device kernel: slot -> dst[h][w][3] (dequantise, integer IDCT, fancy upsampling, YCbCr -> RGB) */
int tise_jpeg_reconstruct_slot_rgb8(const uint8_t* slot, size_t slot_bytes, uint8_t* dst, size_t dst_bytes);
/* the complete decode on the host: file -> dst[h][w][3] uint8 RGB; TISE_JPEG_SIZE when dst_bytes < h*w*3 */
int tise_jpeg_decode_rgb8(const uint8_t* file, size_t len, uint8_t* dst, size_t dst_bytes, int* w, int* h);

#ifdef __cplusplus
}
#endif
#endif
