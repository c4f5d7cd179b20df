// libtise_jpeg.so: the host half of the JPEG feed (include/tise_jpeg.h).  Marker parsing and Huffman decoding -- the
// strictly serial part of a JPEG -- stay here; what is data-parallel (dequantisation, IDCT, chroma upsampling, colour
// conversion) runs in HBM (csrc/jpeg_idct.hip).  tise_jpeg_reconstruct_slot_rgb8 restates that kernel in scalar C: it
// serves host consumers and is the CPU oracle of the kernel.
//
// The arithmetic is the default decode path of libjpeg-turbo as Pillow runs it (JDCT_ISLOW, fancy upsampling, no merged
// upsampling), restated from the JPEG standard (ITU-T T.81) and libjpeg's published algorithm descriptions; no libjpeg
// source is included.  The decoder is strict where libjpeg is lenient: whatever libjpeg would only warn about is
// TISE_JPEG_CORRUPT here, and Pillow decodes the file.
#include "../../include/tise_jpeg.h"

#include <stdlib.h>
#include <string.h>

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

#define LUT_BITS 9

typedef struct {
    int defined;
    uint16_t lut[1 << LUT_BITS];     // (length << 8) | symbol for codes of up to LUT_BITS bits, 0: longer
    int32_t maxcode[18];             // largest code of each length (-1: none)
    int32_t valoff[17];              // symbol index of a code = code + valoff[length]
    uint8_t vals[256];
} huff_t;

typedef struct {
    int w, h, ncomp, hs, vs;         // hs / vs: luma sampling
    int bw[3], bh[3];                // blocks per row / column of each component (whole MCUs)
    int tq[3], td[3], ta[3];
    uint8_t qt[4][64];               // natural order
    int qt_defined[4];
    huff_t dc[4], ac[4];
    int restart;
    size_t scan;                     // offset of the entropy-coded data
} jpg_t;

static int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

static int build_huff(huff_t* t, const uint8_t* counts, const uint8_t* vals, int nvals) {
    memset(t, 0, sizeof(*t));
    memcpy(t->vals, vals, (size_t)nvals);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->valoff[l] = k - code;
        for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return TISE_JPEG_CORRUPT;             // the code space of this length is used up
            if (l <= LUT_BITS) {
                const int lo = code << (LUT_BITS - l);
                for (int j = 0; j < (1 << (LUT_BITS - l)); ++j) t->lut[lo + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        t->maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[17] = 0x7fffffff;
    t->defined = 1;
    return TISE_JPEG_OK;
}

// ---- markers --------------------------------------------------------------------------------------------------------------
static int parse_headers(const uint8_t* f, size_t len, jpg_t* j) {
    memset(j, 0, sizeof(*j));
    if (len < 4 || f[0] != 0xFF || f[1] != 0xD8) return TISE_JPEG_UNSUPPORTED;          // not a JPEG
    size_t p = 2;
    int jfif = 0, adobe = 0, adobe_tr = -1, have_sof = 0;
    int cid[3] = {0, 0, 0}, chs[3] = {0, 0, 0}, cvs[3] = {0, 0, 0};
    for (;;) {
        if (p + 4 > len || f[p] != 0xFF) return TISE_JPEG_CORRUPT;
        while (p + 1 < len && f[p + 1] == 0xFF) ++p;                                     // fill bytes
        if (p + 4 > len) return TISE_JPEG_CORRUPT;
        const int m = f[p + 1];
        p += 2;
        if (m == 0x00 || m == 0x01 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7)) return TISE_JPEG_CORRUPT;
        const int seg = be16(f + p);
        if (seg < 2 || p + (size_t)seg > len) return TISE_JPEG_CORRUPT;
        const uint8_t* d = f + p + 2;
        const int n = seg - 2;
        if (m == 0xE0) {
            if (n >= 14 && !memcmp(d, "JFIF\0", 5)) jfif = 1;
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(d, "Adobe", 5)) { adobe = 1; adobe_tr = d[11]; }
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
            // APPn, COM: skipped
        } else if (m == 0xDB) {
            int q = 0;
            while (q < n) {
                const int pq = d[q] >> 4, t = d[q] & 15;
                if (pq > 1 || t > 3) return TISE_JPEG_CORRUPT;
                if (pq == 1) return TISE_JPEG_UNSUPPORTED;                               // 16-bit table
                if (q + 65 > n) return TISE_JPEG_CORRUPT;
                for (int i = 0; i < 64; ++i) j->qt[t][ZIGZAG[i]] = d[q + 1 + i];
                j->qt_defined[t] = 1;
                q += 65;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (have_sof || n < 6) return TISE_JPEG_CORRUPT;
            if (d[0] != 8) return TISE_JPEG_UNSUPPORTED;                                 // 12-bit
            j->h = be16(d + 1);
            j->w = be16(d + 3);
            j->ncomp = d[5];
            if (j->h == 0) return TISE_JPEG_UNSUPPORTED;                                 // height from a DNL marker
            if (j->w == 0 || j->ncomp == 0) return TISE_JPEG_CORRUPT;
            if (n != 6 + 3 * j->ncomp) return TISE_JPEG_CORRUPT;
            // A SOF marker can state up to 65535, but libjpeg refuses anything above its JPEG_MAX_DIMENSION (65500) and Pillow
            // then raises OSError: the reference job fails on such a file, so it is not turned into pixels here either.
            if (j->w > TISE_JPEG_MAX_DIMENSION || j->h > TISE_JPEG_MAX_DIMENSION) return TISE_JPEG_UNSUPPORTED;
            if (j->ncomp != 1 && j->ncomp != 3) return TISE_JPEG_UNSUPPORTED;            // CMYK / YCCK / two components
            for (int c = 0; c < j->ncomp; ++c) {
                cid[c] = d[6 + 3 * c];
                chs[c] = d[7 + 3 * c] >> 4;
                cvs[c] = d[7 + 3 * c] & 15;
                j->tq[c] = d[8 + 3 * c];
                if (chs[c] < 1 || chs[c] > 4 || cvs[c] < 1 || cvs[c] > 4 || j->tq[c] > 3) return TISE_JPEG_CORRUPT;
            }
            have_sof = 1;
        } else if (m == 0xC4) {
            int q = 0;
            while (q < n) {
                if (q + 17 > n) return TISE_JPEG_CORRUPT;
                const int tc = d[q] >> 4, th = d[q] & 15;
                if (tc > 1 || th > 3) return TISE_JPEG_CORRUPT;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += d[q + 1 + i];
                if (total > 256 || q + 17 + total > n) return TISE_JPEG_CORRUPT;
                const int rc = build_huff(tc ? &j->ac[th] : &j->dc[th], d + q + 1, d + q + 17, total);
                if (rc) return rc;
                q += 17 + total;
            }
        } else if (m == 0xDD) {
            if (n != 2) return TISE_JPEG_CORRUPT;
            j->restart = be16(d);
        } else if (m == 0xDA) {
            if (!have_sof) return TISE_JPEG_CORRUPT;
            if (n < 1) return TISE_JPEG_CORRUPT;
            const int ns = d[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return TISE_JPEG_CORRUPT;
            if (ns != j->ncomp) return TISE_JPEG_UNSUPPORTED;                            // several scans
            for (int c = 0; c < ns; ++c) {
                if (d[1 + 2 * c] != cid[c]) return TISE_JPEG_UNSUPPORTED;                // another component order
                j->td[c] = d[2 + 2 * c] >> 4;
                j->ta[c] = d[2 + 2 * c] & 15;
                if (j->td[c] > 3 || j->ta[c] > 3) return TISE_JPEG_CORRUPT;
            }
            if (d[1 + 2 * ns] != 0 || d[2 + 2 * ns] != 63 || d[3 + 2 * ns] != 0) return TISE_JPEG_UNSUPPORTED;
            j->scan = p + (size_t)seg;
            break;
        } else {
            return TISE_JPEG_UNSUPPORTED;     // SOF2.. (progressive, lossless, arithmetic), DAC, DNL, DHP, EXP, JPGn, reserved
        }
        p += (size_t)seg;
    }
    // sampling and colour space
    if (j->ncomp == 1) {
        if (chs[0] != 1 || cvs[0] != 1) return TISE_JPEG_UNSUPPORTED;
        j->hs = j->vs = 1;
    } else {
        if (chs[1] != 1 || cvs[1] != 1 || chs[2] != 1 || cvs[2] != 1) return TISE_JPEG_UNSUPPORTED;
        if (!((chs[0] == 1 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 2)))
            return TISE_JPEG_UNSUPPORTED;                                                // 4:4:0, 4:1:1, ...
        j->hs = chs[0];
        j->vs = cvs[0];
        if (jfif) {
            // YCbCr
        } else if (adobe) {
            if (adobe_tr != 1) return TISE_JPEG_UNSUPPORTED;                             // RGB (0), YCCK, unknown
        } else if (!(cid[0] == 1 && cid[1] == 2 && cid[2] == 3)) {
            return TISE_JPEG_UNSUPPORTED;                                                // ids R G B, or a guess
        }
    }
    const int mx = (j->w + 8 * j->hs - 1) / (8 * j->hs), my = (j->h + 8 * j->vs - 1) / (8 * j->vs);
    j->bw[0] = mx * j->hs;
    j->bh[0] = my * j->vs;
    for (int c = 1; c < j->ncomp; ++c) { j->bw[c] = mx; j->bh[c] = my; }
    for (int c = 0; c < j->ncomp; ++c) {
        if (!j->qt_defined[j->tq[c]] || !j->dc[j->td[c]].defined || !j->ac[j->ta[c]].defined) return TISE_JPEG_CORRUPT;
    }
    return TISE_JPEG_OK;
}

static int layout_of(const jpg_t* j) {
    if (j->ncomp == 1) return TISE_JPEG_GRAY;
    return j->hs == 1 ? TISE_JPEG_444 : (j->vs == 1 ? TISE_JPEG_422 : TISE_JPEG_420);
}

static size_t nblocks(const jpg_t* j) {
    size_t n = 0;
    for (int c = 0; c < j->ncomp; ++c) n += (size_t)j->bw[c] * j->bh[c];
    return n;
}

size_t tise_jpeg_slot_bytes(int w, int h, int layout) {
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535 || layout < 0 || layout > 3) return 0;
    const int hs = layout >= TISE_JPEG_422 ? 2 : 1, vs = layout == TISE_JPEG_420 ? 2 : 1;
    const size_t mx = ((size_t)w + 8 * hs - 1) / (8 * hs), my = ((size_t)h + 8 * vs - 1) / (8 * vs);
    const size_t blocks = mx * my * (size_t)(hs * vs + (layout == TISE_JPEG_GRAY ? 0 : 2));
    return TISE_JPEG_SLOT_HDR + blocks * 128;
}

int tise_jpeg_probe(const uint8_t* file, size_t len, int* w, int* h, int* layout) {
    if (!file) return TISE_JPEG_CORRUPT;
    jpg_t* j = (jpg_t*)malloc(sizeof(jpg_t));
    if (!j) return TISE_JPEG_CORRUPT;
    const int rc = parse_headers(file, len, j);
    if (rc == TISE_JPEG_OK) {
        if (w) *w = j->w;
        if (h) *h = j->h;
        if (layout) *layout = layout_of(j);
    }
    free(j);
    return rc;
}

// ---- entropy decoding -----------------------------------------------------------------------------------------------------
typedef struct {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int bits;        // valid bits in acc (its low `bits` bits)
    int fake;        // zero bits appended after the data ran into a marker / the end of the file
    int marker;      // 0: in data; 1: p points at 0xFF of a marker; -1: end of file
} bits_t;

static void fill(bits_t* b) {
    while (b->bits <= 56) {
        unsigned c = 0;
        if (b->marker) {
            b->fake += 8;
        } else if (b->p >= b->end) {
            b->marker = -1;
            b->fake += 8;
        } else if (*b->p != 0xFF) {
            c = *b->p++;
        } else if (b->p + 1 >= b->end) {
            b->marker = -1;
            b->fake += 8;
        } else if (b->p[1] == 0) {                     // stuffed byte
            c = 0xFF;
            b->p += 2;
        } else {
            b->marker = 1;
            b->fake += 8;
        }
        b->acc = (b->acc << 8) | c;
        b->bits += 8;
    }
}

static inline unsigned peek(bits_t* b, int n) { return (unsigned)((b->acc >> (b->bits - n)) & ((1u << n) - 1u)); }

static inline int get_symbol(bits_t* b, const huff_t* t) {
    fill(b);
    const unsigned e = t->lut[peek(b, LUT_BITS)];
    if (e) {
        b->bits -= (int)(e >> 8);
        return (int)(e & 255);
    }
    for (int l = LUT_BITS + 1; l <= 16; ++l) {
        const int code = (int)peek(b, l);
        if (code <= t->maxcode[l]) {
            b->bits -= l;
            return t->vals[code + t->valoff[l]];
        }
    }
    return -1;                                         // no such code
}

static inline int get_value(bits_t* b, int s) {       // s bits, sign-extended as T.81 F.2.2.1 (EXTEND)
    fill(b);
    const int v = (int)peek(b, s);
    b->bits -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// the interval's data must end where a marker begins, with less than one byte of padding left and nothing borrowed
static int interval_end(bits_t* b) {
    if (b->bits < b->fake) return TISE_JPEG_CORRUPT;   // decoded past the data
    if (b->bits - b->fake >= 8) return TISE_JPEG_CORRUPT;
    if (b->marker < 0) return TISE_JPEG_CORRUPT;
    if (!b->marker) {
        if (b->p + 1 >= b->end || b->p[0] != 0xFF || b->p[1] == 0) return TISE_JPEG_CORRUPT;
    }
    while (b->p + 1 < b->end && b->p[1] == 0xFF) ++b->p;
    if (b->p + 1 >= b->end) return TISE_JPEG_CORRUPT;
    return TISE_JPEG_OK;
}

static int decode_block(bits_t* b, const huff_t* dc, const huff_t* ac, const uint8_t* q, int* pred, int16_t* out) {
    memset(out, 0, 128);
    int s = get_symbol(b, dc);
    if (s < 0 || s > 11) return TISE_JPEG_CORRUPT;
    if (s) *pred += get_value(b, s);
    if (*pred * (int)q[0] > TISE_JPEG_MAX_PRODUCT || *pred * (int)q[0] < -TISE_JPEG_MAX_PRODUCT || *pred > 32767 || *pred < -32768)
        return TISE_JPEG_UNSUPPORTED;
    out[0] = (int16_t)*pred;
    for (int k = 1; k < 64;) {
        const int rs = get_symbol(b, ac);
        if (rs < 0) return TISE_JPEG_CORRUPT;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;                        // EOB
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return TISE_JPEG_CORRUPT;
        const int v = get_value(b, s), z = ZIGZAG[k];
        if (v * (int)q[z] > TISE_JPEG_MAX_PRODUCT || v * (int)q[z] < -TISE_JPEG_MAX_PRODUCT) return TISE_JPEG_UNSUPPORTED;
        out[z] = (int16_t)v;
        ++k;
    }
    return TISE_JPEG_OK;
}

static void put32(uint8_t* p, int v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static int get32(const uint8_t* p) { return (int)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); }

static int decode_scan(const uint8_t* f, size_t len, const jpg_t* j, int16_t* coef) {
    bits_t b = {f + j->scan, f + len, 0, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    int16_t* plane[3];
    size_t off = 0;
    for (int c = 0; c < j->ncomp; ++c) {
        plane[c] = coef + off * 64;
        off += (size_t)j->bw[c] * j->bh[c];
    }
    const int mcux = j->bw[j->ncomp - 1], mcuy = j->bh[j->ncomp - 1];       // chroma (or the one gray plane): one block per MCU
    long done = 0;
    for (int yy = 0; yy < mcuy; ++yy) {
        for (int xx = 0; xx < mcux; ++xx, ++done) {
            if (j->restart && done && done % j->restart == 0) {
                int rc = interval_end(&b);
                if (rc) return rc;
                if (b.p[1] != 0xD0 + (int)((done / j->restart - 1) & 7)) return TISE_JPEG_CORRUPT;
                b.p += 2;
                b.acc = 0;
                b.bits = b.fake = b.marker = 0;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < j->ncomp; ++c) {
                const int ch = c == 0 ? j->hs : 1, cv = c == 0 ? j->vs : 1;
                for (int v = 0; v < cv; ++v) {
                    for (int h = 0; h < ch; ++h) {
                        const size_t blk = (size_t)(yy * cv + v) * j->bw[c] + (size_t)(xx * ch + h);
                        const int rc = decode_block(&b, &j->dc[j->td[c]], &j->ac[j->ta[c]], j->qt[j->tq[c]], &pred[c], plane[c] + blk * 64);
                        if (rc) return rc;
                    }
                }
            }
        }
    }
    const int rc = interval_end(&b);
    if (rc) return rc;
    if (b.p[1] != 0xD9) return TISE_JPEG_CORRUPT;      // EOI must follow the one scan
    return TISE_JPEG_OK;
}

static void write_header(uint8_t* slot, const jpg_t* j, size_t payload) {
    memset(slot, 0, TISE_JPEG_SLOT_HDR);
    put32(slot + 0, 1);
    put32(slot + 4, j->w);
    put32(slot + 8, j->h);
    put32(slot + 12, j->ncomp);
    put32(slot + 16, j->hs);
    put32(slot + 20, j->vs);
    for (int c = 0; c < j->ncomp; ++c) {
        put32(slot + 24 + 4 * c, j->bw[c]);
        put32(slot + 36 + 4 * c, j->bh[c]);
        memcpy(slot + 64 + 64 * c, j->qt[j->tq[c]], 64);
    }
    put32(slot + 48, (int)payload);
}

int tise_jpeg_entropy_decode(const uint8_t* file, size_t len, uint8_t* slot, size_t slot_bytes, int* w, int* h) {
    if (!file || !slot) return TISE_JPEG_CORRUPT;
    jpg_t* j = (jpg_t*)malloc(sizeof(jpg_t));
    if (!j) return TISE_JPEG_CORRUPT;
    int rc = parse_headers(file, len, j);
    if (rc == TISE_JPEG_OK) {
        if (w) *w = j->w;
        if (h) *h = j->h;
        const size_t payload = nblocks(j) * 128;
        if (payload > 0x7fffffffu || slot_bytes < TISE_JPEG_SLOT_HDR + payload || ((uintptr_t)slot & 1)) {
            rc = TISE_JPEG_SIZE;
        } else {
            rc = decode_scan(file, len, j, (int16_t*)(slot + TISE_JPEG_SLOT_HDR));
            write_header(slot, j, payload);
            if (rc) put32(slot + 0, -1);               // never a header the kernel would take
        }
    }
    free(j);
    return rc;
}

// ---- the scalar restatement of csrc/jpeg_idct.hip ---------------------------------------------------------------------------
// Accurate integer IDCT ("islow": 13-bit constants, 2 extra bits kept between the passes), columns then rows.  Where the
// vectorised libjpeg-turbo (16-bit lanes; what Pillow runs on x86-64) and the textbook form differ, the vectorised one
// is restated: the column pass's results are kept in 16 bits -- saturated, or wrapped when rows 1..7 of the block are all
// zero (its DC-only shortcut is a 16-bit shift) --, the four sums it forms in 16-bit lanes before the multiplications
// (in0 + in4, in0 - in4, in7 + in3, in5 + in1) wrap, and the final samples are clamped.  Inside the encoder's range
// (|product| < 2^13) none of this is ever reached.
#define C_0_298 2446
#define C_0_390 3196
#define C_0_541 4433
#define C_0_765 6270
#define C_0_899 7373
#define C_1_175 9633
#define C_1_501 12299
#define C_1_847 15137
#define C_1_961 16069
#define C_2_053 16819
#define C_2_562 20995
#define C_3_072 25172

#define W16(x) ((int32_t)(int16_t)(uint16_t)(x))      /* a sum the vectorised form keeps in a 16-bit lane */

static inline void idct_1d(const int32_t* in, int stride, int32_t* out, int shift) {
    int32_t z2 = in[2 * stride], z3 = in[6 * stride];
    int32_t z1 = (z2 + z3) * C_0_541;
    int32_t tmp2 = z1 - z3 * C_1_847, tmp3 = z1 + z2 * C_0_765;
    z2 = in[0];
    z3 = in[4 * stride];
    int32_t tmp0 = W16(z2 + z3) * 8192, tmp1 = W16(z2 - z3) * 8192;
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7 * stride];
    tmp1 = in[5 * stride];
    tmp2 = in[3 * stride];
    tmp3 = in[1 * stride];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = W16(tmp0 + tmp2);
    int32_t z4 = W16(tmp1 + tmp3);
    const int32_t z5 = (z3 + z4) * C_1_175;
    tmp0 *= C_0_298;
    tmp1 *= C_2_053;
    tmp2 *= C_3_072;
    tmp3 *= C_1_501;
    z1 *= -C_0_899;
    z2 *= -C_2_562;
    z3 = z3 * -C_1_961 + z5;
    z4 = z4 * -C_0_390 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int32_t r = 1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + r) >> shift;
    out[7] = (tmp10 - tmp3 + r) >> shift;
    out[1] = (tmp11 + tmp2 + r) >> shift;
    out[6] = (tmp11 - tmp2 + r) >> shift;
    out[2] = (tmp12 + tmp1 + r) >> shift;
    out[5] = (tmp12 - tmp1 + r) >> shift;
    out[3] = (tmp13 + tmp0 + r) >> shift;
    out[4] = (tmp13 - tmp0 + r) >> shift;
}

static void idct_block(const int16_t* coef, const uint8_t* q, uint8_t* dst, size_t pitch) {
    int32_t in[64], ws[64], col[8];
    int ac_rows = 0;
    for (int i = 0; i < 64; ++i) {
        in[i] = (int32_t)coef[i] * q[i];
        if (i >= 8 && coef[i]) ac_rows = 1;
    }
    for (int c = 0; c < 8; ++c) {
        idct_1d(in + c, 8, col, 11);
        for (int r = 0; r < 8; ++r) {
            int32_t v = col[r];
            if (ac_rows) v = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
            else v = (int16_t)(uint16_t)v;
            ws[r * 8 + c] = v;
        }
    }
    for (int r = 0; r < 8; ++r) {
        idct_1d(ws + r * 8, 1, col, 18);
        for (int c = 0; c < 8; ++c) {
            const int32_t v = col[c] + 128;
            dst[r * pitch + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
}

static inline int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// chroma sample for output pixel (x, y): replication for tiny planes (downsampled width <= 2), else the triangle filter
static inline int chroma_at(const uint8_t* pl, size_t pitch, int dsw, int dsh, int hs, int vs, int x, int y) {
    if (hs == 1) return pl[(size_t)y * pitch + x];
    const int i = x >> 1;
    if (vs == 1) {
        const uint8_t* r = pl + (size_t)y * pitch;
        if (dsw <= 2) return r[i];
        if (x & 1) return i == dsw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
        return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    if (dsw <= 2) return pl[(size_t)cy * pitch + i];
    int oy = (y & 1) ? cy + 1 : cy - 1;
    oy = oy < 0 ? 0 : (oy > dsh - 1 ? dsh - 1 : oy);
    const uint8_t* r0 = pl + (size_t)cy * pitch;
    const uint8_t* r1 = pl + (size_t)oy * pitch;
    const int cur = 3 * r0[i] + r1[i];
    if (x & 1) return i == dsw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

// header fields the reconstruction indexes with, checked against each other and the slot
static int check_slot(const uint8_t* slot, size_t slot_bytes, int* geo) {
    if (slot_bytes < TISE_JPEG_SLOT_HDR) return TISE_JPEG_CORRUPT;
    const int mode = get32(slot), w = get32(slot + 4), h = get32(slot + 8), nc = get32(slot + 12), hs = get32(slot + 16), vs = get32(slot + 20);
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return TISE_JPEG_CORRUPT;
    const size_t payload = (size_t)(uint32_t)get32(slot + 48);
    if (mode == 0) {
        if (payload != (size_t)w * h * 3 || slot_bytes < TISE_JPEG_SLOT_HDR + payload) return TISE_JPEG_CORRUPT;
    } else if (mode == 1) {
        if (!((nc == 1 && hs == 1 && vs == 1) || (nc == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)))))
            return TISE_JPEG_CORRUPT;
        const int mx = (w + 8 * hs - 1) / (8 * hs), my = (h + 8 * vs - 1) / (8 * vs);
        size_t blocks = 0;
        for (int c = 0; c < 3; ++c) {
            const int bw = c < nc ? (c == 0 ? mx * hs : mx) : 0, bh = c < nc ? (c == 0 ? my * vs : my) : 0;
            if (get32(slot + 24 + 4 * c) != bw || get32(slot + 36 + 4 * c) != bh) return TISE_JPEG_CORRUPT;
            blocks += (size_t)bw * bh;
        }
        if (payload != blocks * 128 || slot_bytes < TISE_JPEG_SLOT_HDR + payload) return TISE_JPEG_CORRUPT;
    } else {
        return TISE_JPEG_CORRUPT;
    }
    geo[0] = mode; geo[1] = w; geo[2] = h; geo[3] = nc; geo[4] = hs; geo[5] = vs;
    return TISE_JPEG_OK;
}

int tise_jpeg_reconstruct_slot_rgb8(const uint8_t* slot, size_t slot_bytes, uint8_t* dst, size_t dst_bytes) {
    int g[6];
    if (!slot || !dst) return TISE_JPEG_CORRUPT;
    const int rc = check_slot(slot, slot_bytes, g);
    if (rc) return rc;
    const int mode = g[0], w = g[1], h = g[2], nc = g[3], hs = g[4], vs = g[5];
    if (dst_bytes < (size_t)w * h * 3) return TISE_JPEG_SIZE;
    if (mode == 0) {
        memcpy(dst, slot + TISE_JPEG_SLOT_HDR, (size_t)w * h * 3);
        return TISE_JPEG_OK;
    }
    if ((uintptr_t)slot & 1) return TISE_JPEG_CORRUPT;
    const int16_t* coef = (const int16_t*)(slot + TISE_JPEG_SLOT_HDR);
    const size_t blocks = ((size_t)(uint32_t)get32(slot + 48)) / 128;
    uint8_t* planes = (uint8_t*)malloc(blocks * 64);
    if (!planes) return TISE_JPEG_CORRUPT;
    uint8_t* pl[3] = {0, 0, 0};
    size_t pitch[3] = {0, 0, 0}, off = 0;
    for (int c = 0; c < nc; ++c) {
        const int bw = get32(slot + 24 + 4 * c), bh = get32(slot + 36 + 4 * c);
        pl[c] = planes + off * 64;
        pitch[c] = (size_t)bw * 8;
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx)
                idct_block(coef + (off + (size_t)by * bw + bx) * 64, slot + 64 + 64 * c, pl[c] + (size_t)by * 8 * pitch[c] + (size_t)bx * 8, pitch[c]);
        off += (size_t)bw * bh;
    }
    const int dsw = (w + hs - 1) / hs, dsh = (h + vs - 1) / vs;
    for (int y = 0; y < h; ++y) {
        uint8_t* o = dst + (size_t)y * w * 3;
        for (int x = 0; x < w; ++x, o += 3) {
            const int yv = pl[0][(size_t)y * pitch[0] + x];
            if (nc == 1) {
                o[0] = o[1] = o[2] = (uint8_t)yv;
                continue;
            }
            const int cb = chroma_at(pl[1], pitch[1], dsw, dsh, hs, vs, x, y) - 128;
            const int cr = chroma_at(pl[2], pitch[2], dsw, dsh, hs, vs, x, y) - 128;
            o[0] = (uint8_t)clamp8(yv + ((91881 * cr + 32768) >> 16));
            o[1] = (uint8_t)clamp8(yv + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            o[2] = (uint8_t)clamp8(yv + ((116130 * cb + 32768) >> 16));
        }
    }
    free(planes);
    return TISE_JPEG_OK;
}

int tise_jpeg_decode_rgb8(const uint8_t* file, size_t len, uint8_t* dst, size_t dst_bytes, int* w, int* h) {
    if (!file || !dst) return TISE_JPEG_CORRUPT;
    int gw = 0, gh = 0, layout = 0;
    int rc = tise_jpeg_probe(file, len, &gw, &gh, &layout);
    if (rc) return rc;
    if (w) *w = gw;
    if (h) *h = gh;
    if (dst_bytes < (size_t)gw * gh * 3) return TISE_JPEG_SIZE;
    const size_t sb = tise_jpeg_slot_bytes(gw, gh, layout);
    uint8_t* slot = (uint8_t*)malloc(sb);
    if (!slot) return TISE_JPEG_CORRUPT;
    rc = tise_jpeg_entropy_decode(file, len, slot, sb, 0, 0);
    if (rc == TISE_JPEG_OK) rc = tise_jpeg_reconstruct_slot_rgb8(slot, sb, dst, dst_bytes);
    free(slot);
    return rc;
}
