"""A minimal sequential JPEG writer for tests: it takes QUANTISED coefficient blocks (natural order), quantisation
tables, sampling factors and a restart interval and emits a file with the example Huffman tables of ITU-T T.81 Annex K.
Tests place exact values with it (blocks that saturate the clamp, DC-only blocks, one maximal AC term, products at the
decoder's guard) and build the layouts Pillow cannot write (4:4:0, 4:1:1, several scans).  Not a product module."""
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [int(x, 16) for x in (
    "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 82 09 0a 16 17 18 "
    "19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 "
    "76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 "
    "c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa").split()])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [int(x, 16) for x in (
    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 0a 16 24 34 e1 25 "
    "f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 "
    "75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba "
    "c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa").split()])
for _bits, _vals in (DC_LUMA, DC_CHROMA, AC_LUMA, AC_CHROMA):
    assert sum(_bits) == len(_vals) == len(set(_vals))


def _codes(table):
    """symbol -> (code, length) of a canonical Huffman table (T.81 Annex C)."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v):
    return int(abs(int(v))).bit_length()


def _encode_block(bw, blk, pred, dc, ac):
    diff = int(blk[0]) - pred
    s = _size(diff)
    bw.put(*dc[s])
    if s:
        bw.put(diff if diff > 0 else diff + (1 << s) - 1, s)
    zz = blk[ZIGZAG]
    run = 0
    last = int(np.max(np.nonzero(zz)[0])) if np.any(zz[1:]) else 0
    for k in range(1, last + 1):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        s = _size(v)
        bw.put(*ac[(run << 4) | s])
        bw.put(v if v > 0 else v + (1 << s) - 1, s)
        run = 0
    if last < 63:
        bw.put(*ac[0x00])
    return int(blk[0])


def _seg(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def blocks_shape(width, height, sampling):
    """[(blocks per column, blocks per row)] of each component of an interleaved scan (block rows padded to whole MCUs)."""
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return [(my * v, mx * h) for h, v in sampling]


def write_jpeg(width, height, blocks, qtables, sampling=None, restart=0, marker="jfif", ids=None, scans=None, sof=0xC0,
               drop_rst=None):
    """``blocks``: one int array (bh, bw, 64) per component, natural order, quantised, shaped as blocks_shape() says.
    ``qtables``: one (64,) table per component, natural order.  ``sampling``: [(h, v)] per component (default all 1x1).
    ``marker``: "jfif" | "adobe" | "adobe0" | None.  ``scans``: lists of component indices (default: one scan with all).
    ``drop_rst``: index of a restart marker to leave out (a damaged file)."""
    nc = len(blocks)
    sampling = sampling or [(1, 1)] * nc
    ids = ids or list(range(1, nc + 1))
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    out = bytearray(b"\xff\xd8")
    if marker == "jfif":
        out += _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    elif marker in ("adobe", "adobe0"):
        out += _seg(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([1 if marker == "adobe" else 0]))
    for c in range(nc):
        out += _seg(0xDB, bytes([c]) + bytes(int(v) for v in np.asarray(qtables[c])[ZIGZAG]))
    sof_body = struct.pack(">BHHB", 8, height, width, nc)
    for c in range(nc):
        sof_body += bytes([ids[c], (sampling[c][0] << 4) | sampling[c][1], c])
    out += _seg(sof, sof_body)
    for tc_th, table in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _seg(0xC4, bytes([tc_th]) + bytes(table[0]) + bytes(table[1]))
    if restart:
        out += _seg(0xDD, struct.pack(">H", restart))
    dcs, acs = [_codes(DC_LUMA), _codes(DC_CHROMA)], [_codes(AC_LUMA), _codes(AC_CHROMA)]
    for comps in (scans or [list(range(nc))]):
        body = bytes([len(comps)])
        for c in comps:
            body += bytes([ids[c], 0x00 if c == 0 else 0x11])
        out += _seg(0xDA, body + b"\0\x3f\0")
        bw = _Bits()
        pred = {c: 0 for c in comps}
        if len(comps) > 1:
            mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
            units = [[(c, yy * sampling[c][1] + v, xx * sampling[c][0] + h) for c in comps for v in range(sampling[c][1])
                      for h in range(sampling[c][0])] for yy in range(my) for xx in range(mx)]
        else:                                              # a scan of one component is not interleaved: its own block raster
            c = comps[0]
            cw, ch = -(-width * sampling[c][0] // hmax), -(-height * sampling[c][1] // vmax)
            units = [[(c, y, x)] for y in range(-(-ch // 8)) for x in range(-(-cw // 8))]
        n_rst = 0
        for i, unit in enumerate(units):
            if restart and i and i % restart == 0:
                bw.flush()
                if drop_rst != n_rst:
                    bw.out += bytes([0xFF, 0xD0 + (n_rst & 7)])
                n_rst += 1
                pred = {c: 0 for c in comps}
            for c, y, x in unit:
                t = 0 if c == 0 else 1
                pred[c] = _encode_block(bw, np.asarray(blocks[c][y, x]), pred[c], dcs[t], acs[t])
        bw.flush()
        out += bw.out
    out += b"\xff\xd9"
    return bytes(out)
