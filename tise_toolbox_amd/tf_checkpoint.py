"""Read float tensors out of a TensorFlow 1 checkpoint without TensorFlow or the protobuf package.

The reference's IS* for CUB birds restores its fine-tuned InceptionV3 with ``tf.train.Saver(...).restore(sess,
FLAGS.checkpoint_dir)`` (image_realism/IS/bird/inception_score_star_bird.py:196-201).  The path it names, ``model.ckpt``,
is one of TF1's two checkpoint formats, both of which are read here:

* V1: ONE file, a table (below) whose entry "" holds a ``SavedTensorSliceMeta`` (every tensor's name, shape, dtype and
  slices) and whose other entries each hold one ``SavedSlice`` (name, slice, ``TensorProto`` with the values in
  ``float_val`` or ``tensor_content``), all wrapped in ``SavedTensorSlices``.
* V2: ``PATH.index``, a table whose entry "" is a ``BundleHeaderProto`` and whose other entries map tensor names to
  ``BundleEntryProto`` (dtype, shape, shard, offset, size, crc32c), and ``PATH.data-NNNNN-of-MMMMM`` with the raw
  little-endian bytes.

The table is LevelDB's sorted-string table as TensorFlow writes it (tensorflow/core/lib/io/table*): a 48-byte footer
(metaindex and index block handles as varints, then the magic 0xdb4775248b80fb57), an index block whose values are the
handles of the data blocks, and blocks of prefix-compressed entries followed by their restart array.  Every block has a
5-byte trailer: its compression type (0 none, 1 Snappy) and the masked CRC-32C of contents + type byte.  Snappy blocks are
decoded by ``snappy_decompress`` below.  The protobuf wire format is parsed by hand (``_fields``).

Every checksum is verified (block trailers; V2 tensors' ``crc32c``, stored masked as TensorFlow's BundleWriter does) with
the CRC-32C of the host library (``tise_crc32c`` in csrc/png_decode.c).  Refused, with an error that names the tensor:
partitioned slices, a dtype other than float, a missing name, a bad checksum, a bad magic number and a truncated file.
"""
import ctypes
import os
import struct

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
FOOTER_BYTES = 48
DT_FLOAT = 1
_MASK_DELTA = 0xa282ead8


class CheckpointError(ValueError):
    """A checkpoint that cannot be read as asked: the message names the file and, where there is one, the tensor."""


# ---- CRC-32C (host library) ------------------------------------------------------------------------------------------
_CRC = None


def _crc_fn():
    global _CRC
    if _CRC is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtise_png.so")
        if not os.path.exists(path):
            raise CheckpointError(f"{path} is missing: run tise_toolbox_amd.build.build_png() (it holds the CRC-32C)")
        fn = ctypes.CDLL(path).tise_crc32c
        fn.restype = ctypes.c_uint32
        fn.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
        _CRC = fn
    return _CRC


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli) of a bytes-like object, continuing ``crc``."""
    mv = memoryview(data).cast("B")
    if mv.nbytes == 0:
        return crc & 0xffffffff
    buf = np.frombuffer(mv, dtype=np.uint8)
    return int(_crc_fn()(crc & 0xffffffff, buf.ctypes.data, buf.nbytes))


def mask_crc(crc):
    """LevelDB / TensorFlow masked CRC: rotate right by 15 bits, add a constant (crc32c::Mask)."""
    return ((((crc >> 15) | (crc << 17)) & 0xffffffff) + _MASK_DELTA) & 0xffffffff


def unmask_crc(masked):
    rot = (masked - _MASK_DELTA) & 0xffffffff
    return ((rot >> 17) | (rot << 15)) & 0xffffffff


# ---- Snappy ----------------------------------------------------------------------------------------------------------
def snappy_decompress(data, what="snappy block"):
    """Raw Snappy format (no framing): varint uncompressed length, then literals and copies with 1-, 2- or 4-byte
    offsets.  A copy may overlap its own output (offset < length), which repeats the last ``offset`` bytes."""
    data = memoryview(data).cast("B")
    n, pos = _varint(data, 0, what)
    out = bytearray(n)
    o = 0
    end = len(data)
    while pos < end:
        tag = data[pos]
        pos += 1
        kind = tag & 3
        if kind == 0:                                         # literal
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                if pos + nb > end:
                    raise CheckpointError(f"{what}: truncated literal length")
                ln = int.from_bytes(data[pos:pos + nb], "little")
                pos += nb
            ln += 1
            if pos + ln > end or o + ln > n:
                raise CheckpointError(f"{what}: literal runs past the end")
            out[o:o + ln] = data[pos:pos + ln]
            pos += ln
            o += ln
            continue
        if kind == 1:                                         # copy, 1-byte offset
            if pos >= end:
                raise CheckpointError(f"{what}: truncated copy")
            ln = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | data[pos]
            pos += 1
        else:                                                 # copy, 2- or 4-byte offset
            nb = 2 if kind == 2 else 4
            if pos + nb > end:
                raise CheckpointError(f"{what}: truncated copy")
            ln = (tag >> 2) + 1
            off = int.from_bytes(data[pos:pos + nb], "little")
            pos += nb
        if off == 0 or off > o or o + ln > n:
            raise CheckpointError(f"{what}: copy outside the output (offset {off}, length {ln})")
        if off >= ln:
            out[o:o + ln] = out[o - off:o - off + ln]
        else:                                                 # overlapping: the pattern of `off` bytes repeats
            pat = bytes(out[o - off:o])
            reps = -(-ln // off)
            out[o:o + ln] = (pat * reps)[:ln]
        o += ln
    if o != n:
        raise CheckpointError(f"{what}: {o} bytes decoded, the header says {n}")
    return bytes(out)


# ---- protobuf wire format --------------------------------------------------------------------------------------------
def _varint(buf, pos, what="varint"):
    shift = result = 0
    while True:
        if pos >= len(buf):
            raise CheckpointError(f"{what}: truncated varint")
        b = buf[pos]
        pos += 1
        result |= (b & 0x7f) << shift
        if not b & 0x80:
            return result, pos
        shift += 7
        if shift > 63:
            raise CheckpointError(f"{what}: varint longer than 64 bits")


def _fields(buf, what="message"):
    """[(field number, wire type, value)] of a protobuf message: varint -> int, 64-bit / 32-bit -> int (little endian),
    length-delimited -> memoryview.  Groups (wire types 3, 4) do not occur in these messages and are refused."""
    buf = memoryview(buf).cast("B")
    out, pos, end = [], 0, len(buf)
    while pos < end:
        key, pos = _varint(buf, pos, what)
        fn, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos, what)
        elif wt == 1:
            if pos + 8 > end:
                raise CheckpointError(f"{what}: truncated field {fn}")
            v = int.from_bytes(buf[pos:pos + 8], "little")
            pos += 8
        elif wt == 2:
            ln, pos = _varint(buf, pos, what)
            if pos + ln > end:
                raise CheckpointError(f"{what}: truncated field {fn}")
            v = buf[pos:pos + ln]
            pos += ln
        elif wt == 5:
            if pos + 4 > end:
                raise CheckpointError(f"{what}: truncated field {fn}")
            v = int.from_bytes(buf[pos:pos + 4], "little")
            pos += 4
        else:
            raise CheckpointError(f"{what}: unsupported wire type {wt} (field {fn})")
        out.append((fn, wt, v))
    return out


def _signed64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def _shape(buf, what):
    """TensorShapeProto: dim = 2 (Dim: size = 1), unknown_rank = 3."""
    dims = []
    for fn, _, v in _fields(buf, what):
        if fn == 2:
            size = 0
            for f2, _, v2 in _fields(v, what):
                if f2 == 1:
                    size = _signed64(v2)
            dims.append(size)
        elif fn == 3 and v:
            raise CheckpointError(f"{what}: unknown rank")
    return tuple(dims)


def _slice_is_full(buf, what):
    """TensorSliceProto (extent = 1: Extent start = 1, length = 2): True when every extent is the whole dimension."""
    for fn, _, v in _fields(buf, what):
        if fn == 1:
            for f2, _, v2 in _fields(v, what):
                if (f2 == 1 and v2 != 0) or f2 == 2:
                    return False
    return True


# ---- table -----------------------------------------------------------------------------------------------------------
class _Table:
    """A LevelDB-format table file held in memory; ``entries()`` yields (key bytes, value memoryview) in key order."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            self.data = memoryview(f.read())
        if len(self.data) < FOOTER_BYTES:
            raise CheckpointError(f"{path}: truncated file ({len(self.data)} bytes, no table footer)")
        footer = self.data[-FOOTER_BYTES:]
        magic = int.from_bytes(footer[40:48], "little")
        if magic != TABLE_MAGIC:
            raise CheckpointError(f"{path}: bad table magic 0x{magic:016x} (not a TensorFlow checkpoint table)")
        _, pos = self._handle(footer, 0)                      # metaindex handle (unused)
        self.index = self._handle(footer, pos)[0]

    def _handle(self, buf, pos):
        off, pos = _varint(buf, pos, f"{self.path}: block handle")
        size, pos = _varint(buf, pos, f"{self.path}: block handle")
        return (off, size), pos

    def block(self, handle):
        off, size = handle
        if off + size + 5 > len(self.data) - FOOTER_BYTES:
            raise CheckpointError(f"{self.path}: truncated file (block at {off} + {size} runs past the end)")
        raw = self.data[off:off + size + 1]
        stored = int.from_bytes(self.data[off + size + 1:off + size + 5], "little")
        if crc32c(raw) != unmask_crc(stored):
            raise CheckpointError(f"{self.path}: bad block checksum at offset {off}")
        kind = raw[size]
        if kind == 0:
            return raw[:size]
        if kind == 1:
            return memoryview(snappy_decompress(raw[:size], f"{self.path}: block at offset {off}"))
        raise CheckpointError(f"{self.path}: unknown block compression {kind} at offset {off}")

    def _block_entries(self, blk):
        what = f"{self.path}: block"
        if len(blk) < 4:
            raise CheckpointError(f"{what} shorter than its restart count")
        nrest = int.from_bytes(blk[-4:], "little")
        limit = len(blk) - 4 - 4 * nrest
        if limit < 0:
            raise CheckpointError(f"{what}: restart array larger than the block")
        pos, key = 0, b""
        while pos < limit:
            shared, pos = _varint(blk, pos, what)
            unshared, pos = _varint(blk, pos, what)
            vlen, pos = _varint(blk, pos, what)
            if shared > len(key) or pos + unshared + vlen > limit:
                raise CheckpointError(f"{what}: corrupt entry")
            key = key[:shared] + bytes(blk[pos:pos + unshared])
            pos += unshared
            yield key, blk[pos:pos + vlen]
            pos += vlen

    def entries(self):
        for _, hv in self._block_entries(self.block(self.index)):
            handle, _ = self._handle(hv, 0)
            yield from self._block_entries(self.block(handle))


# ---- V1 / V2 ---------------------------------------------------------------------------------------------------------
def checkpoint_format(path):
    """"V2" when ``path.index`` exists, "V1" when ``path`` itself is a file; CheckpointError otherwise."""
    if os.path.isfile(path + ".index"):
        return "V2"
    if os.path.isfile(path):
        return "V1"
    raise CheckpointError(f"{path}: no TensorFlow checkpoint (neither {path}.index nor the file itself exists)")


def _tensor_values(buf, shape, name, path):
    """TensorProto -> float32 array: dtype = 1, tensor_content = 4, float_val = 5 (packed or not)."""
    dtype, content, vals = None, None, []
    for fn, wt, v in _fields(buf, f"{path}: tensor {name}"):
        if fn == 1:
            dtype = v
        elif fn == 4:
            content = v
        elif fn == 5:
            if wt == 2:
                vals.append(np.frombuffer(v, dtype="<f4"))
            else:
                vals.append(np.array([struct.unpack("<f", struct.pack("<I", v))[0]], dtype=np.float32))
    if dtype is not None and dtype != DT_FLOAT:
        raise CheckpointError(f"{path}: tensor {name} has dtype {dtype}, only float (1) is read")
    n = int(np.prod(shape, dtype=np.int64))
    if content is not None and len(content):
        arr = np.frombuffer(content, dtype="<f4")
    elif vals:
        arr = np.concatenate(vals)
    else:
        arr = np.zeros(0, dtype=np.float32)
    if arr.size == 1 and n > 1:                              # TensorProto: one value stands for all
        arr = np.full(n, arr[0], dtype=np.float32)
    if arr.size != n:
        raise CheckpointError(f"{path}: tensor {name} holds {arr.size} values, its shape {list(shape)} needs {n}")
    return arr.astype(np.float32).reshape(shape)


def _read_v1(path, wanted):
    table = _Table(path)
    meta, data = {}, {}
    for key, value in table.entries():
        for fn, _, v in _fields(value, f"{path}: entry"):
            if fn == 1 and key == b"":                        # SavedTensorSliceMeta: tensor = 1 (SavedSliceMeta)
                for f2, _, t in _fields(v, f"{path}: meta"):
                    if f2 != 1:
                        continue
                    name, shape, dtype, slices = None, (), None, []
                    for f3, _, x in _fields(t, f"{path}: meta"):
                        if f3 == 1:
                            name = bytes(x).decode()
                        elif f3 == 2:
                            shape = _shape(x, f"{path}: meta")
                        elif f3 == 3:
                            dtype = x
                        elif f3 == 4:
                            slices.append(x)
                    meta[name] = (shape, dtype, slices)
            elif fn == 2:                                     # SavedSlice: name = 1, slice = 2, data = 3
                name, tensor = None, None
                for f2, _, x in _fields(v, f"{path}: slice"):
                    if f2 == 1:
                        name = bytes(x).decode()
                    elif f2 == 3:
                        tensor = x
                if name in wanted:
                    data.setdefault(name, []).append(tensor)
    out = {}
    for name in wanted:
        if name not in meta:
            raise CheckpointError(f"{path}: tensor {name} is not in the checkpoint")
        shape, dtype, slices = meta[name]
        if dtype != DT_FLOAT:
            raise CheckpointError(f"{path}: tensor {name} has dtype {dtype}, only float (1) is read")
        if len(slices) != 1 or not _slice_is_full(slices[0], f"{path}: tensor {name}") or len(data.get(name, [])) != 1:
            raise CheckpointError(f"{path}: tensor {name} is saved in {max(len(slices), len(data.get(name, [])))} partitioned "
                                  f"slices; only whole tensors are read")
        out[name] = _tensor_values(data[name][0], shape, name, path)
    return out


def _read_v2(path, wanted):
    index = path + ".index"
    table = _Table(index)
    entries, num_shards = {}, 1
    for key, value in table.entries():
        if key == b"":                                        # BundleHeaderProto: num_shards = 1, endianness = 2
            for fn, _, v in _fields(value, f"{index}: header"):
                if fn == 1:
                    num_shards = v
                elif fn == 2 and v != 0:
                    raise CheckpointError(f"{index}: big-endian bundle")
            continue
        name = key.decode()
        if name in wanted:
            entries[name] = value
    out, shards = {}, {}
    try:
        for name in wanted:
            if name not in entries:
                raise CheckpointError(f"{index}: tensor {name} is not in the checkpoint")
            dtype, shape, shard, offset, size, crc, nslices = None, (), 0, 0, 0, None, 0
            for fn, _, v in _fields(entries[name], f"{index}: tensor {name}"):
                if fn == 1:
                    dtype = v
                elif fn == 2:
                    shape = _shape(v, f"{index}: tensor {name}")
                elif fn == 3:
                    shard = v
                elif fn == 4:
                    offset = v
                elif fn == 5:
                    size = v
                elif fn == 6:
                    crc = v
                elif fn == 7:
                    nslices += 1
            if nslices:
                raise CheckpointError(f"{index}: tensor {name} is saved in {nslices} partitioned slices; only whole tensors are read")
            if dtype != DT_FLOAT:
                raise CheckpointError(f"{index}: tensor {name} has dtype {dtype}, only float (1) is read")
            n = int(np.prod(shape, dtype=np.int64))
            if size != 4 * n:
                raise CheckpointError(f"{index}: tensor {name} has {size} bytes, its shape {list(shape)} needs {4 * n}")
            if shard not in shards:
                dpath = f"{path}.data-{shard:05d}-of-{num_shards:05d}"
                if not os.path.isfile(dpath):
                    raise CheckpointError(f"{dpath}: missing data shard of tensor {name}")
                with open(dpath, "rb") as f:
                    shards[shard] = (dpath, memoryview(f.read()))
            dpath, buf = shards[shard]
            if offset + size > len(buf):
                raise CheckpointError(f"{dpath}: truncated file (tensor {name} at {offset} + {size})")
            raw = buf[offset:offset + size]
            if crc is None or crc32c(raw) != unmask_crc(crc):
                raise CheckpointError(f"{dpath}: bad checksum of tensor {name}")
            out[name] = np.frombuffer(raw, dtype="<f4").astype(np.float32).reshape(shape)
    finally:
        shards.clear()
    return out


def read_tensors(path, names):
    """{name: float32 ndarray in TF layout} for ``names`` from the V1 or V2 checkpoint ``path``."""
    wanted = list(dict.fromkeys(names))
    fmt = checkpoint_format(path)
    return _read_v2(path, set(wanted)) if fmt == "V2" else _read_v1(path, set(wanted))


def list_tensors(path):
    """{name: (shape, dtype)} of every tensor of a checkpoint (V1: from its meta entry; V2: from its index)."""
    fmt = checkpoint_format(path)
    table = _Table(path + ".index" if fmt == "V2" else path)
    out = {}
    for key, value in table.entries():
        if fmt == "V2":
            if key == b"":
                continue
            dtype, shape = None, ()
            for fn, _, v in _fields(value):
                if fn == 1:
                    dtype = v
                elif fn == 2:
                    shape = _shape(v, key.decode())
            out[key.decode()] = (shape, dtype)
        elif key == b"":
            for fn, _, v in _fields(value):
                if fn != 1:
                    continue
                for f2, _, t in _fields(v):
                    if f2 != 1:
                        continue
                    fs = {f3: x for f3, _, x in _fields(t)}
                    out[bytes(fs[1]).decode()] = (_shape(fs[2], "meta") if 2 in fs else (), fs.get(3))
    return out
