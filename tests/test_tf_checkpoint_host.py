"""CPU: the TensorFlow checkpoint reader (tise_toolbox_amd/tf_checkpoint.py) -- CRC-32C, Snappy, tables, V1 / V2, refusals."""
import os
import struct

import numpy as np
import pytest

from tise_toolbox_amd import build, tf_checkpoint as tfc

from ._tf_ckpt_writer import TableWriter, write_v1, write_v2


@pytest.fixture(scope="module", autouse=True)
def _host_lib():
    build.build_png(verbose=False)


def test_crc32c_rfc3720_vectors_and_mask():
    assert tfc.crc32c(bytes(32)) == 0x8A9136AA
    assert tfc.crc32c(b"\xff" * 32) == 0x62A8AB43
    assert tfc.crc32c(bytes(range(32))) == 0x46DD794E
    assert tfc.crc32c(bytes(range(31, -1, -1))) == 0x113FDB5C
    data = np.random.default_rng(0).bytes(100003)
    assert tfc.crc32c(data[57:], tfc.crc32c(data[:57])) == tfc.crc32c(data)        # running value, unaligned start
    for c in (0, 1, 0x8A9136AA, 0xffffffff, 0x12345678):
        m = tfc.mask_crc(c)
        assert m == ((((c >> 15) | (c << 17)) & 0xffffffff) + 0xa282ead8) & 0xffffffff
        assert tfc.unmask_crc(m) == c and (c == 0 or m != c)


def test_crc32c_speed():
    import time
    buf = np.random.default_rng(1).bytes(100 << 20)
    t = time.perf_counter()
    tfc.crc32c(buf)
    assert time.perf_counter() - t < 0.5


def test_snappy_literals_and_copies():
    # "abcd" literal, 1-byte-offset copy of 8 (overlapping, offset 4), 2-byte-offset copy of 5 (offset 10),
    # 4-byte-offset copy of 3 (offset 17), long literal (60 -> one extra length byte), overlapping offset-1 copy of 20
    lit = b"abcd"
    s = bytearray()
    s.append((len(lit) - 1) << 2)
    s += lit
    s += bytes([((8 - 4) << 2) | 1 | (0 << 5), 4])              # copy1: len 8, offset 4
    s += bytes([((5 - 1) << 2) | 2]) + struct.pack("<H", 10)   # copy2: len 5, offset 10
    s += bytes([((3 - 1) << 2) | 3]) + struct.pack("<I", 17)   # copy4: len 3, offset 17
    long = bytes(range(100, 170))
    s += bytes([60 << 2, len(long) - 1]) + long
    s += bytes([((20 - 1) << 2) | 2]) + struct.pack("<H", 1)
    out = bytearray(b"abcd")
    for ln, off in ((8, 4), (5, 10), (3, 17)):
        for _ in range(ln):
            out.append(out[-off])
    out += long
    out += bytes([long[-1]]) * 20
    stream = bytes(_varint(len(out))) + bytes(s)
    assert tfc.snappy_decompress(stream) == bytes(out)
    with pytest.raises(tfc.CheckpointError):
        tfc.snappy_decompress(bytes(_varint(len(out) + 1)) + bytes(s))          # length mismatch
    with pytest.raises(tfc.CheckpointError):
        tfc.snappy_decompress(bytes(_varint(10)) + bytes([((4 - 1) << 2) | 2]) + struct.pack("<H", 5))   # offset before start


def _varint(v):
    from ._tf_ckpt_writer import varint
    return varint(v)


def _tensors(seed=0, n=40):
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(n):
        shape = [(3, 3, 4, 8), (8,), (16, 5), ()][i % 4]
        out[f"scope_{i // 7}/block/Conv_{i}/weights/ExponentialMovingAverage"] = rng.standard_normal(shape).astype(np.float32)
    return out


@pytest.mark.parametrize("fmt,compression", [("V1", 0), ("V1", 1), ("V2", 0), ("V2", 1)])
def test_round_trip_bit_exact(tmp_path, fmt, compression):
    tensors = _tensors()
    path = str(tmp_path / "model.ckpt")
    # small blocks: many data blocks, keys prefix-compressed across restart points
    (write_v1 if fmt == "V1" else write_v2)(path, tensors, compression=compression, block_size=256)
    assert tfc.checkpoint_format(path) == fmt
    got = tfc.read_tensors(path, list(tensors))
    assert set(got) == set(tensors)
    for k, v in tensors.items():
        assert got[k].dtype == np.float32 and got[k].shape == v.shape
        assert got[k].tobytes() == v.tobytes()
    listed = tfc.list_tensors(path)
    assert {k: s for k, (s, _) in listed.items()} == {k: v.shape for k, v in tensors.items()}
    sub = tfc.read_tensors(path, [sorted(tensors)[3]])
    assert list(sub) == [sorted(tensors)[3]]


def test_v2_shards(tmp_path):
    tensors = _tensors(1, 9)
    path = str(tmp_path / "m")
    write_v2(path, tensors, shards=3)
    got = tfc.read_tensors(path, list(tensors))
    assert all(got[k].tobytes() == v.tobytes() for k, v in tensors.items())


def test_table_multi_block_prefix_keys(tmp_path):
    tw = TableWriter(block_size=64, restart_interval=3)
    keys = [f"common/prefix/key_{i:04d}".encode() for i in range(200)]
    for k in keys:
        tw.add(k, k[::-1])
    p = tmp_path / "t"
    p.write_bytes(tw.finish())
    t = tfc._Table(str(p))
    got = [(k, bytes(v)) for k, v in t.entries()]
    assert got == [(k, k[::-1]) for k in keys]
    assert len(tw.index) > 10


NAME = "mixed_8x8x2048b/branch_pool/Conv/weights/ExponentialMovingAverage"


@pytest.mark.parametrize("fmt", ["V1", "V2"])
def test_refusals_name_the_tensor(tmp_path, fmt):
    w = write_v1 if fmt == "V1" else write_v2
    a = {NAME: np.ones((4, 3), np.float32), "other/beta": np.zeros(3, np.float32)}
    p = str(tmp_path / "part")
    w(p, a, slices={NAME: 2})
    with pytest.raises(tfc.CheckpointError, match="tensor " + NAME + " .*partitioned"):
        tfc.read_tensors(p, [NAME])
    p = str(tmp_path / "dtype")
    w(p, a, dtypes={NAME: 2})
    with pytest.raises(tfc.CheckpointError, match="tensor " + NAME + " has dtype 2"):
        tfc.read_tensors(p, [NAME])
    p = str(tmp_path / "ok")
    w(p, a)
    with pytest.raises(tfc.CheckpointError, match="tensor missing/tensor is not in the checkpoint"):
        tfc.read_tensors(p, ["missing/tensor"])
    assert tfc.read_tensors(p, [NAME])[NAME].tobytes() == a[NAME].tobytes()


def test_v2_bad_tensor_checksum(tmp_path):
    p = str(tmp_path / "m")
    write_v2(p, {NAME: np.arange(12, dtype=np.float32)})
    d = p + ".data-00000-of-00001"
    raw = bytearray(open(d, "rb").read())
    raw[5] ^= 1
    open(d, "wb").write(bytes(raw))
    with pytest.raises(tfc.CheckpointError, match="bad checksum of tensor " + NAME):
        tfc.read_tensors(p, [NAME])


@pytest.mark.parametrize("fmt", ["V1", "V2"])
def test_bad_block_checksum_magic_truncation(tmp_path, fmt):
    p = str(tmp_path / "m")
    (write_v1 if fmt == "V1" else write_v2)(p, {NAME: np.arange(12, dtype=np.float32)})
    table = p if fmt == "V1" else p + ".index"
    good = open(table, "rb").read()
    bad = bytearray(good)
    bad[3] ^= 0x40                                            # inside the first data block
    open(table, "wb").write(bytes(bad))
    with pytest.raises(tfc.CheckpointError, match="checksum"):
        tfc.read_tensors(p, [NAME])
    bad = bytearray(good)
    bad[-1] ^= 1
    open(table, "wb").write(bytes(bad))
    with pytest.raises(tfc.CheckpointError, match="magic"):
        tfc.read_tensors(p, [NAME])
    open(table, "wb").write(good[:20])
    with pytest.raises(tfc.CheckpointError, match="truncated"):
        tfc.read_tensors(p, [NAME])
    open(table, "wb").write(good[:30] + good[-48:])
    with pytest.raises(tfc.CheckpointError, match="truncated|checksum"):
        tfc.read_tensors(p, [NAME])
    if fmt == "V2":
        open(table, "wb").write(good)
        d = p + ".data-00000-of-00001"
        open(d, "wb").write(open(d, "rb").read()[:20])
        with pytest.raises(tfc.CheckpointError, match="truncated file \\(tensor " + NAME):
            tfc.read_tensors(p, [NAME])


def test_no_checkpoint(tmp_path):
    with pytest.raises(tfc.CheckpointError, match="no TensorFlow checkpoint"):
        tfc.read_tensors(str(tmp_path / "nothing"), [NAME])
    assert not os.path.exists(str(tmp_path / "nothing"))
