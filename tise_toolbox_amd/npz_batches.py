"""Stream an image batch out of an ``.npz``: the feed of the ADM sample-batch suite (adm_eval.py).

The guided-diffusion evaluator takes its two sides as ``.npz`` files whose ``arr_0`` is (N, H, W, 3) uint8 -- 9.8 GB for
50 000 images of 256 x 256, beside an optional ``arr_1`` of labels.  ``np.load`` would materialise the whole array (and, for a
deflated member, inflate it in one piece).  ``NpzImageBatches`` opens the zip member as a stream, parses the ``.npy`` header
itself and reads (b, H, W, 3) batches sequentially into page-locked buffers -- stored and deflated members alike, the array is
never whole in memory.
"""
import ast
import struct
import zipfile

import numpy as np
import torch

_MAGIC = b"\x93NUMPY"


def is_statistics_npz(path):
    """True when ``path`` holds statistics (a ``mu`` array: the evaluator's {mu, sigma, mu_s, sigma_s} files and this
    project's --save-stats files), False when it is a batch of images.  Only the zip directory is read."""
    with zipfile.ZipFile(path) as zf:
        return "mu.npy" in zf.namelist()


def read_npy_header(fp, what):
    """Parse the ``.npy`` header at the start of the stream ``fp`` (format versions 1 to 3) -> (descr, fortran_order, shape);
    ``fp`` is left at the first byte of the data.  ``what`` names the file and member in messages."""
    head = fp.read(8)
    if len(head) != 8 or head[:6] != _MAGIC:
        raise ValueError(f"{what}: not an .npy member (bad magic)")
    major = head[6]
    if major == 1:
        (hlen,) = struct.unpack("<H", fp.read(2))
    elif major in (2, 3):
        (hlen,) = struct.unpack("<I", fp.read(4))
    else:
        raise ValueError(f"{what}: .npy format version {major}.{head[7]} is not supported (1 to 3 are)")
    raw = fp.read(hlen)
    if len(raw) != hlen:
        raise ValueError(f"{what}: truncated .npy header")
    try:
        d = ast.literal_eval(raw.decode("utf-8" if major == 3 else "latin1"))
        descr, fortran, shape = d["descr"], bool(d["fortran_order"]), tuple(int(v) for v in d["shape"])
    except Exception as e:                                               # noqa: BLE001
        raise ValueError(f"{what}: unreadable .npy header ({type(e).__name__}: {e})") from None
    return descr, fortran, shape


class NpzImageBatches:
    """Iterable over the (b, H, W, 3) uint8 batches of ``path[key]``, in order; the last batch is shorter when N is no multiple
    of ``batch``.  ``len()`` is the number of batches, ``n_images`` is N, ``image_shape`` (H, W, 3).

    The batches are torch tensors that VIEW one of ``ring`` page-locked buffers (plain host memory where there is no HIP
    device), refilled in turn: a batch stays valid until ``ring - 1`` further batches have been taken.  A consumer that copies
    a batch to the device asynchronously hands the copy's event to ``in_flight(event)``; the buffer is refilled only after it.
    Every iteration opens the member afresh, so the object can be walked more than once."""

    def __init__(self, path, key="arr_0", batch=1000, pin=None, ring=2):
        self.path, self.key, self.batch = str(path), str(key), int(batch)
        if self.batch <= 0:
            raise ValueError("batch must be positive")
        self.member = self.key if self.key.endswith(".npy") else self.key + ".npy"
        self._what = f"{self.path}[{self.key!r}]"
        with zipfile.ZipFile(self.path) as zf:
            names = zf.namelist()
            if self.member not in names:
                have = ", ".join(n[:-4] if n.endswith(".npy") else n for n in names) or "nothing"
                raise KeyError(f"{self.path}: no array {self.key!r} in this file (it holds {have})")
            with zf.open(self.member) as fp:
                descr, fortran, shape = read_npy_header(fp, self._what)
        if fortran:
            raise ValueError(f"{self._what}: Fortran-ordered array; an image batch must be saved in C order")
        if not isinstance(descr, str) or np.dtype(descr) != np.uint8:
            raise ValueError(f"{self._what}: dtype {descr!r}; an image batch is uint8 ('|u1')")
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError(f"{self._what}: shape {shape}; an image batch is (N, H, W, 3)")
        if shape[1] <= 0 or shape[2] <= 0:
            raise ValueError(f"{self._what}: shape {shape}: empty images")
        self.n_images = shape[0]
        self.image_shape = shape[1:]
        self._image_bytes = shape[1] * shape[2] * 3
        self._pin = torch.cuda.is_available() if pin is None else bool(pin)
        self._ring = max(2, int(ring))
        self._bufs = [None] * self._ring
        self._events = [None] * self._ring
        self._last = None

    def __len__(self):
        return -(-self.n_images // self.batch)

    def in_flight(self, event):
        """The batch taken last is being copied to the device: ``event`` (recorded after the copy) must have completed before
        its buffer is written again."""
        if self._last is not None:
            self._events[self._last] = event

    def _buffer(self, slot):
        if self._events[slot] is not None:
            self._events[slot].synchronize()
            self._events[slot] = None
        if self._bufs[slot] is None:
            rows = min(self.batch, max(self.n_images, 1))
            t = torch.empty((rows,) + self.image_shape, dtype=torch.uint8)
            self._bufs[slot] = t.pin_memory() if self._pin else t
        return self._bufs[slot]

    def __iter__(self):
        with zipfile.ZipFile(self.path) as zf, zf.open(self.member) as fp:
            read_npy_header(fp, self._what)
            slot = 0
            for lo in range(0, self.n_images, self.batch):
                rows = min(self.batch, self.n_images - lo)
                buf = self._buffer(slot)[:rows]
                view = memoryview(buf.numpy().reshape(-1))
                need, got = rows * self._image_bytes, 0
                while got < need:
                    k = fp.readinto(view[got:need])
                    if not k:
                        raise ValueError(f"{self._what}: the member ends after {lo * self._image_bytes + got} bytes of image data, "
                                         f"its header promises {self.n_images * self._image_bytes}")
                    got += k
                self._last = slot
                yield buf
                slot = (slot + 1) % self._ring
        self._last = None
