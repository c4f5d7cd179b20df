"""CPU: the host side of the ADM sample-batch suite -- the streaming .npz image feed (tise_toolbox_amd/npz_batches.py), the
statistics-file detection, and the chunk bookkeeping of the evaluator's Inception Score rule (adm_eval.py)."""
import io
import zipfile

import numpy as np
import pytest

from tise_toolbox_amd import adm_eval
from tise_toolbox_amd.npz_batches import NpzImageBatches, is_statistics_npz, read_npy_header


@pytest.fixture(scope="module")
def arrays():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (11, 6, 5, 3), dtype=np.uint8)
    x.setflags(write=False)
    return x, np.arange(11, dtype=np.int64)


@pytest.mark.parametrize("save", [np.savez, np.savez_compressed], ids=["stored", "deflated"])
def test_batches_equal_np_load(tmp_path, arrays, save, monkeypatch):
    x, labels = arrays
    path = tmp_path / "batch.npz"
    save(path, x, labels)                                         # arr_0 = images, arr_1 = labels
    with zipfile.ZipFile(path) as zf:
        kind = zf.getinfo("arr_0.npy").compress_type
    assert kind == (zipfile.ZIP_STORED if save is np.savez else zipfile.ZIP_DEFLATED)
    monkeypatch.setattr(np, "load", lambda *a, **k: pytest.fail("the feed must not call np.load"))
    feed = NpzImageBatches(path, batch=4)
    assert feed.n_images == 11 and len(feed) == 3 and feed.image_shape == (6, 5, 3)
    for _ in range(2):                                            # the object can be walked again
        got = [b.numpy().copy() for b in feed]
        assert [g.shape[0] for g in got] == [4, 4, 3] and all(g.dtype == np.uint8 and g.shape[1:] == (6, 5, 3) for g in got)
        assert np.array_equal(np.concatenate(got), x)
    monkeypatch.undo()
    assert np.array_equal(np.load(path)["arr_0"], x)
    # one batch holds everything; a batch of one image
    assert np.array_equal(next(iter(NpzImageBatches(path, batch=64))).numpy(), x)
    assert len(NpzImageBatches(path, batch=1)) == 11
    assert np.array_equal(np.concatenate([b.numpy().copy() for b in NpzImageBatches(path, batch=1)]), x)
    # another key
    path2 = tmp_path / "named.npz"
    save(path2, images=x[:3], arr_0=x[3:5])
    assert np.array_equal(np.concatenate([b.numpy().copy() for b in NpzImageBatches(path2, key="images", batch=2)]), x[:3])


def test_a_batch_stays_valid_while_the_next_is_read(tmp_path, arrays):
    x, _ = arrays
    path = tmp_path / "b.npz"
    np.savez(path, x)
    it = iter(NpzImageBatches(path, batch=4))
    first = next(it)
    second = next(it)                                             # two buffers in turn
    assert np.array_equal(first.numpy(), x[:4]) and np.array_equal(second.numpy(), x[4:8])


def _npy_bytes(version, descr="|u1", fortran=False, shape=(2, 2, 2, 3), data=None):
    head = ("{'descr': %r, 'fortran_order': %r, 'shape': %r, }" % (descr, fortran, shape))
    pre = 10 if version == 1 else 12
    head = head + " " * (-(pre + len(head) + 1) % 64) + "\n"
    enc = head.encode("utf-8" if version == 3 else "latin1")
    out = b"\x93NUMPY" + bytes([version, 0]) + len(enc).to_bytes(2 if version == 1 else 4, "little") + enc
    return out + (data if data is not None else bytes(int(np.prod(shape)) * np.dtype(descr).itemsize))


def _npz(path, **members):
    with zipfile.ZipFile(path, "w") as zf:
        for k, v in members.items():
            zf.writestr(k + ".npy", v)
    return path


@pytest.mark.parametrize("version", [1, 2, 3])
def test_npy_header_versions(tmp_path, version):
    data = bytes(range(24))
    raw = _npy_bytes(version, data=data)
    assert read_npy_header(io.BytesIO(raw), "x") == ("|u1", False, (2, 2, 2, 3))
    assert np.array_equal(np.load(io.BytesIO(raw)), np.frombuffer(data, np.uint8).reshape(2, 2, 2, 3))      # numpy reads it the same way
    path = _npz(tmp_path / f"v{version}.npz", arr_0=raw)
    got = np.concatenate([b.numpy().copy() for b in NpzImageBatches(path, batch=1)])
    assert np.array_equal(got.reshape(-1), np.frombuffer(data, np.uint8))


def test_refusals_name_the_file(tmp_path, arrays):
    x, labels = arrays
    cases = {
        "fortran": (_npy_bytes(1, fortran=True), "Fortran"),
        "dtype": (_npy_bytes(1, descr="<f4"), "dtype"),
        "int8": (_npy_bytes(1, descr="|i1"), "dtype"),
        "rank": (_npy_bytes(1, shape=(2, 2, 6)), "shape"),
        "channels": (_npy_bytes(1, shape=(2, 2, 3, 2)), "shape"),
        "version": (b"\x93NUMPY" + bytes([4, 0]) + bytes(64), "version"),
        "magic": (b"not an npy file at all", "magic"),
    }
    for name, (raw, word) in cases.items():
        path = _npz(tmp_path / f"{name}.npz", arr_0=raw)
        with pytest.raises(ValueError) as e:
            NpzImageBatches(path)
        assert str(path) in str(e.value) and word in str(e.value), (name, str(e.value))
    path = tmp_path / "nokey.npz"
    np.savez(path, images=x)
    with pytest.raises(KeyError) as e:
        NpzImageBatches(path)
    assert str(path) in str(e.value) and "arr_0" in str(e.value) and "images" in str(e.value)
    # a member shorter than its header promises is an error, not a short batch
    path = _npz(tmp_path / "short.npz", arr_0=_npy_bytes(1, shape=(4, 2, 2, 3))[:-5])
    with pytest.raises(ValueError) as e:
        list(NpzImageBatches(path, batch=3))
    assert str(path) in str(e.value)
    with pytest.raises(ValueError):
        NpzImageBatches(tmp_path / "fortran.npz", batch=0)


def test_statistics_file_detection(tmp_path, arrays):
    x, labels = arrays
    imgs, stats, evaluator = tmp_path / "i.npz", tmp_path / "s.npz", tmp_path / "e.npz"
    np.savez(imgs, x, labels)
    np.savez(stats, mu=np.zeros(4), sigma=np.eye(4))
    np.savez(evaluator, mu=np.zeros(4), sigma=np.eye(4), mu_s=np.zeros(3), sigma_s=np.eye(3))
    assert not is_statistics_npz(imgs) and is_statistics_npz(stats) and is_statistics_npz(evaluator)


def test_statistics_file_rules(tmp_path):
    d, ds = 4, 3
    base = dict(mu=np.zeros(d), sigma=np.eye(d), mu_s=np.zeros(ds), sigma_s=np.eye(ds))
    feats = np.ones((5, d), dtype=np.float32)
    # the evaluator's own file: untagged, with mu_s -- accepted; Precision / Recall need the rows
    p = tmp_path / "evaluator.npz"
    np.savez(p, **base)
    got = adm_eval.load_statistics(p, need_features=False)
    assert got["features"] is None and got["mu_s"].shape == (ds,) and got["sigma_s"].shape == (ds, ds)
    with pytest.raises(RuntimeError) as e:
        adm_eval.load_statistics(p, need_features=True)
    assert "features" in str(e.value) and "--no-prdc" in str(e.value) and str(p) in str(e.value)
    # this project's file
    p = tmp_path / "adm.npz"
    np.savez(p, features=feats, network=np.asarray("inception-2015"), mode=np.asarray("adm"), **base)
    assert adm_eval.load_statistics(p, need_features=True)["features"].shape == (5, d)
    # another mode, another network, a plain {mu, sigma} file
    p = tmp_path / "clean.npz"
    np.savez(p, features=feats, network=np.asarray("inception-2015"), mode=np.asarray("clean"), **base)
    with pytest.raises(RuntimeError) as e:
        adm_eval.load_statistics(p, need_features=False)
    assert "clean" in str(e.value) and str(p) in str(e.value)
    p = tmp_path / "tv.npz"
    np.savez(p, network=np.asarray("torchvision"), **base)
    with pytest.raises(RuntimeError):
        adm_eval.load_statistics(p, need_features=False)
    p = tmp_path / "fid.npz"
    np.savez(p, mu=base["mu"], sigma=base["sigma"])
    with pytest.raises(RuntimeError) as e:
        adm_eval.load_statistics(p, need_features=False)
    assert "mu_s" in str(e.value)


def test_inception_score_chunk_bookkeeping():
    assert adm_eval.is_chunks(12, 5) == [(0, 5), (5, 10), (10, 12)]
    assert adm_eval.is_chunks(10, 5) == [(0, 5), (5, 10)]
    assert adm_eval.is_chunks(3, 5000) == [(0, 3)]
    with pytest.raises(ValueError):
        adm_eval.is_chunks(12, 0)
    # device batches of 4, 4, 4: the second straddles the first border, the third the second
    assert adm_eval.chunk_slices(0, 4, 12, 5) == [(0, 0, 4, 0)]
    assert adm_eval.chunk_slices(4, 4, 12, 5) == [(0, 0, 1, 4), (1, 1, 4, 0)]
    assert adm_eval.chunk_slices(8, 4, 12, 5) == [(1, 0, 2, 3), (2, 2, 4, 0)]
    # one batch over all three chunks; a batch that ends on a border
    assert adm_eval.chunk_slices(0, 12, 12, 5) == [(0, 0, 5, 0), (1, 5, 10, 0), (2, 10, 12, 0)]
    assert adm_eval.chunk_slices(5, 5, 12, 5) == [(1, 0, 5, 0)]
    # every image lands in exactly one chunk, at its own position, whatever the batching
    for batch in (1, 3, 5, 7, 12):
        seen = {c: [] for c in range(3)}
        for base in range(0, 12, batch):
            rows = min(batch, 12 - base)
            for c, a, b, i0 in adm_eval.chunk_slices(base, rows, 12, 5):
                assert len(seen[c]) == i0
                seen[c] += list(range(base + a, base + b))
        assert [seen[c] for c in range(3)] == [list(range(0, 5)), list(range(5, 10)), list(range(10, 12))]


def test_result_lines_are_in_the_evaluators_order():
    r = dict(recall=0.5, fid=1.0, precision=0.25, sfid=2.0, inception_score=3.0, n_ref=4)
    assert adm_eval.result_lines(r, " [t]") == ["Inception Score: 3.0 [t]", "FID: 1.0 [t]", "sFID: 2.0 [t]", "Precision: 0.25 [t]",
                                                "Recall: 0.5 [t]"]
    del r["precision"], r["recall"]
    assert [ln.split(":")[0] for ln in adm_eval.result_lines(r)] == ["Inception Score", "FID", "sFID"]


def test_more_than_one_rank_is_refused(monkeypatch, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError) as e:
        adm_eval.evaluate(str(tmp_path / "a.npz"), str(tmp_path / "b.npz"))
    assert "one process" in str(e.value)
