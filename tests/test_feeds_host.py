"""feeds.py without a GPU: which loader every site picks for every combination of the feed flags and kind of shard (the table
below restates the decision of the commit BEFORE feeds.py existed, read off its code line by line -- it never calls choose), and
the life cycle of a feed session with stub loaders: close() exactly once on every road out, the feed line on the main rank only,
one fall-back to the DataLoader in one process, a RuntimeError under torchrun, ``feeds.last``."""
import itertools
import os

import numpy as np
import pytest
from PIL import Image

from tests import _cases, _jpeg_cases as jc, _png_cases
from tise_toolbox_amd import feeds, png_ring

PNG, JPEG, CROP = ("ring", "dataloader"), (None, "native", "pillow"), (None, "native", "dataloader")
ANY = object()


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    """kind of shard -> files: JPEG files of the native subset (one size; ragged), native-subset PNG files, palette PNG files
    (outside the subset), no file at all."""
    from tise_toolbox_amd import build, crop_feed, jpeg_feed
    build.build_jpeg(force=False, verbose=False)
    build.build_png(force=False, verbose=False)
    root = tmp_path_factory.mktemp("feeds")
    imgs = _cases.smooth_images(3, 40, 56, seed=5)
    out = {"empty": [], "jpeg": [], "jpeg-ragged": [], "png": [], "palette": []}
    for i, im in enumerate(imgs):
        for kind, pix in (("jpeg", im), ("jpeg-ragged", im[:40 - 8 * i, :56 - 8 * i])):
            out[kind].append(str(root / f"{kind}_{i}.jpg"))
            jc.save_jpeg(np.ascontiguousarray(pix), out[kind][-1], quality=85, subsampling=2)
        out["png"].append(str(root / f"rgb_{i}.png"))
        open(out["png"][-1], "wb").write(_png_cases.write_png(im, [(i + y) % 5 for y in range(im.shape[0])]))
        out["palette"].append(str(root / f"pal_{i}.png"))
        Image.fromarray(im).convert("P", palette=Image.ADAPTIVE, colors=16).save(out["palette"][-1])
    # the premises of the table: what the two probes (untouched by feeds.py) say about the first file of each shard
    assert jpeg_feed.probe_file(out["jpeg"][0]) and jpeg_feed.probe_file(out["jpeg-ragged"][0])
    assert not jpeg_feed.probe_file(out["png"][0]) and not jpeg_feed.probe_file(out["palette"][0])
    assert crop_feed.probe_file(out["png"][0]) and not crop_feed.probe_file(out["palette"][0]) and not crop_feed.probe_file(out["jpeg"][0])
    return out


# site -> decision list (png_feed, jpeg_feed, crop_feed, shard kinds) -> kind, first match wins; ANY = the site never looks at it.
# File:line are those of the commit before feeds.py ("Pin the retrieval kernel to CLIP.forward's rounding, bit for bit").
ALL, FILES = ("empty", "jpeg", "jpeg-ragged", "png", "palette"), ("jpeg", "jpeg-ragged", "png", "palette")
TABLE = {
    "FID": (feeds.FID, [                                                    # fid_score._compute_statistics_of_path
        # fid_score.py:441 -> :326 (ring and a non-empty shard) -> jpeg_feed.py:95 (native: the first file is a native JPEG)
        (("ring",), ("native",), ANY, ("jpeg", "jpeg-ragged"), "jpeg"),
        # fid_score.py:441 -> :326 -> jpeg_feed.py:97-105 (flag unset: only when the first files differ in size)
        (("ring",), (None,), ANY, ("jpeg-ragged",), "jpeg"),
        # fid_score.py:448 (--crop-feed native and a non-empty shard, whatever --png-feed says and whatever the files are)
        (ANY, ANY, ("native",), FILES, "crop"),
        # fid_score.py:455 (ring, the empty shard included: loader None, nothing is started)
        (("ring",), ANY, ANY, ALL, "ring"),
        # fid_score.py:501 (what is left)
        (("dataloader",), ANY, ANY, ALL, "dataloader"),
    ]),
    "per-class": (feeds.CROPS, [                                            # fid_score._class_statistics
        # fid_score.py:700 -> crop_feed.py:92 (dataloader, or no file)
        (ANY, ANY, ("dataloader",), ALL, "dataloader"),
        (ANY, ANY, ANY, ("empty",), "dataloader"),
        # fid_score.py:700 -> crop_feed.py:94-96 (asked for by name: any file)
        (ANY, ANY, ("native",), FILES, "crop"),
        # fid_score.py:700 -> crop_feed.py:97 (flag unset: the first file probes as a PNG of the native subset)
        (ANY, ANY, (None,), ("png",), "crop"),
        # fid_score.py:704-708 (flag unset, another first file)
        (ANY, ANY, (None,), ("jpeg", "jpeg-ragged", "palette"), "dataloader"),
    ]),
    "O-IS": (feeds.CROPS, [                                                 # object_centric_inception_score.inception_score
        # object_centric_inception_score.py:83 -> crop_feed.py:92
        (ANY, ANY, ("dataloader",), ALL, "dataloader"),
        (ANY, ANY, ANY, ("empty",), "dataloader"),
        # object_centric_inception_score.py:83-84 -> crop_feed.py:94-96
        (ANY, ANY, ("native",), FILES, "crop"),
        # object_centric_inception_score.py:83-84 -> crop_feed.py:97
        (ANY, ANY, (None,), ("png",), "crop"),
        # object_centric_inception_score.py:87-91
        (ANY, ANY, (None,), ("jpeg", "jpeg-ragged", "palette"), "dataloader"),
    ]),
    "IS": (feeds.IS, [                                                      # inception_score.feed_images
        # inception_score.py:130-132 (ring, hi > lo) -> jpeg_feed.py:95
        (("ring",), ("native",), ANY, ("jpeg", "jpeg-ragged"), "jpeg"),
        # inception_score.py:130-132 -> jpeg_feed.py:97-105
        (("ring",), (None,), ANY, ("jpeg-ragged",), "jpeg"),
        # inception_score.py:154 (ring, hi > lo)
        (("ring",), ANY, ANY, FILES, "ring"),
        # inception_score.py:167-168 (--png-feed loader, or an empty range)
        (ANY, ANY, ANY, ALL, "dataloader"),
    ]),
    "RP / PA": (feeds.CLIP, [                                               # RP_coco.embed_paths
        # RP_coco.py:182 (ring and at least one path)
        (("ring",), ANY, ANY, FILES, "ring"),
        # RP_coco.py:193
        (ANY, ANY, ANY, ALL, "dataloader"),
    ]),
}


def _expected(rows, png, jpeg, crop, shard):
    for r_png, r_jpeg, r_crop, r_shards, kind in rows:
        if (r_png is ANY or png in r_png) and (r_jpeg is ANY or jpeg in r_jpeg) and (r_crop is ANY or crop in r_crop) and shard in r_shards:
            return kind
    raise AssertionError(("no row", png, jpeg, crop, shard))


@pytest.mark.parametrize("site", list(TABLE))
def test_choose_picks_what_the_sites_picked_before(shards, site):
    allow, rows = TABLE[site]
    n = 0
    for png, jpeg, crop, shard in itertools.product(PNG, JPEG, CROP, ALL):
        got = feeds.choose(shards[shard], feeds.Options(png, jpeg, crop), allow)
        assert got == _expected(rows, png, jpeg, crop, shard), (site, png, jpeg, crop, shard, got)
        n += 1
    assert n == 2 * 3 * 3 * 5
    # the IS CLIs' spelling of the DataLoader mode
    assert feeds.Options("loader") == feeds.Options("dataloader")
    assert feeds.choose(shards["png"], feeds.Options("loader"), allow) == feeds.choose(shards["png"], feeds.Options("dataloader"), allow)


def test_resolve_workers_equals_the_expression_it_replaces():
    for world in (1, 8):
        for w in (None, 0, -1, "3", 5):
            want = int(w) if w and int(w) > 0 else png_ring.auto_workers(world)      # fid_score._num_workers of the commit before
            assert feeds.resolve_workers(w, world) == want, (w, world)
    assert feeds.resolve_workers("3", 8) == 3 and feeds.resolve_workers(5, 1) == 5 and feeds.resolve_workers(-1, 8) == png_ring.auto_workers(8)


class _Stub:
    """A loader of three items; ``ragged_at`` = k: RaggedImages instead of item k."""
    num_workers = workers = 2

    def __init__(self, kind, ragged_at=None):
        self.kind, self.ragged_at, self.closed = kind, ragged_at, 0

    def __iter__(self):
        for k in range(3):
            if k == self.ragged_at:
                raise png_ring.RaggedImages(f"000{k}.png: 7x9 where the first image is 8x8")
            yield k

    def close(self):
        self.closed += 1

    def feed_line(self, wall):
        return f"[tise] {self.kind} feed: stub"


RING_SITE = feeds.Site(("ring", "dataloader"), True, png_line=True)         # the plain FID site without the probing kinds
FILES2 = ["a.png", "b.png"]


@pytest.fixture
def stubs(monkeypatch):
    built = []

    def build_loader(kind, files, device, **kw):
        built.append(_Stub(kind, ragged_at=1 if kind == "ring" and stubs_ragged[0] else None))
        return built[-1]
    stubs_ragged = [False]
    monkeypatch.setattr(feeds, "build_loader", build_loader)
    monkeypatch.setattr(feeds, "last", feeds.Last(None, None))
    return built, stubs_ragged


def test_success_closes_once_prints_on_the_main_rank_only_and_is_remembered(stubs, monkeypatch, capsys):
    built, _ = stubs
    site = feeds.Site(("crop",), False, crop_on_request=True)
    seen = []
    out = feeds.run(site, FILES2, feeds.Options(crop_feed="native"), lambda ld: seen.append(list(ld)) or "result", "cpu", 2)
    assert out == "result" and seen == [[0, 1, 2]] and [(s.kind, s.closed) for s in built] == [("crop", 1)]
    assert capsys.readouterr().err == "[tise] crop feed: stub\n"
    assert feeds.last == feeds.Last("crop", built[0])
    monkeypatch.setattr(feeds.tdist, "is_main", lambda: False)             # another rank: the same run, no line
    feeds.run(site, FILES2, feeds.Options(crop_feed="native"), list, "cpu", 2)
    assert capsys.readouterr().err == "" and built[1].closed == 1 and feeds.last.loader is built[1]


def test_ragged_ring_falls_back_once_in_one_process(stubs, capsys):
    built, ragged = stubs
    ragged[0] = True
    calls = []

    def consume(loader):
        calls.append(loader)
        assert all(s.closed == 1 for s in built[:-1]) and loader.closed == 0      # the ring is closed before the second call
        return list(loader)
    assert feeds.run(RING_SITE, FILES2, feeds.Options(), consume, "cpu", 2) == [0, 1, 2]
    assert [s.kind for s in calls] == ["ring", "dataloader"] and calls == built
    assert [s.closed for s in built] == [1, 1]
    err = capsys.readouterr().err
    assert err.count("falling back to the DataLoader path") == 1 and "0001.png" in err
    lines = [ln for ln in err.splitlines() if "falling back" not in ln]
    assert len(lines) == 1 and "DataLoader decode workers" in lines[0] and "shared pinned ring" not in err    # no line for the failed attempt
    assert feeds.last == feeds.Last("dataloader", built[1])


def test_ragged_ring_raises_under_torchrun(stubs, monkeypatch, capsys):
    built, ragged = stubs
    ragged[0] = True
    monkeypatch.setattr(feeds.tdist, "env_world", lambda: (1, 2, 1))
    calls = []
    with pytest.raises(RuntimeError, match="use --png-feed dataloader") as info:
        feeds.run(RING_SITE, FILES2, feeds.Options(), lambda ld: calls.append(ld) or list(ld), "cpu", 2)
    assert isinstance(info.value.__cause__, png_ring.RaggedImages)
    assert len(calls) == 1 and [(s.kind, s.closed) for s in built] == [("ring", 1)]
    assert "[tise]" not in capsys.readouterr().err
    assert feeds.last == feeds.Last("ring", built[0])
    # a site whose consume holds no collective (RP / PA) lets the rank fall back alone, as before
    calls.clear()
    assert feeds.run(RING_SITE._replace(ragged_raises=False), FILES2, feeds.Options(), lambda ld: calls.append(ld) or list(ld), "cpu", 2) == [0, 1, 2]
    assert len(calls) == 2 and [s.closed for s in built] == [1, 1, 1]


def test_an_unrelated_error_closes_once_and_passes_through(stubs, capsys):
    built, _ = stubs

    def consume(loader):
        next(iter(loader))
        raise KeyError("boom")
    with pytest.raises(KeyError, match="boom"):
        feeds.run(RING_SITE, FILES2, feeds.Options(), consume, "cpu", 2)
    assert [(s.kind, s.closed) for s in built] == [("ring", 1)] and feeds.last == feeds.Last("ring", built[0])
    assert capsys.readouterr().err == ""


def test_site_arguments_reach_the_loader_and_the_dataloader_is_the_sites(monkeypatch):
    import torch
    seen = []
    monkeypatch.setattr(feeds, "build_loader", lambda kind, files, device, **kw: seen.append((kind, kw)) or _Stub(kind))
    lazy = []
    feeds.run(feeds.IS, [], feeds.Options(num_workers=3), list, "cpu", 50,
              loader_args={"jpeg": lambda: lazy.append(1) or {}, "ring": {"batch_size": 1}})
    assert seen == [("dataloader", {"batch_size": 50, "workers": 3, "drop_last": False})] and not lazy      # made only for the chosen kind
    feeds.run(feeds.CLIP, FILES2, feeds.Options(num_workers=3), list, "cpu", 50, loader_args={"ring": {"batch_size": 1, "group": 50, "rgb_only": True}})
    assert seen[-1] == ("ring", {"batch_size": 1, "workers": 3, "drop_last": False, "group": 50, "rgb_only": True})
    # the uint8 DataLoader of the CLIs, and a caller's own dataset taken as it is (O-IS)
    dl = feeds.u8_dataloader(FILES2, 8, 40, True)
    assert (dl.batch_size, dl.drop_last, dl.num_workers, dl.pin_memory) == (8, True, 32, True)
    assert dl.collate_fn is feeds.img_data.collate_u8 and dl.worker_init_fn is feeds.img_data.worker_init and dl.dataset.file_names == FILES2
    ds = torch.utils.data.TensorDataset(torch.zeros(5, 3))
    own = feeds.u8_dataloader(torch.utils.data.Subset(ds, range(1, 4)), 2, 40, False, pin_memory=False, collate=None, max_workers=None)
    assert (own.num_workers, own.pin_memory, own.drop_last, len(own.dataset)) == (40, False, False, 3)
    assert own.collate_fn is torch.utils.data.dataloader.default_collate
