"""GPU parity of the R-precision / positional-alignment reduction (section 8 f3): csrc/retrieval.hip through the
C ABI against oracle/rp_oracle.py (fp64) and against what the reference scripts wrote (stub-CLIP fixtures)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import rp_oracle
from tests import _retrieval_cases as rc

pytestmark = pytest.mark.gpu


def _oracle_verdict(top1, p0, img, txt, index, normalize, scale, dtype, seed_note):
    """rp_oracle.clip_forward_probs_batched on exactly the values the kernel saw, and tests/_retrieval_cases.judge:
    bit-exact at every settled item, one unit in the last place at an unsettled probability.  Conditions on the data,
    asserted on the oracle's own counts: no unsettled item in fp16, no unsettled norm, unsettled probabilities in at most
    10 % of an fp32 case.  At 1501 items x 100 candidates x d = 512 in fp32 no seed avoids unsettled DOT PRODUCTS (the
    worst-case band of a 512-term sum, times 8, catches one logit in ~850): those items get the interval that a move of
    their logits by one fp32 spacing allows (judge), everything else the strict rule."""
    n = img.shape[0]
    probs, settled, flipped, eps = [], [], [], []
    for lo in range(0, n, 1000):                                         # slabs: the 30 000-item gather is 3 GB at once
        ix = slice(lo, min(n, lo + 1000))
        cand = txt[index[ix]] if index is not None else txt.reshape(n, -1, txt.shape[1])[ix]
        pr, ok, flags = rp_oracle.clip_forward_probs_batched(img[ix], cand, scale, normalize, dtype, detail=True)
        assert not flags["norm"].any(), seed_note
        assert ok.all() if dtype == np.float16 else flags["prob"].sum() <= 0.10 * len(ok), seed_note
        probs.append(pr), settled.append(ok), flipped.append(flags["dot"]), eps.append(flags["eps"])
    probs, settled, flipped, eps = (np.concatenate(x) for x in (probs, settled, flipped, eps))
    print(f"{seed_note}: unsettled {int((~settled).sum())} of {n}, {int(flipped.sum())} of them by a dot product")
    p0 = p0 if p0 is not None else probs[:, 0].astype(np.float32)
    assert rc.judge(top1, p0, probs, settled, np.dtype(dtype), flipped=flipped, eps=eps) == []
    return probs, settled


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("d,c,use_index,normalize", [(512, 100, True, True), (512, 100, True, False), (768, 7, False, True),
                                                     (100, 33, True, True), (1024, 2, False, False), (64, 1, True, True)])
def test_cosine_top1_matches_fp64_oracle(cuda_device, dtype, d, c, use_index, normalize):
    from tise_toolbox_amd import device
    rng = np.random.default_rng(d + c)
    n, rows = 1501, 4000
    img = rng.standard_normal((n, d)).astype(np.float32)
    if use_index:
        txt = rng.standard_normal((rows, d)).astype(np.float32)
        index = rng.integers(0, rows, size=(n, c)).astype(np.int32)
        # make about half of the items retrieve candidate 0
        for i in range(0, n, 2):
            txt[index[i, 0]] = img[i] + 0.7 * rng.standard_normal(d).astype(np.float32)
    else:
        txt = rng.standard_normal((n * c, d)).astype(np.float32)
        index = None
    if not normalize:
        img /= np.linalg.norm(img, axis=1, keepdims=True)
        txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    ti = torch.from_numpy(img).to(cuda_device).to(dtype)
    tt = torch.from_numpy(txt).to(cuda_device).to(dtype)
    tidx = torch.from_numpy(index).to(cuda_device) if index is not None else None
    top1, p0 = device.cosine_top1(ti, tt, tidx, normalize=normalize, logit_scale=100.0)
    # the oracle sees exactly the values the kernel sees and rounds like CLIP.forward (fp16 model / fp32 model)
    npdt = np.float16 if dtype == torch.float16 else np.float32
    got1 = top1.cpu().numpy()
    _oracle_verdict(got1, p0.cpu().numpy(), ti.cpu().numpy(), tt.cpu().numpy(), index, normalize, 100.0, npdt, (d, c))
    again, p0_again = device.cosine_top1(ti, tt, tidx, normalize=normalize, logit_scale=100.0)
    assert torch.equal(again, top1) and torch.equal(p0_again.view(torch.int32), p0.view(torch.int32))
    if c > 1 and use_index:
        assert 0.2 < float((got1 == 0).mean()) < 0.9


def test_rp_full_size_30k_items_100_candidates(cuda_device):
    """BASELINE configs[3] at its FULL size through the scoring path: 30 000 items x (1 true + 99 mismatched) candidates
    drawn from 40 000 distinct caption embeddings, d = 512, fp16 (the model clip.load serves on a GPU).  Every item against
    the oracle (rp_oracle.clip_forward_probs_batched: what CLIP.forward + softmax round; every item settled, so every
    top-1 exact), the ten bin scores / mean / std against rp_oracle.rp_score on the oracle's own success flags, and the
    size-independent property the 8-GPU run relies on: per-bin {successes, count} of 8 item shards add up to the
    one-process result."""
    from tise_toolbox_amd import RP_coco, device
    rng = np.random.default_rng(30)
    n, c, d, rows = 30000, 100, 512, 40000
    txt = rng.standard_normal((rows, d)).astype(np.float32)
    img = rng.standard_normal((n, d)).astype(np.float32)
    index = rng.integers(0, rows, size=(n, c)).astype(np.int32)
    hit = rng.random(n) < 0.55                                           # ~55 % of the items retrieve their true caption
    img[hit] = txt[index[hit, 0]] + 2.0 * rng.standard_normal((int(hit.sum()), d)).astype(np.float32)
    ti = torch.from_numpy(img).to(cuda_device).half()
    tt = torch.from_numpy(txt).to(cuda_device).half()
    tidx = torch.from_numpy(index).to(cuda_device)
    top1, _ = device.cosine_top1(ti, tt, tidx, normalize=True, logit_scale=100.0, want_p0=False)
    got = (top1 == 0).cpu().numpy().astype(np.int64)
    probs, _ = _oracle_verdict(top1.cpu().numpy(), None, ti.cpu().numpy(), tt.cpu().numpy(), index, True, 100.0, np.float16, 30)
    want = (np.argmax(probs, 1) == 0).astype(np.int64)
    assert np.array_equal(got, want)
    assert 0.4 < got.mean() < 0.7
    perm = RP_coco.shuffled_ids(n, 11)
    mean, std, scores = RP_coco.r_precision(ti, tt, tidx, perm)
    m2, s2, sc2 = rp_oracle.rp_score(want, perm)
    assert (mean, std) == (m2, s2) and list(scores) == list(sc2)
    sums = np.zeros((10, 2))
    for r in range(8):
        lo, hi_ = r * n // 8, (r + 1) * n // 8
        t1, _ = device.cosine_top1(ti[lo:hi_], tt, tidx[lo:hi_], normalize=True, logit_scale=100.0, want_p0=False)
        sums += RP_coco.bin_sums((t1 == 0).cpu().numpy().astype(np.int64), lo, perm)
    m8, s8, _ = RP_coco.r_precision_from_bin_sums(sums)
    assert (m8, s8) == (mean, std)


@pytest.mark.parametrize("name", ["rp_stub_57x10.npz", "rp_stub_40x100.npz"])
def test_rp_through_the_kernel_reproduces_reference_text(cuda_device, golden_dir, name):
    """The fixture's logits (what the stub CLIP returned inside the reference script) are fed as 1-d 'embeddings'
    (txt_j = logit_j, img = 1, raw dot product): bins + kernel + reduction must write the reference's text."""
    from tise_toolbox_amd import RP_coco
    g = np.load(os.path.join(golden_dir, name))
    logits = g["logits"]
    n, c = logits.shape
    d = 64
    img = torch.zeros((n, d), device=cuda_device)
    img[:, 0] = 1.0
    txt = torch.zeros((n * c, d), device=cuda_device)
    txt[:, 0] = torch.from_numpy(logits.reshape(-1)).float().to(cuda_device)
    index = torch.arange(n * c, dtype=torch.int32, device=cuda_device).view(n, c)
    mean, std, _ = RP_coco.r_precision(img, txt, index, g["perm"].tolist(), normalize=False, logit_scale=1.0)
    assert f"R-precision: {mean} +- {std}" == str(g["expected_text"])


def test_pa_through_the_kernel_reproduces_reference_text(cuda_device, golden_dir):
    from tise_toolbox_amd import device
    g = json.load(open(os.path.join(golden_dir, "pa_stub.json")))
    scores = []
    for p in g["phrases"]:
        lg = torch.tensor(g["logits"][p], dtype=torch.float32, device=cuda_device)          # (n, 2) [true, false]
        n = lg.shape[0]
        img = torch.zeros((n, 64), device=cuda_device); img[:, 0] = 1.0
        txt = torch.zeros((2 * n, 64), device=cuda_device); txt[:, 0] = lg.reshape(-1)
        _, p0 = device.cosine_top1(img, txt, None, normalize=False, logit_scale=1.0)
        ok = (p0 > 0.6).float()                                                              # PA.py:41
        scores.append(float(ok.sum().item()) / n)
    assert f"PA = {np.mean(scores)}" == g["expected_text"]


def test_rp_cli_end_to_end_with_stand_in_towers(cuda_device, tmp_path):
    """Whole drop-in: pickle + PNGs -> towers (seeded stand-ins, fp16 like clip.load on a GPU) -> kernel -> file.
    Checked against the oracle applied to the SAME embeddings (the towers themselves: parity unpinned)."""
    from PIL import Image
    from tise_toolbox_amd import RP_coco, clip_model
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    words = ["a", "red", "bus", "dog", "on", "the", "grass", "two", "people", "near", "table"]
    model, scale = RP_coco.build_towers(None, cuda_device)

    def make_case(data_seed, root):
        rng = np.random.default_rng(data_seed)
        items = []
        img_dir = root / f"images{data_seed}"
        img_dir.mkdir()
        pool = [" ".join(rng.choice(words, 5)) + f" x{k}" for k in range(30)]          # mismatched captions repeat
        for i in range(23):
            items.append({"caption_id": 100 + i, "caption": " ".join(rng.choice(words, 5)) + f" {i}",
                          "mismatched_captions": [pool[(i * 3 + 5 * j) % 30] for j in range(6)]})
            Image.fromarray(rng.integers(0, 256, (64, 80, 3), dtype=np.uint8)).save(img_dir / f"{100 + i}.png")
        # oracle on the embeddings of the towers the CLI builds (csrc/clip_ops.hip by default)
        caps, index = RP_coco.caption_table(items)
        assert len(caps) < 23 * 7                                         # captions are de-duplicated
        txt = RP_coco.embed_texts(model, clip_model.HashTokenizer(), caps, cuda_device, 8).float().cpu().numpy().astype(np.float64)
        img = RP_coco.embed_images(model, str(img_dir), [it["caption_id"] for it in items], cuda_device, 8, workers=0)
        img = img.float().cpu().numpy().astype(np.float64)
        success, margins = [], []
        for i in range(len(items)):
            lg = rp_oracle.clip_logits(img[i], txt[index[i]], scale, normalize=False)
            success.append(int(np.argmax(lg) == 0))
            margins.append(np.sort(lg)[-1] - np.sort(lg)[-2])
        return items, img_dir, success, min(margins)

    # the fp64 oracle is only an oracle where no item is a near-tie (the kernel rounds what CLIP.forward rounds: the test
    # below covers that side): take the first data seed whose smallest top-1 margin is clear, and REQUIRE that one exists
    case = None
    for data_seed in range(8):
        items, img_dir, success, margin = make_case(data_seed, tmp_path)
        if margin > 1e-3:
            case = (items, img_dir, success)
            break
    assert case is not None, "no data seed in 0..7 without a near-tie"
    items, img_dir, success = case
    pkl = tmp_path / "rp.pkl"
    pickle.dump(items, open(pkl, "wb"))
    out = tmp_path / "rp.txt"
    mean, std = RP_coco.main(["--image_dir", str(img_dir), "--rp_input_file", str(pkl), "--saved_file_path", str(out),
                              "--gpu_id", str(cuda_device.index or 0), "--seed", "4", "--batch-size", "8",
                              "--num-workers", "0", "--synthetic-weights"])
    assert open(out).read() == f"R-precision: {mean} +- {std}" + SYNTHETIC_TAG
    m2, s2, _ = rp_oracle.rp_score(success, RP_coco.shuffled_ids(len(items), 4))
    assert (m2, s2) == (mean, std)


def test_fp16_near_ties_resolve_like_clip_forward(cuda_device):
    """with the fp16 model the reference compares fp16 softmax outputs and np.argmax takes the FIRST
    maximum, so a distractor whose logit exceeds the true caption's by less than the fp16 rounding still loses.
    Constructed items (all inputs exactly representable in fp16): img = (1, 1, 0, ...), true caption (b, 0, ...),
    distractor 3 = (b, e, ...): its logit is larger by 100 e, from 1e-4 to 0.4, around the fp16 spacing of logits
    near 30 (0.0156)."""
    from tise_toolbox_amd import device
    d, c = 64, 8
    es = [0.0, 2.0 ** -20, 2.0 ** -18, 2.0 ** -16, 2.0 ** -14, 2.0 ** -12, 2.0 ** -10, 2.0 ** -8]
    n = len(es)
    b = float(np.float16(0.3))
    img = np.zeros((n, d), np.float32); img[:, 0] = 1.0; img[:, 1] = 1.0
    txt = np.zeros((n * c, d), np.float32)
    for i, e in enumerate(es):
        for j in range(c):
            txt[i * c + j, 0] = b if j in (0, 3) else float(np.float16(b - 0.05 * j))
        txt[i * c + 3, 1] = e
    ti = torch.from_numpy(img).to(cuda_device).half()
    tt = torch.from_numpy(txt).to(cuda_device).half()
    assert torch.equal(tt.float().cpu(), torch.from_numpy(txt))              # nothing lost in the inputs
    top1, p0 = device.cosine_top1(ti, tt, None, normalize=False, logit_scale=100.0)
    want = [int(np.argmax(rp_oracle.clip_forward_probs(ti[i].cpu().numpy(), tt[i * c:(i + 1) * c].cpu().numpy(), 100.0, False, np.float16)))
            for i in range(n)]
    exact = [int(np.argmax(rp_oracle.clip_logits(img[i], txt[i * c:(i + 1) * c], 100.0, False))) for i in range(n)]
    assert top1.cpu().tolist() == want
    assert exact == [0] + [3] * (n - 1)                                       # in exact arithmetic every e > 0 wins
    assert want[:4] == [0, 0, 0, 0] and want[-3:] == [3, 3, 3]                # below half an fp16 ulp of the logit: tie -> 0
    # the fp32 model (CPU path of the reference) resolves all of them
    top1_32, _ = device.cosine_top1(ti.float(), tt.float(), None, normalize=False, logit_scale=100.0)
    assert top1_32.cpu().tolist() == exact


@pytest.mark.parametrize("d", [64, 768])
def test_fp16_near_ties_under_normalize_resolve_like_clip_forward(cuda_device, d):
    """The same question with normalize=True, in both kernel instances.  Every vector but one has four equal non-zero
    entries, so its norm (2|x|) and its quotients (1/2) are exact in fp16.  img = four ones; distractor 3 = four b
    (cosine exactly 1); the TRUE caption = the same four b plus e in a direction the image does not have, so in exact
    arithmetic the distractor wins for every e > 0.  In fp16 the true caption's norm and quotients round back to the
    distractor's until e reaches 2^-5: an exact tie of rounded probabilities, which index 0 wins.  The other candidates
    share three of the four positions (logit 75).  For d = 768 the fourth position and e sit in the lane strides only
    the KMAX = 16 instance reads.  Every item is settled in the oracle's sense, so the kernel has no freedom."""
    from tise_toolbox_amd import device
    es = [0.0] + [2.0 ** -k for k in (20, 14, 10, 8, 7, 6, 5, 4, 3, 2)]
    n, c, hi = len(es), 8, d - 60
    b = float(np.float16(0.3))
    img = np.zeros((n, d), np.float32)
    img[:, [0, 1, 2, hi]] = 1.0
    cand = np.zeros((n, c, d), np.float32)
    for i, e in enumerate(es):
        for j in range(c):
            cand[i, j, [0, 1, 2]] = b
            cand[i, j, hi if j in (0, 3) else hi - 8 - j] = b
        cand[i, 0, hi + 5] = e
    assert np.array_equal(cand.astype(np.float16).astype(np.float32), cand)       # nothing lost in the inputs
    exact = [int(np.argmax(rp_oracle.clip_logits(img[i], cand[i], 100.0, True))) for i in range(n)]
    assert exact == [0] + [3] * (n - 1)
    for dtype, want in ((np.float16, [0] * 7 + [3] * 4), (np.float32, [0] * 3 + [3] * 8)):
        probs, settled = rp_oracle.clip_forward_probs_batched(img, cand, 100.0, True, dtype)
        assert settled.all() and np.argmax(probs, 1).tolist() == want
        ti = torch.from_numpy(img.astype(dtype)).to(cuda_device)
        tt = torch.from_numpy(cand.astype(dtype).reshape(n * c, d)).to(cuda_device)
        top1, p0 = device.cosine_top1(ti, tt, None, normalize=True, logit_scale=100.0)
        assert rc.judge(top1.cpu().numpy(), p0.cpu().numpy(), probs, settled, np.dtype(dtype)) == []
        assert top1.cpu().tolist() == want
        assert p0.cpu().tolist()[:7 if dtype == np.float16 else 3] == [0.5] * (7 if dtype == np.float16 else 3)


def test_fp16_near_ties_resolve_like_clip_forward_in_the_wide_instance(cuda_device):
    """test_fp16_near_ties_resolve_like_clip_forward at d = 768, the deciding entries in lane strides 10 and 11."""
    from tise_toolbox_amd import device
    d, c, hi = 768, 8, 700
    es = [0.0, 2.0 ** -20, 2.0 ** -18, 2.0 ** -16, 2.0 ** -14, 2.0 ** -12, 2.0 ** -10, 2.0 ** -8]
    n = len(es)
    b = float(np.float16(0.3))
    img = np.zeros((n, d), np.float16)
    img[:, [640, hi]] = 1.0
    cand = np.zeros((n, c, d), np.float16)
    for i, e in enumerate(es):
        for j in range(c):
            cand[i, j, 640] = b if j in (0, 3) else np.float16(b - 0.05 * j)
        cand[i, 3, hi] = e
    probs, settled = rp_oracle.clip_forward_probs_batched(img, cand, 100.0, False, np.float16)
    want = np.argmax(probs, 1).tolist()
    assert settled.all() and want[:4] == [0, 0, 0, 0] and want[-3:] == [3, 3, 3]
    top1, p0 = device.cosine_top1(torch.from_numpy(img).to(cuda_device), torch.from_numpy(cand.reshape(n * c, d)).to(cuda_device), None,
                                  normalize=False, logit_scale=100.0)
    assert rc.judge(top1.cpu().numpy(), p0.cpu().numpy(), probs, settled, np.dtype(np.float16)) == []


def _pa_fixture(tmp_path, n_per_phrase=(7, 5, 9)):
    from PIL import Image
    rng = np.random.default_rng(2)
    phrases = ["on top of", "under", "left of"]
    data = {}
    for p, n in zip(phrases, n_per_phrase):
        (tmp_path / "images" / p).mkdir(parents=True)
        data[p] = []
        for i in range(n):
            cid = 30 + i
            data[p].append({"caption_id": cid, "caption": f"a cup {p} a table {i}", "false_caption": f"a table {p} a cup {i}"})
            Image.fromarray(rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)).save(tmp_path / "images" / p / f"{cid}.png")
    pkl = tmp_path / "pa.pkl"
    pickle.dump(data, open(pkl, "wb"))
    return data, pkl


def test_pa_cli_end_to_end_and_two_ranks(cuda_device, tmp_path):
    """PA.py drop-in (positional_alignment/PA.py): pickle + image_dir/<phrase>/<id>.png -> `PA = value`; the value is
    the oracle's on the same embeddings (fp16 CLIP.forward rounding), and a 2-rank run (items sharded, per-phrase
    {success, total} all-reduced) writes the same text."""
    from tise_toolbox_amd import PA, clip_model
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    from tests.test_gpu_pipeline import _run_ranks
    data, pkl = _pa_fixture(tmp_path)
    out = tmp_path / "pa.txt"
    argv = ["--image_dir", str(tmp_path / "images"), "--pa_input_file", str(pkl), "--saved_file_path", str(out),
            "--gpu_id", "0", "--num-workers", "0", "--synthetic-weights", "--batch-size", "4"]
    val = PA.main(argv)
    assert out.read_text() == f"PA = {val}" + SYNTHETIC_TAG
    from tise_toolbox_amd.RP_coco import build_towers
    model, scale = build_towers(None, cuda_device)
    scores = []
    for p, items in data.items():
        caps = [c for it in items for c in (it["caption"], it["false_caption"])]
        from tise_toolbox_amd.RP_coco import embed_texts
        txt = embed_texts(model, clip_model.HashTokenizer(), caps, cuda_device, 8).cpu().numpy()
        img = PA._embed_paths(model, [str(tmp_path / "images" / p / f"{it['caption_id']}.png") for it in items], cuda_device, 8, workers=0).cpu().numpy()
        ok = [float(rp_oracle.clip_forward_probs(img[i], txt[2 * i:2 * i + 2], scale, False, np.float16)[0] > 0.6) for i in range(len(items))]
        scores.append(sum(ok) / len(ok))
    assert abs(val - float(np.mean(scores))) <= 1e-12
    out2 = tmp_path / "pa2.txt"
    res = _run_ranks(2, argv[:5] + [str(out2)] + argv[6:], tmp_path, module="tise_toolbox_amd.PA")
    assert all(rc == 0 for rc, _ in res), res
    assert out2.read_text() == out.read_text()
    with pytest.raises(RuntimeError, match="no parameters for CLIP"):
        PA.main([a for a in argv if a != "--synthetic-weights"])


def test_rp_cli_two_ranks_equals_one(cuda_device, tmp_path):
    """Item-sharded RP under 2 ranks (gloo rendezvous on this box's GPU; nccl = RCCL on a node): same seed, same text."""
    from PIL import Image
    from tise_toolbox_amd import RP_coco
    from tests.test_gpu_pipeline import _run_ranks
    rng = np.random.default_rng(1)
    words = ["a", "red", "bus", "dog", "on", "the", "grass", "two", "people", "near", "table"]
    img_dir = tmp_path / "images"; img_dir.mkdir()
    items = []
    for i in range(27):
        items.append({"caption_id": 500 + i, "caption": " ".join(rng.choice(words, 5)) + f" {i}",
                      "mismatched_captions": [" ".join(rng.choice(words, 5)) + f" m{i}_{j}" for j in range(5)]})
        Image.fromarray(rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)).save(img_dir / f"{500 + i}.png")
    pkl = tmp_path / "rp.pkl"; pickle.dump(items, open(pkl, "wb"))
    o1, o2 = tmp_path / "one.txt", tmp_path / "two.txt"
    base = ["--image_dir", str(img_dir), "--rp_input_file", str(pkl), "--seed", "9", "--batch-size", "8", "--num-workers", "0",
            "--synthetic-weights"]
    RP_coco.main(base + ["--saved_file_path", str(o1)])
    res = _run_ranks(2, base + ["--saved_file_path", str(o2)], tmp_path, module="tise_toolbox_amd.RP_coco")
    assert all(rc == 0 for rc, _ in res), res
    assert o1.read_text() == o2.read_text()
