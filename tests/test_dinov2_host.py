"""CPU: the DINOv2 module of FD-DINOv2 (tise_toolbox_amd/dinov2_model.py) and the parts of its CLI that need no GPU: the official
state-dict key names, the refused checkpoints, the position-table rule, the preprocessing, the argument refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _official_keys(layers):
    keys = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight", "norm.bias"]
    for i in range(layers):
        for part in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                     "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                     "mlp.fc2.bias", "ls2.gamma"):
            keys.append(f"blocks.{i}.{part}")
    return sorted(keys)


@pytest.mark.parametrize("arch,width,heads", [("vits14", 384, 6), ("vitb14", 768, 12), ("vitl14", 1024, 16)])
def test_state_dict_round_trip_under_the_official_names(tmp_path, arch, width, heads):
    """Each architecture at 2 layers: the keys are the official ones, a file with them (and a mask_token) loads strictly
    through build_dinov2, the configuration is read off the shapes, and the loaded module computes what the saved one did."""
    from tise_toolbox_amd import dinov2_model as dm
    cfg = dict(dm.CONFIGS[arch], layers=2)
    assert (cfg["width"], cfg["heads"], cfg["patch"], cfg["width"] // cfg["heads"]) == (width, heads, 14, 64)
    assert dm.CONFIGS[arch]["layers"] == (24 if arch == "vitl14" else 12) and dm.DEFAULT_ARCH == "vitl14"
    model = dm.seeded_init_(dm.DinoVisionTransformer(cfg), 3).finalize().eval()
    sd = model.state_dict()
    assert sorted(sd) == _official_keys(2)
    assert sd["pos_embed"].shape == (1, 1 + 37 * 37, width) and sd["cls_token"].shape == (1, 1, width)
    assert sd["patch_embed.proj.weight"].shape == (width, 3, 14, 14) and sd["blocks.0.mlp.fc1.weight"].shape == (4 * width, width)
    assert dm.config_from_state_dict(sd) == cfg
    path = str(tmp_path / "w.pth")
    torch.save(dict(sd, mask_token=torch.zeros(1, width)), path)
    again = dm.build_dinov2(path, arch=cfg)
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        a, b = model(x), again(x)
    assert a.shape == (1, width) and torch.equal(a, b)
    with pytest.raises(RuntimeError, match="parameters of"):
        dm.build_dinov2(path, arch=dict(cfg, layers=3))
    bad = dict(sd)
    del bad["blocks.1.ls2.gamma"]
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match="ls2.gamma"):
        dm.build_dinov2(path, arch=cfg)


def test_seeded_init_leaves_nothing_at_its_default():
    from tise_toolbox_amd import dinov2_model as dm
    m = dm.seeded_init_(dm.DinoVisionTransformer(dict(width=128, layers=1, heads=2, patch=14, resolution=84)), 0)
    for name, p in m.named_parameters():
        assert p.std() > 0, name                                           # no untouched table, no constant vector
        if name.endswith("bias"):
            assert (p != 0).all(), name
        if name.endswith("gamma"):
            assert 0.5 <= p.min() and p.max() <= 1.5 and p.std() > 0.1
        elif "norm" not in name:
            assert p.abs().max() <= 0.04 + 1e-6, name                      # truncated at two standard deviations of 0.02
    assert dm.get_config(None) is dm.CONFIGS["vitl14"]
    with pytest.raises(ValueError, match="unknown DINOv2 tower"):
        dm.get_config("vitg14")


def test_register_and_giant_checkpoints_are_refused_with_the_reason():
    from tise_toolbox_amd import dinov2_model as dm
    sd = dm.DinoVisionTransformer(dict(width=128, layers=1, heads=2, patch=14, resolution=224)).state_dict()
    with pytest.raises(RuntimeError, match="REGISTERS"):
        dm.config_from_state_dict(dict(sd, register_tokens=torch.zeros(1, 4, 128)))
    giant = {k: v for k, v in sd.items() if ".mlp." not in k}
    giant["blocks.0.mlp.w12.weight"] = torch.zeros(8, 128)
    giant["blocks.0.mlp.w3.weight"] = torch.zeros(128, 4)
    with pytest.raises(RuntimeError, match="SwiGLU"):
        dm.config_from_state_dict(giant)
    with pytest.raises(RuntimeError, match="not a DINOv2 state_dict"):
        dm.config_from_state_dict({"visual.conv1.weight": torch.zeros(1)})


@pytest.mark.parametrize("g", [16, 11])
def test_position_table_rule_equals_a_direct_interpolate(g):
    from tise_toolbox_amd import dinov2_model as dm
    d = 24
    table = torch.randn(1 + 37 * 37, d, generator=torch.Generator().manual_seed(g))
    got = dm.interpolate_pos_table(table, g)
    want = F.interpolate(table[1:].reshape(1, 37, 37, d).permute(0, 3, 1, 2), scale_factor=((g + 0.1) / 37, (g + 0.1) / 37),
                         mode="bicubic", antialias=False)
    assert want.shape == (1, d, g, g)
    assert got.shape == (1 + g * g, d) and got.dtype == torch.float32
    assert torch.equal(got[0], table[0])
    assert torch.equal(got[1:], want.permute(0, 2, 3, 1).reshape(g * g, d))
    assert torch.equal(got[1 + g + 2], want[0, :, 1, 2])                   # row-major over the grid: (y, x) -> 1 + y g + x


def test_position_table_is_unchanged_at_its_own_grid():
    from tise_toolbox_amd import dinov2_model as dm
    table = torch.randn(1 + 37 * 37, 8, generator=torch.Generator().manual_seed(0))
    assert dm.interpolate_pos_table(table, 37) is table
    with pytest.raises(RuntimeError, match="square grid"):
        dm.interpolate_pos_table(table[:-1], 16)
    m = dm.DinoVisionTransformer(dict(width=64, layers=1, heads=1, patch=14, resolution=518))
    dm.seeded_init_(m, 0).finalize()
    assert torch.equal(m.pos, m.pos_embed[0])


@pytest.mark.parametrize("w,h", [(256, 256), (640, 480), (37, 91)])
def test_preprocess_equals_pillow_and_numpy(w, h):
    from PIL import Image
    from tise_toolbox_amd import dinov2_model as dm
    rng = np.random.default_rng(w * 1000 + h)
    img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    got = dm.preprocess(img)
    a = np.asarray(img.convert("RGB").resize((224, 224), Image.BICUBIC), dtype=np.float32) / np.float32(255.0)
    want = (a - np.array((0.485, 0.456, 0.406), np.float32)) / np.array((0.229, 0.224, 0.225), np.float32)
    assert got.shape == (3, 224, 224) and got.dtype == torch.float32
    assert np.array_equal(got.numpy(), want.transpose(2, 0, 1))
    grey = dm.preprocess(img.convert("L"))                                 # converted to RGB first
    assert grey.shape == (3, 224, 224)
    lut = dm.preprocess_lut()
    u8 = np.asarray(img.convert("RGB").resize((224, 224), Image.BICUBIC))
    assert np.array_equal(got.numpy(), np.stack([lut[c][u8[:, :, c]] for c in range(3)]))


def test_preprocess_lut_bit_for_bit():
    from tise_toolbox_amd import dinov2_model as dm
    lut = dm.preprocess_lut()
    assert lut.shape == (3, 256) and lut.dtype == np.float32 and lut.flags["C_CONTIGUOUS"]
    for c, (m, s) in enumerate(zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        for v in range(256):
            want = (np.float32(v) / np.float32(255.0) - np.float32(m)) / np.float32(s)
            assert lut[c, v].tobytes() == np.float32(want).tobytes(), (c, v)


def test_cli_refusals_that_need_no_gpu(tmp_path):
    from tise_toolbox_amd import dinov2_model as dm, fd_dinov2, fid_score, weights
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir(), d2.mkdir()
    with pytest.raises(SystemExit):
        fd_dinov2.parse_args(["--path1", str(d1), "--path2", str(d2), "--arch", "vitg14"])
    with pytest.raises(SystemExit):
        fd_dinov2.parse_args(["--path1", str(d1), "--path2", str(d2), "--weights", "w.pth", "--synthetic-weights"])
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        weights.resolve("w.pth", True, "dinov2-vitl14")
    args = fd_dinov2.parse_args(["--path1", str(d1), "--path2", str(d2)])
    assert (args.arch, args.batch_size, args.prdc_k, args.kd, args.prdc, args.png_feed) == ("vitl14", 50, 5, False, False, "ring")
    # a feature file of another network, and of another architecture
    other = str(tmp_path / "clip.npz")
    fid_score.save_stats_npz(other, np.zeros(1024), np.eye(1024), "clip-vit-l14-336", np.zeros((3, 1024), np.float32))
    with pytest.raises(RuntimeError, match="clip-vit-l14-336"):
        fd_dinov2.main(["--path1", other, "--path2", str(d2), "--synthetic-weights"])
    small = str(tmp_path / "s.npz")
    fid_score.save_stats_npz(small, np.zeros(384), np.eye(384), "dinov2-vits14", np.zeros((3, 384), np.float32))
    with pytest.raises(RuntimeError, match="dinov2-vits14"):
        fd_dinov2.main(["--path1", str(d1), "--path2", small, "--synthetic-weights", "--arch", "vitb14"])
    assert fd_dinov2.load_features_npz(small, "vits14")[0].shape == (3, 384)
    with pytest.raises(RuntimeError, match="no network tag"):
        np.savez(str(tmp_path / "plain.npz"), mu=np.zeros(4), sigma=np.eye(4))
        fd_dinov2.check_feature_file(str(tmp_path / "plain.npz"), "vitl14")
    # tags, widths and default parameter files
    for arch, dims in (("vits14", 384), ("vitb14", 768), ("vitl14", 1024)):
        assert fd_dinov2.arch_info(arch) == (dims, "dinov2-" + arch, "dinov2-" + arch)
        assert weights._KINDS["dinov2-" + arch][1]()[0].endswith(f"hub/checkpoints/dinov2_{arch}_pretrain.pth")
    assert dm.RESOLUTION == 224


# ---------------------------------------------------------------------------------------------------------------------
def _evaluate(model, x, mode):
    """The module's forward on the CPU: "a" as it is (fp32); "b" with every Linear's (and the patch convolution's) operands and
    output rounded to fp16, and the attention's and the GELU's outputs, which is what torch.autocast(fp16) rounds -- LayerNorm,
    LayerScale and the residual stream stay fp32; "c" = "b" with the stream also rounded to fp16 after each residual add, which
    is clip_hip.HipTowers' arithmetic.  -> (features, the stream after the last block)."""
    r = (lambda t: t.half().float()) if mode != "a" else (lambda t: t)
    s = (lambda t: t.half().float()) if mode == "c" else (lambda t: t)
    lin = lambda t, l: r(F.linear(r(t), r(l.weight), r(l.bias)))
    pe = model.patch_embed.proj
    t = r(F.conv2d(r(x), r(pe.weight), r(pe.bias), stride=model.patch)).flatten(2).transpose(1, 2)
    t = torch.cat([model.cls_token.expand(t.shape[0], -1, -1), t], 1) + model.pos
    for blk in model.blocks:
        y = F.layer_norm(t, t.shape[-1:], blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
        b, n, w = y.shape
        q, k, v = lin(y, blk.attn.qkv).view(b, n, 3, blk.attn.heads, w // blk.attn.heads).permute(2, 0, 3, 1, 4)
        o = r(F.scaled_dot_product_attention(q, k, v)).transpose(1, 2).reshape(b, n, w)
        t = s(t + blk.ls1.gamma * lin(o, blk.attn.proj))
        y = F.layer_norm(t, t.shape[-1:], blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
        t = s(t + blk.ls2.gamma * lin(r(F.gelu(lin(y, blk.mlp.fc1))), blk.mlp.fc2))
    return F.layer_norm(t, t.shape[-1:], model.norm.weight, model.norm.bias, model.norm.eps)[:, 0], t


def _one_minus_cos(a, b):
    a, b = a.double(), b.double()
    return (1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max().item()


def test_an_fp16_stream_misses_the_end_to_end_condition_on_outliers():
    """The condition of tests/test_gpu_dinov2.py has teeth on the inputs the fp32 stream exists for.  The tiny 154-pixel tower with
    tests/_tower_audit.make_outliers_ (+-3000 on channels 5 and 77 of two patch tokens' position rows, +-50 on the class row's,
    block 0's fc2 rows of those channels x 40) on the 3 seeded images of tests/test_gpu_tower_launches.py, three CPU evaluations
    (_evaluate): (a) the fp32 module, (b) fp16-rounded Linear operands and outputs = what autocast rounds, (c) = (b) with the
    stream rounded to fp16 after each residual add.  Asserted: 1 - cos(c, a) >= 10 x (1 - cos(b, a)), worst image.

    Measured (worst of 3 images): 1 - cos(b, a) = 3.033e-10, 1 - cos(c, a) = 6.949e-08, ratio 229; evaluation "a" equals the
    module's own forward to 2e-16.  The same tower WITHOUT outliers: 1.405e-07 and 2.500e-07, ratio 1.8 -- two layers of O(1)
    activations do not tell the two streams apart, which is why the suite never did.

    How the magnitudes were chosen (on the CPU, from the references alone): everything that passes a LayerNorm is rounded to
    fp16 as a Linear operand in (b) as well, so in a 2-layer tower an fp16 stream can only lose what reaches the features
    directly: the class row.  With 3000 on the class row too the two channels are all the final LayerNorm sees of it (every
    other feature is ~1e-3 of them) and (b) drops to 1e-14, the rounding noise of fp32 features, where no condition can be
    tested (ratio 2e6); with no outlier on the class row the ratio is 3.4 (3.1e-07 / 1.05e-06).  At +-50 the class row's outlier
    channels are 8 sigma of its LayerNorm and an fp16 ulp of them (2^-5) is 1e2 x the fp16 rounding of an O(0.1) update.
    The construction itself is asserted: the fp32 stream reaches 1e3 with its median below 10."""
    from tests import _tower_audit as A
    from tise_toolbox_amd import dinov2_model as dm
    model = A.make_outliers_(dm.build_dinov2(None, 0, A.TINY154))
    x = A.seeded_images(3, 154, 5, "cpu").half().float()
    with torch.no_grad():
        fa, stream = _evaluate(model, x, "a")
        fb, fc = _evaluate(model, x, "b")[0], _evaluate(model, x, "c")[0]
        assert _one_minus_cos(model(x), fa) < 1e-12                        # _evaluate restates the module
    assert stream.abs().max() >= 1e3 and stream.abs().median() < 10
    eb, ec = _one_minus_cos(fb, fa), _one_minus_cos(fc, fa)
    print(f"1 - cos against the fp32 module: autocast restatement {eb:.3e}, fp16 stream {ec:.3e}, ratio {ec / eb:.1f}")
    assert torch.isfinite(fc).all() and eb > 1e-11                         # well above the noise of fp32 features (1e-14)
    assert ec >= 10 * eb, (ec, eb)
