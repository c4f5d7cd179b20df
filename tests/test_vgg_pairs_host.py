"""CPU: the VGG-16 trunk that LPIPS and DISTS share (vgg_pairs.VGG16Pairs) -- one stand-in draw, one trunk loader."""
import pytest
import torch

from tise_toolbox_amd import dists_model, lpips_model, vgg_pairs


@pytest.mark.parametrize("seed", [0, 7])
def test_stand_in_trunks_are_bit_identical(seed):
    a, b = lpips_model.LpipsVGG16().init_synthetic(seed), dists_model.DistsVGG16().init_synthetic(seed)
    assert len(a.convs) == len(b.convs) == 13
    for ca, cb in zip(a.convs, b.convs):
        assert ca.weight.dtype == cb.weight.dtype == torch.float32
        assert ca.weight.numpy().tobytes() == cb.weight.numpy().tobytes() and ca.bias.numpy().tobytes() == cb.bias.numpy().tobytes()
    assert a.synthetic and b.synthetic


def test_both_models_are_the_shared_trunk_and_refuse_alike():
    a, b = lpips_model.LpipsVGG16(), dists_model.DistsVGG16()
    assert isinstance(a, vgg_pairs.VGG16Pairs) and isinstance(b, vgg_pairs.VGG16Pairs)
    assert type(a).load_trunk is type(b).load_trunk is vgg_pairs.VGG16Pairs.load_trunk
    alex = {"features.0.weight": torch.zeros(64, 3, 11, 11), "features.0.bias": torch.zeros(64)}
    said = []
    for m in (a, b):
        with pytest.raises(ValueError, match=r"features\.0\.weight is \(64, 3, 11, 11\), VGG-16 has \(64, 3, 3, 3\).*AlexNet") as e:
            m.load_trunk(alex)
        said.append(str(e.value))
    assert said[0] == said[1]
    for name in ("CONV_INDICES", "CONV_CHANNELS", "TAP_AFTER", "POOL_BEFORE", "MIN_SIDE"):     # the constants read through the models
        assert getattr(lpips_model, name) is getattr(dists_model, name) is getattr(vgg_pairs, name)
