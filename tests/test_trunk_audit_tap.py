"""CPU: the launch audit's check of the spatial tap (tests/_trunk_audit.py check_tap, check_assembly) on fabricated launches.

The GPU audit (tests/test_gpu_trunk_launches.py) can only show that the product's tap passes; here the check itself is shown
to fail, with a message that names the tap, for a tap one channel off, one pixel off, with a non-zero or a -0 padding column,
with an input it changed, with scalars other than the trunk's, and for a tap that reads a slice nobody wrote."""
import types

import pytest
import torch

from tests import _trunk_audit as A

TRUNK = types.SimpleNamespace(SPATIAL_C0=0, SPATIAL_NC=7, SPATIAL_LD=128, sfc=None)
N, H, W, C = 2, 3, 5, 48                  # 32-block + 16-wide tail; 3 * 5 * 7 = 105 values, 23 padding columns
SRC, ROWS = 1000, 2000                    # stand-ins for the two tensors' addresses


def _split_tensor(seed=0):
    """(N, H, W, 2C) fp16 in the split layout, built from the layout's restatement, and the fp32 values it stands for."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, C), generator=g) * 3.0
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    ih, il = A.split_index(C, "cpu")
    t = torch.zeros((N, H, W, 2 * C), dtype=torch.float16)
    t[..., ih], t[..., il] = hi, lo
    return t, hi.float() + lo.float() / 2048.0


def _rows(values, c0, nc, ld):
    out = torch.zeros((N, ld), dtype=torch.float32)
    out[:, :H * W * nc] = values[..., c0:c0 + nc].reshape(N, -1)
    return out


def _tap(t, rows, c0=0, nc=7, ld=128, after=None):
    L = A.Launch(A.TAP)
    L.inputs, L.inputs_after = [t.clone()], [(t if after is None else after).clone()]
    L.ints = {1: N, 2: H * W, 3: C, 4: c0, 5: nc, 7: ld}
    L.dsts = [(torch.full((N, ld), float("nan")), rows)]
    L.in_ptr, L.dst_ptrs = SRC, [ROWS]
    return L


def _writer(t, c0, c1):
    """A launch that writes channels [c0, c1) of the tap's source (a split max pool: own_rows reads its slice from ints)."""
    L = A.Launch("tise_maxpool3s1p1_split_nhwc")
    L.ints = {6: c1 - c0, 8: C, 9: c0}
    L.dsts = [(t.clone(), t.clone())]
    L.in_ptr, L.dst_ptrs = 1, [SRC]
    return L


def test_a_correct_tap_passes():
    t, v = _split_tensor()
    L = _tap(t, _rows(v, 0, 7, 128))
    assert A.check_launch(L, TRUNK) == ("tap", N * H * W * 7)
    assert A.check_assembly([_writer(t, 0, C), L]) == []
    assert A.check_assembly([_writer(t, 0, 32), _writer(t, 32, C), L]) == []          # two writers tile the source
    assert A.check_assembly([_writer(t, 0, 16), L, _writer(t, 16, C)]) == []          # only the tap's slice has to be there


def _fails(L, match):
    with pytest.raises(AssertionError, match=match) as e:
        A.check_launch(L, TRUNK)
    assert "tap" in str(e.value) and A.TAP in str(e.value)


def test_a_tap_one_channel_off_fails():
    t, v = _split_tensor()
    _fails(_tap(t, _rows(v, 1, 7, 128)), "values are not merge")


def test_a_tap_one_pixel_off_fails():
    t, v = _split_tensor()
    good = _rows(v, 0, 7, 128)
    shifted = torch.zeros_like(good)
    shifted[:, :98] = good[:, 7:105]                                     # every row starts at the second pixel
    _fails(_tap(t, shifted), "values are not merge")
    wc = _rows(v.transpose(1, 2), 0, 7, 128)                             # w, h, c order
    _fails(_tap(t, wc), "values are not merge")


@pytest.mark.parametrize("value", [1e-30, -0.0, float("nan")])
def test_a_padding_column_that_is_not_plus_zero_fails(value):
    t, v = _split_tensor()
    for col in (105, 127):
        rows = _rows(v, 0, 7, 128)
        rows[1, col] = value
        _fails(_tap(t, rows), "padding columns from 105 on are not \\+0")


def test_minus_zero_among_the_values_fails():
    """Bit equality, not numeric equality: a kernel that writes -0 where merge gives +0 is told apart."""
    t, v = _split_tensor()
    t[0, 0, 0, 0] = 0.0                                                  # hi of channel 0 ...
    t[0, 0, 0, 32] = 0.0                                                 # ... and its lo: the value is +0
    rows = _rows(v, 0, 7, 128)
    rows[0, 0] = -0.0
    _fails(_tap(t, rows), "values are not merge")
    rows[0, 0] = 0.0
    assert A.check_launch(_tap(t, rows), TRUNK)[0] == "tap"


def test_a_tap_that_changes_its_input_fails():
    t, v = _split_tensor()
    after = t.clone()
    after[1, 2, 4, 95] += 1
    _fails(_tap(t, _rows(v, 0, 7, 128), after=after), "changed its input")


def test_scalars_other_than_the_trunks_fail():
    t, v = _split_tensor()
    _fails(_tap(t, _rows(v, 1, 7, 128), c0=1), "the trunk states")
    _fails(_tap(t, _rows(v, 0, 6, 128), nc=6), "the trunk states")
    _fails(_tap(t, _rows(v, 0, 7, 112), ld=112), "the trunk states")


def test_a_tap_reading_a_slice_nobody_wrote_is_reported_at_the_tap():
    t, v = _split_tensor()
    L = _tap(t, _rows(v, 0, 7, 128))
    for launches, k in (([L], 0),                                        # no launch wrote its source at all
                        ([L, _writer(t, 0, C)], 0),                      # in front of the launch that fills it
                        ([_writer(t, 8, C), L], 1),                      # none of its channels written
                        ([_writer(t, 0, 6), _writer(t, 16, C), L], 2)):  # the last of its channels missing
        fails = A.check_assembly(launches)
        assert any(f.startswith(f"launch {k}: tap ") and A.TAP in f for f in fails), fails
    other = _tap(t, _rows(v, 0, 7, 128))
    other.in_ptr = SRC + 64                                              # another buffer than the one the writers filled
    fails = A.check_assembly([_writer(t, 0, C), other])
    assert any(f.startswith("launch 1: tap ") for f in fails), fails
