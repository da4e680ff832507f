"""The fused stem kernels at the boundaries of their tiling (csrc/stem.hip): one workgroup per pooled tile walks every 32-channel
group over one staged patch; stem7 takes the horizontal half of its 3x3 max in registers (DPP rows of 16 lanes), conv columns 16
and 32 of a tile pass through a side array.  Reference, bit for bit after nan_to_num: the un-fused convolution followed by the
pooling kernel, as in tests/test_gpu_kernels.py and tests/test_gpu_conv_exact.py.

stem7 tiles are 5 x 16 pooled outputs over 11 x 33 conv outputs, the 3x3 stem's 4 x 16 over 10 x 34: the shapes below are the
smallest with one pixel, ragged last tiles in both directions, several tiles per direction and several images."""
import pytest
import torch

from rfx import ops
from rfx.ops import ConvPlan, ACT_RELU

pytestmark = pytest.mark.gpu


def _bn(g, c):
    return dict(weight=torch.rand(c, generator=g) + 0.5, bias=torch.randn(c, generator=g) * 0.3,
                running_mean=torch.randn(c, generator=g) * 0.2, running_var=torch.rand(c, generator=g) + 0.5)


def _plan7(dev, cout=64, seed=11):
    g = torch.Generator().manual_seed(seed)
    return ConvPlan(torch.randn(cout, 3, 7, 7, generator=g) * 0.1, _bn(g, cout), 2, 3, ACT_RELU, dev)


def _plan3(dev, cout=64, seed=12):
    g = torch.Generator().manual_seed(seed)
    return ConvPlan(torch.randn(cout, 3, 3, 3, generator=g) * 0.3, _bn(g, cout), 1, 1, ACT_RELU, dev)


def _x(shape, seed, dev):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _same(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _ref7(x, plan):
    return ops.maxpool2d(plan(x), 3, 2, 1)


def _ref3(x, plan):
    return ops.maxblurpool2d(plan(x), 2)


STEM7_SHAPES = [(1, 3, 1, 1), (2, 3, 37, 45), (1, 3, 43, 70), (1, 3, 130, 70), (3, 3, 16, 16)]
STEM3_SHAPES = [(1, 3, 3, 3), (1, 3, 7, 9), (2, 3, 40, 56), (1, 3, 19, 70), (2, 3, 64, 130)]


@pytest.mark.parametrize("shape", STEM7_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem7_equals_conv_then_maxpool(dev, shape):
    plan = _plan7(dev)
    x = _x(shape, 100 + shape[2], dev)
    assert _same(ops.stem_conv7_maxpool(x, plan), _ref7(x, plan))


@pytest.mark.parametrize("val", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_stem7_nan_and_inf_pixels_at_the_hand_overs(dev, val):
    """1x3x43x70 -> conv 22 x 35 -> pooled 11 x 18: input column 62 feeds conv column 31 = column 32 of the first column tile
    (side array -> pooled column 15); input row 0 feeds the first pooled row; input row 42 feeds conv row 21 = the single row of
    the ragged third row tile."""
    plan = _plan7(dev)
    base = _x((1, 3, 43, 70), 7, dev)
    for (y, xx) in ((20, 62), (0, 5), (42, 33), (0, 62), (42, 62)):
        x = base.clone()
        x[0, 1, y, xx] = val
        ref = _ref7(x, plan)
        if val == float("inf"):                             # (the kernels' ReLU, v > 0 ? v : 0, turns a NaN sum into 0)
            assert torch.isinf(ref).any()                   # the pixel does reach the pooled map
        assert _same(ops.stem_conv7_maxpool(x, plan), ref), (y, xx)


def test_stem7_all_negative_image_gives_the_identity_of_the_max(dev):
    """Positive weights, positive BN scale, negative BN shift on a negative image: every ReLU output is 0, and so is every pooled
    output -- also where a window hangs over the conv map's edge or a tile is ragged."""
    g = torch.Generator().manual_seed(5)
    bn = dict(weight=torch.ones(64), bias=-0.1 * torch.ones(64), running_mean=torch.zeros(64), running_var=torch.ones(64))
    plan = ConvPlan(torch.rand(64, 3, 7, 7, generator=g) * 0.1, bn, 2, 3, ACT_RELU, dev)
    x = (-torch.rand(2, 3, 43, 70, generator=g) - 0.01).to(dev)
    ref = _ref7(x, plan)
    assert float(ref.abs().max()) == 0.0
    assert torch.equal(ops.stem_conv7_maxpool(x, plan), ref)


@pytest.mark.parametrize("cout", [32, 64, 96, 128])
def test_stem7_every_group_count(dev, cout):
    plan = _plan7(dev, cout, seed=20 + cout)
    x = _x((2, 3, 70, 58), cout, dev)
    assert _same(ops.stem_conv7_maxpool(x, plan), _ref7(x, plan))


def test_stem7_grouped_launch_equals_single_launches(dev):
    plan = _plan7(dev, 96, seed=31)
    xs = [_x(s, 40 + i, dev) for i, s in enumerate([(1, 3, 43, 70), (2, 3, 16, 16), (1, 3, 130, 37)])]
    single = [ops.stem_conv7_maxpool(x, plan) for x in xs]
    with ops.launch_group(dev, False):
        grouped = [ops.stem_conv7_maxpool(x, plan) for x in xs]
    torch.cuda.synchronize()
    for x, a, b in zip(xs, grouped, single):
        assert torch.equal(a, b) and _same(a, _ref7(x, plan))


@pytest.mark.parametrize("shape", STEM3_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem3_equals_conv_then_maxblurpool(dev, shape):
    plan = _plan3(dev)
    x = _x(shape, 200 + shape[3], dev)
    assert _same(ops.stem_conv_maxblur(x, plan), _ref3(x, plan))


@pytest.mark.parametrize("cout", [32, 96])
def test_stem3_other_group_counts(dev, cout):
    plan = _plan3(dev, cout, seed=60 + cout)
    x = _x((2, 3, 19, 70), cout, dev)
    assert _same(ops.stem_conv_maxblur(x, plan), _ref3(x, plan))


@pytest.mark.parametrize("val", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_stem3_nan_and_inf_pixels_on_the_reflected_border_and_inside(dev, val):
    plan = _plan3(dev)
    base = _x((1, 3, 19, 70), 9, dev)
    for (y, xx) in ((0, 0), (18, 69), (0, 33), (9, 30), (10, 31)):
        x = base.clone()
        x[0, 2, y, xx] = val
        assert _same(ops.stem_conv_maxblur(x, plan), _ref3(x, plan)), (y, xx)


def test_both_stems_twice_on_one_input_give_the_same_bits(dev):
    """Nothing stale in LDS carries from one channel group, or one launch, to the next: a different input in between, then the
    first input again."""
    p7, p3 = _plan7(dev, 96, seed=71), _plan3(dev, 96, seed=72)
    x, other = _x((2, 3, 43, 70), 1, dev), _x((2, 3, 43, 70), 2, dev) * 50.0
    a7, a3 = ops.stem_conv7_maxpool(x, p7), ops.stem_conv_maxblur(x, p3)
    ops.stem_conv7_maxpool(other, p7), ops.stem_conv_maxblur(other, p3)
    b7, b3 = ops.stem_conv7_maxpool(x, p7), ops.stem_conv_maxblur(x, p3)
    assert torch.equal(a7.view(torch.int32), b7.view(torch.int32)) and torch.equal(a3.view(torch.int32), b3.view(torch.int32))
    assert _same(a7, _ref7(x, p7)) and _same(a3, _ref3(x, p3))
