"""rfx_conv1x1_expand64_f32 / rfx_conv1x1_expand64_dual_f32 (csrc/conv1x1e.hip): the 64 -> 256 expansions of the trunk's layer1 as a
kernel of their own, held to the launches they replace BIT FOR BIT.

Every case is checked both ways:
  * random float32 data against today's launches (rfx_conv2d_f32: the shortcut, then conv3 with it as the residual) -- the path
    RFX_EXPAND64=0 restores;
  * the exact-operand families of tests/test_gpu_conv_exact.py (dense, apieces, wpieces) against float64.
The kernel is called through ops.conv1x1_expand64 with the measured launch-size rule (ops.EXPAND64_MIN_PIXELS) set to zero: the
tests hold the kernel itself at every size, whichever sizes the product routes to it."""
import ctypes

import pytest
import torch

from rfx import ops, nets, weights, _lib
from test_gpu_conv_exact import operands, epilogue, exact_reference, _mismatch

pytestmark = pytest.mark.gpu

NONE, RELU = ops.ACT_NONE, ops.ACT_RELU
FAMILIES = ("dense", "apieces", "wpieces")


@pytest.fixture(autouse=True)
def every_size_on_the_new_kernel(monkeypatch):
    monkeypatch.setattr(ops, "_EXPAND64", True)
    monkeypatch.setattr(ops, "EXPAND64_MIN_PIXELS", {"plain": 0, "dual": 0})


def _bn(g, C):
    return dict(weight=torch.rand(C, generator=g) + 0.5, bias=torch.randn(C, generator=g) * 0.1,
                running_mean=torch.randn(C, generator=g) * 0.1, running_var=torch.rand(C, generator=g) + 0.5)


def _plans(g, dev, Cin=64, Cout=256, stride=1):
    c3 = ops.ConvPlan(torch.randn(Cout, Cin, 1, 1, generator=g) * 0.1, _bn(g, Cout), stride, 0, RELU, dev)
    ds = ops.ConvPlan(torch.randn(Cout, Cin, 1, 1, generator=g) * 0.1, _bn(g, Cout), stride, 0, NONE, dev)
    return c3, ds


def _old(c3, o, residual=None, shortcut=None):
    """Today's launches."""
    if shortcut is not None:
        residual = shortcut[1](shortcut[0])
    return c3(o, residual=residual)


def _grid_waves(dev):
    """Wavefront slots of the persistent launch (include/rfx_api.h): one workgroup of 8 wavefronts per CU."""
    return 8 * torch.cuda.get_device_properties(dev).multi_processor_count


def _second_tile_shape(dev):
    """(N, H, W), N = 2 and W odd, whose 32-pixel tiles exceed the launch's wavefront slots by 1 to 3: a wavefront walks a second
    tile (at 256 CUs: 2048 slots, 2 x 271 x 121 = 65582 pixels, 2050 tiles, 67 MB out)."""
    slots = _grid_waves(dev)
    for W in range(127, 32, -2):
        H = (slots * 16) // W + 1                         # the first H with 2 H W > 32 slots
        if 1 <= (2 * H * W + 31) // 32 - slots <= 3:
            return 2, H, W
    raise AssertionError("no shape for %d wavefront slots" % slots)


def _random_check(dev, N, H, W, seed, forms=("plain", "plain_nores", "dual")):
    g = torch.Generator().manual_seed(seed)
    c3, ds = _plans(g, dev)
    o = torch.randn(N, 64, H, W, generator=g).to(dev)
    x = torch.randn(N, 64, H, W, generator=g).to(dev)
    r = torch.randn(N, 256, H, W, generator=g).to(dev)
    for form in forms:
        kw = {"plain": dict(residual=r), "plain_nores": dict(), "dual": dict(shortcut=(x, ds))}[form]
        want = _old(c3, o, **kw)
        with ops.Profiler() as prof:
            got = ops.conv1x1_expand64(o, c3, **kw)
        assert torch.equal(got, want), (form, (N, H, W), _mismatch(got, want))
        # recorded under the id today's conv3 launch has, with both GEMMs' FLOPs
        (kid, flops, _, _, shape, nbytes), = prof.conv
        assert kid == _lib.load().rfx_conv2d_kernel_id(N, 64, 256, 1, 1, 1, 0, H, W)
        assert flops == (2 if form == "dual" else 1) * 2.0 * N * H * W * 256 * 64 and shape == (N, 64, H, W, 256, 1, 1)
        planes = {"plain": 64 + 512, "plain_nores": 64 + 256, "dual": 128 + 256}[form]
        assert nbytes == 4.0 * (N * H * W * planes + (2 if form == "dual" else 1) * 256 * 64)


def _exact_check(dev, N, H, W, seed, fams=FAMILIES):
    g = torch.Generator().manual_seed(seed)
    for fam in fams:
        # one nonzero product per output in the sparse families: main sum + shortcut + shifts stay below 2^24 quanta
        o, w3, qx, qw = operands(fam, g, N, 64, 256, H, W, 1, 1, T=1)
        x, wd, _, _ = operands(fam, g, N, 64, 256, H, W, 1, 1, T=1)
        s3, b3, Q3 = epilogue(fam, g, 256, qx, qw)
        sd, bd, Qd = epilogue(fam, g, 256, qx, qw)
        Q = min(Q3, Qd)
        span = 2048 if fam == "dense" else 1 << 17
        res = torch.randint(-span, span + 1, (N, 256, H, W), generator=g).float() * Q
        c3 = ops.ConvPlan(w3, None, 1, 0, RELU, dev)
        ds = ops.ConvPlan(wd, None, 1, 0, NONE, dev)
        c3.scale, c3.shift, ds.scale, ds.shift = s3.to(dev), b3.to(dev), sd.to(dev), bd.to(dev)
        od, xd = o.to(dev), x.to(dev)
        ref = exact_reference(o, w3, s3, b3, res, RELU, Q, qx, qw, 1, 0, dev=dev, fam=fam)
        got = ops.conv1x1_expand64(od, c3, residual=res.to(dev))
        assert torch.equal(got, ref), (fam, "plain", _mismatch(got, ref))
        ref = exact_reference(o, w3, s3, b3, None, RELU, Q, qx, qw, 1, 0, dev=dev, fam=fam)
        got = ops.conv1x1_expand64(od, c3)
        assert torch.equal(got, ref), (fam, "plain, no residual", _mismatch(got, ref))
        d = exact_reference(x, wd, sd, bd, None, NONE, Q, qx, qw, 1, 0, dev=dev, fam=fam)
        ref = exact_reference(o, w3, s3, b3, d.cpu(), RELU, Q, qx, qw, 1, 0, dev=dev, fam=fam)
        got = ops.conv1x1_expand64(od, c3, shortcut=(xd, ds))
        assert torch.equal(got, ref), (fam, "dual", _mismatch(got, ref))


def test_three_tiles_last_ragged_one_across_two_images(dev):
    """Cases 1 and 2: N = 2, 64 -> 256, 9 x 17 maps -- 306 pixels, ten 32-pixel wavefront tiles (three 128-pixel spans), the last
    ragged, tile 4 (pixels 128..159) straddling the two images; residual + ReLU, no residual, and the two-source form against
    the shortcut launch followed by the conv3 launch."""
    _random_check(dev, 2, 9, 17, 1)
    _exact_check(dev, 2, 9, 17, 2)


def test_less_than_one_tile(dev):
    """Case 3: N = 1, 3 x 5 -- 15 pixels, one ragged tile, one workgroup with seven idle wavefronts."""
    _random_check(dev, 1, 3, 5, 3)
    _exact_check(dev, 1, 3, 5, 4)


def test_a_wavefront_walks_a_second_tile(dev):
    """Case 4: the 32-pixel tiles exceed the persistent launch's wavefront slots (8 per CU) by 1 to 3, so the first wavefronts of
    the first workgroup walk on to a second tile with their resident weights: both forms, random data against today's
    launches and the dense exact family against float64."""
    N, H, W = _second_tile_shape(dev)
    tiles, slots = (N * H * W + 31) // 32, _grid_waves(dev)
    assert 1 <= tiles - slots <= 3, (N, H, W, tiles, slots)
    _random_check(dev, N, H, W, 5, forms=("plain", "dual"))
    _exact_check(dev, N, H, W, 6, fams=("dense",))


@pytest.mark.parametrize("Cin,Cout,stride,rc", [(128, 256, 1, -1), (64, 192, 1, -1), (64, 256, 2, -1), (64, 512, 1, -2)])
def test_ineligible_geometries(dev, Cin, Cout, stride, rc):
    """Case 5: the entry points refuse what the kernel does not serve (RFX_E_ARG; RFX_E_LIMIT past the resident weights) without
    launching, and the op runs such a layer on today's kernel, bit-equal."""
    g = torch.Generator().manual_seed(7)
    c3, ds = _plans(g, dev, Cin, Cout, stride)
    N, H, W = 2, 9, 17
    o = torch.randn(N, Cin, H, W, generator=g).to(dev)
    Ho, Wo = c3.out_hw(H, W)
    out = torch.full((N, Cout, Ho, Wo), 7.0, device=dev)
    lib, st, p = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ops._p
    assert lib.rfx_conv1x1_expand64_f32(p(o), p(c3.wT), p(c3.scale), p(c3.shift), None, p(out), N, Cin, H * W, Cout, stride, RELU, st) == rc
    assert lib.rfx_conv1x1_expand64_dual_f32(p(o), p(c3.wT), p(c3.scale), p(c3.shift), p(o), p(ds.wT), p(ds.scale), p(ds.shift), p(out),
                                             N, Cin, H * W, Cout, stride, st) == rc
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert not ops.expand64_eligible(c3) and ops.expand64_form(c3) is None and ops.expand64_form(c3, ds) is None
    r = torch.randn(N, Cout, Ho, Wo, generator=g).to(dev)
    assert torch.equal(ops.conv1x1_expand64(o, c3, residual=r), c3(o, residual=r))
    assert torch.equal(ops.conv1x1_expand64(o, c3, shortcut=(o, ds)), c3(o, residual=ds(o)))


def test_entry_points_refuse_other_activations_and_recording_groups(dev):
    g = torch.Generator().manual_seed(8)
    c3, ds = _plans(g, dev)
    o = torch.randn(1, 64, 3, 5, generator=g).to(dev)
    out = torch.empty(1, 256, 3, 5, device=dev)
    lib, st, p = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ops._p
    args = (p(o), p(c3.wT), p(c3.scale), p(c3.shift), None, p(out), 1, 64, 15, 256, 1)
    assert lib.rfx_conv1x1_expand64_f32(*args, ops.ACT_SIGMOID, st) == -1
    with ops.launch_group(dev, False):
        assert lib.rfx_conv1x1_expand64_f32(*args, RELU, st) == -1
        y = ops.conv1x1_expand64(o, c3)                          # the op records today's launch instead
    assert lib.rfx_conv1x1_expand64_f32(*args, RELU, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, c3(o)) and torch.equal(y, out)


def test_whole_trunk_switch_on_and_off(dev, monkeypatch):
    """Case 6: ResNet50Trunk on (2, 3, 64, 96) and forward_group on two inputs of different sizes: RFX_EXPAND64 on and off return
    the same bits, and with it on the three layer1 blocks really take the new launches."""
    monkeypatch.setenv("RFX_CONV_SPLIT", "1")
    trunk = nets.ResNet50Trunk(weights.resnet50_trunk_sd(0), dev)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 64, 96, generator=g).to(dev)
    xs = [torch.randn(1, 3, 64, 96, generator=g).to(dev), torch.randn(1, 3, 48, 80, generator=g).to(dev)]
    assert [trunk.expand64_form(b) for b in trunk.blocks[:4]] == ["dual", "plain", "plain", None]
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        on, on_g = trunk(x), trunk.forward_group(xs)
        n_new = [calls.count("rfx_conv1x1_expand64_dual_f32"), calls.count("rfx_conv1x1_expand64_f32")]
        monkeypatch.setattr(ops, "_EXPAND64", False)
        del calls[:]
        off, off_g = trunk(x), trunk.forward_group(xs)
    assert n_new == [1, 2] and not [c for c in calls if "expand64" in c]
    assert torch.equal(on, off)
    for a, b, xi in zip(on_g, off_g, xs):
        assert torch.equal(a, b) and torch.equal(a, trunk(xi))
