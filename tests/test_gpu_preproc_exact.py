"""csrc/preproc.hip held to exact references: the Lanczos passes to Pillow byte for byte (through every channel instance, a row
window, the grid-stride trips and the entry point's refusals), ToTensor + Normalize to the IEEE float32 operations bit for bit.
tests/test_lanczos_cpu.py pins the host tables to Pillow without a device, so a failure here is the kernel's."""
import numpy as np
import pytest
import torch

import lanczos_cases as L
from rfx import _lib, lanczos, ops
from rfx.pipeline import IMAGENET_MEAN, IMAGENET_STD

pytestmark = pytest.mark.gpu
CAP = 8192 * 256                     # outputs of one trip of the capped grid (grid_for in preproc.hip)
DEV_FAMILIES = ("noise", "binary", "checker")


@pytest.mark.parametrize("size", L.SMALL, ids=lambda s: "%dx%d-%dx%d" % s)
def test_lanczos_resize_equals_pillow_for_one_to_four_channels(dev, size):
    """ops.lanczos_resize_u8 takes (N,H,W,C) with C in 1..4: C = 3 is the unrolled instance, 1, 2 and 4 the runtime-channel one.
    Three different images per call.  tests/test_lanczos_cpu.py checks that these inputs reach both ends of the uint8 clamp."""
    w, h, ow, oh = size
    for fam in DEV_FAMILIES:
        for c in (1, 2, 3, 4):
            imgs = np.stack([L.image(fam, h, w, c, seed=10 * k + c) if fam != "checker" else np.roll(L.image(fam, h, w, c), k, axis=1)
                             for k in range(3)])
            ref = np.stack([L.pillow(im, ow, oh) for im in imgs])
            got = ops.lanczos_resize_u8(torch.from_numpy(imgs).to(dev), ow, oh)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (3, oh, ow, c)
            assert np.array_equal(got.cpu().numpy(), ref), (size, fam, c)


def test_unchanged_size_is_a_copy_in_other_storage(dev):
    img = torch.from_numpy(np.stack([L.image("noise", 19, 21, 3, seed=k) for k in range(2)])).to(dev)
    out = ops.lanczos_resize_u8(img, 21, 19)
    assert torch.equal(out, img) and out.data_ptr() != img.data_ptr()


def _pass(dev, src, out, outH, outW, bounds, kk, ksize, vertical, row_offset, C=None):
    N, inH, inW, Cs = src.shape
    ops._call("rfx_lanczos_pass_u8", src.device, ops._p(src), ops._p(out), N, inH, inW, outH, outW, Cs if C is None else C,
              ops._p(bounds), ops._p(kk), ksize, vertical, row_offset)


@pytest.mark.parametrize("C", [3, 2])
def test_horizontal_pass_over_a_row_window(dev, C):
    """row_offset > 0 is not reachable through ops.lanczos_resize_u8 (tests/test_lanczos_cpu.py: the plan of a full-image box
    always starts at row 0): the entry point directly.  Rows [5, 16) of a 29-row image."""
    inH, inW, outW, off, rows = 29, 23, 40, 5, 11
    imgs = np.stack([L.image("binary", inH, inW, C, seed=k) for k in range(2)])
    full = np.stack([L.pillow(im, outW, inH) for im in imgs])                         # horizontal pass only
    bounds, kk, ksize = lanczos.coeffs(inW, outW)
    src = torch.from_numpy(imgs).to(dev)
    b, k = torch.from_numpy(bounds).to(dev), torch.from_numpy(kk).to(dev)
    out_full = torch.full((2, inH, outW, C), 0xA5, dtype=torch.uint8, device=dev)
    _pass(dev, src, out_full, inH, outW, b, k, ksize, 0, 0)
    assert np.array_equal(out_full.cpu().numpy(), full)
    out = torch.full((2, rows + 1, outW, C), 0xA5, dtype=torch.uint8, device=dev)      # one sentinel row per image behind ...
    for n in range(2):                                                                 # (the window's rows are packed per call)
        _pass(dev, src[n:n + 1], out[n:n + 1, :rows], rows, outW, b, k, ksize, 0, off)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :rows], full[:, off:off + rows]) and (got[:, rows] == 0xA5).all()
    both = torch.empty((2, rows, outW, C), dtype=torch.uint8, device=dev)              # N = 2 in one call: the batch stride is inH
    _pass(dev, src, both, rows, outW, b, k, ksize, 0, off)
    assert np.array_equal(both.cpu().numpy(), full[:, off:off + rows])
    last = torch.empty((2, rows, outW, C), dtype=torch.uint8, device=dev)              # the last admissible window
    _pass(dev, src, last, rows, outW, b, k, ksize, 0, inH - rows)
    assert np.array_equal(last.cpu().numpy(), full[:, inH - rows:])


@pytest.mark.parametrize("size,C", [((40, 30, 1500, 1400), 3), ((30, 1400, 1500, 1400), 2), ((1500, 30, 1500, 1400), 1)])
def test_lanczos_passes_beyond_the_launch_cap(dev, size, C):
    """More than 8192 x 256 outputs: the vertical pass of a two-pass upscale (its horizontal pass stays below the cap), a
    horizontal-only and a vertical-only pass, over both kernel instances."""
    w, h, ow, oh = size
    assert ow * oh > CAP
    img = L.image("noise", h, w, C, seed=5)
    got = ops.lanczos_resize_u8(torch.from_numpy(img[None]).to(dev), ow, oh)
    assert np.array_equal(got[0].cpu().numpy(), L.pillow(img, ow, oh))


def test_lanczos_pass_refusals_leave_the_output_alone(dev):
    inH, inW, outW, outH = 9, 17, 40, 20
    bh, kh, ksh = lanczos.coeffs(inW, outW)
    bv, kv, ksv = lanczos.coeffs(inH, outH)
    t = lambda a: torch.from_numpy(a).to(dev)
    bh, kh, bv, kv = t(bh), t(kh), t(bv), t(kv)
    src = torch.zeros((1, inH, inW, 5), dtype=torch.uint8, device=dev)
    out = torch.full((1, 64, 64, 5), 0xA5, dtype=torch.uint8, device=dev)
    bad = [
        dict(outH=inH, outW=outW, bounds=bh, kk=kh, ksize=ksh, vertical=0, row_offset=0, C=5),          # C = 5
        dict(outH=outH, outW=inW + 1, bounds=bv, kk=kv, ksize=ksv, vertical=1, row_offset=0, C=3),      # vertical, outW != inW
        dict(outH=inH - 1, outW=outW, bounds=bh, kk=kh, ksize=ksh, vertical=0, row_offset=2, C=3),      # outH + row_offset > inH
        dict(outH=inH, outW=outW, bounds=bh, kk=kh, ksize=0, vertical=0, row_offset=0, C=3),            # ksize = 0
    ]
    for kw in bad:
        with pytest.raises(_lib.RfxError, match="bad argument"):
            _pass(dev, src, out, **kw)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    with pytest.raises(_lib.RfxError, match="bad argument"):
        ops.lanczos_resize_u8(src, outW, outH)                                                          # the wrapper: C = 5
    # the same calls with the one argument put right go through
    _pass(dev, src, out, inH, outW, bh, kh, ksh, 0, 0, C=3)
    _pass(dev, src, out, inH - 2, outW, bh, kh, ksh, 0, 2, C=3)


def _ramps(N, H, W):
    """uint8 (N,H,W,3): three distinct ramps, each taking every byte value within any 256 consecutive pixels."""
    p = np.arange(N * H * W, dtype=np.int64).reshape(N, H, W)
    return np.stack((p % 256, (255 - p) % 256, (3 * p + 7) % 256), axis=3).astype(np.uint8)


def _to_tensor_reference(img):
    """ToTensor + Normalize as IEEE float32 operations: x / 255, then (. - mean) / std."""
    x = np.ascontiguousarray(img.transpose(0, 3, 1, 2)).astype(np.float32)
    raw = x / np.float32(255)
    mean = np.asarray(IMAGENET_MEAN, dtype=np.float32).reshape(1, 3, 1, 1)
    std = np.asarray(IMAGENET_STD, dtype=np.float32).reshape(1, 3, 1, 1)
    norm = (raw - mean) / std
    assert raw.dtype == np.float32 and norm.dtype == np.float32
    return raw, norm


def _same_bits(t, a):
    return t.dtype == torch.float32 and tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32))


@pytest.mark.parametrize("shape", [(2, 7, 37), (1, 1449, 1448)], ids=["every-byte", "beyond-the-cap"])
def test_u8_to_f32_bit_for_bit_in_its_three_call_forms(dev, shape):
    N, H, W = shape
    img = _ramps(N, H, W)
    if H * W < CAP:
        assert H * W >= 256 and (H * W) % 256 != 0
        for n in range(N):
            for c in range(3):
                assert len(np.unique(img[n, :, :, c])) == 256
        assert not any(np.array_equal(img[..., i], img[..., j]) for i, j in ((0, 1), (0, 2), (1, 2)))      # a swap shows
    else:
        assert N * H * W > CAP
    raw_ref, norm_ref = _to_tensor_reference(img)
    d = torch.from_numpy(img).to(dev)
    raw, norm = ops.u8_to_f32(d, IMAGENET_MEAN, IMAGENET_STD)
    assert _same_bits(raw, raw_ref) and _same_bits(norm, norm_ref)
    raw, norm = ops.u8_to_f32(d)
    assert norm is None and _same_bits(raw, raw_ref)
    raw, norm = ops.u8_to_f32(d, IMAGENET_MEAN, IMAGENET_STD, want_raw=False)
    assert raw is None and _same_bits(norm, norm_ref)


def test_u8_to_f32_refuses_nothing_to_write_and_other_channel_counts(dev):
    d = torch.zeros((1, 4, 5, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.RfxError, match="bad argument"):
        ops.u8_to_f32(d, want_raw=False)
    with pytest.raises(ValueError):
        ops.u8_to_f32(torch.zeros((1, 4, 5, 4), dtype=torch.uint8, device=dev))
