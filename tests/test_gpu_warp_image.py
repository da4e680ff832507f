"""The aligned source images of a whole batch from its device records in one launch (ops.warp_records_u8, rfx_warp_records_u8) and
from a stored flow (ops.warp_flow_u8, rfx_warp_flow_u8), compared AS BYTES with the existing chain
    assemble_records -> per pair ops.grid_sample(u8_to_f32(src) raw, flow) -> clamp(0, 1).mul(255).byte() -> HWC, ``binary`` for the mask
(tests/test_gpu_assemble_records.py holds the first link to the per-pair chain and to the reference, tests/test_gpu_pointwise_exact.py
the second to float64), with the numpy rule of tests/test_warp_image_cpu.py and with the reference's own bytes in
tests/golden/warp_image.npz.  Entries of a record past nbH are NaN, so a kernel that read one would show."""
import os

import numpy as np
import pytest
import torch

import test_gpu_assemble_kitti_records as kitti_helpers
import test_gpu_assemble_records as rec_helpers
from test_warp_image_cpu import CASES, golden, rule_corners, rule_overlay, rule_warp_u8
from rfx import assemble, ops, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
_random_pair, _dense, _ragged = rec_helpers._random_pair, rec_helpers._dense, rec_helpers._ragged


# ---------------------------------------------------------------- helpers

def _image(g, h, w):
    """A uint8 (h,w,3) image: every byte random."""
    return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)


def _chain_image(src, flow):
    """One pair of the chain: src (Hs,Ws,3) uint8 and flow (H,W,2) on the device -> (H,W,3) uint8."""
    raw, _ = ops.u8_to_f32(src[None].contiguous())
    img = ops.grid_sample(raw, flow[None].contiguous())
    return img.clamp(0, 1).mul(255).byte()[0].permute(1, 2, 0).contiguous()


def _chain(R, srcs, th, multiH, cycle, out_hw=None, bg=None, tgts=None):
    """The yardstick for a batch: per pair (img, overlay | None, mask) as uint8 device tensors."""
    fg, _, b, valid = ops.assemble_records(R, th, multiH, cycle, out_hw=out_hw, bg=bg)
    out = []
    for k in range(R.B):
        img = _chain_image(srcs[k], fg[k])
        ov = ((img.to(torch.int32) + tgts[k].to(torch.int32)) >> 1).to(torch.uint8) if tgts is not None else None
        out.append((img, ov, b[k].to(torch.uint8) * 255))
    return out, valid


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.uint8 and bool(torch.equal(a, b))


def _assert_batch(got, want, what, overlay=True, mask=True):
    img, ov, mk, _ = got
    for k, (wi, wo, wm) in enumerate(want):
        assert _same(img[k], wi), (what, k, "img", int((img[k] != wi).sum()))
        if overlay:
            assert _same(ov[k], wo), (what, k, "overlay", int((ov[k] != wo).sum()))
        if mask:
            assert _same(mk[k], wm), (what, k, "mask", int((mk[k] != wm).sum()))


# ---------------------------------------------------------------- 1. dense records

HD, WD = 3, 4
NBH = (1, 2, 11, 0)                                                 # one, several, max_h, none
SRC_HW = ((13, 17), (2, 3), (1, 1), (40, 50))                       # odd, tiny, one pixel, larger than the 24 x 32 map


@pytest.fixture(scope="module")
def dense_case():
    g = torch.Generator().manual_seed(301)
    pairs = [_random_pair(g, n, HD, WD) if n else None for n in NBH]
    return pairs, [_image(g, h, w) for h, w in SRC_HW], g


@pytest.mark.parametrize("out_hw", [(24, 32), (27, 30)], ids=str)
@pytest.mark.parametrize("cycle", [False, True])
@pytest.mark.parametrize("multiH", [False, True])
def test_dense_records_equal_the_chain_byte_for_byte(dev, dense_case, multiH, cycle, out_hw):
    pairs, srcs, _ = dense_case
    g = torch.Generator().manual_seed(302)
    srcs = [s.to(dev) for s in srcs]
    tgts = [_image(g, *out_hw).to(dev) for _ in NBH]
    bg = (torch.rand((4,) + out_hw, generator=g) > 0.4).to(dev)
    th = 0.15 if cycle else 0.35
    R = _dense(pairs, HD, WD, dev)
    ohw = None if out_hw == (24, 32) else out_hw
    got = ops.warp_records_u8(R, srcs, th, multiH, cycle, out_hw=ohw, bg=bg, tgt=torch.stack(tgts), want_mask=True)
    assert got[0].shape == got[1].shape == (4,) + out_hw + (3,) and got[2].shape == (4,) + out_hw and got[0].dtype == torch.uint8
    assert got[3].tolist() == [True, True, True, False] and got[3].device == got[0].device
    want, _ = _chain(R, srcs, th, multiH, cycle, out_hw=ohw, bg=bg, tgts=tgts)
    _assert_batch(got, want, (multiH, cycle, out_hw))
    plain, _ = _chain(R, srcs, th, multiH, cycle, out_hw=ohw)
    assert any(bool((w[2] != p[2]).any()) for w, p in zip(want, plain)), "bg changes no mask byte"
    assert 0 < int((got[2][0] == 255).sum()) < got[2][0].numel() and set(got[2].unique().tolist()) <= {0, 255}
    # the pair without a homography has the zero flow: the source's centre everywhere (one pixel at 40 x 50's centre blend)
    assert bool((got[0][3] == got[0][3][0, 0]).all()) and not bool(got[2][3].any())
    # without bg, tgt or mask: only the image, and the same bytes
    img, ov, mk, _ = ops.warp_records_u8(R, srcs, th, multiH, cycle, out_hw=ohw)
    assert ov is None and mk is None and _same(img, got[0])
    # same-size sources as ONE tensor
    S = torch.stack([srcs[0]] * 4)
    img4 = ops.warp_records_u8(R, S, th, multiH, cycle, out_hw=ohw)[0]
    assert _same(img4[0], got[0][0]) and _same(img4[1], _chain_image(srcs[0], ops.assemble_records(R, th, multiH, cycle, out_hw=ohw)[0][1]))


# ---------------------------------------------------------------- 2. ragged records, positions, empty pairs, slices

RAGGED = ((3, 4, 2), (5, 3, 1), (2, 2, 3), (2, 3, 0))               # (h8, w8, nbH)


def _ragged_pairs(g):
    return [_random_pair(g, max(n, 1), h, w) for h, w, n in RAGGED]


def _ragged_records(pairs, order, dev):
    """The pairs in ``order``; the one with nbH = 0 keeps its sizes and has no homography."""
    R = ops.MultiHRecordsRagged([pairs[k][0].shape[2] for k in order], [pairs[k][0].shape[3] for k in order], dev, max_h=11)
    for b, k in enumerate(order):
        nbH, _, Hs, f8, m8 = R.views(b)
        rec_helpers._fill((nbH, Hs, f8, m8), pairs[k] if RAGGED[k][2] else None, dev)
    return R


@pytest.mark.parametrize("order", [(3, 0, 1, 2), (0, 3, 1, 2), (0, 1, 2, 3)], ids=["empty-first", "empty-middle", "empty-last"])
@pytest.mark.parametrize("cycle", [False, True])
def test_ragged_records_equal_the_chain_at_any_position(dev, order, cycle):
    g = torch.Generator().manual_seed(303)
    pairs = _ragged_pairs(g)
    sizes = [(27, 30), (16, 16), (1, 257), (5, 7)]                  # not 8x, a 1-row map, maps smaller than a wavefront
    srcs = [_image(g, h, w).to(dev) for h, w in ((13, 17), (31, 9), (2, 3), (1, 1))]
    th = 0.15 if cycle else 0.35
    for out_hw in (None, [sizes[k] for k in order]):
        hw = out_hw or [(8 * RAGGED[k][0], 8 * RAGGED[k][1]) for k in order]
        tgts = [_image(g, h, w).to(dev) for h, w in hw]
        bgs = [(torch.rand(h, w, generator=g) > 0.4).to(dev) for h, w in hw]
        R = _ragged_records(pairs, order, dev)
        S = [srcs[k] for k in order]
        got = ops.warp_records_u8(R, S, th, True, cycle, out_hw=out_hw, bg=bgs, tgt=tgts, want_mask=True)
        assert [tuple(t.shape) for t in got[0]] == [s + (3,) for s in hw] and [tuple(t.shape) for t in got[2]] == hw
        assert got[3].tolist() == [RAGGED[k][2] > 0 for k in order]
        want, _ = _chain(R, S, th, True, cycle, out_hw=out_hw, bg=bgs, tgts=tgts)
        _assert_batch(got, want, (order, cycle, out_hw is None))
        # packed storage: the views of one call lie one behind the other
        assert got[0][1].data_ptr() == got[0][0].data_ptr() + 3 * hw[0][0] * hw[0][1]
        assert got[2][1].data_ptr() == got[2][0].data_ptr() + hw[0][0] * hw[0][1]
        # a rows() slice gives the same bytes as the pairs gave inside the whole batch
        sl = ops.warp_records_u8(R.rows(1, 3), S[1:3], th, True, cycle, out_hw=None if out_hw is None else out_hw[1:3], bg=bgs[1:3],
                                 tgt=tgts[1:3], want_mask=True)
        for j in range(2):
            assert _same(sl[0][j], got[0][1 + j]) and _same(sl[1][j], got[1][1 + j]) and _same(sl[2][j], got[2][1 + j]), (order, j)


def test_dense_rows_slice(dev, dense_case):
    pairs, srcs, _ = dense_case
    srcs = [s.to(dev) for s in srcs]
    R = _dense(pairs, HD, WD, dev)
    whole = ops.warp_records_u8(R, srcs, 0.35, True, False, want_mask=True)
    part = ops.warp_records_u8(R.rows(1, 4), srcs[1:], 0.35, True, False, want_mask=True)
    assert _same(part[0], whole[0][1:]) and _same(part[2], whole[2][1:]) and part[3].tolist() == [True, True, False]


# ---------------------------------------------------------------- 3. packed offsets that are no multiple of 4, guard bytes

def test_packed_offsets_unaligned_and_guard_bytes(dev):
    """Maps of 1x1, 5x7, 3x3 and 9x11 pixels in caller-owned buffers that start 2 bytes past a 4-byte boundary: the pairs' images
    start at byte offsets 2, 5, 110 and 137 -- none a multiple of 4 -- and three of the maps are smaller than a wavefront.  Every
    output byte equals the chain's, and the guard bytes before and after each buffer keep their fill."""
    g = torch.Generator().manual_seed(304)
    sizes = [(1, 1), (5, 7), (3, 3), (9, 11)]
    pairs = [_random_pair(g, n, h, w) for (h, w), n in zip(((1, 1), (2, 2), (1, 2), (2, 3)), (2, 1, 3, 2))]
    srcs = [_image(g, h, w).to(dev) for h, w in ((13, 17), (2, 3), (1, 1), (6, 5))]
    tgts = [_image(g, h, w).to(dev) for h, w in sizes]
    bgs = [(torch.rand(h, w, generator=g) > 0.4).to(dev) for h, w in sizes]
    total, GUARD, FILL = sum(h * w for h, w in sizes), 66, 0xAB
    offs = np.cumsum([0] + [h * w for h, w in sizes])[:-1]
    assert all((2 + 3 * int(o)) % 4 for o in offs)
    bufs = [torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device=dev) for n in (3 * total, 3 * total, total)]
    assert all(b.data_ptr() % 4 == 0 for b in bufs)
    out = (bufs[0][GUARD:GUARD + 3 * total].view(total, 3), bufs[1][GUARD:GUARD + 3 * total].view(total, 3), bufs[2][GUARD:GUARD + total])
    assert out[0].data_ptr() % 4 == 2
    R = _ragged(pairs, dev)
    got = ops.warp_records_u8(R, srcs, 0.35, True, True, out_hw=sizes, bg=bgs, tgt=tgts, want_mask=True, out=out)
    assert got[0][0].data_ptr() == out[0].data_ptr() and got[0][3].data_ptr() == out[0].data_ptr() + 3 * int(offs[3])
    want, _ = _chain(R, srcs, 0.35, True, True, out_hw=sizes, bg=bgs, tgts=tgts)
    _assert_batch(got, want, "unaligned")
    for b, n in zip(bufs, (3 * total, 3 * total, total)):
        assert bool((b[:GUARD] == FILL).all()) and bool((b[GUARD + n:] == FILL).all())
    # the packed bytes themselves, one after the other
    assert _same(out[0], torch.cat([w[0].reshape(-1, 3) for w in want])) and _same(out[2], torch.cat([w[2].reshape(-1) for w in want]))
    # the flow form into the same kind of buffers
    for b in bufs:
        b.fill_(FILL)
    fg, _, bn, _ = ops.assemble_records(R, 0.35, True, True, out_hw=sizes, bg=bgs)
    got2 = ops.warp_flow_u8(fg, srcs, tgt=tgts, binary=bn, out=out)
    for k in range(4):
        assert _same(got2[0][k], want[k][0]) and _same(got2[1][k], want[k][1]) and _same(got2[2][k], want[k][2]), k
    for b, n in zip(bufs, (3 * total, 3 * total, total)):
        assert bool((b[:GUARD] == FILL).all()) and bool((b[GUARD + n:] == FILL).all())


# ---------------------------------------------------------------- 4. borders, NaN, degenerate homographies

def test_borders_and_samples_with_corners_outside(dev):
    """Flows built from the source's pixel coordinates k/4, k from two pixels before the image to two after it, on a 4 x 8 source
    (power-of-two sizes: the un-normalised coordinate is exact): samples on -1 and +1, beyond, and with three and two corners
    outside (the 2 x 2 footprint of a sample meets a rectangle in 0, 1, 2 or 4 corners: exactly one corner outside does not
    occur, which is asserted).  The flow form against the chain and against the numpy rule."""
    g = torch.Generator().manual_seed(305)
    Hs, Ws = 4, 8
    src = _image(g, Hs, Ws)
    src[0, 0], src[-1, -1] = 255, 255
    ky, kx = torch.arange(-8, 4 * Hs + 9, dtype=torch.float64) / 4, torch.arange(-8, 4 * Ws + 9, dtype=torch.float64) / 4
    gy, gx = torch.meshgrid((2 * ky + 1) / Hs - 1, (2 * kx + 1) / Ws - 1, indexing="ij")
    flow = torch.stack((gx, gy), -1).float()
    assert torch.equal(flow.double(), torch.stack((gx, gy), -1))
    extra = torch.tensor([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, -1.0], [-1.0, 0.0], [0.0, 1.0], [NAN, 0.0], [0.0, NAN],
                          [float("inf"), 0.0], [0.0, -float("inf")], [1e30, 0.0], [3e9, -3e9], [-1.0000001, 0.3], [1.0000001, -0.3]])
    flow = torch.cat((flow, extra.view(1, -1, 2).expand(flow.shape[0], -1, -1)), dim=1).contiguous()
    _, _, _, xin0, xin1 = rule_corners(flow[..., 0].numpy(), Ws)
    _, _, _, yin0, yin1 = rule_corners(flow[..., 1].numpy(), Hs)
    inside = (yin0 & xin0).astype(int) + (yin0 & xin1) + (yin1 & xin0) + (yin1 & xin1)
    assert all(int((inside == n).sum()) > 10 for n in (0, 1, 2, 4)) and not (inside == 3).any()
    img = ops.warp_flow_u8(flow.to(dev), src.to(dev))[0]
    assert _same(img, _chain_image(src.to(dev), flow.to(dev)))
    want = rule_warp_u8(flow.numpy(), src.numpy())
    assert np.array_equal(img.cpu().numpy(), want)
    assert not img.cpu().numpy()[inside == 0].any() and bool(img[:, -8:-2].eq(0).all())         # NaN, inf, huge: 0
    assert all(img.cpu().numpy()[inside == n].any() for n in (1, 2, 4))


def test_nan_and_degenerate_homography_in_a_record_give_zero_pixels(dev):
    hd, wd = 2, 3
    src = torch.full((5, 6, 3), 200, dtype=torch.uint8)
    one = lambda: torch.ones(1, 2, hd, wd)
    zero_h = (torch.zeros(1, 2, hd, wd), torch.zeros(1, 3, 3), one())           # 0 / 0 everywhere
    nan_flow = (torch.zeros(1, 2, hd, wd), torch.eye(3)[None].clone(), one())
    nan_flow[0][0, 0, 0, 0] = NAN                                               # compose_flow's clamp turns this NaN into -1: no NaN flow
    nan_h = (torch.zeros(1, 2, hd, wd), torch.eye(3)[None].clone(), one())
    nan_h[1][0, 0, 2] = NAN
    ok = (torch.zeros(1, 2, hd, wd), torch.eye(3)[None].clone(), one())
    pairs = [zero_h, nan_flow, nan_h, ok]
    R = _dense(pairs, hd, wd, dev, max_h=2)
    S = torch.stack([src] * 4).to(dev)
    img, _, mask, valid = ops.warp_records_u8(R, S, 0.5, True, False, want_mask=True)
    want, _ = _chain(R, list(S), 0.5, True, False)
    for k in range(4):
        assert _same(img[k], want[k][0]) and _same(mask[k], want[k][2]), k
    assert valid.tolist() == [True] * 4
    assert not bool(img[0].any()) and not bool(img[2].any())                    # every pixel's flow is NaN
    # a finite flow samples the constant source: 200 / 255 under weights that add up to 1 within rounding gives 199 or 200 inside
    for k in (1, 3):
        assert bool((img[k][4:-4, 4:-4] >= 199).all()) and bool((img[k] <= 200).all()), k


# ---------------------------------------------------------------- 5. exact families

def _centres(n, size):
    """Normalised coordinates of the pixel centres 0..n-1 of an axis of ``size`` pixels (size a power of two: exact in float32)."""
    return (2 * torch.arange(n, dtype=torch.float64) + 1) / size - 1


def test_integer_samples_reproduce_all_256_levels(dev):
    lv = torch.arange(256, dtype=torch.uint8).view(16, 16)
    src = torch.stack((lv, lv.flip(0, 1), lv.t()), dim=2).contiguous()
    gy, gx = torch.meshgrid(_centres(16, 16), _centres(16, 16), indexing="ij")
    flow = torch.stack((gx, gy), -1).float().contiguous()
    img = ops.warp_flow_u8(flow.to(dev), src.to(dev))[0]
    assert _same(img.cpu(), src) and _same(img, _chain_image(src.to(dev), flow.to(dev)))
    assert sorted(img[..., 0].reshape(-1).tolist()) == list(range(256))


def test_half_weight_blends_are_the_floor_of_the_mean(dev):
    g = torch.Generator().manual_seed(306)
    src = _image(g, 64, 64)
    src[0, :8, 0] = torch.tensor([0, 255, 254, 1, 0, 1, 255, 255], dtype=torch.uint8)
    gy, gx = torch.meshgrid(_centres(64, 64), _centres(63, 64) + 1.0 / 64, indexing="ij")        # half way to the right neighbour
    flow = torch.stack((gx, gy), -1).float().contiguous()
    img = ops.warp_flow_u8(flow.to(dev), src.to(dev))[0].cpu()
    a, b = src[:, :-1].to(torch.int32), src[:, 1:].to(torch.int32)
    assert torch.equal(img.to(torch.int32), (a + b) >> 1)
    gy, gx = torch.meshgrid(_centres(63, 64) + 1.0 / 64, _centres(64, 64), indexing="ij")        # ... and to the lower one
    flow = torch.stack((gx, gy), -1).float().contiguous()
    img = ops.warp_flow_u8(flow.to(dev), src.to(dev))[0].cpu()
    assert torch.equal(img.to(torch.int32), (src[:-1].to(torch.int32) + src[1:].to(torch.int32)) >> 1)


def test_overlay_of_all_256_x_256_level_pairs(dev):
    """One 256 x 256 map: pixel (a, b) samples source level a (integer samples, exact) and is averaged with target level b; against
    the float64 rule of the reference."""
    a = torch.arange(256, dtype=torch.uint8).view(256, 1, 1).expand(256, 256, 3).contiguous()
    b = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(256, 256, 3).contiguous()
    gy, gx = torch.meshgrid(_centres(256, 256), _centres(256, 256), indexing="ij")
    flow = torch.stack((gx, gy), -1).float().contiguous()
    img, ov, _ = ops.warp_flow_u8(flow.to(dev), a.to(dev), tgt=b.to(dev))
    assert _same(img.cpu(), a)
    assert np.array_equal(ov.cpu().numpy(), rule_overlay(a.numpy(), b.numpy()))


# ---------------------------------------------------------------- 6. the flow form

def test_flow_form_equals_the_records_form(dev, dense_case):
    pairs, srcs, _ = dense_case
    g = torch.Generator().manual_seed(307)
    srcs = [s.to(dev) for s in srcs]
    tgts = torch.stack([_image(g, 24, 32) for _ in NBH]).to(dev)
    R = _dense(pairs, HD, WD, dev)
    want = ops.warp_records_u8(R, srcs, 0.15, True, True, tgt=tgts, want_mask=True)
    fg, _, b, _ = ops.assemble_records(R, 0.15, True, True)
    got = ops.warp_flow_u8(fg, srcs, tgt=tgts, binary=b)
    assert all(_same(x, y) for x, y in zip(got, want[:3]))
    got8 = ops.warp_flow_u8(fg, srcs, binary=b.to(torch.uint8) * 7)             # any non-zero byte counts
    assert got8[1] is None and _same(got8[2], want[2])
    one = ops.warp_flow_u8(fg[1], srcs[1], tgt=tgts[1])                          # a single (H,W,2) map
    assert one[2] is None and _same(one[0], want[0][1]) and _same(one[1], want[1][1])
    assert _same(assemble.aligned_image(fg[1], srcs[1]), want[0][1]) and _same(assemble.aligned_image(fg, srcs, tgts)[1], want[1])
    ar = assemble.aligned_images_records(R, srcs, 0.15, True, True, tgt_u8=tgts, want_mask=True)
    assert all(_same(x, y) for x, y in zip(ar[:3], want[:3]))
    # ragged: the views assemble_records returns are taken as the packed buffer they are; other lists are concatenated
    gr = torch.Generator().manual_seed(308)
    rp = [_random_pair(gr, n, h, w) for h, w, n in RAGGED[:3]]
    Rr = _ragged(rp, dev)
    wr = ops.warp_records_u8(Rr, srcs[:3], 0.35, True, False, want_mask=True)
    fr, _, br, _ = ops.assemble_records(Rr, 0.35, True, False)
    for flows, bins in ((fr, br), ([f.clone() for f in fr], [x.clone() for x in br])):
        gotr = ops.warp_flow_u8(flows, srcs[:3], binary=bins)
        for k in range(3):
            assert _same(gotr[0][k], wr[0][k]) and _same(gotr[2][k], wr[2][k]), k


def test_flow_form_on_the_kitti_assembly(dev):
    """KITTI records are refused by the records form; their assembled flow goes through the flow form and equals the chain."""
    g = torch.Generator().manual_seed(309)
    sizes = [(3, 4, 2, 2, 2), (2, 3, 1, 2, 1)]                                   # h8, w8, hd2, wd2, nbH
    pairs = [kitti_helpers._random_pair(g, n, h, w, h2, w2) for h, w, h2, w2, n in sizes]
    R = kitti_helpers._ragged(pairs, dev)
    srcs = [_image(g, 13, 17).to(dev), _image(g, 30, 41).to(dev)]
    with pytest.raises(ValueError, match="flowD2"):
        ops.warp_records_u8(R, srcs, 0.3, True, False)
    fg, _, b, _ = ops.assemble_kitti_records(R, 0.3, True)
    img, _, mask = ops.warp_flow_u8(fg, srcs, binary=b)
    for k in range(2):
        assert _same(img[k], _chain_image(srcs[k], fg[k])) and _same(mask[k], b[k].to(torch.uint8) * 255), k


# ---------------------------------------------------------------- 7. the pipeline

def test_align_pairs_want_u8_is_the_byte_image_of_img1_fine(dev):
    from rfx import weights
    from rfx.pipeline import AlignPipeline
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3))
    pipe = AlignPipeline(sds, nbScale=3, nbIter=100, tolerance=0.05, minSize=160, scaleR=1.2, device=dev)
    same = [synth.make_pair(128, 160, seed=5)]
    mixed = [synth.make_pair(128, 160, seed=5), (synth.make_pair(120, 168, seed=6)[0], synth.make_pair(136, 152, seed=6)[1])]
    def check(res):
        for r in res:
            want = (r["img1_fine"].clamp(0, 1) * 255).byte()[0].permute(1, 2, 0).contiguous()
            assert r["img1_fine_u8"].shape == (1,) + tuple(want.shape) and _same(r["img1_fine_u8"][0], want)
            assert int(want.max()) > 100

    for pairs in (same, mixed):
        torch.manual_seed(1)
        check(pipe.align_pairs(pairs, fine=True, want_u8=True))
    assert "img1_fine_u8" not in pipe.align_pairs(same, fine=True)[0]
    # the device preps hold the bytes anyway; the PIL preps only on request
    check(pipe.align_prepared(pipe.prepare_device(*pipe.upload_raw(same)), fine=True, want_u8=True))
    check(pipe.align_prepared(pipe.prepare_ragged_device(*pipe._upload_lists(mixed)), fine=True, want_u8=True))
    assert pipe.prepare(same)["Is_u8"] is None and pipe.prepare_ragged(mixed)["Is_u8"] is None
    with pytest.raises(ValueError, match="Is_u8"):
        pipe.align_prepared(pipe.prepare(same), fine=True, want_u8=True)


# ---------------------------------------------------------------- 8. beyond the launch cap

def test_maps_beyond_the_launch_cap(dev):
    """The grid is capped at 8192 workgroups of 256 pixels per pair: a 1450 x 1450 map (2 102 500 > 2 097 152 pixels) takes a second
    trip.  The source is an index image: every pixel another value in its three bytes."""
    hd, wd, out_hw = 6, 7, (1450, 1450)
    idx = (torch.arange(2 * hd * wd, dtype=torch.float32) + 1).view(1, 2, hd, wd)
    pm = torch.eye(3)[None].clone()
    pm[0, 1, 2] = -0.0625
    pair = (idx * 2.0 ** -10, pm, idx / float(2 * hd * wd))
    n = torch.arange(300 * 300, dtype=torch.int32).view(300, 300)
    src = torch.stack((n & 255, (n >> 8) & 255, (n >> 16) + 7), dim=2).to(torch.uint8).contiguous().to(dev)
    R = _dense([pair], hd, wd, dev, max_h=2)
    img, _, mask, _ = ops.warp_records_u8(R, src[None], 0.3, True, False, out_hw=out_hw, want_mask=True)
    want, _ = _chain(R, [src], 0.3, True, False, out_hw=out_hw)
    assert _same(img[0], want[0][0]) and _same(mask[0], want[0][2])
    assert bool(img[0, -1].any()) and bool(mask[0, -1].any()) and not bool(mask[0, 0].any())
    # the flow form beyond the cap
    fg = ops.assemble_records(R, 0.3, True, False, out_hw=out_hw)[0]
    assert _same(ops.warp_flow_u8(fg, src[None])[0], img)


# ---------------------------------------------------------------- 9. no host sync

def test_the_calls_do_not_sync_with_the_host(dev, dense_case):
    pairs, srcs, _ = dense_case
    srcs = [s.to(dev) for s in srcs]
    tgts = torch.zeros((4, 24, 32, 3), dtype=torch.uint8, device=dev)
    R = _dense(pairs, HD, WD, dev)
    Rr = _ragged([p for p in pairs[:3]], dev)
    bg = torch.ones((4, 24, 32), dtype=torch.bool, device=dev)
    ops.warp_records_u8(R, srcs, 0.3, True, True, bg=bg, tgt=tgts, want_mask=True)       # the library is loaded, the allocators are warm
    fg, _, b, _ = ops.assemble_records(R, 0.3, True, True)
    ops.warp_flow_u8(fg, srcs, binary=b)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                           # the mode does see a sync on this build
            R.rec[0, 0].item()
        out = ops.warp_records_u8(R, srcs, 0.3, True, True, bg=bg, tgt=tgts, want_mask=True)
        out_r = ops.warp_records_u8(Rr, srcs[:3], 0.3, True, False, out_hw=[(27, 30), (16, 16), (1, 257)])
        out_f = ops.warp_flow_u8(fg, srcs, tgt=tgts, binary=b)
        out_a = assemble.aligned_images_records(R, srcs, 0.3, True, True)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert out[3].is_cuda and out_r[3].is_cuda and out_a[3].is_cuda and out_f[0].is_cuda
    assert out[3].tolist() == [True, True, True, False] and _same(out_f[0], out[0]) and _same(out_a[0], out[0])


# ---------------------------------------------------------------- 10. the reference's own bytes

def test_records_of_the_golden_inputs_give_the_reference_images(dev):
    """Every byte equals the device chain; every byte is within one level of the reference's CPU bytes: the flows are held to the
    reference by tests/test_gpu_assemble_records.py, and float32 differences of a few ulp in v move v * 255 by far less than one
    level, so the truncation flips by at most one -- and with it the overlay's sum by one, its half by at most one."""
    g = golden()
    n, hd, wd = int(g["n"]), int(g["hd"]), int(g["wd"])
    ch, cw = (int(v) for v in g["cut"])
    fd, _, pm, md = synth.assembly_arrays(int(g["seed"]), n, hd, wd)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    full, cut = (t(fd), t(pm), t(md)), (t(fd[:, :, :ch, :cw]), t(pm), t(md[:, :, :ch, :cw]))
    srcs = [torch.from_numpy(g["src0"]).to(dev), torch.from_numpy(g["src1"]).to(dev)]
    tgt = torch.from_numpy(g["tgt"]).to(dev)
    exact = total = 0
    for k in CASES:
        cfg = g[k + "_cfg"]
        hpatch = k.startswith("hpatch")
        pair, hw8 = (full, (hd, wd)) if hpatch else (cut, (ch, cw))
        R = _dense([pair, pair], hw8[0], hw8[1], dev, max_h=max(n, 4))                   # the same record under both sources
        out_hw = (int(cfg[2]), int(cfg[3])) if hpatch else None
        got = ops.warp_records_u8(R, srcs, float(cfg[0]), bool(cfg[1]), not hpatch, out_hw=out_hw, tgt=torch.stack([tgt, tgt]))
        want, _ = _chain(R, srcs, float(cfg[0]), bool(cfg[1]), not hpatch, out_hw=out_hw, tgts=[tgt, tgt])
        _assert_batch(got, want, k, mask=False)
        for s in range(2):
            d = got[0][s].cpu().numpy().astype(np.int32) - g["%s_img%d" % (k, s)]
            assert np.abs(d).max() <= 1, (k, s, int(np.abs(d).max()), int((d != 0).sum()))
            do = got[1][s].cpu().numpy().astype(np.int32) - g["%s_avg%d" % (k, s)]
            assert np.abs(do).max() <= 1, (k, s, int(np.abs(do).max()))
            exact += int((d == 0).sum())
            total += d.size
    print("golden: %d of %d image bytes equal the reference's, the others are one level away" % (exact, total))
