"""Sky masks for a batch of targets on the device: Pillow's BILINEAR through the table-driven resampler, the fused up-sample /
softmax / average / arg-max kernel against the three-kernel chain it replaces, the scripts' ``imresize(mask, (h, w)) < 128``,
SegNetDevice.get_sky_batch against get_sky_device per image, and the ``seg=`` argument of the pairs drivers against It_bg made on the
host from getSky.  Everything is held bit for bit.  ``-m gpu``."""
import os

import numpy as np
import pytest
import torch
import PIL.Image as Image

from rfx import ops, weights, synth
from rfx.pipeline import AlignPipeline, resize_dims
from rfx.segnet import SegNetDevice, input_sizes, img_transform
from test_sky_cpu import case_image, pil_resize, script_background, sky_maps

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------- pil_resize_u8
def test_pil_resize_u8_bilinear_and_lanczos_equal_pillow():
    rgb = np.stack([case_image(3, (96, 128), s) for s in (1, 2)])
    kitti = np.stack([case_image(3, (375, 1242), s) for s in (3, 4)])
    maps = np.stack([case_image(1, (97, 131), s) for s in (5, 6)])
    # (the five scales of a 96 x 128 image come in two sizes: the long side stops at 500)
    cases = [(rgb, (th, tw)) for tw, th in sorted(set(input_sizes(128, 96)))] + [(kitti, (152, 504)), (maps, (48, 64)), (maps, (200, 131))]
    for batch, out_hw in cases:
        x = _up(batch)
        for name, pil in (("bilinear", Image.BILINEAR), ("lanczos", Image.LANCZOS)):
            got = (ops.pil_resize_u8(x, out_hw[1], out_hw[0], name) if name == "bilinear" else ops.lanczos_resize_u8(x, out_hw[1], out_hw[0]))
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, out_hw[0], out_hw[1], batch.shape[3])
            for n in range(2):
                assert np.array_equal(got[n].cpu().numpy(), pil_resize(batch[n], out_hw, pil)), (name, batch.shape, out_hw, n)
    assert torch.equal(ops.pil_resize_u8(_up(rgb), 400, 304), ops.lanczos_resize_u8(_up(rgb), 400, 304))
    assert torch.equal(ops.pil_resize_u8(_up(rgb), 128, 96, "bilinear"), _up(rgb))               # unchanged size: Pillow copies
    with pytest.raises(ValueError):
        ops.pil_resize_u8(_up(rgb), 64, 48, "bicubic")


# ---------------------------------------------------------------------------------------------------- seg_vote
MAP_SIZES = [(5, 7), (7, 9), (9, 12), (11, 14), (13, 17)]


def _logits(N, C, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(N, C, h, w, generator=g) * 3).to(DEV) for h, w in sizes]


def _chain(logits, out_hw, cid, complement, div=None):
    """segNet/segEval.py:27-43 as SegNetDevice.scores + get_sky_device run it: three kernels per scale and one at the end."""
    scores = None
    for l in logits:
        scores = ops.softmax_accum(ops.resize_bilinear(l, out_hw, align_corners=False), scores, div=float(len(logits) if div is None else div))
    return ops.argmax_mask(scores, cid, complement=complement, want_pred=True)


def _assert_vote_is_chain(logits, out_hw, div=None):
    _, pred_c = _chain(logits, out_hw, 0, False, div)
    cid = int(pred_c.flatten().mode()[0])
    for complement in (False, True):
        mask_c, pred_c = _chain(logits, out_hw, cid, complement, div)
        mask, pred = ops.seg_vote(logits, out_hw, cid, complement=complement, want_pred=True, div=div)
        assert pred.dtype == torch.int32 and mask.dtype == torch.float32 and mask.shape == pred.shape == (logits[0].shape[0],) + tuple(out_hw)
        assert torch.equal(pred, pred_c) and torch.equal(mask, mask_c)
        assert torch.equal(ops.seg_vote(logits, out_hw, cid, complement=complement, div=div), mask_c)      # without pred
    assert 0.0 < float(mask_c.mean()) < 1.0
    return pred_c


@pytest.mark.parametrize("case", ["up", "down", "one_scale", "one_class", "eight_scales_div"])
def test_seg_vote_equals_the_three_kernel_chain(case):
    if case == "up":                                                        # 37 * 51 * 2 pixels: no multiple of the 256-thread block
        pred = _assert_vote_is_chain(_logits(2, 150, MAP_SIZES, 1), (37, 51))
        assert len(pred.unique()) > 20
    elif case == "down":                                                    # smaller than the largest map
        _assert_vote_is_chain(_logits(2, 150, MAP_SIZES, 2), (4, 6))
    elif case == "one_scale":
        _assert_vote_is_chain(_logits(2, 150, MAP_SIZES[2:3], 3), (37, 51))
    elif case == "one_class":
        lg = _logits(2, 1, MAP_SIZES, 4)
        mask_c, pred_c = _chain(lg, (37, 51), 0, False)
        mask, pred = ops.seg_vote(lg, (37, 51), 0, want_pred=True)
        assert torch.equal(pred, pred_c) and torch.equal(mask, mask_c) and int(pred.abs().max()) == 0 and float(mask.min()) == 1.0
        assert torch.equal(ops.seg_vote(lg, (37, 51), 0, complement=True), torch.zeros_like(mask))
    else:                                                                   # the most maps the kernel takes, div not their number
        _assert_vote_is_chain(_logits(1, 19, MAP_SIZES + [(3, 3), (1, 1), (16, 2)], 5), (33, 47), div=5.0)


def test_seg_vote_ties_nan_and_refusals():
    # two identical, dominant class planes in every scale: exactly equal sums, the lower index wins at every pixel
    lg = _logits(2, 150, MAP_SIZES, 6)
    for l in lg:
        l[:, 63] = l[:, 17] = l[:, 17] * 0.1 + 30.0
    mask_c, pred_c = _chain(lg, (37, 51), 17, False)
    mask, pred = ops.seg_vote(lg, (37, 51), 17, want_pred=True)
    assert torch.equal(pred, pred_c) and torch.equal(mask, mask_c)
    assert bool((pred == 17).all()) and float(mask.min()) == 1.0
    assert float(ops.seg_vote(lg, (37, 51), 63).max()) == 0.0
    # one NaN logit: the class the chain gives, at the pixels it reaches and everywhere else
    lg = _logits(2, 150, MAP_SIZES, 7)
    lg[1][1, 40, 3, 4] = float("nan")
    mask_c, pred_c = _chain(lg, (37, 51), 40, False)
    mask, pred = ops.seg_vote(lg, (37, 51), 40, want_pred=True)
    assert torch.equal(pred, pred_c) and torch.equal(mask, mask_c)
    assert not torch.equal(pred[1], _chain(_logits(2, 150, MAP_SIZES, 7), (37, 51), 40, False)[1][1])      # the NaN did reach pixels
    with pytest.raises(ValueError):
        ops.seg_vote([], (4, 4), 0)
    with pytest.raises(ValueError):
        ops.seg_vote(_logits(1, 3, [(2, 2)] * 9, 8), (4, 4), 0)
    with pytest.raises(ValueError):
        ops.seg_vote(_logits(1, 3, [(2, 2)], 8) + _logits(1, 4, [(2, 2)], 8), (4, 4), 0)
    with pytest.raises(RuntimeError):
        ops.seg_vote([torch.zeros(1, 3, 2, 2)], (4, 4), 0)
    with pytest.raises(ops._lib.RfxError):
        ops.seg_vote(_logits(1, 3, [(2, 2)], 8), (0, 4), 0)


def test_seg_vote_allocates_no_class_volume():
    """A condition on the design: the call's outputs are 8 bytes per pixel, nothing of size N * C * H * W exists at any time."""
    N, C, H, W = 2, 150, 96, 128
    lg = _logits(N, C, [(th // 8, tw // 8) for tw, th in input_sizes(W, H)], 9)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    mask, pred = ops.seg_vote(lg, (H, W), 3, want_pred=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("seg_vote peak rise %d bytes; one class volume %d bytes" % (rise, N * C * H * W * 4))
    assert rise < N * C * H * W * 4 // 4
    mask_c, pred_c = _chain(lg, (H, W), 3, False)
    assert torch.equal(pred, pred_c) and torch.equal(mask, mask_c)


# ---------------------------------------------------------------------------------------------------- sky_background
def test_sky_background_equals_imresize_and_threshold():
    maps = sky_maps((61, 83), seed=2)
    names = ["mixed", "zeros", "ones"]
    batch = _up(np.stack([maps[n] for n in names]))
    single = _up(maps["one_px"][None])
    for k in range(4):
        for out in ((48, 64), (200, 131)):
            out = out[::-1] if k & 1 else out
            got = ops.sky_background(batch, out, k)
            assert got.dtype == torch.float32 and tuple(got.shape) == (3,) + out
            for n, name in enumerate(names):                                 # the byte rule is per map, not per batch
                assert np.array_equal(got[n].cpu().numpy(), script_background(maps[name], out, k)), (name, out, k)
            assert 0.0 < float(got[0].mean()) < 1.0 and float(got[1:].min()) == 1.0
            assert np.array_equal(ops.sky_background(single, out, k)[0].cpu().numpy(), script_background(maps["one_px"], out, k))
        # the byte map itself
        b = ops.sky_bytes(batch, k)[..., 0].cpu().numpy()
        assert np.array_equal(b[0], np.rot90((maps["mixed"] * 255).astype(np.uint8), k)) and not b[1:].any()
    # two sizes from one call (evaluation/evalKITTI/evaluation.py:247-248), and an unchanged size
    two = ops.sky_background(batch, [(48, 64), (200, 131), (61, 83)])
    assert isinstance(two, list) and len(two) == 3
    for got, out in zip(two, ((48, 64), (200, 131), (61, 83))):
        for n, name in enumerate(names):
            assert np.array_equal(got[n].cpu().numpy(), script_background(maps[name], out, 0)), (name, out)
    with pytest.raises(ValueError):
        ops.sky_background(batch, (48, 64), 4)


# ---------------------------------------------------------------------------------------------------- the network
IMAGES = [(96, 128, 3), (72, 104, 1), (96, 128, 5)]       # (H, W, seed); the first is the image of tests/golden/seg.npz


@pytest.fixture(scope="module")
def seg():
    g = np.load(os.path.join(GOLD, "seg.npz"))
    enc, dec = weights.seg_encoder_sd(4, randomize_bn=True), weights.seg_decoder_sd(5, randomize_bn=True, logit_std=0.003)
    net = SegNetDevice(enc, dec, segId=int(g["seg_id"]), segFg=True, device=DEV)
    imgs = [synth.make_pair(h, w, seed=s)[0] for h, w, s in IMAGES]
    single = [net.get_sky_device(im, want_pred=True) for im in imgs]          # the reference of every test below, computed once
    return dict(net=net, imgs=imgs, single=single, gold=g)


def test_network_inputs_equal_the_host_transform(seg):
    for im in seg["imgs"][:2]:
        W, H = im.size
        got = seg["net"].scale_inputs(_up(np.array(im.convert("RGB")))[None])
        assert len(got) == 5
        for x, (tw, th) in zip(got, input_sizes(W, H)):
            ref = img_transform(im.resize((tw, th), Image.BILINEAR)).unsqueeze(0)
            assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, th, tw) and torch.equal(x.cpu(), ref), (im.size, tw, th)


@pytest.mark.parametrize("max_batch", [8, 1])
def test_get_sky_batch_equals_get_sky_device_per_image(seg, max_batch):
    net, imgs, single = seg["net"], seg["imgs"], seg["single"]
    for m, _ in single:
        assert 0.0 < float(m.mean()) < 1.0                                   # every mask holds both values
    u8 = [_up(np.array(im.convert("RGB"))) for im in imgs]
    masks, preds = net.get_sky_batch(u8, max_batch=max_batch, want_pred=True)
    assert len(masks) == len(preds) == 3
    for (m1, p1), m, p in zip(single, masks, preds):
        assert m.shape == m1.shape and torch.equal(m, m1) and torch.equal(p, p1)
    if max_batch == 8:
        only = net.get_sky_batch(imgs)                                       # PIL images, masks only
        assert all(torch.equal(a, b[0]) for a, b in zip(only, single))
        frac = float((preds[0].cpu().numpy() != seg["gold"]["pred"]).mean())
        print("golden: %.5f of the pixels differ in class" % frac)
        assert frac < 2e-3
        with pytest.raises(ValueError):
            net.get_sky_batch(u8, max_batch=0)
        with pytest.raises(TypeError):
            net.get_sky_batch([u8[0].float()])


def test_get_sky_batch_of_five_images_of_one_shape(seg):
    """From four images on, the 1 x 1 pooled map of a batch would reach the k-major kernel's chunked sums (ppm.0, the pyramid branch
    of pool scale 1): the batched decoder runs that layer image by image, and a mask does not depend on its batch."""
    net = seg["net"]
    imgs = [seg["imgs"][1], synth.make_pair(72, 104, seed=2)[0]]
    single = [seg["single"][1], net.get_sky_device(imgs[1], want_pred=True)]
    order = [0, 1, 0, 1, 1]
    masks, preds = net.get_sky_batch([imgs[i] for i in order], want_pred=True)
    for i, m, p in zip(order, masks, preds):
        assert torch.equal(m, single[i][0]) and torch.equal(p, single[i][1])
    assert not torch.equal(single[0][1], single[1][1])


# ---------------------------------------------------------------------------------------------------- drivers
# (seed, H, W, rows / columns cropped off the target): the first two pairs of the ragged driver tests, at their settings
PAIRS = [(7, 240, 320, 0, 0), (8, 256, 320, 0, 16)]


def _pairs():
    out = []
    for seed, H, W, dh, dw in PAIRS:
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
        out.append((I1, I2.crop((0, 0, W - dw, H - dh))))
    return out


def _pipe(variant):
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    return AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant=variant, device=DEV, seed=5,
                         degenerate="lapack")


def _host_bg(net, target, k, min_size):
    """The scripts' It_bg of one target: getSky on the PIL image, the quarter turns, imresize to the resized (turned) target, < 128."""
    mask = net.getSky(target)
    h, w = mask.shape[::-1] if k & 1 else mask.shape
    nw, nh = resize_dims(w, h, min_size, "min")
    return torch.from_numpy(script_background(mask, (nh, nw), k)).to(DEV)


def _assert_same_results(a, b, keys):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["nbH"] == y["nbH"] == len(x["H"]) and all(x.get(k) == y.get(k) for k in keys)
        assert torch.equal(x["mask"], y["mask"])
        for key in ("H", "flowDown8", "matchDown8"):
            assert len(x[key]) == len(y[key]) and all(torch.equal(p, q) for p, q in zip(x[key], y[key])), key


def test_multi_h_pairs_with_seg_equals_host_made_backgrounds(seg):
    net, pairs, pipe = seg["net"], _pairs(), _pipe("B")
    bgs = [_host_bg(net, p[1], 0, 240) for p in pairs]
    print("background fraction per pair:", [round(1.0 - float(b.mean()), 4) for b in bgs])
    dev_bgs = pipe.sky_backgrounds(net, [_up(np.array(p[1])) for p in pairs], [tuple(b.shape) for b in bgs])
    assert all(torch.equal(a, b) for a, b in zip(dev_bgs, bgs))
    kw = dict(maxCoarse=3, maskRegionTh=0.01, pair_ids=[100, 107])
    ref = pipe.multi_h_pairs(pairs, It_bg=bgs, **kw)
    got = pipe.multi_h_pairs(pairs, seg=net, **kw)
    _assert_same_results(got, ref, ())
    with pytest.raises(ValueError):
        pipe.multi_h_pairs(pairs, seg=net, It_bg=bgs, **kw)
    with pytest.raises(ValueError):
        pipe.multi_h_kitti_pairs(pairs, seg=net, It_bg=bgs)


def test_multi_h_variant_c_pairs_with_seg_equals_host_made_backgrounds(seg):
    net, pairs, pipe = seg["net"], _pairs(), _pipe("C")
    angles = (0, 90)
    bgs = [[_host_bg(net, p[1], a // 90, 240) for p in pairs] for a in angles]
    kw = dict(angles=angles, maxCoarse=3, maskRegionTh=0.03, pair_ids=[100, 107])
    ref = pipe.multi_h_variant_c_pairs(pairs, It_bg=bgs, **kw)
    got = pipe.multi_h_variant_c_pairs(pairs, seg=net, **kw)
    _assert_same_results(got, ref, ("candidate", "nbInlier"))
    with pytest.raises(ValueError):
        pipe.multi_h_variant_c_pairs(pairs, seg=net, It_bg=bgs, **kw)
