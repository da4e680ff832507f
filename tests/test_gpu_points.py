"""The point correspondences and the keypoint transfer on the device (csrc/points.hip: rfx_flow_points_f32, rfx_sample_points_f32;
ops.flow_points / matches_from_flow / sample_points; assemble.assemble_yfcc / yfcc_matches / corr_alignment_error) against the rule
stated in numpy in tests/test_points_cpu.py, which that file pins to the reference's own outputs.  Integer positions and float32
steps rounded one by one: everything is compared with torch.equal, pts1 as int32 bit patterns; no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

from rfx import _lib, assemble, ops, synth
from test_points_cpu import TILE, golden, rule_alignment_error, rule_points, rule_sample, sha

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flow(rng, shape):
    """Distinct-looking float32 flows in [-1, 1) formed in float64: their sums with 1 are inexact, and a row that lands in the
    wrong place shows."""
    return (rng.rand(*shape, 2) * 2 - 1).astype(np.float32)


def _size_b(shape, k):
    """(wB, hB) of the unrotated target whose grid, turned k times, has the maps' shape."""
    return (shape[1], shape[0]) if k % 2 == 0 else (shape[0], shape[1])


def _check(flow, keep, sizeA, angle, dev, what, bg=None):
    """One batch (N,H,W,...) through ops.matches_from_flow: rows and offsets equal to the rule's."""
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    sizeB = _size_b(keep.shape[1:], (angle // 90) % 4)
    pts1, pts2, off = ops.matches_from_flow(up(flow), up(keep), sizeA, sizeB, angle, bg=up(bg))
    w1, w2, woff = rule_points(flow, keep, sizeA, sizeB, angle, bg)
    assert pts1.is_cuda and pts2.is_cuda and pts1.dtype == torch.float32 and pts2.dtype == torch.int64 and off.dtype == torch.int64
    assert torch.equal(off, torch.from_numpy(woff)), what
    assert tuple(pts1.shape) == tuple(pts2.shape) == (len(w1), 2), what
    assert torch.equal(pts2.cpu(), torch.from_numpy(w2)), what
    assert torch.equal(pts1.cpu().view(torch.int32), torch.from_numpy(w1.view(np.int32))), what
    return pts1, pts2, off


def test_every_mask_of_a_3x4_map_in_one_batch(dev):
    """All 4096 masks of a 3 x 4 map as ONE batch, for each quarter turn: offsets are the cumulative counts, the empty map (map 0)
    and the full one (map 4095) included."""
    bits = (np.arange(4096)[:, None] >> np.arange(12)[None, :]) & 1
    masks = bits.reshape(4096, 3, 4).astype(bool)
    flow = _flow(np.random.RandomState(0), (4096, 3, 4))
    for k in range(4):
        _, _, off = _check(flow, masks, (640 + k, 480 - k), 90 * k, dev, "3x4 exhaustive, k = %d" % k)
        assert off[0] == off[1] == 0 and off[-1] == 4096 * 6 and off[-1] - off[-2] == 12


def _masks(H, W, rng):
    n = H * W
    p = np.arange(n)
    fam = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": p == 0, "last": p == n - 1,
           "beside multiples of 64": (p % 64 == 0) | (p % 64 == 63), "p = 0.5": rng.rand(n) < 0.5, "p = 0.05": rng.rand(n) < 0.05}
    return {name: m.reshape(1, H, W) for name, m in fam.items()}


SHAPES = [(1, m + d) for m in (64, 256, 1024, 4096) for d in (-1, 0, 1)] + [(1, 1), (31, 33), (37, 83)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_tile_and_wavefront_edges(dev, shape):
    """Single maps whose size sits on, one below and one above a wavefront (64), a pass (256), a tile (1024) and four tiles; the
    masks that put the first and the last kept pixel of a ballot, a pass and a tile on those edges."""
    assert TILE == 1024
    H, W = shape
    rng = np.random.RandomState(H * 10007 + W)
    flow = _flow(rng, (1, H, W))
    for q, (name, m) in enumerate(_masks(H, W, rng).items()):
        angle = 90 * (q % 4)
        if angle in (90, 270):                                     # the same pixels as a (W,H) map: both orientations of every shape
            m, f = m.reshape(1, W, H), flow.reshape(1, W, H, 2)
        else:
            f = flow
        _check(f, m, (640, 480), angle, dev, "%dx%d %s" % (H, W, name))


def test_mixed_batch_with_and_without_background(dev):
    """Five non-square maps, one empty and one full, each quarter turn, with and without bg; the buffers of flow_points hold
    N*H*W rows, of which only the first offsets[-1] are the result."""
    rng = np.random.RandomState(3)
    N, H, W = 5, 37, 83                                            # 3071 pixels: three tiles per map, the last one short
    keep = rng.rand(N, H, W) < 0.4
    keep[1], keep[3] = False, True
    bg = rng.rand(N, H, W) < 0.8
    flow = _flow(rng, (N, H, W))
    for k in range(4):
        shape = (N, H, W) if k % 2 == 0 else (N, W, H)
        f, m, b = flow.reshape(shape + (2,)), keep.reshape(shape), bg.reshape(shape)
        _, _, off = _check(f, m, (1920, 1080), 90 * k, dev, "mixed, k = %d" % k)
        assert off[2] == off[1] and off[4] - off[3] == H * W
        _, _, offb = _check(f, m, (1920, 1080), 90 * k, dev, "mixed with bg, k = %d" % k, bg=b)
        assert offb[2] == offb[1] and 0 < offb[4] - offb[3] < H * W
        for dm in (torch.from_numpy(m).to(dev), torch.from_numpy(m.astype(np.uint8) * 7).to(dev)):   # bytes: any non-zero value counts
            p1, p2, o = ops.flow_points(torch.from_numpy(f).to(dev), dm, (1920, 1080), _size_b(shape[1:], k), 90 * k)
            assert tuple(p1.shape) == tuple(p2.shape) == (N * H * W, 2) and o.is_cuda and tuple(o.shape) == (N + 1,)
            assert torch.equal(o.cpu(), off)
            w1, w2, _ = rule_points(f, m, (1920, 1080), _size_b(shape[1:], k), 90 * k)
            assert torch.equal(p2[:int(off[-1])].cpu(), torch.from_numpy(w2))
            assert torch.equal(p1[:int(off[-1])].cpu().view(torch.int32), torch.from_numpy(w1.view(np.int32)))
    # a single (H,W,2) map: two results, no offsets
    one = ops.matches_from_flow(torch.from_numpy(flow[0]).to(dev), torch.from_numpy(keep[0]).to(dev), (640, 480), (W, H), 0)
    w1, w2, _ = rule_points(flow[:1], keep[:1], (640, 480), (W, H), 0)
    assert len(one) == 2 and torch.equal(one[1].cpu(), torch.from_numpy(w2))
    assert torch.equal(one[0].cpu().view(torch.int32), torch.from_numpy(w1.view(np.int32)))
    # an empty batch: (0,2) results
    e = ops.matches_from_flow(torch.from_numpy(flow).to(dev), torch.zeros(N, H, W, dtype=torch.bool, device=dev), (640, 480), (W, H))
    assert tuple(e[0].shape) == tuple(e[1].shape) == (0, 2) and e[2].tolist() == [0] * (N + 1)


def test_more_tiles_than_any_grid(dev):
    """9000 maps of 2 x 3: one tile each, more tiles than the launch's 8192 workgroups -- they stride -- and nine trips of the scan."""
    rng = np.random.RandomState(9)
    keep = rng.rand(9000, 2, 3) < 0.5
    flow = _flow(rng, (9000, 2, 3))
    _check(flow, keep, (640, 480), 0, dev, "9000 maps")
    _check(flow.reshape(9000, 3, 2, 2), keep.reshape(9000, 3, 2), (640, 480), 270, dev, "9000 maps, k = 3")


def test_pts1_is_three_float32_steps(dev):
    """add 1, times (size - 1), halve -- each rounded to float32 -- on flows where a fused, reordered or double-precision step
    differs: +-1, -0.0, the float32 neighbours of +-1, halves of an ulp of 1 (ties of the first step), seeded values formed in float64."""
    f32 = np.float32
    special = [1.0, -1.0, -0.0, 0.0, np.nextafter(f32(1), f32(2)), np.nextafter(f32(1), f32(0)), np.nextafter(f32(-1), f32(-2)),
               np.nextafter(f32(-1), f32(0)), 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25,
               1e-8, -1e-8, 0.5, -0.5, 1.0 / 3, -1.0 / 3]
    rng = np.random.RandomState(11)
    x = np.concatenate((np.asarray(special, np.float32), (rng.rand(4000) * 2 - 1).astype(f32), (rng.randn(76) * 1e-3).astype(f32)))
    y = x[::-1].copy()
    flow = np.stack((x, y), axis=1).reshape(1, 1, len(x), 2)
    keep = np.ones((1, 1, len(x)), bool)
    sizes = (2, 640, 1920, 4096)                                   # size - 1 = 1, 639, 1919, 4095
    differs = 0
    for i, wA in enumerate(sizes):
        hA = sizes[(i + 1) % 4]
        pts1, _, _ = _check(flow, keep, (wA, hA), 0, dev, "wA = %d" % wA)
        once = ((x.astype(np.float64) + 1) * (wA - 1) / 2).astype(f32)               # rounded once: what float64 steps would give
        differs += int((pts1[:, 0].cpu().numpy() != once).sum())
    assert differs > 0                                             # the inputs do tell the two apart


def test_goldens_through_the_device(dev):
    """The reference's flowGlobal / binary in, the reference's pts1 / pts2 out (their SHA-256, and one combination row for row),
    for every case and angle; the keypoint transfer and the alignment tally against the alignmentError golden."""
    G = golden()
    g = G["raw"]
    for c, (th, multiH, flow, binary) in enumerate(G["cases"]):
        for a, angle in enumerate(G["angles"]):
            pts1, pts2 = assemble.yfcc_matches(flow[None], binary[None], G["sizeA"][a], G["sizeB"][a], angle)
            assert pts1.is_cuda and len(pts1) == int(g["case%d_a%d_n" % (c, a)])
            p1, p2 = pts1.cpu().numpy(), pts2.cpu().numpy()
            assert p1.dtype == np.float32 and p2.dtype == np.int64
            assert sha(p1) == str(g["case%d_a%d_sha1" % (c, a)]) and sha(p2) == str(g["case%d_a%d_sha2" % (c, a)]), (c, angle)
            if (c, a) == (int(g["full_case"]), int(g["full_angle"])):
                assert torch.equal(pts1.cpu().view(torch.int32), torch.from_numpy(g["full_pts1"].view(np.int32)))
                assert torch.equal(pts2.cpu(), torch.from_numpy(g["full_pts2"].astype(np.int64)))
        # the background mask fused: the reference's mask already carries it, so the result is the same
        up = lambda x: torch.from_numpy(x).to(dev)
        again = ops.matches_from_flow(up(flow), up(binary), G["sizeA"][0], G["sizeB"][0], 0, bg=up(G["bg"]))
        assert sha(again[0].cpu().numpy()) == str(g["case%d_a0_sha1" % c]) and sha(again[1].cpu().numpy()) == str(g["case%d_a0_sha2" % c])
    wB, hB, wA, hA = (int(v) for v in g["ae_dims"])
    flow, match = g["ae_flow"], g["ae_match"]
    xb, yb = g["ae_XB"].astype(np.int64), g["ae_YB"].astype(np.int64)
    xa, ya, keep = ops.sample_points(torch.from_numpy(flow).to(dev), torch.from_numpy(match).to(dev), g["ae_XB"], g["ae_YB"], (wA, hA))
    wx, wy, wk = rule_sample(flow[0], match[0, :, :, 0], xb, yb, (wA, hA))
    assert xa.is_cuda and keep.dtype == torch.bool and torch.equal(keep.cpu(), torch.from_numpy(wk)) and int(keep.sum()) == 22
    assert torch.equal(xa.cpu().view(torch.int32), torch.from_numpy(wx.view(np.int32)))
    assert torch.equal(ya.cpu().view(torch.int32), torch.from_numpy(wy.view(np.int32)))
    args = (wB, hB, wA, hA, g["ae_XA"], g["ae_YA"], g["ae_XB"], g["ae_YB"])
    for mm, counts_key, nb_key in ((match, "ae_counts", "ae_nb"), (match * np.float32(0.5), "ae_none_counts", "ae_none_nb")):
        for to_dev in (False, True):                               # arrays as the script loads them, or tensors of corr_getFlow
            fl, ma = (torch.from_numpy(flow).to(dev), torch.from_numpy(mm).to(dev)) if to_dev else (flow, mm)
            counts, nb = assemble.corr_alignment_error(*args, fl, ma, g["ae_grid"])
            assert nb == int(g[nb_key]) and np.array_equal(counts, g[counts_key]) and counts.dtype == g[counts_key].dtype
            assert np.array_equal(counts, rule_alignment_error(*args, flow, mm, g["ae_grid"])[0])
    # flows whose sum with 1 is inexact, every pixel of a map as a keypoint
    rng = np.random.RandomState(2)
    H, W = 21, 35
    f, m = _flow(rng, (H, W)), rng.rand(H, W).astype(np.float32)
    m[0, :8] = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1)), 0, 1, np.nan, np.inf, -1, 0.75
    yy, xx = np.mgrid[0:H, 0:W]
    for sizeA in ((2, 640), (1920, 4096), (301, 200)):
        got = ops.sample_points(torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev), xx.ravel(), yy.ravel() + 0.75, sizeA)
        want = rule_sample(f, m, xx.ravel(), yy.ravel(), sizeA)
        assert torch.equal(got[2].cpu(), torch.from_numpy(want[2]))
        for k in range(2):
            assert torch.equal(got[k].cpu().view(torch.int32), torch.from_numpy(want[k].view(np.int32)))
    # a keypoint outside the map: a bad argument, found on the host; no keypoints: empty results
    for bad in (([W], [0]), ([0], [H]), ([-1], [0]), ([0], [-1.5])):
        with pytest.raises(_lib.RfxError, match="bad argument"):
            ops.sample_points(torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev), bad[0], bad[1], (640, 480))
    e = ops.sample_points(torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev), [], [], (640, 480))
    assert [tuple(t.shape) for t in e] == [(0,)] * 3


def _assembly_case():
    g = golden()["raw"]
    n, hd, wd = int(g["n"]), int(g["hd"]), int(g["wd"])
    fd, _, pm, md = synth.assembly_arrays(int(g["seed"]), n, hd, wd)
    return fd, pm, md, golden()["bg"], (hd * 8, wd * 8)


def test_assemble_yfcc_and_yfcc_matches(dev):
    """assemble_yfcc is assemble(..., cycle=True) with the background mask ANDed in; yfcc_matches on the device's OWN maps is the
    rule applied to those maps copied to the host (not a CPU assembly: its threshold ties differ)."""
    fd, pm, md, bg, (H, W) = _assembly_case()
    for th, multiH in ((0.5, True), (0.95, True), (0.5, False)):
        fg, binary = assemble.assemble_yfcc(fd, pm, md, bg, th, multiH, device=dev)
        wf, _, wb = assemble.assemble(fd, pm, md, (H, W), th, multiH, True, dev)
        assert tuple(fg.shape) == (1, H, W, 2) and tuple(binary.shape) == (1, H, W) and binary.dtype == torch.bool
        assert torch.equal(fg, wf) and torch.equal(binary, wb & torch.from_numpy(bg).to(dev)[None])
        assert 0 < int(binary.sum()) < int(wb.sum())
        fg2, binary2 = assemble.assemble_yfcc(fd, pm, md, torch.from_numpy(bg.astype(np.float32)).to(dev), th, multiH, device=dev)
        assert torch.equal(fg2, fg) and torch.equal(binary2, binary)
        hf, hb = fg.cpu().numpy(), binary.cpu().numpy()
        for angle, sizeA in zip((0, 90, 180, 270), ((640, 480), (1920, 1080), (97, 211), (4096, 2))):
            sizeB = _size_b((H, W), angle // 90)
            pts1, pts2 = assemble.yfcc_matches(fg, binary, sizeA, sizeB, angle)
            w1, w2, _ = rule_points(hf, hb, sizeA, sizeB, angle)
            assert pts1.is_cuda and torch.equal(pts2.cpu(), torch.from_numpy(w2))
            assert torch.equal(pts1.cpu().view(torch.int32), torch.from_numpy(w1.view(np.int32)))
        with pytest.raises(ValueError, match="do not fit"):
            assemble.yfcc_matches(fg, binary, (640, 480), (W, H), 90)


def test_file_level_entries_and_the_dropin_namespace(dev, tmp_path):
    """yfcc_getFlow reads the script's files (the ([], []) sentinel when the pair has none); getResults.yfcc.* take the reference's
    argument lists and return numpy arrays of the reference's dtypes."""
    fd, pm, md, bg, (H, W) = _assembly_case()
    fine, coarse, maskp = (str(tmp_path / x) for x in ("fine", "coarse", "mask"))
    for d in (fine, coarse, maskp):
        os.makedirs(d)
    np.save(os.path.join(fine, "flow_7_3H.npy"), fd)
    np.save(os.path.join(coarse, "flow_7_3H.npy"), pm)
    np.save(os.path.join(fine, "mask_7_3H.npy"), md)
    np.save(os.path.join(maskp, "maskBG_7_3H.npy"), bg)
    names = os.listdir(fine)
    assert assemble.yfcc_getFlow(8, fine, names, coarse, maskp, True, 0.5, device=dev) == ([], [])
    fg, binary = assemble.yfcc_getFlow(7, fine, names, coarse, maskp, True, 0.5, device=dev)
    wf, wb = assemble.assemble_yfcc(fd, pm, md, bg, 0.5, True, device=dev)
    assert torch.equal(fg, wf) and torch.equal(binary, wb)
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    assert getResults.yfcc.getFlow(8, fine, names, coarse, maskp, True, 0.5) == ([], [])
    f, b = getResults.yfcc.getFlow(7, fine, names, coarse, maskp, True, 0.5)
    assert isinstance(f, np.ndarray) and f.dtype == np.float32 and f.shape == (H, W, 2)
    assert isinstance(b, np.ndarray) and b.dtype == bool and b.shape == (H, W)
    assert np.array_equal(f, wf[0].cpu().numpy()) and np.array_equal(b, wb[0].cpu().numpy())
    f2, b2 = getResults.yfcc._getFlow(torch.from_numpy(fd), torch.from_numpy(pm), torch.from_numpy(md), bg, True, 0.5)   # multiH, th
    assert np.array_equal(f2, f) and np.array_equal(b2, b) and f2.dtype == np.float32 and b2.dtype == bool
    pts1, pts2 = getResults.yfcc.matches_from_flow(f, b, (640, 480), (H, W), 270)
    w1, w2, _ = rule_points(f[None], b[None], (640, 480), (H, W), 270)
    assert isinstance(pts1, np.ndarray) and pts1.dtype == np.float32 and isinstance(pts2, np.ndarray) and pts2.dtype == np.int64
    assert np.array_equal(pts1.view(np.int32), w1.view(np.int32)) and np.array_equal(pts2, w2)
    pts1f, pts2f = getResults.yfcc.matches_from_flow(f, b.astype(np.float32), (640, 480), (H, W), 270)      # a float mask, as astype('bool')
    assert np.array_equal(pts1f, pts1) and np.array_equal(pts2f, pts2)
    g = golden()["raw"]
    wB, hB, wA, hA = (int(v) for v in g["ae_dims"])
    counts, nb = getResults.corr.alignmentError(wB, hB, wA, hA, g["ae_XA"], g["ae_YA"], g["ae_XB"], g["ae_YB"],
                                                torch.from_numpy(g["ae_flow"]), torch.from_numpy(g["ae_match"]), g["ae_grid"])
    assert nb == int(g["ae_nb"]) and np.array_equal(counts, g["ae_counts"])


def test_variant_c_result_to_correspondences_without_a_host_copy(dev):
    """One multi_h_variant_c result on a small synthetic pair: its device lists go through assemble_yfcc and yfcc_matches as they
    are; the points equal the rule applied to the assembled maps."""
    from rfx import weights
    from rfx.pipeline import AlignPipeline
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    I1, I2 = synth.make_pair(128, 160, seed=0)
    pipe = AlignPipeline(sds, nbScale=3, nbIter=200, tolerance=0.05, minSize=160, scaleR=1.2, variant="C", device=dev)
    up = lambda im: torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)[None]).to(dev)
    torch.manual_seed(5)
    res = pipe.multi_h_variant_c(up(I1), [up(I2)], maxCoarse=2)[0]
    assert res["nbH"] >= 1
    flowDown, matchDown, param = torch.cat(res["flowDown8"]), torch.cat(res["matchDown8"]), torch.stack(res["H"])
    assert flowDown.is_cuda and param.is_cuda and tuple(param.shape) == (res["nbH"], 3, 3)
    h, w = flowDown.shape[2:]
    bg = torch.ones(8 * h, 8 * w, dtype=torch.bool, device=dev)
    bg[:, :5] = False
    fg, binary = assemble.assemble_yfcc(flowDown, param, matchDown, bg, 0.5, True, device=dev)
    pts1, pts2 = assemble.yfcc_matches(fg, binary, I1.size, (8 * w, 8 * h), 0)
    w1, w2, _ = rule_points(fg.cpu().numpy(), binary.cpu().numpy(), I1.size, (8 * w, 8 * h), 0)
    assert pts1.is_cuda and pts2.is_cuda and not binary[0, :, :5].any()
    assert torch.equal(pts2.cpu(), torch.from_numpy(w2)) and torch.equal(pts1.cpu().view(torch.int32), torch.from_numpy(w1.view(np.int32)))
