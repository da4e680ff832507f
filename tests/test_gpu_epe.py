"""The end-point error of an assembled flow on the device (csrc/epe.hip: rfx_epe_homography_f32, rfx_epe_flow_f32; ops.epe_homography
/ epe_flow; assemble.hpatch_epe / kitti_epe) against the rule stated in numpy in tests/test_epe_cpu.py, which that file pins to the
reference's own outputs.  The per-pixel error is compared as bit patterns, NaN placement included, and the count exactly.  A sum
may differ from the exact sum of those errors (math.fsum) by what ANY order of count - 1 float64 additions of non-negative numbers
can lose, (count - 1) * 2^-53 * sum, and must have the same bits in every run and at every position of a batch."""
import os
import sys

import numpy as np
import pytest
import torch

from rfx import assemble, ops, synth
from test_epe_cpu import (TILE, bits, flow_est_for, fsum_of, golden, rule_epe_flow, rule_epe_homography, rule_grid_gt, rule_lin,
                          ulp32)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
U = 2.0 ** -53


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_sums(total, count, werr, wcount, what):
    """count equal; |sum - fsum(err)| <= (count - 1) * 2^-53 * fsum per map; an empty map sums to +0.0, a single counted pixel to its
    own error exactly."""
    total, count = total.cpu().numpy().reshape(-1), count.cpu().numpy().reshape(-1)
    assert total.dtype == f64 and count.dtype == np.int32
    assert np.array_equal(count, wcount.astype(np.int32)), what
    for n in range(len(total)):
        fs, c = fsum_of(werr[n])
        assert c == count[n]
        assert abs(float(total[n]) - fs) <= max(c - 1, 0) * U * fs, (what, n, float(total[n]), fs, c)
        if c == 0:
            assert bits(total[n:n + 1])[0] == 0, (what, n)
        if c == 1:
            assert float(total[n]) == float(werr[n][~np.isnan(werr[n])][0]), (what, n)


def _hom(flow, Hinv, dev, what):
    """One batch through ops.epe_homography, with and without the error map."""
    f, h = _up(flow, dev), _up(np.asarray(Hinv, f64).reshape(len(flow), 9), dev)
    total, count, err = ops.epe_homography(f, h, want_err=True)
    werr, wcount = rule_epe_homography(flow, Hinv)
    assert total.is_cuda and count.is_cuda and err.is_cuda and err.dtype == torch.float32 and tuple(err.shape) == flow.shape[:3]
    got = err.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(werr)), what
    assert np.array_equal(bits(got), bits(werr)), (what, int((bits(got) != bits(werr)).sum()))
    _check_sums(total, count, werr, wcount, what)
    t2, c2 = ops.epe_homography(f, h.reshape(-1, 3, 3))
    assert torch.equal(t2.view(torch.int64), total.view(torch.int64)) and torch.equal(c2, count), what
    return total, count


def _flo(flow, u, v, valid, dev, what):
    """One batch through ops.epe_flow, with and without the error map; the average against the script's own sum over error * valid."""
    f, uu, vv, m = _up(flow, dev), _up(u, dev), _up(v, dev), _up(valid, dev)
    total, count, err = ops.epe_flow(f, uu, vv, m, want_err=True)
    werr, wcount = rule_epe_flow(flow, u, v, valid)
    assert total.is_cuda and count.is_cuda and err.is_cuda and err.dtype == torch.float64 and tuple(err.shape) == flow.shape[:3]
    got = err.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(werr)), what
    assert np.array_equal(bits(got), bits(werr)), (what, int((bits(got) != bits(werr)).sum()))
    _check_sums(total, count, werr, wcount, what)
    t2, c2 = ops.epe_flow(f, uu, vv, m)
    assert torch.equal(t2.view(torch.int64), total.view(torch.int64)) and torch.equal(c2, count), what
    for n in range(len(flow)):                                         # evaluation/evalKITTI/getResults.py:228, numpy's own summation
        c = int(wcount[n])
        if c:
            ref = np.sum(np.nan_to_num(werr[n]) * (valid[n] != 0)) / np.sum(valid[n] != 0)
            assert abs(float(total[n]) / c - ref) <= 2 * (c - 1) * U * ref, (what, n)
    return total, count


def _perspective(rng, Sh, Sw):
    """An inverse homography in pixel units that keeps part of a Sh x Sw map inside."""
    return np.array([[1 + 0.2 * rng.randn(), 0.2 * rng.randn(), 0.3 * Sw * rng.randn()],
                     [0.2 * rng.randn(), 1 + 0.2 * rng.randn(), 0.3 * Sh * rng.randn()],
                     [0.3 * rng.randn() / Sw, 0.3 * rng.randn() / Sh, 1]], f64).reshape(9)


def _away(Sh, Sw):
    """Every pixel maps far outside."""
    return np.array([1, 0, 10.0 * Sw, 0, 1, 10.0 * Sh, 0, 0, 1], f64)


def _flow(rng, shape):
    """Estimates in [-1.1, 1.1) formed in float64: their sums with 1 are inexact, every float32 step of the rule rounds."""
    return (rng.rand(*shape, 2) * 2.2 - 1.1).astype(f32)


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.int64), b.reshape(-1).view(torch.int64))


def test_goldens_through_the_device(dev):
    """Every case of tests/golden/epe.npz: the error map of the seeded estimate equals the rule's; the average that assemble.hpatch_epe
    returns is the reference's float32 mean up to the two roundings of the same exact value."""
    G = golden()
    alone = []
    for c in G:
        S = c["S"]
        est = flow_est_for(c["seed"], S)
        total, count = _hom(est[None], c["Hinv"][None], dev, "golden %s S = %d" % (c["kind"], S))
        assert int(count[0]) == c["inside"]
        alone.append(total[0])
        werr, _ = rule_epe_homography(est[None], c["Hinv"][None])
        fs, n = fsum_of(werr)
        exact = fs / n
        for aepe in (assemble.hpatch_epe(_up(est[None], dev), c["Hinv"].reshape(3, 3)),
                     assemble.hpatch_epe(_up(est, dev), _up(c["Hinv"], dev).reshape(3, 3))):
            assert isinstance(aepe, float) and aepe == float(f32(float(total[0]) / n))
            assert abs(aepe - float(c["aepe"])) <= abs(float(c["aepe"]) - exact) + ulp32(exact), (c["kind"], S, aepe, float(c["aepe"]))
    # the cases of one size as ONE batch: each map's sum has the bits it has alone; hpatch_epe returns a list
    for S in (17, 24, 33):
        idx = [i for i, c in enumerate(G) if c["S"] == S]
        est = np.stack([flow_est_for(G[i]["seed"], S) for i in idx])
        Hinv = np.stack([G[i]["Hinv"] for i in idx])
        total, _ = _hom(est, Hinv, dev, "golden batch S = %d" % S)
        for k, i in enumerate(idx):
            assert _same_bits(total[k], alone[i]), (S, k)
        lst = assemble.hpatch_epe(_up(est, dev), Hinv.reshape(-1, 3, 3))
        assert isinstance(lst, list) and len(lst) == len(idx)
        assert lst == [float(f32(float(alone[i]) / G[i]["inside"])) for i in idx]


# 63, 64, 65, 1023, 1024, 1025 and 4097 pixels as maps with at least two rows and columns (the rule divides by size - 1: a map of one
# pixel, or one row, is refused -- the flow form below takes those)
HOM_SHAPES = [(7, 9), (2, 32), (5, 13), (3, 341), (2, 512), (32, 32), (5, 205), (17, 241)]


@pytest.mark.parametrize("shape", HOM_SHAPES + [(w, h) for h, w in HOM_SHAPES if h != w], ids=lambda s: "%dx%d" % s)
def test_homography_tile_and_wavefront_edges(dev, shape):
    """Maps whose size sits on, one below and one above a wavefront (64), a tile (1024) and four tiles, both orientations: the
    identity (everything inside), a map with nothing inside, seeded perspective ones -- alone and as one batch."""
    assert TILE == 1024
    Sh, Sw = shape
    rng = np.random.RandomState(Sh * 10007 + Sw)
    Hinv = np.stack([np.eye(3).reshape(9), _away(Sh, Sw)] + [_perspective(rng, Sh, Sw) for _ in range(3)])
    flow = _flow(rng, (len(Hinv), Sh, Sw))
    total, count = _hom(flow, Hinv, dev, "%dx%d batch" % shape)
    assert int(count[0]) == Sh * Sw and int(count[1]) == 0 and 0 < int(count[2:].sum()) < 3 * Sh * Sw
    for n in range(len(Hinv)):
        t1, c1 = _hom(flow[n:n + 1], Hinv[n:n + 1], dev, "%dx%d map %d alone" % (Sh, Sw, n))
        assert _same_bits(t1, total[n]) and int(c1[0]) == int(count[n])


def _valids(n, rng):
    p = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": p == 0, "last": p == n - 1,
            "beside multiples of 64": (p % 64 == 0) | (p % 64 == 63), "p = 0.5": rng.rand(n) < 0.5}


def _kitti_like(rng, N, H, W):
    """A flow near the identity grid, ground truth on KITTI's grid of 1/64 pixel."""
    grid = np.stack(np.broadcast_arrays(rule_lin(W)[None, :], rule_lin(H)[:, None]), axis=2).astype(f32)
    flow = (grid[None] + rng.randn(N, H, W, 2) * 0.05).astype(f32)
    u = ((rng.randint(0, 65536, (N, H, W)) - 32768) / 64.0 / 128).astype(f32)     # exact: multiples of 2^-13 below 4
    v = ((rng.randint(0, 65536, (N, H, W)) - 32768) / 64.0).astype(f32)
    return flow, u, v


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 4097))
def test_flow_tile_and_wavefront_edges(dev, n):
    """Maps of n pixels as one row and as one column; valid all-true, all-false, first-only, last-only, beside every multiple of 64
    and seeded -- as one batch and each alone.  A single valid pixel makes sum that pixel's error exactly (_check_sums)."""
    rng = np.random.RandomState(n)
    fam = _valids(n, rng)
    for H, W in ((1, n), (n, 1)):
        flow, u, v = _kitti_like(rng, len(fam), H, W)
        valid = np.stack([m.reshape(H, W) for m in fam.values()])
        total, count = _flo(flow, u, v, valid, dev, "%dx%d batch" % (H, W))
        assert int(count[0]) == n and int(count[1]) == 0 and int(count[2]) == int(count[3]) == 1
        for k, name in enumerate(fam):
            m8 = valid[k:k + 1].astype(np.uint8) * 7                   # bytes: any non-zero value counts
            t1, c1 = _flo(flow[k:k + 1], u[k:k + 1], v[k:k + 1], m8, dev, "%dx%d %s" % (H, W, name))
            assert _same_bits(t1, total[k]) and int(c1[0]) == int(count[k]), name


def test_flow_two_dimensional_maps_and_float32_steps(dev):
    """Non-square maps of several tiles, the last one short; flows on which a fused, reordered or double-precision form of
    ((f - lin) * (size - 1)) / 2 differs from the float32 steps."""
    rng = np.random.RandomState(4)
    N, H, W = 4, 37, 83
    flow, u, v = _kitti_like(rng, N, H, W)
    valid = rng.rand(N, H, W) < 0.6
    valid[1], valid[2] = False, True
    total, count = _flo(flow, u, v, valid, dev, "37x83")
    assert int(count[1]) == 0 and int(count[2]) == H * W
    again, _ = ops.epe_flow(_up(flow, dev), _up(u, dev), _up(v, dev), _up(valid, dev))
    assert _same_bits(again, total)
    werr, _ = rule_epe_flow(flow, u, v, valid)
    once = (flow[..., 0].astype(f64) - rule_lin(W).astype(f64)[None, None, :]) * (W - 1) / 2
    e64 = np.sqrt((once - u) ** 2 + ((flow[..., 1].astype(f64) - rule_lin(H).astype(f64)[None, :, None]) * (H - 1) / 2 - v) ** 2)
    assert (e64[valid] != werr[valid]).any()                           # the inputs do tell float64 steps from float32 steps
    # single maps: 0-dim results
    t0, c0, e0 = ops.epe_flow(_up(flow[0], dev), _up(u[0], dev), _up(v[0], dev), _up(valid[0], dev), want_err=True)
    assert t0.dim() == 0 and c0.dim() == 0 and tuple(e0.shape) == (H, W) and _same_bits(t0, total[0])


def test_pixels_at_equality_and_beside_it(dev):
    """Equality counts as inside: the identity's border sits AT -1 and 1.  Then the float32 values next to -1 and 1 that the rule's
    last step, q - 1, can produce (q has half the resolution above 2 that 1 has: 1 + 2^-22 is the first value past 1), each as the
    coordinate of EVERY pixel of a 5 x 5 map, once in x and once in y."""
    for S in (2, 3, 9, 240):
        total, count = _hom(_flow(np.random.RandomState(S), (1, S, S)), np.eye(3).reshape(1, 9), dev, "identity %d" % S)
        assert int(count[0]) == S * S
    m1, p1 = f32(-1), f32(1)
    # q -> (the coordinate q - 1, inside?)
    cases = [(2.0 ** -24, np.nextafter(m1, f32(0)), True), (0.0, m1, True), (-2.0 ** -24, m1, True),      # -1 - 2^-24 ties to -1
             (-2.0 ** -23, np.nextafter(m1, f32(-2)), False), (2 - 2.0 ** -23, p1 - f32(2.0 ** -23), True), (2.0, p1, True),
             (2 + 2.0 ** -22, p1 + f32(2.0 ** -22), False), (1.0, f32(0), True)]
    Hinv, want = [], []
    for q, coord, inside in cases:
        # S - 1 = 4: x' = 2 q, ((2 x') / 1) / 4 = q exactly; the other coordinate sits at 0
        Hinv.append([0, 0, 2 * q, 0, 0, 2, 0, 0, 1])
        Hinv.append([0, 0, 2, 0, 0, 2 * q, 0, 0, 1])
        want += [inside, inside]
        gx, gy = rule_grid_gt(Hinv[-2], 5, 5)
        assert gx[2, 3] == coord and bits(gx[2:3, 3])[0] == bits(np.asarray([coord], f32))[0] and gy[2, 3] == 0, q
        gx, gy = rule_grid_gt(Hinv[-1], 5, 5)
        assert gy[2, 3] == coord and gx[2, 3] == 0, q
    Hinv = np.asarray(Hinv, f64)
    total, count = _hom(_flow(np.random.RandomState(1), (len(Hinv), 5, 5)), Hinv, dev, "beside +-1")
    assert count.cpu().tolist() == [25 if w else 0 for w in want]
    # a denominator of exactly 0, and NaN entries: outside, the sum stays +0.0
    bad = np.array([[1, 0, 0, 0, 1, 0, 0, 0, -float(f32(1e-8))], [np.nan, 0, 0, 0, 1, 0, 0, 0, 1]], f64)
    total, count = _hom(_flow(np.random.RandomState(2), (2, 5, 5)), bad, dev, "degenerate")
    assert count.cpu().tolist() == [0, 0]


def test_batch_with_an_empty_and_a_full_map(dev):
    """Five maps of three tiles each, the last tile short: map 0 full, map 1 empty.  Every map's sum is bit-equal to the map alone,
    to a second run, and to the map at another position of another batch."""
    rng = np.random.RandomState(3)
    N, Sh, Sw = 5, 37, 83
    Hinv = np.stack([np.eye(3).reshape(9), _away(Sh, Sw)] + [_perspective(rng, Sh, Sw) for _ in range(3)])
    flow = _flow(rng, (N, Sh, Sw))
    total, count = _hom(flow, Hinv, dev, "37x83 batch")
    assert int(count[0]) == Sh * Sw and int(count[1]) == 0 and all(0 < int(c) < Sh * Sw for c in count[2:])
    again, _ = ops.epe_homography(_up(flow, dev), _up(Hinv, dev))
    assert _same_bits(again, total)
    order = [3, 1, 4, 0, 2, 3]
    moved, _ = ops.epe_homography(_up(flow[order], dev), _up(Hinv[order], dev))
    assert _same_bits(moved, total[order])
    for n in range(N):
        t1, c1, e1 = ops.epe_homography(_up(flow[n], dev), _up(Hinv[n], dev).reshape(3, 3), want_err=True)
        assert t1.dim() == 0 and c1.dim() == 0 and tuple(e1.shape) == (Sh, Sw) and _same_bits(t1, total[n]) and int(c1) == int(count[n])


def test_more_tiles_than_any_grid(dev):
    """9000 maps of 2 x 3 (3 x 2): one tile each, more tiles than the launch's 8192 workgroups -- they stride, as the wavefronts of the
    finishing launch do over the maps."""
    rng = np.random.RandomState(9)
    N = 9000
    Hinv = np.stack([_perspective(rng, 2, 3) for _ in range(N)])
    flow = _flow(rng, (N, 2, 3))
    total, count = _hom(flow, Hinv, dev, "9000 maps")
    assert 0 < int((count == 0).sum()) < N and int(count.max()) == 6
    t8, _ = ops.epe_homography(_up(flow[8191:8193], dev), _up(Hinv[8191:8193], dev))
    assert _same_bits(t8, total[8191:8193])
    _hom(flow.reshape(N, 3, 2, 2), Hinv, dev, "9000 maps, 3 x 2")
    kf, u, v = _kitti_like(rng, N, 2, 3)
    valid = rng.rand(N, 2, 3) < 0.5
    total, count = _flo(kf, u, v, valid, dev, "9000 maps, flow form")
    t8, _ = ops.epe_flow(_up(kf[8999:], dev), _up(u[8999:], dev), _up(v[8999:], dev), _up(valid[8999:], dev))
    assert _same_bits(t8, total[8999:])


def test_refusals_raise_before_any_launch(dev):
    f, h = torch.zeros(6, 8, 2, device=dev), torch.eye(3, dtype=torch.float64, device=dev)
    u, m = torch.zeros(6, 8, device=dev), torch.ones(6, 8, dtype=torch.bool, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epe_homography(f, h.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epe_flow(f, u, u.cpu(), m)
    with pytest.raises(TypeError):
        ops.epe_homography(f, h.float())                              # Hinv is float64: nine numbers carry the whole ground truth
    with pytest.raises(TypeError):
        ops.epe_flow(f, u.double(), u, m)
    for bad in ((f, h[None]), (f[None], h), (f[:1], h), (f[:, :1], h), (torch.zeros(6, 8, 3, device=dev), h)):
        with pytest.raises(ValueError):
            ops.epe_homography(*bad)
    for bad in ((f, u[:5], u, m), (f, u, u, m[:, :7]), (f[None], u, u, m)):
        with pytest.raises(ValueError):
            ops.epe_flow(*bad)
    t, c = ops.epe_homography(f, h)                                    # and the well-formed call goes through
    assert t.is_cuda and int(c) == 48


def test_assembled_flow_to_the_hpatches_number_without_a_host_copy(dev):
    """assemble.assemble(...) -> hpatch_epe with device tensors only: the number is float32(sum / count) of the rule applied to the
    assembled map copied to the host.  The drop-in's attribute is the same function; a pair without a saved flow is the identity."""
    S, n = 48, 3
    fd, _, pm, md = synth.assembly_arrays(51, n, S // 8, S // 8)
    flow_est = assemble.assemble(fd, pm, md, (S, S), 0.5, True, False, dev)[0]
    assert flow_est.is_cuda and tuple(flow_est.shape) == (1, S, S, 2)
    H = np.array([[0.9, 0.08, 25.0], [-0.05, 1.1, -18.0], [1e-4, -5e-5, 1.0]])
    Hs, Hinv = assemble.hpatch_gt_homography(H, (480, 640), (600, 800), S)
    aepe = assemble.hpatch_epe(flow_est, Hinv)
    werr, wcount = rule_epe_homography(flow_est.cpu().numpy(), Hinv.reshape(1, 9))
    fs, c = fsum_of(werr)
    assert S * S / 4 < c < S * S and isinstance(aepe, float)
    total, count = ops.epe_homography(flow_est, _up(Hinv.reshape(1, 9), dev))
    _check_sums(total, count, werr, wcount, "assembled")
    assert aepe == float(f32(float(total[0]) / c)) and abs(aepe - fs / c) <= ulp32(fs / c)
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    assert getResults.hpatch.epe_from_homography(flow_est.cpu(), Hinv) == aepe       # the drop-in's getFlow_all returns CPU tensors
    ident = assemble.identity_grid(S, S, dev)
    grid = np.stack(np.broadcast_arrays(rule_lin(S)[None, :], rule_lin(S)[:, None]), axis=2).astype(f32)
    assert np.array_equal(bits(ident[0].cpu().numpy()), bits(grid))
    assert assemble.hpatch_epe([], Hinv, size=S) == assemble.hpatch_epe(ident, Hinv)
    assert np.isnan(assemble.hpatch_epe(flow_est, _away(S, S).reshape(3, 3)))        # nothing inside: the mean of nothing


def test_assembled_flow_to_the_kitti_number_without_a_host_copy(dev):
    """assemble_kitti(fill="device", interpolate=True) -> kitti_epe with the flow on the device throughout: the number is the
    script's sum(error * valid) / sum(valid) on the assembled map copied to the host, up to the order of the float64 additions."""
    n, hd, wd = 3, 6, 10
    H, W = hd * 8, wd * 8
    fd, fd2, pm, md = synth.assembly_arrays(52, n, hd, wd)
    fg = assemble.assemble_kitti(fd2, fd, pm, md, (H, W), 0.5, True, 0.0, True, dev, fill="device")[0]
    assert fg.is_cuda and tuple(fg.shape) == (1, H, W, 2)
    rng = np.random.RandomState(6)
    u = (rng.randint(0, 65536, (H, W)).astype(float) - 32768) / 64.0 / 256            # float64, as readFlow returns them
    v = (rng.randint(0, 65536, (H, W)).astype(float) - 32768) / 64.0 / 256
    valid = rng.rand(H, W) < 0.3
    got = assemble.kitti_epe(fg, u, v, valid)
    werr, wcount = rule_epe_flow(fg.cpu().numpy(), u[None].astype(f32), v[None].astype(f32), valid[None])
    c = int(wcount[0])
    ref = np.sum(np.nan_to_num(werr[0]) * valid) / np.sum(valid)
    assert isinstance(got, float) and 0 < c < H * W and abs(got - ref) <= 2 * (c - 1) * U * ref
    total, count = ops.epe_flow(fg, _up(u[None].astype(f32), dev), _up(v[None].astype(f32), dev), _up(valid[None], dev))
    assert got == float(total[0]) / c
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    assert getResults.kitti.epe(fg.cpu(), u, v, valid) == got
    assert np.isnan(assemble.kitti_epe(fg, u, v, np.zeros((H, W), bool)))               # nothing valid: 0 / 0
    # a pair without prediction: the identity grid, whose flow is 0 -- the error is the length of the ground truth
    zero = assemble.kitti_epe([], u, v, valid)
    want = np.sum(np.sqrt(u * u + v * v) * valid) / np.sum(valid)
    assert abs(zero - want) <= 2 * (c - 1) * U * want
    lst = assemble.kitti_epe(torch.cat((fg, fg)), np.stack((u, u)), np.stack((v, v)), np.stack((valid, valid)))
    assert lst == [got, got]
