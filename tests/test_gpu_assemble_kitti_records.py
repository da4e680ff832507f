"""The KITTI flow assembly of a whole batch from its device records (ops.assemble_kitti_records: rfx_assemble_kitti_records_f32, with a
component filter also rfx_kitti_scores_records_f32 and rfx_remove_small_cc_ragged_f32; assemble.assemble_kitti_records) against the
per-pair chain assemble.assemble_kitti(..., fill="device") on the record's first nbH entries (tests/test_gpu_assemble.py holds that
chain to the reference): all three maps as BIT PATTERNS, NaN payloads included.  Entries of a record past nbH are filled with NaN
here, so a kernel that read one would show."""
import os

import numpy as np
import pytest
import torch

import assemble_explained as ae
from rfx import assemble, ops, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-4
NAN = float("nan")


# ---------------------------------------------------------------- helpers

def _bits(a, b):
    """Same shape, dtype and bit pattern (float32 compared as int32: -0.0 != 0.0, a NaN equals only the same NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


def _next(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _random_pair(g, n, hd, wd, hd2, wd2, flow_amp=0.3, h_amp=0.12):
    """(flowD2, flowDown8, H, matchDown8) of one pair: flows large enough to push sampling points beyond [-1,1] near the border at
    both levels, homographies that move part of the image out of bounds, matchability in [0,1]."""
    fd2 = torch.randn(n, 2, hd2, wd2, generator=g) * flow_amp
    fd = torch.randn(n, 2, hd, wd, generator=g) * flow_amp
    pm = torch.eye(3)[None].repeat(n, 1, 1) + h_amp * torch.randn(n, 3, 3, generator=g)
    pm[:, :2, 2] += torch.rand(n, 2, generator=g) - 0.5
    md = torch.rand(n, 2, hd, wd, generator=g)
    return fd2, fd, pm, md


def _fill(views, pair, dev):
    """Write one pair's arrays (or None: no homography) into its record views; the entries past nbH become NaN."""
    nbH, Hs, f8, m8, d2 = views
    Hs.fill_(NAN), f8.fill_(NAN), m8.fill_(NAN), d2.fill_(NAN)
    n = 0 if pair is None else pair[0].shape[0]
    if n:
        d2[:n], f8[:n], Hs[:n], m8[:n] = (t.to(dev) for t in pair)
    nbH.fill_(float(n))


def _dense(pairs, hd, wd, hd2, wd2, dev, max_h=11):
    R = ops.MultiHRecords(len(pairs), hd, wd, dev, max_h=max_h, hd2=hd2, wd2=wd2)
    nbH, _, Hs, f8, m8, d2 = R.views()
    for b, pair in enumerate(pairs):
        _fill((nbH[b], Hs[b], f8[b], m8[b], d2[b]), pair, dev)
    return R


def _ragged(pairs, dev, max_h=11):
    R = ops.MultiHRecordsRagged([p[1].shape[2] for p in pairs], [p[1].shape[3] for p in pairs], dev, max_h=max_h,
                                hd2_list=[p[0].shape[2] for p in pairs], wd2_list=[p[0].shape[3] for p in pairs])
    for b, pair in enumerate(pairs):
        nbH, _, Hs, f8, m8, d2 = R.views(b)
        _fill((nbH, Hs, f8, m8, d2), pair, dev)
    return R


def _chain(pair, out_hw, th, multiH, dev, cc_th=0.0, interpolate=False):
    """The yardstick: the per-pair chain on the pair's own arrays."""
    return assemble.assemble_kitti(*(t.to(dev) for t in pair), out_hw, th, multiH, cc_th, interpolate, dev, fill="device")


def _assert_pair(got, want, what):
    """got: (flow (H,W,2), match (H,W), binary (H,W)) of one pair; want: the chain's (1,H,W,2), (1,H,W), (1,H,W)."""
    for x, y, name in zip(got, want, ("flowGlobal", "matchGlobal", "binary")):
        assert _bits(x, y[0]), (what, name, int((x != y[0]).sum()))


def _assert_zero(fg, mg, b):
    assert not bool(fg.contiguous().view(torch.int32).any()) and not bool(mg.contiguous().view(torch.int32).any()) and not bool(b.any())


def _per_homography(pair, out_hw, dev, cc_th=0.0):
    """Per homography, from the chain's own kernels: flow_i (n,H,W,2), the score_i (n,H,W) the merge reads (filtered with cc_th > 0),
    the unfiltered score, and (flowUp, inb) of both levels."""
    d2d, fd, pm, md = (t.to(dev) for t in pair)
    H, W = out_hw
    d2, inb1, fup1 = ops.compose_flow(d2d, ops.warp_grid(pm, H, W), clamp=True, want_inb=True, want_flow_up=True)
    flow, inb, fup = ops.compose_flow(fd, d2, clamp=True, want_inb=True, want_flow_up=True)
    m = ops.resize_bilinear(md, (H, W), align_corners=False)
    raw = ops.match_score(m[:, 0], cyc=ops.grid_sample(m[:, 1:2].contiguous(), fup)[:, 0], inb=inb)
    return flow, (assemble.remove_small_cc(raw, cc_th) if cc_th else raw), raw, (fup1, inb1), (fup, inb)


def _restated(flow, score, th, multiH):
    """The merge restated on per-homography flows and scores: the first index that reaches th owns the pixel, else index 0."""
    ok = score >= th
    if not multiH:
        ok[1:] = False
    found = ok.any(0)
    owner = torch.where(found, ok.float().argmax(0), torch.zeros_like(found, dtype=torch.int64))
    fg = torch.gather(flow, 0, owner[None, :, :, None].expand(1, -1, -1, 2))[0]
    return torch.clamp(fg, -1, 1), torch.gather(score, 0, owner[None])[0], found


# ---------------------------------------------------------------- 1. dense records

HD, WD, HD2, WD2 = 4, 6, 2, 3
NBH = (1, 2, 11, 0)
TH1 = 0.15


@pytest.fixture(scope="module")
def dense_pairs():
    g = torch.Generator().manual_seed(201)
    return [_random_pair(g, n, HD, WD, HD2, WD2) if n else None for n in NBH]


def test_random_contents_reach_the_clamp_the_border_and_out_of_bounds_at_both_levels(dev, dense_pairs):
    flow, score, _, (fup1, inb1), (fup, inb) = _per_homography(dense_pairs[2], (32, 48), dev)
    for level, (u, i) in enumerate(((fup1, inb1), (fup, inb)), 1):
        assert bool((u.abs() == 1.0).any()), "no sampling point on the clamp at level %d" % level       # the border taps: masked corners
        assert bool((u.abs() < 1.0).all(3).any()) and bool((i == 0).any()) and bool((i == 1).any()), level
    assert bool(((score[0] < TH1) & (score[1:] >= TH1).any(0)).any()), "no pixel is owned by a homography i >= 1"
    assert bool((score[0] >= TH1).any())


@pytest.mark.parametrize("out_hw", [(32, 48), (27, 50), (3, 85), (1, 257)], ids=str)
@pytest.mark.parametrize("multiH", [False, True])
def test_dense_records_equal_the_chain_bit_for_bit(dev, dense_pairs, out_hw, multiH):
    R = _dense(dense_pairs, HD, WD, HD2, WD2, dev)
    fg, mg, b, valid = ops.assemble_kitti_records(R, TH1, multiH, out_hw=None if out_hw == (32, 48) else out_hw)
    assert fg.shape == (4,) + out_hw + (2,) and mg.shape == b.shape == (4,) + out_hw and b.dtype == torch.bool
    assert valid.tolist() == [True, True, True, False] and valid.device == fg.device
    for k, pair in enumerate(dense_pairs[:3]):
        _assert_pair((fg[k], mg[k], b[k]), _chain(pair, out_hw, TH1, multiH, dev), (k, out_hw, multiH))
    _assert_zero(fg[3], mg[3], b[3])
    assert bool(b[0].any()) and not bool(b[0].all())            # one homography: explained in part
    # the thin wrapper
    w = assemble.assemble_kitti_records(R, out_hw, TH1, multiH)
    assert all(_bits(x, y) for x, y in zip(w, (fg, mg, b, valid)))


# ---------------------------------------------------------------- 2. ragged records

RAGGED = ((5, 7, 3, 4, 2), (4, 6, 2, 3, 1), (2, 2, 1, 1, 3))    # (h8, w8, hd2, wd2, nbH): hd2 != h8 / 2


@pytest.mark.parametrize("sizes", [None, [(27, 50), (16, 16), (1, 257)]], ids=str)
def test_ragged_records_equal_the_chain_at_any_position(dev, sizes):
    g = torch.Generator().manual_seed(202)
    pairs = [_random_pair(g, n, h, w, h2, w2) for h, w, h2, w2, n in RAGGED]
    hw = sizes or [(8 * r[0], 8 * r[1]) for r in RAGGED]
    fg, mg, b, valid = ops.assemble_kitti_records(_ragged(pairs, dev), TH1, True, out_hw=sizes)
    assert valid.tolist() == [True] * 3 and [tuple(t.shape) for t in mg] == hw
    want = [_chain(p, s, TH1, True, dev) for p, s in zip(pairs, hw)]
    for k in range(3):
        _assert_pair((fg[k], mg[k], b[k]), want[k], ("ragged", k))
    order = [2, 0, 1]                                           # the same pairs at other positions of the batch
    fg2, mg2, b2, _ = ops.assemble_kitti_records(_ragged([pairs[k] for k in order], dev), TH1, True,
                                                 out_hw=None if sizes is None else [sizes[k] for k in order])
    for pos, k in enumerate(order):
        assert _bits(fg2[pos], fg[k]) and _bits(mg2[pos], mg[k]) and _bits(b2[pos], b[k]), (pos, k)
    # caller-owned packed buffers are filled in place; the views of one call share three buffers
    total = sum(h * w for h, w in hw)
    out = (torch.full((total, 2), NAN, device=dev), torch.full((total,), NAN, device=dev), torch.zeros(total, dtype=torch.bool, device=dev))
    fg3, mg3, b3, _ = ops.assemble_kitti_records(_ragged(pairs, dev), TH1, True, out_hw=sizes, out=out)
    assert fg3[0].data_ptr() == out[0].data_ptr() and mg3[2].data_ptr() == out[1].data_ptr() + 4 * (total - hw[2][0] * hw[2][1])
    assert all(_bits(fg3[k], fg[k]) and _bits(mg3[k], mg[k]) and _bits(b3[k], b[k]) for k in range(3))
    assert fg[1].data_ptr() == fg[0].data_ptr() + 8 * hw[0][0] * hw[0][1] and b[1].data_ptr() == b[0].data_ptr() + hw[0][0] * hw[0][1]


# ---------------------------------------------------------------- 3. the component filter

def _plateau_pair(hd, wd, hd2, wd2, blocks0, blocks1):
    """An exact-operand family: matchability 1->2 of zeros and ones, 2->1 all ones, zero residual flows at both levels, homography 0
    the identity and 1 the identity moved by 1/64.  The score of a pixel is above 0.99 exactly where all four /8 cells under it hold
    a one (one cell of zero weighs at least 1/16), so an interior block of cells rows r0..r1 x columns c0..c1 is ONE plateau of
    8 (r1 - r0) x 8 (c1 - c0) pixels, rows 8 r0 + 4 .. 8 r1 + 3; the plateaus stay in bounds.  blocks0 / blocks1: the blocks
    (r0, r1, c0, c1) of homographies 0 and 1."""
    md = torch.zeros(2, 2, hd, wd)
    md[:, 1] = 1.0
    for i, blocks in enumerate((blocks0, blocks1)):
        for r0, r1, c0, c1 in blocks:
            md[i, 0, r0:r1 + 1, c0:c1 + 1] = 1.0
    pm = torch.eye(3)[None].repeat(2, 1, 1)
    pm[1, 0, 2] = 1.0 / 64
    return torch.zeros(2, 2, hd2, wd2), torch.zeros(2, 2, hd, wd), pm, md


def _whole_pair(hd, wd, hd2, wd2):
    """One identity homography whose only component is the whole map: match12 all ones and match21 all FOUR -- the sampling points of
    the border pixels lie half outside the map (the reference's grid runs over [-1,1] with align_corners off), where a map of ones
    samples to 0.5 and 0.25; of fours it stays at or above 1."""
    md = torch.ones(1, 2, hd, wd)
    md[:, 1] = 4.0
    return torch.zeros(1, 2, hd2, wd2), torch.zeros(1, 2, hd, wd), torch.eye(3)[None].clone(), md


# 8 x 12 cells, 64 x 96 = 6144 pixels.  Homography 0: plateaus of 64, 128 and 192 pixels; homography 1: one of 16 x 16 = 256 that
# covers the first.  cc_th = 128 / 6144: the second plateau's area fraction is exactly on it (<= removes it), the first is below,
# the third and homography 1's above.
CC_A = ((8, 12, 4, 6), [(1, 2, 1, 2), (1, 3, 5, 6), (5, 6, 1, 4)], [(1, 3, 1, 3)])
CC_B = ((6, 10, 3, 5), [(1, 2, 1, 2), (3, 4, 4, 8)], [(1, 3, 1, 3)])                   # 48 x 80 = 3840 pixels: 64 | 256; 256
CC_ON = 128.0 / 6144.0


@pytest.mark.parametrize("multiH", [True, False])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("cc_th", [CC_ON, 1.0], ids=["on-a-component", "all-but-the-whole-map"])
def test_component_filter_between_score_and_merge(dev, ragged, multiH, cc_th):
    th = 0.5
    a = _plateau_pair(*CC_A[0], CC_A[1], CC_A[2])
    if ragged:
        pairs = [a, _plateau_pair(*CC_B[0], CC_B[1], CC_B[2]), _whole_pair(4, 6, 2, 3)]
        R = _ragged(pairs, dev, max_h=4)
    else:
        pairs = [a, _whole_pair(8, 12, 4, 6), a]
        R = _dense(pairs, 8, 12, 4, 6, dev, max_h=4)
    sizes = [(8 * p[1].shape[2], 8 * p[1].shape[3]) for p in pairs]
    # what the family was built for, on the chain's own scores
    _, filt, raw, _, _ = _per_homography(a, (64, 96), dev, cc_th)
    plateau, kept = raw > 0.99, filt > 0.99
    assert [int(p.sum()) for p in plateau] == [64 + 128 + 192, 256] and ops.cc_max_area(6144, CC_ON) == 128
    assert int((plateau[0][:40, 40:64]).sum()) == 128                                    # the plateau whose fraction is exactly cc_th
    assert bool((plateau & ~kept).any()), "the filter must remove a component"
    assert not bool(filt[plateau & ~kept].any()) and _bits(filt[~plateau | kept], raw[~plateau | kept])
    if cc_th == CC_ON:
        assert [int(k.sum()) for k in kept] == [192, 256] and bool(kept[0][44:52, 12:36].all())
    else:
        assert [int(k.sum()) for k in kept] == [0, 0]
    w = [p for p in pairs if p[1].shape[0] == 1][0]                                      # a component that is the whole map stays
    whw = (8 * w[1].shape[2], 8 * w[1].shape[3])
    _, wf, wr, _, _ = _per_homography(w, whw, dev, cc_th)
    assert bool((wr > 0.99).all()) and _bits(wf, wr), "the filter must keep a component"
    got = ops.assemble_kitti_records(R, th, multiH, cc_th=cc_th)
    plain = ops.assemble_kitti_records(R, th, multiH, cc_th=0.0)
    for k, (pair, hw) in enumerate(zip(pairs, sizes)):
        _assert_pair((got[0][k], got[1][k], got[2][k]), _chain(pair, hw, th, multiH, dev, cc_th), (k, ragged, multiH, cc_th))
        _assert_pair((plain[0][k], plain[1][k], plain[2][k]), _chain(pair, hw, th, multiH, dev), (k, ragged, multiH, 0.0))
    b1, b0 = got[2][0], plain[2][0]
    assert not _bits(b1, b0), "the filter changes nothing: the case proves nothing"
    # the first plateau of homography 0 is removed: with multiH its pixels go to homography 1, which covers them
    first = torch.zeros((64, 96), dtype=torch.bool, device=dev)
    first[12:20, 12:20] = True
    assert bool(plateau[0][first].all()) and bool(b0[first].all())
    if cc_th == CC_ON:
        assert bool(b1[first].all()) == multiH and bool(b1[first].any()) == multiH
        if multiH:
            flow1 = _per_homography(a, (64, 96), dev)[0][1]
            assert _bits(got[0][0][first], torch.clamp(flow1, -1, 1)[first]) and not _bits(got[0][0][first], plain[0][0][first])
    else:
        assert not bool(b1[first].any())


# ---------------------------------------------------------------- 4. threshold and order

def _order_pair():
    """Matchability 1->2 in {0.125, 0.25, 0.5, 1} constant over blocks of 2 x 2 cells (4 x 6 cells), 2->1 all ones, zero flows,
    homography 0 the identity, 1 and 2 moved by a quarter to either side (in-bounds mask 0 on one edge):
        columns    0-1      2-3                      4-5
        match12_0  0.25     0.125                    0.125      on th | below | below
        match12_1  0.125    0.5 (rows 0-1) | 0.125   0.125      1 and 2 pass: the first wins | only 2 passes, on th
        match12_2  0.125    1.0 (rows 0-1) | 0.25    0.125      nobody passes in the last columns"""
    n, hd, wd = 3, 4, 6
    md = torch.full((n, 2, hd, wd), 0.125)
    md[:, 1] = 1.0
    md[0, 0, :, :2] = 0.25
    md[1, 0, :2, 2:4], md[2, 0, :2, 2:4], md[2, 0, 2:, 2:4] = 0.5, 1.0, 0.25
    pm = torch.eye(3)[None].repeat(n, 1, 1)
    pm[1, 0, 2], pm[2, 0, 2] = 0.25, -0.25
    return torch.zeros(n, 2, 2, 3), torch.zeros(n, 2, hd, wd), pm, md


@pytest.mark.parametrize("multiH", [True, False])
@pytest.mark.parametrize("cc_th", [0.0, 0.06])
def test_threshold_and_order(dev, multiH, cc_th):
    pair = _order_pair()
    out_hw = (32, 48)
    flow, score, raw, _, (_, inb) = _per_homography(pair, out_hw, dev, cc_th)
    s0, s1, s2 = score
    assert bool((inb[1:] == 0).any())
    if cc_th:
        assert bool(((raw > 0.99) & (score == 0)).any()), "the filter removes the plateau of homography 2"
    # th = a value scores take exactly: the commonest score of homography 0 in its own block, and of homography 2 where only it passes
    th_a = float(s0[:, :12].flatten().mode().values)
    th_b = float(s2[20:, 20:28].flatten().mode().values)
    assert 0.2 < th_a < 0.3 and 0.2 < th_b < 0.3
    R = _dense([pair, pair], 4, 6, 2, 3, dev, max_h=5)
    for th in (th_a, th_b):
        on0 = s0 == th
        on2 = (s0 < th) & (s1 < th) & (s2 == th)
        nobody = (score < th).all(0)
        both = (s0 < th) & (s1 >= _next(th)) & (s2 >= _next(th))
        assert int(on0.sum()) > 0 and int(nobody.sum()) > 0 and (th != th_b or int(on2.sum()) > 0)
        if not cc_th:
            assert int(both.sum()) > 0 and bool((flow[1][both] != flow[2][both]).any())
        binary = {}
        for t in (th, _next(th)):                               # scores == th, and the same scores one ulp below th
            fg, mg, b, _ = ops.assemble_kitti_records(R, t, multiH, cc_th=cc_th)
            _assert_pair((fg[0], mg[0], b[0]), _chain(pair, out_hw, t, multiH, dev, cc_th), (t, multiH, cc_th))
            assert _bits(fg[0], fg[1]) and _bits(mg[0], mg[1]) and _bits(b[0], b[1])
            want = _restated(flow, score, t, multiH)            # the first index that reaches th, on the chain's own (filtered) scores
            assert _bits(fg[0], want[0]) and _bits(mg[0], want[1]) and _bits(b[0], want[2]), (t, multiH, cc_th)
            binary[t] = b[0]
        alone = on0 & (s1 < th) & (s2 < th)
        assert int(alone.sum()) > 0 and bool(binary[th][on0].all()) and not bool(binary[_next(th)][alone].any())
        assert bool(binary[th][on2].all()) == (multiH or not bool(on2.any())) and not bool(binary[_next(th)][on2].any())
        assert not bool(binary[th][nobody].any())
        if bool(both.any()):
            assert bool(binary[th][both].all()) == multiH


# ---------------------------------------------------------------- 5. NaN

@pytest.mark.parametrize("cc_th", [0.0, 0.05])
def test_nan_of_a_degenerate_homography_and_nan_scores(dev, cc_th):
    hd, wd, hd2, wd2 = 4, 6, 2, 3
    out_hw = (hd * 8, wd * 8)
    zero, eye = torch.zeros(3, 3), torch.eye(3)
    md = torch.ones(2, 2, hd, wd)
    md[1, 0, :, wd // 2:] = 0.0
    fd, fd2 = torch.zeros(2, 2, hd, wd), torch.zeros(2, 2, hd2, wd2)
    first = (fd2, fd, torch.stack((zero, eye)), md)             # z' = 0 everywhere at index 0: owns what index 1 does not
    md2 = torch.ones(2, 2, hd, wd)
    md2[0, 0, :, wd // 2:] = 0.0
    second = (fd2, fd, torch.stack((eye, zero)), md2)           # ... and at index 1: 0/0 flow, in-bounds mask 0
    g = torch.Generator().manual_seed(204)
    holes = list(_random_pair(g, 3, hd, wd, hd2, wd2))          # NaN matchability: through match12 at 0 and 2, through match21 at 1
    holes[3][0, 0, :2], holes[3][2, 0, 1:3, 2:5], holes[3][1, 1, 2:, :3] = NAN, NAN, NAN
    plate = list(_plateau_pair(hd, wd, hd2, wd2, [(0, 3, 0, 2)], []))   # a plateau above 0.99 with a NaN cell inside
    plate[3][0, 0, 1, 1] = NAN
    huge = list(_random_pair(g, 1, hd, wd, hd2, wd2))           # match12 * cycle overflows before the in-bounds factor: inf * 0 = NaN
    huge[3] = huge[3] * 3.0e38
    huge[2][0, 0, 2] = 0.5                                      # a band out of bounds whatever the draw
    pairs = [first, second, tuple(holes), tuple(plate), tuple(huge)]
    th = 0.3                                                    # no score of the first two pairs is near it
    fg, mg, b, _ = ops.assemble_kitti_records(_dense(pairs, hd, wd, hd2, wd2, dev), th, True, cc_th=cc_th)
    for k, pair in enumerate(pairs):
        _assert_pair((fg[k], mg[k], b[k]), _chain(pair, out_hw, th, True, dev, cc_th), (k, cc_th))
    assert bool(fg[0].isnan().any()) and bool(fg[0][~b[0]].isnan().all()) and not bool(fg[0][b[0]].isnan().any())
    assert bool(b[1][2:-2, 2:wd * 4 - 8].all()) and not bool(b[1][:, wd * 4 + 8:].any()) and not bool(fg[1].isnan().any())
    score = _per_homography(tuple(holes), out_hw, dev, cc_th)[1]
    assert int(score.isnan().sum()) > 100
    owner_nan = mg[2].isnan()
    assert bool(owner_nan.any()) and not bool(b[2][owner_nan].any()), "a NaN score owns a pixel"
    assert bool((score[0].isnan() & b[2]).any()), "no pixel with a NaN score at 0 is taken by a later homography"
    # a NaN score is not above 0.99: it is no pixel of a component and stays a NaN through the filter
    _, filt, raw, _, _ = _per_homography(tuple(plate), out_hw, dev, cc_th)
    assert bool(raw[0].isnan().any()) and bool((raw[0] > 0.99).any()) and _bits(filt[0][raw[0].isnan()], raw[0][raw[0].isnan()])
    assert bool(mg[3].isnan().any()) and not bool(b[3][mg[3].isnan()].any())
    assert bool(mg[4].isnan().any()) and bool(mg[4].isinf().any()) and not bool(b[4][mg[4].isnan()].any())


# ---------------------------------------------------------------- 6. interpolate

@pytest.mark.parametrize("cc_th", [0.0, 0.05])
def test_interpolate_is_the_nearest_fill_of_the_chain(dev, dense_pairs, cc_th):
    g = torch.Generator().manual_seed(206)
    empty = list(_random_pair(g, 2, HD, WD, HD2, WD2))
    empty[3][:, 0] = 0.0                                        # match12 zero: no score reaches th, the binary map is empty
    pairs = [dense_pairs[1], None, tuple(empty), dense_pairs[2]]
    out_hw = (27, 50)
    fg, mg, b, valid = ops.assemble_kitti_records(_dense(pairs, HD, WD, HD2, WD2, dev), TH1, True, cc_th=cc_th, interpolate=True,
                                                  out_hw=out_hw)
    raw = ops.assemble_kitti_records(_dense(pairs, HD, WD, HD2, WD2, dev), TH1, True, cc_th=cc_th, out_hw=out_hw)
    assert valid.tolist() == [True, False, True, True] and _bits(mg, raw[1]) and _bits(b, raw[2])
    for k in (0, 2, 3):
        f0, m0, b0 = _chain(pairs[k], out_hw, TH1, True, dev, cc_th)
        assert _bits(fg[k], ops.nearest_fill(f0, b0)[0]), k
        _assert_pair((fg[k], mg[k], b[k]), _chain(pairs[k], out_hw, TH1, True, dev, cc_th, True), (k, "interpolate"))
    _assert_zero(fg[1], mg[1], b[1])
    assert not bool(b[2].any()) and _bits(fg[2], raw[0][2][-1, 0].expand(27, 50, 2).contiguous())    # an empty map reads pixel (H-1, 0)
    assert bool(b[0].any()) and any(not bool(b[k].all()) and not _bits(fg[k], raw[0][k]) for k in (0, 3))
    # ragged records: one fill per run of same-size pairs; caller-owned buffers receive the filled flow
    g2 = torch.Generator().manual_seed(207)
    same = [_random_pair(g2, 2, 4, 6, 2, 3), _random_pair(g2, 1, 4, 6, 2, 3), _random_pair(g2, 3, 2, 2, 1, 1)]
    total = 2 * 32 * 48 + 256
    out = (torch.full((total, 2), NAN, device=dev), torch.full((total,), NAN, device=dev), torch.zeros(total, dtype=torch.bool, device=dev))
    fr, mr, br, _ = ops.assemble_kitti_records(_ragged(same, dev), TH1, True, cc_th=cc_th, interpolate=True, out=out)
    assert fr[0].data_ptr() == out[0].data_ptr()
    for k, pair in enumerate(same):
        hw = (8 * pair[1].shape[2], 8 * pair[1].shape[3])
        _assert_pair((fr[k], mr[k], br[k]), _chain(pair, hw, TH1, True, dev, cc_th, True), (k, "ragged interpolate"))


# ---------------------------------------------------------------- 7. the reference's own outputs

def _close(dev_t, ref, what, max_bad, excuse):
    """tests/test_gpu_assemble.py's rule: at most max_bad of the values differ by more than TOL and none of them at a pixel outside
    ``excuse`` (ae.excusable)."""
    d = (dev_t.cpu().float() - torch.as_tensor(ref).float()).abs()
    bad = float((d > TOL).float().mean())
    assert bad <= max_bad, "%s: %.4f%% of the values differ by more than %g (max %g)" % (what, 100 * bad, TOL, float(d.max()))
    unexplained, differing = ae.unexplained(dev_t, ref, excuse, TOL)
    assert unexplained == 0, "%s: %d of %d differing pixels are not within rounding of a threshold" % (what, unexplained, differing)


def test_records_of_the_golden_inputs_give_the_reference_outputs(dev):
    gold = np.load(os.path.join(GOLD, "assemble.npz"))
    n, hd, wd = int(gold["n"]), int(gold["hd"]), int(gold["wd"])
    fd, fd2, pm, md = synth.assembly_arrays(int(gold["seed"]), n, hd, wd)
    pair = tuple(torch.from_numpy(np.ascontiguousarray(a)).float() for a in (fd2, fd, pm, md))
    cmp = ae.comparisons(gold)
    for row, tag in enumerate("abcd"):                          # tag k in row k of a batch of four, the other rows empty
        R = _dense([pair if k == row else None for k in range(4)], hd, wd, hd // 2, wd // 2, dev, max_h=max(n, 11))
        th, cc, interp, multiH = gold["kitti_%s_cfg" % tag]
        fg, _, _, valid = assemble.assemble_kitti_records(R, (hd * 8, wd * 8), float(th), bool(multiH), float(cc), bool(interp))
        assert valid.tolist() == [k == row for k in range(4)]
        case, cth, cm, ccc, cint, _ = cmp["golden-kitti-" + tag]
        _close(fg[row:row + 1], gold["kitti_%s" % tag], "kitti " + tag, 0.01, ae.excusable(case, cth, cm, ccc, cint))


# ---------------------------------------------------------------- 8. the result does not depend on the chunk plan

def test_one_pair_per_chunk_gives_the_same_bits(dev):
    g = torch.Generator().manual_seed(208)
    pairs = [_random_pair(g, n, h, w, h2, w2) for h, w, h2, w2, n in RAGGED + ((4, 6, 2, 3, 11),)]
    pairs[1][3][0, 0] = 1.0                                     # plateaus for the filter to work on
    pairs[3][3][:, 0, :2, :3] = 1.0
    R = _ragged(pairs, dev)
    assert ops.assemble_kitti_records_plan(R, cc_th=0.02) == [(0, 4)]
    assert ops.assemble_kitti_records_plan(R, cc_th=0.02, ws_bytes=1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    for interp in (False, True):
        whole = ops.assemble_kitti_records(R, TH1, True, cc_th=0.02, interpolate=interp)
        split = ops.assemble_kitti_records(R, TH1, True, cc_th=0.02, interpolate=interp, ws_bytes=1)
        mid = ops.assemble_kitti_records(R, TH1, True, cc_th=0.02, interpolate=interp, ws_bytes=16 * 11 * (2240 + 1536))
        for k in range(4):
            assert all(_bits(whole[j][k], split[j][k]) and _bits(whole[j][k], mid[j][k]) for j in range(3)), (k, interp)
    for k, pair in enumerate(pairs):
        hw = (8 * pair[1].shape[2], 8 * pair[1].shape[3])
        _assert_pair((split[0][k], split[1][k], split[2][k]), _chain(pair, hw, TH1, True, dev, 0.02, True), (k, "chunks"))
    D = _dense([pairs[3], pairs[1], None], 4, 6, 2, 3, dev)
    assert all(_bits(x, y) for x, y in zip(ops.assemble_kitti_records(D, TH1, True, cc_th=0.02),
                                           ops.assemble_kitti_records(D, TH1, True, cc_th=0.02, ws_bytes=1)))


# ---------------------------------------------------------------- 9. beyond the launch cap

@pytest.mark.parametrize("cc_th", [0.0, 0.3])
def test_maps_beyond_the_launch_cap(dev, cc_th):
    """The grid is capped at 8192 workgroups of 256 pixels per pair: a 1450 x 1450 map (2 102 500 > 2 097 152 pixels) takes a second
    trip.  Index images as /8 maps (every cell another value), two homographies; the second owns the top rows."""
    hd, wd, out_hw = 6, 7, (1450, 1450)
    idx = (torch.arange(2 * hd * wd, dtype=torch.float32) + 1).view(1, 2, hd, wd)
    pm = torch.eye(3)[None].repeat(2, 1, 1)
    pm[0, 1, 2], pm[1, 0, 2] = -0.0625, 0.03125
    md = torch.cat((idx / float(2 * hd * wd), 1.0 - 0.5 * idx / float(2 * hd * wd)))
    md[:, 1] = 1.0
    md[0, 0, 4:] = 1.0                                          # a plateau of homography 0 at the bottom for the filter
    pair = (torch.cat((idx, -idx))[:, :, :3, :3].contiguous() * 2.0 ** -9, torch.cat((-idx, idx)) * 2.0 ** -10, pm, md)
    fg, mg, b, _ = ops.assemble_kitti_records(_dense([pair], hd, wd, 3, 3, dev, max_h=2), 0.3, True, cc_th=cc_th, out_hw=out_hw)
    _assert_pair((fg[0], mg[0], b[0]), _chain(pair, out_hw, 0.3, True, dev, cc_th), ("beyond the cap", cc_th))
    assert bool(b.any()) and not bool(b.all())
    if cc_th:                                                   # the plateau is removed, in the second trip's rows too
        plain = ops.assemble_kitti_records(_dense([pair], hd, wd, 3, 3, dev, max_h=2), 0.3, True, out_hw=out_hw)
        assert not _bits(fg[0, -3:], plain[0][0, -3:]) and not _bits(mg[0, -3:], plain[1][0, -3:])


# ---------------------------------------------------------------- 9b. the score kernel on its own

@pytest.mark.parametrize("multiH", [True, False])
def test_score_kernel_fills_the_filter_table_and_only_the_maps_the_merge_reads(dev, dense_pairs, multiH):
    """rfx_kitti_scores_records_f32 called directly: row (pair, i) of the component filter's table is (H, W, max_area) for i < last and
    (0, 0, 0) -- a map the filter skips -- for the rest and for a pair whose table row is refused; the score maps i < last are the
    chain's match_score, the others are not written."""
    out_hw, max_h = (27, 50), 11
    pairs = list(dense_pairs) + [dense_pairs[1]]
    R = _dense(pairs, HD, WD, HD2, WD2, dev)
    rows, max_hw, total = ops.assemble_kitti_records_table(R, out_hw, cc_th=0.05)
    rows[4] = rows[4][:4] + (R.width - 4,) + rows[4][5:]        # a flowD2 part that would leave the record: the row is refused
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    hw = out_hw[0] * out_hw[1]
    scores = torch.full((5 * max_h * hw,), -7.0, device=dev)
    dims = torch.full((5 * max_h, 3), -1, dtype=torch.int32, device=dev)
    ops._call("rfx_kitti_scores_records_f32", R.rec.device, ops._p(R.rec), R.rec.numel(), R.width, max_h, R.off_H, R.off_flow,
              ops._p(table), 5, max_hw, 1 if multiH else 0, ops._p(scores), 0, scores.numel(), ops._p(dims), total)
    area = ops.cc_max_area(hw, 0.05)
    last = [(n if multiH else min(n, 1)) for n in NBH] + [0]
    want = [[out_hw[0], out_hw[1], area] if i < last[b] else [0, 0, 0] for b in range(5) for i in range(max_h)]
    assert dims.tolist() == want and area == 67
    maps = scores.view(5, max_h, *out_hw)
    for b in range(5):
        if last[b]:
            assert _bits(maps[b, :last[b]], _per_homography(pairs[b], out_hw, dev)[2][:last[b]]), b
        assert bool((maps[b, last[b]:] == -7.0).all()), b


# ---------------------------------------------------------------- 10. no host sync

def test_the_call_does_not_sync_with_the_host(dev, dense_pairs):
    R = _dense(dense_pairs, HD, WD, HD2, WD2, dev)
    Rr = _ragged([p for p in dense_pairs[:3]] + [dense_pairs[0]], dev)
    sizes = [(27, 50), (27, 50), (3, 85), (1, 257)]
    ops.assemble_kitti_records(R, 0.3, True, cc_th=0.05, interpolate=True)               # the library is loaded, the allocators are warm
    ops.assemble_kitti_records(Rr, 0.3, True, cc_th=0.05, interpolate=True, out_hw=sizes, ws_bytes=1)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                       # the mode does see a sync on this build
            R.rec[0, 0].item()
        out = ops.assemble_kitti_records(R, 0.3, True, cc_th=0.05, interpolate=True)
        out_r = ops.assemble_kitti_records(Rr, 0.3, True, cc_th=0.05, interpolate=True, out_hw=sizes, ws_bytes=1)
        out_w = assemble.assemble_kitti_records(R, (27, 50), 0.3, False)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert out[3].is_cuda and out_r[3].is_cuda and out_w[3].is_cuda
    assert out[3].tolist() == [True, True, True, False]


# ---------------------------------------------------------------- 11. end to end: records -> flow -> end-point error

def test_batch_end_point_error_equals_the_per_pair_path(dev):
    g = torch.Generator().manual_seed(211)
    H, W = 27, 50
    nb = (3, 1, 11, 2)
    pairs = [_random_pair(g, n, HD, WD, HD2, WD2, flow_amp=0.05, h_amp=0.04) for n in nb]
    u = (torch.randint(-640, 640, (4, H, W), generator=g).float() / 64).to(dev)          # KITTI's (uint16 - 32768) / 64: exact in float32
    v = (torch.randint(-320, 320, (4, H, W), generator=g).float() / 64).to(dev)
    valid = (torch.rand(4, H, W, generator=g) > 0.3).to(dev)
    fg, _, _, _ = ops.assemble_kitti_records(_dense(pairs, HD, WD, HD2, WD2, dev), 0.35, True, cc_th=0.01, out_hw=(H, W))
    total, count = ops.epe_flow(fg, u, v, valid)
    means = assemble.kitti_epe(fg, u, v, valid)
    for k, pair in enumerate(pairs):
        f1 = _chain(pair, (H, W), 0.35, True, dev, 0.01)[0]
        t1, c1 = ops.epe_flow(f1, u[k:k + 1], v[k:k + 1], valid[k:k + 1])
        assert _bits(total[k:k + 1].view(torch.int64), t1.view(torch.int64)) and int(count[k]) == int(c1[0]) > 0, k
        m1 = assemble.kitti_epe(f1, u[k], v[k], valid[k])
        assert np.float64(means[k]).tobytes() == np.float64(m1).tobytes(), k


# ---------------------------------------------------------------- 12. the driver's own records

def test_records_filled_by_the_kitti_driver(dev):
    import test_gpu_ragged_kitti as rk
    pipe, pairs = rk._pipe("device"), rk._pairs()
    two, ids = [pairs[2], pairs[3]], [rk.IDS[2], rk.IDS[3]]     # the two smallest pairs of different sizes
    tabs = rk._tables(pipe, two)
    R = rk._records(tabs, 8)
    outs = pipe.multi_h_kitti_batched([rk._up(p[0]) for p in two], [rk._up(p[1]) for p in two], records=R, pair_ids=ids, **rk.KW)
    assert [o["nbH"] for o in outs] == [rk.NBH_ALONE[2], rk.NBH_ALONE[3]]
    sizes = [tuple(s) for s in tabs["org"]]
    for cc_th, interp in ((0.0, False), (rk.KW["cc_th"], True)):
        fg, mg, b, valid = assemble.assemble_kitti_records(R, sizes, 0.5, True, cc_th, interp)
        assert valid.tolist() == [True, True]
        for k in range(2):
            nbH, _, Hs, f8, m8, d2 = R.views(k)
            n = int(nbH)
            want = assemble.assemble_kitti(d2[:n], f8[:n], Hs[:n], m8[:n], sizes[k], 0.5, True, cc_th, interp, dev, fill="device")
            _assert_pair((fg[k], mg[k], b[k]), want, ("driver", k, cc_th, interp))
