"""The flow assembly of a whole batch from its device records in one launch (ops.assemble_records, rfx_assemble_records_f32;
assemble.assemble_records / assemble_yfcc_records) against the per-pair chain assemble.assemble on the record's first nbH entries
(tests/test_gpu_assemble.py holds that chain to the reference): all three maps as BIT PATTERNS, NaN payloads included.  Entries of a
record past nbH are filled with NaN here, so a kernel that read one would show."""
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
TH = 0.25
TH_NEXT = float(np.nextafter(np.float32(TH), np.float32(1)))
NAN = float("nan")


# ---------------------------------------------------------------- helpers

def _bits(a, b):
    """Same shape, dtype and bit pattern (float32 compared as int32: -0.0 != 0.0, a NaN equals only the same NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


def _random_pair(g, n, hd, wd, flow_amp=0.3, h_amp=0.12):
    """flowDown8 large enough to push sampling points beyond [-1,1] near the border, homographies that move part of the image out of
    bounds, matchability in [0,1]."""
    fd = torch.randn(n, 2, hd, wd, generator=g) * flow_amp
    pm = torch.eye(3)[None].repeat(n, 1, 1) + h_amp * torch.randn(n, 3, 3, generator=g)
    pm[:, :2, 2] += torch.rand(n, 2, generator=g) - 0.5
    md = torch.rand(n, 2, hd, wd, generator=g)
    return fd, pm, md


def _fill(views, pair, dev):
    """Write one pair's arrays (or None: no homography) into its record views; the entries past nbH become NaN."""
    nbH, Hs, f8, m8 = views
    Hs.fill_(NAN), f8.fill_(NAN), m8.fill_(NAN)
    n = 0 if pair is None else pair[0].shape[0]
    if n:
        f8[:n], Hs[:n], m8[:n] = pair[0].to(dev), pair[1].to(dev), pair[2].to(dev)
    nbH.fill_(float(n))


def _dense(pairs, hd, wd, dev, max_h=11):
    R = ops.MultiHRecords(len(pairs), hd, wd, dev, max_h=max_h)
    nbH, _, Hs, f8, m8, _ = R.views()
    for b, pair in enumerate(pairs):
        _fill((nbH[b], Hs[b], f8[b], m8[b]), pair, dev)
    return R


def _ragged(pairs, dev, max_h=11):
    R = ops.MultiHRecordsRagged([p[0].shape[2] for p in pairs], [p[0].shape[3] for p in pairs], dev, max_h=max_h)
    for b, pair in enumerate(pairs):
        nbH, _, Hs, f8, m8 = R.views(b)
        _fill((nbH, Hs, f8, m8), pair, dev)
    return R


def _chain(pair, out_hw, th, multiH, cycle, dev):
    """The yardstick: the per-pair chain (five or six launches) on the pair's own arrays."""
    return assemble.assemble(pair[0].to(dev), pair[1].to(dev), pair[2].to(dev), out_hw, th, multiH, cycle, dev)


def _assert_pair(got, want, what):
    """got: (flow (H,W,2), match (H,W), binary (H,W)) of one pair; want: the chain's (1,H,W,2), (1,H,W), (1,H,W)."""
    for x, y, name in zip(got, want, ("flowGlobal", "matchGlobal", "binary")):
        assert _bits(x, y[0]), (what, name, int((x != y[0]).sum()))


def _per_homography(pair, out_hw, cycle, dev):
    """flow_i (n,H,W,2) and score_i (n,H,W) of one pair from the chain's own kernels (what merge_multi_h sees)."""
    fd, pm, md = (t.to(dev) for t in pair)
    H, W = out_hw
    flow, inb, fup = ops.compose_flow(fd, ops.warp_grid(pm, H, W), clamp=True, want_inb=True, want_flow_up=True)
    m = ops.resize_bilinear(md, (H, W), align_corners=False)
    cyc = ops.grid_sample(m[:, 1:2].contiguous(), fup)[:, 0] if cycle else None
    return flow, ops.match_score(m[:, 0], cyc=cyc, inb=inb), inb, fup


# ---------------------------------------------------------------- 1. dense records

HD, WD = 3, 4
NBH = (1, 2, 11, 0)


@pytest.fixture(scope="module")
def dense_pairs():
    g = torch.Generator().manual_seed(101)
    return [_random_pair(g, n, HD, WD) if n else None for n in NBH]


def test_random_contents_reach_the_clamp_the_border_and_out_of_bounds(dev, dense_pairs):
    flow, score, inb, fup = _per_homography(dense_pairs[2], (24, 32), True, dev)
    assert bool((fup.abs() == 1.0).any()) and bool((inb == 0).any()) and bool((inb == 1).any())
    assert bool(((score[0] < 0.15) & (score[1:] >= 0.15).any(0)).any()), "no pixel is owned by a homography i >= 1"


@pytest.mark.parametrize("out_hw,cycle", [((24, 32), False), ((24, 32), True), ((27, 30), False), ((3, 85), False), ((16, 16), False),
                                          ((1, 257), False)], ids=str)
@pytest.mark.parametrize("multiH", [False, True])
def test_dense_records_equal_the_chain_bit_for_bit(dev, dense_pairs, out_hw, cycle, multiH):
    th = 0.15 if cycle else 0.35
    R = _dense(dense_pairs, HD, WD, dev)
    fg, mg, b, valid = ops.assemble_records(R, th, multiH, cycle, out_hw=None if out_hw == (24, 32) else out_hw)
    assert fg.shape == (4,) + out_hw + (2,) and mg.shape == b.shape == (4,) + out_hw and b.dtype == torch.bool
    assert valid.tolist() == [True, True, True, False] and valid.device == fg.device
    for k, pair in enumerate(dense_pairs[:3]):
        _assert_pair((fg[k], mg[k], b[k]), _chain(pair, out_hw, th, multiH, cycle, dev), (k, out_hw, cycle, multiH))
    assert not bool(fg[3].view(torch.int32).any()) and not bool(mg[3].view(torch.int32).any()) and not bool(b[3].any())
    assert bool(b[0].any()) and not bool(b[0].all())            # one homography: explained in part


# ---------------------------------------------------------------- 2. ragged records

RAGGED = ((3, 4, 2), (5, 3, 1), (2, 2, 3))                      # (h8, w8, nbH)


@pytest.mark.parametrize("sizes,cycle", [(None, True), (None, False), ([(27, 30), (16, 16), (1, 257)], False)], ids=str)
def test_ragged_records_equal_the_chain_at_any_position(dev, sizes, cycle):
    g = torch.Generator().manual_seed(102)
    pairs = [_random_pair(g, n, h, w) for h, w, n in RAGGED]
    th = 0.15 if cycle else 0.35
    hw = sizes or [(8 * h, 8 * w) for h, w, _ in RAGGED]
    fg, mg, b, valid = ops.assemble_records(_ragged(pairs, dev), th, True, cycle, out_hw=sizes)
    assert valid.tolist() == [True] * 3 and [tuple(t.shape) for t in mg] == hw
    want = [_chain(p, s, th, True, cycle, dev) for p, s in zip(pairs, hw)]
    for k in range(3):
        _assert_pair((fg[k], mg[k], b[k]), want[k], ("ragged", k, cycle))
    order = [2, 0, 1]                                           # the same pairs at other positions of the batch
    fg2, mg2, b2, _ = ops.assemble_records(_ragged([pairs[k] for k in order], dev), th, True, cycle,
                                           out_hw=None if sizes is None else [sizes[k] for k in order])
    for pos, k in enumerate(order):
        assert _bits(fg2[pos], fg[k]) and _bits(mg2[pos], mg[k]) and _bits(b2[pos], b[k]), (pos, k)
    # caller-owned packed buffers are filled in place
    total = sum(h * w for h, w in hw)
    out = (torch.full((total, 2), NAN, device=dev), torch.full((total,), NAN, device=dev), torch.zeros(total, dtype=torch.bool, device=dev))
    fg3, mg3, b3, _ = ops.assemble_records(_ragged(pairs, dev), th, True, cycle, out_hw=sizes, out=out)
    assert fg3[0].data_ptr() == out[0].data_ptr() and mg3[2].data_ptr() == out[1].data_ptr() + 4 * (total - hw[2][0] * hw[2][1])
    assert all(_bits(fg3[k], fg[k]) and _bits(mg3[k], mg[k]) and _bits(b3[k], b[k]) for k in range(3))
    # packed storage: the views of one call share three buffers
    assert fg[1].data_ptr() == fg[0].data_ptr() + 8 * hw[0][0] * hw[0][1] and b[1].data_ptr() == b[0].data_ptr() + hw[0][0] * hw[0][1]


# ---------------------------------------------------------------- 3. threshold and order

def _exact_pair():
    """Scores whose every product is exact (the recipe of _exact_inputs in tests/test_gpu_assemble.py, on the /8 maps): matchability
    cells in {0.125, 0.25, 0.5, 1}, constant over blocks of 2 x 2 cells -- up-sampled by 8 the weights are multiples of 1/16 and add
    up to 1 exactly, so a pixel between four equal cells has exactly their value --, zero residual flow, homography 0 the identity,
    1 and 2 the identity shifted by a quarter to either side (in-bounds mask 0 on one edge, 1 in the middle).  4 x 6 cells:
        columns    0-1      2-3                      4-5
        match12_0  0.25     0.125                    0.125      on th | below | below
        match12_1  0.125    0.5 (rows 0-1) | 0.125   0.125      1 and 2 pass: the first wins | only 2 passes, on th
        match12_2  0.125    1.0 (rows 0-1) | 0.25    0.125      nobody passes in the last columns"""
    n, hd, wd = 3, 4, 6
    md = torch.full((n, 2, hd, wd), 0.125)
    md[0, 0, :, :2] = 0.25
    md[1, 0, :2, 2:4], md[2, 0, :2, 2:4], md[2, 0, 2:, 2:4] = 0.5, 1.0, 0.25
    md[:, 1] = torch.tensor([0.125, 0.25, 0.5, 1.0])[torch.randint(0, 4, (n, hd, wd), generator=torch.Generator().manual_seed(103))]
    pm = torch.eye(3)[None].repeat(n, 1, 1)
    pm[1, 0, 2], pm[2, 0, 2] = 0.25, -0.25
    return (torch.zeros(n, 2, hd, wd), pm, md), hd, wd


@pytest.mark.parametrize("multiH", [True, False])
def test_threshold_and_order_on_exact_scores(dev, multiH):
    pair, hd, wd = _exact_pair()
    out_hw = (8 * hd, 8 * wd)
    flow, score, inb, _ = _per_homography(pair, out_hw, False, dev)
    s0, s1, s2 = score
    assert bool((inb[1:] == 0).any()) and set(score.unique().tolist()) <= {k / 4096.0 for k in range(4097)}
    on0, on2 = s0 == TH, (s0 < TH) & (s1 < TH) & (s2 == TH)
    both = (s0 < TH) & (s1 >= TH_NEXT) & (s2 >= TH_NEXT)
    nobody = (score < TH).all(0)
    assert min(int(on0.sum()), int(on2.sum()), int(both.sum()), int(nobody.sum())) > 50
    assert bool((flow[1][both] != flow[2][both]).any()) and bool((s1[both] != s2[both]).all()) and bool((s0[nobody] != s2[nobody]).any())
    R = _dense([pair, pair], hd, wd, dev, max_h=5)
    binary = {}
    for th in (TH, TH_NEXT):                                    # scores == th, and the same scores one ulp below th
        fg, mg, b, _ = ops.assemble_records(R, th, multiH, False)
        _assert_pair((fg[0], mg[0], b[0]), _chain(pair, out_hw, th, multiH, False, dev), (th, multiH))
        assert _bits(fg[0], fg[1]) and _bits(mg[0], mg[1]) and _bits(b[0], b[1])
        # the rule restated on the chain's own per-homography scores: the first index that reaches th, else 0
        ok = score >= th
        if not multiH:
            ok[1:] = False
        found = ok.any(0)
        owner = torch.where(found, ok.float().argmax(0), torch.zeros_like(found, dtype=torch.int64))
        pick = lambda t: torch.gather(t, 0, owner[None].expand((1,) + t.shape[1:]) if t.dim() == 3 else
                                      owner[None, :, :, None].expand((1,) + t.shape[1:]))[0]
        assert _bits(b[0], found) and _bits(mg[0], pick(score)) and _bits(fg[0], torch.clamp(pick(flow), -1, 1)), (th, multiH)
        binary[th] = b[0]
    assert bool(binary[TH][on0].all()) and not bool(binary[TH_NEXT][on0].any())
    assert bool(binary[TH][both].all()) == multiH and bool(binary[TH][on2].all()) == multiH and not bool(binary[TH_NEXT][on2].any())
    assert not bool(binary[TH][nobody].any())


# ---------------------------------------------------------------- 4. NaN and non-finite scores

@pytest.mark.parametrize("cycle", [False, True])
def test_nan_of_a_degenerate_homography_and_nan_scores(dev, cycle):
    hd, wd = 4, 6
    out_hw = (hd * 8, wd * 8)
    zero, eye = torch.zeros(3, 3), torch.eye(3)
    md = torch.ones(2, 2, hd, wd)
    md[1, 0, :, wd // 2:] = 0.0
    fd = torch.zeros(2, 2, hd, wd)
    first = (fd, torch.stack((zero, eye)), md)                  # z' = 0 everywhere at index 0: owns what index 1 does not
    md2 = torch.ones(2, 2, hd, wd)
    md2[0, 0, :, wd // 2:] = 0.0
    second = (fd, torch.stack((eye, zero)), md2)                # ... and at index 1: 0/0 flow, in-bounds mask 0
    g = torch.Generator().manual_seed(104)
    holes = list(_random_pair(g, 3, hd, wd))                    # NaN matchability: through match12 at 0 and 2, through match21 at 1
    holes[2][0, 0, :2], holes[2][2, 0, 1:3, 2:5], holes[2][1, 1, 2:, :3] = NAN, NAN, NAN
    huge = list(_random_pair(g, 1, hd, wd))                     # match12 * cycle overflows before the in-bounds factor: inf * 0 = NaN
    huge[2] = huge[2] * 3.0e38
    huge[1][0, 0, 2] = 0.5                                      # a band out of bounds whatever the draw
    pairs = [first, second, tuple(holes), tuple(huge)]
    th = 0.3                                                    # no score of the first two pairs (multiples of 1/64) is near it
    fg, mg, b, _ = ops.assemble_records(_dense(pairs, hd, wd, dev), th, True, cycle)
    for k, pair in enumerate(pairs):
        _assert_pair((fg[k], mg[k], b[k]), _chain(pair, out_hw, th, True, cycle, dev), (k, cycle))
    assert bool(fg[0].isnan().any()) and bool(fg[0][~b[0]].isnan().all()) and not bool(fg[0][b[0]].isnan().any())
    assert bool(b[1][2:-2, 2:wd * 4 - 8].all()) and not bool(b[1][:, wd * 4 + 8:].any()) and not bool(fg[1].isnan().any())
    score = _per_homography(tuple(holes), out_hw, cycle, dev)[1]
    assert int(score.isnan().sum()) > 100
    owner_nan = mg[2].isnan()
    assert bool(owner_nan.any()) and not bool(b[2][owner_nan].any()), "a NaN score owns a pixel"
    assert bool((score[0].isnan() & b[2]).any()), "no pixel with a NaN score at 0 is taken by a later homography"
    if cycle:
        assert bool(mg[3].isnan().any()) and not bool(b[3][mg[3].isnan()].any())


# ---------------------------------------------------------------- 5. background maps (YFCC)

def test_background_maps_only_change_binary(dev):
    g = torch.Generator().manual_seed(105)
    pairs = [_random_pair(g, n, HD, WD) for n in (2, 3)]
    th, out_hw = 0.15, (8 * HD, 8 * WD)
    bg = torch.rand((2,) + out_hw, generator=g) > 0.4
    R = _dense(pairs, HD, WD, dev)
    plain = ops.assemble_records(R, th, True, True)
    for form in (bg.to(dev), (bg.to(torch.uint8) * 255).to(dev), (bg.to(torch.uint8) * 2).to(dev), bg.numpy()):
        fg, b, valid = assemble.assemble_yfcc_records(R, form, th, True)
        assert _bits(fg, plain[0]) and valid.tolist() == [True, True]
        for k, pair in enumerate(pairs):
            wf, wb = assemble.assemble_yfcc(pair[0].to(dev), pair[1].to(dev), pair[2].to(dev), bg[k].to(dev), th, True, dev)
            assert _bits(fg[k], wf[0]) and _bits(b[k], wb[0]), k
    _, mg, b, _ = ops.assemble_records(R, th, True, True, bg=bg.to(dev))
    assert _bits(mg, plain[1]) and _bits(b, plain[2] & bg.to(dev)) and bool((plain[2] & ~bg.to(dev)).any())
    # ragged: one map per pair
    sizes = [(3, 4, 2), (2, 2, 1)]
    rp = [_random_pair(g, n, h, w) for h, w, n in sizes]
    bgs = [torch.rand(8 * h, 8 * w, generator=g) > 0.4 for h, w, _ in sizes]
    fg, b, _ = assemble.assemble_yfcc_records(_ragged(rp, dev), [m.to(dev) for m in bgs], th, True)
    for k, pair in enumerate(rp):
        wf, wb = assemble.assemble_yfcc(pair[0].to(dev), pair[1].to(dev), pair[2].to(dev), bgs[k].to(dev), th, True, dev)
        assert _bits(fg[k], wf[0]) and _bits(b[k], wb[0]), k


# ---------------------------------------------------------------- 6. the reference's own outputs

def _close(dev_t, ref, what, max_bad=0.002, excuse=None):
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
    fd, _, pm, md = synth.assembly_arrays(int(gold["seed"]), n, hd, wd)
    pair = tuple(torch.from_numpy(np.ascontiguousarray(a)).float() for a in (fd, pm, md))
    cmp = ae.comparisons(gold)

    def excuse(name):
        case, th, multiH, cc, interp, _ = cmp[name]
        return ae.excusable(case, th, multiH, cc, interp)

    for row, tag in enumerate("abc"):                           # tag k in row k of a batch of three, the other rows empty
        R = _dense([pair if k == row else None for k in range(3)], hd, wd, dev, max_h=max(n, 11))
        th, multiH, oh, ow = gold["hpatch_%s_cfg" % tag]
        fg, _, _, valid = assemble.assemble_records(R, float(th), bool(multiH), False, out_hw=(int(oh), int(ow)))
        assert valid.tolist() == [k == row for k in range(3)]
        _close(fg[row:row + 1], gold["hpatch_%s" % tag], "hpatch " + tag, excuse=excuse("golden-hpatch-" + tag))
        th, multiH = gold["corr_%s_cfg" % tag]
        fg, mg, _, _ = assemble.assemble_records(R, float(th), bool(multiH), True)
        _close(fg[row:row + 1], gold["corr_%s_flow" % tag], "corr flow " + tag, excuse=excuse("golden-corr-" + tag))
        _close(mg[row:row + 1].unsqueeze(3), gold["corr_%s_match" % tag], "corr match " + tag, excuse=excuse("golden-corr-" + tag))


# ---------------------------------------------------------------- 7. end to end: records -> flow -> end-point error

def test_batch_end_point_error_equals_the_per_pair_path(dev):
    g = torch.Generator().manual_seed(107)
    hd = wd = 5
    S = 40
    nb = (3, 1, 11, 2)
    pairs = [_random_pair(g, n, hd, wd, flow_amp=0.05, h_amp=0.04) for n in nb]
    Hinv = torch.eye(3, dtype=torch.float64)[None].repeat(4, 1, 1) + 0.05 * torch.randn(4, 3, 3, generator=g, dtype=torch.float64)
    Hinv[:, 2, :2] *= 0.02                                      # pixel coordinates: keep z' near 1 over the 40 x 40 map
    fg, _, _, _ = ops.assemble_records(_dense(pairs, hd, wd, dev), 0.35, True, False, out_hw=(S, S))
    total, count = ops.epe_homography(fg, Hinv.to(dev))
    means = assemble.hpatch_epe(fg, Hinv)
    for k, pair in enumerate(pairs):
        f1 = _chain(pair, (S, S), 0.35, True, False, dev)[0]
        t1, c1 = ops.epe_homography(f1, Hinv[k:k + 1].to(dev))
        assert _bits(total[k:k + 1].view(torch.int64), t1.view(torch.int64)) and int(count[k]) == int(c1[0]) > 0, k
        m1 = assemble.hpatch_epe(f1, Hinv[k])
        assert np.float32(means[k]).tobytes() == np.float32(m1).tobytes(), k


# ---------------------------------------------------------------- 8. beyond the launch cap

def test_maps_beyond_the_launch_cap(dev):
    """The grid is capped at 8192 workgroups of 256 pixels per pair: a 1450 x 1450 map (2 102 500 > 2 097 152 pixels) takes a second
    trip.  Index images as /8 maps (every cell another value), one homography."""
    hd, wd, out_hw = 6, 7, (1450, 1450)
    idx = (torch.arange(2 * hd * wd, dtype=torch.float32) + 1).view(1, 2, hd, wd)
    pm = torch.eye(3)[None].clone()
    pm[0, 1, 2] = -0.0625
    pair = (idx * 2.0 ** -10, pm, idx / float(2 * hd * wd))
    fg, mg, b, _ = ops.assemble_records(_dense([pair], hd, wd, dev, max_h=2), 0.3, True, False, out_hw=out_hw)
    _assert_pair((fg[0], mg[0], b[0]), _chain(pair, out_hw, 0.3, True, False, dev), "beyond the cap")
    assert bool(b[0, -1].any()) and not bool(b[0, 0].any())


# ---------------------------------------------------------------- 9. no host sync

def test_the_call_does_not_sync_with_the_host(dev, dense_pairs):
    R = _dense(dense_pairs, HD, WD, dev)
    Rr = _ragged([p for p in dense_pairs[:3]], dev)
    bg = torch.ones((4, 24, 32), dtype=torch.bool, device=dev)
    ops.assemble_records(R, 0.3, True, True, bg=bg)             # the library is loaded, the allocators are warm
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                       # the mode does see a sync on this build
            R.rec[0, 0].item()
        out = ops.assemble_records(R, 0.3, True, True, bg=bg)
        out_r = ops.assemble_records(Rr, 0.3, True, False, out_hw=[(27, 30), (16, 16), (1, 257)])
        out_y = assemble.assemble_yfcc_records(R, bg, 0.3, True)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert out[3].is_cuda and out_r[3].is_cuda and out_y[2].is_cuda
    assert out[3].tolist() == [True, True, True, False]
