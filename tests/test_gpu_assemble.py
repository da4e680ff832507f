"""Offline flow assembly on the GPU: rfx.assemble / the getResults drop-in against the CPU oracle,
against the reference's own outputs (tests/golden/assemble.npz) and, at full evaluation sizes, through
size-independent properties.  The device composes flows to ~1e-6 of the CPU result, so a pixel whose score lies
within float rounding of the threshold may change owner: comparisons allow a vanishing fraction of such pixels -- and, where the
inputs come from synth.assembly_arrays, accept a differing value only at a pixel that the float64 restatement shows to be such a
pixel (tests/assemble_explained.py).  The merge and score kernels themselves are held bit for bit to restate.merge_multi_h on given
scores: scores exactly on the threshold, NaN scores, every input form, flow at and beyond +-1."""
import os
import sys

import numpy as np
import pytest
import torch

import assemble_explained as ae
import restate
from rfx import assemble, ops, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-4


def _close(dev_t, ref, what, max_bad=0.002, excuse=None):
    """At most max_bad of the values differ by more than TOL and, with ``excuse`` (H,W) bool (ae.excusable), none of them at a
    pixel outside it."""
    d = (dev_t.cpu().float() - torch.as_tensor(ref).float()).abs()
    bad = float((d > TOL).float().mean())
    assert bad <= max_bad, "%s: %.4f%% of the values differ by more than %g (max %g)" % (what, 100 * bad, TOL, float(d.max()))
    if excuse is not None:
        unexplained, differing = ae.unexplained(dev_t, ref, excuse, TOL)
        print("EXPLAINED %s: differing pixels %d, unexplained %d, excusable %d of %d" % (what, differing, unexplained,
                                                                                       int(excuse.sum()), excuse.numel()))
        assert unexplained == 0, "%s: %d of %d differing pixels are not within rounding of a threshold" % (what, unexplained, differing)


def _same_binary(b, rb, what, excuse, max_bad=0.002):
    assert float((b.cpu() != rb).float().mean()) <= max_bad
    unexplained, differing = ae.unexplained(b.float(), torch.as_tensor(rb).float(), excuse, 0.5)
    print("EXPLAINED %s: differing pixels %d, unexplained %d" % (what, differing, unexplained))
    assert unexplained == 0, "%s: %d of %d differing pixels are not within rounding of a threshold" % (what, unexplained, differing)


def test_assemble_matches_reference_golden(dev):
    g = np.load(os.path.join(GOLD, "assemble.npz"))
    n, hd, wd = int(g["n"]), int(g["hd"]), int(g["wd"])
    fd, fd2, pm, md = synth.assembly_arrays(int(g["seed"]), n, hd, wd)
    cmp = ae.comparisons(g)

    def excuse(name):
        case, th, multiH, cc, interp, _ = cmp[name]
        return ae.excusable(case, th, multiH, cc, interp)

    for tag in "abc":
        th, multiH, oh, ow = g["hpatch_%s_cfg" % tag]
        fg, _, _ = assemble.assemble(fd, pm, md, (int(oh), int(ow)), float(th), bool(multiH), False, dev)
        _close(fg, g["hpatch_%s" % tag], "hpatch " + tag, excuse=excuse("golden-hpatch-" + tag))
        th, multiH = g["corr_%s_cfg" % tag]
        fg, mg, _ = assemble.assemble(fd, pm, md, (hd * 8, wd * 8), float(th), bool(multiH), True, dev)
        _close(fg, g["corr_%s_flow" % tag], "corr flow " + tag, excuse=excuse("golden-corr-" + tag))
        _close(mg.unsqueeze(3), g["corr_%s_match" % tag], "corr match " + tag, excuse=excuse("golden-corr-" + tag))
    for tag in "abcd":
        th, cc, interp, multiH = g["kitti_%s_cfg" % tag]
        fg, _, _ = assemble.assemble_kitti(fd2, fd, pm, md, (hd * 8, wd * 8), float(th), bool(multiH), float(cc),
                                           bool(interp), dev)
        _close(fg, g["kitti_%s" % tag], "kitti " + tag, max_bad=0.01, excuse=excuse("golden-kitti-" + tag))


@pytest.mark.parametrize("seed,n,cycle", [(21, 1, False), (22, 5, True), (23, 11, False)])
def test_assemble_matches_oracle(dev, seed, n, cycle):
    hd, wd = 9, 13
    fd, _, pm, md = synth.assembly_arrays(seed, n, hd, wd)
    t = torch.from_numpy
    out_hw = (hd * 8, wd * 8) if cycle else (61, 83)
    th = 0.2 if cycle else 0.45
    fg, mg, b = assemble.assemble(fd, pm, md, out_hw, th, True, cycle, dev)
    rf, rm, rb = restate.assemble_flow(t(fd), t(pm), t(md), out_hw, th, True, cycle)
    case, th_ = ae.ORACLE_CASES["oracle-%d" % seed]
    assert case == ae.oracle_case(seed, n, cycle) and th_ == th
    E = ae.excusable(case, th, True)
    _close(fg, rf, "oracle-%d flow" % seed, excuse=E)
    _close(mg, rm, "oracle-%d match" % seed, excuse=E)
    _same_binary(b, rb, "oracle-%d binary" % seed, E)


@pytest.mark.parametrize("name", ["oracle-odd-24", "oracle-odd-27"])
def test_assemble_matches_oracle_at_odd_output_sizes_with_cycle(dev, name):
    """cycle=True at 8x the saved size is always even: 7 x 11 -> 57 x 87 and 9 x 13 -> 61 x 83 put the cycle check's grid_sample on
    an odd last row and column (two shapes; the no-cycle cases above are 61 x 83 too)."""
    case, th = ae.ORACLE_CASES[name]
    seed, n, hd, wd, out_hw, cycle, _ = case
    assert cycle and out_hw[0] % 2 == 1 and out_hw[1] % 2 == 1
    fd, _, pm, md = synth.assembly_arrays(seed, n, hd, wd)
    t = torch.from_numpy
    fg, mg, b = assemble.assemble(fd, pm, md, out_hw, th, True, True, dev)
    rf, rm, rb = restate.assemble_flow(t(fd), t(pm), t(md), out_hw, th, True, True)
    E = ae.excusable(case, th, True)
    _close(fg, rf, name + " flow", excuse=E)
    _close(mg, rm, name + " match", excuse=E)
    _same_binary(b, rb, name + " binary", E)


def test_merge_kernel_is_exact_on_given_scores(dev):
    """With the scores handed over (no device-side composition in front) the ownership rule is integer work."""
    g = torch.Generator().manual_seed(5)
    n, H, W = 7, 37, 53
    flow = (torch.rand(n, H, W, 2, generator=g) * 2.4 - 1.2)
    m = torch.rand(n, 2, H, W, generator=g)
    cyc = torch.rand(n, H, W, generator=g)
    inb = (torch.rand(n, H, W, generator=g) > 0.2).float()
    for multiH in (True, False):
        fg, mg, b = ops.merge_multi_h(flow.to(dev), m.to(dev)[:, 0], 0.3, multiH, cyc=cyc.to(dev), inb=inb.to(dev))
        rf, rm, rb = restate.merge_multi_h(flow.clamp(-1, 1), m[:, 0] * cyc * inb, 0.3, multiH)
        assert torch.equal(fg.cpu(), rf) and torch.equal(mg.cpu(), rm) and torch.equal(b.cpu(), rb)
    sc = ops.match_score(m.to(dev)[:, 0], cyc=cyc.to(dev), inb=inb.to(dev))
    assert torch.equal(sc.cpu(), m[:, 0] * cyc * inb)


def test_merge_and_score_kernels_beyond_the_launch_cap(dev):
    """n*HW and HW above 2^21 (the capped grid of 8192 x 256 threads): both kernels must walk the whole range
    (KITTI assembly at 375x1242 with >= 5 homographies is n*HW = 2.33 M; a 1500x1500 evaluation image is HW = 2.25 M)."""
    g = torch.Generator().manual_seed(6)
    n, H, W = 5, 375, 1242                                     # n*HW = 2 328 750 > 2 097 152
    m = torch.rand(n, 2, H, W, generator=g)
    cyc = torch.rand(n, H, W, generator=g)
    inb = (torch.rand(n, H, W, generator=g) > 0.2).float()
    sc = ops.match_score(m.to(dev)[:, 0], cyc=cyc.to(dev), inb=inb.to(dev))
    assert torch.equal(sc.cpu(), m[:, 0] * cyc * inb)
    n, H, W = 3, 1500, 1500                                    # HW = 2 250 000 > 2 097 152
    flow = (torch.rand(n, H, W, 2, generator=g) * 2.4 - 1.2)
    m = torch.rand(n, H, W, generator=g)
    fg, mg, b = ops.merge_multi_h(flow.to(dev), m.to(dev), 0.6, True)
    rf, rm, rb = restate.merge_multi_h(flow.clamp(-1, 1), m, 0.6, True)
    assert torch.equal(fg.cpu(), rf) and torch.equal(mg.cpu(), rm) and torch.equal(b.cpu(), rb)


def test_assemble_full_size_properties(dev):
    """480x640 output, 11 homographies (the padded maximum of the result record): properties that need no oracle."""
    n, hd, wd = 11, 60, 80
    fd, fd2, pm, md = synth.assembly_arrays(31, n, hd, wd)
    H, W = 480, 640
    single, _, _ = assemble.assemble(fd, pm, md, (H, W), 0.5, False, True, dev)
    allpass, mg, b = assemble.assemble(fd, pm, md, (H, W), -1.0, True, True, dev)     # every score >= th: owner 0
    assert torch.equal(single, allpass) and bool(b.all())
    nopass, _, b2 = assemble.assemble(fd, pm, md, (H, W), 2.0, True, True, dev)       # nothing reaches th: owner 0
    assert torch.equal(single, nopass) and not bool(b2.any())
    multi, mg, b3 = assemble.assemble(fd, pm, md, (H, W), 0.5, True, True, dev)
    assert float(multi.abs().max()) <= 1.0
    # wherever homography 0 already reaches th the merged flow is homography 0's
    _, m0, b0 = assemble.assemble(fd[:1], pm[:1], md[:1], (H, W), 0.5, True, True, dev)
    assert torch.equal(multi[b0], single[b0]) and bool((b3 | ~b0).all())
    assert torch.equal(mg[b0], m0[b0]) and float(mg[b3].min()) >= 0.5
    # reversing the order of homographies 1..n-1 changes owners only where two of them qualify
    perm = [0] + list(range(n - 1, 0, -1))
    rev, _, b4 = assemble.assemble(fd[perm], pm[perm], md[perm], (H, W), 0.5, True, True, dev)
    assert torch.equal(b4, b3)
    # KITTI variant: the nearest-neighbour fill only touches unexplained pixels, and every filled pixel carries the
    # flow of some explained pixel
    k0, _, kb = assemble.assemble_kitti(fd2, fd, pm, md, (H, W), 0.5, True, 0.0, False, dev)
    k1, _, kb1 = assemble.assemble_kitti(fd2, fd, pm, md, (H, W), 0.5, True, 0.0, True, dev)
    assert torch.equal(kb, kb1) and torch.equal(k0[kb], k1[kb]) and float(k1.abs().max()) <= 1.0
    if bool(kb.any()) and not bool(kb.all()):
        explained = set(map(tuple, k0[kb].cpu().numpy().round(6).tolist()))
        filled = k1[~kb].cpu().numpy().round(6).tolist()[:2000]
        assert all(tuple(v) in explained for v in filled)


def test_getresults_dropin_reads_the_on_disk_format(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    n, hd, wd = 3, 8, 10
    fd, fd2, pm, md = synth.assembly_arrays(41, n, hd, wd)
    fine, coarse, maskp, kit = [tmp_path / x for x in ("fine", "coarse", "mask", "kitti")]
    for x in (fine, coarse, maskp, kit):
        x.mkdir()
    np.save(fine / "flow_3_3H.npy", fd.astype(np.float64))          # the scripts save whatever dtype they had
    np.save(fine / "mask_3_3H.npy", md)
    np.save(coarse / "flow_3_3H.npy", pm)
    np.save(maskp / "maskBG_3_3H.npy", np.ones((hd * 8, wd * 8), bool))
    np.save(kit / "Homograpy_3_3.npy", pm)
    np.save(kit / "Finetune_D2_3_3.npy", fd2)
    np.save(kit / "Finetune_3_3.npy", fd)
    np.save(kit / "Finetune_Mask_3_3.npy", md)
    t = torch.from_numpy
    names = os.listdir(fine)
    f = getResults.hpatch.getFlow_all(3, str(fine), str(coarse), names, True, None, None, 0.45, 72, 48)
    assert f.device.type == "cpu" and tuple(f.shape) == (1, 48, 72, 2)
    _close(f, restate.assemble_flow(t(fd), t(pm), t(md), (48, 72), 0.45, True, False)[0], "hpatch drop-in")
    assert getResults.hpatch.getFlow_all(4, str(fine), str(coarse), names, True, None, None, 0.45, 72, 48) == []
    c = getResults.hpatch.getFlow_onlyCoarse(3, str(fine), str(coarse), names, True, None, None, 0.45, 72, 48)
    _close(c, restate.warp_grid(t(pm[:1]), 48, 72), "coarse only")
    f, m = getResults.corr.getFlow(3, str(fine), names, str(coarse), str(maskp), True, 0.2)
    rf, rm, _ = restate.assemble_flow(t(fd), t(pm), t(md), (hd * 8, wd * 8), 0.2, True, True)
    assert tuple(m.shape) == (1, hd * 8, wd * 8, 1)
    _close(f, rf, "corr drop-in flow")
    _close(m[..., 0], rm, "corr drop-in match")
    c, ones = getResults.corr.getFlow_Coarse(3, names, str(fine), str(coarse))
    assert tuple(c.shape) == (1, hd * 8, wd * 8, 2) and float(ones.min()) == 1.0
    grid_org = restate.identity_grid(hd * 8, wd * 8)
    f = getResults.kitti.getFlow_all(3, str(kit), 3, "Finetune", None, True, grid_org, 0.25, 0.01, True)
    rf, _, _ = restate.assemble_flow_kitti(t(fd2), t(fd), t(pm), t(md), (hd * 8, wd * 8), 0.25, True, 0.01, True)
    _close(f, rf, "kitti drop-in", max_bad=0.01)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_online_records_feed_offline_assembly_like_the_reference(dev, tag):
    """SURVEY rows 8f1 -> 8f3 in one piece: the device multi-homography driver fills its per-pair record
    (evaluation/evalHpatch/evaluation.py:254-260 saves exactly these arrays), rfx.assemble composes the final flow from the
    record's views (evalHpatch/getResults.py:48-80), and the result is compared with the oracle's assembly of the arrays the
    REFERENCE's own loop produced for the same pair and index draws (tests/golden/multi_h.npz).  Owner changes at pixels whose
    score sits at the threshold are counted, everything else must agree to 1e-3 (normalised flow units)."""
    from rfx import weights
    from rfx.pipeline import AlignPipeline
    g = np.load(os.path.join(GOLD, "multi_h.npz"))
    seed, maxCoarse, th, draw_seed = g["%s_cfg" % tag]
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=float(g["match_std"])))
    I1, I2 = synth.make_pair(240, 320, seed=int(seed), homography=True)
    pipe = AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant="B", device=dev, draw="host")
    prep = pipe.prepare([(I1, I2)])
    h, w = prep["ItTensor"].shape[2], prep["ItTensor"].shape[3]
    R = ops.MultiHRecords(1, h // 8, w // 8, dev)
    torch.manual_seed(int(draw_seed))
    pipe.multi_h_batched(prep, maxCoarse=int(maxCoarse), maskRegionTh=float(th), records=R, want_lists=False)
    nbH, status, Hs, f8, m8, _ = R.views()
    nb = int(nbH[0])
    assert int(status[0]) == 0 and nb == int(g["%s_nb" % tag])
    t = torch.from_numpy
    for a_th, multiH, cycle in ((0.5, True, False), (0.3, True, True), (0.5, False, False)):
        fg, mg, b = assemble.assemble(f8[0, :nb], Hs[0, :nb], m8[0, :nb], (h, w), a_th,
                                      multiH, cycle, dev)
        rf, rm, rb = restate.assemble_flow(t(g["%s_flowDown8" % tag]), t(g["%s_H" % tag]), t(g["%s_matchDown8" % tag]), (h, w),
                                           a_th, multiH, cycle)
        same = (b.cpu() == rb)
        assert float((~same).float().mean()) < 5e-3, (a_th, multiH, cycle, float((~same).float().mean()))
        d = (fg.cpu() - rf).abs().amax(dim=3)
        bad = float(((d > 1e-3) & same).float().mean())
        assert bad < 5e-3, (a_th, multiH, cycle, bad, float(d.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the merge and score kernels at their edges: given scores, restate.merge_multi_h bit for bit

TH = 0.25
TH_NEXT = float(np.nextafter(np.float32(TH), np.float32(1)))


def _bits_equal(a, b):
    """Bit for bit (signed zeros told apart), every NaN equal to every NaN."""
    a, b = a.cpu(), torch.as_tensor(b)
    if a.dtype != torch.float32:
        return a.dtype == b.dtype and torch.equal(a, b)
    if b.dtype != torch.float32 or a.shape != b.shape or not torch.equal(a.isnan(), b.isnan()):
        return False
    seven = torch.full_like(a, 7.0)
    return torch.equal(torch.where(a.isnan(), seven, a).view(torch.int32), torch.where(b.isnan(), seven, b).view(torch.int32))


def _exact_inputs(n, H, W, seed):
    """Scores whose every product is exact: m in {0.25, 0.5, 1}, cyc in {0.5, 1}, inb in {0, 1}; m comes as channel 0 of an
    (n,2,H,W) tensor.  Flow in [-1.2, 1.2]."""
    g = torch.Generator().manual_seed(seed)

    def pick(vals, shape):
        return torch.tensor(vals)[torch.randint(0, len(vals), shape, generator=g)]

    m2 = pick([0.25, 0.5, 1.0], (n, 2, H, W))
    cyc = pick([0.5, 1.0], (n, H, W))
    inb = pick([0.0, 1.0], (n, H, W))
    flow = torch.rand(n, H, W, 2, generator=g) * 2.4 - 1.2
    return flow, m2, cyc, inb


def _score(m, cyc, inb):
    v = m.clone()                       # left to right in float32, like the reference's tensor expression
    if cyc is not None:
        v = v * cyc
    if inb is not None:
        v = v * inb
    return v


def _merge_both(dev, flow, m2, cyc, inb, th, multiH, sliced=True):
    d = lambda x: None if x is None else x.to(dev)
    m = m2.to(dev)[:, 0] if sliced else m2[:, 0].contiguous().to(dev)
    got = ops.merge_multi_h(flow.to(dev), m, th, multiH, cyc=d(cyc), inb=d(inb))
    want = restate.merge_multi_h(flow.clamp(-1, 1), _score(m2[:, 0], cyc, inb), th, multiH)
    return got, want


def _assert_merge(got, want, what):
    for x, y, name in zip(got, want, ("flowGlobal", "matchGlobal", "binary")):
        assert x.shape == y.shape and _bits_equal(x, y), (what, name)


def test_merge_scores_exactly_on_the_threshold(dev):
    """``v >= th`` with v == th: a third of the products m * cyc are 0.25 exactly, half of those survive inb.  One ulp above,
    exactly those entries stop qualifying."""
    n, H, W = 7, 37, 53
    flow, m2, cyc, inb = _exact_inputs(n, H, W, 50)
    s = _score(m2[:, 0], cyc, inb)
    on = s == TH
    assert 0.12 < float(on[0].float().mean()) < 0.22 and 0.12 < float(on[1:].float().mean()) < 0.22      # expected 1/6
    # ... and the on-threshold entry is the one that decides: at homography 0, and at a later one after only smaller scores
    earlier_below = torch.cumsum((s >= TH).int(), 0) - (s >= TH).int() == 0
    deciders = on & earlier_below
    assert int(deciders[0].sum()) > 100 and int(deciders[1:].sum()) > 100
    assert TH < TH_NEXT < TH * (1 + 2e-7) and torch.equal((s >= TH) ^ (s >= TH_NEXT), on)
    for multiH in (True, False):
        for th in (TH, TH_NEXT):
            got, want = _merge_both(dev, flow, m2, cyc, inb, th, multiH)
            _assert_merge(got, want, (multiH, th))
        # the two thresholds differ at the deciders
        b0 = restate.merge_multi_h(flow.clamp(-1, 1), s, TH, multiH)[2]
        b1 = restate.merge_multi_h(flow.clamp(-1, 1), s, TH_NEXT, multiH)[2]
        assert int((b0 & ~b1).sum()) > 100 and not bool((b1 & ~b0).any())


@pytest.mark.parametrize("HW", [1, 255, 256, 257])
def test_merge_and_score_input_forms(dev, HW):
    """n = 1 and n = 7, multiH on and off, cyc / inb each present or absent, match12 as a channel slice (stride 2 HW) and
    contiguous, one pixel, one block less one, one block, one block plus one."""
    for n in (1, 7):
        flow, m2, cyc, inb = _exact_inputs(n, 1, HW, 60 + n)
        m2[:, 0, :, ::5] *= -1.0                                              # negative scores: -0.0 where inb is 0
        for c in (cyc, None):
            for b in (inb, None):
                for sliced in (True, False):
                    for multiH in (True, False):
                        got, want = _merge_both(dev, flow, m2, c, b, TH, multiH, sliced)
                        _assert_merge(got, want, (n, c is not None, b is not None, sliced, multiH))
                    m = m2.to(dev)[:, 0] if sliced else m2[:, 0].contiguous().to(dev)
                    sc = ops.match_score(m, cyc=None if c is None else c.to(dev), inb=None if b is None else b.to(dev))
                    assert _bits_equal(sc, _score(m2[:, 0], c, b)), (n, c is not None, b is not None, sliced)
    if HW == 257:
        s = _score(m2[:, 0], cyc, inb)
        assert bool(((s == 0) & torch.signbit(s)).any()) and bool(((s == 0) & ~torch.signbit(s)).any())


def test_merge_and_score_with_nan_scores(dev):
    """NaN >= th is false: a NaN score at homography 0 does not qualify, matchGlobal is the NaN and the owner 0 unless a later
    homography qualifies; a NaN score at a later homography is skipped.  NaN arrives through m, through cyc and as NaN * 0."""
    n, H, W = 5, 9, 31
    flow, m2, cyc, inb = _exact_inputs(n, H, W, 70)
    nan = float("nan")
    m2[0, 0, :3] = nan                        # homography 0, three rows: inb 0 and 1, later homographies qualifying or not
    m2[2, 0, 2:6] = nan
    cyc[1, 5:8, ::2] = nan
    cyc[0, 8, 10:20] = nan
    s = _score(m2[:, 0], cyc, inb)
    later = (s[1:] >= TH).any(0)
    assert bool((s[0].isnan() & later).any()) and bool((s[0].isnan() & ~later).any())
    assert bool((s[1:].isnan() & (inb[1:] == 0)).any())
    for multiH in (True, False):
        got, want = _merge_both(dev, flow, m2, cyc, inb, TH, multiH)
        _assert_merge(got, want, multiH)
        fg, mg, b = (x.cpu() for x in got)
        lost = s[0].isnan() & ~(later if multiH else torch.zeros_like(later))
        assert bool(mg[0][lost].isnan().all()) and not bool(b[0][lost].any())
        assert _bits_equal(fg[0][lost], flow[0].clamp(-1, 1)[lost])
        if multiH:
            assert not bool(mg[0][s[0].isnan() & later].isnan().any())
    sc = ops.match_score(m2.to(dev)[:, 0], cyc=cyc.to(dev), inb=inb.to(dev))
    assert _bits_equal(sc, s) and int(s.isnan().sum()) > 50


FLOW_EDGES = [1.0, -1.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 1.0 + 2.0 ** -22, -(1.0 + 2.0 ** -22), 1.0 - 2.0 ** -24,
              -(1.0 - 2.0 ** -24), 0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1e-45, -1e-45, 3.0e38, -3.0e38]


def test_merge_flow_at_and_beyond_the_clamp(dev):
    """flowGlobal = torch.clamp(flow_owner, -1, 1) bit for bit: +-1 and their neighbours, -0.0, +-inf -- and NaN, which
    torch.clamp keeps.  A NaN does reach this kernel from finite inputs (test_assemble_hands_on_the_nan_of_a_degenerate_homography),
    so the kernel keeps it too (until then it returned -1: fminf / fmaxf drop a NaN)."""
    e = torch.tensor(FLOW_EDGES)
    k = len(FLOW_EDGES)
    n, H, W = 2, k, k
    flow = torch.stack((e.view(k, 1).expand(k, k), e.view(1, k).expand(k, k)), dim=2)            # every pair (x, y)
    flow = torch.stack((flow, flow.flip(0, 1)))
    assert bool(torch.signbit(flow[0, 9, 9, 0])) and float(flow[0, 9, 9, 0]) == 0.0
    m = torch.tensor([0.5, 0.125])[(torch.arange(k * k) % 2).view(1, k, k)].expand(2, k, k).clone()
    m[1] = 0.75 - m[1]                                                                           # owner alternates 0 / 1
    got = ops.merge_multi_h(flow.to(dev), m.to(dev), TH, True)
    want = restate.merge_multi_h(torch.clamp(flow, -1, 1), m, TH, True)
    _assert_merge(got, want, "edges")
    fg = got[0].cpu()
    assert int(fg.isnan().sum()) == int(torch.clamp(flow, -1, 1).isnan()[0].sum()) > 0          # flip(0, 1) keeps the count
    assert float(fg[~fg.isnan()].abs().max()) == 1.0


def test_assemble_hands_on_the_nan_of_a_degenerate_homography(dev):
    """Can a NaN reach the merge through assemble()?  Yes, from finite inputs: compose_flow(clamp=True) pins a non-finite RESIDUAL
    flow, but the coarse grid is x'/z', y'/z', and a homography with z' = 0 inside the image puts 0/0 or x/0 there; sampling it
    hands the NaN on.  The reference (kornia's warper, F.grid_sample, torch.clamp) returns NaN at the pixels such a homography
    still owns, and so must the device.  Homography 0 is all zero (0/0 everywhere, no rounding involved), homography 1 the identity;
    every score of homography 1 is a multiple of 1/64 (up-sampled 1 | 0 steps, halved by the cycle check's zero padding on the
    border), th = 0.45 is none, so the owners are exact."""
    hd, wd = 4, 6
    H, W = hd * 8, wd * 8
    fd = np.zeros((2, 2, hd, wd), np.float32)
    pm = np.stack((np.zeros((3, 3), np.float32), np.eye(3, dtype=np.float32)))
    md = np.ones((2, 2, hd, wd), np.float32)
    md[1, 0, :, wd // 2:] = 0.0
    t = torch.from_numpy
    for cycle in (False, True):
        fg, mg, b = (x.cpu() for x in assemble.assemble(fd, pm, md, (H, W), 0.45, True, cycle, dev))
        rf, rm, rb = restate.assemble_flow(t(fd), t(pm), t(md), (H, W), 0.45, True, cycle)
        assert torch.equal(b, rb) and 0.4 < float(rb.float().mean()) <= 0.5 and not bool(rb[0, :, W // 2:].any())
        assert torch.equal(fg.isnan(), rf.isnan()) and bool(rf[~rb].isnan().all()) and not bool(rf[rb].isnan().any())
        assert float((fg[rb] - rf[rb]).abs().max()) <= TOL and float((mg[rb] - rm[rb]).abs().max()) <= TOL
        assert float(rm[~rb].abs().max()) == 0.0 and float(mg[~rb].abs().max()) == 0.0      # score_0 = match * in-bounds(NaN) = 0
