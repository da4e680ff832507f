"""The cycle-checked fine stage for all shape groups: ops.cycle_tail (rfx_cycle_tail_f32) against the four-kernel chain it fuses
(resize_bilinear -> compose_flow -> grid_sample -> match_score), the grouped forms AlignPipeline.pred_flow_mask_cycle_groups /
pred_flow_mask_kitti_groups / kitti_fine_round_groups against the one-group methods (which keep the four-kernel tail), and the
RFX_FINE_GROUPS switch of the ragged YFCC and KITTI drivers.

Every comparison is on bit patterns (NaN payloads included): there is no tolerance anywhere in this file.
"""
import numpy as np
import pytest
import torch

from rfx import ops, weights, synth
from rfx.pipeline import AlignPipeline

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAD = [float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 3e9, -3e9]


def _bits(a, b):
    """Bit equality of two float32 tensors (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _unit(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g).to(DEV)


def _homs(B, seed, far=None):
    g = torch.Generator().manual_seed(seed)
    H = torch.eye(3).repeat(B, 1, 1) + 0.05 * torch.randn(B, 3, 3, generator=g)
    H[:, 2, 2] = 1.0
    if far is not None:
        H[far, 0, 2] = 5.0                     # strongly out of bounds
    return H.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernel against the chain
def chain(fd, m12, m21, cg, out_hw=None):
    """The four-kernel tail as AlignPipeline.pred_flow_mask_lists(cycle=True) issues it -> (flow12, match (B,H,W), flowUp)."""
    B = fd.shape[0]
    H, W = cg.shape[1:3] if out_hw is None else out_hw
    m = ops.resize_bilinear(torch.cat((m12, m21), dim=0), (H, W), align_corners=False)
    flow12, inb, flowUp = ops.compose_flow(fd, cg, clamp=True, want_inb=True, want_flow_up=True, out_hw=(H, W))
    return flow12, ops.match_score(m[:B, 0], ops.grid_sample(m[B:], flowUp)[:, 0], inb), flowUp


# (B, /8 map, coarse grid, output)
CASES = {"yfcc": (2, (5, 7), (40, 56), (40, 56)),            # the YFCC form
         "kitti": (1, (3, 5), (24, 40), (19, 33)),           # the KITTI form: out_hw != grid, odd sizes
         "one_cell": (1, (1, 1), (8, 8), (8, 8)),            # every tap clamps to one cell
         "halves": (3, (7, 9), (56, 72), (56, 72))}          # width no multiple of 64; the match maps are halves of one tensor
FAMILIES = ("small", "pm3", "edge", "far", "huge", "nan_flow", "nan_m12", "nan_m21", "zero_one")


def _near_grid(B, Hc, Wc, seed):
    return ops.warp_grid(_homs(B, seed), Hc, Wc)


def _inputs(case, family, seed):
    """-> flowDown8 (B,2,hd,wd), match12Down8, match21Down8 (B,1,hd,wd), coarse grid (B,Hc,Wc,2), out_hw."""
    B, (hd, wd), (Hc, Wc), out = CASES[case]
    fd = _rand(B, 2, hd, wd, seed=seed, scale=0.05)                         # small residual flow: most pixels in bounds
    both = _unit(2 * B, 1, hd, wd, seed=seed + 1)
    cg = _near_grid(B, Hc, Wc, seed + 2)
    if family == "pm3":
        # +-3: the clamp puts flowUp at exactly +-1 inside the cells, taps fall outside the image
        fd = torch.where(_rand(B, 2, hd, wd, seed=seed + 3) > 0, 3.0, -3.0).to(torch.float32)
    elif family == "edge":
        # coarse-grid values of exactly +-1 in whole patches, and the corner cell at +-4: the upper left output pixels lie before the
        # first /8 cell centre, so their residual flow is exactly -3, flowUp exactly (-1, -1), the one tap inside the image is the
        # corner cell with weight 0.25 -> flow12 = (1, -1) exactly: the in-bounds comparisons at equality
        fd[:, :, 0, 0] = -3.0
        cg[:, : Hc // 2, : Wc // 3, 0] = 1.0
        cg[:, Hc // 3:, Wc // 2:, 1] = -1.0
        cg[:, 0, 0, 0], cg[:, 0, 0, 1] = 4.0, -4.0
    elif family in ("far", "huge"):
        Hm = _homs(B, seed + 4, far=B - 1)
        Hm[0, 2, 0] = 2.0                                                   # z' = 0 inside the image: huge / inf cells
        cg = ops.warp_grid(Hm, Hc, Wc)
        for k, v in enumerate(BAD):
            cg[k % B, (3 * k + 1) % Hc, (5 * k + 2) % Wc, k % 2] = v
        if family == "huge":
            # match12 * cycle overflows to inf BEFORE the in-bounds factor: out of bounds the chain gives inf * 0 = NaN, which a
            # product taken in another order would not
            both = both * 2e30 + 1e30
    elif family == "nan_flow":
        fd[B - 1, 1, hd // 2, wd // 2] = float("nan")
    elif family == "nan_m12":
        both[B - 1, 0, hd // 2, wd // 2] = float("nan")
    elif family == "nan_m21":
        both[2 * B - 1, 0, hd // 2, wd // 2] = float("nan")
    elif family == "zero_one":
        both = (both > 0.5).to(torch.float32)
    if case == "halves":
        m12, m21 = both[:B], both[B:]                                        # views: batch stride hd * wd, second one offset
    else:
        m12, m21 = both[:B].clone(), both[B:].clone()
    return fd, m12, m21, cg, (None if out == (Hc, Wc) else out)


@pytest.mark.parametrize("case", list(CASES))
def test_cycle_tail_equals_the_four_kernel_chain(case):
    B, _, _, (H, W) = CASES[case]
    seen = {}
    for i, family in enumerate(FAMILIES):
        fd, m12, m21, cg, out_hw = _inputs(case, family, 100 * i + 7)
        ref12, refm, ref_up = chain(fd, m12, m21, cg, out_hw)
        got12, gotm = ops.cycle_tail(fd, m12, m21, cg, out_hw=out_hw)
        torch.cuda.synchronize()
        assert tuple(got12.shape) == (B, H, W, 2) and tuple(gotm.shape) == (B, H, W)
        d12 = int((ref12.view(torch.int32) != got12.view(torch.int32)).sum())
        dm = int((refm.view(torch.int32) != gotm.view(torch.int32)).sum())
        print("%s / %s: differing words flow12 %d, match %d" % (case, family, d12, dm))
        assert _bits(got12, ref12), (case, family, "flow12", d12)
        assert _bits(gotm, refm), (case, family, "match", dm)
        seen[family] = (ref12, refm, ref_up)
    # the families did what they are for (on the chain's own results): nothing here can pass vacuously
    f12, m, up = seen["small"]
    assert float((m > 0).float().mean()) > 0.5 and float((up.abs() < 1).float().mean()) > 0.8
    f12, m, up = seen["pm3"]
    assert float((up.abs() == 1).float().mean()) > 0.3 and bool((m > 0).any())       # the clamp saturated: taps outside the image
    f12, m, up = seen["edge"]
    at_one = (f12[..., 0] == 1.0) & (f12[..., 1] == -1.0)
    assert bool(at_one[:, 0, 0].all()) and bool((m[at_one] > 0).all())       # equality counts as in bounds, and shows in match
    f12, m, up = seen["far"]
    assert not bool(torch.isfinite(f12).all()) and bool((m[B - 1] == 0).float().mean() > 0.9)
    # a NaN residual flow ends at the clamp (fminf / fmaxf drop it: flowUp is -1 there); a NaN matchability reaches match
    assert not bool(torch.isnan(seen["nan_flow"][2]).any())
    f12, m, up = seen["huge"]
    assert bool(torch.isnan(m[B - 1]).any()) and bool(torch.isinf(m).any() or B == 1)
    for family in ("nan_m12", "nan_m21"):
        assert bool(torch.isnan(seen[family][1]).any()), family
    f12, m, up = seen["zero_one"]
    if case != "one_cell":                                                   # (one cell: one value per map)
        assert bool((m == 0).any()) and bool((m > 0).any())


def test_cycle_tail_out_buffers_and_refusals():
    fd, m12, m21, cg, _ = _inputs("halves", "small", 3)
    B, H, W = 3, 56, 72
    ref12, refm, _ = chain(fd, m12, m21, cg)
    buf12 = torch.full((6 + B * H * W * 2,), -7.0, device=DEV)             # (flow12 is written as float2: an even offset)
    bufm = torch.full((B * H * W + 9,), -7.0, device=DEV)
    got12, gotm = ops.cycle_tail(fd, m12, m21, cg, flow12_out=buf12[6:].view(B, H, W, 2), match_out=bufm[:B * H * W].view(B, H, W))
    assert got12.data_ptr() == buf12[6:].data_ptr() and gotm.data_ptr() == bufm.data_ptr()
    assert _bits(got12, ref12) and _bits(gotm, refm)
    assert bool((buf12[:6] == -7.0).all()) and bool((bufm[B * H * W:] == -7.0).all())             # nothing outside the views
    with pytest.raises(RuntimeError):
        ops.cycle_tail(fd.cpu(), m12, m21, cg)
    with pytest.raises(TypeError):
        ops.cycle_tail(fd.double(), m12, m21, cg)
    with pytest.raises(ValueError):
        ops.cycle_tail(fd, m12[:2], m21, cg)
    with pytest.raises(ValueError):
        ops.cycle_tail(fd, m12, m21.transpose(2, 3), cg)
    with pytest.raises(ValueError):
        ops.cycle_tail(fd, m12, m21, cg[:2])
    with pytest.raises(ValueError):
        ops.cycle_tail(fd, m12, m21, cg, match_out=torch.empty((B, H, W + 1), device=DEV))


def test_cycle_tail_is_recorded_in_a_launch_group():
    # 1024 x 2049 outputs = 8197 blocks of 256, above the 8192-block cap, next to two small problems: each strides by its own grid
    big = (_rand(1, 2, 8, 8, seed=0, scale=0.05), _unit(1, 1, 8, 8, seed=1), _unit(1, 1, 8, 8, seed=2), _near_grid(1, 64, 64, 3), (1024, 2049))
    probs = [big, _inputs("kitti", "pm3", 5), _inputs("halves", "far", 6)]
    alone = [ops.cycle_tail(*p[:4], out_hw=p[4]) for p in probs]
    ref_big = chain(*big[:4], big[4])
    n0 = ops.group_stats()
    with ops.launch_group(DEV, False):
        got = [ops.cycle_tail(*p[:4], out_hw=p[4]) for p in probs]
    n1 = ops.group_stats()
    torch.cuda.synchronize()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 1)
    for i, (a, g) in enumerate(zip(alone, got)):
        assert _bits(a[0], g[0]) and _bits(a[1], g[1]), i
    assert _bits(alone[0][0], ref_big[0]) and _bits(alone[0][1], ref_big[1])


# ------------------------------------------------------------------------------------------------ 2. groups
def _sds():
    return dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
                match=weights.net_matchability_sd(3, last_std=3.0))


@pytest.fixture(scope="module")
def pipe():
    return AlignPipeline(_sds(), nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant="B", device=DEV, seed=5,
                         degenerate="device")


# (B, target h, w, source h, w): /8 widths 8, 10, 6, 9 -- three of them are padded for the correlation
FINE = [(2, 48, 64, 40, 56), (1, 64, 80, 72, 64), (1, 80, 48, 64, 64), (3, 56, 72, 48, 80)]
PACKED = ("match", "flowDown8", "match12Down8", "match21Down8")


def _fine_inputs():
    Is = [_rand(B, 3, sh, sw, seed=i) for i, (B, h, w, sh, sw) in enumerate(FINE)]
    It = [_rand(B, 3, h, w, seed=10 + i) for i, (B, h, w, sh, sw) in enumerate(FINE)]
    Hs = [_homs(B, 20 + i, far=(B - 1 if i == 3 else None)) for i, (B, h, w, sh, sw) in enumerate(FINE)]
    return Is, It, Hs, [(h, w) for _, h, w, _, _ in FINE]


def _check_groups(alone, call):
    """``call(sub, out)`` runs the grouped form on the groups ``sub``: all four equal ``alone`` on every key and in the packed
    buffers; groups {0, 3} issue as many grouped launches as all four; one group issues none."""
    packed = {}
    n0 = ops.group_stats()[1]
    got = call([0, 1, 2, 3], packed)
    n4 = ops.group_stats()[1] - n0
    torch.cuda.synchronize()
    for g in range(4):
        assert set(got[g]) == set(alone[g])
        for key in alone[g]:
            assert _bits(got[g][key], alone[g][key]), (g, key)
    for key in PACKED:
        assert packed[key].dim() == 1 and _bits(packed[key], torch.cat([a[key].reshape(-1) for a in alone])), key
    assert packed["layout"]["total"] == sum(a["match"].numel() for a in alone)
    # groups 0 and 3 use between them every kernel instance the four do (tests/test_gpu_fine_groups.py::test_pred_flow_mask_groups)
    n0 = ops.group_stats()[1]
    got2 = call([0, 3], None)
    n2 = ops.group_stats()[1] - n0
    print("grouped launches: 4 groups %d, 2 groups %d" % (n4, n2))
    assert all(_bits(got2[k][key], alone[g][key]) for k, g in enumerate([0, 3]) for key in alone[g])
    assert n4 == n2 and n4 > 0, (n4, n2)
    for g in (0, 3):
        packed = {}
        n0 = ops.group_stats()
        one = call([g], packed)
        assert ops.group_stats() == n0                                      # zero grouped launches
        assert len(one) == 1 and all(_bits(one[0][key], alone[g][key]) for key in alone[g])
        for key in PACKED:
            assert packed[key].dim() == 1 and _bits(packed[key], alone[g][key].reshape(-1)), (g, key)


def test_pred_flow_mask_cycle_groups(pipe):
    Is, It, Hs, hw = _fine_inputs()
    featt = [ops.l2norm(pipe.feat(t)) for t in It]
    alone = [pipe.pred_flow_mask_cycle(Is[g], featt[g], ops.warp_grid(Hs[g], *hw[g])) for g in range(4)]
    # the far homography leaves (almost) nothing in bounds, the near ones do
    assert float((alone[3]["match"][2] == 0).float().mean()) > 0.9 and float((alone[0]["match"] > 0).float().mean()) > 0.5
    pick = lambda xs, sub: [xs[g] for g in sub]
    _check_groups(alone, lambda sub, out: pipe.pred_flow_mask_cycle_groups(pick(Is, sub), pick(featt, sub), pick(Hs, sub), pick(hw, sub),
                                                                           out=out))


@pytest.mark.parametrize("shrink", [None, (3, 7)])
def test_pred_flow_mask_kitti_groups(pipe, shrink):
    _, It, Hs, hw = _fine_inputs()
    IsS = [_rand(B, 3, h, w, seed=30 + i) for i, (B, h, w, _, _) in enumerate(FINE)]
    fcs = [ops.warp_grid(Hs[g], *hw[g]) for g in range(4)]
    out_hw = [None if shrink is None else (h - shrink[0], w - shrink[1]) for h, w in hw]          # 45x57, 61x73, 77x41, 53x65
    alone = [pipe.pred_flow_mask_kitti(IsS[g], It[g], fcs[g], out_hw=out_hw[g]) for g in range(4)]
    for g in range(4):
        assert tuple(alone[g]["match"].shape[2:]) == (hw[g] if shrink is None else out_hw[g])
    assert float((alone[0]["match"] > 0).float().mean()) > 0.5
    pick = lambda xs, sub: [xs[g] for g in sub]
    _check_groups(alone, lambda sub, out: pipe.pred_flow_mask_kitti_groups(pick(IsS, sub), pick(It, sub), pick(fcs, sub),
                                                                           out_hw_list=None if shrink is None else pick(out_hw, sub),
                                                                           out=out))


def test_cycle_lists_of_several_groups_still_refused(pipe):
    Is, It, Hs, hw = _fine_inputs()
    fcs = [ops.warp_grid(Hs[g], *hw[g]) for g in (0, 1)]
    featt = [ops.l2norm(pipe.feat(It[g])) for g in (0, 1)]
    with pytest.raises(ValueError, match="one shape group"):
        pipe.pred_flow_mask_lists(featt, featt, fcs, cycle=True)


# ------------------------------------------------------------------------------------------------ 3. the KITTI round
# (B, source, d2 target, resize target, original)
KITTI_ROUND = [(2, (40, 104), (48, 112), (96, 224), (45, 110)), (1, (48, 96), (40, 96), (80, 192), (43, 97))]


def test_kitti_fine_round_groups(pipe):
    Hs = [_homs(B, 40 + i) for i, (B, *_) in enumerate(KITTI_ROUND)]
    Ts = [_rand(B, 3, *s, seed=50 + i) for i, (B, s, _, _, _) in enumerate(KITTI_ROUND)]
    Td2 = [_rand(B, 3, *d, seed=60 + i) for i, (B, _, d, _, _) in enumerate(KITTI_ROUND)]
    Tr = [_rand(B, 3, *r, seed=70 + i) for i, (B, _, _, r, _) in enumerate(KITTI_ROUND)]
    org = [k[4] for k in KITTI_ROUND]
    alone = [pipe.kitti_fine_round(Hs[g], Ts[g], Td2[g], Tr[g], org[g], cc_th=0) for g in range(2)]
    packed = {}
    n0 = ops.group_stats()[1]
    got = pipe.kitti_fine_round_groups(Hs, Ts, Td2, Tr, org, out=packed)
    n2 = ops.group_stats()[1] - n0
    torch.cuda.synchronize()
    assert n2 > 0
    for g in range(2):
        (fa, pa, ma), (fg, pg, mg) = alone[g], got[g]
        assert tuple(ma.shape) == (KITTI_ROUND[g][0],) + org[g] and float((ma > 0).float().mean()) > 0.2
        assert _bits(fg, fa), (g, "flow_d2")
        assert set(pg) == set(pa) and all(_bits(pg[key], pa[key]) for key in pa), g
        assert _bits(mg, ma), (g, "match")
    for key in PACKED:
        assert _bits(packed[key], torch.cat([a[1][key].reshape(-1) for a in alone])), key
    assert _bits(packed["flowD2"], torch.cat([a[0].reshape(-1) for a in alone]))
    # one group: the eager launches
    n0 = ops.group_stats()
    one = pipe.kitti_fine_round_groups(Hs[1:], Ts[1:], Td2[1:], Tr[1:], org[1:])
    assert ops.group_stats() == n0
    assert _bits(one[0][0], alone[1][0]) and _bits(one[0][2], alone[1][2]) and all(_bits(one[0][1][k], alone[1][1][k]) for k in alone[1][1])


# ------------------------------------------------------------------------------------------------ 4. drivers
def _up(im):
    return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(DEV)


def _same_outputs(on, off, keys):
    for b, (o, p) in enumerate(zip(on, off)):
        assert o["nbH"] == p["nbH"] and o["mask"].shape == p["mask"].shape and torch.equal(o["mask"], p["mask"]), b
        for key in keys:
            assert len(o[key]) == len(p[key]) == o["nbH"], (b, key)
            assert all(x.shape == y.shape and _bits(x, y) for x, y in zip(o[key], p[key])), (b, key)


def test_variant_c_lists_fine_groups_switch(monkeypatch):
    """multi_h_variant_c on lists: 3 pairs, 2 shapes, 2 candidates each (the target as stored and turned by 180 degrees)."""
    pipe = AlignPipeline(_sds(), nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant="C", device=DEV, seed=5,
                         degenerate="device")
    pairs = []
    for seed, H, W, dw in ((80, 240, 320, 0), (82, 256, 320, 16), (81, 240, 320, 0)):
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
        pairs.append((I1, I2.crop((0, 0, W - dw, H))))
    src, tgt = [_up(p[0]) for p in pairs], [_up(p[1]) for p in pairs]
    cands = [[torch.rot90(t, k, (0, 1)).contiguous() for t in tgt] for k in (0, 2)]
    assert len({(tuple(s.shape), tuple(t.shape)) for s, t in zip(src, tgt)}) == 2

    def run(flag):
        monkeypatch.setenv("RFX_FINE_GROUPS", flag)
        n0 = ops.group_stats()[1]
        outs = pipe.multi_h_variant_c(src, cands, maxCoarse=2, maskRegionTh=0.03, pair_ids=[100, 107, 114], split=1)
        torch.cuda.synchronize()
        return outs, ops.group_stats()[1] - n0

    off, n_off = run("0")
    on, n_on = run("1")
    nbh = [o["nbH"] for o in off]
    print("variant C: nbH %s, grouped launches RFX_FINE_GROUPS=0 %d, =1 %d" % (nbh, n_off, n_on))
    # some pair accepts a homography; all pairs are active in the first round and the accepted ones in the second: two fine groups
    # (two (source, target) shapes) run in one round
    assert max(nbh) >= 1
    assert len({tuple(o["mask"].shape) for o in off}) == 2
    _same_outputs(on, off, ("H", "flowDown8", "matchDown8"))
    assert [o["candidate"] for o in on] == [o["candidate"] for o in off]
    assert n_on > n_off


def test_kitti_lists_fine_groups_switch(monkeypatch):
    """multi_h_kitti_batched on lists: 3 pairs of 2 sizes, traced: the pre-filter match maps the trace shows are equal too."""
    pipe = AlignPipeline(_sds(), nbScale=3, nbIter=300, tolerance=0.05, minSize=160, scaleR=1.2, variant="B", device=DEV, seed=7,
                         degenerate="device")
    pairs = []
    for seed, H, W, amp in ((11, 96, 312, 0.03), (30, 94, 311, 0.08), (33, 96, 312, 0.08)):
        pairs.append(synth.make_pair(H, W, seed=seed, homography=True, amp=amp))
    src, tgt = [_up(p[0]) for p in pairs], [_up(p[1]) for p in pairs]
    assert len({(tuple(s.shape), tuple(t.shape)) for s, t in zip(src, tgt)}) == 2

    def run(flag):
        monkeypatch.setenv("RFX_FINE_GROUPS", flag)
        trace = []
        n0 = ops.group_stats()[1]
        outs = pipe.multi_h_kitti_batched(src, tgt, fineSize=200, maskRegionTh=0.005, cc_th=0.01, pair_ids=[40, 30, 33], split=1,
                                          trace=trace)
        torch.cuda.synchronize()
        return outs, trace, ops.group_stats()[1] - n0

    off, t_off, n_off = run("0")
    on, t_on, n_on = run("1")
    nbh = [o["nbH"] for o in off]
    print("KITTI: nbH %s, rounds %d, grouped launches RFX_FINE_GROUPS=0 %d, =1 %d" % (nbh, len(t_off), n_off, n_on))
    assert max(nbh) >= 1
    shape_of = lambda b: (tuple(src[b].shape), tuple(tgt[b].shape))
    assert any(len({shape_of(b) for b in e["active"]}) == 2 for e in t_off)          # a round with two fine groups active
    _same_outputs(on, off, ("H", "flowD2", "flowDown8", "matchDown8"))
    assert len(t_on) == len(t_off)
    filtered = 0
    for e1, e0 in zip(t_on, t_off):
        assert list(e1["active"]) == list(e0["active"])
        for k in range(len(e0["active"])):
            assert all(_bits(e1["pm"][k][key], e0["pm"][k][key]) for key in e0["pm"][k]), ("pm", k)
            assert _bits(e1["match"][k], e0["match"][k]) and _bits(e1["flowD2"][k], e0["flowD2"][k]), k
            filtered += int((e1["match"][k] != e1["pm"][k]["match"][0, 0]).sum())
    assert filtered > 0                       # the filter removed something, and PredFlowMask's own map still shows it
    assert n_on > n_off
