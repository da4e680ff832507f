"""Grouped forms of the fine-stage kernels (ops.launch_group over warp_grid, grid_sample, compose_flow, the FeatureExtractor stem,
blurpool, l2norm, flow_head, resize_bilinear and the 7x7 correlation), the grouped forwards of the FeatureExtractor and the two
heads, AlignPipeline.pred_flow_mask_groups / fine_quickstart_groups, and the RFX_FINE_GROUPS switch of the ragged drivers.  Every
chain is one body over lists (ops.stage): the grouped calls are compared with the same body at list length one, which must launch
eagerly (no grouped launch).

Everything is compared bit for bit (no tolerance) with the same op / net / method called on each problem alone.  The grid-stride
kernels get one problem whose own grid is above the 8192-block cap next to a tiny one: a body that strode by the launch's gridDim.x
(the largest problem's) instead of the problem's own grid would write pixels twice or skip them.
"""
import numpy as np
import pytest
import torch

from rfx import ops, weights, synth
from rfx.nets import FeatureExtractorNet, NetFlowCoarseNet, NetMatchabilityNet
from rfx.pipeline import AlignPipeline

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAD = [float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 3e9, -3e9]


def _bits(a, b):
    """Bit equality of two float32 tensors (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return _bits(a, b)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _grouped(fn, problems):
    """-> (outputs of fn on every problem alone, outputs recorded in ONE launch_group, launches that group issued)."""
    alone = [fn(*p) for p in problems]
    n0 = ops.group_stats()[1]
    with ops.launch_group(DEV, False):
        got = [fn(*p) for p in problems]
    n1 = ops.group_stats()[1]
    torch.cuda.synchronize()
    return alone, got, n1 - n0


def _check(fn, problems, nine):
    """3 problems of different shapes in one group equal the op alone; 9 problems (two chunks) issue 2 launches and are equal too."""
    alone, got, n = _grouped(fn, problems)
    for i, (a, g) in enumerate(zip(alone, got)):
        assert _same(a, g), ("problem", i)
    assert n == 1
    alone, got, n = _grouped(fn, nine)
    assert len(nine) == 9 and n == 2, n
    for i, (a, g) in enumerate(zip(alone, got)):
        assert _same(a, g), ("nine", i)


def _homs(B, seed, far=None):
    g = torch.Generator().manual_seed(seed)
    H = torch.eye(3).repeat(B, 1, 1) + 0.05 * torch.randn(B, 3, 3, generator=g)
    H[:, 2, 2] = 1.0
    if far is not None:
        H[far, 0, 2] = 5.0                     # strongly out of bounds
    return H.to(DEV)


def _bad_grid(N, h, w, seed):
    """A sampling grid in about [-1.3, 1.3] with NaN / +-inf / huge cells."""
    g = _rand(N, h, w, 2, seed=seed, scale=0.65)
    for k, v in enumerate(BAD):
        g[k % N, (3 * k + 1) % h, (5 * k + 2) % w, k % 2] = v
    return g


# ------------------------------------------------------------------------------------------------ 1. ops
def test_warp_grid_group():
    # 1 x 1024 x 2049 = 2 098 176 pixels: 8197 blocks of 256, capped at 8192
    _check(lambda H, h, w: ops.warp_grid(H, h, w), [(_homs(1, 0), 1024, 2049), (_homs(3, 1, far=1), 5, 7), (_homs(2, 2), 48, 61)],
           [(_homs(1 + k % 3, 10 + k), 9 + k, 17 - k) for k in range(9)])


def test_grid_sample_group():
    def prob(N, C, Hi, Wi, Ho, Wo, seed):
        return _rand(N, C, Hi, Wi, seed=seed), _bad_grid(N, Ho, Wo, seed + 100)
    _check(lambda x, g: ops.grid_sample(x, g), [prob(1, 1, 8, 8, 1024, 2049, 0), prob(2, 3, 5, 7, 3, 5, 1), prob(3, 2, 33, 21, 40, 57, 2)],
           [prob(1 + k % 3, 1 + k % 2, 7 + k, 9, 11, 6 + k, 10 + k) for k in range(9)])


@pytest.mark.parametrize("clamp", [False, True])
def test_compose_flow_group(clamp):
    def prob(N, hd, wd, H, W, seed):
        fd = _rand(N, 2, hd, wd, seed=seed, scale=0.3)
        for k, v in enumerate(BAD):
            fd[k % N, k % 2, (2 * k + 1) % hd, (3 * k + 1) % wd] = v
        return fd, _bad_grid(N, H, W, seed + 50)
    fn = lambda fd, cg: ops.compose_flow(fd, cg, clamp=clamp, want_inb=True, want_flow_up=True)
    _check(fn, [prob(1, 8, 8, 1024, 2049, 0), prob(2, 2, 3, 5, 7, 1), prob(3, 6, 8, 48, 64, 2)],
           [prob(1 + k % 2, 3, 4, 20 + k, 31 - k, 10 + k) for k in range(9)])


def test_blurpool_group():
    # 1449 x 1449 outputs at stride 1 = 2 099 601 > 8192 * 256
    fn = lambda x, s: ops.blurpool2d(x, s)
    _check(fn, [(_rand(1, 1, 1449, 1449, seed=0), 1), (_rand(2, 3, 5, 7, seed=1), 2), (_rand(3, 2, 33, 40, seed=2), 2)],
           [(_rand(1 + k % 3, 2, 9 + k, 12, seed=10 + k), 1 + k % 2) for k in range(9)])


def test_resize_bilinear_group():
    # 2 x 1025 x 1024 = 2 099 200 outputs > 8192 * 256
    fn = lambda x, size, ac: ops.resize_bilinear(x, size, align_corners=ac)
    _check(fn, [(_rand(1, 2, 8, 8, seed=0), (1025, 1024), True), (_rand(2, 1, 3, 5, seed=1), (7, 4), False),
                (_rand(3, 2, 6, 8, seed=2), (48, 64), True)],
           [(_rand(1 + k % 2, 1, 5, 6 + k, seed=10 + k), (13 + k, 21), bool(k % 2)) for k in range(9)])


def test_flow_head_group():
    # 725 x 724 = 524 900 pixels > 8192 * 64
    fn = lambda x: ops.flow_head(x, 7)
    _check(fn, [(_rand(1, 49, 725, 724, seed=0, scale=3.0),), (_rand(2, 49, 3, 5, seed=1, scale=3.0),), (_rand(3, 49, 30, 41, seed=2, scale=3.0),)],
           [(_rand(1 + k % 3, 49, 6 + k, 9, seed=10 + k, scale=3.0),) for k in range(9)])


def test_l2norm_group_both_kernels():
    fn = lambda x: ops.l2norm(x)
    # the one-wavefront kernel (C = 3): 725 x 724 pixels > 8192 * 64
    _check(fn, [(_rand(1, 3, 725, 724, seed=0),), (_rand(2, 5, 3, 5, seed=1),), (_rand(3, 30, 17, 23, seed=2),)],
           [(_rand(1 + k % 3, 3 + k, 6 + k, 9, seed=10 + k),) for k in range(9)])
    # the four-wavefront kernel (C % 4 == 0, C >= 32): one workgroup per 64 pixels, several LDS blocks of channels at C = 256
    _check(fn, [(_rand(2, 256, 21, 23, seed=3),), (_rand(1, 32, 3, 5, seed=4),), (_rand(3, 36, 9, 15, seed=5),)],
           [(_rand(1 + k % 3, 32 + 4 * k, 6 + k, 9, seed=20 + k),) for k in range(9)])
    # one group with both kernels: two launches
    alone, got, n = _grouped(fn, [(_rand(1, 3, 9, 11, seed=6),), (_rand(2, 64, 7, 9, seed=7),)])
    assert n == 2 and all(_same(a, g) for a, g in zip(alone, got))


def test_stem_conv_maxblur_group():
    net = FeatureExtractorNet(weights.feature_extractor_sd(1), DEV)
    fn = lambda x: ops.stem_conv_maxblur(x, net.conv1)
    _check(fn, [(_rand(2, 3, 48, 64, seed=0),), (_rand(1, 3, 9, 11, seed=1),), (_rand(3, 3, 57, 71, seed=2),)],
           [(_rand(1 + k % 2, 3, 12 + k, 30 - k, seed=10 + k),) for k in range(9)])


def test_corr_plain_kernel_group():
    # widths that are no multiple of 4 with an explicit variant 0: the plain kernel; 1025 x 2049 pixels > 8192 * 256
    fn = lambda x, y: ops.corr_neigh(x, y, variant=0)
    def prob(N, C, H, W, seed):
        return _rand(N, C, H, W, seed=seed), _rand(N, C, H, W, seed=seed + 1)
    _check(fn, [prob(1, 2, 1025, 2049, 0), prob(2, 8, 3, 5, 2), prob(3, 8, 7, 10, 4)], [prob(1 + k % 2, 4, 5 + k, 9, 10 + 2 * k) for k in range(9)])


# ------------------------------------------------------------------------------------------------ 2. correlation
CORR = [(2, 6, 8), (1, 10, 12), (3, 7, 10), (128, 16, 48)]     # (N, H, W) at C = 8; the last one goes to a tuned 48-column tile


def _corr_inputs():
    return ([_rand(N, 8, H, W, seed=2 * i) for i, (N, H, W) in enumerate(CORR)],
            [_rand(N, 8, H, W, seed=2 * i + 1) for i, (N, H, W) in enumerate(CORR)])


def test_corr_groups_equal_alone_and_split_by_variant():
    xs, ys = _corr_inputs()
    alone2 = [ops.corr_neigh_bidir(x, y) for x, y in zip(xs, ys)]
    alone1 = [ops.corr_neigh(x, y) for x, y in zip(xs, ys)]
    for i, (x, y) in enumerate(zip(xs, ys)):                       # every variant is the reference of the others (existing tests hold that)
        assert _bits(alone2[i][0], alone1[i]) and _bits(alone2[i][1], ops.corr_neigh(y, x)), i
    n0 = ops.group_stats()[1]
    got2 = ops.corr_neigh_bidir_group(xs, ys)
    n1 = ops.group_stats()[1]
    got1 = ops.corr_neigh_group(xs, ys)
    n2 = ops.group_stats()[1]
    torch.cuda.synchronize()
    for i in range(len(CORR)):
        assert _same(got2[i], alone2[i]), ("bidir", i)
        assert _bits(got1[i], alone1[i]), ("one", i)
    # the three 16x16-tile problems share a launch, the tuned problem has its own
    assert n1 - n0 == 2 and n2 - n1 == 2, (n1 - n0, n2 - n1)
    # with caller buffers (padded width included)
    outs = [torch.empty((2 * N, 49, H, W), dtype=torch.float32, device=DEV) for N, H, W in CORR]
    ops.corr_neigh_bidir_group(xs, ys, outs=outs)
    for i, (N, H, W) in enumerate(CORR):
        assert _bits(outs[i][:N], alone2[i][0]) and _bits(outs[i][N:], alone2[i][1]), ("outs", i)


def test_corr_nine_problems_two_chunks():
    xs = [_rand(1 + k % 2, 8, 5 + k, 8, seed=k) for k in range(9)]
    ys = [_rand(1 + k % 2, 8, 5 + k, 8, seed=50 + k) for k in range(9)]
    alone = [ops.corr_neigh_bidir(x, y) for x, y in zip(xs, ys)]
    n0 = ops.group_stats()[1]
    got = ops.corr_neigh_bidir_group(xs, ys)
    assert ops.group_stats()[1] - n0 == 2
    assert all(_same(a, g) for a, g in zip(alone, got))


def test_corr_bidir_inside_group_with_ragged_width_raises():
    x, y = _rand(3, 8, 7, 10, seed=0), _rand(3, 8, 7, 10, seed=1)
    with pytest.raises(RuntimeError, match="corr_neigh_bidir_group"):
        with ops.launch_group(DEV, False):
            ops.corr_neigh_bidir(x, y)
    with pytest.raises(RuntimeError, match="corr_neigh_group"):
        with ops.launch_group(DEV, False):
            ops.corr_neigh(x, y)
    assert _same(ops.corr_neigh_bidir_group([x], [y])[0], ops.corr_neigh_bidir(x, y))      # the recorder is usable again


def test_corr_odd_width_alone_is_the_one_problem_group():
    # width 10: padded to 12 and cropped by the ONE implementation; alone it launches eagerly
    x, y = _rand(3, 8, 7, 10, seed=0), _rand(3, 8, 7, 10, seed=1)
    n0 = ops.group_stats()
    a1, g1 = ops.corr_neigh(x, y), ops.corr_neigh_group([x], [y])[0]
    a2, g2 = ops.corr_neigh_bidir(x, y), ops.corr_neigh_bidir_group([x], [y])[0]
    assert ops.group_stats() == n0
    assert tuple(a1.shape) == (3, 49, 7, 10) and _bits(a1, g1) and _same(a2, g2)
    assert _bits(a2[0], a1) and _bits(a2[1], ops.corr_neigh(y, x))


# ------------------------------------------------------------------------------------------------ 2b. the stage helper
def test_stage_one_row_is_eager_and_rows_are_one_group():
    probs = [(_rand(1, 3, 9, 11, seed=6),), (_rand(2, 64, 7, 9, seed=7),), (_rand(3, 36, 9, 15, seed=5),)]
    calls = []

    def fn(x):
        calls.append(ops.launch_group.recording())
        return ops.l2norm(x)
    n0 = ops.group_stats()
    one = ops.stage(fn, [probs[1][0]], device=DEV, side_streams=False)
    assert ops.group_stats() == n0 and calls == [False]                    # no group opened, no grouped launch
    assert len(one) == 1 and _bits(one[0], ops.l2norm(probs[1][0]))
    alone, ref, n_ref = _grouped(ops.l2norm, probs)
    n0 = ops.group_stats()
    got = ops.stage(fn, [p[0] for p in probs], device=DEV, side_streams=False)
    n1 = ops.group_stats()
    torch.cuda.synchronize()
    assert calls[1:] == [True] * 3
    assert n1[0] - n0[0] == 1 and n1[1] - n0[1] == n_ref == 2, (n0, n1, n_ref)       # the one- and the four-wavefront kernel
    assert all(_bits(a, g) for a, g in zip(alone, got))
    with pytest.raises(ValueError):
        ops.stage(lambda a, b: a, [1, 2], [1], device=DEV)


# ------------------------------------------------------------------------------------------------ 3. nets
NET_IN = [(2, 3, 48, 64), (1, 3, 64, 80), (1, 3, 80, 48), (3, 3, 56, 72)]


def test_feature_extractor_forward_group():
    net = FeatureExtractorNet(weights.feature_extractor_sd(1), DEV)
    xs = [_rand(*s, seed=i) for i, s in enumerate(NET_IN)]
    alone = [net(x) for x in xs]
    got = net.forward_group(xs, False)
    torch.cuda.synchronize()
    for i, (a, g) in enumerate(zip(alone, got)):
        assert tuple(a.shape) == (NET_IN[i][0], 256, NET_IN[i][2] // 8, NET_IN[i][3] // 8)
        assert _bits(a, g), i
    assert all(_bits(a, g) for a, g in zip(alone, net.forward_group(xs)))                 # with side streams


@pytest.mark.parametrize("up8X", [False, True])
def test_heads_forward_group(up8X):
    flow = NetFlowCoarseNet(weights.net_flow_coarse_sd(2), 7, DEV)
    match = NetMatchabilityNet(weights.net_matchability_sd(3, last_std=3.0), 7, DEV)
    vols = [_rand(N, 49, H // 8, W // 8, seed=i) for i, (N, _, H, W) in enumerate(NET_IN)]
    for net in (flow, match):
        alone = [net(v, up8X) for v in vols]
        got = net.forward_group(vols, up8X, False)
        torch.cuda.synchronize()
        for i, (a, g) in enumerate(zip(alone, got)):
            assert _bits(a, g), (type(net).__name__, i)


def test_forward_group_of_one_input_is_the_eager_call():
    x = _rand(*NET_IN[0], seed=0)
    v = _rand(NET_IN[0][0], 49, NET_IN[0][2] // 8, NET_IN[0][3] // 8, seed=0)
    feat = FeatureExtractorNet(weights.feature_extractor_sd(1), DEV)
    flow = NetFlowCoarseNet(weights.net_flow_coarse_sd(2), 7, DEV)
    match = NetMatchabilityNet(weights.net_matchability_sd(3, last_std=3.0), 7, DEV)
    n0 = ops.group_stats()
    got = feat.forward_group([x])
    assert len(got) == 1 and _bits(got[0], feat(x))
    for net in (flow, match):
        for up8X in (False, True):
            got = net.forward_group([v], up8X)
            assert len(got) == 1 and _bits(got[0], net(v, up8X)), (type(net).__name__, up8X)
    assert ops.group_stats() == n0


# ------------------------------------------------------------------------------------------------ 4. pipeline
def _pipe():
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    return AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant="B", device=DEV, seed=5,
                         degenerate="device")


@pytest.fixture(scope="module")
def pipe():
    return _pipe()


# (B, target h, w, source h, w): /8 widths 8, 10, 6, 9 -- three of them are padded for the correlation
FINE = [(2, 48, 64, 40, 56), (1, 64, 80, 72, 64), (1, 80, 48, 64, 64), (3, 56, 72, 48, 80)]


def _fine_inputs(pipe):
    Is = [_rand(B, 3, sh, sw, seed=i) for i, (B, h, w, sh, sw) in enumerate(FINE)]
    It = [_rand(B, 3, h, w, seed=10 + i) for i, (B, h, w, sh, sw) in enumerate(FINE)]
    Hs = [_homs(B, 20 + i, far=(B - 1 if i == 3 else None)) for i, (B, h, w, sh, sw) in enumerate(FINE)]
    return Is, It, Hs, [(h, w) for _, h, w, _, _ in FINE]


def test_pred_flow_mask_groups(pipe):
    Is, It, Hs, hw = _fine_inputs(pipe)
    featt = [ops.l2norm(pipe.feat(t)) for t in It]
    alone = [pipe.pred_flow_mask(Is[g], featt[g], ops.warp_grid(Hs[g], *hw[g])) for g in range(4)]
    packed = {}
    n0 = ops.group_stats()[1]
    got = pipe.pred_flow_mask_groups(Is, featt, Hs, hw, out=packed)
    n4 = ops.group_stats()[1] - n0
    torch.cuda.synchronize()
    for g in range(4):
        assert set(got[g]) == set(alone[g])
        for key in alone[g]:
            assert _bits(got[g][key], alone[g][key]), (g, key)
    for key in ("match", "flowDown8", "match12Down8", "match21Down8"):
        assert _bits(packed[key], torch.cat([a[key].reshape(-1) for a in alone])), key
    # the far homography leaves (almost) nothing in bounds, the near ones do
    assert float((alone[3]["match"][2] == 0).float().mean()) > 0.9 and float((alone[0]["match"] > 0).float().mean()) > 0.5
    # the number of launches does not depend on the number of groups (<= 8): one launch per stage and kernel instance.  The 2-group
    # call takes groups 0 and 3, which between them use every kernel instance the four do: the 7x9 map of group 3 (63 pixels, no
    # multiple of 4) takes the scalar-load instance of the strided blocks' 1x1 shortcut convolution, the other three the vector one
    sub = [0, 3]
    pick = lambda xs: [xs[g] for g in sub]
    n0 = ops.group_stats()[1]
    got2 = pipe.pred_flow_mask_groups(pick(Is), pick(featt), pick(Hs), pick(hw))
    n2 = ops.group_stats()[1] - n0
    print("grouped launches: 4 groups %d, 2 groups %d" % (n4, n2))
    assert all(_bits(got2[k][key], alone[g][key]) for k, g in enumerate(sub) for key in alone[g])
    assert n4 == n2, (n4, n2)
    # one group: pred_flow_mask itself
    one = pipe.pred_flow_mask_groups(Is[3:], featt[3:], Hs[3:], hw[3:])
    assert all(_bits(one[0][key], alone[3][key]) for key in alone[3])


def test_pred_flow_mask_groups_one_group_packs_its_own_tensors(pipe):
    from rfx.pipeline import packed_group_offsets
    Is, It, Hs, hw = _fine_inputs(pipe)
    for g in (0, 3):                                                       # /8 widths 8 and 9 (padded correlation)
        featt = ops.l2norm(pipe.feat(It[g]))
        alone = pipe.pred_flow_mask(Is[g], featt, ops.warp_grid(Hs[g], *hw[g]))
        packed = {}
        n0 = ops.group_stats()
        got = pipe.pred_flow_mask_groups([Is[g]], [featt], [Hs[g]], [hw[g]], out=packed)
        assert ops.group_stats() == n0                                     # zero grouped launches
        torch.cuda.synchronize()
        assert len(got) == 1 and set(got[0]) == set(alone) and all(_bits(got[0][key], alone[key]) for key in alone)
        for key in ("match", "flowDown8", "match12Down8", "match21Down8"):
            assert packed[key].dim() == 1 and _bits(packed[key], alone[key].reshape(-1)), (g, key)
        assert packed["layout"] == packed_group_offsets([(FINE[g][0],) + hw[g] + tuple(featt.shape[2:])])


def test_cycle_forms_take_one_group(pipe):
    Is, It, Hs, hw = _fine_inputs(pipe)
    sub = [0, 1]
    fcs = [ops.warp_grid(Hs[g], *hw[g]) for g in sub]
    featt = [ops.l2norm(pipe.feat(It[g])) for g in sub]
    feats = [ops.l2norm(pipe.feat(ops.grid_sample(Is[g], fcs[g]))) for g in sub]
    with pytest.raises(ValueError, match="one shape group"):               # pred_flow_mask_cycle's form
        pipe.pred_flow_mask_lists(feats, featt, fcs, cycle=True)
    with pytest.raises(ValueError, match="one shape group"):               # pred_flow_mask_kitti's form
        pipe.pred_flow_mask_lists(feats, featt, fcs, cycle=True, out_hw=(90, 70))
    # one group through the list form is the named method, bit for bit
    one = pipe.pred_flow_mask_lists(feats[:1], featt[:1], fcs[:1], cycle=True)[0]
    ref = pipe.pred_flow_mask_cycle(Is[0], featt[0], fcs[0])
    assert set(one) == set(ref) and all(_bits(one[key], ref[key]) for key in ref)


def test_fine_quickstart_groups(pipe):
    Is, It, Hs, hw = _fine_inputs(pipe)
    preps = [dict(IsTensor=a, ItTensor=b) for a, b in zip(Is, It)]
    alone = [pipe.fine_quickstart(p, h) for p, h in zip(preps, Hs)]
    n0 = ops.group_stats()[1]
    got = pipe.fine_quickstart_groups(preps, Hs)
    n4 = ops.group_stats()[1] - n0
    torch.cuda.synchronize()
    for g in range(4):
        assert set(got[g]) == set(alone[g])
        for key in alone[g]:
            assert _bits(got[g][key], alone[g][key]), (g, key)
    n0 = ops.group_stats()[1]
    pipe.fine_quickstart_groups([preps[0], preps[3]], [Hs[0], Hs[3]])     # groups 0 and 3: see test_pred_flow_mask_groups
    n2 = ops.group_stats()[1] - n0
    print("grouped launches: 4 groups %d, 2 groups %d" % (n4, n2))
    assert n4 == n2, (n4, n2)


# ------------------------------------------------------------------------------------------------ 5. switch
def test_rfx_fine_groups_switch(pipe, monkeypatch):
    from PIL import Image  # noqa: F401
    pairs = []
    for seed, H, W, dh, dw in ((7, 240, 320, 0, 0), (8, 256, 320, 0, 16), (9, 240, 336, 0, 0)):
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
        pairs.append((I1, I2.crop((0, 0, W - dw, H - dh))))
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(DEV)

    def run(flag):
        monkeypatch.setenv("RFX_FINE_GROUPS", flag)
        prep = pipe.prepare_ragged_device([up(p[0]) for p in pairs], [up(p[1]) for p in pairs])
        n0 = ops.group_stats()[1]
        outs = pipe.multi_h_batched(prep, maxCoarse=3, maskRegionTh=0.01, pair_ids=[11, 12, 13], split=1)
        torch.cuda.synchronize()
        return outs, ops.group_stats()[1] - n0

    off, n_off = run("0")
    on, n_on = run("1")
    assert max(o["nbH"] for o in off) >= 1
    for b, (o, p) in enumerate(zip(on, off)):
        assert o["nbH"] == p["nbH"] and torch.equal(o["mask"], p["mask"]), b
        for key in ("H", "flowDown8", "matchDown8"):
            assert len(o[key]) == len(p[key]) and all(torch.equal(x, y) for x, y in zip(o[key], p[key])), (b, key)
    print("grouped launches per call: RFX_FINE_GROUPS=0 %d, =1 %d" % (n_off, n_on))
    assert n_on > n_off                          # the fine stage issued grouped launches (the trunk pass does either way)
