"""ConvPlan's routes, on the host: which kernel family every convolution of every net runs on (a literal table), that a plan
holds exactly its route's weight packs, and that a net packs each of its convolutions once.  Plans are built with device="cpu"."""
import inspect
import os

import pytest
import torch

from rfx import nets, ops, segnet, weights

ENVS = ({}, {"RFX_CONV_SPLIT": "0"}, {"RFX_SPLIT_TAILS": "0"})

# layer -> route under (the default environment, RFX_CONV_SPLIT=0, RFX_SPLIT_TAILS=0); one name: the same under all three
ROUTES = {
    "trunk": {
        "conv1": "gemm", "blocks.0.c1": "gemm", "blocks.0.c2": ("split3x3", "fp32_3x3", "fp32_3x3"), "blocks.0.c3": "gemm",
        "blocks.0.ds": "gemm", "blocks.1.c1": ("split1x1", "gemm", "split1x1"), "blocks.1.c2": ("split3x3", "fp32_3x3", "fp32_3x3"),
        "blocks.1.c3": "gemm", "blocks.2.c1": ("split1x1", "gemm", "split1x1"), "blocks.2.c2": ("split3x3", "fp32_3x3", "fp32_3x3"),
        "blocks.2.c3": "gemm", "blocks.3.c1": ("split1x1", "gemm", "split1x1"),
        "blocks.3.c2": ("split3x3_s2", "fp32_3x3", "split3x3_s2"), "blocks.3.c3": ("split1x1", "gemm", "split1x1"),
        "blocks.3.ds": ("split1x1", "gemm", "split1x1"), "blocks.4.c1": ("split1x1", "gemm", "split1x1"),
        "blocks.4.c2": ("split3x3", "fp32_3x3", "fp32_3x3"), "blocks.4.c3": ("split1x1", "gemm", "gemm"),
        "blocks.5.c1": ("split1x1", "gemm", "split1x1"), "blocks.5.c2": ("split3x3", "fp32_3x3", "fp32_3x3"),
        "blocks.5.c3": ("split1x1", "gemm", "gemm"), "blocks.6.c1": ("split1x1", "gemm", "split1x1"),
        "blocks.6.c2": ("split3x3", "fp32_3x3", "fp32_3x3"), "blocks.6.c3": ("split1x1", "gemm", "gemm"),
        "blocks.7.c1": ("split1x1", "gemm", "split1x1"), "blocks.7.c2": ("split3x3_s2", "fp32_3x3", "split3x3_s2"),
        "blocks.7.c3": ("split1x1", "gemm", "split1x1"), "blocks.7.ds": ("split1x1", "gemm", "split1x1"),
        "blocks.8.c1": ("split1x1", "gemm", "split1x1"), "blocks.8.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.8.c3": ("split1x1", "gemm", "split1x1"), "blocks.9.c1": ("split1x1", "gemm", "split1x1"),
        "blocks.9.c2": ("split3x3", "fp32_3x3", "split3x3"), "blocks.9.c3": ("split1x1", "gemm", "split1x1"),
        "blocks.10.c1": ("split1x1", "gemm", "split1x1"), "blocks.10.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.10.c3": ("split1x1", "gemm", "split1x1"), "blocks.11.c1": ("split1x1", "gemm", "split1x1"),
        "blocks.11.c2": ("split3x3", "fp32_3x3", "split3x3"), "blocks.11.c3": ("split1x1", "gemm", "split1x1"),
        "blocks.12.c1": ("split1x1", "gemm", "split1x1"), "blocks.12.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.12.c3": ("split1x1", "gemm", "split1x1"),
    },
    "feat": {
        "conv1": "gemm", "blocks.0.c1": ("split3x3", "fp32_3x3", "split3x3"), "blocks.0.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.1.c1": ("split3x3", "fp32_3x3", "split3x3"), "blocks.1.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.2.c1": ("split3x3_s2", "fp32_3x3", "split3x3_s2"), "blocks.2.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.2.ds": "gemm", "blocks.3.c1": ("split3x3", "fp32_3x3", "split3x3"), "blocks.3.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.4.c1": ("split3x3_s2", "fp32_3x3", "split3x3_s2"), "blocks.4.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "blocks.4.ds": "gemm", "blocks.5.c1": ("split3x3", "fp32_3x3", "split3x3"), "blocks.5.c2": ("split3x3", "fp32_3x3", "split3x3"),
    },
    "flow": {
        "trunk.c1": ("split3x3", "fp32_3x3", "split3x3"), "trunk.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "trunk.c3": ("split3x3", "fp32_3x3", "split3x3"), "trunk.c4": "fp32_3x3",
    },
    "match": {
        "trunk.c1": ("split3x3", "fp32_3x3", "split3x3"), "trunk.c2": ("split3x3", "fp32_3x3", "split3x3"),
        "trunk.c3": ("split3x3", "fp32_3x3", "split3x3"), "trunk.c4": "fp32_3x3",
    },
    "segenc": {
        "stem.0": "gemm", "stem.1": "fp32_3x3", "stem.2": "fp32_3x3", "blocks.0.c1": "gemm", "blocks.0.c2": "fp32_3x3",
        "blocks.0.c3": "gemm", "blocks.0.ds": "gemm", "blocks.1.c1": "gemm", "blocks.1.c2": "fp32_3x3", "blocks.1.c3": "gemm",
        "blocks.2.c1": "gemm", "blocks.2.c2": "fp32_3x3", "blocks.2.c3": "gemm", "blocks.3.c1": "gemm", "blocks.3.c2": "fp32_3x3",
        "blocks.3.c3": "gemm", "blocks.3.ds": "gemm", "blocks.4.c1": "gemm", "blocks.4.c2": "fp32_3x3", "blocks.4.c3": "gemm",
        "blocks.5.c1": "gemm", "blocks.5.c2": "fp32_3x3", "blocks.5.c3": "gemm", "blocks.6.c1": "gemm", "blocks.6.c2": "fp32_3x3",
        "blocks.6.c3": "gemm", "blocks.7.c1": "gemm", "blocks.7.c2": "fp32_3x3", "blocks.7.c3": "gemm", "blocks.7.ds": "gemm",
        "blocks.8.c1": "gemm", "blocks.8.c2": "dilated", "blocks.8.c3": "gemm", "blocks.9.c1": "gemm", "blocks.9.c2": "dilated",
        "blocks.9.c3": "gemm", "blocks.10.c1": "gemm", "blocks.10.c2": "dilated", "blocks.10.c3": "gemm", "blocks.11.c1": "gemm",
        "blocks.11.c2": "dilated", "blocks.11.c3": "gemm", "blocks.12.c1": "gemm", "blocks.12.c2": "dilated", "blocks.12.c3": "gemm",
        "blocks.13.c1": "gemm", "blocks.13.c2": "dilated", "blocks.13.c3": "gemm", "blocks.13.ds": "gemm", "blocks.14.c1": "gemm",
        "blocks.14.c2": "dilated", "blocks.14.c3": "gemm", "blocks.15.c1": "gemm", "blocks.15.c2": "dilated", "blocks.15.c3": "gemm",
    },
    "segdec": {
        "ppm.0": "gemm", "ppm.1": "gemm", "ppm.2": "gemm", "ppm.3": "gemm", "conv_last": "fp32_3x3", "classify": "gemm",
    },
}


def _walk(obj, prefix=""):
    if isinstance(obj, ops.ConvPlan):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _walk(v, "%s.%s" % (prefix, k) if prefix else str(k))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _walk(v, "%s.%d" % (prefix, i) if prefix else str(i))
    elif type(obj).__module__.startswith("rfx"):
        for k, v in vars(obj).items():
            yield from _walk(v, "%s.%s" % (prefix, k) if prefix else k)


@pytest.fixture(scope="module", params=range(3), ids=["default", "RFX_CONV_SPLIT=0", "RFX_SPLIT_TAILS=0"])
def built(request):
    """(environment index, {net: object}, {id(plan): the split= it was built with}, ConvPlan constructions of the trunk)."""
    saved = {k: os.environ.pop(k, None) for k in ("RFX_CONV_SPLIT", "RFX_SPLIT_TAILS")}
    os.environ.update(ENVS[request.param])
    init, asked = ops.ConvPlan.__init__, {}

    def counting_init(self, *a, **kw):
        asked[id(self)] = inspect.signature(init).bind(self, *a, **kw).arguments.get("split", False)
        init(self, *a, **kw)

    ops.ConvPlan.__init__ = counting_init
    try:
        built = {"trunk": nets.ResNet50Trunk(weights.resnet50_trunk_sd(0), "cpu")}
        n_trunk = len(asked)
        built.update(feat=nets.FeatureExtractorNet(weights.feature_extractor_sd(1), "cpu"),
                     flow=nets.NetFlowCoarseNet(weights.net_flow_coarse_sd(2), device="cpu"),
                     match=nets.NetMatchabilityNet(weights.net_matchability_sd(3), device="cpu"),
                     segenc=segnet.SegEncoder(weights.seg_encoder_sd(4), "cpu"), segdec=segnet.SegDecoder(weights.seg_decoder_sd(5), "cpu"))
    finally:
        ops.ConvPlan.__init__ = init
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return request.param, built, asked, n_trunk


def test_route_of_every_layer(built):
    env, objs, asked, _ = built
    assert set(objs) == set(ROUTES)
    for net, obj in objs.items():
        plans = dict(_walk(obj))
        assert set(plans) == set(ROUTES[net]), net
        for name, p in plans.items():
            want = ROUTES[net][name]
            assert p.route == (want if isinstance(want, str) else want[env]), (net, name)
            # the pure function, fed the layer's geometry and what its net asked for, names the route the plan was built on
            assert ops.conv_route(p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.dilation, asked[id(p)], "RFX_CONV_SPLIT" not in ENVS[env]) == p.route
            packs = {a for a in ("wS", "wP", "wT", "ktab") if getattr(p, a) is not None}
            assert packs == PACKS[p.route], (net, name)


def test_trunk_packs_each_convolution_once(built):
    _, objs, _, n_trunk = built
    sd = weights.resnet50_trunk_sd(0)
    assert n_trunk == sum(1 for k, v in sd.items() if v.dim() == 4) == 43
    assert len(dict(_walk(objs["trunk"]))) == 43
    for blk in objs["trunk"].blocks:             # the question the trunk asks before it packs has the plans' own answer
        g2, g3 = (ops.ConvGeometry(p.Cout, p.Cin, p.KH, p.KW, p.stride, p.pad, p.act, True) for p in (blk["c2"], blk["c3"]))
        assert ops.bottleneck_tail_shape(g2, g3) == ops.bottleneck_tail_shape(blk["c2"], blk["c3"])
        assert blk["c2"].k_chunk == (4 if ops.bottleneck_tail_shape(g2, g3) else 0)


PACKS = {"dilated": {"wT", "ktab"}, "gemm": {"wT", "ktab"}, "fp32_3x3": {"wP", "wT", "ktab"},
         "split1x1": {"wS"}, "split3x3": {"wS"}, "split3x3_s2": {"wS"}}


@pytest.mark.parametrize("route,shape,stride,pad,dil,split", [
    ("dilated", (70, 24, 3, 3), 1, 2, 2, True), ("gemm", (70, 24, 1, 1), 1, 0, 1, False), ("gemm", (70, 3, 7, 7), 2, 3, 1, True),
    ("fp32_3x3", (70, 49, 3, 3), 1, 1, 1, False), ("fp32_3x3", (70, 24, 3, 3), 2, 1, 1, True), ("split1x1", (70, 48, 1, 1), 2, 0, 1, True),
    ("split3x3", (70, 49, 3, 3), 1, 1, 1, True), ("split3x3_s2", (130, 32, 3, 3), 2, 1, 1, True)])
def test_a_plan_holds_its_routes_packs_and_no_others(monkeypatch, route, shape, stride, pad, dil, split):
    monkeypatch.delenv("RFX_CONV_SPLIT", raising=False)
    w = torch.randn(*shape, generator=torch.Generator().manual_seed(7))
    p = ops.ConvPlan(w, None, stride, pad, ops.ACT_NONE, "cpu", dilation=dil, split=split)
    assert p.route == route == ops.conv_route(shape[1], shape[0], shape[2], shape[3], stride, pad, dil, split, True)
    want = {"wT": ops.pack_wT(w), "ktab": ops.pack_ktab(w, dil)} if "wT" in PACKS[route] else {}
    if "wP" in PACKS[route]:
        want["wP"] = ops.pack_wP(w)
    if "wS" in PACKS[route]:
        want["wS"] = ops.split_weights(w.reshape(shape[0], shape[1])) if route == "split1x1" else ops.split_weights_3x3(w)
    for a in ("wS", "wP", "wT", "ktab"):
        assert (getattr(p, a) is None) == (a not in want), a
        assert a not in want or (getattr(p, a).dtype == want[a].dtype and torch.equal(getattr(p, a), want[a])), a
    assert (p.w2d is None) == (shape[2] != 1)                       # the host copy quad_weights() packs from: 1x1 plans only
    if shape[2] == 1 and shape[1] % 8 == 0:
        assert torch.equal(p.quad_weights(), ops.pack_wQ(w.reshape(shape[0], shape[1])))


def test_pack_layouts():
    """Every pack function against the index formula include/rfx_api.h documents for its kernel."""
    w = torch.randn(70, 10, 3, 3, generator=torch.Generator().manual_seed(8))
    w2 = w.reshape(70, 90)
    wT, ktab, wP = ops.pack_wT(w), ops.pack_ktab(w, 2), ops.pack_wP(w)
    assert tuple(wT.shape) == (96, 128) and torch.equal(wT[:90, :70], w2.t()) and float(wT[90:].abs().max()) == float(wT[:, 70:].abs().max()) == 0.0
    kt = ktab.view(3, 2, 16).permute(0, 2, 1).reshape(-1)            # undo the [16 even k | 16 odd k] order of a 32-k block
    for k in (0, 1, 17, 40, 89):
        c, kh, kw = k // 9, (k % 9) // 3, k % 3
        assert int(kt[k]) == (c << 8) | ((kh * 2) << 4) | (kw * 2)
    assert bool((kt[90:] == -1).all()) and ktab.dtype == torch.int32
    assert tuple(wP.shape) == (1, 2, 2, 128, 36)                     # Cin = 10: two K steps of 8 channels, the last one ragged
    for (s, h, m, kk) in ((0, 0, 0, 0), (0, 1, 69, 35), (1, 0, 5, 8), (1, 1, 33, 0)):
        assert wP[0, s, h, m, kk] == w2[m, s * 72 + 2 * kk + h]
    assert float(wP[0, 1, :, :, 9:].abs().max()) == 0.0 and float(wP[0, :, :, 70:].abs().max()) == 0.0
    w1 = torch.randn(70, 16, generator=torch.Generator().manual_seed(9))
    wQ = ops.pack_wQ(w1)
    assert tuple(wQ.shape) == (2, 2, 70, 4)
    for (q, h, m, j) in ((0, 0, 0, 0), (1, 1, 69, 3), (1, 0, 7, 2)):
        assert wQ[q, h, m, j] == w1[m, 8 * q + 2 * j + h]
    wS3 = ops.split_weights_3x3(w)                                   # [c / 16][tap][piece][h][m][8]: every tap is split_weights of its slice
    assert tuple(wS3.shape) == (1, 9, 3, 2, 128, 8)
    for tap in range(9):
        assert torch.equal(wS3[:, tap], ops.split_weights(w[:, :, tap // 3, tap % 3]))


def test_split_plan_holds_six_bytes_per_padded_weight():
    """A split 1x1 plan's tensors: wS = three bf16 pieces of every weight of the (Mpad, Cin) matrix, + scale + shift; no fp32 pack."""
    Cout, Cin = 200, 48
    g = torch.Generator().manual_seed(10)
    bn = dict(weight=torch.rand(Cout, generator=g), bias=torch.rand(Cout, generator=g), running_mean=torch.rand(Cout, generator=g),
              running_var=torch.rand(Cout, generator=g) + 0.5)
    p = ops.ConvPlan(torch.randn(Cout, Cin, 1, 1, generator=g), bn, 1, 0, ops.ACT_RELU, "cpu", split=True)
    held = {k: t.numel() * t.element_size() for k, t in vars(p).items() if isinstance(t, torch.Tensor) and k != "w2d"}   # w2d: host copy
    assert held == {"wS": 6 * 256 * Cin, "scale": 4 * Cout, "shift": 4 * Cout}
