"""Host side of the layer1 expansion kernel (csrc/conv1x1e.hip): which layers ops.expand64_eligible admits (a literal table over
every 1x1 convolution of the four nets), which form each trunk block takes with RFX_EXPAND64 on and off, the launch-size rule,
and the binding's prototypes against the header.  Plans are built with device="cpu"; nothing is launched."""
import ctypes
import os
import re

import pytest

from rfx import nets, ops, weights, _lib
from test_conv_routes_cpu import _walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the only 1x1 convolutions with Cin = 64: conv3 of the three layer1 blocks and layer1.0's projection shortcut
ELIGIBLE = {"trunk": {"blocks.0.c3", "blocks.0.ds", "blocks.1.c3", "blocks.2.c3"}, "feat": set(), "flow": set(), "match": set()}


@pytest.fixture(scope="module")
def four_nets():
    saved = {k: os.environ.pop(k, None) for k in ("RFX_CONV_SPLIT", "RFX_SPLIT_TAILS", "RFX_FUSE_BOTTLENECK")}
    try:
        return dict(trunk=nets.ResNet50Trunk(weights.resnet50_trunk_sd(0), "cpu"),
                    feat=nets.FeatureExtractorNet(weights.feature_extractor_sd(1), "cpu"),
                    flow=nets.NetFlowCoarseNet(weights.net_flow_coarse_sd(2), device="cpu"),
                    match=nets.NetMatchabilityNet(weights.net_matchability_sd(3), device="cpu"))
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def test_eligibility_of_every_1x1_layer(four_nets):
    seen = 0
    for net, obj in four_nets.items():
        ones = {name: p for name, p in _walk(obj) if p.KH == 1 and p.KW == 1}
        seen += len(ones)
        assert {name for name, p in ones.items() if ops.expand64_eligible(p)} == ELIGIBLE[net], net
        for name, p in ones.items():
            # the geometry tuple the nets ask about before they pack gives the plan's own answer
            g = ops.ConvGeometry(p.Cout, p.Cin, p.KH, p.KW, p.stride, p.pad, p.act, p.scale)
            assert ops.expand64_eligible(g) == ops.expand64_eligible(p), (net, name)
    assert seen == 13 * 2 + 3 + 2      # trunk: c1 + c3 of 13 blocks, 3 projections; FeatureExtractor: 2 projections; the heads: none
    c3 = four_nets["trunk"].blocks[0]["c3"]
    base = dict(Cout=256, Cin=64, KH=1, KW=1, stride=1, pad=0, act=ops.ACT_RELU, scale=c3.scale)
    assert ops.expand64_eligible(ops.ConvGeometry(**base))
    for change in (dict(Cin=128), dict(Cin=32), dict(Cout=192), dict(Cout=128), dict(Cout=64), dict(Cout=512), dict(stride=2), dict(pad=1), dict(KH=3, KW=3),
                   dict(scale=None), dict(act=ops.ACT_SIGMOID)):
        assert not ops.expand64_eligible(ops.ConvGeometry(**dict(base, **change))), change
    assert ops.expand64_eligible(ops.ConvGeometry(**dict(base, act=ops.ACT_NONE)))


@pytest.mark.parametrize("switch", [True, False])
def test_forms_of_the_trunk_blocks(four_nets, monkeypatch, switch):
    monkeypatch.setattr(ops, "_EXPAND64", switch)
    for k in ("RFX_CONV_SPLIT", "RFX_SPLIT_TAILS", "RFX_FUSE_BOTTLENECK"):
        monkeypatch.delenv(k, raising=False)
    trunk = four_nets["trunk"]
    forms = [trunk.expand64_form(b) for b in trunk.blocks]
    assert forms == (["dual", "plain", "plain"] if switch else [None] * 3) + [None] * 10
    # layer2.0 / layer3.0: their projections are stride 2 with Cin >= 256 -- not this kernel's, whatever the switch
    for i in (3, 7):
        assert trunk.blocks[i]["ds"] is not None and ops.expand64_form(trunk.blocks[i]["c3"], trunk.blocks[i]["ds"]) is None


def test_fused_tails_keep_their_kernel(monkeypatch):
    """With the layer1 tails on the fused fp32 kernel (RFX_SPLIT_TAILS=0 / RFX_CONV_SPLIT=0) conv3 is not a launch of its own."""
    monkeypatch.setattr(ops, "_EXPAND64", True)
    monkeypatch.delenv("RFX_FUSE_BOTTLENECK", raising=False)
    monkeypatch.setenv("RFX_SPLIT_TAILS", "0")
    trunk = nets.ResNet50Trunk(weights.resnet50_trunk_sd(0), "cpu")
    assert [trunk.expand64_form(b) for b in trunk.blocks] == [None] * 13
    monkeypatch.setenv("RFX_FUSE_BOTTLENECK", "0")          # ... and as two kernels again, conv3 takes the new launches
    assert [trunk.expand64_form(b) for b in trunk.blocks[:3]] == ["dual", "plain", "plain"]


def test_switch_is_read_once(monkeypatch):
    monkeypatch.setattr(ops, "_EXPAND64", None)
    monkeypatch.setenv("RFX_EXPAND64", "0")
    assert ops.expand64_enabled() is False
    monkeypatch.setenv("RFX_EXPAND64", "1")
    assert ops.expand64_enabled() is False
    monkeypatch.setattr(ops, "_EXPAND64", None)
    assert ops.expand64_enabled() is True
    monkeypatch.setattr(ops, "_EXPAND64", None)
    monkeypatch.delenv("RFX_EXPAND64")
    assert ops.expand64_enabled() is True


def test_launch_size_rule(four_nets, monkeypatch):
    """Launches below the measured limits stay on today's kernels (profiles/expand64_ab.json): a single pair's largest layer1
    map (240 x 320) takes neither form, the bench's smallest batched level (64 x 60 x 80) takes both."""
    monkeypatch.setattr(ops, "_EXPAND64", True)
    b0, b1 = four_nets["trunk"].blocks[:2]
    lim = ops.EXPAND64_MIN_PIXELS
    assert 76800 < lim["dual"] <= lim["plain"] <= 64 * 60 * 80
    assert ops.expand64_form(b0["c3"], b0["ds"], 240 * 320) is None and ops.expand64_form(b1["c3"], None, 240 * 320) is None
    assert ops.expand64_form(b0["c3"], b0["ds"], lim["dual"]) == "dual" and ops.expand64_form(b0["c3"], b0["ds"], lim["dual"] - 1) is None
    assert ops.expand64_form(b1["c3"], None, lim["plain"]) == "plain" and ops.expand64_form(b1["c3"], None, lim["plain"] - 1) is None
    assert ops.expand64_form(b0["c3"], b0["ds"]) == "dual"       # no size given: the geometry alone


def test_prototypes_mirror_the_header():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rfx_api.h")).read(), flags=re.S)
    assert int(re.search(r"#define RFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    for name in ("rfx_conv1x1_expand64_f32", "rfx_conv1x1_expand64_dual_f32"):
        ret, args = re.search(r"\b(int)\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S).groups()
        kinds = [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args.split(",")]
        assert all(re.match(r"\s*(const\s+float\s*\*|float\s*\*|void\s*\*|int)\s*\w+\s*$", a) for a in args.split(",")), args
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and argtypes == kinds, name
    # plain: 6 pointers, N Cin HW Cout stride act, stream; two-source: 2 x 4 operand pointers + out, N Cin HW Cout stride, stream
    assert len(_lib.SIGNATURES["rfx_conv1x1_expand64_f32"][1]) == 13 and len(_lib.SIGNATURES["rfx_conv1x1_expand64_dual_f32"][1]) == 15
