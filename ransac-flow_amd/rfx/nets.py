"""The four networks of the hot path as sequences of librfx kernel launches.

Each class is built from a reference-keyed ``state_dict`` (see rfx/weights.py), packs the conv weights and
folds eval-mode BatchNorm once, and then runs forward-only on device tensors.  Activations stay NCHW fp32
from the first layer to the last: there is no layout conversion between kernels.
"""
import functools
import os

import torch

from . import ops
from .ops import ConvPlan, ACT_NONE, ACT_RELU, ACT_SIGMOID


def _bn(sd, p):
    return {k: sd[p + "." + k] for k in ("weight", "bias", "running_mean", "running_var")}


class ResNet50Trunk:
    """ResNet-50 conv1..layer3 (stride 16, 1024 channels): model/resnet50.py:68-104,112-169 as sliced by
    quick_start/coarseAlignFeatMatch.py:34-52.  Bottleneck = 1x1 -> 3x3 (stride here) -> 1x1, BN folded into
    every conv's epilogue, residual add + ReLU fused into the third conv."""

    def __init__(self, sd, device="cuda"):
        self.conv1 = ConvPlan(sd["conv1.weight"], _bn(sd, "bn1"), stride=2, pad=3, act=ACT_RELU, device=device)
        self.blocks = []
        for layer, nblk, stride in (("layer1", 3, 1), ("layer2", 4, 2), ("layer3", 6, 2)):
            for b in range(nblk):
                p = "%s.%d" % (layer, b)
                s = stride if b == 0 else 1
                w1, w2, w3 = (sd["%s.conv%d.weight" % (p, i)] for i in (1, 2, 3))
                # Which convolutions ask for the split kernels (float32 sums from exact bf16 operand pieces, closer to the exact sum
                # than the fp32-MFMA kernels and 1.3-1.5x faster: profiles/r06_split_conv_bench.json) is decided here, from the
                # layer's shapes, before anything is packed.  c1 and the projection shortcut: the long-K 1x1 layers (K >= 128).
                # (scale: bottleneck_tail_shape only asks whether one is folded -- every convolution here has its BatchNorm)
                tail = ops.bottleneck_tail_shape(ops.ConvGeometry(*w2.shape, stride=s, pad=1, act=ACT_RELU, scale="bn2"),
                                                 ops.ConvGeometry(*w3.shape, stride=1, pad=0, act=ACT_RELU, scale="bn3"))
                if not tail:
                    # layer3 (256 -> 256 3x3, K = 2304; conv3 with K = 256, + residual) and the stride-2 3x3 of a layer's first block
                    split2 = split3 = True
                elif ops.conv_split_enabled() and os.environ.get("RFX_SPLIT_TAILS", "1") != "0":
                    # layer1 / layer2 tails (3x3 64 -> 64 / 128 -> 128, then the 1x1 expansion): two split kernels beat the fused fp32
                    # kernel (the 3x3 runs 1.3-1.45x faster on the bf16 pipe; measured per block in profiles/r06_split_conv_bench.json)
                    split2, split3 = True, w3.shape[1] >= 128
                else:
                    # the tail stays on the fp32 kernels: fused and two-kernel forms stay bit-identical
                    split2 = split3 = False
                blk = {
                    "c1": ConvPlan(w1, _bn(sd, p + ".bn1"), 1, 0, ACT_RELU, device, split=w1.shape[1] >= 128),
                    "c2": ConvPlan(w2, _bn(sd, p + ".bn2"), s, 1, ACT_RELU, device, split=split2),
                    "c3": ConvPlan(w3, _bn(sd, p + ".bn3"), 1, 0, ACT_RELU, device, split=split3),
                    "ds": None,
                }
                if (p + ".downsample.0.weight") in sd:
                    wd = sd[p + ".downsample.0.weight"]       # the stride-2 projections (256 -> 512, 512 -> 1024): split kernel, strided pixels
                    blk["ds"] = ConvPlan(wd, _bn(sd, p + ".downsample.1"), s, 0, ACT_NONE, device, split=wd.shape[1] >= 128)
                if tail:
                    # the tail's 3x3 (K = 576 / 1152) sums in chunks of 4 K steps -- in the fused kernel and, with this argument,
                    # in the stand-alone one (RFX_FUSE_BOTTLENECK=0): the two forms stay bit-identical
                    blk["c2"].k_chunk = 4
                self.blocks.append(blk)

    def __call__(self, x):
        return self._forward([x], True, True)[0]

    def forward_group(self, xs, side_streams=True):
        """The same pass over several inputs of DIFFERENT sizes (a single pair's 7 pyramid levels + target), layer by layer with
        one grouped launch per kernel instance and layer instead of one launch per layer and input: bit-identical to
        [self(x) for x in xs].  The expand64 forms are never used here, whatever the list length."""
        return self._forward(xs, side_streams, False)

    def _forward(self, xs, side_streams, expand64):
        """The layer sequence, one ops.stage per layer over the inputs ``xs``.  ``expand64``: layer1's 64 -> 256 expansions may take
        ops.conv1x1_expand64's forms (expand64_form)."""
        st = functools.partial(ops.stage, device=xs[0].device, side_streams=side_streams)
        xs = st(lambda x: ops.stem_conv7_maxpool(x, self.conv1), xs)  # conv1 + BN + ReLU + MaxPool2d(3, 2, 1) in one kernel
        for blk in self.blocks:
            c1, c2, c3, ds = blk["c1"], blk["c2"], blk["c3"], blk["ds"]
            form = self.expand64_form(blk) if expand64 else None
            if form == "dual":
                # layer1.0: conv3 and the projection shortcut in one launch -- the 256-channel shortcut never goes to memory
                xs = st(lambda m, x: ops.conv1x1_expand64(m, c3, shortcut=(x, ds)), st(c2, st(c1, xs)), xs)
                continue
            # c1 and the projection shortcut both read x only: one stage
            os_, rs = zip(*st(lambda x: (c1(x), ds(x) if ds is not None else x), xs))
            if ops.bottleneck_tail_eligible(c2, c3):
                xs = st(lambda o, r: ops.bottleneck_tail(o, c2, c3, residual=r), os_, rs)   # conv2 + conv3 in one kernel
            elif form == "plain":
                xs = st(lambda m, r: ops.conv1x1_expand64(m, c3, residual=r), st(c2, os_), rs)   # layer1.1 / layer1.2
            else:
                xs = st(lambda m, r: c3(m, residual=r), st(c2, os_), rs)  # relu(bn3(conv3(o)) + r)
        return xs

    @staticmethod
    def expand64_form(blk):
        """The form of ops.conv1x1_expand64 a block's conv3 takes in __call__ ("dual", "plain" or None): the 64 -> 256 expansions of
        layer1 where they run as a kernel of their own (not inside the fused tail) and RFX_EXPAND64 is not 0."""
        if ops.bottleneck_tail_eligible(blk["c2"], blk["c3"]):
            return None
        return ops.expand64_form(blk["c3"], blk["ds"])


class FeatureExtractorNet:
    """model/model.py:59-125: conv3x3(3->64)+BN+ReLU, MaxPool(2,1)+BlurPool/2, 2xBasicBlock(64),
    2x(128,/2), 2x(256,/2).  Shortcut of the strided blocks = BlurPool/2 -> 1x1 conv -> BN (:92-93)."""

    def __init__(self, sd, device="cuda"):
        self.conv1 = ConvPlan(sd["conv1.weight"], _bn(sd, "bn1"), 1, 1, ACT_RELU, device)
        self.blocks = []
        for layer, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
            for b in range(2):
                p = "%s.%d" % (layer, b)
                s = stride if b == 0 else 1
                blk = {
                    # the stride-1 3x3 convolutions (64 / 128 / 256 channels): rfx_conv3x3_split_f32 (round 6; csrc/conv3x3s.hip)
                    "c1": ConvPlan(sd[p + ".conv1.weight"], _bn(sd, p + ".bn1"), s, 1, ACT_RELU, device, split=True),      # stride 2: ..._split_s2_f32
                    "c2": ConvPlan(sd[p + ".conv2.weight"], _bn(sd, p + ".bn2"), 1, 1, ACT_RELU, device, split=True),
                    "ds": None, "stride": s,
                }
                if (p + ".downsample.1.weight") in sd:
                    blk["ds"] = ConvPlan(sd[p + ".downsample.1.weight"], _bn(sd, p + ".downsample.2"), 1, 0, ACT_NONE,
                                         device)
                self.blocks.append(blk)

    def __call__(self, x):
        return self.forward_group([x])[0]

    def forward_group(self, xs, side_streams=True):
        """The pass over inputs of DIFFERENT sizes (the shape groups of a ragged fine stage), one ops.stage per layer: bit-identical
        to [self(x) for x in xs]."""
        st = functools.partial(ops.stage, device=xs[0].device, side_streams=side_streams)
        xs = st(lambda x: ops.stem_conv_maxblur(x, self.conv1), xs)  # conv1 + BN + ReLU + MaxPool2d(2, stride 1) + BlurPool/2 in one kernel
        for blk in self.blocks:
            c1, c2, ds, s = blk["c1"], blk["c2"], blk["ds"], blk["stride"]
            if ds is None:
                os_, rs = st(c1, xs), xs
            else:
                os_, bs = zip(*st(lambda x: (c1(x), ops.blurpool2d(x, s)), xs))          # c1 and the shortcut's blur both read x only
                rs = st(ds, bs)
            xs = st(lambda o, r: c2(o, residual=r), os_, rs)
        return xs


class _HeadTrunk:
    def __init__(self, sd, last_act, device):
        self.c1 = ConvPlan(sd["conv1.weight"], _bn(sd, "bn1"), 1, 1, ACT_RELU, device, split=True)      # 49 -> 512 (a ragged 4th channel block),
        self.c2 = ConvPlan(sd["conv2.weight"], _bn(sd, "bn2"), 1, 1, ACT_RELU, device, split=True)      # 512 -> 256, 256 -> 128:
        self.c3 = ConvPlan(sd["conv3.weight"], _bn(sd, "bn3"), 1, 1, ACT_RELU, device, split=True)      # rfx_conv3x3_split_f32
        self.c4 = ConvPlan(sd["conv4.weight"], None, 1, 1, last_act, device)

    def __call__(self, coef):
        return self.forward_group([coef])[0]

    def forward_group(self, coefs, side_streams=True, halves_out=None):
        """[self(c) for c in coefs] for volumes of different sizes, one ops.stage per layer.  ``halves_out``: one (out_a, out_b) per
        input -- the last convolution then runs on the two halves of each batch as two problems and writes them to out_a / out_b
        (views of two packed buffers: PredFlowMask's match12Down8 / match21Down8 of several groups); returns those pairs.  Without
        it the last convolution is one launch over each whole batch."""
        st = functools.partial(ops.stage, device=coefs[0].device, side_streams=side_streams)
        xs = coefs
        for c in (self.c1, self.c2, self.c3):
            xs = st(c, xs)
        if halves_out is None:
            return st(self.c4, xs)
        return st(lambda x, o: (self.c4(x[:x.shape[0] // 2], out=o[0]), self.c4(x[x.shape[0] // 2:], out=o[1])), xs, halves_out)


def _up8(m):
    """F.upsample_bilinear x8 (align_corners=True)."""
    return ops.resize_bilinear(m, (m.shape[2] * 8, m.shape[3] * 8), align_corners=True)


class NetFlowCoarseNet:
    """model/model.py:167-249.  up8X=True -> F.upsample_bilinear x8 (align_corners=True, :234)."""

    def __init__(self, sd, kernelSize=7, device="cuda"):
        self.k = kernelSize
        self.trunk = _HeadTrunk(sd, ACT_NONE, device)

    def __call__(self, coef, up8X=True):
        return self.forward_group([coef], up8X)[0]

    def forward_group(self, coefs, up8X=True, side_streams=True, outs=None):
        """[self(c, up8X) for c in coefs] for volumes of different sizes: the trunk, the flow head and the x8 resize as stages,
        bit-identical to the per-input calls.  ``outs``: where the /8 flows go (views of a packed buffer)."""
        st = functools.partial(ops.stage, device=coefs[0].device, side_streams=side_streams)
        flows = st(lambda l, o: ops.flow_head(l, self.k, out=o), self.trunk.forward_group(coefs, side_streams),
                   outs if outs is not None else [None] * len(coefs))
        return st(_up8, flows) if up8X else flows


class NetMatchabilityNet:
    """model/model.py:254-322: sigmoid fused into the last conv's epilogue."""

    def __init__(self, sd, kernelSize=7, device="cuda"):
        self.trunk = _HeadTrunk(sd, ACT_SIGMOID, device)

    def __call__(self, feat, up8X=True):
        return self.forward_group([feat], up8X)[0]

    def forward_group(self, feats, up8X=True, side_streams=True):
        """[self(f, up8X) for f in feats] for volumes of different sizes, as stages, bit-identical to the per-input calls."""
        ms = self.trunk.forward_group(feats, side_streams)
        return ops.stage(_up8, ms, device=feats[0].device, side_streams=side_streams) if up8X else ms
