"""The four networks of the hot path as sequences of librfx kernel launches.

Each class is built from a reference-keyed ``state_dict`` (see rfx/weights.py), packs the conv weights and
folds eval-mode BatchNorm once, and then runs forward-only on device tensors.  Activations stay NCHW fp32
from the first layer to the last: there is no layout conversion between kernels.
"""
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
        x = ops.stem_conv7_maxpool(x, self.conv1)  # conv1 + BN + ReLU + MaxPool2d(3, 2, 1) in one kernel
        for blk in self.blocks:
            o = blk["c1"](x)
            form = self.expand64_form(blk)
            if form == "dual":
                # layer1.0: conv3 and the projection shortcut in one launch -- the 256-channel shortcut never goes to memory
                x = ops.conv1x1_expand64(blk["c2"](o), blk["c3"], shortcut=(x, blk["ds"]))
                continue
            r = blk["ds"](x) if blk["ds"] is not None else x
            if ops.bottleneck_tail_eligible(blk["c2"], blk["c3"]):
                x = ops.bottleneck_tail(o, blk["c2"], blk["c3"], residual=r)   # conv2 + conv3 in one kernel
            elif form == "plain":
                x = ops.conv1x1_expand64(blk["c2"](o), blk["c3"], residual=r)   # layer1.1 / layer1.2
            else:
                o = blk["c2"](o)
                x = blk["c3"](o, residual=r)  # relu(bn3(conv3(o)) + r)
        return x

    @staticmethod
    def expand64_form(blk):
        """The form of ops.conv1x1_expand64 a block's conv3 takes in __call__ ("dual", "plain" or None): the 64 -> 256 expansions of
        layer1 where they run as a kernel of their own (not inside the fused tail) and RFX_EXPAND64 is not 0."""
        if ops.bottleneck_tail_eligible(blk["c2"], blk["c3"]):
            return None
        return ops.expand64_form(blk["c3"], blk["ds"])


    def forward_group(self, xs, side_streams=True):
        """The same pass over several inputs of DIFFERENT sizes (a single pair's 7 pyramid levels + target), layer by layer
        with one grouped launch per kernel instance and layer (ops.launch_group) instead of one launch per layer and input:
        bit-identical to [self(x) for x in xs]."""
        dev = xs[0].device
        with ops.launch_group(dev, side_streams):
            xs = [ops.stem_conv7_maxpool(x, self.conv1) for x in xs]
        for blk in self.blocks:
            with ops.launch_group(dev, side_streams):          # c1 and the projection shortcut both read x only: one group
                os_ = [blk["c1"](x) for x in xs]
                rs = [blk["ds"](x) for x in xs] if blk["ds"] is not None else xs
            # outputs get NEW names inside a group and are rebound after it: the recorded launches read their inputs when the
            # group ends, so every input tensor must stay referenced until then (launch_group's contract)
            if ops.bottleneck_tail_eligible(blk["c2"], blk["c3"]):
                with ops.launch_group(dev, side_streams):
                    ys = [ops.bottleneck_tail(o, blk["c2"], blk["c3"], residual=r) for o, r in zip(os_, rs)]
            else:
                with ops.launch_group(dev, side_streams):
                    ms = [blk["c2"](o) for o in os_]
                with ops.launch_group(dev, side_streams):
                    ys = [blk["c3"](m, residual=r) for m, r in zip(ms, rs)]
            xs = ys
        return xs


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
        x = ops.stem_conv_maxblur(x, self.conv1)  # conv1 + BN + ReLU + MaxPool2d(2, stride 1) + BlurPool/2 in one kernel
        for blk in self.blocks:
            o = blk["c1"](x)
            r = blk["ds"](ops.blurpool2d(x, blk["stride"])) if blk["ds"] is not None else x
            x = blk["c2"](o, residual=r)
        return x

    def forward_group(self, xs, side_streams=True):
        """The same pass over several inputs of DIFFERENT sizes (the shape groups of a ragged fine stage), layer by layer with one
        grouped launch per kernel instance and layer (ops.launch_group): bit-identical to [self(x) for x in xs].  Outputs get new
        names inside a group and are rebound after it (launch_group's contract, as in ResNet50Trunk.forward_group)."""
        dev = xs[0].device
        with ops.launch_group(dev, side_streams):
            xs = [ops.stem_conv_maxblur(x, self.conv1) for x in xs]
        for blk in self.blocks:
            with ops.launch_group(dev, side_streams):          # c1 and the shortcut's blur both read x only: one group
                os_ = [blk["c1"](x) for x in xs]
                bs = [ops.blurpool2d(x, blk["stride"]) for x in xs] if blk["ds"] is not None else None
            if bs is not None:
                with ops.launch_group(dev, side_streams):
                    rs = [blk["ds"](b) for b in bs]
            else:
                rs = xs
            with ops.launch_group(dev, side_streams):
                ys = [blk["c2"](o, residual=r) for o, r in zip(os_, rs)]
            xs = ys
        return xs


class _HeadTrunk:
    def __init__(self, sd, last_act, device):
        self.c1 = ConvPlan(sd["conv1.weight"], _bn(sd, "bn1"), 1, 1, ACT_RELU, device, split=True)      # 49 -> 512 (a ragged 4th channel block),
        self.c2 = ConvPlan(sd["conv2.weight"], _bn(sd, "bn2"), 1, 1, ACT_RELU, device, split=True)      # 512 -> 256, 256 -> 128:
        self.c3 = ConvPlan(sd["conv3.weight"], _bn(sd, "bn3"), 1, 1, ACT_RELU, device, split=True)      # rfx_conv3x3_split_f32
        self.c4 = ConvPlan(sd["conv4.weight"], None, 1, 1, last_act, device)

    def __call__(self, coef):
        return self.c4(self.c3(self.c2(self.c1(coef))))

    def forward_group(self, coefs, side_streams=True, halves_out=None):
        """[self(c) for c in coefs] for volumes of different sizes, one grouped launch per kernel instance and layer.  The 49-channel
        volumes must come from an earlier group: c1 copies them into its zero-padded input eagerly (launch_group's contract).
        ``halves_out``: one (out_a, out_b) per input -- the last convolution then runs on the two halves of each batch as two
        problems and writes them to out_a / out_b (views of two packed buffers: PredFlowMask's match12Down8 / match21Down8);
        returns those pairs."""
        dev = coefs[0].device
        xs = coefs
        for c in (self.c1, self.c2, self.c3):
            with ops.launch_group(dev, side_streams):
                ys = [c(x) for x in xs]
            xs = ys
        with ops.launch_group(dev, side_streams):
            if halves_out is None:
                ys = [self.c4(x) for x in xs]
            else:
                ys = [(self.c4(x[:x.shape[0] // 2], out=oa), self.c4(x[x.shape[0] // 2:], out=ob)) for x, (oa, ob) in zip(xs, halves_out)]
        return ys


class NetFlowCoarseNet:
    """model/model.py:167-249.  up8X=True -> F.upsample_bilinear x8 (align_corners=True, :234)."""

    def __init__(self, sd, kernelSize=7, device="cuda"):
        self.k = kernelSize
        self.trunk = _HeadTrunk(sd, ACT_NONE, device)

    def __call__(self, coef, up8X=True):
        flow = ops.flow_head(self.trunk(coef), self.k)
        if up8X:
            flow = ops.resize_bilinear(flow, (flow.shape[2] * 8, flow.shape[3] * 8), align_corners=True)
        return flow

    def forward_group(self, coefs, up8X=True, side_streams=True, outs=None):
        """[self(c, up8X) for c in coefs] for volumes of different sizes: the trunk, the flow head and the x8 resize as grouped
        launches, bit-identical to the per-input calls.  ``outs``: where the /8 flows go (views of a packed buffer)."""
        dev = coefs[0].device
        logits = self.trunk.forward_group(coefs, side_streams)
        with ops.launch_group(dev, side_streams):
            flows = [ops.flow_head(l, self.k, out=None if outs is None else outs[i]) for i, l in enumerate(logits)]
        if up8X:
            with ops.launch_group(dev, side_streams):
                ups = [ops.resize_bilinear(f, (f.shape[2] * 8, f.shape[3] * 8), align_corners=True) for f in flows]
            flows = ups
        return flows


class NetMatchabilityNet:
    """model/model.py:254-322: sigmoid fused into the last conv's epilogue."""

    def __init__(self, sd, kernelSize=7, device="cuda"):
        self.trunk = _HeadTrunk(sd, ACT_SIGMOID, device)

    def __call__(self, feat, up8X=True):
        m = self.trunk(feat)
        if up8X:
            m = ops.resize_bilinear(m, (m.shape[2] * 8, m.shape[3] * 8), align_corners=True)
        return m

    def forward_group(self, feats, up8X=True, side_streams=True):
        """[self(f, up8X) for f in feats] for volumes of different sizes, as grouped launches, bit-identical to the per-input calls."""
        dev = feats[0].device
        ms = self.trunk.forward_group(feats, side_streams)
        if up8X:
            with ops.launch_group(dev, side_streams):
                ups = [ops.resize_bilinear(m, (m.shape[2] * 8, m.shape[3] * 8), align_corners=True) for m in ms]
            ms = ups
        return ms
