"""Tensor-level wrappers over the librfx C ABI.

PyTorch is used for device memory and streams only: every function takes ``torch`` tensors that already
live on a HIP device, passes ``data_ptr()`` / sizes / that device's current torch stream to the C entry point
(``_call``: device-guarded) and returns freshly allocated output tensors.  No op has a CPU or eager-PyTorch fallback.
"""
import collections
import ctypes
import os
import threading

import torch

from . import _lib
from .cache import BoundedCache

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def _stream(dev=None):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _on_device(dev, fn, *args):
    """fn(*args, stream) with ``dev`` the HIP current device: the stream is torch's current stream OF THAT DEVICE, and the HIP
    current device is switched for the call when it is another one (ctypes bypasses torch's device guard)."""
    if dev.index is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return fn(*args, _stream(dev))
    return fn(*args, _stream())


def _call(name, dev, *args):
    """lib.<name>(*args, stream) on the device the tensors live on (_on_device)."""
    _lib.check(_on_device(dev, getattr(_lib.load(), name), *args), name)


def _one_device(*tensors):
    """All operands of an op must share one HIP device (foreign pointers fault or, worse, do not)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("rfx op operands live on different devices: %s and %s" % (dev, t.device))
    return dev


class Profiler:
    """Explicit, thread-local launch profiler (bench.py): inside ``with ops.Profiler() as prof:`` every
    convolution-class launch and every correlation launch of THIS thread is bracketed by two HIP events on the
    launch stream; nothing is recorded -- and no event is created -- outside such a block.

        prof.conv: list of (kernel_id, flops, ev0, ev1, shape, algorithmic_bytes)
        prof.corr: list of (algorithmic_bytes, ev0, ev1)                       one-direction launches
        prof.corr_bidir: list of (minimal_bytes, per_direction_bytes, ev0, ev1)   both directions of a pair in one launch
    """
    _tls = threading.local()

    def __init__(self):
        self.conv, self.corr, self.corr_bidir = [], [], []
        self.corr_kernel_us = None      # kernel durations of the correlation launches in launch order (corr_durations())
        self._corr_order = []           # "one" / "bidir" per captured launch

    def __enter__(self):
        self._prev = getattr(Profiler._tls, "active", None)
        Profiler._tls.active = self
        # the correlation launches of this thread carry dispatch-level start / stop events from here on (rfx_corr_timing)
        self._prev_timing = _lib.load().rfx_corr_timing(1)
        _lib.load().rfx_corr_timing_collect(None, 0)          # drop captures nobody collected
        return self

    def __exit__(self, *exc):
        Profiler._tls.active = self._prev
        _lib.load().rfx_corr_timing(self._prev_timing)
        return False

    def corr_durations(self):
        """Kernel durations (us) of the captured correlation launches: (one-direction list, bidir list), each in launch order.
        Call after the profiled region (synchronises on the captured events)."""
        if self.corr_kernel_us is None:
            n = len(self._corr_order)
            buf = (ctypes.c_float * max(n, 1))()
            got = _lib.load().rfx_corr_timing_collect(buf, n)
            us = [float(buf[i]) for i in range(n)] if got == n else []      # a launch that bypassed the DMA kernels: no pairing possible
            self.corr_kernel_us = ([u for u, k in zip(us, self._corr_order) if k == "one"],
                                   [u for u, k in zip(us, self._corr_order) if k == "bidir"])
        return self.corr_kernel_us

    @staticmethod
    def active():
        return getattr(Profiler._tls, "active", None)

    @staticmethod
    def begin(dev=None):
        """Start event on the current stream OF THE DEVICE THE LAUNCH GOES TO (``dev``: a tensor of the op or its device;
        default: the current device) -- the stream _call() launches on."""
        if getattr(Profiler._tls, "active", None) is None:
            return None
        dev = dev.device if isinstance(dev, torch.Tensor) else dev
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(dev))
        e0._rfx_dev = dev
        return e0

    @staticmethod
    def end(e0):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(torch.cuda.current_stream(getattr(e0, "_rfx_dev", None)))
        return e1

    @staticmethod
    def record_conv(kid, flops, e0, shape, nbytes):
        """End the event pair ``e0`` opened and append the launch's ``conv`` tuple (bench.py decodes exactly this layout)."""
        Profiler.active().conv.append((kid, flops, e0, Profiler.end(e0), shape, nbytes))


class launch_group:
    """``with ops.launch_group(device):`` -- the convolution ops and the fine-stage ops (stem_conv_maxblur, blurpool2d, l2norm,
    flow_head, resize_bilinear, corr_neigh / corr_neigh_bidir, warp_grid, grid_sample, compose_flow, cycle_tail) issued inside are RECORDED by
    the library and launched at exit as ONE launch per kernel instance (rfx_group_begin / rfx_group_end: blockIdx.y selects the
    problem).  For the same layer of several independent inputs of different sizes; chains use it through ``stage``, which also
    keeps the one rule: a recorded op may not READ an output of the same group, on the device or with an eager torch op.  Not used
    under a Profiler (per-launch events are meaningless for a recorded launch: callers take their per-problem path).  Operands must
    stay referenced until the block ends; temporaries an op makes for a recorded launch are held by the block (``keep``): the side
    streams join the caller's stream before rfx_group_end returns, so releasing them then is stream-ordered."""
    _tls = threading.local()

    def __init__(self, device, side_streams=True):
        # side_streams=False: the group's kernel instances stay on the caller's stream (rfx_group_side_streams) -- for callers that
        # run several grouped chains on streams of their own
        self.dev, self.side = torch.device(device), bool(side_streams)
        self._held = []

    @staticmethod
    def recording():
        """True inside a ``with ops.launch_group(...)`` block of this thread."""
        return getattr(launch_group._tls, "active", None) is not None

    @staticmethod
    def keep(t):
        """Hold ``t`` until the active group (if any) has launched: a recorded launch reads its operands at the block's end."""
        g = getattr(launch_group._tls, "active", None)
        if g is not None:
            g._held.append(t)

    def __enter__(self):
        _lib.check(_lib.load().rfx_group_begin(), "rfx_group_begin")
        self._prev = getattr(launch_group._tls, "active", None)
        launch_group._tls.active = self
        return self

    def __exit__(self, et, ev, tb):
        lib = _lib.load()
        launch_group._tls.active = self._prev
        try:
            if et is not None:
                lib.rfx_group_abort()
                return False
            prev = lib.rfx_group_side_streams(1 if self.side else 0)
            try:
                rc = _on_device(self.dev, lib.rfx_group_end)
            finally:
                lib.rfx_group_side_streams(prev)
            _lib.check(rc, "rfx_group_end")
            return False
        finally:
            self._held = []


def group_stats():
    """(groups, launches): this thread's cumulative number of launch_group blocks that ended (rfx_group_end) and of the kernel
    launches they issued (rfx_group_stats)."""
    g, n = ctypes.c_longlong(0), ctypes.c_longlong(0)
    _lib.check(_lib.load().rfx_group_stats(ctypes.byref(g), ctypes.byref(n)), "rfx_group_stats")
    return g.value, n.value


def stage(fn, *lists, device, side_streams=True):
    """[fn(*row) for row in zip(*lists)] as ONE launch step of a chain over equally long lists (one entry per problem).  Several
    rows: the calls are recorded in one launch_group(device, side_streams).  One row: fn is called directly -- no group, the
    single-launch kernel on the current stream, so Profiler events and the correlation's timing capture work as for any eager call.
    fn receives only its row, which the caller took from EARLIER stages' results: that is what keeps a recorded op from reading an
    output of its own group.  An eager read inside fn (ConvPlan's copy of a 49-channel input) is of an earlier stage for the same
    reason.  Ops that cannot be recorded (match_score, torch ops) stay plain list comprehensions between stages."""
    if len({len(l) for l in lists}) != 1:
        raise ValueError("stage: lists of different lengths")
    rows = list(zip(*lists))
    if len(rows) == 1:
        return [fn(*rows[0])]
    with launch_group(device, side_streams):
        return [fn(*row) for row in rows]


def _dev(t, name="tensor", dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: rfx ops run only on a HIP device (no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.is_contiguous():
        return t
    t = t.contiguous()
    launch_group.keep(t)          # a recorded launch reads the copy at the group's end
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


KID_SPLIT_3X3 = 65536      # ... of rfx_conv3x3_split_f32
KID_SPLIT_1X1 = 32768      # Profiler kernel id of rfx_conv1x1_split_f32 (| 1: 64-channel tiles, | 2: 128-channel tiles)
KID_DIRECT_3X3 = 32        # bit 5 of the library's ids (include/rfx_api.h, rfx_conv2d_kernel_id): served by rfx_conv3x3_f32
KID_DIRECT_3X3_S2 = 8192   # bit 13: served by rfx_conv3x3_s2_f32


# on by default: measured 1.057x on the ragged multi-homography call, its slowest repetition below the per-group form's fastest
# (profiles/ragged_fine_groups_bench.json)
FINE_GROUPS_DEFAULT = True


def fine_groups_enabled(env=None):
    """RFX_FINE_GROUPS: the fine stage of the ragged drivers (rounds.RaggedGroup, AlignPipeline._fine_ragged) as ONE chain of grouped
    launches over all shape groups (AlignPipeline.pred_flow_mask_groups / pred_flow_mask_cycle_groups / kitti_fine_round_groups /
    fine_quickstart_groups) instead of one chain per shape group.  "1" / "0"; unset = FINE_GROUPS_DEFAULT (and, in the round drivers,
    the driver's own ``grouped_fine``).  Always off under a Profiler (grouped launches are not profiled)."""
    env = os.environ if env is None else env
    v = str(env.get("RFX_FINE_GROUPS", "")).strip()
    on = FINE_GROUPS_DEFAULT if v == "" else v != "0"
    return on and Profiler.active() is None


def _out_or_new(out, shape, ref, what):
    """``out`` checked against ``shape`` (a contiguous float32 tensor on ref's device, e.g. a view of a packed buffer), or a new tensor."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=ref.device)
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != ref.device:
        raise ValueError("%s: out must be a contiguous float32 %s tensor on %s" % (what, tuple(shape), ref.device))
    return out


def conv_split_enabled():
    """RFX_CONV_SPLIT=0: every convolution on the fp32 MFMA kernels (A/B runs; the float32-only figure of the bench line)."""
    return os.environ.get("RFX_CONV_SPLIT", "1") != "0"


def split_weights(w2d):
    """(Cout, Cin) float32 -> rfx_conv1x1_split_f32's wS: the three bf16 pieces of every weight (hi = bf16(w), mid = bf16(w - hi),
    lo = bf16(w - hi - mid); round to nearest even, hi + mid + lo == w exactly) in fragment order
    [k / 16][piece][(k % 16) / 8][m (Mpad)][k % 8], as int16 bit patterns."""
    w = w2d.detach().float().cpu()
    Cout, Cin = w.shape
    if Cin % 16:       # a ragged last block (rfx_conv3x3_split_f32 stages the missing channels as zeros): zero weights
        w = torch.cat((w, torch.zeros(Cout, 16 - Cin % 16)), dim=1)
        Cin = w.shape[1]
    hi = w.bfloat16()
    r1 = w - hi.float()
    mid = r1.bfloat16()
    lo = (r1 - mid.float()).bfloat16()
    Mpad = (Cout + 127) // 128 * 128
    pieces = torch.zeros(3, Mpad, Cin, dtype=torch.bfloat16)
    pieces[:, :Cout] = torch.stack((hi, mid, lo))
    return pieces.view(3, Mpad, Cin // 16, 2, 8).permute(2, 0, 3, 1, 4).contiguous().view(torch.int16)


def split_weights_3x3(w):
    """(Cout, Cin, 3, 3) float32 -> rfx_conv3x3_split_f32's wS3: split_weights of every tap, [c / 16][tap][piece][h][m][8]."""
    return torch.stack([split_weights(w[:, :, kh, kw]) for kh in range(3) for kw in range(3)], dim=1).contiguous()


def pack_wT(w):
    """(Cout, Cin, KH, KW) float32 -> rfx_conv2d_f32's wT: the (K, Cout) transpose, zero-padded to (Kpad, Mpad) (32 / 128)."""
    Cout, K = w.shape[0], w[0].numel()
    wT = torch.zeros((K + 31) // 32 * 32, (Cout + 127) // 128 * 128, dtype=torch.float32)
    wT[:K, :Cout] = w.reshape(Cout, K).t()
    return wT


def pack_ktab(w, dilation=1):
    """rfx_conv2d_f32's gather table of a (Cout, Cin, KH, KW) weight: per k, c << 8 | row offset << 4 | column offset (-1 past K)."""
    _, Cin, KH, KW = w.shape
    K = Cin * KH * KW
    k = torch.arange(K)
    c, r = k // (KH * KW), k % (KH * KW)
    ktab = torch.full(((K + 31) // 32 * 32,), -1, dtype=torch.int32)
    # the gather adds these offsets to the window origin as they are: a dilated convolution stores kh*d / kw*d
    ktab[:K] = ((c << 8) | (((r // KW) * dilation) << 4) | ((r % KW) * dilation)).int()
    # per 32-k block: [16 even k | 16 odd k] (the order in which one MFMA lane-half consumes them)
    return ktab.view(-1, 16, 2).permute(0, 2, 1).reshape(-1).contiguous()


def pack_wP(w):
    """(Cout, Cin, 3, 3) float32 -> rfx_conv3x3_f32's order: wP[mt][s][h][m][kk] = W[mt*128 + m][s*72 + 2*kk + h]; a Cin that is not
    a multiple of 8 (the 49-channel correlation volume) gets zero rows for the missing channels of its last K step."""
    Cout, Cin = w.shape[:2]
    Mpad, Kp = (Cout + 127) // 128 * 128, (Cin + 7) // 8 * 72
    wp = torch.zeros(Mpad, Kp, dtype=torch.float32)
    wp[:Cout, :Cin * 9] = w.reshape(Cout, Cin * 9)
    return wp.view(Mpad // 128, 128, Kp // 72, 36, 2).permute(0, 2, 4, 1, 3).contiguous()


def pack_wQ(w2d):
    """(Cout, Cin) float32 -> 1x1 weights in the order rfx_conv3x3_conv1x1_f32 reads them: wQ[q][h][m][j] = W[m][8q + 2j + h]."""
    Cout, Cin = w2d.shape
    return w2d.t().reshape(Cin // 8, 4, 2, Cout).permute(0, 2, 3, 1).contiguous()      # [q][j][h][m] -> [q][h][m][j]


def conv_route(Cin, Cout, KH, KW, stride, pad, dilation, split, split_enabled):
    """The kernel family a convolution of this geometry runs on, fixed when its plan is built (``split``: the caller asked for the
    split kernels; ``split_enabled``: conv_split_enabled()).  Each route holds only its own weight packs:
        dilated      rfx_conv2d_dilated_f32                                                     wT + ktab
        split3x3     rfx_conv3x3_split_f32                                                      wS
        split3x3_s2  rfx_conv3x3_split_s2_f32                                                   wS
        split1x1     rfx_conv1x1_split_f32 / rfx_conv1x1_split_strided_f32 (stride 2)           wS
        fp32_3x3     rfx_conv3x3_f32 / rfx_conv3x3_s2_f32, or rfx_conv2d_f32 where the library's
                     *_kernel_id says so for the launch's shape                                 wP + wT + ktab
        gemm         rfx_conv2d_f32 (implicit GEMM; the k-major 1x1 kernel is one of its instances)   wT + ktab"""
    if dilation != 1:
        return "dilated"
    if split and split_enabled:
        if KH == 1 and KW == 1 and stride in (1, 2) and pad == 0 and Cin % 16 == 0:
            return "split1x1"
        if KH == 3 and KW == 3 and pad == 1:
            if stride == 1 and Cin >= 16:
                return "split3x3"
            if stride == 2 and Cin % 16 == 0 and Cout >= 128:
                return "split3x3_s2"
    if KH == 3 and KW == 3 and pad == 1 and Cin >= 8 and (stride == 1 or (stride == 2 and Cin % 8 == 0)):
        return "fp32_3x3"
    return "gemm"


class ConvPlan:
    """Packed weights + folded BatchNorm of one convolution (see rfx_conv2d_f32 in include/rfx_api.h).  ``route`` (conv_route) names
    the kernel family every call goes to; the packs of the other routes are None."""

    def __init__(self, weight, bn=None, stride=1, pad=0, act=ACT_NONE, device=None, eps=1e-5, dilation=1, bias=None, split=False):
        # weight: (Cout, Cin, KH, KW) float32 (any device); bn: dict(weight,bias,running_mean,running_var) or None;
        # dilation > 1: rfx_conv2d_dilated_f32 (the sky-segmentation encoder, segNet/segModel.py:196-205); bias: the convolution's own
        # bias (segModel.py:243,245: the classifier convolutions), only without bn;
        # split=True: the convolution runs on the split kernels (float32 sums from exact bf16 operand pieces on the bf16 matrix
        # cores: csrc/conv1x1s.hip, csrc/conv3x3s.hip) where the shape allows it and RFX_CONV_SPLIT != 0
        w = weight.detach().float().cpu()
        self.Cout, self.Cin, self.KH, self.KW = w.shape
        self.stride, self.pad, self.act, self.dilation = stride, pad, act, int(dilation)
        if bias is not None and bn is not None:
            raise ValueError("ConvPlan: a convolution bias together with a BatchNorm is not folded here")
        # rfx_conv3x3_f32's k_chunk: 0 = the library's rule (chunks for K >= 2048); 4 = chunks of 4 K steps whatever K is -- set by
        # the nets on the 3x3 convolution of a Bottleneck tail, so that the two-kernel form equals the fused kernel bit for bit
        self.k_chunk = 0
        self.route = conv_route(self.Cin, self.Cout, self.KH, self.KW, stride, pad, self.dilation, split, conv_split_enabled())
        dev = self._device = device or "cuda"
        # every pack of the route is uploaded here, never at first use: a first use inside a HIP-graph capture would capture the copy
        self.wS = self.wP = self.wT = self.ktab = None
        if self.route == "split1x1":
            self.wS = split_weights(w.reshape(self.Cout, self.Cin)).to(dev)
        elif self.route in ("split3x3", "split3x3_s2"):
            self.wS = split_weights_3x3(w).to(dev)
        else:
            self.wT, self.ktab = pack_wT(w).to(dev), pack_ktab(w, self.dilation).to(dev)
            if self.route == "fp32_3x3":
                self.wP = pack_wP(w).to(dev)
        self.w2d = w.reshape(self.Cout, self.Cin) if (self.KH == 1 and self.KW == 1) else None   # kept for quad_weights()
        self._wq = None
        if bn is not None:
            # eval-mode BatchNorm as ATen's CPU kernel evaluates it: alpha = w * (1/sqrt(var+eps)), beta = b - mean*alpha
            invstd = 1.0 / torch.sqrt(bn["running_var"].detach().float().cpu() + eps)
            alpha = bn["weight"].detach().float().cpu() * invstd
            beta = bn["bias"].detach().float().cpu() - bn["running_mean"].detach().float().cpu() * alpha
            self.scale, self.shift = alpha.to(dev), beta.to(dev)
        elif bias is not None:
            self.scale, self.shift = torch.ones(self.Cout, dtype=torch.float32).to(dev), bias.detach().float().cpu().to(dev)
        else:
            self.scale = self.shift = None

    def quad_weights(self):
        """pack_wQ of a 1x1 plan on its device, for rfx_conv3x3_conv1x1_f32 (cached; the nets' first use is in the warm-up)."""
        if getattr(self, "_wq", None) is None:
            self._wq = pack_wQ(self.w2d).to(self._device)
        return self._wq

    def out_hw(self, H, W):
        eh, ew = (self.KH - 1) * self.dilation + 1, (self.KW - 1) * self.dilation + 1
        return (H + 2 * self.pad - eh) // self.stride + 1, (W + 2 * self.pad - ew) // self.stride + 1

    def __call__(self, x, residual=None, act=None, out=None):
        x = _dev(x, "conv input")
        N, C, H, W = x.shape
        if C != self.Cin:
            raise ValueError("conv expects %d input channels, got %d" % (self.Cin, C))
        Ho, Wo = self.out_hw(H, W)
        out = _out_or_new(out, (N, self.Cout, Ho, Wo), x, "conv")
        res = _dev(residual, "residual") if residual is not None else None
        if res is not None and res.shape != out.shape:
            raise ValueError("residual shape %s != output shape %s" % (tuple(res.shape), tuple(out.shape)))
        self._RUN[self.route](self, x, res, out, self.act if act is None else act)
        return out

    # One method per route: launch into ``out`` and, under a Profiler, record the launch.

    def _run_dilated(self, x, res, out, act):       # records nothing
        N, C, H, W = x.shape
        _call("rfx_conv2d_dilated_f32", _one_device(x, res, self.wT), _p(x), _p(self.wT), _p(self.ktab), _p(self.scale), _p(self.shift),
              _p(res), _p(out), N, C, H, W, self.Cout, self.KH, self.KW, self.stride, self.pad, self.dilation, act)

    def _run_split3x3(self, x, res, out, act):      # both strides
        N, C, H, W = x.shape
        e0 = Profiler.begin(x)
        xin, Cp = x, C
        if C % 16:
            # the 49-channel correlation volume: the kernel takes whole blocks of 16 channels -- the input goes into a zero-padded
            # buffer (one device copy, 5 % of the layer's time; the padded weights are zero: split_weights)
            Cp = (C + 15) // 16 * 16
            xin = torch.zeros((N, Cp, H, W), dtype=torch.float32, device=x.device)
            xin[:, :C].copy_(x)
            launch_group.keep(xin)              # inside a group the kernel reads it at the block's end, after this call returns
        _call("rfx_conv3x3_split_f32" if self.stride == 1 else "rfx_conv3x3_split_s2_f32", _one_device(xin, res, self.wS), _p(xin),
              _p(self.wS), _p(self.scale), _p(self.shift), _p(res), _p(out), N, Cp, H, W, self.Cout, act)
        if e0 is not None:
            Ho, Wo = out.shape[2:]
            Profiler.record_conv(KID_SPLIT_3X3 | (2 if self.Cout > 64 else 1) | (4 if self.stride != 1 else 0),
                                 2.0 * N * Ho * Wo * self.Cout * self.Cin * 9, e0, (N, self.Cin, H, W, self.Cout, 3, self.stride),
                                 4.0 * (N * C * H * W + N * self.Cout * Ho * Wo * (2 if res is not None else 1)) + 54.0 * self.Cout * self.Cin)

    def _run_split1x1(self, x, res, out, act):
        N, C, H, W = x.shape
        e0 = Profiler.begin(x)
        if self.stride == 1:
            _call("rfx_conv1x1_split_f32", _one_device(x, res, self.wS), _p(x), _p(self.wS), _p(self.scale), _p(self.shift), _p(res), _p(out),
                  N, C, H * W, self.Cout, act)
        else:
            _call("rfx_conv1x1_split_strided_f32", _one_device(x, res, self.wS), _p(x), _p(self.wS), _p(self.scale), _p(self.shift), _p(res),
                  _p(out), N, C, H, W, self.Cout, self.stride, act)
        if e0 is not None:
            Ho, Wo = out.shape[2:]
            Profiler.record_conv(KID_SPLIT_1X1 | (2 if self.Cout > 64 else 1) | (4 if self.stride != 1 else 0),
                                 2.0 * N * Ho * Wo * self.Cout * self.Cin, e0, (N, self.Cin, H, W, self.Cout, 1, self.stride),
                                 4.0 * (N * C * Ho * Wo + N * self.Cout * Ho * Wo * (2 if res is not None else 1)) + 6.0 * self.Cout * self.Cin)

    def _run_fp32_3x3(self, x, res, out, act):
        # the direct kernels where the library takes them for this launch's shape, else the implicit GEMM
        N, C, H, W = x.shape
        Ho, Wo = out.shape[2:]
        lib = _lib.load()
        kid0 = (lib.rfx_conv3x3_kernel_id(N, self.Cin, self.Cout, Ho, Wo, self.k_chunk) if self.stride == 1 else
                lib.rfx_conv2d_kernel_id(N, self.Cin, self.Cout, self.KH, self.KW, self.stride, self.pad, Ho, Wo))
        if not kid0 & (KID_DIRECT_3X3 | KID_DIRECT_3X3_S2):
            return self._run_gemm(x, res, out, act)
        e0 = Profiler.begin(x)
        if kid0 & KID_DIRECT_3X3:
            _call("rfx_conv3x3_f32", _one_device(x, res, self.wP), _p(x), _p(self.wP), _p(self.scale), _p(self.shift),
                  _p(res), _p(out), N, C, H, W, self.Cout, act, self.k_chunk)
        else:
            _call("rfx_conv3x3_s2_f32", _one_device(x, res, self.wP), _p(x), _p(self.wP), _p(self.scale), _p(self.shift),
                  _p(res), _p(out), N, C, H, W, self.Cout, act)
        if e0 is not None:
            self._record_fp32(kid0, e0, x, res, out)

    def _run_gemm(self, x, res, out, act):
        N, C, H, W = x.shape
        e0 = Profiler.begin(x)
        _call("rfx_conv2d_f32", _one_device(x, res, self.wT), _p(x), _p(self.wT), _p(self.ktab), _p(self.scale),
              _p(self.shift), _p(res), _p(out), N, C, H, W, self.Cout, self.KH, self.KW, self.stride, self.pad, act)
        if e0 is not None:
            self._record_fp32(0, e0, x, res, out)

    def _record_fp32(self, kid0, e0, x, res, out):
        N, C, H, W = x.shape
        Ho, Wo = out.shape[2:]
        kid = kid0 if (kid0 & KID_DIRECT_3X3) else _lib.load().rfx_conv2d_kernel_id(N, self.Cin, self.Cout, self.KH, self.KW, self.stride, self.pad, Ho, Wo)
        flops = 2.0 * N * Ho * Wo * self.Cout * self.Cin * self.KH * self.KW
        nbytes = 4.0 * (N * C * H * W + N * self.Cout * Ho * Wo * (2 if res is not None else 1)
                        + self.Cout * self.Cin * self.KH * self.KW)
        Profiler.record_conv(kid, flops, e0, (N, self.Cin, H, W, self.Cout, self.KH, self.stride), nbytes)

    _RUN = {"dilated": _run_dilated, "split3x3": _run_split3x3, "split3x3_s2": _run_split3x3, "split1x1": _run_split1x1,
            "fp32_3x3": _run_fp32_3x3, "gemm": _run_gemm}


# what bottleneck_tail_shape reads of a plan: the nets ask it about a layer before they pack anything (scale: not None where a
# BatchNorm or a bias is folded)
ConvGeometry = collections.namedtuple("ConvGeometry", "Cout Cin KH KW stride pad act scale")


def bottleneck_tail_shape(plan2, plan3):
    """Do conv2 (3x3) + conv3 (1x1 expansion) of a Bottleneck have the shape rfx_conv3x3_conv1x1_f32 serves?  (ConvPlans or
    ConvGeometry tuples.)"""
    return (plan2.KH == 3 and plan2.KW == 3 and plan2.stride == 1 and plan2.pad == 1 and plan2.Cin % 8 == 0
            and plan2.Cout in (64, 128) and plan2.act in (ACT_NONE, ACT_RELU) and plan3.KH == 1 and plan3.KW == 1
            and plan3.stride == 1 and plan3.pad == 0 and plan3.Cin == plan2.Cout and plan3.Cout % 128 == 0
            and plan3.act in (ACT_NONE, ACT_RELU) and plan3.scale is not None)


def bottleneck_tail_eligible(plan2, plan3):
    """Can conv2 (3x3) + conv3 (1x1 expansion) of a Bottleneck run as one kernel (rfx_conv3x3_conv1x1_f32)?"""
    return (bottleneck_tail_shape(plan2, plan3) and os.environ.get("RFX_FUSE_BOTTLENECK", "1") != "0"
            and getattr(plan2, "wS", None) is None and getattr(plan3, "wS", None) is None)        # split plans run as two kernels


def bottleneck_tail(x, plan2, plan3, residual=None):
    """plan3(plan2(x), residual) in one kernel: the plan2.Cout-channel intermediate stays in LDS."""
    x = _dev(x, "bottleneck input")
    N, C, H, W = x.shape
    if C != plan2.Cin:
        raise ValueError("conv expects %d input channels, got %d" % (plan2.Cin, C))
    res = _dev(residual, "residual") if residual is not None else None
    out = torch.empty((N, plan3.Cout, H, W), dtype=torch.float32, device=x.device)
    if res is not None and res.shape != out.shape:
        raise ValueError("residual shape %s != output shape %s" % (tuple(res.shape), tuple(out.shape)))
    e0 = Profiler.begin(x)
    _call("rfx_conv3x3_conv1x1_f32", _one_device(x, res, plan2.wP, plan3.scale), _p(x), _p(plan2.wP), _p(plan2.scale),
          _p(plan2.shift), plan2.act, _p(plan3.quad_weights()), _p(plan3.scale), _p(plan3.shift), _p(res), plan3.act,
          _p(out), N, C, H, W, plan2.Cout, plan3.Cout)
    if e0 is not None:
        Profiler.record_conv(_lib.load().rfx_conv3x3_conv1x1_kernel_id(N, H, W, plan2.Cout),
                             2.0 * N * H * W * (plan2.Cout * plan2.Cin * 9 + plan3.Cout * plan3.Cin), e0, (N, C, H, W, plan3.Cout, 3, 1),
                             4.0 * N * H * W * (C + plan3.Cout * (2 if res is not None else 1)))
    return out


_EXPAND64 = None      # RFX_EXPAND64, read once (expand64_enabled)


def expand64_enabled():
    """RFX_EXPAND64=0 (environment, read once per process): the 64 -> 256 expansions of the trunk's layer1 stay on rfx_conv2d_f32's
    k-major kernel, shortcut and conv3 as two launches (A/B runs and tests).  Both settings return the same bits."""
    global _EXPAND64
    if _EXPAND64 is None:
        _EXPAND64 = os.environ.get("RFX_EXPAND64", "1") != "0"
    return _EXPAND64


def expand64_eligible(plan):
    """Does a convolution (ConvPlan or ConvGeometry) have the geometry rfx_conv1x1_expand64_f32 serves?  1x1, stride 1, pad 0,
    Cin = 64, Cout a multiple of the 256 channels a workgroup's resident weights cover (and no more than them), a folded scale, activation
    none or ReLU.  Pure: no environment, no device."""
    return (plan.KH == 1 and plan.KW == 1 and plan.stride == 1 and plan.pad == 0 and getattr(plan, "dilation", 1) == 1
            and plan.Cin == 64 and plan.Cout % 256 == 0 and plan.Cout <= 256 and plan.scale is not None
            and plan.act in (ACT_NONE, ACT_RELU))


# Launch sizes (N * H * W pixels) from which the measured rule sends a form to conv1x1e.hip (scripts/ubench/expand64_bench.py,
# profiles/expand64_ab.json).  The persistent launch costs ~35 us (plain) / ~50 us (two-source) before its first
# tile -- every workgroup copies the weights into LDS -- so single pairs' maps (<= 76 800 pixels) stay on rfx_conv2d_f32's
# launches; between the two limits only the two-source form wins by more than the old launches' spread (plain at 271 360 pixels:
# 1.03x, inside it).
EXPAND64_MIN_PIXELS = {"plain": 300000, "dual": 100000}


def expand64_form(plan3, plan_ds=None, pixels=None):
    """The form of rfx_conv1x1_expand64_f32 a Bottleneck's conv3 takes: "dual" (with its projection shortcut ``plan_ds``, ACT_NONE,
    over the same pixels), "plain" (conv3 + residual alone) or None (rfx_conv2d_f32's launches: RFX_EXPAND64=0, a geometry the
    kernel does not serve, a plan on another route, or -- ``pixels`` given -- a launch size at which the old launches measured no
    slower).  A block whose shortcut is ineligible takes no form at all: its conv3 would read the shortcut back from memory."""
    def ok(p):
        return expand64_eligible(p) and getattr(p, "route", "gemm") == "gemm"
    if not expand64_enabled() or not ok(plan3) or plan3.act != ACT_RELU:
        return None
    if plan_ds is not None:
        form = "dual" if (ok(plan_ds) and plan_ds.act == ACT_NONE and plan_ds.Cout == plan3.Cout) else None
    else:
        form = "plain"
    if form is not None and pixels is not None and pixels < EXPAND64_MIN_PIXELS[form]:
        return None
    return form


def conv1x1_expand64(x, plan, residual=None, shortcut=None):
    """plan(x, residual=residual) -- or, with ``shortcut`` = (xs, plan_s), plan(x, residual=plan_s(xs)) -- on conv1x1e.hip where
    expand64_form() says so for this launch, else as those calls themselves (also inside a launch_group, whose grouped launches
    keep rfx_conv2d_f32's kernels): the same bits either way.  Under a Profiler the launch is recorded under the kernel id
    rfx_conv2d_f32 runs ``plan`` at for this geometry, with the FLOPs of both GEMMs and the bytes the launch moves."""
    if residual is not None and shortcut is not None:
        raise ValueError("conv1x1_expand64: a residual or a shortcut, not both")
    x = _dev(x, "conv input")
    N, C, H, W = x.shape
    plan_s = shortcut[1] if shortcut is not None else None
    form = expand64_form(plan, plan_s, N * H * W)
    if getattr(launch_group._tls, "active", None) is not None:
        form = None
    if form is None:
        return plan(x, residual=plan_s(shortcut[0]) if shortcut is not None else residual)
    if C != plan.Cin:
        raise ValueError("conv expects %d input channels, got %d" % (plan.Cin, C))
    out = torch.empty((N, plan.Cout, H, W), dtype=torch.float32, device=x.device)
    e0 = Profiler.begin(x)
    if form == "dual":
        xs = _dev(shortcut[0], "shortcut input")
        if xs.shape != x.shape:
            raise ValueError("shortcut input shape %s != conv input shape %s" % (tuple(xs.shape), tuple(x.shape)))
        _call("rfx_conv1x1_expand64_dual_f32", _one_device(x, xs, plan.wT, plan_s.wT), _p(x), _p(plan.wT), _p(plan.scale), _p(plan.shift),
              _p(xs), _p(plan_s.wT), _p(plan_s.scale), _p(plan_s.shift), _p(out), N, C, H * W, plan.Cout, 1)
    else:
        res = _dev(residual, "residual") if residual is not None else None
        if res is not None and res.shape != out.shape:
            raise ValueError("residual shape %s != output shape %s" % (tuple(res.shape), tuple(out.shape)))
        _call("rfx_conv1x1_expand64_f32", _one_device(x, res, plan.wT), _p(x), _p(plan.wT), _p(plan.scale), _p(plan.shift), _p(res), _p(out),
              N, C, H * W, plan.Cout, 1, plan.act)
    if e0 is not None:
        gemms = 2 if form == "dual" else 1
        planes = plan.Cout * (2 if (form == "plain" and residual is not None) else 1)
        Profiler.record_conv(_lib.load().rfx_conv2d_kernel_id(N, plan.Cin, plan.Cout, 1, 1, 1, 0, H, W),
                             gemms * 2.0 * N * H * W * plan.Cout * plan.Cin, e0, (N, plan.Cin, H, W, plan.Cout, 1, 1),
                             4.0 * (N * H * W * (gemms * C + planes) + gemms * plan.Cout * plan.Cin))
    return out


def maxpool2d(x, k, stride, pad=0):
    x = _dev(x, "maxpool input")
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    _call("rfx_maxpool2d_f32", x.device, _p(x), _p(out), N * C, H, W, k, stride, pad)
    return out


def blurpool2d(x, stride=2):
    x = _dev(x, "blurpool input")
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    _call("rfx_blurpool2d_f32", x.device, _p(x), _p(out), N * C, H, W, stride)
    return out


def maxblurpool2d(x, stride=2):
    """MaxPool2d(2, stride 1) + BlurPool(stride) fused (FeatureExtractor stem)."""
    x = _dev(x, "maxblurpool input")
    N, C, H, W = x.shape
    Ho, Wo = (H - 2) // stride + 1, (W - 2) // stride + 1
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    _call("rfx_maxblurpool2d_f32", x.device, _p(x), _p(out), N * C, H, W, stride)
    return out


def stem_conv_maxblur(x, plan):
    """FeatureExtractor stem: plan = ConvPlan of the 3x3 / stride 1 / pad 1 / ReLU convolution with 3 input channels;
    returns maxblurpool2d(plan(x), 2) without materialising plan(x)."""
    x = _dev(x, "stem input")
    N, C, H, W = x.shape
    if not (C == 3 and plan.Cin == 3 and plan.KH == 3 and plan.KW == 3 and plan.stride == 1 and plan.pad == 1
            and plan.act == ACT_RELU and plan.Cout % 32 == 0):
        raise ValueError("stem_conv_maxblur: not a 3x3/s1/p1 ReLU convolution of a 3-channel image")
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    out = torch.empty((N, plan.Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    e0 = Profiler.begin(x)
    _call("rfx_stem_conv3x3_maxblur_f32", _one_device(x, plan.wT), _p(x), _p(plan.wT), _p(plan.scale), _p(plan.shift), _p(out), N, H, W,
                                                       plan.Cout)
    if e0 is not None:
        Profiler.record_conv(256, 2.0 * N * H * W * plan.Cout * 27, e0, (N, 3, H, W, plan.Cout, 3, 1),
                             4.0 * (N * 3 * H * W + N * plan.Cout * Ho * Wo))
    return out


def stem_conv7_maxpool(x, plan):
    """ResNet-50 stem: plan = ConvPlan of the 7x7 / stride 2 / pad 3 / ReLU convolution with 3 input channels; returns
    maxpool2d(plan(x), 3, 2, 1) without materialising plan(x)."""
    x = _dev(x, "stem input")
    N, C, H, W = x.shape
    if not (C == 3 and plan.Cin == 3 and plan.KH == 7 and plan.KW == 7 and plan.stride == 2 and plan.pad == 3
            and plan.act == ACT_RELU and plan.Cout % 32 == 0):
        raise ValueError("stem_conv7_maxpool: not a 7x7/s2/p3 ReLU convolution of a 3-channel image")
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = torch.empty((N, plan.Cout, Hp, Wp), dtype=torch.float32, device=x.device)
    e0 = Profiler.begin(x)
    _call("rfx_stem_conv7x7_maxpool_f32", _one_device(x, plan.wT), _p(x), _p(plan.wT), _p(plan.scale), _p(plan.shift), _p(out), N, H, W,
                                                       plan.Cout)
    if e0 is not None:
        Profiler.record_conv(257, 2.0 * N * Hc * Wc * plan.Cout * 147, e0, (N, 3, H, W, plan.Cout, 7, 2),
                             4.0 * (N * 3 * H * W + N * plan.Cout * Hp * Wp))
    return out


def adaptive_avgpool2d(x, size):
    """nn.AdaptiveAvgPool2d(size) (segNet/segModel.py:227)."""
    x = _dev(x, "adaptive_avgpool input")
    N, C, H, W = x.shape
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    _call("rfx_adaptive_avgpool2d_f32", x.device, _p(x), _p(out), N * C, H, W, Ho, Wo)
    return out


def softmax_accum(logits, scores=None, div=1.0):
    """scores (+)= softmax(logits, dim=1) / div for (N,C,H,W) logits (segNet/segModel.py:258 + segNet/segEval.py:34-35); a new
    tensor when ``scores`` is None, else updated IN PLACE."""
    logits = _dev(logits, "logits")
    N, C = logits.shape[0], logits.shape[1]
    HW = logits.numel() // (N * C)
    acc = scores is not None
    if acc:
        if not scores.is_contiguous() or scores.shape != logits.shape or scores.dtype != torch.float32 or not scores.is_cuda:
            raise ValueError("scores must be a contiguous float32 device tensor of the logits' shape (updated in place)")
    else:
        scores = torch.empty_like(logits)
    _call("rfx_softmax_accum_f32", _one_device(logits, scores), _p(logits), _p(scores), N, C, HW, float(div), 1 if acc else 0)
    return scores


def argmax_mask(scores, class_id, complement=False, want_pred=False):
    """torch.max(scores, dim=1) -> float32 mask (N,H,W) = (pred == class_id) (``complement``: 1 - that) [, pred int32]
    (segNet/segEval.py:37-43)."""
    scores = _dev(scores, "scores")
    N, C, H, W = scores.shape
    mask = torch.empty((N, H, W), dtype=torch.float32, device=scores.device)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=scores.device) if want_pred else None
    _call("rfx_argmax_mask_f32", scores.device, _p(scores), N, C, H * W, int(class_id), 1 if complement else 0, _p(mask), _p(pred))
    return (mask, pred) if want_pred else mask


SEG_VOTE_MAX_SCALES = 8


def seg_vote(logits_list, out_hw, class_id, complement=False, want_pred=False, div=None):
    """resize_bilinear(align_corners=False) to ``out_hw`` -> softmax_accum(div) per logit map in list order -> argmax_mask, in one
    kernel and bit for bit that chain, without the (N, C, H, W) up-sampled logits and scores (segNet/segEval.py:27-43 after the network
    passes).  logits_list: 1..8 float32 (N, C, h_s, w_s) device tensors of one N and C; div defaults to their number.
    -> mask (N, H, W) float32 [, pred (N, H, W) int32]."""
    maps = [_dev(t, "logits[%d]" % i) for i, t in enumerate(logits_list)]
    S = len(maps)
    if not 1 <= S <= SEG_VOTE_MAX_SCALES:
        raise ValueError("seg_vote takes 1..%d logit maps, got %d" % (SEG_VOTE_MAX_SCALES, S))
    if any(t.dim() != 4 or t.shape[:2] != maps[0].shape[:2] for t in maps):
        raise ValueError("seg_vote: every logit map must be (N, C, h, w) with the same N and C")
    N, C = int(maps[0].shape[0]), int(maps[0].shape[1])
    H, W = int(out_hw[0]), int(out_hw[1])
    dev = _one_device(*maps)
    mask = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=dev) if want_pred else None
    ptrs = (ctypes.c_void_p * S)(*[t.data_ptr() for t in maps])
    hs = (ctypes.c_int32 * S)(*[int(t.shape[2]) for t in maps])
    ws = (ctypes.c_int32 * S)(*[int(t.shape[3]) for t in maps])
    launch_group.keep(maps)
    _call("rfx_seg_vote_f32", dev, ptrs, hs, ws, S, N, C, H, W, float(S if div is None else div), int(class_id),
          1 if complement else 0, _p(mask), _p(pred))
    return (mask, pred) if want_pred else mask


def sky_bytes(mask, k=0):
    """The byte image the scripts' ``imresize`` makes of a 0 / 1 sky mask (scipy 1.2.3 bytescale: 255 where non-zero if the map holds
    both values, a constant map -> zeros; per map), turned ``k`` quarter turns as np.rot90 (evaluation/evalYFCC/evaluation.py:193).
    mask (N, H, W) float32 -> (N, Ho, Wo, 1) uint8, the one-channel layout pil_resize_u8 reads."""
    mask = _dev(mask, "mask")
    if mask.dim() != 3:
        raise ValueError("sky_bytes expects (N, H, W) masks")
    k = int(k)
    if not 0 <= k <= 3:
        raise ValueError("k must be a number of quarter turns in 0..3")
    N, H, W = (int(v) for v in mask.shape)
    Ho, Wo = (W, H) if k & 1 else (H, W)
    out = torch.empty((N, Ho, Wo, 1), dtype=torch.uint8, device=mask.device)
    ws = torch.empty((max(1, _lib.load().rfx_sky_bytes_ws_bytes(N) // 4),), dtype=torch.int32, device=mask.device)
    _call("rfx_sky_bytes_u8", mask.device, _p(mask), N, H, W, k, _p(out), _p(ws))
    return out


def less_than_u8(img, threshold):
    """(img < threshold) as float32 1.0 / 0.0 for a uint8 device tensor, same shape."""
    img = _dev(img, "bytes", torch.uint8)
    out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
    _call("rfx_less_than_u8_f32", img.device, _p(img), img.numel(), int(threshold), _p(out))
    return out


def sky_background(mask, out_hw, k=0):
    """The scripts' ``(imresize(np.rot90(mask, k), (h, w)) < 128).astype(np.float32)`` (evaluation/evalYFCC/evaluation.py:193-200;
    k = 0: evalHpatch/evaluation.py:180, evalKITTI/evaluation.py:247-248) for a batch of 0 / 1 masks (N, H, W) on the device, bit for
    bit: byte form per map (sky_bytes), Pillow BILINEAR on the one-channel bytes (pil_resize_u8), threshold.  ``out_hw`` = (h, w) ->
    (N, h, w) float32, or a list of such sizes -> a list of maps made from ONE byte map."""
    many = len(out_hw) > 0 and hasattr(out_hw[0], "__len__")
    sizes = [tuple(int(v) for v in s) for s in (out_hw if many else [out_hw])]
    b = sky_bytes(mask, k)
    outs = [less_than_u8(pil_resize_u8(b, w, h, "bilinear"), 128)[..., 0] for (h, w) in sizes]
    return outs if many else outs[0]


def l2norm(x, out=None, out_batch_stride=0, out_chan_stride=0):
    """F.normalize(x, dim=1) for (N,C,H,W) or (N,C,L).  With ``out`` (a float32 device tensor/view start) the
    result is scattered with the given strides (elements)."""
    x = _dev(x, "l2norm input")
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // (N * C)
    if out is None:
        out = torch.empty_like(x)
        obs = ocs = 0
    else:
        if not out.is_cuda or out.dtype != torch.float32:
            raise TypeError("l2norm out must be a float32 device tensor")
        obs, ocs = out_batch_stride, out_chan_stride
    _call("rfx_l2norm_nchw_f32", _one_device(x, out), _p(x), _p(out), N, C, HW, obs, ocs)
    return out



def l2norm_scatter(x, out, dst_off, out_chan_stride):
    """F.normalize(x, dim=1) of the N images of one shape bucket x (N,C,H,W), image n written to ``out`` at element offset
    dst_off[n] with channel stride ``out_chan_stride`` (e.g. its pair's columns of a padded (B,C,ld) match matrix).  Sums bit-equal to
    l2norm.  dst_off: (N,) int64 device tensor."""
    x = _dev(x, "l2norm input")
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
        raise TypeError("l2norm_scatter out must be a float32 device tensor")
    dst_off = _dev(dst_off, "dst_off", torch.int64)
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // (N * C)
    if dst_off.numel() != N:
        raise ValueError("dst_off must hold one offset per image")
    _call("rfx_l2norm_nchw_scatter_f32", _one_device(x, out, dst_off), _p(x), _p(out), N, C, HW, _p(dst_off), int(out_chan_stride))
    return out

def flow_head(logits, K=7, out=None):
    logits = _dev(logits, "flow logits")
    N, C, R, Cc = logits.shape
    if C != K * K:
        raise ValueError("flow head expects %d logits, got %d" % (K * K, C))
    out = _out_or_new(out, (N, 2, R, Cc), logits, "flow_head")
    _call("rfx_flow_head_f32", logits.device, _p(logits), _p(out), N, K, R, Cc)
    return out


def resize_bilinear(x, size, align_corners=False, out=None):
    x = _dev(x, "resize input")
    N, C, H, W = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    out = _out_or_new(out, (N, C, Ho, Wo), x, "resize_bilinear")
    _call("rfx_resize_bilinear_f32", x.device, _p(x), _p(out), N * C, H, W, Ho, Wo, 1 if align_corners else 0)
    return out


_LANCZOS_TABLES = BoundedCache(64)      # (sizes, device) -> coefficient tables, LRU-bounded: a stream of variable-size images must
                                        # not grow it for ever (a table set is a few KB)


def pil_resize_u8(img, out_w, out_h, resample="lanczos"):
    """PIL.Image.resize((out_w, out_h), LANCZOS | BILINEAR) for a uint8 (N,H,W,C) device tensor, C in 1..4 (every channel is resampled
    on its own, as Pillow does for L and RGB) -- bit-identical to Pillow: rfx_lanczos_pass_u8 is table-driven, only rfx/lanczos.py
    knows the filter.  Another C is refused (RfxError), another filter is a ValueError."""
    from . import lanczos
    img = _dev(img, "image", torch.uint8)
    N, H, W, C = img.shape
    p = lanczos.plan(W, H, out_w, out_h, resample)
    if p is None:
        return img.clone()
    # evicted tables stay alive for as long as a kernel that reads them is queued (stream-ordered allocator); a captured HIP graph
    # that baked their addresses in holds them by lease (trunk_pass.graphed).  The Lanczos key is the one it always was; every other
    # filter's carries its name.
    key = (W, H, out_w, out_h, str(img.device)) + (() if resample == "lanczos" else (resample,))
    tabs = _LANCZOS_TABLES.get(key, lambda: {k: torch.from_numpy(p[k]).to(img.device) for k in ("bounds_h", "kk_h", "bounds_v", "kk_v")})
    cur, curH = img, H
    if p["need_h"]:
        tmp = torch.empty((N, p["rows_h"], out_w, C), dtype=torch.uint8, device=img.device)
        _call("rfx_lanczos_pass_u8", img.device, _p(cur), _p(tmp), N, H, W, p["rows_h"], out_w, C, _p(tabs["bounds_h"]),
                                           _p(tabs["kk_h"]), p["ks_h"], 0, p["y_first"])
        cur, curH = tmp, p["rows_h"]
    if p["need_v"]:
        out = torch.empty((N, out_h, out_w, C), dtype=torch.uint8, device=img.device)
        _call("rfx_lanczos_pass_u8", img.device, _p(cur), _p(out), N, curH, out_w, out_h, out_w, C, _p(tabs["bounds_v"]),
                                           _p(tabs["kk_v"]), p["ks_v"], 1, 0)
        cur = out
    return cur


def lanczos_resize_u8(img, out_w, out_h):
    """PIL.Image.resize((out_w, out_h), LANCZOS): pil_resize_u8 with the filter of the image pyramid (3 channels on the product
    path)."""
    return pil_resize_u8(img, out_w, out_h, "lanczos")


def u8_to_f32(img, mean=None, std=None, want_raw=True):
    """ToTensor (/255) and, with mean/std, Normalize: uint8 (N,H,W,3) -> float32 (N,3,H,W) raw and/or normalised."""
    img = _dev(img, "image", torch.uint8)
    N, H, W, C = img.shape
    if C != 3:
        raise ValueError("u8_to_f32 expects 3 channels")
    raw = torch.empty((N, 3, H, W), dtype=torch.float32, device=img.device) if want_raw else None
    norm = torch.empty((N, 3, H, W), dtype=torch.float32, device=img.device) if mean is not None else None
    m = (ctypes.c_float * 3)(*mean) if mean is not None else None
    s = (ctypes.c_float * 3)(*std) if std is not None else None
    _call("rfx_u8_to_f32_chw", img.device, _p(img), _p(raw), _p(norm), N, H, W, m, s)
    return raw, norm


def copy_cols(src, w_dst):
    """(rows, w_src) -> (rows, w_dst): copy min(w_src, w_dst) columns per row, zero-fill the rest."""
    src = _dev(src, "matrix")
    rows, ws = src.shape
    dst = torch.empty((rows, int(w_dst)), dtype=torch.float32, device=src.device)
    _call("rfx_copy_cols_f32", src.device, _p(src), _p(dst), rows, ws, int(w_dst))
    return dst


def corr_neigh(x, y, K=7, variant=None):
    """``variant``: force a tile shape of rfx_corr_neigh_variant_f32 (tuning / tests); default = RFX_CORR_VARIANT or
    the library's automatic choice.  All variants are bit-identical."""
    x, y = _dev(x, "corr x"), _dev(y, "corr y")
    if x.shape != y.shape:
        raise ValueError("corr_neigh: x %s and y %s differ" % (tuple(x.shape), tuple(y.shape)))
    N, C, H, W = x.shape
    if W % 4 != 0 and variant is None and os.environ.get("RFX_CORR_PAD", "1") == "1":
        if launch_group.recording():
            raise RuntimeError("corr_neigh inside a launch_group with W %% 4 != 0 (W = %d): the crop would read a launch that has not "
                               "run yet -- use ops.corr_neigh_group, which pads before the group and crops after it" % W)
        return _corr_group([x], [y], False, None, False, K)[0]
    out = torch.empty((N, K * K, H, W), dtype=torch.float32, device=x.device)
    e0 = Profiler.begin(x)
    v = int(os.environ.get("RFX_CORR_VARIANT", "0")) if variant is None else int(variant)
    _call("rfx_corr_neigh_variant_f32", _one_device(x, y), _p(x), _p(y), _p(out), N, C, H, W, K, v)
    if e0 is not None:
        Profiler.active().corr.append(((2 * C + K * K) * 4.0 * N * H * W, e0, Profiler.end(e0)))  # algorithmic bytes
        Profiler.active()._corr_order.append("one")
    return out


def corr_neigh_bidir(x, y, K=7, out=None):
    """Both directions of a pair in ONE launch: returns (corr_neigh(x, y), corr_neigh(y, x)), each (N,49,H,W).  The reverse
    volume is the forward one at mirrored taps and shifted pixels -- corr(y,x)[(6-i)*7+(6-j), r+i-3, c+j-3] =
    corr(x,y)[i*7+j, r, c], the same channel-ordered sums -- so it costs a second store, not a second 2*C*H*W read
    (evaluation/evalHpatch/evaluation.py:29-35 computes both).  ``out``: optional (2N,49,H,W) buffer; the two results are
    its halves (what the matchability head consumes as one batch)."""
    x, y = _dev(x, "corr x"), _dev(y, "corr y")
    if x.shape != y.shape:
        raise ValueError("corr_neigh_bidir: x %s and y %s differ" % (tuple(x.shape), tuple(y.shape)))
    N, C, H, W = x.shape
    if W % 4 != 0:
        if launch_group.recording():
            raise RuntimeError("corr_neigh_bidir inside a launch_group with W %% 4 != 0 (W = %d): the crop would read a launch that "
                               "has not run yet -- use ops.corr_neigh_bidir_group, which pads before the group and crops after it" % W)
        return _corr_group([x], [y], True, [out], False, K)[0]
    if out is None:
        out = torch.empty((2 * N, K * K, H, W), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (2 * N, K * K, H, W) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("corr_neigh_bidir: out must be a contiguous float32 (2N,49,H,W) tensor")
    e0 = Profiler.begin(x)
    _call("rfx_corr_neigh_bidir_f32", _one_device(x, y, out), _p(x), _p(y), _p(out[:N]), _p(out[N:]), N, C, H, W, K)
    if e0 is not None:
        Profiler.active().corr_bidir.append(((2 * C + 2 * K * K) * 4.0 * N * H * W, 2 * (2 * C + K * K) * 4.0 * N * H * W, e0,
                                             Profiler.end(e0)))
        Profiler.active()._corr_order.append("bidir")
    return out[:N], out[N:]


def _corr_group(xs, ys, bidir, outs, side_streams, K=7):
    """The one pad-and-crop implementation of the correlation ops.  The LDS-DMA kernels move 16-byte quads: widths that are no
    multiple of 4 run on copies zero-padded with copy_cols BEFORE the launch step (one stage: one problem launches eagerly, several
    are recorded in one group) and the results are cropped AFTER it -- the window's own padding is zero (model/model.py:135,143),
    so the result is the unpadded one, bit for bit.  The one-direction form pads under RFX_CORR_PAD (default), like corr_neigh."""
    if launch_group.recording():
        raise RuntimeError("corr_neigh(_bidir)_group opens its own launch_group: call it outside one")
    if len(xs) != len(ys) or not xs:
        raise ValueError("corr group: one y per x, at least one problem")
    pad = bidir or os.environ.get("RFX_CORR_PAD", "1") == "1"
    work = []
    for i, (x, y) in enumerate(zip(xs, ys)):
        x, y = _dev(x, "corr x"), _dev(y, "corr y")
        if x.shape != y.shape:
            raise ValueError("corr group: x %s and y %s differ" % (tuple(x.shape), tuple(y.shape)))
        N, C, H, W = x.shape
        Wp = (W + 3) // 4 * 4 if pad else W
        out = outs[i] if bidir and outs is not None else None
        if Wp != W:
            x, y, out = copy_cols(x.view(-1, W), Wp).view(N, C, H, Wp), copy_cols(y.view(-1, W), Wp).view(N, C, H, Wp), None
        work.append((x, y, out))

    def run(x, y, out):
        if not bidir:
            return corr_neigh(x, y, K)
        if out is None:
            out = torch.empty((2 * x.shape[0], K * K, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
        corr_neigh_bidir(x, y, K, out=out)
        return out
    res = stage(run, *zip(*work), device=_one_device(*xs, *ys), side_streams=side_streams)
    final = []
    for i, (x, r) in enumerate(zip(xs, res)):
        N, W = x.shape[0], x.shape[3]
        if r.shape[3] != W:
            r = copy_cols(r.view(-1, r.shape[3]), W).view(r.shape[0], K * K, r.shape[2], W)
            if bidir and outs is not None and outs[i] is not None:
                outs[i].copy_(r)
                r = outs[i]
        final.append((r[:N], r[N:]) if bidir else r)
    return final


def corr_neigh_group(xs, ys, side_streams=False):
    """[corr_neigh(x, y) for x, y in zip(xs, ys)] as ONE stage: every problem keeps the tile variant it gets alone (problems of
    different variants are different launches), bit-identical to the single calls."""
    return _corr_group(xs, ys, False, None, side_streams)


def corr_neigh_bidir_group(xs, ys, outs=None, side_streams=False):
    """[corr_neigh_bidir(x, y, out=o) for ...] as ONE stage (see corr_neigh_group).  ``outs``: optional list of (2N,49,H,W)
    buffers (entries may be None)."""
    return _corr_group(xs, ys, True, outs, side_streams)


def warp_grid(Hm, h, w):
    Hm = _dev(Hm, "homography")
    B = Hm.shape[0]
    grid = torch.empty((B, h, w, 2), dtype=torch.float32, device=Hm.device)
    _call("rfx_warp_grid_f32", Hm.device, _p(Hm), _p(grid), B, h, w)
    return grid


def grid_sample(inp, grid, align_corners=False):
    inp, grid = _dev(inp, "grid_sample input"), _dev(grid, "grid")
    N, C, Hi, Wi = inp.shape
    if grid.shape[0] != N or grid.shape[3] != 2:
        raise ValueError("grid must be (N,Ho,Wo,2)")
    Ho, Wo = grid.shape[1], grid.shape[2]
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=inp.device)
    _call("rfx_grid_sample_f32", _one_device(inp, grid), _p(inp), _p(grid), _p(out), N, C, Hi, Wi, Ho, Wo,
                                              1 if align_corners else 0)
    return out


def compose_flow(flowDown, coarseGrid, clamp=False, want_inb=False, want_flow_up=False, out_hw=None, inb_out=None):
    """flow12 = grid_sample(coarseGrid, [clamp](upsample(flowDown) + identity grid)).  ``out_hw``: output resolution when
    it differs from the coarse grid's (KITTI full-resolution pass); default = the coarse grid's.  ``inb_out``: where the in-bounds
    mask (N,H,W) goes (a view of a packed buffer) instead of a new tensor."""
    flowDown, coarseGrid = _dev(flowDown, "flowDown"), _dev(coarseGrid, "coarse grid")
    N, two, hd, wd = flowDown.shape
    _, Hc, Wc, _ = coarseGrid.shape
    H, W = (Hc, Wc) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    flow12 = torch.empty((N, H, W, 2), dtype=torch.float32, device=flowDown.device)
    inb = _out_or_new(inb_out, (N, H, W), flowDown, "compose_flow inb") if want_inb else None
    fup = torch.empty((N, H, W, 2), dtype=torch.float32, device=flowDown.device) if want_flow_up else None
    _call("rfx_compose_flow_f32", _one_device(flowDown, coarseGrid), _p(flowDown), _p(coarseGrid), _p(flow12), _p(inb), _p(fup),
          N, hd, wd, Hc, Wc, H, W, 1 if clamp else 0)
    return flow12, inb, fup


def flow_grad_clamp(flowCoarse, grid, want_grad=True):
    """model.predFlowCoarse's tail (model/model.py:333-340): -> (flowGrad (B,1,H-1,W-1) or None, clamp(flow^T + grid, -1, 1))."""
    f = _dev(flowCoarse, "flowCoarse")
    g = _dev(grid, "grid")
    B, C, H, W = f.shape
    if C != 2 or g.dim() != 4 or tuple(g.shape[1:]) != (H, W, 2) or g.shape[0] not in (1, B):
        raise ValueError("flowCoarse (B,2,H,W) / grid (1|B,H,W,2) expected, got %s / %s" % (tuple(f.shape), tuple(g.shape)))
    flow = torch.empty((B, H, W, 2), dtype=torch.float32, device=f.device)
    fg = torch.empty((B, 1, H - 1, W - 1), dtype=torch.float32, device=f.device) if want_grad else None
    _call("rfx_flow_grad_clamp_f32", _one_device(f, g), _p(f), _p(g), _p(fg), _p(flow), B, H, W, int(g.shape[0]))
    return fg, flow


def _match_plane(match12, n, H, W):
    if not isinstance(match12, torch.Tensor) or not match12.is_cuda or match12.dtype != torch.float32:
        raise RuntimeError("match12 must be a float32 tensor on a HIP device (no CPU fallback)")
    if tuple(match12.shape) != (n, H, W) or match12.stride(2) != 1 or match12.stride(1) != W:
        raise ValueError("match12 must be (n,H,W) with contiguous planes")
    return match12.stride(0) if n > 1 else H * W


def match_score(match12, cyc=None, inb=None):
    """match12 (n,H,W) (channel slice allowed) * cyc * inb -> (n,H,W)."""
    n, H, W = match12.shape
    stride = _match_plane(match12, n, H, W)
    c = _dev(cyc, "cyc") if cyc is not None else None
    b = _dev(inb, "inb") if inb is not None else None
    out = torch.empty((n, H, W), dtype=torch.float32, device=match12.device)
    _call("rfx_match_score_f32", _one_device(match12, c, b), match12.data_ptr(), stride, _p(c), _p(b), n, H * W, _p(out))
    return out


def _down8_planes(m, B, hd, wd, name):
    """A /8 matchability map (B,1,hd,wd) with contiguous planes (a batch slice of a larger tensor allowed) -> its batch stride."""
    if not isinstance(m, torch.Tensor) or not m.is_cuda or m.dtype != torch.float32:
        raise RuntimeError("%s must be a float32 tensor on a HIP device (no CPU fallback)" % name)
    if tuple(m.shape) != (B, 1, hd, wd) or (hd * wd > 1 and (m.stride(3) != 1 or m.stride(2) != wd)) or \
            (B > 1 and m.stride(0) < hd * wd):
        raise ValueError("%s must be (%d,1,%d,%d) with contiguous planes, got %s" % (name, B, hd, wd, tuple(m.shape)))
    return m.stride(0) if B > 1 else hd * wd


def cycle_tail(flowDown8, match12Down8, match21Down8, coarseGrid, out_hw=None, flow12_out=None, match_out=None):
    """The tail of the cycle-checked PredFlowMask forms in one kernel (rfx_cycle_tail_f32): bit for bit what
    resize_bilinear(both matchability maps) -> compose_flow(clamp=True, want_inb, want_flow_up, out_hw) -> grid_sample(up-sampled
    match21, flowUp) -> match_score give, without their full-resolution intermediates.  flowDown8 (B,2,hd,wd); match12Down8 /
    match21Down8 (B,1,hd,wd), e.g. the two halves of one (2B,1,hd,wd) tensor; coarseGrid (B,Hc,Wc,2); ``out_hw``: the output size when
    it is not the coarse grid's (KITTI full-resolution pass).  ``flow12_out`` (B,H,W,2) / ``match_out`` (B,H,W): where the results go
    (views of packed buffers) instead of new tensors; they may not alias an input.  -> (flow12 (B,H,W,2), match (B,H,W))."""
    flowDown8, coarseGrid = _dev(flowDown8, "flowDown8"), _dev(coarseGrid, "coarse grid")
    if flowDown8.dim() != 4 or flowDown8.shape[1] != 2:
        raise ValueError("flowDown8 must be (B,2,hd,wd), got %s" % (tuple(flowDown8.shape),))
    B, _, hd, wd = flowDown8.shape
    if coarseGrid.dim() != 4 or coarseGrid.shape[0] != B or coarseGrid.shape[3] != 2:
        raise ValueError("coarse grid must be (%d,Hc,Wc,2), got %s" % (B, tuple(coarseGrid.shape)))
    s12 = _down8_planes(match12Down8, B, hd, wd, "match12Down8")
    s21 = _down8_planes(match21Down8, B, hd, wd, "match21Down8")
    Hc, Wc = coarseGrid.shape[1], coarseGrid.shape[2]
    H, W = (Hc, Wc) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    flow12 = _out_or_new(flow12_out, (B, H, W, 2), flowDown8, "cycle_tail flow12")
    match = _out_or_new(match_out, (B, H, W), flowDown8, "cycle_tail match")
    if flow12.data_ptr() % 8 or coarseGrid.data_ptr() % 8:
        raise ValueError("cycle_tail: flow12 and the coarse grid are accessed as float2 and must be 8-byte aligned")
    _call("rfx_cycle_tail_f32", _one_device(flowDown8, match12Down8, match21Down8, coarseGrid), _p(flowDown8), _p(match12Down8), s12,
          _p(match21Down8), s21, _p(coarseGrid), _p(flow12), _p(match), B, hd, wd, Hc, Wc, H, W)
    return flow12, match


def merge_multi_h(flow, match12, th, multiH, cyc=None, inb=None):
    """flow (n,H,W,2); match12 (n,H,W) -- may be a channel slice of an (n,C,H,W) tensor (batch stride honoured);
    cyc / inb (n,H,W) contiguous or None  ->  flowGlobal (1,H,W,2), matchGlobal (1,H,W), binary (1,H,W) bool."""
    flow = _dev(flow, "flow")
    n, H, W, _ = flow.shape
    HW = H * W
    stride = _match_plane(match12, n, H, W)
    c = _dev(cyc, "cyc") if cyc is not None else None
    b = _dev(inb, "inb") if inb is not None else None
    fg = torch.empty((1, H, W, 2), dtype=torch.float32, device=flow.device)
    mg = torch.empty((1, H, W), dtype=torch.float32, device=flow.device)
    binary = torch.empty((1, H, W), dtype=torch.uint8, device=flow.device)
    _call("rfx_merge_multi_h_f32", _one_device(flow, match12, c, b), _p(flow), match12.data_ptr(), stride, _p(c),
                                                _p(b), n, HW, float(th), 1 if multiH else 0, _p(fg), _p(mg),
                                                _p(binary))
    return fg, mg, binary.bool()


def cc_max_area(size, cc_th):
    """Largest pixel count a with ``a / float(size) <= cc_th`` in float64 -- the reference's test
    (``np.mean(lab == i) <= cc_th`` / ``area <= cc_th`` on area fractions, evalKITTI/evaluation.py:96) as an integer bound."""
    a = int(cc_th * size)
    while (a + 1) / float(size) <= cc_th:
        a += 1
    while a > 0 and a / float(size) > cc_th:
        a -= 1
    return a


def remove_small_cc(match, cc_th, match_th=0.99):
    """evaluation/evalKITTI/evaluation.py:85-100 / getResults.py:66-84 on the device: zero every 8-connected component of
    (match > match_th) whose area fraction is <= cc_th.  match (N,H,W) or (H,W) float32; returns a new tensor."""
    m = _dev(match, "match map")
    if cc_th == 0:
        return m
    squeeze = m.dim() == 2
    m3 = (m[None] if squeeze else m).contiguous()
    N, H, W = m3.shape
    lib = _lib.load()
    ws = torch.empty(lib.rfx_remove_small_cc_ws_bytes(N, H, W), dtype=torch.uint8, device=m3.device)
    out = torch.empty_like(m3)
    _call("rfx_remove_small_cc_f32", _one_device(m3), _p(m3), _p(out), N, H, W, float(match_th), cc_max_area(H * W, float(cc_th)),
          _p(ws))
    return out[0] if squeeze else out


def cc_dims_table(hw_list, cc_th):
    """Rows (h, w, max_area) of rfx_remove_small_cc_ragged_f32's table for maps of the sizes ``hw_list``: max_area is each map's own
    cc_max_area(h * w, cc_th)."""
    return [(int(h), int(w), cc_max_area(int(h) * int(w), float(cc_th))) for h, w in hw_list]


def remove_small_cc_ragged(match, match_off, hw, cc_th, match_th=0.99, inplace=False, max_hw=None):
    """remove_small_cc for maps of DIFFERENT sizes in one launch chain (rfx_remove_small_cc_ragged_f32): ``match`` is a packed 1-D
    float32 buffer, map k's h_k * w_k values at element ``match_off[k]`` ((n,) int64 device tensor) -- the layout
    multih_accept_ragged consumes.  ``hw``: a list of n (h, w) (the table is built with cc_dims_table and uploaded here), or the
    (n,3) int32 device table itself (rows h, w, max_area; then ``max_hw`` = the largest h * w is required and ``cc_th`` only
    decides whether anything runs).  Each map's area bound comes from its OWN size; map k's result equals remove_small_cc on that
    map alone bit for bit.  Returns a new packed buffer, or ``match`` itself filtered in place (``inplace=True``).  cc_th == 0: the
    identity."""
    m = _dev(match, "match buffer")
    if m.dim() != 1:
        raise ValueError("match of a ragged round is a packed 1-D buffer")
    if inplace and m is not match:
        raise ValueError("match must be a contiguous float32 device tensor (filtered in place)")
    if cc_th == 0:
        return m
    off = _dev(match_off, "match_off", torch.int64)
    n = off.numel()
    if isinstance(hw, torch.Tensor):
        dims = _dev(hw, "dims", torch.int32)
        if max_hw is None:
            raise ValueError("a device table needs max_hw = the largest h * w of its maps")
    else:
        rows = cc_dims_table(hw, cc_th)
        dims = torch.tensor(rows, dtype=torch.int32).to(m.device)
        max_hw = max(h * w for h, w, _ in rows)
    if dims.shape != (n, 3):
        raise ValueError("one (h, w[, max_area]) per offset expected")
    total = m.numel()
    lib = _lib.load()
    ws = torch.empty(lib.rfx_remove_small_cc_ragged_ws_bytes(total), dtype=torch.uint8, device=m.device)
    out = m if inplace else torch.empty_like(m)
    if not inplace:
        out.copy_(m)                  # elements of the buffer that belong to no map pass through
    _call("rfx_remove_small_cc_ragged_f32", _one_device(m, off, dims), _p(m), _p(out), _p(off), _p(dims), n, total, int(max_hw),
          float(match_th), _p(ws))
    return out


def nearest_fill(values, explained, want_index=False):
    """evaluation/evalKITTI/getResults.py:87-93 on the device (rfx_nearest_fill_f32): every pixel takes the values of its nearest
    explained pixel -- scipy.ndimage.distance_transform_edt(~explained, return_indices=True) index for index, ties included (the
    smallest column, then the smallest row; a map without explained pixel reads pixel (H-1, 0)).  values (N,H,W,C) or (H,W,C)
    float32, C <= 8; explained (N,H,W) or (H,W) bool.  Returns a new tensor, with want_index also scipy's indices (N,2,H,W) int32
    ((2,H,W) for a single map)."""
    v = _dev(values, "values")
    e = _dev(explained, "explained", torch.bool)
    squeeze = v.dim() == 3
    if v.dim() not in (3, 4) or e.dim() != v.dim() - 1 or tuple(e.shape) != tuple(v.shape[:-1]):
        raise RuntimeError("nearest_fill: values (N,H,W,C) / (H,W,C) with explained (N,H,W) / (H,W) expected, got %s and %s"
                           % (tuple(v.shape), tuple(e.shape)))
    v4, e3 = (v[None], e[None]) if squeeze else (v, e)
    N, H, W, C = v4.shape
    out = torch.empty_like(v4)
    idx = torch.empty((N, 2, H, W), dtype=torch.int32, device=v4.device) if want_index else None
    ws = torch.empty(_lib.load().rfx_nearest_fill_ws_bytes(N, H, W), dtype=torch.uint8, device=v4.device)
    _call("rfx_nearest_fill_f32", _one_device(v4, e3), _p(v4), _p(e3), _p(out), _p(idx), N, H, W, C, _p(ws))
    if squeeze:
        out, idx = out[0], (idx[0] if want_index else None)
    return (out, idx) if want_index else out


def _points_geometry(flow, keep, sizeA, sizeB, angle, bg):
    """Shapes of a flow_points call, checked before anything touches a device -> (single map?, k, (wA, hA), (wB, hB))."""
    for name, t in (("flow", flow), ("keep", keep), ("bg", bg)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    (wA, hA), (wB, hB) = (int(sizeA[0]), int(sizeA[1])), (int(sizeB[0]), int(sizeB[1]))
    k = (int(angle) // 90) % 4
    single = flow.dim() == 3
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2 or tuple(keep.shape) != tuple(flow.shape[:-1]):
        raise ValueError("flow_points: flow (N,H,W,2) / (H,W,2) with keep (N,H,W) / (H,W) expected, got %s and %s"
                         % (tuple(flow.shape), tuple(keep.shape)))
    if bg is not None and tuple(bg.shape) != tuple(keep.shape):
        raise ValueError("flow_points: bg %s is not of keep's shape %s" % (tuple(bg.shape), tuple(keep.shape)))
    want = (wB, hB) if k & 1 else (hB, wB)
    if tuple(flow.shape[-3:-1]) != want or min(want) < 1 or (not single and flow.shape[0] < 1):
        raise ValueError("flow_points: maps of shape %s do not fit sizeB = %s at angle %s (%s expected)"
                         % (tuple(flow.shape[-3:-1]), (wB, hB), angle, want))
    if wA < 1 or hA < 1:
        raise ValueError("flow_points: sizeA = %s" % ((wA, hA),))
    return single, k, (wA, hA), (wB, hB)


def _mask_bytes(t, name):
    """A bool or uint8 mask on a HIP device (non-zero = set), contiguous."""
    return _dev(t, name, torch.uint8 if t.dtype == torch.uint8 else torch.bool)


def flow_points(flow, keep, sizeA, sizeB, angle=0, bg=None):
    """evaluation/evalYFCC/getResults.py:53-71 (matches_from_flow) on the device (rfx_flow_points_f32): the correspondences of all
    pixels with keep (and bg, if given) set, map after map, row-major inside a map -- numpy's boolean indexing of the flow and of
    np.rot90(gridB, angle // 90).  flow (N,H,W,2) / (H,W,2) float32, keep and bg (N,H,W) / (H,W) bool or uint8; sizeA = (wA, hA),
    sizeB = (wB, hB) the unrotated target size.  No host sync: returns (pts1_buf (N*H*W,2) float32, pts2_buf (N*H*W,2) int64,
    offsets (N+1,) int64), all on the device; only the first offsets[-1] rows of the buffers are written, map n's rows are
    offsets[n]:offsets[n+1]."""
    single, k, (wA, hA), (wB, hB) = _points_geometry(flow, keep, sizeA, sizeB, angle, bg)
    f, m = _dev(flow, "flow"), _mask_bytes(keep, "keep")
    b = _mask_bytes(bg, "bg") if bg is not None else None
    N, (H, W) = (1 if single else f.shape[0]), f.shape[-3:-1]
    lib = _lib.load()
    pts1 = torch.empty((N * H * W, 2), dtype=torch.float32, device=f.device)
    pts2 = torch.empty((N * H * W, 2), dtype=torch.int64, device=f.device)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=f.device)
    ws = torch.empty(lib.rfx_flow_points_ws_bytes(N, H, W), dtype=torch.uint8, device=f.device)
    _call("rfx_flow_points_f32", _one_device(f, m, b), _p(f), _p(m), _p(b), N, H, W, k, wA, hA, wB, hB, _p(pts1), _p(pts2),
          _p(offsets), _p(ws))
    return pts1, pts2, offsets


def matches_from_flow(flow, keep, sizeA, sizeB, angle=0, bg=None):
    """flow_points, exactly sized: ONE read of the offsets (the only host sync), then views of the first offsets[-1] rows.
    A single (H,W,2) map -> (pts1 (n,2) float32, pts2 (n,2) int64); a batch (N,H,W,2) -> (pts1, pts2, offsets) with offsets the
    (N+1,) int64 HOST copy just read: map n's points are rows offsets[n]:offsets[n+1].  The results are views of flow_points'
    N*H*W-row buffers (no copy); ``.clone()`` them to let the buffers go."""
    pts1, pts2, offsets = flow_points(flow, keep, sizeA, sizeB, angle, bg)
    off = offsets.cpu()
    total = int(off[-1])
    if flow.dim() == 3:
        return pts1[:total], pts2[:total]
    return pts1[:total], pts2[:total], off


POINTS_TILE = 1024             # pixels of one workgroup's tile (csrc/points_tile.h)


def flow_points_ragged_table(sizes, sizesA, angles):
    """The table of rfx_flow_points_ragged_f32 for B maps of different sizes, on the host: a pure function of ``sizes[b]`` = (H, W) of
    map b as it lies in the packed buffers, ``sizesA[b]`` = (wA, hA) of its source and ``angles[b]`` (a multiple of 90 degrees; one
    int = the same for all).  -> (rows, total_px, total_tiles): row b = (pixel offset | H | W | k | wA | hA | index of the map's first
    tile | 0) with k = (angle // 90) % 4; a map has ceil(H * W / 1024) tiles.  The unrotated target size follows from (H, W, k):
    (wB, hB) = (W, H) for even k, (H, W) for odd k."""
    B = len(sizes)
    angles = [angles] * B if isinstance(angles, int) else list(angles)
    if B == 0 or len(sizesA) != B or len(angles) != B:
        raise ValueError("flow_points_ragged: one (H, W), one (wA, hA) and one angle per map, got %d, %d and %d"
                         % (B, len(sizesA), len(angles)))
    rows, off, tile = [], 0, 0
    for (H, W), (wA, hA), a in zip(sizes, sizesA, angles):
        H, W, wA, hA = int(H), int(W), int(wA), int(hA)
        if int(a) != a or int(a) % 90:
            raise ValueError("flow_points_ragged: angles are multiples of 90 degrees, got %r" % (a,))
        if H < 1 or W < 1:
            raise ValueError("flow_points_ragged: a map of shape %s" % ((H, W),))
        if wA < 1 or hA < 1:
            raise ValueError("flow_points_ragged: sizeA = %s" % ((wA, hA),))
        rows.append((off, H, W, int(a) // 90 % 4, wA, hA, tile, 0))
        off += H * W
        tile += (H * W + POINTS_TILE - 1) // POINTS_TILE
    return rows, off, tile


def _packed_maps(x, name):
    """A packed buffer from ``x`` (shapes checked by the caller): a tensor as it is; a list of one map per pair taken as ONE view
    where the maps already lie one behind the other in one buffer (what assemble_records returns), concatenated otherwise."""
    if isinstance(x, torch.Tensor):
        return x
    parts, trailing = list(x), tuple(x[0].shape[2:])
    total = sum(t.shape[0] * t.shape[1] for t in parts)
    if any(not t.is_cuda for t in parts):
        raise RuntimeError("%s is on %s: rfx ops run only on a HIP device (no CPU fallback)" % (name, parts[0].device))
    if any(t.dtype != parts[0].dtype for t in parts):
        raise TypeError("flow_points_ragged: the maps of %s differ in dtype" % name)
    first, size = parts[0], parts[0].element_size()
    ptr, consecutive = first.data_ptr(), True
    for t in parts:
        consecutive = consecutive and t.is_contiguous() and t.data_ptr() == ptr and \
            t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
        ptr += t.numel() * size
    if consecutive:
        return first.new_empty(0).set_(first.untyped_storage(), first.storage_offset(), (total,) + trailing)
    return torch.cat([t.reshape((-1,) + trailing) for t in parts])


def flow_points_ragged(flow, keep, sizes, sizesA, angles, bg=None):
    """flow_points for B maps of DIFFERENT sizes, each with its own angle and source size, in one chain (rfx_flow_points_ragged_f32:
    three launches for the whole batch): evaluation/evalYFCC/getResults.py:53-71 as the script calls it per pair (:318).
    ``sizes[b]`` = (H, W) of map b, ``sizesA[b]`` = (wA, hA), ``angles[b]`` a multiple of 90 (or one int for all); the unrotated
    target size is (W, H) for even k = angle // 90, (H, W) for odd k.  flow / keep / bg (optional): the packed buffers of
    assemble_records on ragged records -- (total_px,2) float32, (total_px,) bool or uint8 -- or lists of per-pair maps (H_b,W_b,2) /
    (H_b,W_b), which are concatenated only when they are not already consecutive views of one buffer.  No host sync: returns
    (pts1_buf (total_px,2) float32, pts2_buf (total_px,2) int64, offsets (B+1,) int64), all on the device; pair b's rows are
    offsets[b]:offsets[b+1], a pair without a kept pixel has none, only the first offsets[-1] rows are written."""
    rows, total, tiles = flow_points_ragged_table(sizes, sizesA, angles)
    sizes = [(r[1], r[2]) for r in rows]
    for name, x, trailing in (("flow", flow, (2,)), ("keep", keep, ()), ("bg", bg, ())):     # every shape before any device
        shapes = [tuple(x.shape)] if isinstance(x, torch.Tensor) else None if x is None else [tuple(getattr(t, "shape", ())) for t in x]
        if shapes is not None and shapes != [(total,) + trailing] and shapes != [s + trailing for s in sizes]:
            raise ValueError("flow_points_ragged: %s is a packed %s buffer or one map per pair of the shapes %r, got %r"
                             % (name, (total,) + trailing, sizes, shapes))
    f = _dev(_packed_maps(flow, "flow"), "flow")
    m = _mask_bytes(_packed_maps(keep, "keep"), "keep")
    b = _mask_bytes(_packed_maps(bg, "bg"), "bg") if bg is not None else None
    B, dev = len(rows), f.device
    pts1 = torch.empty((total, 2), dtype=torch.float32, device=dev)
    pts2 = torch.empty((total, 2), dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.load().rfx_flow_points_ragged_ws_bytes(tiles), dtype=torch.uint8, device=dev)
    table = torch.tensor(rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    _call("rfx_flow_points_ragged_f32", _one_device(f, m, b), _p(f), _p(m), _p(b), _p(table), B, total, tiles, _p(pts1), _p(pts2),
          _p(offsets), _p(ws))
    return pts1, pts2, offsets


def matches_from_flow_ragged(flow, keep, sizes, sizesA, angles, bg=None):
    """flow_points_ragged, exactly sized: ONE read of the offsets (the only host sync of the batch), then views of the first
    offsets[-1] rows -> (pts1 (n,2) float32, pts2 (n,2) int64, offsets (B+1,) int64 HOST copy): pair b's points are rows
    offsets[b]:offsets[b+1].  Views of flow_points_ragged's buffers (no copy); ``.clone()`` them to let the buffers go."""
    pts1, pts2, offsets = flow_points_ragged(flow, keep, sizes, sizesA, angles, bg)
    off = offsets.cpu()
    total = int(off[-1])
    return pts1[:total], pts2[:total], off


def sample_points(flow, match, xb, yb, sizeA):
    """evaluation/evalCorr/getResults.py:15-31 (alignmentError's reads of the assembled maps) on the device (rfx_sample_points_f32):
    for K target pixels (xb, yb) -- host integers, or floats truncated toward zero like ``astype(np.int64)`` -- of ONE map,
    xa = ((flow[yb,xb,0] + 1) * 0.5) * (wA - 1), ya likewise with channel 1 and hA - 1, keep = match[yb,xb] > 0.5.  flow (H,W,2) or
    (1,H,W,2), match (H,W) with any number of size-1 axes around it, float32 on the device.  A pixel outside the map is a bad
    argument (RfxError), found on the host before anything is launched.  Returns device tensors (xa, ya float32, keep bool) of K."""
    import numpy as np
    f = _dev(flow, "flow")
    m = _dev(match, "match")
    if f.dim() == 4 and f.shape[0] == 1:
        f = f[0]
    if f.dim() != 3 or f.shape[2] != 2 or m.numel() != f.shape[0] * f.shape[1]:
        raise ValueError("sample_points: flow (H,W,2) with match (H,W) expected, got %s and %s" % (tuple(flow.shape), tuple(match.shape)))
    H, W = int(f.shape[0]), int(f.shape[1])
    wA, hA = int(sizeA[0]), int(sizeA[1])
    x = np.asarray(xb.cpu() if isinstance(xb, torch.Tensor) else xb).astype(np.int64).reshape(-1)
    y = np.asarray(yb.cpu() if isinstance(yb, torch.Tensor) else yb).astype(np.int64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError("sample_points: %d xb for %d yb" % (x.size, y.size))
    K = int(x.size)
    if wA < 1 or hA < 1 or (K and (x.min() < 0 or x.max() >= W or y.min() < 0 or y.max() >= H)):
        _lib.check(-1, "rfx_sample_points_f32 (a keypoint outside the %d x %d map, or sizeA = %s)" % (W, H, (wA, hA)))
    xa = torch.empty(K, dtype=torch.float32, device=f.device)
    ya = torch.empty(K, dtype=torch.float32, device=f.device)
    keep = torch.empty(K, dtype=torch.bool, device=f.device)
    if K:
        xy = torch.from_numpy(np.stack((x, y)).astype(np.int32)).to(f.device)
        _call("rfx_sample_points_f32", _one_device(f, m), _p(f), _p(m), _p(xy[0]), _p(xy[1]), K, H, W, wA, hA, _p(xa), _p(ya),
              _p(keep))
    return xa, ya, keep


def _epe_outputs(name, N, H, W, err_dtype, want_err, *operands):
    """The shared tail of the two end-point-error ops: outputs, workspace, the call."""
    dev = _one_device(*operands)
    total = torch.empty(N, dtype=torch.float64, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    err = torch.empty((N, H, W), dtype=err_dtype, device=dev) if want_err else None
    ws = torch.empty(_lib.load().rfx_epe_ws_bytes(N, H, W), dtype=torch.uint8, device=dev)
    _call(name, dev, *[_p(t) for t in operands], N, H, W, _p(total), _p(count), _p(err), _p(ws))
    return total, count, err


def epe_homography(flow, Hinv, want_err=False):
    """evaluation/evalHpatch/getResults.py:83-156,221-250 on the device (rfx_epe_homography_f32): the end-point error of an estimated
    correspondence map against the map ONE inverse ground-truth homography defines, over the pixels that homography keeps inside
    [-1,1]^2.  flow (N,Sh,Sw,2) float32 with Hinv (N,3,3) or (N,9) float64, or a single map (Sh,Sw,2) with Hinv (3,3) or (9,).  No
    host sync: returns device tensors (sum (N,) float64, count (N,) int32[, err (N,Sh,Sw) float32, NaN outside]) -- 0-dim and (Sh,Sw)
    for a single map; the average is sum / count.  A map's sum has the same bits alone or anywhere in a batch."""
    for name, t in (("flow", flow), ("Hinv", Hinv)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    single = flow.dim() == 3
    n = 1 if single else (flow.shape[0] if flow.dim() == 4 else -1)
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2 or n < 1 or Hinv.numel() != 9 * n or \
            tuple(Hinv.shape) not in (((3, 3), (9,)) if single else ((n, 3, 3), (n, 9))):
        raise ValueError("epe_homography: flow (N,Sh,Sw,2) with Hinv (N,3,3) / (N,9), or (Sh,Sw,2) with (3,3) / (9,), expected, got "
                         "%s and %s" % (tuple(flow.shape), tuple(Hinv.shape)))
    Sh, Sw = int(flow.shape[-3]), int(flow.shape[-2])
    if Sh < 2 or Sw < 2:
        raise ValueError("epe_homography: maps of %d x %d pixels (the rule divides by size - 1)" % (Sh, Sw))
    f, h = _dev(flow, "flow"), _dev(Hinv, "Hinv", torch.float64)
    total, count, err = _epe_outputs("rfx_epe_homography_f32", n, Sh, Sw, torch.float32, want_err, f, h)
    if single:
        total, count, err = total[0], count[0], (err[0] if want_err else None)
    return (total, count, err) if want_err else (total, count)


def epe_flow(flow, u, v, valid, want_err=False):
    """evaluation/evalKITTI/getResults.py:221-228 on the device (rfx_epe_flow_f32): the flow minus the identity grid, scaled to
    pixels in float32 steps, its float64 distance to the ground truth (u, v) over the pixels with valid set.  flow (N,H,W,2) float32,
    u, v (N,H,W) float32, valid (N,H,W) bool or uint8 -- or single maps (H,W,2) / (H,W).  No host sync: returns device tensors
    (sum (N,) float64, count (N,) int32[, err (N,H,W) float64, NaN where not valid]) -- 0-dim and (H,W) for single maps."""
    for name, t in (("flow", flow), ("u", u), ("v", v), ("valid", valid)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    single = flow.dim() == 3
    maps = tuple(flow.shape[:-1])
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2 or min(maps) < 1 or any(tuple(t.shape) != maps for t in (u, v, valid)):
        raise ValueError("epe_flow: flow (N,H,W,2) / (H,W,2) with u, v, valid (N,H,W) / (H,W) expected, got %s, %s, %s and %s"
                         % tuple(tuple(t.shape) for t in (flow, u, v, valid)))
    f, uu, vv, m = _dev(flow, "flow"), _dev(u, "u"), _dev(v, "v"), _mask_bytes(valid, "valid")
    n, (H, W) = (1 if single else int(f.shape[0])), (int(x) for x in f.shape[-3:-1])
    total, count, err = _epe_outputs("rfx_epe_flow_f32", n, H, W, torch.float64, want_err, f, uu, vv, m)
    if single:
        total, count, err = total[0], count[0], (err[0] if want_err else None)
    return (total, count, err) if want_err else (total, count)


_HOST_KC = None


def host_sgemm_k_block(K=1024):
    """How the HOST's float32 matrix product -- torch.mm, the reference's score product (utils/outil.py:34) -- sums over k: MKL's
    sgemm accumulates an fma chain inside blocks of KC products and adds each block's sum to C; KC depends on the code path MKL
    picks for the CPU (192 on the GPU box's EPYC 9575F, 384 on a Xeon; MKL 2024.2; scripts/mm_blocking_probe.py).  Returns the
    KC whose float32 emulation reproduces torch.mm on a 384 x 256 post-ReLU, L2-normalised problem (MKL's small-matrix paths sum
    differently: the probe has to be large enough to take the blocked path the real 8 531 ... 25 747 x 1 200 ... 8 250 products
    take) bit for bit on all but <= 1e-4 of the elements (an edge kernel), or None when no candidate does -- another BLAS: the
    device then keeps its default chunking.  Pure host arithmetic, ~0.3 s per candidate, cached."""
    global _HOST_KC
    if _HOST_KC is not None:
        return _HOST_KC or None
    import numpy as np
    g = torch.Generator().manual_seed(7)
    A = torch.relu(torch.randn(K, 384, generator=g))
    B = torch.relu(torch.randn(K, 256, generator=g))
    A, B = A / A.norm(dim=0, keepdim=True), B / B.norm(dim=0, keepdim=True)
    mm = (A.t() @ B).numpy()
    a, b = A.numpy().astype(np.float64), B.numpy().astype(np.float64)
    found = 0
    for kc in (192, 384, 256, 128, 512, K):
        tot = np.zeros(mm.shape, np.float32)
        for k0 in range(0, K, kc):
            acc = np.zeros(mm.shape, np.float32)
            for k in range(k0, min(K, k0 + kc)):
                acc = (acc.astype(np.float64) + np.outer(a[k], b[k])).astype(np.float32)      # fma: exact product, one rounding
            tot = (tot.astype(np.float64) + acc).astype(np.float32)
        if float((tot != mm).mean()) <= 1e-4:
            found = kc
            break
    _HOST_KC = found
    return found or None


DEFAULT_SCORE_CHUNK = 256        # products per accumulation chunk of a mutual-NN score when nothing else is asked for


def resolve_score_chunk(spec=None):
    """The score chunk of ONE pipeline / drop-in module -> (products per chunk, where the value came from).  ``spec``:
      None      -> the environment variable RFX_SCORE_CHUNK if set (same grammar), else the fixed default of 256 products;
      an int    -> that many products per chunk (a positive multiple of 32); 0 = the library default of 256 (what 0 means in
                   rfx_api.h and ops.mutual_nn, one convention in every layer); < 0: ONE fma chain over all products (-1);
      "default" -> 256;
      "host"    -> the K blocking of THIS host's sgemm (host_sgemm_k_block: ~0.3-2 s of host arithmetic, cached per process), which
                   makes the device's scores equal the reference's torch.mm on this host bit for bit (the parity modes: drop-in
                   modules, parity sweeps, bench.py); 256 when no candidate reproduces the host's torch.mm (another BLAS).
    Called where a pipeline is CONSTRUCTED, never inside a launch: the value is an explicit argument of every
    rfx_mutual_nn*_f32 call (ABI 8) and travels with the results (AlignPipeline.score_chunk / .score_chunk_source)."""
    src = "argument"
    if spec is None:
        spec, src = os.environ.get("RFX_SCORE_CHUNK"), "RFX_SCORE_CHUNK"
        if spec is None or spec == "":
            return DEFAULT_SCORE_CHUNK, "default (fixed 256 products)"
    if isinstance(spec, str):
        if spec == "default":
            return DEFAULT_SCORE_CHUNK, "default (fixed 256 products)"
        if spec == "host":
            kc = host_sgemm_k_block()
            if kc and kc % 32 == 0:
                return int(kc), "host probe (host_sgemm_k_block: this host's torch.mm sums k in blocks of %d)" % kc
            return DEFAULT_SCORE_CHUNK, "fallback (no K blocking reproduced this host's torch.mm: fixed 256 products)"
        spec = int(spec)
    spec = int(spec)
    if spec == 0:
        return DEFAULT_SCORE_CHUNK, "%s = 0 (the library default: fixed 256 products)" % src
    if spec < 0:
        return -1, "%s (one chain)" % src
    if spec % 32:
        raise ValueError("score_chunk must be a multiple of 32 products, got %d" % spec)
    return spec, src


def mutual_nn(featA, featB, maskB=None, ldA=None, ldB=None, nA=None, nB=None, score_chunk=0):
    """featA (C,nA), featB (C,nB) -> (index1, index2) int64 device tensors (ascending index1).
    ``score_chunk``: products per accumulation chunk of a score (rfx_api.h; 0 = the library default of 256, < 0 = one chain).
    Synchronises once to read the match count (the reference's nonzero() does the same)."""
    featA, featB = _dev(featA, "featA"), _dev(featB, "featB")
    C = featA.shape[0]
    nA = nA or featA.shape[1]
    nB = nB or featB.shape[1]
    ldA = ldA or featA.stride(0)
    ldB = ldB or featB.stride(0)
    lib = _lib.load()
    ws = torch.empty(lib.rfx_mutual_nn_ws_bytes(nA, nB), dtype=torch.uint8, device=featA.device)
    cap = min(nA, nB)
    idx1 = torch.empty(cap, dtype=torch.int64, device=featA.device)
    idx2 = torch.empty(cap, dtype=torch.int64, device=featA.device)
    count = torch.zeros(1, dtype=torch.int32, device=featA.device)
    m = _dev(maskB, "maskB") if maskB is not None else None
    _call("rfx_mutual_nn_f32", _one_device(featA, featB, m), _p(featA), ldA, nA, _p(featB), ldB, nB, C, _p(m), _p(idx1), _p(idx2), _p(count),
                                     _p(ws), int(score_chunk))
    n = int(count.item())
    return idx1[:n], idx2[:n]



def mutual_nn_ragged(featA, featB, nA, nB, maxNA=None, maxNB=None, maskB=None, score_chunk=0, cap=None):
    """featA (B,C,ldA), featB (B,C,ldB) on a common padded layout, nA / nB (B,) int32 device tensors (pair b's own sizes) ->
    idx1, idx2 (B,cap) int64, count (B,) int32.  ``maxNA`` / ``maxNB``: host maxima of nA / nB (they size the grid; default ldA /
    ldB); ``cap``: max_b min(nA[b], nB[b]) (default min(maxNA, maxNB)); maskB (B,ldB) or None.  Pair b's indices and count equal mutual_nn on its own
    features bit for bit.  No host sync."""
    featA, featB = _dev(featA, "featA"), _dev(featB, "featB")
    nA, nB = _dev(nA, "nA", torch.int32), _dev(nB, "nB", torch.int32)
    if featA.dim() != 3 or featB.dim() != 3 or featA.shape[:2] != featB.shape[:2]:
        raise ValueError("featA / featB must be (B,C,ldA) / (B,C,ldB)")
    B, C, ldA = featA.shape
    ldB = featB.shape[2]
    if nA.numel() != B or nB.numel() != B:
        raise ValueError("nA / nB must hold one size per pair")
    maxNA = int(maxNA or ldA)
    maxNB = int(maxNB or ldB)
    m = _dev(maskB, "maskB") if maskB is not None else None
    if m is not None and tuple(m.shape) != (B, ldB):
        raise ValueError("maskB must be (B, ldB)")
    lib = _lib.load()
    ws = torch.empty(B * lib.rfx_mutual_nn_ws_bytes(maxNA, maxNB), dtype=torch.uint8, device=featA.device)
    cap = int(cap or min(maxNA, maxNB))
    idx1 = torch.empty((B, cap), dtype=torch.int64, device=featA.device)
    idx2 = torch.empty((B, cap), dtype=torch.int64, device=featA.device)
    count = torch.zeros(B, dtype=torch.int32, device=featA.device)
    _call("rfx_mutual_nn_ragged_f32", _one_device(featA, featB, nA, nB, m), _p(featA), ldA, _p(featB), ldB, _p(nA), _p(nB), maxNA,
          maxNB, C, _p(m), _p(idx1), _p(idx2), cap, _p(count), _p(ws), B, int(score_chunk))
    return idx1, idx2, count

def lapack_dlt(X, Y):
    """The reference's own solve (utils/outil.py:68-87: float32 products stored into a float64 8x9 system, numpy's LAPACK SVD,
    Vh[8], float32) for the FEW hypotheses the device flags as rank deficient.  For those systems the null space is two-
    dimensional and "the reference's value" is by definition whatever LAPACK returns on THIS host (it differs between LAPACK
    builds): no device restatement can pin it, the host's own LAPACK does.  X, Y: (k,4,3) float32 numpy -> (k,3,3) float32."""
    import numpy as np
    from . import _lapack
    # the system is built and solved by ONE source text (rfx/_lapack.py: float32 products stored into a float64 8x9 matrix, numpy's
    # full SVD, row 8 of Vh) -- in this process for small batches, dealt to worker processes for large ones (numpy's batched SVD is
    # a serial loop of one dgesdd per system): per system the same LAPACK call on the same data, the same bits
    return _lapack.null_vectors(X, Y).reshape(X.shape[0], 3, 3).astype(np.float32)


def dlt4_homography(X, Y, degenerate="device", info=None):
    """outil.Homography.  ``degenerate="lapack"``: systems flagged rank deficient (csrc/dlt.h) are re-solved with the host's
    LAPACK (lapack_dlt) -- one sync; ``info`` (a dict) receives n_degenerate."""
    X, Y = _dev(X, "X"), _dev(Y, "Y")
    N = X.shape[0]
    H = torch.empty((N, 3, 3), dtype=torch.float32, device=X.device)
    if degenerate != "lapack":
        _call("rfx_dlt4_homography", _one_device(X, Y), _p(X), _p(Y), N, _p(H))
        return H
    fl = torch.empty(N, dtype=torch.uint8, device=X.device)
    _call("rfx_dlt4_homography_flags", _one_device(X, Y), _p(X), _p(Y), N, _p(H), _p(fl))
    bad = ((fl & 4) != 0).nonzero()[:, 0]
    if info is not None:
        info["n_degenerate"] = int(bad.numel())
    if bad.numel():
        H[bad] = torch.from_numpy(lapack_dlt(X[bad].cpu().numpy(), Y[bad].cpu().numpy())).to(H.device)
    return H


def prediction(match1, match2, Hs):
    """outil.Prediction for match1/match2 (n,3) and Hs (N,3,3) -> (N,n) float32 errors."""
    match1, match2, Hs = _dev(match1, "match1"), _dev(match2, "match2"), _dev(Hs, "H21")
    n, N = match1.shape[0], Hs.shape[0]
    err = torch.empty((N, n), dtype=torch.float32, device=match1.device)
    _call("rfx_prediction_f32", _one_device(match1, match2, Hs), _p(match1), _p(match2), n, _p(Hs), N, _p(err))
    return err


def score_hypotheses(match1, match2, samples, tol, degenerate="device"):
    """outil.ScoreRANSAC -> (H (N,3,3), counts (N,) int64).  ``degenerate="lapack"``: rank-deficient samples get the host
    LAPACK's homography (lapack_dlt) and their counts are re-evaluated (rfx_prediction_f32 + torch.det on the host, like the
    reference on a CPU run)."""
    match1, match2 = _dev(match1, "match1"), _dev(match2, "match2")
    samples = _dev(samples, "samples", torch.int64)
    n, N = match1.shape[0], samples.shape[0]
    lib = _lib.load()
    H = torch.empty((N, 3, 3), dtype=torch.float32, device=match1.device)
    counts = torch.empty(N, dtype=torch.int64, device=match1.device)
    ws = torch.empty(lib.rfx_ransac_ws_bytes(n, N), dtype=torch.uint8, device=match1.device)
    fl = torch.empty(N, dtype=torch.uint8, device=match1.device) if degenerate == "lapack" else None   # flags of the SAME DLT pass
    _call("rfx_score_hypotheses", _one_device(match1, match2, samples), _p(match1), _p(match2), n, _p(samples), N, float(tol), _p(H), _p(counts),
          _p(fl), _p(ws))
    if fl is not None:
        bad = ((fl & 4) != 0).nonzero()[:, 0]
        if bad.numel():
            sb = samples[bad]
            Hp = torch.from_numpy(lapack_dlt(match1[sb].cpu().numpy(), match2[sb].cpu().numpy()))
            H[bad] = Hp.to(H.device)
            cnt = torch.cat([(prediction(match1, match2, H[bad[i:i + 4096]]) < tol).sum(dim=1) for i in range(0, bad.numel(), 4096)])
            counts[bad] = cnt * (torch.det(Hp) > 1e-6).long().to(cnt.device)
    return H, counts


def ransac_h4(match1, match2, samples, tol, degenerate="device", info=None):
    """Device RANSAC.  Returns (bestH (3,3) f32, inlier (n,) bool, result int32[4]) as device tensors
    (result = [status, best count, winning hypothesis index, #hypotheses after the duplicate filter]).
    ``degenerate="lapack"``: the two-stage form of ransac_h4_batched for this one pair."""
    match1, match2 = _dev(match1, "match1"), _dev(match2, "match2")
    samples = _dev(samples, "samples", torch.int64)
    n, N = match1.shape[0], samples.shape[0]
    if degenerate == "lapack" and n >= 4:
        nd = torch.tensor([n], dtype=torch.int32, device=match1.device)
        bH, inl, res = ransac_h4_batched(match1[None], match2[None], nd, samples[None], tol, degenerate="lapack", info=info)
        return bH[0], inl[0], res[0]
    lib = _lib.load()
    dev = match1.device
    bestH = torch.empty((3, 3), dtype=torch.float32, device=dev)
    inl = torch.empty(n, dtype=torch.uint8, device=dev)
    res = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.rfx_ransac_ws_bytes(n, N), dtype=torch.uint8, device=dev)
    _call("rfx_ransac_h4", _one_device(match1, match2, samples), _p(match1), _p(match2), n, _p(samples), N, float(tol), _p(bestH), _p(inl), _p(res),
                                 _p(ws))
    return bestH, inl.bool(), res


def gather_matches(idx1, idx2, n, xa, ya, xb, yb):
    """idx1/idx2 (B,cap) int64, n (B,) int32 (device) -> match1, match2 (B,cap,3) float32 (rows >= n[b] are zero)."""
    idx1, idx2 = _dev(idx1, "idx1", torch.int64), _dev(idx2, "idx2", torch.int64)
    n = _dev(n, "n", torch.int32)
    B, cap = idx1.shape
    m1 = torch.empty((B, cap, 3), dtype=torch.float32, device=idx1.device)
    m2 = torch.empty((B, cap, 3), dtype=torch.float32, device=idx1.device)
    _call("rfx_gather_matches_f32", _one_device(idx1, idx2, n, xa, ya, xb, yb), _p(idx1), _p(idx2), _p(n), cap, _p(_dev(xa, "xa")), _p(_dev(ya, "ya")),
                                                 _p(_dev(xb, "xb")), _p(_dev(yb, "yb")), _p(m1), _p(m2), B)
    return m1, m2



def gather_matches_ragged(idx1, idx2, n, xa, ya, offA, xb, yb, offB):
    """gather_matches for a ragged batch: pair b's cell coordinates are xa/ya[offA[b]:], xb/yb[offB[b]:] of the packed tables
    (offA, offB: (B,) int64 device tensors) -> match1, match2 (B,cap,3) float32 (rows >= n[b] are zero)."""
    idx1, idx2 = _dev(idx1, "idx1", torch.int64), _dev(idx2, "idx2", torch.int64)
    n = _dev(n, "n", torch.int32)
    offA, offB = _dev(offA, "offA", torch.int64), _dev(offB, "offB", torch.int64)
    B, cap = idx1.shape
    if n.numel() != B or offA.numel() != B or offB.numel() != B:
        raise ValueError("n / offA / offB must hold one entry per pair")
    m1 = torch.empty((B, cap, 3), dtype=torch.float32, device=idx1.device)
    m2 = torch.empty((B, cap, 3), dtype=torch.float32, device=idx1.device)
    _call("rfx_gather_matches_ragged_f32", _one_device(idx1, idx2, n, xa, ya, offA, xb, yb, offB), _p(idx1), _p(idx2), _p(n), cap,
          _p(_dev(xa, "xa")), _p(_dev(ya, "ya")), _p(offA), _p(_dev(xb, "xb")), _p(_dev(yb, "yb")), _p(offB), _p(m1), _p(m2), B)
    return m1, m2

def _ransac_batched_buffers(match1, match2, n, samples):
    """The validated inputs of a batched search and its freshly allocated outputs: (match1, match2, n, samples), (bestH (B,3,3) f32,
    inl (B,cap) uint8, res (B,4) int32, ws)."""
    match1, match2 = _dev(match1, "match1"), _dev(match2, "match2")
    n = _dev(n, "n", torch.int32)
    samples = _dev(samples, "samples", torch.int64)
    B, cap, _ = match1.shape
    N = samples.shape[1]
    if samples.shape[0] != B or n.shape[0] != B:
        raise ValueError("batch sizes differ")
    dev = match1.device
    bestH = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    inl = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    res = torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().rfx_ransac_batched_ws_bytes(cap, N, B), dtype=torch.uint8, device=dev)
    return (match1, match2, n, samples), (bestH, inl, res, ws)


def ransac_h4_batched(match1, match2, n, samples, tol, degenerate="device", info=None):
    """match1/match2 (B,cap,3), n (B,) int32 device, samples (B,N,4) int64 -> bestH (B,3,3), inlier (B,cap) bool,
    result (B,4) int32 [status (3 = fewer than 4 matches), count, winner, nUnique] -- all device tensors.
    ``degenerate``: what to do with 4-point samples whose 8x9 DLT system is rank deficient (three matched points collinear in
    both images; ~1 % of the draws on the cell lattices).  "device" (default, no host round trip): the Householder sweep's
    own null vector -- a valid unit vector of the 2-D null space, but not the one the host LAPACK's rounding noise picks.
    "lapack": the search runs in two stages around ONE sync: the flagged hypotheses (rfx_ransac_degenerate_gather) are re-solved
    with the host's LAPACK (lapack_dlt: utils/outil.py:68-87 itself) and patched in before counting, so that inlier counts,
    the winner and its inlier indices equal a CPU run of the reference on this host bit for bit even when such a sample wins
    (late multi-homography rounds with a handful of matches left).  ``info`` (dict) receives n_degenerate per pair."""
    if degenerate == "lapack":
        return ransac_h4_batched_finish(ransac_h4_batched_begin(match1, match2, n, samples, tol), info=info)
    (match1, match2, n, samples), (bestH, inl, res, ws) = _ransac_batched_buffers(match1, match2, n, samples)
    (B, cap, _), N = match1.shape, samples.shape[1]
    _call("rfx_ransac_h4_batched", _one_device(match1, match2, n, samples), _p(match1), _p(match2), _p(n), cap, _p(samples), N,
          float(tol), _p(bestH), _p(inl), _p(res), _p(ws), B)
    return bestH, inl.bool(), res


# ---- the exact mode's search, split at its one host wait so that a caller can put other work between the halves -------------

def _alloc_exchange(n_off, rows):
    """One set of pinned exchange buffers of the exact mode: off (n_off) int32, xy (rows,16) f32, H (rows,9) f32 -- written by the
    gather kernel / read by the patch kernel in place (device-visible, coherent memory)."""
    return dict(off=torch.zeros(n_off, dtype=torch.int32).pin_memory(), xy=torch.empty((rows, 16), dtype=torch.float32).pin_memory(),
                H=torch.empty((rows, 9), dtype=torch.float32).pin_memory())


class _ExchangePool:
    """The free list of exchange sets.  A search owns the set it took until it gives it back together with an event recorded behind
    its last launch (rfx_ransac_patch_h_rows reads H asynchronously, and the next owner's host solve writes H): a set is handed out
    again only once that event has completed, to a taker on any stream.  Beyond MAX_IDLE idle sets the oldest whose event has
    completed are dropped; a set still being read is never freed."""
    MAX_IDLE = 8

    def __init__(self):
        self.lock, self.idle, self.allocations = threading.Lock(), [], 0

    def take(self, n_off, rows):
        with self.lock:
            for k, (s, ev) in enumerate(self.idle):
                if s["off"].shape[0] >= n_off and s["xy"].shape[0] >= rows and ev.query():
                    del self.idle[k]
                    return s
            self.allocations += 1
        return _alloc_exchange(n_off, rows)

    def give(self, s, event):
        with self.lock:
            self.idle.append((s, event))
            over = self.idle[:-self.MAX_IDLE]
            self.idle = [e for e in over if not e[1].query()] + self.idle[len(over):]


_EXCHANGE = _ExchangePool()


class _ExactSearch:
    __slots__ = ("odev", "args", "bestH", "inl", "res", "ws", "idx", "cnt", "off", "buf", "event", "B", "N", "cap", "gather_args", "t_begin")


def ransac_h4_batched_begin(match1, match2, n, samples, tol):
    """First half of ransac_h4_batched(degenerate="lapack"): stage 1 (pack + DLT with rank flags) and rfx_ransac_degenerate_gather --
    the flagged samples of all pairs, one 64-byte row each, written by the device straight into pinned host memory -- then an event
    on the launch stream.  Nothing waits here: the caller may enqueue more device work, run another batch's host work or begin
    another search, on this stream or another, before ransac_h4_batched_finish: every search owns its exchange buffers, and
    searches may finish in any order."""
    c = _ExactSearch()
    (match1, match2, n, samples), (c.bestH, c.inl, c.res, c.ws) = _ransac_batched_buffers(match1, match2, n, samples)
    from . import _lapack
    _lapack.load()
    (B, cap, _), N, dev = match1.shape, samples.shape[1], match1.device
    c.odev = _one_device(match1, match2, n, samples)
    c.B, c.N, c.cap = B, N, cap
    c.args = (_p(match1), _p(match2), _p(n), cap, _p(samples), N, float(tol), _p(c.bestH), _p(c.inl), _p(c.res), _p(c.ws), B)
    c.gather_args = (match1, match2, n, samples)                           # kept alive until finish
    _call("rfx_ransac_h4_batched_stage", c.odev, *c.args, 1)
    c.idx = torch.empty((B, N), dtype=torch.int32, device=dev)
    c.cnt = torch.empty(B, dtype=torch.int32, device=dev)
    c.off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    c.buf = _EXCHANGE.take(B + 1, min(B * N, max(1 << 16, B * N // 8)))      # the search's own until finish gives it back
    _exact_gather(c)
    return c


def _exact_gather(c):
    m1, m2, n, smp = c.gather_args
    _call("rfx_ransac_degenerate_gather", c.odev, _p(c.ws), _p(m1), _p(m2), _p(n), c.cap, _p(smp), c.N, c.B, _p(c.idx), _p(c.cnt),
          _p(c.off), _p(c.buf["off"]), _p(c.buf["xy"]), int(c.buf["xy"].shape[0]))
    c.event = torch.cuda.Event()
    c.event.record(torch.cuda.current_stream(c.odev))


def ransac_h4_batched_finish(c, info=None):
    """Second half: wait for the gather (the exact mode's ONE host wait), re-solve the flagged systems with the host's LAPACK
    (rfx/_lapack.py -> librfxhost.so: numpy's own dgesdd on std::threads, utils/outil.py:68-87), patch them in
    (rfx_ransac_patch_h_rows reads the pinned result rows in place), stage 2 (count + select).  Must run under the stream
    ransac_h4_batched_begin ran under.  ``info`` (dict) receives n_degenerate per pair, n_solved, host_ms."""
    import time
    from . import _lapack
    c.event.synchronize()
    B = c.B
    off = c.buf["off"].numpy()
    total = int(off[B])
    if total > c.buf["xy"].shape[0]:                                          # more flagged samples than rows: grow, gather again
        _EXCHANGE.give(c.buf, c.event)
        c.buf = _EXCHANGE.take(B + 1, total)
        _exact_gather(c)
        c.event.synchronize()
        off = c.buf["off"].numpy()
    t0 = time.perf_counter()
    n_solved = 0
    if total > 0:
        _, n_solved = _lapack.solve_rows(c.buf["xy"].numpy()[:total], out=c.buf["H"].numpy())
        _call("rfx_ransac_patch_h_rows", c.odev, _p(c.ws), c.cap, c.N, B, _p(c.idx), _p(c.cnt), _p(c.off), _p(c.buf["H"]),
              int(c.buf["H"].shape[0]))
    if info is not None:
        info["n_degenerate"] = (off[1:B + 1] - off[:B]).tolist()
        info["n_solved"] = n_solved
        info["host_ms"] = (time.perf_counter() - t0) * 1e3
    _call("rfx_ransac_h4_batched_stage", c.odev, *c.args, 2)
    c.event = torch.cuda.Event()
    c.event.record(torch.cuda.current_stream(c.odev))
    _EXCHANGE.give(c.buf, c.event)
    c.gather_args = c.buf = None
    return c.bestH, c.inl.bool(), c.res


# ------------------------------------------------------------------------------------------------ multi-homography rounds (multih.hip)

def draw_samples(n, nb_iter, seed, stream_id, pair_ids=None):
    """RANSAC index draw on the device (utils/outil.py:120 on a GPU run): n (B,) int32 device match counts ->
    samples (B, nb_iter, 4) int64, Philox4x32-10 keyed by (seed, stream_id, pair id, hypothesis) modulo n[b]; pair id =
    pair_ids[b] ((B,) int32 device tensor: the caller's absolute ids) or b.  No host sync."""
    n = _dev(n, "n", torch.int32)
    B = n.shape[0]
    ids = _dev(pair_ids, "pair_ids", torch.int32) if pair_ids is not None else None
    if ids is not None and ids.numel() != B:
        raise ValueError("pair_ids must hold one id per count")
    smp = torch.empty((B, int(nb_iter), 4), dtype=torch.int64, device=n.device)
    _call("rfx_draw_samples_i64", _one_device(n, ids), _p(n), _p(smp), int(nb_iter), B, int(seed) & (2 ** 64 - 1),
          int(stream_id) & (2 ** 64 - 1), _p(ids))
    return smp


def filter_matches(idx1, idx2, count, active, mask, bg, rt, ct, xa, ya, xb, yb, want_kept=False):
    """The cached matches of the active pairs that lie outside the explained region, compacted in order (one launch):
    -> match1, match2 (a,cap,3) float32, n (a,) int32[, kept (a,cap) int32].  ``active``: (a,) int32 device tensor or None."""
    idx1, idx2 = _dev(idx1, "idx1", torch.int64), _dev(idx2, "idx2", torch.int64)
    count = _dev(count, "count", torch.int32)
    mask = _dev(mask, "mask")
    bg = _dev(bg, "bg") if bg is not None else None
    act = _dev(active, "active", torch.int32) if active is not None else None
    B, cap = idx1.shape
    a = B if act is None else act.shape[0]
    h, w = mask.shape[1], mask.shape[2]
    dev = idx1.device
    m1 = torch.empty((a, cap, 3), dtype=torch.float32, device=dev)
    m2 = torch.empty((a, cap, 3), dtype=torch.float32, device=dev)
    n = torch.empty(a, dtype=torch.int32, device=dev)
    kept = torch.empty((a, cap), dtype=torch.int32, device=dev) if want_kept else None
    _call("rfx_filter_matches_f32", _one_device(idx1, idx2, count, act, mask, bg, xa, ya, xb, yb), _p(idx1), _p(idx2), _p(count), cap,
          _p(act), a, _p(mask), _p(bg), h, w, int(rt), int(ct), _p(_dev(xa, "xa")), _p(_dev(ya, "ya")), _p(_dev(xb, "xb")),
          _p(_dev(yb, "yb")), _p(m1), _p(m2), _p(n), _p(kept))
    return (m1, m2, n, kept) if want_kept else (m1, m2, n)


def filter_matches_ragged(idx1, idx2, count, active, mask, bg, moff, geom, xa, ya, offA, xb, yb, offB, want_kept=False):
    """filter_matches for active pairs of DIFFERENT sizes (rfx_filter_matches_ragged_f32, one launch): ``mask`` / ``bg`` are packed
    1-D float32 buffers, pair b's h*w values at element ``moff[b]`` ((B,) int64); ``geom`` (B,6) int32 = h, w, rt, ct, h8, w8 per
    pair; the cell-coordinate tables are packed pair after pair (offA / offB (B,) int64, as for gather_matches_ragged); idx1 / idx2
    (B,cap) + count as mutual_nn_ragged returns them.  Per pair the result is filter_matches' on that pair's own tensors:
    -> match1, match2 (a,cap,3) float32, n (a,) int32[, kept (a,cap) int32]."""
    idx1, idx2 = _dev(idx1, "idx1", torch.int64), _dev(idx2, "idx2", torch.int64)
    count = _dev(count, "count", torch.int32)
    mask = _dev(mask, "mask")
    bg = _dev(bg, "bg") if bg is not None else None
    act = _dev(active, "active", torch.int32) if active is not None else None
    moff, offA, offB = _dev(moff, "moff", torch.int64), _dev(offA, "offA", torch.int64), _dev(offB, "offB", torch.int64)
    geom = _dev(geom, "geom", torch.int32)
    B, cap = idx1.shape
    if mask.dim() != 1 or (bg is not None and bg.shape != mask.shape):
        raise ValueError("mask / bg of a ragged batch are packed 1-D buffers of one size")
    if geom.shape != (B, 6) or moff.numel() != B or offA.numel() != B or offB.numel() != B or count.numel() != B:
        raise ValueError("geom must be (B,6) and moff / offA / offB / count hold one entry per pair")
    a = B if act is None else act.shape[0]
    dev = idx1.device
    m1 = torch.empty((a, cap, 3), dtype=torch.float32, device=dev)
    m2 = torch.empty((a, cap, 3), dtype=torch.float32, device=dev)
    n = torch.empty(a, dtype=torch.int32, device=dev)
    kept = torch.empty((a, cap), dtype=torch.int32, device=dev) if want_kept else None
    _call("rfx_filter_matches_ragged_f32", _one_device(idx1, idx2, count, act, mask, bg, moff, geom, xa, ya, offA, xb, yb, offB),
          _p(idx1), _p(idx2), _p(count), cap, _p(act), a, _p(mask), _p(bg), _p(moff), _p(geom), _p(_dev(xa, "xa")), _p(_dev(ya, "ya")),
          _p(offA), _p(_dev(xb, "xb")), _p(_dev(yb, "yb")), _p(offB), _p(m1), _p(m2), _p(n), _p(kept))
    return (m1, m2, n, kept) if want_kept else (m1, m2, n)


def keep_mask(mask, bg, active, rt, ct, n=None, hw=None, device=None):
    """The (a, rt*ct) 0/1 keep map of variant A / C's getCoarse for the active pairs (rfx_keep_mask_f32): what the per-call
    mutual matching takes as its column mask.  ``mask`` (B,h,w) float32 or None (nothing explained yet: a zero mask is used when
    a background map ``bg`` is given; without ``bg`` either, ``n`` = number of pairs, ``hw`` = (h, w) and ``device`` are
    required)."""
    bgd = _dev(bg, "bg") if bg is not None else None
    act = _dev(active, "active", torch.int32) if active is not None else None
    if mask is None:
        if bgd is None and (n is None or hw is None or device is None):
            raise ValueError("keep_mask without a mask and without a background map needs n, hw = (h, w) and device")
        dev_ = bgd.device if bgd is not None else torch.device(device)
        h, w = (bgd.shape[1], bgd.shape[2]) if bgd is not None else (int(hw[0]), int(hw[1]))
        B = bgd.shape[0] if bgd is not None else int(n)
        m = torch.zeros((B, h, w), dtype=torch.float32, device=dev_) if bgd is not None else None
    else:
        m = _dev(mask, "mask")
        B, h, w = m.shape
        dev_ = m.device
    a = B if act is None else act.shape[0]
    keep = torch.empty((a, int(rt) * int(ct)), dtype=torch.float32, device=dev_)
    _call("rfx_keep_mask_f32", _one_device(keep, m, bgd, act), _p(m), _p(bgd), _p(act), a, h, w, int(rt), int(ct), _p(keep))
    return keep


def keep_mask_ragged(mask, bg, moff, geom, active, ldB, max_cells, keep=None, nB_round=None):
    """keep_mask for active pairs of DIFFERENT sizes (rfx_keep_mask_ragged_f32, one launch): ``mask`` / ``bg`` are the packed 1-D
    float32 buffers of the ragged rounds (pair b's h*w values at element ``moff[b]`` ((B,) int64), ``geom`` (B,6) int32 = h, w, rt, ct,
    h8, w8 per pair); ``bg`` None = all foreground, ``mask`` None = nothing explained yet, both None = every cell kept.  ``active``:
    (a,) int32 device tensor or None (all pairs).  -> ``keep`` (B, ldB) float32: row b of an ACTIVE pair holds its 0/1 keep map in
    its first rt*ct columns (what mutual_nn_ragged takes as maskB); everything else is left as it was (a new tensor: zero).
    ``nB_round`` ((B,) int32, zeroed by the caller, or None) receives rt*ct at the active pairs' positions: the nB with which
    mutual_nn_ragged matches the active pairs only.  ``max_cells``: the largest rt*ct among the active pairs (<= ldB)."""
    m = _dev(mask, "mask") if mask is not None else None
    bgd = _dev(bg, "bg") if bg is not None else None
    act = _dev(active, "active", torch.int32) if active is not None else None
    moff, geom = _dev(moff, "moff", torch.int64), _dev(geom, "geom", torch.int32)
    B, ldB, max_cells = moff.numel(), int(ldB), int(max_cells)
    if geom.shape != (B, 6) or B == 0:
        raise ValueError("geom must be (B,6) and moff hold one offset per pair")
    if any(t is not None and t.dim() != 1 for t in (m, bgd)) or (m is not None and bgd is not None and m.shape != bgd.shape):
        raise ValueError("mask / bg of a ragged batch are packed 1-D buffers of one size")
    if not 0 < max_cells <= ldB:
        raise ValueError("max_cells = %d must lie in [1, ldB = %d]" % (max_cells, ldB))
    if keep is None:
        keep = torch.zeros((B, ldB), dtype=torch.float32, device=moff.device)
    elif not isinstance(keep, torch.Tensor) or keep.dtype != torch.float32 or tuple(keep.shape) != (B, ldB) or not keep.is_contiguous():
        raise ValueError("keep must be a contiguous float32 (B, ldB) tensor (written in place)")
    if nB_round is not None and (not isinstance(nB_round, torch.Tensor) or nB_round.dtype != torch.int32 or nB_round.numel() != B or
                                 not nB_round.is_contiguous()):
        raise ValueError("nB_round must be a contiguous int32 (B,) tensor (written in place)")
    keep = _dev(keep, "keep")
    nbr = _dev(nB_round, "nB_round", torch.int32) if nB_round is not None else None
    a = B if act is None else act.numel()
    if a == 0:
        raise ValueError("no active pair")
    _call("rfx_keep_mask_ragged_f32", _one_device(keep, m, bgd, moff, geom, act, nbr), _p(m), _p(bgd), _p(moff), _p(geom), _p(act), a,
          ldB, max_cells, _p(keep), _p(nbr))
    return keep


class MultiHRecords:
    """The fixed-size per-pair result records of the multi-homography drivers (what
    evaluation/evalHpatch/evaluation.py:254-260 saves per pair), one float32 row per pair so that ONE all_gather moves them:
    [0] nbH (<= max_h) | [1] status (0 ok, 1 no homography, 3 more homographies accepted than the record holds, 4 stopped by the KITTI driver at the record's capacity -- the reference's ``while True`` has no limit) | H (max_h,9) | flowDown8 (max_h,2,h8,w8) | matchDown8 (max_h,2,h8,w8)
    [| flowD2 (max_h,2,hd2,wd2): the half-resolution /8 flow of the KITTI driver].  Filled on the device by multih_accept."""

    def __init__(self, B, h8, w8, device, max_h=11, hd2=0, wd2=0):
        self.B, self.h8, self.w8, self.hd2, self.wd2, self.max_h = B, h8, w8, hd2, wd2, max_h
        r4 = lambda x: (x + 3) // 4 * 4
        self.off_H = 4
        self.off_flow = self.off_H + r4(9 * max_h)
        self.off_match = self.off_flow + 2 * h8 * w8 * max_h
        self.off_d2 = self.off_match + 2 * h8 * w8 * max_h
        self.width = r4(self.off_d2 + 2 * hd2 * wd2 * max_h)
        self.rec = torch.zeros((B, self.width), dtype=torch.float32, device=device)
        self.rec[:, 1] = 1.0

    def rows(self, lo, hi):
        """The records of pairs [lo, hi) as a MultiHRecords of their own over the SAME storage (a lock-step group of the batch)."""
        import copy
        r = copy.copy(self)
        r.B, r.rec = hi - lo, self.rec[lo:hi]
        return r

    def views(self):
        """(nbH (B,), status (B,), H (B,max_h,3,3), flowDown8 (B,max_h,2,h8,w8), matchDown8 (B,max_h,2,h8,w8), flowD2 or None)."""
        r, B, m = self.rec, self.B, self.max_h
        n8 = 2 * self.h8 * self.w8
        d2 = r[:, self.off_d2:self.off_d2 + 2 * self.hd2 * self.wd2 * m].view(B, m, 2, self.hd2, self.wd2) if self.hd2 else None
        return (r[:, 0], r[:, 1], r[:, self.off_H:self.off_H + 9 * m].view(B, m, 3, 3),
                r[:, self.off_flow:self.off_flow + n8 * m].view(B, m, 2, self.h8, self.w8),
                r[:, self.off_match:self.off_match + n8 * m].view(B, m, 2, self.h8, self.w8), d2)


    @staticmethod
    def ragged(h8_list, w8_list, device, max_h=11, hd2_list=None, wd2_list=None):
        """The records of a batch whose pairs differ in size: a MultiHRecordsRagged (the dense layout above is unchanged)."""
        return MultiHRecordsRagged(h8_list, w8_list, device, max_h=max_h, hd2_list=hd2_list, wd2_list=wd2_list)


class MultiHRecordsRagged:
    """MultiHRecords for pairs of DIFFERENT sizes: still one fixed-width float32 row per pair (one all_gather moves a batch), the
    width set by the batch's largest h8 * w8.  Row b: [0] nbH | [1] status (the dense codes) | [2] h8 | [3] w8 of the pair |
    H (max_h,9) from off_H = 4 | flowDown8 (max_h,2,h8,w8) from off_flow | matchDown8 (max_h,2,h8,w8) from off_flow + 2 h8 w8 max_h,
    both laid out with the pair's OWN h8 * w8 (a row of one pair = the dense row of MultiHRecords(1, h8, w8)); the rest of the row
    is zero.  With ``hd2_list`` / ``wd2_list`` (the KITTI driver: the half-resolution /8 sizes per pair) row b gains flowD2
    (max_h,2,hd2,wd2) from off_d2[b] = off_match[b] + 2 h8 w8 max_h, again the dense row of MultiHRecords(1, h8, w8, hd2=, wd2=);
    without them width, offsets and views are unchanged.  A pure function of the size lists.  Filled on the device by
    multih_accept_ragged.
    What the YFCC driver's candidate search decided rides on the object as plain attributes (None unless
    multi_h_variant_c(..., want_records=True) built the records; ``rows`` slices them): ``candidate`` the chosen k per pair (host
    list) and ``candidate_dev`` the same as an int32 device tensor; ``size_src`` (w, h) of each resized source; ``size_tgt`` (w, h)
    of each CHOSEN candidate as resized -- the assembled maps are 8 h8 x 8 w8 = (h, w) of it; ``bg`` the chosen candidates'
    background maps (the script's maskBG) as ONE packed byte buffer in assemble_records' output layout, or None when no It_bg was
    given; ``angle`` (multi_h_variant_c_pairs only) angles[candidate] per pair."""
    candidate = candidate_dev = size_src = size_tgt = bg = angle = None

    def __init__(self, h8_list, w8_list, device, max_h=11, hd2_list=None, wd2_list=None):
        if len(h8_list) != len(w8_list) or not h8_list:
            raise ValueError("one (h8, w8) per pair")
        if (hd2_list is None) != (wd2_list is None) or (hd2_list is not None and
                                                        (len(hd2_list) != len(h8_list) or len(wd2_list) != len(h8_list))):
            raise ValueError("hd2_list and wd2_list: both, one (hd2, wd2) per pair")
        self.h8, self.w8 = [int(x) for x in h8_list], [int(x) for x in w8_list]
        self.B, self.max_h = len(self.h8), max_h
        r4 = lambda x: (x + 3) // 4 * 4
        self.off_H = 4
        self.off_flow = self.off_H + r4(9 * max_h)
        self.off_match = [self.off_flow + 2 * a * b * max_h for a, b in zip(self.h8, self.w8)]
        end = [o + 2 * a * b * max_h for o, a, b in zip(self.off_match, self.h8, self.w8)]
        self.hd2 = self.wd2 = self.off_d2 = self.d2dims = None
        if hd2_list is not None:
            self.hd2, self.wd2, self.off_d2 = [int(x) for x in hd2_list], [int(x) for x in wd2_list], end
            end = [o + 2 * a * b * max_h for o, a, b in zip(self.off_d2, self.hd2, self.wd2)]
            self.d2dims = torch.tensor(list(zip(self.hd2, self.wd2)), dtype=torch.int32).to(device)      # (B,2): the store kernel's table
        self.width = r4(max(end))
        self.rec = torch.zeros((self.B, self.width), dtype=torch.float32, device=device)
        self.rec[:, 1] = 1.0
        self.rec[:, 2] = torch.tensor(self.h8, dtype=torch.float32).to(device)
        self.rec[:, 3] = torch.tensor(self.w8, dtype=torch.float32).to(device)

    def rows(self, lo, hi):
        """The records of pairs [lo, hi) as a MultiHRecordsRagged of their own over the SAME storage (a lock-step group)."""
        import copy
        r = copy.copy(self)
        r.B, r.rec = hi - lo, self.rec[lo:hi]
        r.h8, r.w8, r.off_match = self.h8[lo:hi], self.w8[lo:hi], self.off_match[lo:hi]
        cut = lambda x: None if x is None else x[lo:hi]
        r.candidate, r.candidate_dev, r.size_src, r.size_tgt, r.angle = (cut(x) for x in (self.candidate, self.candidate_dev, self.size_src,
                                                                                           self.size_tgt, self.angle))
        if self.bg is not None:                                  # packed like the assembled maps: 64 h8 w8 bytes per pair
            px = [64 * sum(a * b for a, b in zip(self.h8[:n], self.w8[:n])) for n in (lo, hi)]
            r.bg = self.bg[px[0]:px[1]]
        if self.hd2 is not None:
            r.hd2, r.wd2, r.off_d2, r.d2dims = self.hd2[lo:hi], self.wd2[lo:hi], self.off_d2[lo:hi], self.d2dims[lo:hi]
        return r

    @staticmethod
    def require(records, sizes8, sizes_d2=None):
        """ValueError unless ``records`` is a MultiHRecordsRagged built from a driver's own size lists: ``sizes8[b]`` = (h8, w8) of
        pair b's fine pass and -- the KITTI driver -- ``sizes_d2[b]`` = (hd2, wd2) of its half-resolution pass."""
        ok = isinstance(records, MultiHRecordsRagged) and list(zip(records.h8, records.w8)) == [tuple(s) for s in sizes8]
        if ok and sizes_d2 is not None:
            ok = records.hd2 is not None and list(zip(records.hd2, records.wd2)) == [tuple(s) for s in sizes_d2]
        if not ok:
            raise ValueError("a ragged batch fills an ops.MultiHRecordsRagged built from its pairs' own sizes: h8_list / w8_list = the /8 "
                             "sizes of the fine pass %s%s" % ([tuple(s) for s in sizes8], "" if sizes_d2 is None else
                                                              ", hd2_list / wd2_list = those of the half-resolution pass %s"
                                                              % ([tuple(s) for s in sizes_d2],)))

    def views(self, b):
        """Pair b's (nbH, status, H (max_h,3,3), flowDown8 (max_h,2,h8,w8), matchDown8 (max_h,2,h8,w8)[, flowD2 (max_h,2,hd2,wd2):
        records built with the d2 lists])."""
        r, m, h8, w8 = self.rec[b], self.max_h, self.h8[b], self.w8[b]
        n8 = 2 * h8 * w8
        v = (r[0], r[1], r[self.off_H:self.off_H + 9 * m].view(m, 3, 3), r[self.off_flow:self.off_flow + n8 * m].view(m, 2, h8, w8),
             r[self.off_match[b]:self.off_match[b] + n8 * m].view(m, 2, h8, w8))
        if self.hd2 is not None:
            hd2, wd2 = self.hd2[b], self.wd2[b]
            v += (r[self.off_d2[b]:self.off_d2[b] + 2 * hd2 * wd2 * m].view(m, 2, hd2, wd2),)
        return v


def assemble_records_table(records, out_hw=None):
    """The size table of rfx_assemble_records_f32 for a MultiHRecords / MultiHRecordsRagged, on the host: a pure function of the
    records' size lists and ``out_hw`` -- None (8x each pair's /8 size), one (H, W) for a dense batch, a list of one (H, W) per pair
    for a ragged one.  -> (rows, max_hw, total_px): row b = (element offset of pair b's row | h8 | w8 | off_match | H | W | offset
    of the pair's pixels in the packed outputs | 0), the largest H * W, the pixels of all pairs together."""
    B, ragged = records.B, isinstance(records, MultiHRecordsRagged)
    if (records.hd2 is not None) if ragged else bool(records.hd2):
        raise ValueError("assemble_records: records with a flowD2 part (the KITTI driver's) are not covered; use assemble_kitti per pair")
    h8 = records.h8 if ragged else [records.h8] * B
    w8 = records.w8 if ragged else [records.w8] * B
    offm = records.off_match if ragged else [records.off_match] * B
    if out_hw is None:
        sizes = [(8 * a, 8 * b) for a, b in zip(h8, w8)]
    elif ragged:
        sizes = [tuple(s) if hasattr(s, "__len__") else () for s in out_hw]
        if len(sizes) != B or any(len(s) != 2 for s in sizes):
            raise ValueError("assemble_records: out_hw of a ragged batch is a list of one (H, W) per pair (%d pairs), got %r" % (B, out_hw))
    else:
        if len(out_hw) != 2 or any(hasattr(s, "__len__") for s in out_hw):
            raise ValueError("assemble_records: out_hw of a dense batch is ONE (H, W), got %r" % (out_hw,))
        sizes = [tuple(out_hw)] * B
    sizes = [(int(H), int(W)) for H, W in sizes]
    if any(H <= 0 or W <= 0 or H * W > 0x7fffffff for H, W in sizes):
        raise ValueError("assemble_records: output sizes must be positive (and below 2^31 pixels), got %r" % (sizes,))
    rows, off = [], 0
    for b, (H, W) in enumerate(sizes):
        rows.append((b * records.width, h8[b], w8[b], offm[b], H, W, off, 0))
        off += H * W
    return rows, max(H * W for H, W in sizes), off


def assemble_records(records, th, multiH, cycle, out_hw=None, bg=None, out=None):
    """The offline flow assembly (rfx.assemble.assemble: evalHpatch / evalCorr / evalYFCC getResults.py) of EVERY pair of a batch from
    the drivers' records, in one launch (rfx_assemble_records_f32): per pair bit for bit what assemble.assemble gives on the first
    nbH entries of its record -- nbH is read on the device, no (n,H,W) intermediate exists, nothing syncs with the host.
    records: MultiHRecords or MultiHRecordsRagged (not the KITTI form with flowD2).  out_hw: see assemble_records_table.  bg: the
    background maps ANDed into ``binary`` (YFCC), bool or uint8 -- (B,H,W) for dense records; for ragged ones a list of one (H_b,W_b)
    map per pair or a packed 1-D buffer in the outputs' layout.  out: (flow (total_px,2) float32, match (total_px,) float32, binary
    (total_px,) bool) packed buffers to fill instead of new ones (flow 8-byte aligned); they may not alias the records.
    -> (flowGlobal, matchGlobal, binary, valid): dense records (B,H,W,2), (B,H,W), (B,H,W) bool; ragged records lists of per-pair
    views (H_b,W_b,2), (H_b,W_b), (H_b,W_b) of packed buffers; valid (B,) bool = nbH > 0, on the device (a pair without a homography
    has zeros in all three maps)."""
    if not isinstance(records, (MultiHRecords, MultiHRecordsRagged)):
        raise TypeError("records must be an ops.MultiHRecords or ops.MultiHRecordsRagged")
    ragged = isinstance(records, MultiHRecordsRagged)
    rows, max_hw, total = assemble_records_table(records, out_hw)
    B, dev = records.B, records.rec.device
    sizes = [(r[4], r[5]) for r in rows]
    if bg is not None:
        if ragged and isinstance(bg, (list, tuple)):
            if len(bg) != B or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != s for t, s in zip(bg, sizes)):
                raise ValueError("assemble_records: bg of a ragged batch is one (H, W) map per pair of the sizes %r" % (sizes,))
            parts = bg
        else:
            want = (total,) if ragged else (B,) + sizes[0]
            if not isinstance(bg, torch.Tensor) or tuple(bg.shape) != want:
                raise ValueError("assemble_records: bg must have the shape %r" % (want,))
            parts = [bg]
        if any(t.device != dev for t in parts):
            raise ValueError("assemble_records: bg must live on the records' device %s" % dev)
        if any(t.dtype not in (torch.bool, torch.uint8) for t in parts):
            raise ValueError("assemble_records: bg must be bool or uint8")
        bg = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]) if len(parts) > 1 else parts[0]
    if out is not None:
        fg, mg, binary = out
        for t, shape, dts, name in ((fg, (total, 2), (torch.float32,), "flow"), (mg, (total,), (torch.float32,), "match"),
                                    (binary, (total,), (torch.bool,), "binary")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype not in dts or not t.is_contiguous() or t.device != dev:
                raise ValueError("assemble_records: out %s must be a contiguous %s %s tensor on %s" % (name, shape, dts[0], dev))
        if fg.data_ptr() % 8:
            raise ValueError("assemble_records: the flow output is accessed as float2 and must be 8-byte aligned")
    rec = _dev(records.rec, "records")
    if out is None:
        fg = torch.empty((total, 2), dtype=torch.float32, device=dev)
        mg = torch.empty(total, dtype=torch.float32, device=dev)
        binary = torch.empty(total, dtype=torch.bool, device=dev)
    b8 = _mask_bytes(bg, "bg") if bg is not None else None
    table = torch.tensor(rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    _call("rfx_assemble_records_f32", _one_device(rec, b8, fg, mg, binary), _p(rec), rec.numel(), records.width, records.max_h,
          records.off_H, records.off_flow, _p(table), B, max_hw, float(th), 1 if multiH else 0, 1 if cycle else 0, _p(b8), _p(fg),
          _p(mg), _p(binary), total)
    valid = rec[:, 0] >= 1                                    # the kernel's own test of nbH
    if not ragged:
        H, W = sizes[0]
        return fg.view(B, H, W, 2), mg.view(B, H, W), binary.view(B, H, W), valid
    views = [(r[6], r[4], r[5]) for r in rows]
    return ([fg[o:o + H * W].view(H, W, 2) for o, H, W in views], [mg[o:o + H * W].view(H, W) for o, H, W in views],
            [binary[o:o + H * W].view(H, W) for o, H, W in views], valid)


def warp_image_table(sizes, src, tgt=None, device=None):
    """The image table of rfx_warp_records_u8 / rfx_warp_flow_u8, on the host: ``sizes[b]`` = (H, W) of pair b's OUTPUT map; ``src`` a
    (B,Hs,Ws,3) uint8 tensor or a list of one (Hs_b,Ws_b,3) uint8 tensor per pair (any sizes, read where they lie); ``tgt`` None, or
    the targets in the same two forms, each (H_b,W_b,3) -- the pair's output size.  ``device``: the device every image must live on
    (None: not checked, for a host-only look at the table).  -> (rows, keep): row b = (source address | Hs | Ws | target address or
    0); keep = the tensors whose addresses the rows carry, to be held until the launch is enqueued.  ValueError for a wrong count,
    dtype, shape, contiguity or target size, RuntimeError for a wrong device."""
    B = len(sizes)

    def images(x, name):
        if isinstance(x, torch.Tensor):
            if x.dim() != 4 or x.shape[0] != B:
                raise ValueError("warp_image: %s is a (B,H,W,3) uint8 tensor or a list of one (H,W,3) uint8 tensor per pair (%d pairs), "
                                 "got the shape %r" % (name, B, tuple(x.shape)))
            return [x[b] for b in range(B)]
        if not isinstance(x, (list, tuple)) or len(x) != B or any(not isinstance(t, torch.Tensor) for t in x):
            raise ValueError("warp_image: %s is a (B,H,W,3) uint8 tensor or a list of one (H,W,3) uint8 tensor per pair (%d pairs)"
                             % (name, B))
        return list(x)

    def check(t, name, b, want=None):
        if t.dtype != torch.uint8:
            raise ValueError("warp_image: %s of pair %d must be uint8, got %s" % (name, b, t.dtype))
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1 or t.shape[0] * t.shape[1] > 0x7fffffff:
            raise ValueError("warp_image: %s of pair %d must be (H,W,3) with 1 <= H*W < 2^31, got %r" % (name, b, tuple(t.shape)))
        if want is not None and tuple(t.shape[:2]) != tuple(want):
            raise ValueError("warp_image: %s of pair %d must have the pair's output size %r, got %r" % (name, b, tuple(want), tuple(t.shape[:2])))
        if not t.is_contiguous():
            raise ValueError("warp_image: %s of pair %d must be contiguous (it is read where it lies)" % (name, b))
        if device is not None and t.device != torch.device(device):
            raise RuntimeError("warp_image: %s of pair %d is on %s, the call runs on %s" % (name, b, t.device, device))

    srcs = images(src, "src")
    tgts = images(tgt, "tgt") if tgt is not None else [None] * B
    rows = []
    for b, (s, t) in enumerate(zip(srcs, tgts)):
        check(s, "src", b)
        if t is not None:
            check(t, "tgt", b, want=sizes[b])
        rows.append((s.data_ptr(), int(s.shape[0]), int(s.shape[1]), t.data_ptr() if t is not None else 0))
    return rows, srcs + [t for t in tgts if t is not None]


def _warp_u8_outputs(out, total, dev, overlay, mask, what):
    """(img, overlay | None, mask | None) packed uint8 buffers: new ones, or ``out`` = (img (total,3), overlay (total,3) | None,
    mask (total,) | None) checked."""
    if out is None:
        return (torch.empty((total, 3), dtype=torch.uint8, device=dev),
                torch.empty((total, 3), dtype=torch.uint8, device=dev) if overlay else None,
                torch.empty(total, dtype=torch.uint8, device=dev) if mask else None)
    if len(out) != 3:
        raise ValueError("%s: out is (img, overlay or None, mask or None)" % what)
    for t, shape, name, need in ((out[0], (total, 3), "img", True), (out[1], (total, 3), "overlay", overlay), (out[2], (total,), "mask", mask)):
        if t is None and not need:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.uint8 or not t.is_contiguous() or t.device != dev:
            raise ValueError("%s: out %s must be a contiguous %s uint8 tensor on %s" % (what, name, shape, dev))
    return out[0], out[1] if overlay else None, out[2] if mask else None


def _warp_u8_views(bufs, rows, dense):
    """The packed outputs as the caller sees them: (B,H,W[,3]) tensors for a dense batch, lists of per-pair views for a ragged one."""
    def view(t):
        if t is None:
            return None
        tail = tuple(t.shape[1:])
        if dense:
            return t.view((len(rows), rows[0][4], rows[0][5]) + tail)
        return [t[r[6]:r[6] + r[4] * r[5]].view((r[4], r[5]) + tail) for r in rows]
    return tuple(view(t) for t in bufs)


def warp_records_u8(records, src, th, multiH, cycle, out_hw=None, bg=None, tgt=None, want_mask=False, out=None):
    """The aligned source image of EVERY pair of a batch from the drivers' records, as uint8 HWC, in one launch
    (rfx_warp_records_u8; quick_start/align2images.py:97-98,117 and, with ``tgt``, the 50 % overlay of :25-28,112): per pair bit
    for bit what assemble_records -> grid_sample(u8_to_f32(src) raw, flow) -> clamp(0,1).mul(255).byte() -> HWC gives, without the
    flow, the float source or the float image.  records, th, multiH, cycle, out_hw, bg: as assemble_records takes them (KITTI
    records are refused: warp_flow_u8 takes their assembled flow).  src / tgt: see warp_image_table -- sources of any sizes, read
    where they lie; a target has its pair's output size.  want_mask: also ``binary`` of assemble_records as a 0 / 255 byte map.
    out: (img (total_px,3), overlay (total_px,3) or None, mask (total_px,) or None) packed uint8 buffers to fill.
    -> (img, overlay | None, mask | None, valid): dense records (B,H,W,3), (B,H,W,3), (B,H,W) uint8; ragged records lists of
    per-pair views of packed buffers; valid (B,) bool = nbH > 0 on the device (a pair without a homography has the zero flow: its
    image is the source's centre colour).  Everything is checked on the host before any HIP call; nothing syncs."""
    if not isinstance(records, (MultiHRecords, MultiHRecordsRagged)):
        raise TypeError("records must be an ops.MultiHRecords or ops.MultiHRecordsRagged")
    ragged = isinstance(records, MultiHRecordsRagged)
    rows, max_hw, total = assemble_records_table(records, out_hw)          # refuses records with a flowD2 part
    B, dev = records.B, records.rec.device
    sizes = [(r[4], r[5]) for r in rows]
    irows, keep = warp_image_table(sizes, src, tgt, device=dev)
    if bg is not None:
        parts = list(bg) if isinstance(bg, (list, tuple)) else [bg]
        shapes = [tuple(getattr(t, "shape", ())) for t in parts]
        dense_shape = None if ragged else [(B,) + sizes[0]]
        if (shapes != sizes) if isinstance(bg, (list, tuple)) else (shapes not in ([(total,)], dense_shape)):
            raise ValueError("warp_records_u8: bg is a packed (%d,) buffer%s or one map per pair of the shapes %r, got %r"
                             % (total, "" if ragged else ", a %r tensor" % (dense_shape[0],), sizes, shapes))
        if any(not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8) for t in parts):
            raise ValueError("warp_records_u8: bg must be bool or uint8 tensors")
        if any(t.device != dev for t in parts):
            raise RuntimeError("warp_records_u8: bg must live on the records' device %s" % dev)
    img, overlay, mask = _warp_u8_outputs(out, total, dev, tgt is not None, want_mask, "warp_records_u8")
    rec = _dev(records.rec, "records")
    if bg is not None:
        bg = _mask_bytes(_packed_maps(parts if len(parts) > 1 else parts[0], "bg").reshape(-1), "bg")
    import numpy as np
    table, itable = _upload_i64([np.asarray(rows, np.int64), np.asarray(irows, np.int64)], dev)
    _call("rfx_warp_records_u8", _one_device(rec, bg, img, overlay, mask), _p(rec), rec.numel(), records.width, records.max_h,
          records.off_H, records.off_flow, _p(table), B, max_hw, float(th), 1 if multiH else 0, 1 if cycle else 0, _p(bg), _p(itable),
          _p(img), _p(overlay), _p(mask), total)
    del keep                                                   # the images were referenced until the launch was enqueued
    valid = rec[:, 0] >= 1
    return _warp_u8_views((img, overlay, mask), rows, not ragged) + (valid,)


def warp_flow_u8(flow, src, tgt=None, binary=None, out=None):
    """The image tail of warp_records_u8 on a stored flow (rfx_warp_flow_u8): quick-start's flow12, assemble_kitti_records' flow, any
    flow a caller holds.  flow: (H,W,2) or (B,H,W,2) float32, or a list of one (H_b,W_b,2) map per pair (the views assemble_records
    returns for a ragged batch are taken as the one packed buffer they are; other lists are concatenated).  src / tgt: see
    warp_image_table.  binary: None, or bool / uint8 maps in flow's form without the last axis, passed through as a 0 / 255 byte map.
    -> (img, overlay | None, mask | None) in flow's form: (H,W,3) / (B,H,W,3) uint8 or lists of per-pair views.  No sync."""
    single = isinstance(flow, torch.Tensor) and flow.dim() == 3
    listed = isinstance(flow, (list, tuple))
    parts = list(flow) if listed else [flow]
    if not parts or any(not isinstance(t, torch.Tensor) for t in parts) or \
            (listed and any(t.dim() != 3 or t.shape[2] != 2 for t in parts)) or \
            (not listed and (flow.dim() not in (3, 4) or flow.shape[-1] != 2)):
        raise ValueError("warp_flow_u8: flow is (H,W,2), (B,H,W,2) or a list of (H,W,2) float32 maps")
    if any(t.dtype != torch.float32 for t in parts):
        raise ValueError("warp_flow_u8: flow must be float32, got %s" % parts[0].dtype)
    if not listed and not flow.is_contiguous():
        raise ValueError("warp_flow_u8: flow must be contiguous")
    if parts[0].data_ptr() % 8:
        raise ValueError("warp_flow_u8: the flow is read as float2 and must be 8-byte aligned")
    if any(t.numel() == 0 for t in parts):
        raise ValueError("warp_flow_u8: an empty flow map")
    if listed:
        sizes = [(int(t.shape[0]), int(t.shape[1])) for t in parts]
    else:
        sizes = [(int(flow.shape[-3]), int(flow.shape[-2]))] * (1 if single else int(flow.shape[0]))
    if any(H * W > 0x7fffffff for H, W in sizes):
        raise ValueError("warp_flow_u8: maps have fewer than 2^31 pixels, got %r" % (sizes,))
    B, dev = len(sizes), parts[0].device
    rows, off = [], 0
    for H, W in sizes:
        rows.append((0, 0, 0, 0, H, W, off, 0))
        off += H * W
    total, max_hw = off, max(H * W for H, W in sizes)
    if single:                                                 # one map: its images may come without the batch axis
        src = [src] if isinstance(src, torch.Tensor) and src.dim() == 3 else src
        tgt = [tgt] if isinstance(tgt, torch.Tensor) and tgt.dim() == 3 else tgt
    irows, keep = warp_image_table(sizes, src, tgt, device=dev)
    if binary is not None:
        bparts = list(binary) if isinstance(binary, (list, tuple)) else [binary]
        want = sizes if listed else [tuple(flow.shape[:-1])]
        if [tuple(getattr(t, "shape", ())) for t in bparts] != want:
            raise ValueError("warp_flow_u8: binary has flow's form without the last axis %r" % (want,))
        if any(not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8) for t in bparts):
            raise ValueError("warp_flow_u8: binary must be bool or uint8")
        if any(t.device != dev for t in bparts):
            raise RuntimeError("warp_flow_u8: binary must live on the flow's device %s" % dev)
    img, overlay, mask = _warp_u8_outputs(out, total, dev, tgt is not None, binary is not None, "warp_flow_u8")
    f = _dev(_packed_maps(parts if listed else flow, "flow").reshape(-1, 2), "flow")
    if f.data_ptr() % 8:
        raise ValueError("warp_flow_u8: the flow is read as float2 and must be 8-byte aligned")
    if binary is not None:
        binary = _mask_bytes(_packed_maps(bparts if listed else binary, "binary").reshape(-1), "binary")
    import numpy as np
    table, itable = _upload_i64([np.asarray(rows, np.int64), np.asarray(irows, np.int64)], dev)
    _call("rfx_warp_flow_u8", _one_device(f, binary, img, overlay, mask), _p(f), _p(table), B, max_hw, _p(binary), _p(itable), _p(img),
          _p(overlay), _p(mask), total)
    del keep                                                   # the images were referenced until the launch was enqueued
    if listed:
        return _warp_u8_views((img, overlay, mask), rows, False)
    shape = tuple(flow.shape[:-1])
    return tuple(None if t is None else t.view(shape + tuple(t.shape[1:])) for t in (img, overlay, mask))


def _host_pixels(v, what):
    """A host keypoint coordinate array as int64, floats truncated toward zero like the scripts' ``astype(np.int64)``."""
    import numpy as np
    a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
    if a.dtype.kind not in "iuf":
        raise TypeError("%s: keypoint coordinates are integers or floats, got %s" % (what, a.dtype))
    return a.astype(np.int64).reshape(-1)


def records_keypoints_table(records, xb, yb, sizesA=None, out_hw=None):
    """The host part of records_keypoints, a pure function of the records' size lists and the keypoints: -> (rows, total_px, krows,
    x, y, koff).  rows / total_px: assemble_records_table's; krows[b] = (first keypoint | number of keypoints | wA | hA), the
    keypoint table of rfx_records_keypoints_f32; x, y the target pixels of all pairs, pair after pair, as int32 arrays (floats
    truncated toward zero); koff (B+1,) the host offset list, pair b's keypoints are koff[b]:koff[b+1].  ``xb`` / ``yb``: one host
    array per pair (empty arrays allowed); ``sizesA[b]`` = (wA, hA), by default records.size_src.  A keypoint outside its pair's
    map is refused here (RfxError), as sample_points refuses it."""
    import numpy as np
    if not isinstance(records, (MultiHRecords, MultiHRecordsRagged)):
        raise TypeError("records must be an ops.MultiHRecords or ops.MultiHRecordsRagged")
    rows, _, total = assemble_records_table(records, out_hw)       # refuses records with a flowD2 part (the KITTI drivers')
    B = records.B
    sizesA = getattr(records, "size_src", None) if sizesA is None else sizesA
    if sizesA is None:
        raise ValueError("records_keypoints: these records carry no size_src; pass sizesA = one (wA, hA) per pair")
    if len(xb) != B or len(yb) != B or len(sizesA) != B:
        raise ValueError("records_keypoints: one xb, one yb and one (wA, hA) per pair (%d pairs), got %d, %d and %d"
                         % (B, len(xb), len(yb), len(sizesA)))
    krows, xs, ys, off = [], [], [], 0
    for b in range(B):
        x, y = _host_pixels(xb[b], "records_keypoints"), _host_pixels(yb[b], "records_keypoints")
        if x.shape != y.shape:
            raise ValueError("records_keypoints: pair %d has %d xb for %d yb" % (b, x.size, y.size))
        wA, hA = int(sizesA[b][0]), int(sizesA[b][1])
        H, W = rows[b][4], rows[b][5]
        if wA < 1 or hA < 1 or wA > 0x7fffffff or hA > 0x7fffffff or \
                (x.size and (x.min() < 0 or x.max() >= W or y.min() < 0 or y.max() >= H)):
            _lib.check(-1, "rfx_records_keypoints_f32 (pair %d: a keypoint outside the %d x %d map, or sizeA = %s)" % (b, W, H, (wA, hA)))
        krows.append((off, int(x.size), wA, hA))
        xs.append(x)
        ys.append(y)
        off += int(x.size)
    if off > 0x7fffffff:
        _lib.check(-2, "rfx_records_keypoints_f32 (%d keypoints)" % off)
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return rows, total, krows, cat(xs), cat(ys), [r[0] for r in krows] + [off]


def _upload_i64(parts, dev):
    """Host int64 arrays -> device tensors through ONE pinned, non-blocking copy (no sync)."""
    import numpy as np
    flat = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])
    buf = torch.from_numpy(flat).pin_memory().to(dev, non_blocking=True)
    out, o = [], 0
    for p in parts:
        n = int(np.asarray(p).size)
        out.append(buf[o:o + n])
        o += n
    return out


def records_keypoints(records, th, multiH, cycle, xb, yb, sizesA=None, out_hw=None, bg=None):
    """The assembled maps of EVERY pair of a batch of device records, read at annotated target pixels only
    (rfx_records_keypoints_f32; evaluation/evalCorr/getResults.py:78-136 as :15-31 and :281-282 read it): per pair bit for bit what
    assemble_records followed by sample_points gives at the same pixels, without the maps -- one thread per keypoint walks the
    record's homographies at its pixel.  records, th, multiH, cycle, out_hw: as assemble_records takes them; xb, yb, sizesA: see
    records_keypoints_table; bg: a packed (total_px,) bool / uint8 buffer in assemble_records' output layout, a (B,H,W) tensor for
    dense records, or a list of one (H_b,W_b) map per pair.
    -> (xa, ya float32, m float32 = matchGlobal at the pixel, flag uint8: bit 0 = binary at the pixel (ANDed with bg), bit 1 = both
    flow channels in [-1, 1] (clear only for a NaN), koff): device tensors of K_total = koff[-1] entries, pair b's at
    koff[b]:koff[b+1]; koff is the host list.  The tables and keypoints go up in one pinned, non-blocking copy; nothing syncs."""
    import numpy as np
    rows, total, krows, x, y, koff = records_keypoints_table(records, xb, yb, sizesA, out_hw)
    B, dev, K = records.B, records.rec.device, koff[-1]
    if bg is not None:
        parts = list(bg) if isinstance(bg, (list, tuple)) else [bg]
        shapes = [tuple(getattr(t, "shape", ())) for t in parts]
        sizes = [(r[4], r[5]) for r in rows]
        dense = [(B,) + sizes[0]] if not isinstance(records, MultiHRecordsRagged) else None
        if not isinstance(bg, (list, tuple)) and shapes not in ([(total,)], dense) or isinstance(bg, (list, tuple)) and shapes != sizes:
            raise ValueError("records_keypoints: bg is a packed (%d,) buffer%s or one map per pair of the shapes %r, got %r"
                             % (total, "" if dense is None else ", a %r tensor" % (dense[0],), sizes, shapes))
        if any(not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8) for t in parts):
            raise ValueError("records_keypoints: bg must be bool or uint8 tensors")
        if any(t.device != dev for t in parts):
            raise ValueError("records_keypoints: bg must live on the records' device %s" % dev)
        bg = _mask_bytes(_packed_maps(parts if len(parts) > 1 else parts[0], "bg").reshape(-1), "bg")
    rec = _dev(records.rec, "records")
    xa = torch.empty(K, dtype=torch.float32, device=dev)
    ya = torch.empty(K, dtype=torch.float32, device=dev)
    m = torch.empty(K, dtype=torch.float32, device=dev)
    flag = torch.empty(K, dtype=torch.uint8, device=dev)
    if K:
        xy = np.concatenate((x, y)).view(np.int64)                # 2 K int32 pixels ride in the int64 upload two to a word
        table, ktable, xyd = _upload_i64([np.asarray(rows, np.int64), np.asarray(krows, np.int64), xy], dev)
        xyd = xyd.view(torch.int32)
        _call("rfx_records_keypoints_f32", _one_device(rec, bg, xa), _p(rec), rec.numel(), records.width, records.max_h, records.off_H,
              records.off_flow, _p(table), B, total, float(th), 1 if multiH else 0, 1 if cycle else 0, _p(bg), _p(ktable),
              _p(xyd[:K]), _p(xyd[K:]), K, _p(xa), _p(ya), _p(m), _p(flag))
    return xa, ya, m, flag, koff


PCK_MAX_GRID = 16              # thresholds of the pixel grid rfx_pck_tally_f64 takes


def pck_pixel_grid():
    """The pixel grid of evaluation/evalCorr/getResults.py:230: 1, 2, 3, 5, 8, 13, 22, 36."""
    import numpy as np
    return np.around(np.logspace(0, np.log10(36), 8))


def pck_tally(xa, ya, m, flag, xs, ys, koff, match_ths=(0.0,), pixel_grid=None, valid=None, want_dist=False):
    """evaluation/evalCorr/getResults.py:279-285 with alignmentError (:25-36) on the outputs of records_keypoints, for every pair and
    every matchability threshold at once (rfx_pck_tally_f64): threshold t > 0 keeps a keypoint with m >= t whose flow is inside
    [-1, 1], t <= 0 keeps every keypoint; d = sqrt((double(xa) - xs)^2 + (double(ya) - ys)^2) in float64 steps like numpy's.
    xs, ys: the source keypoints, one host array per pair (floats truncated toward zero) in koff's order; match_ths (M); pixel_grid
    (T <= 16 values, default the script's 1..36 grid); valid: (B,) bool / uint8 on the device or None -- a pair with valid 0 follows
    the script's ``continue`` branch (:273-277): nb = its keypoints, counts zero.
    -> (counts (M,B,T) int64, nb (M,B) int64[, dist (M,K_total) float64, NaN where a keypoint is not kept]) on the device.  No sync."""
    import numpy as np
    B, K = len(koff) - 1, int(koff[-1])
    if B < 1 or len(xs) != B or len(ys) != B:
        raise ValueError("pck_tally: one xs and one ys per pair (%d pairs), got %d and %d" % (B, len(xs), len(ys)))
    grid = pck_pixel_grid() if pixel_grid is None else np.asarray(pixel_grid, dtype=np.float64).reshape(-1)
    ths = np.asarray(match_ths, dtype=np.float32).reshape(-1)
    T, M = int(grid.size), int(ths.size)
    if T < 1 or T > PCK_MAX_GRID or M < 1:
        raise ValueError("pck_tally: 1 to %d pixel thresholds and at least one matchability threshold, got %d and %d" % (PCK_MAX_GRID, T, M))
    outs = ((xa, torch.float32, "xa"), (ya, torch.float32, "ya"), (m, torch.float32, "m"), (flag, torch.uint8, "flag"))
    for t, dt, name in outs:                                      # every host-side check before any device
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.numel() != K or not t.is_contiguous():
            raise ValueError("pck_tally: %s must be a contiguous %s tensor of koff[-1] = %d entries" % (name, dt, K))
    hx, hy = [], []
    for b in range(B):
        sx, sy = _host_pixels(xs[b], "pck_tally"), _host_pixels(ys[b], "pck_tally")
        n = int(koff[b + 1]) - int(koff[b])
        if sx.size != n or sy.size != n:
            raise ValueError("pck_tally: pair %d has %d keypoints, got %d xs and %d ys" % (b, n, sx.size, sy.size))
        if n and max(np.abs(sx).max(), np.abs(sy).max()) > 0x7fffffff:
            _lib.check(-2, "rfx_pck_tally_f64 (a source keypoint beyond int32)")
        hx.append(sx)
        hy.append(sy)
    if valid is not None and (not isinstance(valid, torch.Tensor) or valid.numel() != B or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("pck_tally: valid is a (B,) bool or uint8 tensor")
    for t, dt, name in outs:
        _dev(t, name, dt)
    if valid is not None:
        valid = _mask_bytes(valid.reshape(-1), "valid")
    dev = xa.device
    xy = np.concatenate(hx + hy).astype(np.int32)
    xy = np.concatenate((xy, np.zeros(xy.size % 2, np.int32))).view(np.int64)      # int32 pixels, two to a word
    krows = np.asarray([(int(koff[b]), int(koff[b + 1]) - int(koff[b]), 1, 1) for b in range(B)], np.int64)
    ktable, gd, td, xyd = _upload_i64([krows, grid.view(np.int64), np.concatenate((ths, np.zeros(M % 2, np.float32))).view(np.int64), xy],
                                      dev)
    gd, td, xyd = gd.view(torch.float64), td.view(torch.float32), xyd.view(torch.int32)
    counts = torch.empty((M, B, T), dtype=torch.int64, device=dev)
    nb = torch.empty((M, B), dtype=torch.int64, device=dev)
    dist = torch.empty((M, K), dtype=torch.float64, device=dev) if want_dist else None
    _call("rfx_pck_tally_f64", _one_device(xa, ya, m, flag, valid, counts), _p(xa), _p(ya), _p(m), _p(flag), _p(xyd[:K]), _p(xyd[K:]),
          _p(ktable), B, K, _p(td), M, _p(gd), T, _p(valid), _p(counts), _p(nb), _p(dist))
    return (counts, nb, dist) if want_dist else (counts, nb)


KITTI_WS_BYTES = 1 << 30       # default workspace bound of assemble_kitti_records (scores + component-filter workspace of one chunk)
KITTI_TABLE_COLS = 12


def _kitti_records(records, what):
    """(ragged?, per-pair hd2, wd2, off_d2) of records with a flowD2 part; TypeError / ValueError otherwise."""
    if not isinstance(records, (MultiHRecords, MultiHRecordsRagged)):
        raise TypeError("records must be an ops.MultiHRecords or ops.MultiHRecordsRagged")
    ragged = isinstance(records, MultiHRecordsRagged)
    if not ((records.hd2 is not None) if ragged else bool(records.hd2)):
        raise ValueError("%s: records without a flowD2 part are not the KITTI drivers'; use assemble_records" % what)
    B = records.B
    if ragged:
        return True, records.hd2, records.wd2, records.off_d2
    return False, [records.hd2] * B, [records.wd2] * B, [records.off_d2] * B


def assemble_kitti_records_table(records, out_hw=None, cc_th=0.0):
    """The size table of rfx_assemble_kitti_records_f32 / rfx_kitti_scores_records_f32 for records of the KITTI drivers, on the host:
    a pure function of the records' size lists, ``out_hw`` (None: 8x each pair's /8 size; one (H, W) for a dense batch; one (H, W)
    per pair for a ragged one) and ``cc_th``.  -> (rows, max_hw, total_px): row b = (element offset of pair b's row | h8 | w8 |
    off_match | off_d2 | hd2 | wd2 | H | W | offset of the pair's pixels in the packed outputs | element offset of the pair's score
    map 0 in the batch's packed scores, max_h maps of H * W per pair | cc_max_area(H * W, cc_th))."""
    what = "assemble_kitti_records"
    ragged, hd2, wd2, offd2 = _kitti_records(records, what)
    cc_th = float(cc_th)
    if not cc_th >= 0:
        raise ValueError("%s: cc_th must be >= 0, got %r" % (what, cc_th))
    B = records.B
    h8 = records.h8 if ragged else [records.h8] * B
    w8 = records.w8 if ragged else [records.w8] * B
    offm = records.off_match if ragged else [records.off_match] * B
    if out_hw is None:
        sizes = [(8 * a, 8 * b) for a, b in zip(h8, w8)]
    elif ragged:
        sizes = [tuple(s) if hasattr(s, "__len__") else () for s in out_hw]
        if len(sizes) != B or any(len(s) != 2 for s in sizes):
            raise ValueError("%s: out_hw of a ragged batch is a list of one (H, W) per pair (%d pairs), got %r" % (what, B, out_hw))
    else:
        if len(out_hw) != 2 or any(hasattr(s, "__len__") for s in out_hw):
            raise ValueError("%s: out_hw of a dense batch is ONE (H, W), got %r" % (what, out_hw))
        sizes = [tuple(out_hw)] * B
    sizes = [(int(H), int(W)) for H, W in sizes]
    if any(H <= 0 or W <= 0 or H * W > 0x7fffffff for H, W in sizes):
        raise ValueError("%s: output sizes must be positive (and below 2^31 pixels), got %r" % (what, sizes))
    rows, off, soff = [], 0, 0
    for b, (H, W) in enumerate(sizes):
        rows.append((b * records.width, h8[b], w8[b], offm[b], offd2[b], hd2[b], wd2[b], H, W, off, soff, cc_max_area(H * W, cc_th)))
        off += H * W
        soff += records.max_h * H * W
    return rows, max(H * W for H, W in sizes), off


def _kitti_plan(rows, max_h, cc_th, ws_bytes):
    if ws_bytes is None:
        ws_bytes = KITTI_WS_BYTES
    if isinstance(ws_bytes, bool) or not isinstance(ws_bytes, int) or ws_bytes <= 0:
        raise ValueError("assemble_kitti_records: ws_bytes must be a positive int, got %r" % (ws_bytes,))
    if max_h > 65535:
        raise ValueError("assemble_kitti_records: max_h above 65535")
    max_pairs = 65535 // max_h                                # blockIdx.y of the score kernel = (pair, homography)
    plan, lo, elems = [], 0, 0
    for b, r in enumerate(rows):
        need = max_h * r[7] * r[8] if cc_th > 0 else 0        # floats of scores; 16 bytes each with the filter's three int32
        if need > 0x7fffffff:
            raise ValueError("assemble_kitti_records: the %d score maps of pair %d exceed 2^31 - 1 elements" % (max_h, b))
        if b > lo and (b - lo >= max_pairs or 16 * (elems + need) > ws_bytes or elems + need > 0x7fffffff):
            plan.append((lo, b))
            lo, elems = b, 0
        elems += need
    plan.append((lo, len(rows)))
    return plan


def assemble_kitti_records_plan(records, out_hw=None, cc_th=0.0, ws_bytes=None):
    """The chunks assemble_kitti_records processes one after the other: [(lo, hi), ...], consecutive, covering every pair once.  With
    cc_th > 0 a chunk's workspace -- 4 bytes of scores and 12 bytes of component-filter workspace per pixel and homography, sized by
    max_h because nbH is known to the device only -- stays within ``ws_bytes`` (default 1 GiB) unless a single pair needs more (at least
    one pair per chunk).  A chunk also holds at most 65535 // max_h pairs and 2^31 - 1 score elements.  A pure host function."""
    rows, _, _ = assemble_kitti_records_table(records, out_hw, cc_th)
    return _kitti_plan(rows, records.max_h, float(cc_th), ws_bytes)


def assemble_kitti_records(records, th, multiH, cc_th=0.0, interpolate=False, out_hw=None, out=None, ws_bytes=None):
    """The KITTI flow assembly (rfx.assemble.assemble_kitti: evalKITTI/getResults.py:95-141) of EVERY pair of a batch from the KITTI
    drivers' records (built with the d2 lists), per pair bit for bit what assemble_kitti(..., fill="device") gives on the first nbH
    entries of its record: nbH is read on the device and nothing syncs with the host.  cc_th == 0: ONE launch
    (rfx_assemble_kitti_records_f32).  cc_th > 0: per chunk of pairs (assemble_kitti_records_plan; the result does not depend on the
    plan) the scores of all homographies (rfx_kitti_scores_records_f32), the component filter in place on them
    (rfx_remove_small_cc_ragged_f32) and the merge on the filtered scores -- six launches; the score buffer and the filter's workspace
    are the only (n,H,W) memory.  interpolate: ops.nearest_fill of the flow with ``binary``, one call for dense records, one per run
    of consecutive same-size pairs for ragged ones.  out_hw, out and the result: as for assemble_records."""
    what = "assemble_kitti_records"
    rows, max_hw, total = assemble_kitti_records_table(records, out_hw, cc_th)
    ragged = isinstance(records, MultiHRecordsRagged)
    cc_th = float(cc_th)
    B, dev, max_h = records.B, records.rec.device, records.max_h
    plan = _kitti_plan(rows, max_h, cc_th, ws_bytes)
    if total > 0x7fffffff:
        raise ValueError("%s: the batch has more than 2^31 - 1 output pixels" % what)
    if out is not None:
        fg, mg, binary = out
        for t, shape, dts, name in ((fg, (total, 2), (torch.float32,), "flow"), (mg, (total,), (torch.float32,), "match"),
                                    (binary, (total,), (torch.bool,), "binary")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype not in dts or not t.is_contiguous() or t.device != dev:
                raise ValueError("%s: out %s must be a contiguous %s %s tensor on %s" % (what, name, shape, dts[0], dev))
        if fg.data_ptr() % 8:
            raise ValueError("%s: the flow output is accessed as float2 and must be 8-byte aligned" % what)
    rec = _dev(records.rec, "records")
    if out is None:
        fg = torch.empty((total, 2), dtype=torch.float32, device=dev)
        mg = torch.empty(total, dtype=torch.float32, device=dev)
        binary = torch.empty(total, dtype=torch.bool, device=dev)
    hws = [r[7] * r[8] for r in rows]
    host = [v for r in rows for v in r]
    if cc_th > 0:                                            # the filter's match_off: the map's offset inside its chunk's score buffer
        for lo, hi in plan:
            host += [rows[b][10] - rows[lo][10] + i * hws[b] for b in range(lo, hi) for i in range(max_h)]
    up = torch.tensor(host, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    table, moff = up[:B * KITTI_TABLE_COLS].view(B, KITTI_TABLE_COLS), up[B * KITTI_TABLE_COLS:]
    scores = ws = dims = None
    if cc_th > 0:
        cap = max(max_h * sum(hws[lo:hi]) for lo, hi in plan)
        scores = torch.empty(cap, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.load().rfx_remove_small_cc_ragged_ws_bytes(cap), dtype=torch.uint8, device=dev)
        dims = torch.empty((max(hi - lo for lo, hi in plan) * max_h, 3), dtype=torch.int32, device=dev)
    one = _one_device(rec, fg, mg, binary)
    head = (_p(rec), rec.numel(), records.width, max_h, records.off_H, records.off_flow)
    for lo, hi in plan:
        Bc, mhw, base, elems = hi - lo, max(hws[lo:hi]), rows[lo][10], max_h * sum(hws[lo:hi])
        if cc_th > 0:
            _call("rfx_kitti_scores_records_f32", one, *head, _p(table[lo:hi]), Bc, mhw, 1 if multiH else 0, _p(scores), base, elems,
                  _p(dims), total)
            _call("rfx_remove_small_cc_ragged_f32", one, _p(scores), _p(scores), _p(moff[lo * max_h:hi * max_h]), _p(dims), Bc * max_h,
                  elems, mhw, 0.99, _p(ws))
        _call("rfx_assemble_kitti_records_f32", one, *head, _p(table[lo:hi]), Bc, mhw, float(th), 1 if multiH else 0, _p(scores), base,
              elems, _p(fg), _p(mg), _p(binary), total)
    valid = rec[:, 0] >= 1                                    # the kernel's own test of nbH
    if interpolate:
        # runs of consecutive pairs of one size: a pair without explained pixel (nbH == 0 among them) takes its pixel (H-1, 0), zero
        b = 0
        while b < B:
            e = b + 1
            while e < B and rows[e][7:9] == rows[b][7:9]:
                e += 1
            (H, W), o, n = rows[b][7:9], rows[b][9], (e - b) * hws[b]
            filled = nearest_fill(fg[o:o + n].view(e - b, H, W, 2), binary[o:o + n].view(e - b, H, W))
            if out is None and e - b == B:
                fg = filled.view(total, 2)
            else:
                fg[o:o + n].copy_(filled.view(n, 2))
            b = e
    if not ragged:
        H, W = rows[0][7:9]
        return fg.view(B, H, W, 2), mg.view(B, H, W), binary.view(B, H, W), valid
    views = [(r[9], r[7], r[8]) for r in rows]
    return ([fg[o:o + H * W].view(H, W, 2) for o, H, W in views], [mg[o:o + H * W].view(H, W) for o, H, W in views],
            [binary[o:o + H * W].view(H, W) for o, H, W in views], valid)


def multih_accept(match, mask, bg, active, ransac_result, n_match, nbH, th, mode, bestH=None, flowDown8=None, match12Down8=None,
                  match21Down8=None, flowD2=None, records=None):
    """Accept rule + mask update + record store of one round (rfx_multih_accept_f32) -> (accept (a,) int32, gain (a,) f32),
    both on the device; ``mask`` (B,h,w) and ``nbH`` (B,) int32 are updated in place."""
    for t, name in ((mask, "mask"), (nbH, "nbH")):          # updated IN PLACE: a silent .contiguous() copy would lose the update
        if isinstance(t, torch.Tensor) and not t.is_contiguous():
            raise ValueError("%s must be contiguous (updated in place)" % name)
    match, mask = _dev(match, "match"), _dev(mask, "mask")
    bg = _dev(bg, "bg") if bg is not None else None
    act = _dev(active, "active", torch.int32) if active is not None else None
    res, n_match, nbH = _dev(ransac_result, "ransac result", torch.int32), _dev(n_match, "n", torch.int32), _dev(nbH, "nbH", torch.int32)
    a = match.shape[0]
    h, w = mask.shape[1], mask.shape[2]
    if match.numel() != a * h * w:
        raise ValueError("match must be (a,h,w) / (a,1,h,w) at the mask's resolution")
    dev = match.device
    accept = torch.empty(a, dtype=torch.int32, device=dev)
    gain = torch.empty(a, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.rfx_multih_accept_ws_bytes(a), dtype=torch.uint8, device=dev)
    h8 = w8 = hd2 = wd2 = 0
    f8 = m12 = m21 = fd2 = None
    if flowDown8 is not None:
        f8 = _dev(flowDown8, "flowDown8")
        h8, w8 = f8.shape[2], f8.shape[3]
        m12, m21 = _dev(match12Down8, "match12Down8"), _dev(match21Down8, "match21Down8")
    if flowD2 is not None:
        fd2 = _dev(flowD2, "flowD2")
        hd2, wd2 = fd2.shape[2], fd2.shape[3]
    R = records
    if R is not None and (R.h8, R.w8, R.hd2, R.wd2) != (h8, w8, hd2, wd2):
        raise ValueError("record layout does not match the round's tensors")
    bh = _dev(bestH, "bestH") if bestH is not None else None
    _call("rfx_multih_accept_f32", _one_device(match, mask, bg, act, res, n_match, nbH, bh, f8, m12, m21, fd2), _p(match), _p(mask), _p(bg),
          _p(act), a, h, w, _p(res), _p(n_match), _p(nbH), float(th), int(mode), _p(accept), _p(gain), _p(ws), _p(bh), _p(f8), _p(m12),
          _p(m21), h8, w8, _p(fd2), hd2, wd2, _p(R.rec) if R is not None else ctypes.c_void_p(0), R.width if R is not None else 0,
          R.max_h if R is not None else 0, R.off_H if R is not None else 0, R.off_flow if R is not None else 0,
          R.off_match if R is not None else 0, R.off_d2 if R is not None else 0)
    return accept, gain


def multih_accept_ragged(match, match_off, mask, bg, moff, geom, active, ransac_result, n_match, nbH, th, mode, max_hw, bestH=None,
                         flowDown8=None, match12Down8=None, match21Down8=None, off8=None, records=None, flowD2=None, offd2=None,
                         d2dims=None):
    """multih_accept for active pairs of DIFFERENT sizes (rfx_multih_accept_ragged_f32) -> (accept (a,) int32, gain (a,) f32).
    ``mask`` / ``bg``: packed 1-D buffers, pair b at ``moff[b]``; ``geom`` (B,6) int32 (see filter_matches_ragged).  The round's
    tensors are packed per ACTIVE pair: ``match`` 1-D, pair k's h*w values at ``match_off[k]``; ``flowDown8`` 1-D, pair k at
    2 * off8[k]; ``match12Down8`` / ``match21Down8`` 1-D, pair k at off8[k] (match_off, off8: (a,) int64).  ``max_hw``: the largest
    h * w among the active pairs.  ``records``: a MultiHRecordsRagged.  ``mask`` and ``nbH`` (B,) int32 are updated in place.
    KITTI rounds (rfx_multih_accept_ragged_d2_f32): ``flowD2`` 1-D, pair k's (2,hd2,wd2) half-resolution /8 flow at 2 * offd2[k]
    ((a,) int64); the per-pair sizes are ``d2dims`` (B,2) int32 or, by default, the records' own (built with the d2 lists)."""
    for t, name in ((mask, "mask"), (nbH, "nbH")):          # updated IN PLACE: a silent .contiguous() copy would lose the update
        if isinstance(t, torch.Tensor) and not t.is_contiguous():
            raise ValueError("%s must be contiguous (updated in place)" % name)
    match, mask = _dev(match, "match"), _dev(mask, "mask")
    bg = _dev(bg, "bg") if bg is not None else None
    act = _dev(active, "active", torch.int32) if active is not None else None
    res, n_match, nbH = _dev(ransac_result, "ransac result", torch.int32), _dev(n_match, "n", torch.int32), _dev(nbH, "nbH", torch.int32)
    match_off, moff, geom = _dev(match_off, "match_off", torch.int64), _dev(moff, "moff", torch.int64), _dev(geom, "geom", torch.int32)
    a, B = match_off.numel(), moff.numel()
    if mask.dim() != 1 or match.dim() != 1 or (bg is not None and bg.shape != mask.shape):
        raise ValueError("match / mask / bg of a ragged batch are packed 1-D buffers")
    if geom.shape != (B, 6) or nbH.numel() != B or res.shape != (a, 4) or n_match.numel() != a or (act is None and a != B) or \
            (act is not None and act.numel() != a):
        raise ValueError("geom (B,6), nbH (B,), ransac result (a,4), n / match_off / active (a,) expected")
    dev = match.device
    accept = torch.empty(a, dtype=torch.int32, device=dev)
    gain = torch.empty(a, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.rfx_multih_accept_ragged_ws_bytes(a), dtype=torch.uint8, device=dev)
    f8 = m12 = m21 = o8 = None
    if flowDown8 is not None:
        f8, m12, m21 = _dev(flowDown8, "flowDown8"), _dev(match12Down8, "match12Down8"), _dev(match21Down8, "match21Down8")
        o8 = _dev(off8, "off8", torch.int64)
        if o8.numel() != a:
            raise ValueError("off8 must hold one offset per active pair")
    R = records
    if R is not None and (not isinstance(R, MultiHRecordsRagged) or R.B != B):
        raise ValueError("records of a ragged batch: a MultiHRecordsRagged with one row per pair")
    bh = _dev(bestH, "bestH") if bestH is not None else None
    rec_args = (_p(R.rec) if R is not None else ctypes.c_void_p(0), R.width if R is not None else 0, R.max_h if R is not None else 0,
                R.off_H if R is not None else 0, R.off_flow if R is not None else 0)
    if flowD2 is None:
        if R is not None and R.hd2 is not None:
            raise ValueError("records with a flowD2 part need the round's flowD2")
        _call("rfx_multih_accept_ragged_f32", _one_device(match, match_off, mask, bg, moff, geom, act, res, n_match, nbH, bh, f8, m12, m21, o8),
              _p(match), _p(match_off), _p(mask), _p(bg), _p(moff), _p(geom), _p(act), a, int(max_hw), _p(res), _p(n_match), _p(nbH),
              float(th), int(mode), _p(accept), _p(gain), _p(ws), _p(bh), _p(f8), _p(m12), _p(m21), _p(o8), *rec_args)
        return accept, gain
    fd2, od2 = _dev(flowD2, "flowD2"), _dev(offd2, "offd2", torch.int64)
    if R is not None and R.hd2 is None:
        raise ValueError("flowD2 needs records built with hd2_list / wd2_list")
    dd = _dev(d2dims if d2dims is not None else (R.d2dims if R is not None else None), "d2dims", torch.int32)
    if fd2.dim() != 1 or od2.numel() != a or dd.shape != (B, 2):
        raise ValueError("flowD2 packed 1-D, offd2 (a,), d2dims (B,2) expected")
    if R is not None and d2dims is not None and not torch.equal(dd, R.d2dims):
        raise ValueError("d2dims differ from the sizes the records were built with")
    _call("rfx_multih_accept_ragged_d2_f32", _one_device(match, match_off, mask, bg, moff, geom, act, res, n_match, nbH, bh, f8, m12, m21,
                                                          o8, fd2, od2, dd),
          _p(match), _p(match_off), _p(mask), _p(bg), _p(moff), _p(geom), _p(act), a, int(max_hw), _p(res), _p(n_match), _p(nbH),
          float(th), int(mode), _p(accept), _p(gain), _p(ws), _p(bh), _p(f8), _p(m12), _p(m21), _p(o8), _p(fd2), _p(od2), _p(dd), *rec_args)
    return accept, gain
