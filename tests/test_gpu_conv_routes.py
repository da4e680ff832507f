"""What every ConvPlan route, the fused Bottleneck tail and the two stems append to ops.Profiler.conv -- the tuples bench.py's roofline
figures are decoded from -- at one smallest shape per recording launch, against literals."""
import pytest
import torch

from rfx import ops, _lib

pytestmark = pytest.mark.gpu

RELU = ops.ACT_RELU


def _bn(c, g):
    return dict(weight=torch.rand(c, generator=g) + 0.5, bias=torch.randn(c, generator=g) * 0.1, running_mean=torch.randn(c, generator=g) * 0.1,
                running_var=torch.rand(c, generator=g) + 0.5)


def test_profiler_records_of_every_route(dev, monkeypatch):
    """(kid, flops, shape, bytes) of each record; the split kernels' ids are ops.KID_SPLIT_* | 1 (64-channel tiles) / 2 (128) | 4
    (strided), the stems' 256 / 257, the fp32 kernels' the library's own *_kernel_id for the launch's shape.  The split 3x3 record
    of the 49-channel input carries the unpadded C = 49.  The dilated route records nothing."""
    monkeypatch.delenv("RFX_CONV_SPLIT", raising=False)
    lib = _lib.load()
    g = torch.Generator().manual_seed(11)

    def plan(Cin, Cout, k, stride=1, split=False, dilation=1, bn=True):
        w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
        return ops.ConvPlan(w, _bn(Cout, g) if bn else None, stride, (k // 2) * dilation, RELU, dev, dilation=dilation, split=split)

    def x(C, H, W):
        return torch.randn(1, C, H, W, generator=g).to(dev)

    S3, S1 = ops.KID_SPLIT_3X3, ops.KID_SPLIT_1X1
    # (route, plan, input, kid, flops, shape, bytes)
    convs = [
        ("split3x3", plan(16, 128, 3, split=True), x(16, 9, 17), S3 | 2, 5640192.0, (1, 16, 9, 17, 128, 3, 1), 198720.0),
        ("split3x3", plan(16, 64, 3, split=True), x(16, 9, 17), S3 | 1, 2820096.0, (1, 16, 9, 17, 64, 3, 1), 104256.0),
        ("split3x3", plan(49, 128, 3, split=True), x(49, 9, 17), S3 | 2, 17273088.0, (1, 49, 9, 17, 128, 3, 1), 447012.0),
        ("split3x3_s2", plan(16, 128, 3, 2, split=True), x(16, 9, 17), S3 | 2 | 4, 1658880.0, (1, 16, 9, 17, 128, 3, 2), 143424.0),
        ("split1x1", plan(32, 128, 1, split=True), x(32, 5, 7), S1 | 2, 286720.0, (1, 32, 5, 7, 128, 1, 1), 46976.0),
        ("split1x1", plan(32, 128, 1, 2, split=True), x(32, 5, 7), S1 | 2 | 4, 98304.0, (1, 32, 5, 7, 128, 1, 2), 32256.0),
        ("fp32_3x3", plan(8, 64, 3), x(8, 9, 17), lib.rfx_conv3x3_kernel_id(1, 8, 64, 9, 17, 0), 1410048.0, (1, 8, 9, 17, 64, 3, 1), 62496.0),
        # 16x32 -> 8x16: one full patch of the direct stride-2 kernel (at 9x17 the library's rule hands the launch to the implicit GEMM)
        ("fp32_3x3", plan(8, 64, 3, 2), x(8, 16, 32), lib.rfx_conv2d_kernel_id(1, 8, 64, 3, 3, 2, 1, 8, 16), 1179648.0, (1, 8, 16, 32, 64, 3, 2),
         67584.0),
        ("gemm", plan(64, 64, 1), x(64, 5, 8), lib.rfx_conv2d_kernel_id(1, 64, 64, 1, 1, 1, 0, 5, 8), 327680.0, (1, 64, 5, 8, 64, 1, 1), 36864.0),
        ("gemm", plan(8, 64, 1), x(8, 5, 8), lib.rfx_conv2d_kernel_id(1, 8, 64, 1, 1, 1, 0, 5, 8), 40960.0, (1, 8, 5, 8, 64, 1, 1), 13568.0),
    ]
    assert convs[6][3] & 32 and convs[7][3] & 8192            # the direct 3x3 kernels themselves, not their fall-back
    assert not convs[8][3] & (32 | 8192) and not convs[9][3] & (32 | 8192)
    p2, p3, xt = plan(8, 64, 3), plan(64, 128, 1), x(8, 9, 17)
    assert ops.bottleneck_tail_eligible(p2, p3)
    stem3, stem7, img = plan(3, 64, 3), plan(3, 64, 7, 2), x(3, 18, 20)
    dil, xd = plan(8, 64, 3, dilation=2), x(8, 9, 17)
    assert dil.route == "dilated"
    others = [
        (lambda: ops.bottleneck_tail(xt, p2, p3), lib.rfx_conv3x3_conv1x1_kernel_id(1, 9, 17, 64), 3916800.0, (1, 8, 9, 17, 128, 3, 1), 83232.0),
        (lambda: ops.stem_conv_maxblur(img, stem3), 256, 1244160.0, (1, 3, 18, 20, 64, 3, 1), 27360.0),
        (lambda: ops.stem_conv7_maxpool(img, stem7), 257, 1693440.0, (1, 3, 18, 20, 64, 7, 2), 10720.0),
    ]
    plain = [p(xin) for _, p, xin, *_ in convs] + [run() for run, *_ in others]
    with ops.Profiler() as prof:
        outs = []
        for route, p, xin, *_ in convs:
            assert p.route == route
            outs.append(p(xin))
            assert len(prof.conv) == len(outs)
        for run, *_ in others:
            outs.append(run())
            assert len(prof.conv) == len(outs)
        dil(xd)
        assert len(prof.conv) == len(outs)                    # the dilated route appends nothing
    torch.cuda.synchronize()
    want = [c[3:] for c in convs] + [o[1:] for o in others]
    for rec, (kid, flops, shape, nbytes), a, b in zip(prof.conv, want, outs, plain):
        assert len(rec) == 6 and (rec[0], rec[1], rec[4], rec[5]) == (kid, flops, shape, nbytes)
        assert type(rec[1]) is float and type(rec[5]) is float
        assert rec[2].elapsed_time(rec[3]) >= 0.0             # a recorded event pair on the launch stream
        assert torch.equal(a, b)                              # the profiled launch is the launch
