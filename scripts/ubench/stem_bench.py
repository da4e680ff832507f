#!/usr/bin/env python
"""Micro-benchmark of the two fused stem kernels on the config-3 shapes: stem7 at 64 images per pyramid level and 128 x 480x640,
the 3x3 stem at 64 / 56 / 8 x 480x640.  One or several builds of the library ("arms") are loaded side by side and timed ALTERNATING
in one process: per shape ``--rounds`` rounds, in each round every arm runs ``--iters`` back-to-back launches between one HIP
event pair; the first round is dropped, medians and min-max per arm are reported.  Every arm is checked bit for bit against the
un-fused convolution + pooling ops of the default library.
    python scripts/ubench/stem_bench.py [--arm parent=/path/librfx_parent.so --arm new=ransac-flow_amd/librfx.so] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))
import torch  # noqa: E402
from rfx import _lib, ops, weights  # noqa: E402
from rfx.ops import ConvPlan, ACT_RELU  # noqa: E402

STEM7 = [(64, 960, 1280), (64, 800, 1056), (64, 640, 848), (64, 480, 640), (64, 400, 528), (64, 320, 416), (64, 240, 320), (128, 480, 640)]
STEM3 = [(64, 480, 640), (56, 480, 640), (8, 480, 640)]


def load_arm(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("rfx_stem_conv7x7_maxpool_f32", "rfx_stem_conv3x3_maxblur_f32"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def launcher(lib, kernel, x, plan, out):
    fn = lib.rfx_stem_conv7x7_maxpool_f32 if kernel == "stem7" else lib.rfx_stem_conv3x3_maxblur_f32
    N, _, H, W = x.shape
    args = (x.data_ptr(), plan.wT.data_ptr(), plan.scale.data_ptr(), plan.shift.data_ptr(), out.data_ptr(), N, H, W, plan.Cout,
            torch.cuda.current_stream().cuda_stream)

    def run():
        rc = fn(*args)
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (kernel, rc))
    return run


def timed(run, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", action="append", default=[], metavar="NAME=LIB", help="a build of librfx.so to time (repeatable)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6, help="alternating rounds per shape; the first is dropped")
    ap.add_argument("--levers", default=None, help="free text for the output file: which levers the builds contain")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arms = [s.split("=", 1) for s in a.arm] or [["lib", _lib.LIB_PATH]]
    _lib.load()                                   # torch's HIP runtime first, then every build binds to the same one
    libs = {name: load_arm(path) for name, path in arms}
    dev = torch.device("cuda:0")
    sd = weights.resnet50_trunk_sd(0, randomize_bn=True)
    plan7 = ConvPlan(sd["conv1.weight"], {k: sd["bn1." + k] for k in ("weight", "bias", "running_mean", "running_var")}, 2, 3, ACT_RELU, dev)
    # the FeatureExtractor stem (conv3x3 3 -> 64 + BN + ReLU + MaxPool(2, 1) + BlurPool/2) on the fine-pass shapes of config 3
    sdf = weights.feature_extractor_sd(1, randomize_bn=True)
    plan3 = ConvPlan(sdf["conv1.weight"], {k: sdf["bn1." + k] for k in ("weight", "bias", "running_mean", "running_var")}, 1, 1, ACT_RELU, dev)
    rows = []
    for kernel, plan, shapes in (("stem7", plan7, STEM7), ("stem3", plan3, STEM3)):
        for (N, H, W) in shapes:
            g = torch.Generator(device=dev).manual_seed(H + N)
            x = torch.randn(N, 3, H, W, device=dev, generator=g)
            if kernel == "stem7":
                ref = ops.maxpool2d(plan(x[:2]), 3, 2, 1)
                Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                flop = 2.0 * N * Hc * Wc * 64 * 147
            else:
                ref = ops.maxblurpool2d(plan(x[:2]), 2)
                flop = 2.0 * N * H * W * 64 * 27
            out = torch.empty((N,) + tuple(ref.shape[1:]), device=dev)
            runs, same = {}, {}
            for name, lib in libs.items():
                out.zero_()
                launcher(lib, kernel, x[:2], plan, out)()
                torch.cuda.synchronize()
                same[name] = bool(torch.equal(out[:2], ref))
                runs[name] = launcher(lib, kernel, x, plan, out)
                for _ in range(3):
                    runs[name]()
            ms = {name: [] for name in libs}
            for r in range(a.rounds):
                for name in libs:
                    t = timed(runs[name], a.iters)
                    if r > 0:
                        ms[name].append(t)
            row = dict(kernel=kernel, N=N, H=H, W=W, arms={})
            for name in libs:
                med = statistics.median(ms[name])
                tf = flop / med / 1e9
                row["arms"][name] = dict(ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                                         tflops=round(tf, 1), frac_of_fp32_matrix_peak=round(tf / 157.3, 3), bit_identical=same[name])
            if len(arms) == 2:
                (p, _), (q, _) = arms
                row["speedup_%s_over_%s" % (q, p)] = round(row["arms"][p]["ms_median"] / row["arms"][q]["ms_median"], 3)
                row["beyond_spread"] = row["arms"][q]["ms_max"] < row["arms"][p]["ms_min"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = dict(what="scripts/ubench/stem_bench.py: arms alternating in one process, %d rounds of %d launches per shape, first round "
                        "dropped; ms per launch" % (a.rounds, a.iters),
                   arms={name: os.path.basename(path) for name, path in arms}, levers=a.levers, rows=rows)
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
