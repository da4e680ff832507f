#!/usr/bin/env python3
# Layer1's 64 -> 256 expansions, today's launches against csrc/conv1x1e.hip, on the seven pyramid levels of bench config 3
# (N = 64 per level) and the 480 x 640 target (N = 128):
#   dual:   shortcut launch + conv3 launch (rfx_conv2d_f32 twice, the 256-channel shortcut through memory)  |  rfx_conv1x1_expand64_dual_f32
#   plain:  conv3 + residual (rfx_conv2d_f32)                                                               |  rfx_conv1x1_expand64_f32
# Random data; the arms alternate inside every round, in one process; the first (clock-ramping) round is dropped; median and minimum
# over the rest.  Every new result is compared with the old one bit for bit before it is timed.
#   python scripts/ubench/expand64_bench.py [--rounds 9] [--batches 64,8,1] [--out profiles/expand64_ab.json]
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))

import torch  # noqa: E402

from rfx import ops  # noqa: E402
from rfx.pipeline import scale_list, resize_dims  # noqa: E402


def layer1_shapes(batch):
    """(N, H, W) of the trunk's layer1 maps at config 3 with ``batch`` pairs: conv1 / 2, max-pool / 2 of the resized inputs."""
    def quarter(v):
        return ((v - 1) // 2 + 1 - 1) // 2 + 1
    out = []
    for s in scale_list(7, 2.0):
        w, h = resize_dims(640, 480, int(480 * s), "min")
        out.append((batch, quarter(h), quarter(w)))
    w, h = resize_dims(640, 480, 480, "min")
    out.append((2 * batch, quarter(h), quarter(w)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batches", default="64", help="pairs per launch, comma separated (64: the bench; 8, 1: where the rule could turn)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    def bn(C):
        return dict(weight=torch.rand(C, generator=g) + 0.5, bias=torch.randn(C, generator=g) * 0.1,
                    running_mean=torch.randn(C, generator=g) * 0.1, running_var=torch.rand(C, generator=g) + 0.5)
    c3 = ops.ConvPlan(torch.randn(256, 64, 1, 1, generator=g) * 0.1, bn(256), 1, 0, ops.ACT_RELU, dev)
    ds = ops.ConvPlan(torch.randn(256, 64, 1, 1, generator=g) * 0.1, bn(256), 1, 0, ops.ACT_NONE, dev)
    ops._EXPAND64 = True
    ops.EXPAND64_MIN_PIXELS = {"plain": 0, "dual": 0}          # time the kernel at every size: the rule is what this run decides
    rows = []
    for (N, H, W) in [shp for b in a.batches.split(",") for shp in layer1_shapes(int(b))]:
        o = torch.randn(N, 64, H, W, device=dev)
        x = torch.randn(N, 64, H, W, device=dev)
        r = torch.randn(N, 256, H, W, device=dev)
        arms = {
            "dual_old": lambda: c3(o, residual=ds(x)),
            "dual_new": lambda: ops.conv1x1_expand64(o, c3, shortcut=(x, ds)),
            "plain_old": lambda: c3(o, residual=r),
            "plain_new": lambda: ops.conv1x1_expand64(o, c3, residual=r),
        }
        same = bool(torch.equal(arms["dual_old"](), arms["dual_new"]())) and bool(torch.equal(arms["plain_old"](), arms["plain_new"]()))
        ms = {k: [] for k in arms}
        for _ in range(a.rounds + 1):
            for k, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                y = fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
                del y
        row = {"N": N, "H": H, "W": W, "pixels": N * H * W, "bit_equal": same}
        for k, v in ms.items():
            v = v[1:]
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        for form in ("dual", "plain"):
            old, new = row[form + "_old"], row[form + "_new"]
            row[form + "_speedup_median"] = round(old["median_ms"] / new["median_ms"], 4)
            # the new kernel wins when its slowest run beats the old launches' fastest: beyond the old one's own spread
            row[form + "_wins"] = new["max_ms"] < old["min_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del o, x, r
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"bench": "scripts/ubench/expand64_bench.py", "rounds": a.rounds, "batches": a.batches, "device": torch.cuda.get_device_name(0),
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
