#!/usr/bin/env python
"""The KITTI nearest-explained-pixel fill at evaluation size (375 x 1242 x 2), device against host, in ONE process:

    device: ops.nearest_fill = rfx_nearest_fill_f32, HIP events around the launches of INNER consecutive calls, time per call
            (and around one call alone: its two launches)
    host:   assemble.interpolate_flow_match(fill="host") end to end as assemble_kitti pays it -- D2H of flow and mask, scipy's
            distance_transform_edt(return_indices=True), the numpy gather, H2D, and a synchronise -- wall clock after a synchronise

on masks with about 0.1 %, 10 % and 70 % explained pixels and on one shaped like a real KITTI result (one large matched region with
holes, plus islands).  The two paths alternate, REPS repetitions each; min / median / max of both are recorded, and that both
return the same tensor.  -> profiles/nearest_fill_bench.json

    python scripts/ubench/nearest_fill_bench.py [--out profiles/nearest_fill_bench.json] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from rfx import assemble, ops  # noqa: E402

H, W, INNER = 375, 1242, 20


def kitti_like(g):
    """Smoothed noise cut twice: a large connected region with holes, and small islands elsewhere."""
    k = 41
    ax = torch.arange(k) - k // 2
    ker = torch.exp(-ax.float() ** 2 / (2 * 9.0 ** 2))
    ker = (ker[:, None] * ker[None, :]) / ker.sum() ** 2
    sm = F.conv2d(torch.randn(1, 1, H, W, generator=g), ker[None, None], padding=k // 2)[0, 0]
    sm = sm / sm.std()
    ramp = torch.linspace(1.5, -1.5, H)[:, None]                   # the road half of a KITTI frame is matched, the sky is not
    return (sm - ramp > 0.3) | (sm > 2.2)


def stats(xs):
    return dict(min=min(xs), median=statistics.median(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_fill_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    masks = {"0.1%": torch.rand(H, W, generator=g) < 0.001, "10%": torch.rand(H, W, generator=g) < 0.1,
             "70%": torch.rand(H, W, generator=g) < 0.7, "kitti-like": kitti_like(g)}
    flow = (torch.rand(1, H, W, 2, generator=g) * 2 - 1).to(dev)
    rec = dict(what="nearest-explained-pixel fill of one %d x %d x 2 flow: device (rfx_nearest_fill_f32, HIP events around %d "
                    "consecutive calls, per call) against the host path of the parent commit (D2H, scipy distance_transform_edt, "
                    "numpy gather, H2D, synchronise; wall clock), alternating in one process, %d repetitions each; milliseconds"
                    % (H, W, INNER, a.reps),
               device=torch.cuda.get_device_name(0), reps=a.reps, masks={})
    for name, m in masks.items():
        b = m[None].to(dev)
        same = torch.equal(assemble.interpolate_flow_match(flow, b, "device"), assemble.interpolate_flow_match(flow, b, "host"))
        for _ in range(3):
            ops.nearest_fill(flow, b)
        torch.cuda.synchronize()
        dev_ms, one_ms, host_ms = [], [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                ops.nearest_fill(flow, b)
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1) / INNER)
            e0.record()
            ops.nearest_fill(flow, b)                                # one call alone: the events bracket its two launches
            e1.record()
            torch.cuda.synchronize()
            one_ms.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            assemble.interpolate_flow_match(flow, b, "host")
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        rec["masks"][name] = dict(explained=float(m.float().mean()), same_tensor=same, device_ms=stats(dev_ms), device_single_call_ms=stats(one_ms), host_ms=stats(host_ms),
                                  host_over_device_median=statistics.median(host_ms) / statistics.median(dev_ms))
        print(name, json.dumps(rec["masks"][name]))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
