#!/usr/bin/env python
"""The YFCC point correspondences at evaluation size (480 x 720 x 2), device against host, in ONE process:

    device: ops.matches_from_flow = rfx_flow_points_f32 (three launches) plus the ONE read of the offsets that sizes the result --
            wall clock after a synchronise, the exactly-sized points left on the device; and ops.flow_points alone (no sync), HIP
            events around INNER consecutive calls, time per call
    host:   what a user pays without it -- D2H of flow and mask, the numpy boolean indexing of evaluation/evalYFCC/getResults.py:53-71
            (stated below), H2D of the points, and a synchronise -- wall clock after a synchronise

on one map with about 5 %, 50 % and 95 % explained pixels and on a batch of 16 maps at 50 % (the host path map by map, as the
script's function takes one map).  The two paths alternate, REPS repetitions each; min / median / max of both are recorded, and that
both return the same points.  -> profiles/points_bench.json

    python scripts/ubench/points_bench.py [--out profiles/points_bench.json] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rfx import ops  # noqa: E402

H, W, INNER = 480, 720, 20
SIZE_A, SIZE_B, ANGLE = (1024, 683), (W, H), 0


def host_points(flow, keep):
    """One (H,W,2) / (H,W) pair of host arrays -> (pts1, pts2) by numpy indexing."""
    gx, gy = np.meshgrid(np.arange(SIZE_B[0]), np.arange(SIZE_B[1]))
    pts2 = np.rot90(np.stack((gx, gy), axis=2), ANGLE // 90)[keep]
    pts1 = flow[keep]
    pts1[:, 0] = (pts1[:, 0] + 1) * (SIZE_A[0] - 1) / 2
    pts1[:, 1] = (pts1[:, 1] + 1) * (SIZE_A[1] - 1) / 2
    return pts1, pts2


def host_path(flow, keep):
    """Device maps (N,H,W,2) / (N,H,W) -> device points, through the host."""
    f, k = flow.cpu().numpy(), keep.cpu().numpy()
    parts = [host_points(f[n], k[n]) for n in range(len(f))]
    pts1 = torch.from_numpy(np.concatenate([p[0] for p in parts])).to(flow.device)
    pts2 = torch.from_numpy(np.concatenate([p[1] for p in parts])).to(flow.device)
    return pts1, pts2


def stats(xs):
    return dict(min=min(xs), median=statistics.median(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    cases = {"5%": (1, 0.05), "50%": (1, 0.5), "95%": (1, 0.95), "batch of 16, 50%": (16, 0.5)}
    rec = dict(what="point correspondences of N %d x %d x 2 flows: device (ops.matches_from_flow: rfx_flow_points_f32 and the one "
                    "read of the offsets, wall clock; ops.flow_points without a sync, HIP events around %d consecutive calls, per "
                    "call) against the host path (D2H of flow and mask, numpy boolean indexing, H2D of the points, synchronise; "
                    "wall clock), alternating in one process, %d repetitions each; milliseconds" % (H, W, INNER, a.reps),
               device=torch.cuda.get_device_name(0), reps=a.reps, cases={})
    for name, (N, p) in cases.items():
        keep = (torch.rand(N, H, W, generator=g) < p).to(dev)
        flow = (torch.rand(N, H, W, 2, generator=g) * 2 - 1).to(dev)
        d1, d2, _ = ops.matches_from_flow(flow, keep, SIZE_A, SIZE_B, ANGLE)
        h1, h2 = host_path(flow, keep)
        same = torch.equal(d1.view(torch.int32), h1.view(torch.int32)) and torch.equal(d2, h2)
        for _ in range(3):
            ops.flow_points(flow, keep, SIZE_A, SIZE_B, ANGLE)
        torch.cuda.synchronize()
        call_ms, launch_ms, host_ms = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ops.matches_from_flow(flow, keep, SIZE_A, SIZE_B, ANGLE)
            torch.cuda.synchronize()
            call_ms.append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                ops.flow_points(flow, keep, SIZE_A, SIZE_B, ANGLE)
            e1.record()
            torch.cuda.synchronize()
            launch_ms.append(e0.elapsed_time(e1) / INNER)
            t0 = time.perf_counter()
            host_path(flow, keep)
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        rec["cases"][name] = dict(maps=N, explained=float(keep.float().mean()), points=int(d1.shape[0]), same_points=same,
                                  device_call_ms=stats(call_ms), device_launches_ms=stats(launch_ms), host_ms=stats(host_ms),
                                  host_over_device_call_median=statistics.median(host_ms) / statistics.median(call_ms))
        print(name, json.dumps(rec["cases"][name]))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
