#!/usr/bin/env python
"""The end-point error of an assembled flow at evaluation size, device against host, in ONE process:

    HPatches, 240 x 240 (the script's minSize), 1 map and a batch of 16:
        device: assemble.hpatch_epe(flow_est, Hinv) = the upload of nine numbers per map, rfx_epe_homography_f32 (two launches), the
                read of one sum and one count per map -- wall clock to the Python float; and ops.epe_homography alone (no sync), HIP
                events around INNER consecutive calls, time per call
        host:   what a user pays without it -- D2H of the flow, then evaluation/evalHpatch/getResults.py:119-156,221-250 (stated
                below: the ground-truth map by a float64 product over all pixels, the mask, the un-normalisation, torch.norm, the
                mean), map by map as the script does -- wall clock after a synchronise
    KITTI, 375 x 1242:
        device: assemble.kitti_epe(flow, u, v, valid) with u, v (float64) and valid as readFlow returns them: the check that float32
                holds them, their upload, rfx_epe_flow_f32, the read of the sum and the count; the same with u, v, valid already on
                the device (ops.epe_flow and the read); and ops.epe_flow alone by HIP events
        host:   D2H of the flow, evaluation/evalKITTI/getResults.py:221-228 in torch / numpy (the linspace grid built once, outside
                the timing)

The paths alternate, REPS repetitions each; min / median / max are recorded, and how far the two results are apart.
-> profiles/epe_bench.json

    python scripts/ubench/epe_bench.py [--out profiles/epe_bench.json] [--reps 15]
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
from rfx import assemble, ops  # noqa: E402

INNER = 20


def host_hpatch(flow_dev, Hinv, S):
    """One (1,S,S,2) device flow -> the AEPE through the host: the ground-truth map as a float64 product over all pixels, rounded to
    float32 and normalised; the mask of its pixels inside [-1,1]^2; both maps in pixels; the mean length of the difference."""
    est = flow_dev.cpu()[0]
    jj, ii = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    w = np.dot(Hinv, np.stack([jj.ravel(), ii.ravel(), np.ones(S * S)]))
    x, y, z = (torch.from_numpy(w[r]).float() for r in range(3))
    gt = torch.stack([(2 * x / (z + 1e-8) / (S - 1) - 1).view(S, S), (2 * y / (z + 1e-8) / (S - 1) - 1).view(S, S)], dim=-1)
    keep = (gt[..., 0] >= -1) & (gt[..., 0] <= 1) & (gt[..., 1] >= -1) & (gt[..., 1] <= 1)
    gt, est = (gt + 1) * (S - 1) / 2, (est + 1) * (S - 1) / 2
    return torch.norm(gt[keep] - est[keep], p=2, dim=1).mean().item()


def host_kitti(flow_dev, grid_org, u, v, valid):
    """One (1,H,W,2) device flow -> the average error through the host: minus the grid (torch), to pixels in float32 (numpy), the
    float64 distance to (u, v), summed over valid."""
    rel = (flow_dev.cpu() - grid_org).numpy()[0]
    h, w = u.shape
    du, dv = rel[:, :, 0] * (w - 1) / 2 - u, rel[:, :, 1] * (h - 1) / 2 - v
    dist = (du ** 2 + dv ** 2) ** 0.5
    return float(np.sum(dist * valid) / np.sum(valid))


def stats(xs):
    return dict(min=min(xs), median=statistics.median(xs), max=max(xs))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / INNER


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epe_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(3)
    rec = dict(what="end-point error of assembled flows: device (assemble.hpatch_epe / kitti_epe: uploads, two launches, the read of "
                    "sum and count, wall clock to the Python float; ops.epe_* without a sync, HIP events around %d consecutive calls, "
                    "per call) against the host path (D2H of the flow, the results script's arithmetic, synchronise; wall clock), "
                    "alternating in one process, %d repetitions each; milliseconds" % (INNER, a.reps),
               device=torch.cuda.get_device_name(0), reps=a.reps, cases={})
    S = 240
    H = np.array([[0.92, 0.06, 40.0], [-0.04, 1.05, -25.0], [8e-5, -4e-5, 1.0]])
    Hinv = assemble.hpatch_gt_homography(H, (480, 640), (600, 800), S)[1]
    for N in (1, 16):
        grid = assemble.identity_grid(S, S, dev)
        flow = (grid + torch.from_numpy(rng.randn(N, S, S, 2).astype(np.float32) * 0.02).to(dev)).contiguous()
        hinv_n = np.repeat(Hinv[None], N, axis=0)
        hinv_dev = torch.from_numpy(hinv_n.reshape(N, 9)).to(dev)
        d = assemble.hpatch_epe(flow, hinv_n)
        h = [host_hpatch(flow[n:n + 1], Hinv, S) for n in range(N)]
        for _ in range(3):
            ops.epe_homography(flow, hinv_dev)
        call_ms, launch_ms, host_ms = [], [], []
        for _ in range(a.reps):
            call_ms.append(wall(lambda: assemble.hpatch_epe(flow, hinv_n))[0])
            launch_ms.append(events(lambda: ops.epe_homography(flow, hinv_dev)))
            host_ms.append(wall(lambda: [host_hpatch(flow[n:n + 1], Hinv, S) for n in range(N)])[0])
        name = "hpatches 240x240, %d map%s" % (N, "" if N == 1 else "s")
        rec["cases"][name] = dict(maps=N, aepe_device=d[0], aepe_host=h[0], max_abs_difference=max(abs(x - y) for x, y in zip(d, h)),
                                  device_call_ms=stats(call_ms), device_launches_ms=stats(launch_ms), host_ms=stats(host_ms),
                                  host_over_device_call_median=statistics.median(host_ms) / statistics.median(call_ms))
        print(name, json.dumps(rec["cases"][name]))
    Hk, Wk = 375, 1242
    grid = assemble.identity_grid(Hk, Wk, dev)
    grid_org = grid.cpu()
    flow = (grid + torch.from_numpy(rng.randn(1, Hk, Wk, 2).astype(np.float32) * 0.02).to(dev)).contiguous()
    u = (rng.randint(0, 65536, (Hk, Wk)).astype(float) - 32768) / 64.0 / 64
    v = (rng.randint(0, 65536, (Hk, Wk)).astype(float) - 32768) / 64.0 / 256
    valid = rng.rand(Hk, Wk) < 0.2                                    # KITTI's sparse ground truth
    ud, vd = (torch.from_numpy(x.astype(np.float32)[None]).to(dev) for x in (u, v))
    md = torch.from_numpy(valid[None]).to(dev)

    def resident():
        total, count = ops.epe_flow(flow, ud, vd, md)
        return float(total.cpu()[0]) / int(count.cpu()[0])
    d, h = assemble.kitti_epe(flow, u, v, valid), host_kitti(flow, grid_org, u, v, valid)
    for _ in range(3):
        ops.epe_flow(flow, ud, vd, md)
    call_ms, resident_ms, launch_ms, host_ms = [], [], [], []
    for _ in range(a.reps):
        call_ms.append(wall(lambda: assemble.kitti_epe(flow, u, v, valid))[0])
        resident_ms.append(wall(resident)[0])
        launch_ms.append(events(lambda: ops.epe_flow(flow, ud, vd, md)))
        host_ms.append(wall(lambda: host_kitti(flow, grid_org, u, v, valid))[0])
    name = "kitti 375x1242"
    rec["cases"][name] = dict(maps=1, valid=float(valid.mean()), epe_device=d, epe_host=h, relative_difference=abs(d - h) / h,
                              device_call_with_uploads_ms=stats(call_ms), device_call_ground_truth_resident_ms=stats(resident_ms),
                              device_launches_ms=stats(launch_ms), host_ms=stats(host_ms),
                              host_over_device_call_median=statistics.median(host_ms) / statistics.median(call_ms),
                              host_over_resident_call_median=statistics.median(host_ms) / statistics.median(resident_ms))
    print(name, json.dumps(rec["cases"][name]))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
