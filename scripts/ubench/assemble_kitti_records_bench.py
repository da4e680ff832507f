#!/usr/bin/env python
"""Dense KITTI flows of a batch of pairs from their device records, in ONE process:

    (a) chain:   per pair, the read of nbH (one host sync: the record lives on the device) and assemble.assemble_kitti(...,
                 fill="device") on the record's first nbH entries -- warp_grid, two compose_flow, resize_bilinear, grid_sample,
                 [match_score, the four-kernel component filter,] merge_multi_h[, nearest_fill], with their (n,H,W) intermediates
    (b) records: one ops.assemble_kitti_records call on the whole batch (rfx_assemble_kitti_records_f32; with cc_th > 0 also
                 rfx_kitti_scores_records_f32 and the ragged component filter; no sync)

10 pairs over the five KITTI frame sizes (two of each), outputs at the frame size, records at the /8 sizes of fineSize = 650 and its
half (outil.resizeImg's rounding), nbH drawn from 1..11, multiH on.  Record contents: synth.assembly_arrays (flows and homographies
near the identity, smooth matchability clipped at 1) with a half-resolution flow of the record's own size.  th: the script's default
1.0 (evaluation/evalKITTI/getResults.py:169), 0.5, and 2.0, which no score reaches -- every pixel then walks all nbH homographies of
its pair, the fused kernel's worst case; cc_th 0 and the script's 0.01; with and without --interpolate.  Wall clock around INNER
consecutive runs between two synchronisations, per run; the two paths alternating, REPS repetitions each: median (min - max),
milliseconds.  Peak allocation of each path above what is allocated before it (the records), in MiB.  The results of both paths are
compared bit for bit.  -> profiles/assemble_kitti_records_bench.json

    python scripts/ubench/assemble_kitti_records_bench.py [--out profiles/assemble_kitti_records_bench.json] [--reps 5]
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
from rfx import assemble, ops, synth  # noqa: E402
from rfx.pipeline import AlignPipeline  # noqa: E402

KITTI_SIZES = [(375, 1242), (376, 1241), (374, 1238), (370, 1226), (370, 1224)]          # (H, W)
MAX_H, INNER, FINE = 11, 5, 650


def records(sizes, nb, dev):
    s8 = [AlignPipeline.resize_img_dims(W, H, 8, FINE) for H, W in sizes]                # (w, h) of the fine pass
    s2 = [AlignPipeline.resize_img_dims(W, H, 8, FINE // 2) for H, W in sizes]           # ... and of the half-resolution pass
    R = ops.MultiHRecordsRagged([h // 8 for _, h in s8], [w // 8 for w, _ in s8], dev, max_h=MAX_H,
                                hd2_list=[h // 8 for _, h in s2], wd2_list=[w // 8 for w, _ in s2])
    for b, n in enumerate(nb):
        nbH, _, Hs, f8, m8, d2 = R.views(b)
        fd, _, pm, md = synth.assembly_arrays(100 + b, n, R.h8[b], R.w8[b])
        f8[:n], Hs[:n], m8[:n] = (torch.from_numpy(np.ascontiguousarray(a)).float().to(dev) for a in (fd, pm, md))
        d2[:n] = (torch.randn(n, 2, R.hd2[b], R.wd2[b], generator=torch.Generator().manual_seed(200 + b)) * 0.05).to(dev)
        nbH.fill_(float(n))
    return R


def chain(R, sizes, th, cc_th, interpolate, dev):
    out = []
    for b in range(R.B):
        nbH, _, Hs, f8, m8, d2 = R.views(b)
        n = int(nbH)                                                  # the sync the per-pair path needs
        out.append(assemble.assemble_kitti(d2[:n], f8[:n], Hs[:n], m8[:n], sizes[b], th, True, cc_th, interpolate, dev, fill="device"))
    return out


def wall(fn):
    """Milliseconds per run of INNER consecutive runs between two synchronisations."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / INNER


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_kitti_records_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [s for s in KITTI_SIZES for _ in range(2)]
    B = len(sizes)
    nb = [int(x) for x in np.random.RandomState(7).randint(1, MAX_H + 1, B)]
    R = records(sizes, nb, dev)
    rec = dict(what="dense KITTI flows of %d pairs (outputs %s) from their device records (/8 sizes %s, half-resolution %s, nbH = %s, "
                    "multiH on): (a) per pair the read of nbH and assemble.assemble_kitti(fill='device'), (b) one "
                    "ops.assemble_kitti_records call; wall clock around %d consecutive runs between synchronisations, per run, alternating "
                    "in one process, %d repetitions each, milliseconds; peak allocation above the records, MiB"
                    % (B, sizes, list(zip(R.h8, R.w8)), list(zip(R.hd2, R.wd2)), nb, INNER, a.reps),
               device=torch.cuda.get_device_name(0), reps=a.reps, cases={})
    for cc_th in (0.0, 0.01):
        rec["chunks cc_th %g" % cc_th] = ops.assemble_kitti_records_plan(R, sizes, cc_th)
        for interpolate in (False, True):
            for th in (1.0, 0.5, 2.0):
                run_a = lambda: chain(R, sizes, th, cc_th, interpolate, dev)
                run_b = lambda: ops.assemble_kitti_records(R, th, True, cc_th=cc_th, interpolate=interpolate, out_hw=sizes)
                want, got = run_a(), run_b()                           # warm, and the same bits
                same = all(torch.equal(w[0][0].view(torch.int32), got[0][b].view(torch.int32)) and
                           torch.equal(w[1][0].view(torch.int32), got[1][b].view(torch.int32)) and torch.equal(w[2][0], got[2][b])
                           for b, w in enumerate(want))
                explained = float(torch.cat([t.reshape(-1) for t in got[2]]).float().mean())
                del want, got
                ta, tb = [], []
                for _ in range(a.reps):
                    ta.append(wall(run_a))
                    tb.append(wall(run_b))
                case = dict(pairs=B, th=th, cc_th=cc_th, interpolate=interpolate, bit_equal=same, explained=explained,
                            chain_ms=stats(ta), records_ms=stats(tb), chain_over_records_median=statistics.median(ta) / statistics.median(tb),
                            records_slowest_below_chain_fastest=max(tb) < min(ta),
                            chain_peak_mib=peak_mib(run_a), records_peak_mib=peak_mib(run_b))
                rec["cases"]["cc_th %g, interpolate %s, th %g" % (cc_th, "on" if interpolate else "off", th)] = case
                print(json.dumps(case), flush=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
