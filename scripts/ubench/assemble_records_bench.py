#!/usr/bin/env python
"""Dense flows of a batch of pairs from their device records, in ONE process:

    (a) chain:   per pair, the read of nbH (one host sync: the record lives on the device) and assemble.assemble on the record's
                 first nbH entries -- warp_grid, compose_flow, resize_bilinear, [grid_sample,] merge_multi_h, with their (n,H,W)
                 intermediates
    (b) records: one ops.assemble_records call on the whole batch (rfx_assemble_records_f32: one launch, no sync)

16 pairs, nbH drawn from 1..11, multiH on; 60 x 80 records at 480 x 640 and 30 x 30 records at the HPatches size 240 x 240, with the
cycle check on and off.  Record contents: synth.assembly_arrays (flows and homographies near the identity, smooth matchability); at
the scripts' thresholds (0.2 with the cycle check, 0.45 without) homography 0 owns nearly every pixel, which is the fused kernel's
best case (it stops at the owner), so each case is also run with th = 2, which no score reaches: every pixel then walks all nbH
homographies of its pair.  Wall clock around INNER consecutive runs between two synchronisations, per run; the two paths
alternating, REPS repetitions each: median (min - max), milliseconds.  Peak allocation of each path above what is allocated before
it (the records), in MiB.  The results of both paths are compared bit for bit.  -> profiles/assemble_records_bench.json

    python scripts/ubench/assemble_records_bench.py [--out profiles/assemble_records_bench.json] [--reps 5]
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

B, MAX_H, INNER = 16, 11, 10


def records(h8, w8, nb, dev):
    R = ops.MultiHRecords(B, h8, w8, dev, max_h=MAX_H)
    nbH, _, Hs, f8, m8, _ = R.views()
    for b, n in enumerate(nb):
        fd, _, pm, md = synth.assembly_arrays(100 + b, n, h8, w8)
        f8[b, :n], Hs[b, :n], m8[b, :n] = (torch.from_numpy(np.ascontiguousarray(a)).float().to(dev) for a in (fd, pm, md))
        nbH[b] = float(n)
    return R


def chain(R, out_hw, th, cycle, dev):
    nbH, _, Hs, f8, m8, _ = R.views()
    out = []
    for b in range(R.B):
        n = int(nbH[b])                                               # the sync the per-pair path needs
        out.append(assemble.assemble(f8[b, :n], Hs[b, :n], m8[b, :n], out_hw, th, True, cycle, dev))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_records_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nb = [int(x) for x in np.random.RandomState(7).randint(1, MAX_H + 1, B)]
    rec = dict(what="dense flows of %d pairs from their device records (nbH = %s, multiH on): (a) per pair the read of nbH and "
                    "assemble.assemble, (b) one ops.assemble_records call; wall clock around %d consecutive runs between synchronisations, per run, "
                    "alternating in one process, %d repetitions each, milliseconds; peak allocation above the records, MiB" % (B, nb, INNER, a.reps),
               device=torch.cuda.get_device_name(0), reps=a.reps, cases={})
    for name, h8, w8, out_hw in (("480x640", 60, 80, (480, 640)), ("hpatches 240x240", 30, 30, (240, 240))):
        R = records(h8, w8, nb, dev)
        for cycle, th in ((True, 0.2), (False, 0.45), (True, 2.0), (False, 2.0)):
            run_a = lambda: chain(R, out_hw, th, cycle, dev)
            run_b = lambda: ops.assemble_records(R, th, True, cycle, out_hw=out_hw)
            want, got = run_a(), run_b()                               # warm, and the same bits
            same = all(torch.equal(w[0][0].view(torch.int32), got[0][b].view(torch.int32)) and
                       torch.equal(w[1][0].view(torch.int32), got[1][b].view(torch.int32)) and torch.equal(w[2][0], got[2][b])
                       for b, w in enumerate(want))
            explained = float(got[2].float().mean())
            owned0 = float(ops.assemble_records(R, th, False, cycle, out_hw=out_hw)[2].float().mean())
            del want, got
            ta, tb = [], []
            for _ in range(a.reps):
                ta.append(wall(run_a))
                tb.append(wall(run_b))
            case = dict(pairs=B, records_hw=(h8, w8), out_hw=out_hw, cycle=cycle, th=th, bit_equal=same, explained=explained,
                        owned_by_0=owned0,
                        chain_ms=stats(ta), records_ms=stats(tb), chain_over_records_median=statistics.median(ta) / statistics.median(tb),
                        records_slowest_below_chain_fastest=max(tb) < min(ta),
                        chain_peak_mib=peak_mib(run_a), records_peak_mib=peak_mib(run_b))
            rec["cases"]["%s, cycle %s, th %g" % (name, "on" if cycle else "off", th)] = case
            print(name, cycle, json.dumps(case))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
