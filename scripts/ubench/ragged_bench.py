#!/usr/bin/env python
"""Ragged batch vs one pair at a time, on a fixed mixed-size set of synthetic pairs.

    timeout -k 10 900 python scripts/ubench/ragged_bench.py [--pairs 32] [--reps 3] [--out profiles/ragged_bench.json]

The set: rfx.synth.make_pair pairs over 480x640, 640x480, 512x384, 384x512, 600x800 and a few odd sizes (quick_start settings:
nbScale 7, minSize 480, 1000 hypotheses, device draws keyed by pair id).  Two legs, each timed as the median of --reps runs after one
warm-up run: "coarse" (features + mutual NN + RANSAC) and "coarse+fine" (+ the quick-start fine stage).  The loop leg is today's
path, align_prepared on each pair's own prepare() (pre-processing outside the timed region for both legs).  Writes the pairs/s of
both legs, their ratio and the number of trunk buckets per pyramid level of the ragged plan.
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

from rfx import synth, weights  # noqa: E402
from rfx.pipeline import AlignPipeline  # noqa: E402

SIZES = [(480, 640), (640, 480), (384, 512), (512, 384), (600, 800), (480, 640), (640, 480), (384, 512),
         (456, 608), (500, 700), (333, 517), (720, 540)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2))
    pipe = AlignPipeline(sds, nbScale=7, nbIter=1000, tolerance=0.05, minSize=480, scaleR=1.2, device=dev, degenerate="device")
    pairs = [synth.make_pair(*SIZES[b % len(SIZES)], seed=b) for b in range(a.pairs)]
    ids = list(range(a.pairs))
    rprep = pipe.prepare_ragged(pairs)
    preps = [pipe.prepare([p]) for p in pairs]
    plan = rprep["plan"]
    nS = plan["nS"]
    per_level = [len({plan["levels"][b][i] for b in range(a.pairs)}) for i in range(nS + 1)]

    def run_ragged(fine):
        return pipe.align_prepared(rprep, fine=fine, pair_ids=ids)

    def run_loop(fine):
        return [pipe.align_prepared(p, fine=fine, pair_ids=[b])[0] for b, p in enumerate(preps)]

    res = dict(pairs=a.pairs, sizes=sorted({tuple(s) for s in SIZES[:a.pairs]}), buckets=len(plan["buckets"]),
               distinct_shapes_per_level=per_level, images=a.pairs * (nS + 1), reps=a.reps)
    for leg, fine in (("coarse", False), ("coarse+fine", True)):
        for name, fn in (("ragged", run_ragged), ("loop", run_loop)):
            fn(fine)                                                   # warm-up (and the loop's graph captures at 2nd sight)
            fn(fine)
            torch.cuda.synchronize(dev)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = fn(fine)
                torch.cuda.synchronize(dev)
                ts.append(time.perf_counter() - t0)
            res["%s_%s_s" % (leg, name)] = statistics.median(ts)
            res["%s_%s_pairs_per_s" % (leg, name)] = a.pairs / statistics.median(ts)
            res["%s_%s_with_H" % (leg, name)] = sum(o["H"] is not None for o in out)
        res["%s_speedup_ragged_over_loop" % leg] = res["%s_loop_s" % leg] / res["%s_ragged_s" % leg]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
