#!/usr/bin/env python
"""The Corr results step (evaluation/evalCorr/getResults.py: getFlow, alignmentError per matchability threshold, the precision table)
of a mixed-size batch from its device records: the keypoint chain against today's path.

    timeout -k 10 600 python scripts/ubench/corr_keypoints_bench.py [--pairs 8] [--reps 5] [--inner 10]
                                                                    [--out profiles/corr_keypoints_bench.json]

The set: the 8-pair mixed-size set of ragged_variant_c_bench.py (rfx.synth.make_pair(homography=True) over the size list of
ragged_bench.py), ONE candidate per pair (the evalCorr-like use of multi_h_variant_c), want_records=True; the records are filled once,
outside the timed legs.  Keypoints: K random target pixels per pair (floats with fractions), the source keypoints near the estimate,
for K = 64, 1 000 and 5 000 and M = 1 and M = 3 matchability thresholds.
Leg "new":  assemble.corr_keypoints_records (two launches, two pinned uploads) then assemble.corr_precision (the one host read).
Leg "old":  assemble.assemble_records (the dense maps of every pair), then per pair and per threshold the script's mask and
            assemble.corr_alignment_error (upload, rfx_sample_points_f32, three copies back, numpy), summed on the host: syncs included.
Both legs end with the precision table on the host, and the tables must be equal.  A repetition is ``--inner`` calls of a leg between
two host clock reads, the second after a device synchronise; the legs alternate, --reps repetitions each after two warm-up calls;
per-call medians and min-max ranges are reported with each leg's peak device allocation, the shader clock before and after and the
host name.  ``win`` is claimed only where the new leg's slowest repetition is below the old leg's fastest.  The driver-to-table path
(driver call, chain, table) is timed once after one warm-up call.  No ratio is expected in advance."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rfx import assemble, ops, synth, weights  # noqa: E402
from rfx.pipeline import AlignPipeline  # noqa: E402
from ragged_bench import SIZES  # noqa: E402
from ragged_multih_bench import clocks  # noqa: E402
from ragged_variant_c_bench import peak_bytes  # noqa: E402

THS = {1: (0.0,), 3: (0.0, 0.5, 0.9)}
TH = 0.95                                                          # the script's --th


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per repetition")
    ap.add_argument("--keypoints", default="64,1000,5000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_keypoints_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    pipe = AlignPipeline(sds, nbScale=7, nbIter=10000, tolerance=0.05, minSize=480, scaleR=2.0, variant="C", device=dev)
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)
    pairs = [synth.make_pair(*SIZES[b % len(SIZES)], seed=b, homography=True) for b in range(a.pairs)]
    src, tgt = [up(p[0]) for p in pairs], [up(p[1]) for p in pairs]
    ids = list(range(a.pairs))
    grid = ops.pck_pixel_grid().reshape(1, -1)

    def driver():
        return pipe.multi_h_variant_c(src, [tgt], maxCoarse=10, maskRegionTh=0.01, pair_ids=ids, want_records=True, want_lists=False)

    clock0 = clocks()
    outs, R = driver()
    torch.cuda.synchronize(dev)
    nbH = [o["nbH"] for o in outs]
    fg, mg, _, _ = ops.assemble_records(R, TH, True, True)
    sizes = [tuple(m.shape) for m in mg]
    res = dict(pairs=a.pairs, reps=a.reps, inner=a.inner, nbH=nbH, map_sizes=sizes, size_src=[list(s) for s in R.size_src], th=TH,
               pixels=sum(h * w for h, w in sizes), max_h=R.max_h, host=socket.gethostname(), cases=[],
               settings="variant C, nbScale 7, minSize 480, scaleR 2, nbIter 10000, tolerance 0.05, maxCoarse 10, maskRegionTh 0.01, "
                        "one candidate per pair, device draws by pair id")
    rng = np.random.RandomState(0)

    def keypoints(K):
        XA, YA, XB, YB = [], [], [], []
        for b, (hB, wB) in enumerate(sizes):
            xb, yb = (rng.rand(K) * wB).astype(np.float32), (rng.rand(K) * hB).astype(np.float32)
            ex, ey, _ = ops.sample_points(fg[b], mg[b], xb, yb, R.size_src[b])
            XB.append(xb), YB.append(yb)
            XA.append((ex.cpu().numpy() + rng.randn(K) * 6).astype(np.float32))
            YA.append((ey.cpu().numpy() + rng.randn(K) * 6).astype(np.float32))
        return XA, YA, XB, YB

    def new_leg(kp, ths):
        counts, nb, _ = assemble.corr_keypoints_records(R, TH, True, *kp, matchability_ths=ths)
        return assemble.corr_precision(counts, nb)

    def old_leg(kp, ths):
        XA, YA, XB, YB = kp
        f, m, _, valid = assemble.assemble_records(R, TH, True, True)
        valid = valid.tolist()
        prec, tot = np.zeros((len(ths), grid.shape[1])), np.zeros(len(ths), np.int64)
        for b, (hB, wB) in enumerate(sizes):
            if not valid[b]:                                        # the script's ``continue`` branch
                tot += len(XA[b])
                continue
            wA, hA = R.size_src[b]
            inside = None
            for t, mt in enumerate(ths):
                if mt > 0:
                    if inside is None:
                        inside = ((f[b] >= -1) & (f[b] <= 1)).all(dim=2).float()
                    mask = (m[b] >= mt).float() * inside
                else:
                    mask = torch.ones_like(m[b])
                c, n = assemble.corr_alignment_error(wB, hB, wA, hA, XA[b], YA[b], XB[b], YB[b], f[b], mask, grid)
                prec[t] += c
                tot[t] += n
        with np.errstate(divide="ignore", invalid="ignore"):
            return prec / tot[:, None], tot

    for K in [int(k) for k in a.keypoints.split(",")]:
        kp = keypoints(K)
        for M, ths in sorted(THS.items()):
            legs = (("new", lambda: new_leg(kp, ths)), ("old", lambda: old_leg(kp, ths)))
            got = {}
            for name, fn in legs:
                fn()
                got[name] = fn()
            assert np.array_equal(got["new"][0], got["old"][0], equal_nan=True) and np.array_equal(got["new"][1], got["old"][1]), got
            rec = dict(K_per_pair=K, K_total=K * a.pairs, M=M, precision=got["new"][0].tolist(), total=got["new"][1].tolist())
            peak = {name: peak_bytes(fn, dev) for name, fn in legs}
            ms = {name: [] for name, _ in legs}
            for _ in range(a.reps):
                for name, fn in legs:                              # interleaved: drift hits both legs alike
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(a.inner):
                        fn()
                    torch.cuda.synchronize(dev)
                    ms[name].append((time.perf_counter() - t0) * 1e3 / a.inner)
            for name, _ in legs:
                rec[name] = dict(ms_per_call=[round(x, 4) for x in ms[name]], median_ms=round(statistics.median(ms[name]), 4),
                                 min_ms=round(min(ms[name]), 4), max_ms=round(max(ms[name]), 4), peak_bytes=peak[name])
            rec["old_over_new_medians"] = round(rec["old"]["median_ms"] / rec["new"]["median_ms"], 3)
            rec["win"] = rec["new"]["max_ms"] < rec["old"]["min_ms"]
            res["cases"].append(rec)
            print(json.dumps(rec), flush=True)

    # driver -> table, once (the driver is warm: it ran above)
    kp = keypoints(1000)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    outs, R2 = driver()
    counts, nb, _ = assemble.corr_keypoints_records(R2, TH, True, *kp, matchability_ths=THS[3])
    table = assemble.corr_precision(counts, nb)
    torch.cuda.synchronize(dev)
    res["driver_to_table_once"] = dict(ms=round((time.perf_counter() - t0) * 1e3, 2), K_per_pair=1000, M=3, total=table[1].tolist())
    res.update(sclk_before=clock0, sclk_after=clocks())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res["driver_to_table_once"]))


if __name__ == "__main__":
    main()
