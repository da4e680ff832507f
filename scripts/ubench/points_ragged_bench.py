#!/usr/bin/env python
"""The YFCC path of a mixed-size batch after the driver: records -> flows -> correspondences, one chain against the per-pair loop.

    timeout -k 10 900 python scripts/ubench/points_ragged_bench.py [--pairs 8] [--reps 5] [--tag NAME]
                                                                   [--out profiles/points_ragged_bench.json]

The set is scripts/ubench/ragged_variant_c_bench.py's: 8 YFCC-like pairs of five sizes, four candidates each, the YFCC script's
settings.  Three measurements in ONE process, the two paths of each alternating, --reps repetitions after two warm-up runs, median
(min-max):
1. *points chain*: maps at the resized sizes of the chosen candidates (the driver's records.size_tgt), seeded flows, 5 % / 50 % / 95 %
   of the pixels explained.  ops.matches_from_flow_ragged on the packed buffers against the per-pair loop of ops.matches_from_flow on
   the same maps, host clock around each (both end in their offset reads: one for the batch, one per pair); and the three launches of
   ops.flow_points_ragged alone between HIP events (no read).
2. *driver*: multi_h_variant_c(..., want_records=True) against the same call without, HIP events around the whole call.
3. *end to end*: driver(want_records=True, want_lists=False) -> assemble.yfcc_matches_records against driver -> per pair
   assemble.assemble_yfcc + assemble.yfcc_matches on the returned lists, th 0.95, host clock from the call to the last read; peak
   device allocation of each.
No ratio is expected in advance: the record says which path was faster."""
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
from ragged_variant_c_bench import ANGLES, peak_bytes  # noqa: E402


def stats(v, unit="ms", digits=3):
    return {"median_" + unit: round(statistics.median(v), digits), "min_" + unit: round(min(v), digits), "max_" + unit: round(max(v), digits),
            unit: [round(x, digits) for x in v]}


def alternate(legs, reps, dev, clock):
    """Two warm-up runs per leg, then ``reps`` alternating repetitions.  clock "host": perf_counter around a call that ends in a host
    read; "event": HIP events around the call."""
    for _, fn in legs:
        fn(), fn()
    torch.cuda.synchronize(dev)
    out = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, fn in legs:
            if clock == "host":
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                out[name].append((time.perf_counter() - t0) * 1e3)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out[name].append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_ragged_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    pipe = AlignPipeline(sds, nbScale=7, nbIter=10000, tolerance=0.05, minSize=480, scaleR=2.0, variant="C", device=dev)
    kw = dict(maxCoarse=10, maskRegionTh=0.01)
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)
    src, tgt = [], []
    for b in range(a.pairs):
        I1, I2 = synth.make_pair(*SIZES[b % len(SIZES)], seed=b, homography=True)
        turn = ANGLES[(b // 2) % 4] if b % 2 else 0                          # every second target is stored turned
        src.append(up(I1))
        tgt.append(torch.rot90(up(I2), turn // 90, (0, 1)).contiguous())
    cands = [[torch.rot90(t, k, (0, 1)).contiguous() for t in tgt] for k in range(4)]
    ids = list(range(a.pairs))
    clock0 = clocks()

    def driver(**more):
        return pipe.multi_h_variant_c(src, cands, pair_ids=ids, **kw, **more)

    outs, R = driver(want_records=True)
    R.angle = [ANGLES[c] for c in R.candidate]
    sizes = [(h, w) for w, h in R.size_tgt]
    res = dict(tag=a.tag, pairs=a.pairs, reps=a.reps, host=socket.gethostname(), map_sizes=sizes, source_sizes=R.size_src,
               chosen=R.candidate, nbH=[o["nbH"] for o in outs], pixels=sum(h * w for h, w in sizes),
               settings="YFCC script: variant C, nbScale 7, minSize 480, scaleR 2, nbIter 10000, tolerance 0.05, maxCoarse 10, "
                        "maskRegionTh 0.01, device draws by pair id, degenerate=lapack")

    # 1. the points chain on maps of the batch's sizes
    g = torch.Generator().manual_seed(1)
    total = res["pixels"]
    flow = (torch.rand(total, 2, generator=g) * 2 - 1).to(dev)
    cut = lambda t, tail: [t[o:o + h * w].view((h, w) + tail) for o, (h, w) in zip(np.cumsum([0] + [h * w for h, w in sizes[:-1]]).tolist(), sizes)]
    flows = cut(flow, (2,))
    res["points"] = {}
    for frac in (0.05, 0.5, 0.95):
        keep = (torch.rand(total, generator=g) < frac).to(dev)
        keeps = cut(keep, ())

        def one_chain():
            return ops.matches_from_flow_ragged(flow, keep, sizes, R.size_src, R.angle)

        def per_pair():
            return [ops.matches_from_flow(flows[b], keeps[b], R.size_src[b], (w, h) if R.candidate[b] % 2 == 0 else (h, w), R.angle[b])
                    for b, (h, w) in enumerate(sizes)]

        x, y = one_chain(), per_pair()
        assert all(torch.equal(x[1][int(x[2][b]):int(x[2][b + 1])], y[b][1]) for b in range(a.pairs))
        assert all(torch.equal(x[0][int(x[2][b]):int(x[2][b + 1])].view(torch.int32), y[b][0].view(torch.int32)) for b in range(a.pairs))
        rows = int(x[2][-1])
        del x, y
        t = alternate((("one_chain", one_chain), ("per_pair_loop", per_pair)), a.reps, dev, "host")
        ev = alternate((("three_launches", lambda: ops.flow_points_ragged(flow, keep, sizes, R.size_src, R.angle)),), a.reps, dev, "event")
        rec = dict(rows=rows, one_chain=stats(t["one_chain"]), per_pair_loop=stats(t["per_pair_loop"]),
                   three_launches_no_read=stats([v * 1e3 for v in ev["three_launches"]], "us", 1),
                   launches=dict(one_chain=3, per_pair_loop=3 * a.pairs), host_reads=dict(one_chain=1, per_pair_loop=a.pairs))
        rec["loop_over_chain"] = round(rec["per_pair_loop"]["median_ms"] / rec["one_chain"]["median_ms"], 3)
        res["points"]["%d%%" % round(100 * frac)] = rec
    del flow, flows, keep, keeps

    # 2. what the record path costs the driver
    t = alternate((("default", lambda: driver()), ("want_records", lambda: driver(want_records=True))), a.reps, dev, "event")
    res["driver"] = dict(default=stats(t["default"], digits=2), want_records=stats(t["want_records"], digits=2),
                         peak_bytes=dict(default=peak_bytes(lambda: driver(), dev), want_records=peak_bytes(lambda: driver(want_records=True), dev)))
    res["driver"]["records_minus_default_ms"] = round(res["driver"]["want_records"]["median_ms"] - res["driver"]["default"]["median_ms"], 2)

    # 3. end to end: uploaded images -> point lists
    th = 0.95

    def batch_form():
        _, rec = driver(want_records=True, want_lists=False)
        rec.angle = [ANGLES[c] for c in rec.candidate]
        return assemble.yfcc_matches_records(rec, th, True)

    def per_pair_form():
        pts = []
        for b, o in enumerate(driver()):
            if not o["nbH"]:
                pts.append(None)
                continue
            h, w = o["mask"].shape
            fg, binary = assemble.assemble_yfcc(torch.cat(o["flowDown8"]), torch.stack(o["H"]), torch.cat(o["matchDown8"]),
                                                torch.ones((h, w), dtype=torch.bool, device=dev), th, True, device=dev)
            k = o["candidate"]
            pts.append(assemble.yfcc_matches(fg, binary, R.size_src[b], (w, h) if k % 2 == 0 else (h, w), ANGLES[k]))
        return pts

    x, y = batch_form(), per_pair_form()
    for b in range(a.pairs):
        rows = slice(int(x[2][b]), int(x[2][b + 1]))
        if y[b] is None:
            assert rows.start == rows.stop
        else:
            assert torch.equal(x[1][rows], y[b][1]) and torch.equal(x[0][rows].view(torch.int32), y[b][0].view(torch.int32)), b
    res["end_to_end"] = dict(th=th, rows=int(x[2][-1]), pairs_with_points=int((x[2][1:] > x[2][:-1]).sum()))
    del x, y
    t = alternate((("batch_form", batch_form), ("per_pair_form", per_pair_form)), a.reps, dev, "host")
    res["end_to_end"].update(batch_form=stats(t["batch_form"], digits=2), per_pair_form=stats(t["per_pair_form"], digits=2),
                             peak_bytes=dict(batch_form=peak_bytes(batch_form, dev), per_pair_form=peak_bytes(per_pair_form, dev)))
    res["end_to_end"]["per_pair_over_batch"] = round(res["end_to_end"]["per_pair_form"]["median_ms"] / res["end_to_end"]["batch_form"]["median_ms"], 3)
    res.update(sclk_before=clock0, sclk_after=clocks())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
