#!/usr/bin/env python
"""KITTI multi-homography alignment of a mixed-size list: one ragged multi_h_kitti_batched call vs one pair at a time through the
dense driver at batch 1.

    timeout -k 10 1100 python scripts/ubench/ragged_kitti_bench.py [--pairs 10] [--reps 5] [--legs ragged,loop]
                                                                   [--out profiles/ragged_kitti_bench.json]

The list: rfx.synth.make_pair(homography=True, amp=0.02) pairs over the five frame sizes of KITTI 2012 / 2015 (1242x375, 1241x376,
1238x374, 1226x370, 1224x370), BASELINE config 5's settings (variant B, coarseSize 800, 3 scales x1.2, 50 000 hypotheses, fineSize
650, maskRegionTh 0.005, cc_th 0.01, device draws keyed by pair id, the default exact ``degenerate`` mode); ``--scale`` shrinks the
frames and both sizes alike (for a quick look; the committed figures are at scale 1).  Leg "ragged": ONE multi_h_kitti_batched call
on the lists.  Leg "loop": the same pairs one after the other, multi_h_kitti_batched on (1,H,W,3) tensors -- the only way to run such
a list without the ragged path, and the baseline.  Both legs start from the raw uint8 images on the device.  Each repetition is timed
with HIP events around the whole call, host readbacks included; after two warm-up runs per leg (the loop's HIP-graph captures happen
at the second sighting of a shape) the legs alternate, --reps repetitions each; median and min-max spread are reported, with the
launch counts of the round kernels per leg, the fine-group sizes, the shader clock seen before and after, and the host name.
``--legs``: which legs run, in this order; "ragged_per_group" is the ragged call with RFX_FINE_GROUPS=0 (both fine passes once per fine
group instead of one grouped chain).  Every leg also reports its peak device allocation, its eager entry calls and its grouped launches
per call.
"""
import argparse
import collections
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rfx import ops, synth, weights  # noqa: E402
from rfx.pipeline import AlignPipeline  # noqa: E402
from ragged_multih_bench import clocks  # noqa: E402
from ragged_variant_c_bench import env_leg, peak_bytes  # noqa: E402

KITTI_SIZES = [(375, 1242), (376, 1241), (374, 1238), (370, 1226), (370, 1224)]          # (H, W)
COUNTED = ("filter_matches", "filter_matches_ragged", "draw_samples", "ransac_h4_batched_begin", "ransac_h4_batched", "remove_small_cc",
           "remove_small_cc_ragged", "multih_accept", "multih_accept_ragged", "warp_grid")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--legs", default="ragged,loop", help="comma-separated: ragged, ragged_per_group, loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_kitti_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    sc = a.scale
    coarse, fine = (800, 650) if sc == 1.0 else (int(round(800 * sc / 16)) * 16, int(round(650 * sc / 2)) * 2)
    pipe = AlignPipeline(sds, nbScale=3, nbIter=50000, tolerance=0.05, minSize=coarse, scaleR=1.2, variant="B", device=dev)
    kw = dict(fineSize=fine, maskRegionTh=0.005, cc_th=0.01, want_lists=False)
    sizes = [(int(round(h * sc)), int(round(w * sc))) for h, w in KITTI_SIZES]
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)
    raw = [tuple(up(im) for im in synth.make_pair(*sizes[b % len(sizes)], seed=b, homography=True, amp=0.02)) for b in range(a.pairs)]
    src, tgt = [r[0] for r in raw], [r[1] for r in raw]
    ids = list(range(a.pairs))

    def run_ragged():
        return [o["nbH"] for o in pipe.multi_h_kitti_batched(src, tgt, pair_ids=ids, **kw)]

    def run_loop():
        return [pipe.multi_h_kitti_batched(s[None], t[None], pair_ids=[b], **kw)[0]["nbH"] for b, (s, t) in enumerate(raw)]

    known = dict(ragged=run_ragged, ragged_per_group=env_leg(run_ragged, RFX_FINE_GROUPS="0"), loop=run_loop)
    legs = tuple((name, known[name]) for name in a.legs.split(","))
    clock0 = clocks()
    nbh = {}
    for name, fn in legs:
        fn()
        nbh[name] = fn()
    torch.cuda.synchronize(dev)
    assert all(n == nbh[legs[0][0]] for n in nbh.values()), nbh               # same work in all legs
    # launch counts of the round kernels, one untimed run per leg
    launches = {}
    for name, fn in legs:
        cnt, saved = collections.Counter(), {}
        for op in COUNTED:
            saved[op] = getattr(ops, op)

            def counted(*args, _f=saved[op], _n=op, **kwargs):
                cnt[_n] += 1
                return _f(*args, **kwargs)
            setattr(ops, op, counted)
        eager, call0 = [0], ops._call

        def counting_call(*args, **kwargs):                                 # every kernel entry call of the mirrors goes through ops._call
            if getattr(ops.launch_group._tls, "active", None) is None:
                eager[0] += 1
            return call0(*args, **kwargs)
        ops._call = counting_call
        g0 = ops.group_stats()[1]
        try:
            fn()
        finally:
            ops._call = call0
            for op, f in saved.items():
                setattr(ops, op, f)
        rounds = cnt["filter_matches"] + cnt["filter_matches_ragged"]          # one filter launch per round (and lock-step group)
        launches[name] = dict(per_call=dict(cnt), rounds=rounds, per_round={k: round(v / rounds, 2) for k, v in cnt.items()},
                              eager_entry_calls=eager[0], grouped_launches=ops.group_stats()[1] - g0, peak_bytes=peak_bytes(fn, dev))
    torch.cuda.synchronize(dev)
    ms = {name: [] for name, _ in legs}
    for _ in range(a.reps):
        for name, fn in legs:                                               # interleaved: drift hits both legs alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    fine_groups = collections.Counter((tuple(s.shape[:2]), tuple(t.shape[:2])) for s, t in raw)
    res = dict(pairs=a.pairs, reps=a.reps, scale=sc, sizes=sorted(set(sizes[:a.pairs])), settings="config 5: variant B, coarseSize %d, "
               "nbScale 3, scaleR 1.2, nbIter 50000, fineSize %d, maskRegionTh 0.005, cc_th 0.01, device draws by pair id, "
               "degenerate=lapack" % (coarse, fine), fine_group_sizes=sorted(fine_groups.values(), reverse=True),
               nbH=nbh[legs[0][0]], homographies=sum(nbh[legs[0][0]]), launches=launches, host=socket.gethostname(),
               sclk_before=clock0, sclk_after=clocks())
    for name, _ in legs:
        med = statistics.median(ms[name])
        res[name] = dict(ms=[round(x, 2) for x in ms[name]], median_ms=round(med, 2), min_ms=round(min(ms[name]), 2),
                         max_ms=round(max(ms[name]), 2), pairs_per_s=round(a.pairs / med * 1e3, 2))
    if "ragged" in res and "loop" in res:
        res["speedup_ragged_over_loop"] = round(res["loop"]["median_ms"] / res["ragged"]["median_ms"], 3)
        res["loop_spread_ms"] = round(res["loop"]["max_ms"] - res["loop"]["min_ms"], 2)
        res["ragged_not_slower_than_loop_beyond_its_spread"] = res["ragged"]["median_ms"] <= res["loop"]["median_ms"] + res["loop_spread_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
