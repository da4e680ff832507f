#!/usr/bin/env python
"""Multi-homography alignment of a mixed-size set: one ragged multi_h_batched call vs one pair at a time through the dense path.

    timeout -k 10 1100 python scripts/ubench/ragged_multih_bench.py [--pairs 32] [--reps 5] [--tag NAME]
                                                                    [--out profiles/ragged_multih_bench.json]

The set: rfx.synth.make_pair(homography=True) pairs over the size list of ragged_bench.py, BASELINE config 3's settings (variant B,
nbScale 7, minSize 480, scaleR 2, 10 000 hypotheses, maxCoarse 10, maskRegionTh 0.01, device draws keyed by pair id, the default
exact ``degenerate`` mode).  Leg "ragged": ONE multi_h_batched call on the ragged prep.  Leg "loop": the same pairs one after the
other, multi_h_batched on each pair's own dense prep -- the only way to run such a set without the ragged path, and the baseline.
Pre-processing (the pyramids) is outside the timed region of both legs.  Each repetition is timed with HIP events around the whole
call, host readbacks included; after two warm-up runs per leg (the loop's HIP-graph captures happen at the second sighting of a
shape) the legs alternate, --reps repetitions each; median and min-max spread are reported, with the launch counts of the round
kernels per leg, the shader clock seen before and after, and the host name.

Where the library has the grouped fine stage (RFX_FINE_GROUPS), the ragged call is timed both ways: leg "ragged" with
RFX_FINE_GROUPS=1 and leg "ragged_per_group" with RFX_FINE_GROUPS=0, interleaved with the loop.  Per leg and call the record also
holds the kernel launches issued by grouped launches (rfx_group_stats) and the number of eager kernel entry calls (ops._call outside
a launch_group).  --tag names the build in the record, for A/B runs of two trees in one job.
"""
import argparse
import collections
import json
import os
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))

import torch  # noqa: E402

from rfx import ops, synth, weights  # noqa: E402
from rfx.pipeline import AlignPipeline  # noqa: E402
from ragged_bench import SIZES  # noqa: E402

COUNTED = ("filter_matches", "filter_matches_ragged", "draw_samples", "ransac_h4_batched_begin", "ransac_h4_batched", "multih_accept",
           "multih_accept_ragged", "warp_grid")


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l][:1]
    except Exception as e:                                              # the figure is a record, never a reason to fail the bench
        return ["unavailable: %s" % type(e).__name__]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="", help="name of this build in the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_multih_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    pipe = AlignPipeline(sds, nbScale=7, nbIter=10000, tolerance=0.05, minSize=480, scaleR=2.0, variant="B", device=dev)
    kw = dict(maxCoarse=10, maskRegionTh=0.01, want_lists=False)
    pairs = [synth.make_pair(*SIZES[b % len(SIZES)], seed=b, homography=True) for b in range(a.pairs)]
    ids = list(range(a.pairs))
    rprep = pipe.prepare_ragged(pairs)
    preps = [pipe.prepare([p]) for p in pairs]

    def run_ragged():
        return [o["nbH"] for o in pipe.multi_h_batched(rprep, pair_ids=ids, **kw)]

    def run_loop():
        return [pipe.multi_h_batched(p, pair_ids=[b], **kw)[0]["nbH"] for b, p in enumerate(preps)]

    def with_fine_groups(flag, fn):
        def run():
            prev = os.environ.get("RFX_FINE_GROUPS")
            os.environ["RFX_FINE_GROUPS"] = flag
            try:
                return fn()
            finally:
                if prev is None:
                    del os.environ["RFX_FINE_GROUPS"]
                else:
                    os.environ["RFX_FINE_GROUPS"] = prev
        return run

    if hasattr(ops, "fine_groups_enabled"):
        legs = (("ragged", with_fine_groups("1", run_ragged)), ("ragged_per_group", with_fine_groups("0", run_ragged)), ("loop", run_loop))
    else:                                                                   # a tree from before the grouped fine stage
        legs = (("ragged", run_ragged), ("loop", run_loop))
    group_launches = (lambda: ops.group_stats()[1]) if hasattr(ops, "group_stats") else None
    clock0 = clocks()
    nbh = {}
    for name, fn in legs:
        fn()
        nbh[name] = fn()
    torch.cuda.synchronize(dev)
    assert all(nbh[name] == nbh["loop"] for name, _ in legs), nbh             # same work in every leg
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
        g0 = group_launches() if group_launches else None
        try:
            fn()
        finally:
            ops._call = call0
            for op, f in saved.items():
                setattr(ops, op, f)
        rounds = cnt["filter_matches"] + cnt["filter_matches_ragged"]          # one filter launch per round (and lock-step group)
        launches[name] = dict(per_call=dict(cnt), rounds=rounds, per_round={k: round(v / rounds, 2) for k, v in cnt.items()},
                              eager_entry_calls=eager[0], grouped_launches=None if g0 is None else group_launches() - g0)
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
    res = dict(tag=a.tag, pairs=a.pairs, reps=a.reps, sizes=sorted({tuple(s) for s in SIZES[:a.pairs]}), settings="config 3: variant B, nbScale 7, "
               "minSize 480, scaleR 2, nbIter 10000, maxCoarse 10, maskRegionTh 0.01, device draws by pair id, degenerate=lapack",
               nbH=nbh["ragged"], homographies=sum(nbh["ragged"]), launches=launches, host=socket.gethostname(),
               sclk_before=clock0, sclk_after=clocks())
    for name, _ in legs:
        med = statistics.median(ms[name])
        res[name] = dict(ms=[round(x, 2) for x in ms[name]], median_ms=round(med, 2), min_ms=round(min(ms[name]), 2),
                         max_ms=round(max(ms[name]), 2), pairs_per_s=round(a.pairs / med * 1e3, 2))
    res["speedup_ragged_over_loop"] = round(res["loop"]["median_ms"] / res["ragged"]["median_ms"], 3)
    res["loop_spread_ms"] = round(res["loop"]["max_ms"] - res["loop"]["min_ms"], 2)
    res["ragged_not_slower_than_loop_beyond_its_spread"] = res["ragged"]["median_ms"] <= res["loop"]["median_ms"] + res["loop_spread_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
