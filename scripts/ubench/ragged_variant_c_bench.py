#!/usr/bin/env python
"""The YFCC (variant C) multi-homography driver on a mixed-size set: one multi_h_variant_c call on lists vs one pair at a time through
the dense driver at batch 1.

    timeout -k 10 900 python scripts/ubench/ragged_variant_c_bench.py [--pairs 8] [--reps 5] [--tag NAME] [--legs ragged,loop] [--tail]
                                                                      [--out profiles/ragged_variant_c_bench.json]

The set: rfx.synth.make_pair(homography=True) pairs over the size list of ragged_bench.py (the first 8 hold five sizes), every second
target stored turned by 90 / 180 / 270 degrees, the four rotations of each target as its candidates
(evaluation/evalYFCC/evaluation.py:189), the YFCC script's settings (variant C, nbScale 7, minSize 480, scaleR 2, 10 000 hypotheses,
tolerance 0.05, maxCoarse 10, maskRegionTh 0.01), device draws keyed by pair id, the default exact ``degenerate`` mode.
Leg "ragged": ONE multi_h_variant_c call on the lists.  Leg "loop": the same pairs one after the other through the dense driver on
(1,H,W,3) tensors -- what a caller has to do with such a set without the list entry, and the baseline.  The images are uploaded and
turned outside the timed region; the device pyramids, the trunk passes, the candidate search and the rounds are inside, in both legs.
Each repetition is timed with HIP events around the whole call, host readbacks included; after two warm-up runs per leg (the loop's
HIP-graph captures happen at the second sighting of a shape) the legs alternate, --reps repetitions each; medians and min-max ranges
are reported, with the launch counts of the search and of a round per leg, the shader clock seen before and after and the host name.
No ratio is expected in advance: the record says which leg was faster.
``--legs``: which legs run, in this order; "ragged_per_group" is the ragged call with RFX_FINE_GROUPS=0 (the fine stage once per fine
group instead of one grouped chain).  Every leg also reports its peak device allocation, its eager entry calls and its grouped launches
per call.  ``--tail``: ops.cycle_tail against the four-kernel chain it fuses, at 480x640 (batch 4) and 375x1242 (batch 2): median of
200 timed calls each and peak allocation (profiles/ragged_cycle_groups_bench.json was made from such records of the parent commit's
build and this one, run alternately in one job)."""
import argparse
import collections
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rfx import ops, synth, weights  # noqa: E402
from rfx.pipeline import AlignPipeline  # noqa: E402
from ragged_bench import SIZES  # noqa: E402
from ragged_multih_bench import clocks  # noqa: E402

ANGLES = (0, 90, 180, 270)
COUNTED = ("keep_mask", "keep_mask_ragged", "mutual_nn_ragged", "gather_matches", "gather_matches_ragged", "draw_samples",
           "ransac_h4_batched_begin", "ransac_h4_batched", "multih_accept", "multih_accept_ragged", "warp_grid")


def peak_bytes(fn, dev):
    """Peak device allocation of one call of fn above what is allocated before it."""
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


def env_leg(fn, **env):
    """fn with the environment variables ``env`` set for the call."""
    def run():
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return fn()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return run


def tail_bench(dev, iters=200):
    """ops.cycle_tail against resize_bilinear -> compose_flow -> grid_sample -> match_score on the same inputs."""
    out = {}
    for name, B, H, W in (("480x640", 4, 480, 640), ("375x1242", 2, 375, 1242)):
        hd, wd = H // 8, W // 8
        g = torch.Generator().manual_seed(H)
        fd = (torch.randn(B, 2, hd, wd, generator=g) * 0.05).to(dev)
        md = torch.rand(2 * B, 1, hd, wd, generator=g).to(dev)
        Hm = (torch.eye(3).repeat(B, 1, 1) + 0.02 * torch.randn(B, 3, 3, generator=g)).to(dev)
        cg = ops.warp_grid(Hm, H, W)

        def chain():
            m = ops.resize_bilinear(md, (H, W), align_corners=False)
            flow12, inb, flowUp = ops.compose_flow(fd, cg, clamp=True, want_inb=True, want_flow_up=True)
            return flow12, ops.match_score(m[:B, 0], ops.grid_sample(m[B:], flowUp)[:, 0], inb)

        fused = lambda: ops.cycle_tail(fd, md[:B], md[B:], cg)
        a, b = chain(), fused()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        del a, b
        rec = dict(batch=B, pixels=B * H * W)
        for leg, fn in (("chain", chain), ("cycle_tail", fused)):
            rec[leg] = dict(peak_bytes=peak_bytes(fn, dev))
        us = {"chain": [], "cycle_tail": []}
        for _ in range(iters):                                              # interleaved
            for leg, fn in (("chain", chain), ("cycle_tail", fused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us[leg].append(e0.elapsed_time(e1) * 1e3)
        for leg in us:
            v = sorted(us[leg])
            rec[leg].update(median_us=round(statistics.median(v), 2), min_us=round(v[0], 2), p90_us=round(v[int(0.9 * len(v))], 2))
        rec["chain_over_cycle_tail"] = round(rec["chain"]["median_us"] / rec["cycle_tail"]["median_us"], 3)
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="", help="name of this build in the record")
    ap.add_argument("--legs", default="ragged,loop", help="comma-separated: ragged, ragged_per_group, loop")
    ap.add_argument("--tail", action="store_true", help="also time ops.cycle_tail against the four-kernel chain")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_variant_c_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    pipe = AlignPipeline(sds, nbScale=7, nbIter=10000, tolerance=0.05, minSize=480, scaleR=2.0, variant="C", device=dev)
    kw = dict(maxCoarse=10, maskRegionTh=0.01)
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)
    src, tgt, stored = [], [], []
    for b in range(a.pairs):
        I1, I2 = synth.make_pair(*SIZES[b % len(SIZES)], seed=b, homography=True)
        turn = ANGLES[(b // 2) % 4] if b % 2 else 0                          # every second target is stored turned
        stored.append(turn)
        src.append(up(I1))
        tgt.append(torch.rot90(up(I2), turn // 90, (0, 1)).contiguous())
    cands = [[torch.rot90(t, k, (0, 1)).contiguous() for t in tgt] for k in range(4)]
    ids = list(range(a.pairs))

    def summary(outs):
        return [(o["nbH"], o["candidate"]) for o in outs]

    def run_ragged():
        return summary(pipe.multi_h_variant_c(src, cands, pair_ids=ids, **kw))

    def run_loop():
        return summary([pipe.multi_h_variant_c(src[b][None], [c[b][None] for c in cands], pair_ids=[b], **kw)[0] for b in range(a.pairs)])

    known = dict(ragged=run_ragged, ragged_per_group=env_leg(run_ragged, RFX_FINE_GROUPS="0"), loop=run_loop)
    legs = tuple((name, known[name]) for name in a.legs.split(","))
    clock0 = clocks()
    got = {}
    for name, fn in legs:
        fn()
        got[name] = fn()
    torch.cuda.synchronize(dev)
    assert all(g == got[legs[0][0]] for g in got.values()), got              # same work in all legs
    # launch counts, one untimed run per leg: the K searches (one draw each) and the rounds (one accept each)
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
        rounds = cnt["multih_accept"] + cnt["multih_accept_ragged"]          # one accept per round (and lock-step / shape group)
        searches = cnt["draw_samples"] - rounds                              # one draw per candidate search and per round
        launches[name] = dict(per_call=dict(cnt), searches=searches, rounds=rounds, eager_entry_calls=eager[0],
                              grouped_launches=ops.group_stats()[1] - g0, peak_bytes=peak_bytes(fn, dev))
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
    res = dict(tag=a.tag, pairs=a.pairs, reps=a.reps, candidates=len(ANGLES), source_sizes=sorted({tuple(x.shape[:2]) for x in src}),
               stored_turns=stored, settings="YFCC script: variant C, nbScale 7, minSize 480, scaleR 2, nbIter 10000, tolerance 0.05, "
               "maxCoarse 10, maskRegionTh 0.01, device draws by pair id, degenerate=lapack",
               nbH=[n for n, _ in got[legs[0][0]]], chosen=[c for _, c in got[legs[0][0]]],
               homographies=sum(n for n, _ in got[legs[0][0]]),
               launches=launches, host=socket.gethostname(), sclk_before=clock0, sclk_after=clocks())
    for name, _ in legs:
        med = statistics.median(ms[name])
        res[name] = dict(ms=[round(x, 2) for x in ms[name]], median_ms=round(med, 2), min_ms=round(min(ms[name]), 2),
                         max_ms=round(max(ms[name]), 2), pairs_per_s=round(a.pairs / med * 1e3, 2))
    if "ragged" in res and "loop" in res:
        res["speedup_ragged_over_loop"] = round(res["loop"]["median_ms"] / res["ragged"]["median_ms"], 3)
        res["ranges_overlap"] = res["ragged"]["max_ms"] >= res["loop"]["min_ms"] and res["loop"]["max_ms"] >= res["ragged"]["min_ms"]
    if a.tail:
        res["cycle_tail"] = tail_bench(dev)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
