#!/usr/bin/env python
"""Library entry calls and results of the public drivers at small sizes, as one JSON -- to compare two trees of this repository.

    timeout -k 10 600 python scripts/entry_trace.py [--tree PATH] --out profiles/NAME.json

Wraps ops._call (every kernel entry call of the Python side goes through it) and reads ops.group_stats().  Per scenario the record
holds ``calls``: the ordered entry names, one string, a leading "+" = recorded in a group, a block of calls repeated n times in a
row written once, as "name*n" or "[name name ...]*n" (fold()); ``groups`` / ``grouped_launches``: the launch_group blocks that ended and the kernel launches they issued; ``sha256``: a digest of every tensor (and number) the call returned, by its
path in the result (of the cached match lists: the rows below the count).  The calls recorded in ONE group are listed sorted by name: a group launches per kernel instance when it ends,
so the order in which its problems were recorded is not an order of launches.  Fixed seed, device draws keyed by pair id, split=1,
RFX_GRAPH=0 (the trunk pass is traced as launches, not replayed as a graph), degenerate="device" (no host stage).  ``--tree``: the
checkout whose package is imported (default: the one this script lies in), so one copy of the script can trace a parent commit.
Reads nothing outside that tree.
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fold(names):
    """A list of entry names with every immediate repetition written once: at each position the block (up to 300 names) whose
    repeats cover most is taken, "[a b c]*n" (one name: "a*n"), blocks folded in turn.  Names hold no space, bracket or asterisk, so
    two lists fold to the same strings only if they are equal."""
    out, i = [], 0
    while i < len(names):
        best = (0, 1, 1)                                                    # (names saved, block length, repeats)
        for L in range(1, min(300, (len(names) - i) // 2) + 1):
            r = 1
            while names[i + r * L:i + (r + 1) * L] == names[i:i + L]:
                r += 1
            if (r - 1) * L > best[0]:
                best = ((r - 1) * L, L, r)
        _, L, r = best
        block = fold(names[i:i + L]) if L > 1 else names[i:i + 1]
        out.append(block[0] if r == 1 else ("%s*%d" % (block[0], r) if L == 1 else "[%s]*%d" % (" ".join(block), r)))
        i += L * r
    return out


def digest(obj, path, out):
    import torch
    if isinstance(obj, torch.Tensor):
        t = obj.detach().cpu().contiguous()
        h = hashlib.sha256(repr((str(t.dtype), tuple(t.shape))).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
        out[path] = h.hexdigest()
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            v = obj[k]
            if k == "matches":                          # (idx1, idx2, count): the rows beyond the count are undefined
                n = int(v[2])
                v = (v[0][:n], v[1][:n], v[2])
            digest(v, "%s.%s" % (path, k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            digest(v, "%s[%d]" % (path, i), out)
    elif isinstance(obj, (int, float, bool)):
        out[path] = repr(obj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.environ["RFX_GRAPH"] = "0"
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "ransac-flow_amd"))
    import numpy as np
    import torch
    from rfx import ops, synth, weights
    from rfx.pipeline import AlignPipeline, resize_dims

    dev = torch.device("cuda:0")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    pipe = AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant="B", device=dev, seed=5,
                         degenerate="device")
    dense = [synth.make_pair(240, 320, seed=20 + b, homography=True) for b in range(4)]
    mixed = []
    for seed, H, W, dh, dw in ((7, 240, 320, 0, 0), (8, 256, 320, 0, 16), (9, 240, 336, 0, 0)):
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
        mixed.append((I1, I2.crop((0, 0, W - dw, H - dh))))
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)
    d_src, d_tgt = torch.stack([up(p[0]) for p in dense]), torch.stack([up(p[1]) for p in dense])
    m_src, m_tgt = [up(p[0]) for p in mixed], [up(p[1]) for p in mixed]
    kitti = dict(fineSize=200, maskRegionTh=0.005, cc_th=0.01)
    ids4, ids3 = [11, 12, 13, 14], [21, 22, 23]
    # the YFCC driver: a variant-C pipeline, K = 2 candidates per pair (the target and its quarter turn)
    pipe_c = AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant="C", device=dev, seed=5,
                           degenerate="device")
    m_cands = [m_tgt, [torch.rot90(t, 1, (0, 1)).contiguous() for t in m_tgt]]

    def half_ones(t):
        """A background map for the uint8 (H,W,3) target ``t`` at its resized size: ones in the left half."""
        nw, nh = resize_dims(t.shape[1], t.shape[0], 240, "min")
        m = torch.zeros((nh, nw), dtype=torch.float32, device=dev)
        m[:, :nw // 2] = 1
        return m
    bg_b = [half_ones(m_tgt[0]), None, half_ones(m_tgt[2])]
    bg_c = [[half_ones(m_cands[0][0]), None, half_ones(m_cands[0][2])], [None, half_ones(m_cands[1][1]), half_ones(m_cands[1][2])]]

    scenarios = [
        ("features_B1", lambda: pipe.features(pipe.prepare_device(d_src[:1], d_tgt[:1]))),
        ("features_B4", lambda: pipe.features(pipe.prepare_device(d_src, d_tgt))),
        ("align_pairs_dense", lambda: pipe.align_pairs(dense, pair_ids=ids4)),
        ("align_pairs_mixed", lambda: pipe.align_pairs(mixed, pair_ids=ids3)),
        ("multi_h_batched_dense", lambda: pipe.multi_h_batched(pipe.prepare_device(d_src, d_tgt), maxCoarse=3, pair_ids=ids4, split=1)),
        ("multi_h_batched_ragged", lambda: pipe.multi_h_batched(pipe.prepare_ragged_device(m_src, m_tgt), maxCoarse=3, pair_ids=ids3,
                                                                split=1)),
        ("multi_h_kitti_batched_dense", lambda: pipe.multi_h_kitti_batched(d_src, d_tgt, pair_ids=ids4, split=1, **kitti)),
        ("multi_h_kitti_batched_ragged", lambda: pipe.multi_h_kitti_batched(m_src, m_tgt, pair_ids=ids3, split=1, **kitti)),
        ("multi_h_variant_c_one_candidate", lambda: pipe.multi_h_variant_c(d_src, [d_tgt], maxCoarse=3, pair_ids=ids4)),
        ("multi_h_one_pair", lambda: pipe.multi_h(pipe.prepare_device(d_src[:1], d_tgt[:1]), 0, maxCoarse=3)),
        ("multi_h_kitti_one_pair", lambda: pipe.multi_h_kitti(d_src[:1], d_tgt[:1], **kitti)),
        ("multi_h_batched_ragged_bg", lambda: pipe.multi_h_batched(pipe.prepare_ragged_device(m_src, m_tgt), maxCoarse=3, It_bg=bg_b,
                                                                   pair_ids=ids3, split=1)),
        ("multi_h_variant_c_lists", lambda: pipe_c.multi_h_variant_c(m_src, m_cands, maxCoarse=3, pair_ids=ids3, split=1)),
        ("multi_h_variant_c_lists_bg", lambda: pipe_c.multi_h_variant_c(m_src, m_cands, maxCoarse=3, It_bg=bg_c, pair_ids=ids3, split=1)),
    ]
    call0 = ops._call
    res = {}
    for name, fn in scenarios:
        pipe.reseed(5)
        pipe_c.reseed(5)
        log = []

        def traced(entry, *args, **kw):
            log.append((entry, ops.launch_group.recording(), ops.group_stats()[0]))
            return call0(entry, *args, **kw)
        g0 = ops.group_stats()
        ops._call = traced
        try:
            out = fn()
        finally:
            ops._call = call0
        torch.cuda.synchronize(dev)
        g1 = ops.group_stats()
        calls, i = [], 0
        while i < len(log):
            j = i + 1
            if log[i][1]:
                while j < len(log) and log[j][1] and log[j][2] == log[i][2]:
                    j += 1
            calls += [("+" if r else "") + e for e, r, _ in sorted(log[i:j])]
            i = j
        sha = {}
        digest(out, "out", sha)
        res[name] = dict(calls=" ".join(fold(calls)), entry_calls=len(calls), groups=g1[0] - g0[0], grouped_launches=g1[1] - g0[1], sha256=sha)
        print("%-34s %5d entry calls (%4d recorded), %3d groups, %4d grouped launches, %3d results" %
              (name, len(calls), sum(1 for c in calls if c[0] == "+"), g1[0] - g0[0], g1[1] - g0[1], len(sha)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
