#!/usr/bin/env python
"""The scripts' --segNet step (sky mask of every target -> It_bg) per target through the host against the batched device path, in ONE
process, the paths alternating:

    (a) 8 targets in two sizes (4 of 480 x 640, 4 of 600 x 450), It_bg at the target's size resized to minSize 480:
        parent:  per target SegNetDevice.getSky(PIL image) -- five PIL BILINEAR resizes and uploads, five network passes at batch 1,
                 per scale the (1, 150, H, W) up-sampled logits and scores, the mask's download -- then the scripts'
                 imresize(mask, (h, w)) < 128 on the host (the scipy 1.2.3 stand-in, stated below) and the upload of It_bg
        batched: the upload of the 8 raw images, then pipeline.sky_backgrounds (get_sky_batch + ops.sky_background)
        wall clock around a synchronise; the two results are compared bit for bit
    (b) ops.seg_vote against resize_bilinear -> softmax_accum per scale -> argmax_mask on the five logit maps of ONE 480 x 640
        image (C = 150), HIP events around INNER consecutive calls, and the peak allocation of one call of each
    (c) get_sky_batch on 8 targets of 480 x 640 with max_batch 1, 4 and 8

REPS repetitions each, median with min and max.  -> profiles/sky_bench.json

    python scripts/ubench/sky_bench.py [--out profiles/sky_bench.json] [--reps 5]
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
import PIL.Image as Image  # noqa: E402
from rfx import ops, pipeline, synth, weights  # noqa: E402
from rfx.segnet import SegNetDevice, input_sizes  # noqa: E402

INNER = 5
MIN_SIZE = 480


def imresize(arr, size):
    """scipy.misc.imresize of scipy 1.2.3 for a 2-D float array, interp="bilinear" (the stand-in of dropin/run_reference_script.py)."""
    data = np.asarray(arr)
    cmin, cmax = data.min(), data.max()
    cscale = (cmax - cmin) or 1
    data = (((data - cmin) * (255.0 / cscale)).clip(0, 255) + 0.5).astype(np.uint8)
    im = Image.frombytes("L", (data.shape[1], data.shape[0]), data.tobytes())
    return np.asarray(im.resize((int(size[1]), int(size[0])), resample=Image.BILINEAR))


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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = SegNetDevice(weights.seg_encoder_sd(4, randomize_bn=True), weights.seg_decoder_sd(5, randomize_bn=True, logit_std=0.003),
                       segId=47, segFg=True, device=dev)
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)
    rec = dict(what="sky masks of targets -> It_bg: the per-target host path of the parent (getSky + imresize + threshold + upload) against "
                    "the batched device path (pipeline.sky_backgrounds), alternating in one process, %d repetitions each; seg_vote "
                    "against the three-kernel chain by HIP events around %d consecutive calls; milliseconds, bytes" % (a.reps, INNER),
               device=torch.cuda.get_device_name(0), reps=a.reps, default_max_batch=8)

    # (a)
    imgs = [synth.make_pair(h, w, seed=20 + i)[0] for i, (h, w) in enumerate([(480, 640), (600, 450)] * 4)]
    sizes = []
    for im in imgs:
        nw, nh = pipeline.resize_dims(im.size[0], im.size[1], MIN_SIZE, "min")
        sizes.append((nh, nw))

    def parent():
        out = []
        for im, hw in zip(imgs, sizes):
            mask = net.getSky(im)
            out.append(torch.from_numpy((imresize(mask, hw) < 128).astype(np.float32)).to(dev))
        return out

    def batched(max_batch=None):
        return pipeline.sky_backgrounds(net, [up(im) for im in imgs], sizes, max_batch=max_batch)

    ref, got = parent(), batched()
    equal = all(torch.equal(x, y) for x, y in zip(ref, got))
    p_ms, b_ms, b1_ms = [], [], []
    for _ in range(a.reps):
        p_ms.append(wall(parent)[0])
        b_ms.append(wall(batched)[0])
        b1_ms.append(wall(lambda: batched(1))[0])
    rec["a_eight_targets_two_sizes"] = dict(
        targets=[list(im.size[::-1]) for im in imgs], out_hw=[list(s) for s in sizes], bit_equal=equal,
        background_fraction=[round(1.0 - float(x.mean()), 4) for x in got], parent_ms=stats(p_ms), sky_backgrounds_ms=stats(b_ms),
        sky_backgrounds_max_batch_1_ms=stats(b1_ms), parent_over_batched_median=statistics.median(p_ms) / statistics.median(b_ms),
        parent_over_max_batch_1_median=statistics.median(p_ms) / statistics.median(b1_ms),
        parent_peak_bytes=peak_of(parent), sky_backgrounds_peak_bytes=peak_of(batched))
    print("(a)", json.dumps(rec["a_eight_targets_two_sizes"]))

    # (b)
    H, W, C = 480, 640, 150
    g = torch.Generator().manual_seed(1)
    logits = [(torch.randn(1, C, th // 8, tw // 8, generator=g) * 3).to(dev) for tw, th in input_sizes(W, H)]

    def chain():
        scores = None
        for l in logits:
            scores = ops.softmax_accum(ops.resize_bilinear(l, (H, W), align_corners=False), scores, div=5.0)
        return ops.argmax_mask(scores, 47, complement=True, want_pred=True)

    vote = lambda: ops.seg_vote(logits, (H, W), 47, complement=True, want_pred=True)
    same = all(torch.equal(x, y) for x, y in zip(chain(), vote()))
    c_ms, v_ms = [], []
    for _ in range(a.reps):
        c_ms.append(events(chain))
        v_ms.append(events(vote))
    rec["b_seg_vote_480x640_c150_s5"] = dict(bit_equal=same, chain_ms=stats(c_ms), seg_vote_ms=stats(v_ms),
                                             chain_over_vote_median=statistics.median(c_ms) / statistics.median(v_ms),
                                             chain_peak_bytes=peak_of(chain), seg_vote_peak_bytes=peak_of(vote),
                                             class_volume_bytes=C * H * W * 4)
    print("(b)", json.dumps(rec["b_seg_vote_480x640_c150_s5"]))

    # (c)
    u8 = [up(synth.make_pair(480, 640, seed=40 + i)[0]) for i in range(8)]
    base = net.get_sky_batch(u8, max_batch=1)
    times = {1: [], 4: [], 8: []}
    same = {mb: all(torch.equal(x, y) for x, y in zip(base, net.get_sky_batch(u8, max_batch=mb))) for mb in times}
    for _ in range(a.reps):
        for mb in times:
            times[mb].append(wall(lambda: net.get_sky_batch(u8, max_batch=mb))[0])
    rec["c_max_batch_8_targets_480x640"] = dict(
        bit_equal_to_max_batch_1=same, ms={str(mb): stats(v) for mb, v in times.items()},
        peak_bytes={str(mb): peak_of(lambda: net.get_sky_batch(u8, max_batch=mb)) for mb in times},
        max_batch_1_over_8_median=statistics.median(times[1]) / statistics.median(times[8]))
    print("(c)", json.dumps(rec["c_max_batch_8_targets_480x640"]))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
