"""Generates tests/golden/corr_records.npz by running the REAL reference's own functions (compiled from where they lie by
oracle/ref_loader.script_functions; nothing of their text is copied): ``getFlow``, ``alignmentError``, ``ResizeMinResolution`` and
``ResizeMinResolution_megadepth`` of evaluation/evalCorr/getResults.py.  Authoring container only.

    python tests/golden/make_golden_corr_records.py

Three pairs of different /8 sizes -- 3x4, 5x4 and 6x8, maps of 24x32, 40x32 and 48x64 -- with nbH = 1, 3 and 0 (the last has no
saved files: getFlow returns its ([], []) sentinel and the script's loop takes its ``continue`` branch, :273-277).  The arrays are
written as the .npy files the script expects, getFlow assembles each pair, and for every matchability threshold the mask of
:281-282 goes into alignmentError with about 60 float keypoints per pair.

What is stored (data only):
    h8, w8, nbH, max_h         the pairs' /8 sizes, their numbers of homographies, the records' capacity
    p{b}_flow, p{b}_param, p{b}_match   pair b's synthetic flowDown8 (n,2,h8,w8), homographies (n,3,3), matchDown8 (n,2,h8,w8)
    th, multiH                 the assembly's arguments
    sizeA                      (wA, hA) per pair
    p{b}_XA, _YA, _XB, _YB     the float32 keypoints (fractions included)
    p{b}_xa, _ya, _m           the reference's estimates ((flow + 1) * 0.5 * (size - 1), float32) and matchGlobal at the target keypoints
    ths, grid                  the matchability thresholds 0, 0.5, 0.9 and the script's pixel grid
    counts (M,B,T), nbAlign (M,B)   alignmentError's returns, summed by nobody; the pair without files: nbAlign = its keypoints, counts 0
    rs_sizes, rs_min, rs_x, rs_y, rs_new, rs_outx, rs_outy, rs_valid   ResizeMinResolution(_megadepth) on a handful of sizes
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))

import ref_loader  # noqa: E402
from rfx import synth  # noqa: E402

SIZES8 = ((3, 4), (5, 4), (6, 8))
NBH = (1, 3, 0)
SIZE_A = ((301, 200), (97, 211), (640, 480))
THS = (0.0, 0.5, 0.9)
TH, MULTI_H, K, MAX_H = 0.3, True, 60, 4
RESIZE = ((1024, 768), (500, 375), (640, 480), (333, 500), (1600, 1067), (479, 2000))


def main():
    from PIL import Image
    f = ref_loader.script_functions("evaluation/evalCorr/getResults.py",
                                    ["getFlow", "alignmentError", "ResizeMinResolution", "ResizeMinResolution_megadepth"])
    f["ResizeMinResolution"].__globals__["Image"] = Image          # the script's own import, which the loader's namespace lacks
    grid = np.around(np.logspace(0, np.log10(36), 8).reshape(-1, 8))
    d = tempfile.mkdtemp()
    fine, coarse = os.path.join(d, "fine"), os.path.join(d, "coarse")
    os.makedirs(fine)
    os.makedirs(coarse)
    out = dict(h8=np.asarray([s[0] for s in SIZES8]), w8=np.asarray([s[1] for s in SIZES8]), nbH=np.asarray(NBH), max_h=np.asarray(MAX_H),
               th=np.asarray(TH), multiH=np.asarray(MULTI_H), sizeA=np.asarray(SIZE_A), ths=np.asarray(THS), grid=grid[0])
    for b, ((hd, wd), n) in enumerate(zip(SIZES8, NBH)):
        flowDown, _, param, md = synth.assembly_arrays(40 + b, max(n, 1), hd, wd)
        md = np.clip(md * 1.3, 0, 1).astype(np.float32)            # (the cycle product of two maps has to reach 0.9 somewhere)
        out.update({"p%d_flow" % b: flowDown.astype(np.float32), "p%d_param" % b: param, "p%d_match" % b: md})
        if n:
            np.save(os.path.join(fine, "flow_%d_%dH.npy" % (b, n)), flowDown)
            np.save(os.path.join(coarse, "flow_%d_%dH.npy" % (b, n)), param)
            np.save(os.path.join(fine, "mask_%d_%dH.npy" % (b, n)), md)
            np.save(os.path.join(fine, "maskBG_%d_%dH.npy" % (b, n)), np.ones((hd * 8, wd * 8), bool))
    flowList = os.listdir(fine)
    counts = np.zeros((len(THS), len(NBH), grid.shape[1]))
    nbAlign = np.zeros((len(THS), len(NBH)), np.int64)
    for b, ((hd, wd), n) in enumerate(zip(SIZES8, NBH)):
        hB, wB = hd * 8, wd * 8
        wA, hA = SIZE_A[b]
        rng = np.random.RandomState(70 + b)
        XB, YB = (rng.rand(K) * wB).astype(np.float32), (rng.rand(K) * hB).astype(np.float32)
        with torch.no_grad():
            flow, match = f["getFlow"](b, fine, flowList, coarse, fine, MULTI_H, TH)
        if len(flow) == 0:
            assert n == 0
            XA, YA = (rng.rand(K) * wA).astype(np.float32), (rng.rand(K) * hA).astype(np.float32)
            out.update({"p%d_XA" % b: XA, "p%d_YA" % b: YA, "p%d_XB" % b: XB, "p%d_YB" % b: YB})
            nbAlign[:, b] = K                                       # the ``continue`` branch: every keypoint counts, none is measured
            continue
        assert flow.shape == (1, hB, wB, 2) and match.shape == (1, hB, wB, 1)
        yb, xb = YB.astype(np.int64), XB.astype(np.int64)
        ex = ((flow[0, :, :, 0] + 1) * 0.5 * (wA - 1)).numpy()[yb, xb]
        ey = ((flow[0, :, :, 1] + 1) * 0.5 * (hA - 1)).numpy()[yb, xb]
        XA = (ex + rng.randn(K) * 5).astype(np.float32)            # near the estimate: the tally is neither all 0 nor all K
        YA = (ey + rng.randn(K) * 5).astype(np.float32)
        out.update({"p%d_XA" % b: XA, "p%d_YA" % b: YA, "p%d_XB" % b: XB, "p%d_YB" % b: YB, "p%d_xa" % b: ex, "p%d_ya" % b: ey,
                    "p%d_m" % b: match.numpy()[0, yb, xb, 0]})
        inside = ((flow[..., 0:1] >= -1) & (flow[..., 0:1] <= 1) & (flow[..., 1:2] >= -1) & (flow[..., 1:2] <= 1)).float()
        for t, th in enumerate(THS):
            # the mask the script's loop hands to alignmentError (:281-282)
            mask = (match >= th).float() * inside if th > 0 else torch.ones(match.size())
            c, nb = f["alignmentError"](wB, hB, wA, hA, XA, YA, XB, YB, flow, mask, grid)
            counts[t, b], nbAlign[t, b] = c, nb
        print("pair %d (%dx%d, nbH %d): nbAlign %s, counts at t=0 %s" % (b, hB, wB, n, nbAlign[:, b], counts[0, b]))
    assert 0 < nbAlign[2, 0] + nbAlign[2, 1] < nbAlign[1, 0] + nbAlign[1, 1] < 2 * K
    out.update(counts=counts, nbAlign=nbAlign)
    rng = np.random.RandomState(9)
    rs = dict(rs_sizes=np.asarray(RESIZE), rs_min=np.asarray([480, 480, 240, 480, 480, 480]))
    xs, ys, news, ox, oy, ov = [], [], [], [], [], []
    for (w, h), ms in zip(RESIZE, rs["rs_min"]):
        x, y = (rng.rand(12) * 1.3 * w - 0.15 * w).round(3), (rng.rand(12) * 1.3 * h - 0.15 * h).round(3)
        sx, sy = ";".join(repr(float(v)) for v in x), ";".join(repr(float(v)) for v in y)
        I = Image.new("RGB", (w, h))
        I1, x1, y1 = f["ResizeMinResolution"](int(ms), I, sx, sy, 16)
        I2, x2, y2, valid = f["ResizeMinResolution_megadepth"](int(ms), I, sx, sy, 16)
        assert I1.size == I2.size and np.array_equal(x1, x2) and np.array_equal(y1, y2) and x1.dtype == np.float32
        xs.append(x); ys.append(y); news.append(I1.size); ox.append(x1); oy.append(y1); ov.append(valid)
    rs.update(rs_x=np.asarray(xs), rs_y=np.asarray(ys), rs_new=np.asarray(news), rs_outx=np.asarray(ox), rs_outy=np.asarray(oy),
              rs_valid=np.asarray(ov))
    out.update(rs)
    path = os.path.join(HERE, "corr_records.npz")
    np.savez_compressed(path, **out)
    print("corr_records.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
