"""Generates tests/golden/points.npz by running the REAL reference's own functions (compiled from where they lie by
oracle/ref_loader.script_functions; nothing of their text is copied): ``_getFlow`` and ``matches_from_flow`` of
evaluation/evalYFCC/getResults.py, ``alignmentError`` of evaluation/evalCorr/getResults.py.  Authoring container only.

    python tests/golden/make_golden_points.py

What is stored (data only):
    seed, n, hd, wd            the synth.assembly_arrays case of assemble.npz (3 homographies, 80 x 112 maps)
    bg                         matchBG = RandomState(3).rand(80, 112) < 0.8, bit-packed
    case{c}_cfg                (th, multiH) of case c = 0, 1, 2
    case{c}_flow / _binary     the reference's flowGlobal (80,112,2) float32 and match_binary (bit-packed) -- _getFlow's returns.
                               The single-homography case (the last) is stored as it is, the others as the XOR of their int32 bit
                               patterns with it (case{c}_flow_xor: zero wherever homography 0 owns the pixel; lossless, and it
                               keeps the file small)
    angles, sizeA, sizeB       per angle index a: the angle, (wA, hA), (wB, hB) -- the unrotated target: (112, 80) at 0 / 180,
                               (80, 112) at 90 / 270, so that the rotated grid has the maps' shape (80,112)
    case{c}_a{a}_n / _sha1 / _sha2   rows, and the SHA-256 of the bytes of the reference's pts1 (float32) / pts2 (int64): twelve full
                               point lists would be several times the maps they come from
    full_case, full_angle, full_pts1, full_pts2    one combination in full (pts2 as int16), so that a failing digest has rows to look at
    ae_*                       one alignmentError call: its inputs, counts and nbAlign; ae_none_*: the same maps with match <= 0.5
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))

import ref_loader  # noqa: E402
from rfx import synth  # noqa: E402

CASES = ((0.5, True), (0.95, True), (0.5, False))
ANGLES = (0, 90, 180, 270)
SIZE_A = ((640, 480), (1920, 1080), (97, 211), (4096, 2))       # wA - 1 = 639, 1919 (odd), 96, 4095; width != height


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    fy = ref_loader.script_functions("evaluation/evalYFCC/getResults.py", ["_getFlow", "matches_from_flow"])
    fc = ref_loader.script_functions("evaluation/evalCorr/getResults.py", ["alignmentError"])
    src = np.load(os.path.join(HERE, "assemble.npz"))
    seed, n, hd, wd = (int(src[k]) for k in ("seed", "n", "hd", "wd"))
    flowDown, _, param, md = synth.assembly_arrays(seed, n, hd, wd)
    H, W = hd * 8, wd * 8
    bg = np.random.RandomState(3).rand(H, W) < 0.8
    out = dict(seed=seed, n=n, hd=hd, wd=wd, bg=np.packbits(bg), angles=np.asarray(ANGLES), sizeA=np.asarray(SIZE_A),
               sizeB=np.asarray([(W, H) if (a // 90) % 2 == 0 else (H, W) for a in ANGLES]))
    flows = []
    for c, (th, multiH) in enumerate(CASES):
        with torch.no_grad():
            flow, binary = fy["_getFlow"](torch.from_numpy(flowDown), torch.from_numpy(param), torch.from_numpy(md), bg, multiH, th)
        assert flow.shape == (H, W, 2) and flow.dtype == np.float32 and binary.shape == (H, W) and binary.dtype == bool
        assert 0 < binary.sum() < binary.size
        out["case%d_cfg" % c] = np.asarray([th, float(multiH)])
        flows.append(flow)
        out["case%d_binary" % c] = np.packbits(binary)
        for a, angle in enumerate(ANGLES):
            pts1, pts2 = fy["matches_from_flow"](flow, binary, tuple(SIZE_A[a]), tuple(int(v) for v in out["sizeB"][a]), angle)
            assert pts1.dtype == np.float32 and pts2.dtype == np.int64 and len(pts1) == len(pts2) == binary.sum()
            out["case%d_a%d_n" % (c, a)] = np.asarray(len(pts1))
            out["case%d_a%d_sha1" % (c, a)] = np.asarray(sha(pts1))
            out["case%d_a%d_sha2" % (c, a)] = np.asarray(sha(pts2))
            if (c, a) == (1, 1):
                out.update(full_case=np.asarray(c), full_angle=np.asarray(a), full_pts1=pts1, full_pts2=pts2.astype(np.int16))
        print("case %d: th %.2f multiH %s -> %d of %d pixels kept (%.1f %%)" % (c, th, multiH, binary.sum(), binary.size,
                                                                              100.0 * binary.mean()))
    assert CASES[-1][1] is False
    out["case%d_flow" % (len(CASES) - 1)] = flows[-1]
    for c in range(len(CASES) - 1):
        out["case%d_flow_xor" % c] = flows[c].view(np.int32) ^ flows[-1].view(np.int32)
    # alignmentError: 40 float keypoints on a 48 x 64 map, about half of them on match <= 0.5
    rng = np.random.RandomState(5)
    hB, wB, wA, hA, K = 48, 64, 301, 200, 40
    flow = torch.from_numpy((rng.rand(1, hB, wB, 2) * 2 - 1).astype(np.float32))
    match2 = torch.from_numpy(rng.rand(1, hB, wB, 1).astype(np.float32))
    XB, YB = (rng.rand(K) * wB).astype(np.float32), (rng.rand(K) * hB).astype(np.float32)
    est = flow.numpy()[0, YB.astype(np.int64), XB.astype(np.int64)]
    XA = ((est[:, 0] + 1) * 0.5 * (wA - 1) + rng.randn(K) * 6).astype(np.float32)      # near the estimate: the tally is not all 0 or K
    YA = ((est[:, 1] + 1) * 0.5 * (hA - 1) + rng.randn(K) * 6).astype(np.float32)
    grid = np.around(np.logspace(0, np.log10(36), 8).reshape(-1, 8))
    counts, nb = fc["alignmentError"](wB, hB, wA, hA, XA, YA, XB, YB, flow, match2, grid)
    none_counts, none_nb = fc["alignmentError"](wB, hB, wA, hA, XA, YA, XB, YB, flow, match2 * 0.5, grid)
    assert 0 < nb < K and none_nb == 0 and 0 < counts[0] and counts[-1] <= nb
    out.update(ae_dims=np.asarray([wB, hB, wA, hA]), ae_flow=flow.numpy(), ae_match=match2.numpy(), ae_XA=XA, ae_YA=YA, ae_XB=XB,
               ae_YB=YB, ae_grid=grid, ae_counts=counts, ae_nb=np.asarray(nb), ae_none_counts=none_counts,
               ae_none_nb=np.asarray(none_nb))
    print("alignmentError: %d of %d keypoints kept, counts %s" % (nb, K, counts))
    path = os.path.join(HERE, "points.npz")
    np.savez_compressed(path, **out)
    print("points.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
