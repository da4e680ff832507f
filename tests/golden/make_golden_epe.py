"""Generates tests/golden/epe.npz by running the REAL reference's own functions (compiled from where they lie by
oracle/ref_loader.script_functions; nothing of their text is copied): ``getGT`` and ``epe`` of evaluation/evalHpatch/getResults.py.
Authoring container only.

    python tests/golden/make_golden_epe.py

getGT reads the target image's shape through cv2 (absent here) and a row of a pandas table: a stand-in cv2 is seated in the
function's globals, the row is built with pandas.  What is stored (data only), one row per case:
    kind      "identity" | "shift" | "dyadic" | "perspective"
    H         the ground-truth homography (3,3) float64 handed to getGT
    shapes    h_ref, w_ref, h_trg, w_trg, S (= minSize)
    Hinv      rfx.assemble.hpatch_gt_homography(H, ref_hw, trg_hw, S)[1], (9,) float64 -- the calls of getGT:107-117
    sha       the SHA-256 of the bytes of getGT's grid_gt (S,S,2) float32
    seed      seed of the estimate test_epe_cpu.flow_est_for(seed, S)
    aepe      the reference's epe of that estimate over the pixels the ground truth keeps (float32)
    inside    the number of those pixels
and grid17 (n,17,17,2): grid_gt itself for the cases of the smallest size, in case order (24 full maps would be ten times the rest).
The float64 product of getGT goes through BLAS, whose last bit depends on the build; after the rounding to float32 the documented
order (tests/test_epe_cpu.rule_grid_gt) must give the stored grid bit for bit: asserted here for every case, a perspective seed
that fails is skipped.  The kinds: the identity; shifts by one pixel; homographies whose entries, and whose inverse's, are small
dyadic numbers (every float64 product and sum exact); seeded perspective ones that push a third to two thirds of the pixels out."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ransac-flow_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ref_loader  # noqa: E402
from rfx import assemble  # noqa: E402
import test_epe_cpu as T  # noqa: E402

SIZES = (17, 24, 33)


def dyadic(a):
    return np.array_equal(a * 4096, np.round(a * 4096)) and np.abs(a).max() < 64


def fixed_cases(S):
    eye = np.eye(3)
    sh = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
    yield "identity", eye, (S, S), (S, S)
    yield "shift", sh(1, 0), (S, S), (S, S)
    yield "shift", sh(0, -1), (S, S), (S, S)
    yield "shift", sh(-1, 1), (4 * S, 2 * S), (4 * S, 2 * S)          # one pixel of the ORIGINAL images: a half / a quarter here
    yield "dyadic", np.array([[1, 0.5, -2], [0, 1, 3], [0, 0, 1]], np.float64), (2 * S, 4 * S), (S, 2 * S)
    yield "dyadic", np.array([[2, 0, 1.5], [-0.25, 0.5, 0.75], [0, 0, 1]], np.float64), (S, S), (8 * S, S)


def main():
    fh = ref_loader.script_functions("evaluation/evalHpatch/getResults.py", ["getGT", "epe"])
    rows, c = [], 0

    def run(kind, H, ref_hw, trg_hw, S, seed):
        T.seat_cv2(fh["getGT"], np.empty(tuple(trg_hw) + (3,), np.uint8))
        grid = fh["getGT"](T.reference_row(H, ref_hw), 0, S, "/nowhere")
        assert tuple(grid.shape) == (1, S, S, 2) and grid.dtype == torch.float32
        Hinv = assemble.hpatch_gt_homography(H, ref_hw, trg_hw, S)[1].reshape(9)
        gx, gy = T.rule_grid_gt(Hinv, S, S)
        if not (np.array_equal(T.bits(gx), T.bits(grid[0, :, :, 0].numpy())) and np.array_equal(T.bits(gy), T.bits(grid[0, :, :, 1].numpy()))):
            return None
        aepe, n = T.reference_aepe(fh["epe"], grid, T.flow_est_for(seed, S))
        return dict(kind=np.asarray(kind), H=np.asarray(H, np.float64), shapes=np.asarray(list(ref_hw) + list(trg_hw) + [S]), Hinv=Hinv,
                    sha=np.asarray(T.sha(grid[0].numpy())), seed=np.asarray(seed), aepe=aepe.numpy(), inside=np.asarray(n),
                    grid=grid[0].numpy())

    for S in SIZES:
        for kind, H, ref_hw, trg_hw in fixed_cases(S):
            r = run(kind, H, ref_hw, trg_hw, S, 1000 + c)
            assert r is not None, (kind, S)                           # exact arithmetic: no BLAS can differ
            if kind != "perspective":
                assert dyadic(r["Hinv"]), (kind, r["Hinv"])
            rows.append(r)
            print("case %2d  S %2d  %-11s inside %4d / %4d  aepe %.6f" % (c, S, kind, int(r["inside"]), S * S, float(r["aepe"])))
            c += 1
        found, seed = 0, 0
        while found < 2:
            seed += 1
            rng = np.random.RandomState(7000 + 100 * S + seed)
            ref_hw, trg_hw = tuple(int(x) for x in rng.randint(200, 900, 2)), tuple(int(x) for x in rng.randint(200, 900, 2))
            H = np.eye(3) + rng.randn(3, 3) * np.array([[0.3, 0.3, 150], [0.3, 0.3, 150], [4e-4, 4e-4, 0]])
            r = run("perspective", H, ref_hw, trg_hw, S, 1000 + c)
            if r is None or not S * S / 3 <= int(r["inside"]) <= 2 * S * S / 3:
                continue
            rows.append(r)
            print("case %2d  S %2d  perspective (seed %d) inside %4d / %4d  aepe %.6f" % (c, S, seed, int(r["inside"]), S * S, float(r["aepe"])))
            c += 1
            found += 1
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0] if k != "grid"}
    out["grid17"] = np.stack([r["grid"] for r in rows if r["grid"].shape[0] == SIZES[0]])
    path = os.path.join(HERE, "epe.npz")
    np.savez_compressed(path, **out)
    print("epe.npz: %d cases, %d bytes" % (c, os.path.getsize(path)))


if __name__ == "__main__":
    main()
