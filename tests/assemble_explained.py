"""Which pixels of an assembled flow may legitimately differ between the device and the CPU reference (tests/test_gpu_assemble.py).

The assembly is continuous in its inputs except at two comparisons: ``score_i >= th`` (who owns the pixel) and ``-1 <= flow_i <= 1``
(the in-bounds factor of the score).  The device composes flows and scores in float32 with its own operation order, so a pixel
whose score lies within rounding of th, or whose flow lies within rounding of +-1, may fall on the other side there -- and ONLY
such a pixel may.  The float64 run of the same expression (restate.assemble_terms(dtype=float64)) names these pixels:

    (a) |score_i - th| <= margin_s for some homography i the merge looks at, or
    (b) ||flow_i,c| - 1| <= margin_f for some such i and component c.

Each margin is 4x the largest disagreement between the float32 and the float64 restatement on the same inputs (scores for (a), over
the pixels whose in-bounds factor agrees; flows for (b)): measured on the CPU from the reference alone, never from the device's
output; the factor leaves room for the device's differently ordered but equally rounded arithmetic, as in the project's other
measured bounds.  MEASURED holds the disagreements (2026-10-20, profiles/assemble_explained.json; tests/test_assemble_explained_cpu.py
checks that this host's stay within the margins and that the share of excusable pixels stays within each comparison's cap).

KITTI adds two consumers downstream of the comparisons.  With cc_th > 0 a flip of ``score_i > 0.99`` or of the in-bounds factor
changes a connected component's area: the may-flip pixels themselves, and every piece of ``(score_i > 0.99) & ~may_flip_i`` that
is small enough to be removed on its own but lies in a component of ``(score_i > 0.99) | may_flip_i`` large enough to be kept, may
be removed or kept.  With interpolate an unexplained pixel copies its nearest explained one: it may differ if that pixel is excusable,
or if an excusable pixel (which may become explained) lies at most as far away."""
import numpy as np
import torch

import restate
from rfx import synth

FACTOR = 4.0
CC_MATCH_TH = 0.99

# case -> (largest |score32 - score64| where the in-bounds factors agree, largest |flow32 - flow64|), measured 2026-10-20
MEASURED = {
    (21, 1, 9, 13, (61, 83), False, False): (1.764e-07, 6.615e-06),
    (22, 5, 9, 13, (72, 104), True, False): (9.332e-06, 1.032e-05),
    (23, 11, 9, 13, (61, 83), False, False): (3.131e-07, 7.852e-06),
    (24, 5, 7, 11, (57, 87), True, False): (7.070e-06, 7.889e-06),
    (27, 3, 9, 13, (61, 83), True, False): (6.763e-06, 5.714e-06),
    (11, 3, 10, 14, (72, 100), False, False): (3.237e-07, 6.603e-06),        # tests/golden/assemble.npz: hpatch
    (11, 3, 10, 14, (80, 112), True, False): (7.360e-06, 9.166e-06),         # ... corr
    (11, 3, 10, 14, (80, 112), True, True): (7.360e-06, 8.878e-06),          # ... kitti
}

# every comparison of tests/test_gpu_assemble.py that carries the rule: name -> (case, th, multiH, cc_th, interpolate, cap), the
# cap being the share of VALUES the comparison lets differ (its max_bad)
ORACLE_CASES = {
    "oracle-21": ((21, 1, 9, 13, (61, 83), False, False), 0.45),
    "oracle-22": ((22, 5, 9, 13, (72, 104), True, False), 0.2),
    "oracle-23": ((23, 11, 9, 13, (61, 83), False, False), 0.45),
    "oracle-odd-24": ((24, 5, 7, 11, (57, 87), True, False), 0.2),
    "oracle-odd-27": ((27, 3, 9, 13, (61, 83), True, False), 0.2),
}


def comparisons(golden):
    """golden: the loaded tests/golden/assemble.npz."""
    out = {k: (c, th, True, 0.0, False, 0.002) for k, (c, th) in ORACLE_CASES.items()}
    seed, n, hd, wd = (int(golden[k]) for k in ("seed", "n", "hd", "wd"))
    for tag in "abc":
        th, multiH, oh, ow = golden["hpatch_%s_cfg" % tag]
        out["golden-hpatch-" + tag] = (golden_case("hpatch", seed, n, hd, wd, (int(oh), int(ow))), float(th), bool(multiH), 0.0, False,
                                       0.002)
        th, multiH = golden["corr_%s_cfg" % tag]
        out["golden-corr-" + tag] = (golden_case("corr", seed, n, hd, wd), float(th), bool(multiH), 0.0, False, 0.002)
    for tag in "abcd":
        th, cc, interp, multiH = golden["kitti_%s_cfg" % tag]
        out["golden-kitti-" + tag] = (golden_case("kitti", seed, n, hd, wd), float(th), bool(multiH), float(cc), bool(interp), 0.01)
    return out


def case_inputs(case):
    """case = (seed, n, hd, wd, out_hw, cycle, kitti) -> dict of tensors."""
    seed, n, hd, wd, out_hw, cycle, kitti = case
    fd, fd2, pm, md = synth.assembly_arrays(seed, n, hd, wd)
    t = torch.from_numpy
    return dict(flowDown=t(fd), param=t(pm), matchDown=t(md), out_hw=tuple(out_hw), cycle=cycle,
                flowd2Down=t(fd2) if kitti else None)


def terms(case, dtype):
    return restate.assemble_terms(**case_inputs(case), dtype=dtype)


def disagreement(case):
    """-> (ds, df): float32 vs float64 restatement, scores (where the in-bounds factors agree) and flows."""
    f32, s32, b32 = terms(case, torch.float32)
    f64, s64, b64 = terms(case, torch.float64)
    same = b32.double() == b64
    ds = float((s32.double() - s64).abs()[same].max()) if bool(same.any()) else 0.0
    df = float((f32.double() - f64).abs().max())
    return ds, df


def margins(case):
    ds, df = MEASURED[case]
    return FACTOR * ds, FACTOR * df


def _label8(binary):
    from scipy import ndimage
    return ndimage.label(binary, structure=np.ones((3, 3), dtype=np.int32))[0]


def excusable(case, th, multiH, cc_th=0.0, interpolate=False):
    """(H,W) bool tensor: the pixels at which a value of the assembled result may differ from the reference's."""
    ms, mf = margins(case)
    flow, score, _ = terms(case, torch.float64)
    last = flow.shape[0] if multiH else 1
    edge = ((flow.abs() - 1).abs() <= mf).any(dim=3)                        # (b), per homography
    may = ((score - th).abs() <= ms) | edge                                 # (a) | (b)
    if cc_th > 0:
        cand = ((score - CC_MATCH_TH).abs() <= ms) | edge
        for i in range(last):
            c = cand[i].numpy()
            if not c.any():
                continue
            # whatever the may-flip pixels do, a component is a union of pieces of `sure` plus some of them: a piece that is large
            # enough on its own is always kept, a piece inside a largest-possible component that is still small is always removed
            sure = (score[i] > CC_MATCH_TH).numpy() & ~c
            piece, whole = _label8(sure), _label8(sure | c)
            piece_small = (np.bincount(piece.ravel()) / piece.size <= cc_th)[piece] & sure
            whole_large = (np.bincount(whole.ravel()) / whole.size > cc_th)[whole]
            may[i] |= torch.from_numpy(c | (piece_small & whole_large))
    E = may[:last].any(dim=0)
    if interpolate and bool(E.any()):
        from scipy import ndimage
        a = case_inputs(case)
        found = restate.assemble_flow_kitti(a["flowd2Down"], a["flowDown"], a["param"], a["matchDown"], a["out_hw"], th, multiH, cc_th,
                                            False)[2][0].numpy()                # the reference's explained mask
        e = E.numpy()
        d_e = ndimage.distance_transform_edt(~e)
        if found.any():
            d_f, idx = ndimage.distance_transform_edt(~found, return_indices=True)
            E = torch.from_numpy(e | (~found & ((d_e <= d_f) | e[tuple(idx)])))
        else:
            E = torch.ones_like(E)                                          # no explained pixel at all: any flip fills the map
    return E


def unexplained(dev_value, ref_value, E, tol):
    """Number of pixels outside E at which some value differs by more than tol (or one side is not finite), and the number of
    differing pixels overall.  Values are (1,H,W) or (1,H,W,C)."""
    d = (torch.as_tensor(dev_value).cpu().double() - torch.as_tensor(ref_value).double()).abs()
    d = d.reshape(E.shape[0], E.shape[1], -1)
    differs = ~(d <= tol).all(dim=2)
    return int((differs & ~E).sum()), int(differs.sum())


# the cases of tests/test_gpu_assemble.py: (seed, n, hd, wd, out_hw, cycle, kitti)
def oracle_case(seed, n, cycle, hd=9, wd=13, out_hw=None):
    return (seed, n, hd, wd, tuple(out_hw) if out_hw else ((hd * 8, wd * 8) if cycle else (61, 83)), cycle, False)


def golden_case(kind, seed, n, hd, wd, out_hw=None):
    """kind: "hpatch" (out_hw given, no cycle), "corr" (8x, cycle), "kitti" (8x, two-level)."""
    if kind == "hpatch":
        return (seed, n, hd, wd, tuple(out_hw), False, False)
    return (seed, n, hd, wd, (hd * 8, wd * 8), True, kind == "kitti")
