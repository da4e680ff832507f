"""The host side of the "every excused pixel must be explained" rule of tests/test_gpu_assemble.py (tests/assemble_explained.py):
the recorded float32-vs-float64 disagreements still bound this host's, the pixels the rule can excuse stay within each comparison's
cap, and the rule holds where no device is involved -- the float32 restatement against the reference's own golden outputs."""
import os

import numpy as np
import pytest
import torch

import assemble_explained as ae
import restate

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assemble.npz"))
COMPARISONS = ae.comparisons(GOLD)
TOL = 1e-4


@pytest.mark.parametrize("case", sorted(ae.MEASURED), ids=str)
def test_recorded_disagreements_bound_this_hosts(case):
    """The margins are 4x the recorded figures; another host's libm or vector width may move the float32 run by an ulp or two, not
    by a factor."""
    ds, df = ae.disagreement(case)
    ms, mf = ae.margins(case)
    assert 0 < ae.MEASURED[case][0] and 0 < ae.MEASURED[case][1]
    assert ds <= 2 * ae.MEASURED[case][0] < ms and df <= 2 * ae.MEASURED[case][1] < mf, (ds, df, ae.MEASURED[case])
    assert ms < TOL and mf < TOL                      # an excusable pixel is decided by something far finer than the tolerance


@pytest.mark.parametrize("name", sorted(COMPARISONS))
def test_share_of_excusable_pixels_is_within_the_cap(name):
    case, th, multiH, cc_th, interp, cap = COMPARISONS[name]
    E = ae.excusable(case, th, multiH, cc_th, interp)
    assert tuple(E.shape) == tuple(case[4])
    assert float(E.float().mean()) <= cap, (name, float(E.float().mean()), cap)


def test_float32_and_float64_restatement_disagree_on_no_unexcused_pixel():
    """merge on the float64 terms against the float32 restatement: every pixel that differs by more than TOL is excusable."""
    for name, (case, th, multiH, cc_th, interp, cap) in COMPARISONS.items():
        if cc_th > 0 or interp or case[6]:
            continue
        a = ae.case_inputs(case)
        f32 = restate.assemble_flow(a["flowDown"], a["param"], a["matchDown"], a["out_hw"], th, multiH, a["cycle"])
        flow, score, _ = ae.terms(case, torch.float64)
        f64 = restate.merge_multi_h(flow.clamp(-1, 1), score, th, multiH)
        E = ae.excusable(case, th, multiH)
        for x, y, what in zip(f32, f64, ("flow", "match", "binary")):
            assert ae.unexplained(x.double(), y.double(), E, TOL)[0] == 0, (name, what)


def test_restatement_against_the_reference_golden_differs_only_at_excusable_pixels():
    t = torch.from_numpy
    seed, n, hd, wd = (int(GOLD[k]) for k in ("seed", "n", "hd", "wd"))
    from rfx import synth
    fd, fd2, pm, md = synth.assembly_arrays(seed, n, hd, wd)
    for tag in "abc":
        case, th, multiH, _, _, _ = COMPARISONS["golden-hpatch-" + tag]
        rf = restate.assemble_flow(t(fd), t(pm), t(md), case[4], th, multiH, False)[0]
        assert ae.unexplained(rf, GOLD["hpatch_" + tag], ae.excusable(case, th, multiH), TOL)[0] == 0
        case, th, multiH, _, _, _ = COMPARISONS["golden-corr-" + tag]
        rf, rm, _ = restate.assemble_flow(t(fd), t(pm), t(md), case[4], th, multiH, True)
        E = ae.excusable(case, th, multiH)
        assert ae.unexplained(rf, GOLD["corr_%s_flow" % tag], E, TOL)[0] == 0
        assert ae.unexplained(rm, GOLD["corr_%s_match" % tag][..., 0], E, TOL)[0] == 0
    for tag in "abcd":
        case, th, multiH, cc_th, interp, _ = COMPARISONS["golden-kitti-" + tag]
        rf = restate.assemble_flow_kitti(t(fd2), t(fd), t(pm), t(md), case[4], th, multiH, cc_th, interp)[0]
        assert ae.unexplained(rf, GOLD["kitti_" + tag], ae.excusable(case, th, multiH, cc_th, interp), TOL)[0] == 0


def test_the_rule_rejects_a_wrong_corner_and_a_short_wrong_border_run():
    """What the caps alone let through (ten values at 61 x 83): a wrong corner pixel, a run of four wrong pixels on the last row."""
    case, th = ae.ORACLE_CASES["oracle-23"]
    a = ae.case_inputs(case)
    rf = restate.assemble_flow(a["flowDown"], a["param"], a["matchDown"], a["out_hw"], th, True, False)[0]
    E = ae.excusable(case, th, True)
    H, W = case[4]
    assert not bool(E[H - 1, W - 5:].any()) and not bool(E[0, 0])
    for sl in ((0, slice(0, 1)), (H - 1, slice(W - 4, W))):
        wrong = rf.clone()
        wrong[0, sl[0], sl[1]] += 3e-4
        assert float(((wrong - rf).abs() > TOL).float().mean()) <= 0.002          # within the cap ...
        assert ae.unexplained(wrong, rf, E, TOL)[0] == sl[1].stop - sl[1].start    # ... and still caught
