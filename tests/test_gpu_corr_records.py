"""The Corr results step of a whole batch from its device records, without the dense maps (csrc/keypoints.hip).
ops.records_keypoints (rfx_records_keypoints_f32) against ops.assemble_records followed by ops.sample_points and reads of
matchGlobal / binary at the same pixels: BIT PATTERNS, NaN payloads included, at every pixel of every map.  ops.pck_tally
(rfx_pck_tally_f64) against the numpy rule tests/test_corr_records_cpu.py pins to the reference's outputs: counts, nb and the float64
distances bit for bit.  assemble.corr_keypoints_records against the reference's golden tallies and, on records a driver filled,
against assemble.corr_alignment_error per pair on the assembled maps.  No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

from rfx import assemble, ops, synth, weights
from rfx.pipeline import AlignPipeline
from test_corr_records_cpu import golden, rule_tally
from test_gpu_assemble_records import _dense, _fill, _ragged, _random_pair

pytestmark = pytest.mark.gpu
NAN = float("nan")
MAX_H = 4
THS = (0.0, 0.5, 0.9)


# ---------------------------------------------------------------- helpers

def _i32(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _all_pixels(H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return xx.reshape(-1), yy.reshape(-1)


def _want(R, th, multiH, cycle, xb, yb, sizesA, out_hw=None, bg=None):
    """The yardstick: the dense maps of every pair (one assembly launch), then per pair sample_points and reads of matchGlobal,
    binary and the flow's range at the keypoints truncated toward zero -> (xa, ya, m, flag) of all pairs, pair after pair."""
    fg, mg, b, _ = ops.assemble_records(R, th, multiH, cycle, out_hw=out_hw, bg=bg)
    outs = ([], [], [], [])
    for k in range(R.B):
        x = torch.from_numpy(np.asarray(xb[k]).astype(np.int64).reshape(-1)).to(fg[k].device)
        y = torch.from_numpy(np.asarray(yb[k]).astype(np.int64).reshape(-1)).to(fg[k].device)
        xa, ya, _ = ops.sample_points(fg[k], mg[k], x, y, sizesA[k])
        f = fg[k][y, x]
        inside = ((f >= -1) & (f <= 1)).all(dim=1)
        for o, v in zip(outs, (xa, ya, mg[k][y, x], b[k][y, x].to(torch.uint8) | (inside.to(torch.uint8) << 1))):
            o.append(v)
    return tuple(torch.cat(o) for o in outs)


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("xa", "ya", "m", "flag")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert torch.equal(_i32(g), _i32(w)), (what, name, int((_i32(g) != _i32(w)).sum()))


SIZES_A = [(301, 200), (97, 211), (640, 480), (33, 1000), (1920, 1080)]     # wA != hA everywhere
DENSE_NBH = (1, 2, MAX_H, 0, 3)
RAGGED = ((3, 4, 2), (5, 3, 1), (2, 2, MAX_H), (6, 8, 0), (4, 4, 3))         # (h8, w8, nbH); 768 + 960 + 256 + 3072 + 1024 pixels


@pytest.fixture(scope="module")
def dense_pairs():
    g = torch.Generator().manual_seed(201)
    return [_random_pair(g, n, 3, 4) if n else None for n in DENSE_NBH]


@pytest.fixture(scope="module")
def ragged_pairs():
    g = torch.Generator().manual_seed(202)
    return [_random_pair(g, max(n, 1), h, w) for h, w, n in RAGGED]


def _ragged5(pairs, dev):
    """Ragged records of RAGGED; the pair with nbH = 0 keeps its size and gets no homography."""
    R = ops.MultiHRecordsRagged([p[0] for p in RAGGED], [p[1] for p in RAGGED], dev, max_h=MAX_H)
    for b, (pair, (_, _, n)) in enumerate(zip(pairs, RAGGED)):
        nbH, _, Hs, f8, m8 = R.views(b)
        _fill((nbH, Hs, f8, m8), pair if n else None, dev)
    return R


# ---------------------------------------------------------------- 1. the keypoints kernel = assembly + sampling, at every pixel

@pytest.mark.parametrize("cycle", [False, True])
@pytest.mark.parametrize("multiH", [False, True])
def test_dense_records_every_pixel(dev, dense_pairs, cycle, multiH):
    th = 0.15 if cycle else 0.35
    R = _dense(dense_pairs, 3, 4, dev, max_h=MAX_H)
    px = [_all_pixels(24, 32)] * 5
    xb, yb = [p[0] for p in px], [p[1] for p in px]
    got = ops.records_keypoints(R, th, multiH, cycle, xb, yb, sizesA=SIZES_A)
    assert got[4] == [768 * b for b in range(6)] and got[0].numel() == 3840        # fifteen 256-thread blocks
    want = _want(R, th, multiH, cycle, xb, yb, SIZES_A)
    _assert_same(got[:4], want, ("dense", cycle, multiH))
    flag = got[3].view(5, 768)
    assert bool((flag[0] & 1).any()) and not bool((flag[0] & 1).all())             # one homography: explained in part
    assert flag[3].tolist() == [2] * 768 and not bool(got[2].view(5, 768)[3].any())   # nbH = 0: zero maps, a finite flow
    assert torch.equal(got[0].view(5, 768)[3], torch.full((768,), 0.5 * 32, device=dev))       # ((0 + 1) * 0.5) * (33 - 1)
    if multiH and not cycle:
        single = ops.records_keypoints(R, th, False, cycle, xb, yb, sizesA=SIZES_A)
        assert not torch.equal(_i32(single[0]), _i32(got[0])), "no pixel is owned by a homography i >= 1"


@pytest.mark.parametrize("cycle", [False, True])
def test_ragged_records_every_pixel(dev, ragged_pairs, cycle):
    th = 0.15 if cycle else 0.35
    R = _ragged5(ragged_pairs, dev)
    px = [_all_pixels(8 * h, 8 * w) for h, w, _ in RAGGED]
    xb, yb = [p[0] for p in px], [p[1] for p in px]
    got = ops.records_keypoints(R, th, True, cycle, xb, yb, sizesA=SIZES_A)
    assert got[4] == [0, 768, 1728, 1984, 5056, 6080]
    _assert_same(got[:4], _want(R, th, True, cycle, xb, yb, SIZES_A), ("ragged", cycle))
    # the same pairs at other positions of the batch, through rows(): slices of the same storage
    for lo, hi in ((1, 4), (0, 1), (4, 5), (2, 5)):
        part = ops.records_keypoints(R.rows(lo, hi), th, True, cycle, xb[lo:hi], yb[lo:hi], sizesA=SIZES_A[lo:hi])
        a, z = got[4][lo], got[4][hi]
        assert part[4] == [o - a for o in got[4][lo:hi + 1]]
        _assert_same(part[:4], tuple(t[a:z] for t in got[:4]), ("rows", lo, hi))
    D = _dense([ragged_pairs[0], ragged_pairs[0], None], 3, 4, dev, max_h=MAX_H).rows(1, 3)
    part = ops.records_keypoints(D, th, True, cycle, xb[:1] * 2, yb[:1] * 2, sizesA=SIZES_A[:2])
    _assert_same(part[:4], _want(D, th, True, cycle, xb[:1] * 2, yb[:1] * 2, SIZES_A[:2]), "dense rows")


def test_background_other_sizes_and_float_keypoints(dev, ragged_pairs):
    R = _ragged5(ragged_pairs, dev)
    sizes = [(27, 30), (16, 16), (1, 257), (48, 64), (9, 9)]
    g = torch.Generator().manual_seed(5)
    bg = [(torch.rand(s, generator=g) < 0.6).to(dev) for s in sizes]
    px = [_all_pixels(*s) for s in sizes]
    xb, yb = [p[0] for p in px], [p[1] for p in px]
    got = ops.records_keypoints(R, 0.35, True, False, xb, yb, sizesA=SIZES_A, out_hw=sizes, bg=bg)
    want = _want(R, 0.35, True, False, xb, yb, SIZES_A, out_hw=sizes, bg=bg)
    _assert_same(got[:4], want, "bg list")
    packed = torch.cat([t.reshape(-1) for t in bg])
    _assert_same(ops.records_keypoints(R, 0.35, True, False, xb, yb, sizesA=SIZES_A, out_hw=sizes, bg=packed)[:4], want, "bg packed")
    nobg = ops.records_keypoints(R, 0.35, True, False, xb, yb, sizesA=SIZES_A, out_hw=sizes)
    assert bool(((nobg[3] & 1) > (got[3] & 1)).any()) and not bool(((nobg[3] & 1) < (got[3] & 1)).any())
    # float keypoints with fractions are truncated toward zero (31.99 -> 31: rounding would leave the map), pairs without keypoints
    # first, in the middle and last
    rng = np.random.RandomState(6)
    fx = [np.zeros(0, np.float32), (rng.rand(300) * 24).astype(np.float32), np.zeros(0), np.concatenate(([63.99, 0.99, -0.9], rng.rand(97) * 64)),
          []]
    fy = [[], (rng.rand(300) * 40).astype(np.float32), np.zeros(0, np.float64), np.concatenate(([47.99, 0.5, -0.5], rng.rand(97) * 48)),
          np.zeros(0, np.int64)]
    got = ops.records_keypoints(R, 0.15, True, True, fx, fy, sizesA=SIZES_A)
    assert got[4] == [0, 0, 300, 300, 400, 400] and got[0].numel() == 400
    _assert_same(got[:4], _want(R, 0.15, True, True, fx, fy, SIZES_A), "float keypoints")
    none = ops.records_keypoints(R, 0.15, True, True, [[]] * 5, [[]] * 5, sizesA=SIZES_A)
    assert none[4] == [0] * 6 and all(t.numel() == 0 and t.is_cuda for t in none[:4])
    # the last keypoint of a pair and the first of the next, around empty pairs: one keypoint each
    one = ops.records_keypoints(R, 0.15, True, True, [[3], [], [7], [5], []], [[2], [], [9], [1], []], sizesA=SIZES_A)
    _assert_same(one[:4], _want(R, 0.15, True, True, [[3], [], [7], [5], []], [[2], [], [9], [1], []], SIZES_A), "single keypoints")


def test_scores_on_the_threshold_degenerate_homography_and_nan_payloads(dev, ragged_pairs):
    # (a) th placed exactly on scores of the maps, and one float32 step above
    R = _ragged5(ragged_pairs, dev)
    px = [_all_pixels(8 * h, 8 * w) for h, w, _ in RAGGED]
    xb, yb = [p[0] for p in px], [p[1] for p in px]
    base = ops.records_keypoints(R, 0.15, True, True, xb, yb, sizesA=SIZES_A)
    m1 = base[2][768:1728]                                         # the pair with ONE homography: m is score_0 everywhere
    score = float(m1[m1 > 0.05].median())
    for th in (score, float(np.nextafter(np.float32(score), np.float32(1)))):
        got = ops.records_keypoints(R, th, True, True, xb, yb, sizesA=SIZES_A)
        _assert_same(got[:4], _want(R, th, True, True, xb, yb, SIZES_A), ("on th", th))
        on = (got[2][768:1728].view(torch.int32) == torch.tensor(np.float32(score).view(np.int32).item(), device=dev))
        assert bool(on.any()) and bool(((got[3][768:1728][on] & 1) == (1 if th == score else 0)).all())
    # (b) a degenerate homography (z' = 0 across the image), NaN payloads in flow and matchability, an infinite entry
    g = torch.Generator().manual_seed(7)
    bad = [list(_random_pair(g, 3, 3, 4)), list(_random_pair(g, 2, 5, 3))]
    bad[0][1][0] = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0]])            # z' = x: zero on the centre column
    bad[0][0][1, 0, 1, 1] = NAN
    bad[0][2][2, 1, 0, 2] = torch.tensor(np.array([0x7fc12345], np.int32).view(np.float32))[0]
    bad[1][1][0] = torch.zeros(3, 3)
    bad[1][0][1, 1, 2, 1] = float("inf")
    bad[1][2][0, 0, 3, 1] = torch.tensor(np.array([0xffc00001], np.uint32).view(np.float32))[0]
    Rb = _ragged([tuple(p) for p in bad], dev, max_h=MAX_H)
    pxb = [_all_pixels(24, 32), _all_pixels(40, 24)]
    for cycle, th in ((True, 0.15), (False, 0.35)):
        got = ops.records_keypoints(Rb, th, True, cycle, [p[0] for p in pxb], [p[1] for p in pxb], sizesA=SIZES_A[:2])
        _assert_same(got[:4], _want(Rb, th, True, cycle, [p[0] for p in pxb], [p[1] for p in pxb], SIZES_A[:2]), ("nan", cycle))
        assert bool(torch.isnan(got[0]).any()) and bool(((got[3] & 2) == 0).any())


# ---------------------------------------------------------------- 2. the tally kernel = the numpy rule

KB = (0, 1, 255, 257, 700)


@pytest.fixture(scope="module")
def tally_case():
    """Five pairs of 0, 1, 255, 257 and 700 keypoints.  Estimates with fractions (a fused step in the distance shows in its last
    bit), integer offsets that land exactly on grid values, m on a threshold and one step below, NaN estimates, flags with bit 1
    clear on keypoints whose m passes."""
    rng = np.random.RandomState(11)
    K = sum(KB)
    koff = [0] + list(np.cumsum(KB))
    xs, ys = rng.randint(0, 640, K).astype(np.int64), rng.randint(0, 480, K).astype(np.int64)
    xa = (xs + rng.randn(K) * 9).astype(np.float32)
    ya = (ys + rng.randn(K) * 9).astype(np.float32)
    m = rng.rand(K).astype(np.float32)
    flag = np.full(K, 3, np.uint8)
    s = koff[3]                                                    # inside the pair of 257
    for i, (dx, dy) in enumerate(((3, 4), (-4, 3), (5, 12), (12, -5), (0, 1), (2, 0), (0, -3), (6, 8), (-8, 0), (36, 0), (0, 22))):
        xa[s + i], ya[s + i] = xs[s + i] + dx, ys[s + i] + dy       # d = 5, 5, 13, 13, 1, 2, 3, 10, 8, 36, 22 exactly
    m[s:s + 11] = 0.95
    below = lambda v: np.nextafter(np.float32(v), np.float32(0))
    m[s + 20:s + 26] = [0.5, below(0.5), 0.9, below(0.9), np.float32(0.9), np.float32(0.5)]
    xa[s + 20:s + 26] = xs[s + 20:s + 26] + 0.25                   # all of them inside the first grid value
    ya[s + 20:s + 26] = ys[s + 20:s + 26]
    flag[s + 30:s + 34] = [1, 0, 1, 0]                             # bit 1 clear with a finite, near estimate and a high m
    m[s + 30:s + 34] = 0.99
    xa[s + 30:s + 34] = xs[s + 30:s + 34] + 0.5
    ya[s + 30:s + 34] = ys[s + 30:s + 34]
    t = koff[4]
    xa[t + 5], ya[t + 9] = np.nan, np.nan                          # NaN flow: bit 1 clear, as the keypoints kernel sets it
    flag[t + 5] = flag[t + 9] = 1
    m[t + 5] = m[t + 9] = 0.99
    # a difference of a float32 and an integer below 2^15 or so has at most 25 significant bits, its square is exact in float64 and a
    # fused step changes nothing; small estimates far from their keypoints have differences of 40 and more bits, and there it shows
    xs[t + 100:t + 300], ys[t + 100:t + 300] = rng.randint(10000, 30000, 200), rng.randint(10000, 30000, 200)
    xa[t + 100:t + 300], ya[t + 100:t + 300] = rng.rand(200).astype(np.float32), rng.rand(200).astype(np.float32)
    m[t + 100:t + 300] = 0.99
    xa[koff[1]], ya[koff[1]], m[koff[1]] = xs[koff[1]] + 0.5, ys[koff[1]], 0.7       # the pair of one keypoint
    return dict(koff=koff, xa=xa, ya=ya, m=m, flag=flag, xs=xs, ys=ys)


def _tally(c, dev, order=None, **kw):
    """ops.pck_tally on the case (its pairs in ``order``) -> numpy (counts, nb, dist), and the rule's."""
    koff = c["koff"]
    order = list(range(len(koff) - 1)) if order is None else order
    idx = np.concatenate([np.arange(koff[b], koff[b + 1]) for b in order]).astype(np.int64)
    ko = [0] + list(np.cumsum([koff[b + 1] - koff[b] for b in order]))
    a = {k: c[k][idx] for k in ("xa", "ya", "m", "flag", "xs", "ys")}
    up = lambda v: torch.from_numpy(v).to(dev)
    split = lambda v: [v[ko[i]:ko[i + 1]] for i in range(len(order))]
    valid = kw.pop("valid", None)
    vd = None if valid is None else torch.tensor([valid[b] for b in order], dtype=torch.bool, device=dev)
    ths, grid = kw.get("match_ths", (0.0,)), kw.get("pixel_grid", None)
    got = ops.pck_tally(up(a["xa"]), up(a["ya"]), up(a["m"]), up(a["flag"]), split(a["xs"].astype(np.float64) + 0.75), split(a["ys"]), ko,
                        valid=vd, want_dist=True, **kw)
    want = rule_tally(a["xa"], a["ya"], a["m"], a["flag"], a["xs"], a["ys"], ko, ths, ops.pck_pixel_grid() if grid is None else grid,
                      valid=None if valid is None else [valid[b] for b in order])
    return tuple(t.cpu().numpy() for t in got), want, ko


def _assert_tally(got, want, what):
    assert got[0].dtype == got[1].dtype == np.int64 and got[2].dtype == np.float64
    assert np.array_equal(got[0], want[0]), (what, "counts", got[0].tolist(), want[0].tolist())
    assert np.array_equal(got[1], want[1]), (what, "nb", got[1].tolist(), want[1].tolist())
    nan = np.isnan(want[2])
    assert np.array_equal(np.isnan(got[2]), nan), (what, "dist: kept keypoints")
    assert np.array_equal(got[2][~nan].view(np.int64), want[2][~nan].view(np.int64)), (what, "dist bits")


def test_tally_equals_the_rule_bit_for_bit(dev, tally_case):
    got, want, ko = _tally(tally_case, dev, match_ths=THS)
    assert got[0].shape == (3, 5, 8) and got[1].shape == (3, 5) and got[2].shape == (3, sum(KB))
    _assert_tally(got, want, "M = 3, T = 8")
    assert want[1][0].tolist() == list(KB) and want[1][1, 1] == 1 and want[1][2, 1] == 0 and not want[0][:, 0].any()
    s = ko[3]
    assert got[2][0, s:s + 11].tolist() == [5, 5, 13, 13, 1, 2, 3, 10, 8, 36, 22]      # exactly on 1, 2, 3, 5, 8, 13, 22 and 36
    assert np.isnan(got[2][1, s + 21]) and got[2][1, s + 20] == 0.25 and np.isnan(got[2][2, s + 23]) and got[2][2, s + 22] == 0.25
    assert np.isnan(got[2][1:, s + 30:s + 34]).all() and (got[2][0, s + 30:s + 34] == 0.5).all()      # bit 1 counts above 0 only
    assert np.isnan(got[2][:, ko[4] + 5]).all() and want[1][0, 4] == 700                # a NaN is kept at 0 and counted under nothing
    # one threshold of the grid, a threshold below zero, seventeen minus one grid values
    for kw in (dict(match_ths=(0.5,), pixel_grid=[5.0]), dict(match_ths=(-1.0, 0.9), pixel_grid=[13.0, 4.999999, 0.0]),
               dict(match_ths=THS, pixel_grid=np.arange(16) * 2.5)):
        g2, w2, _ = _tally(tally_case, dev, **kw)
        _assert_tally(g2, w2, kw)
    # without dist, and a second run: the same bits
    up = lambda v: torch.from_numpy(v).to(dev)
    c = tally_case
    split = lambda v: [v[c["koff"][i]:c["koff"][i + 1]] for i in range(5)]
    for _ in range(2):
        counts, nb = ops.pck_tally(up(c["xa"]), up(c["ya"]), up(c["m"]), up(c["flag"]), split(c["xs"]), split(c["ys"]), c["koff"], match_ths=THS)
        assert np.array_equal(counts.cpu().numpy(), got[0]) and np.array_equal(nb.cpu().numpy(), got[1])


def test_tally_valid_flags_and_positions(dev, tally_case):
    valid = [True, False, True, False, True]
    got, want, _ = _tally(tally_case, dev, match_ths=THS, valid=valid)
    _assert_tally(got, want, "valid")
    assert got[1][:, 1].tolist() == [1, 1, 1] and got[1][:, 3].tolist() == [257] * 3 and not got[0][:, [1, 3]].any()
    full, _, ko = _tally(tally_case, dev, match_ths=THS)
    for order in ([4, 3, 2, 1, 0], [3, 0, 4], [2], [0, 0, 1, 0]):
        g2, w2, ko2 = _tally(tally_case, dev, order=order, match_ths=THS)
        _assert_tally(g2, w2, order)
        for pos, b in enumerate(order):                             # every pair: the bits it has in the full batch
            assert np.array_equal(g2[0][:, pos], full[0][:, b]) and np.array_equal(g2[1][:, pos], full[1][:, b])
            assert np.array_equal(g2[2][:, ko2[pos]:ko2[pos + 1]].view(np.int64), full[2][:, ko[b]:ko[b + 1]].view(np.int64))


# ---------------------------------------------------------------- 3. end to end

def _golden_records(dev):
    G = golden()
    g = G["raw"]
    R = ops.MultiHRecordsRagged([s[0] for s in G["sizes8"]], [s[1] for s in G["sizes8"]], dev, max_h=int(g["max_h"]))
    for b, n in enumerate(G["nbH"]):
        pair = tuple(torch.from_numpy(g["p%d_%s" % (b, k)].astype(np.float32)) for k in ("flow", "param", "match")) if n else None
        nbH, _, Hs, f8, m8 = R.views(b)
        _fill((nbH, Hs, f8, m8), pair, dev)
    R.size_src = G["sizeA"]
    return R


def test_chain_equals_the_reference_tallies_of_the_golden(dev):
    G = golden()
    g = G["raw"]
    R = _golden_records(dev)
    XA, YA, XB, YB = ([k[i] for k in G["kp"]] for i in range(4))
    counts, nb, valid = assemble.corr_keypoints_records(R, float(g["th"]), bool(g["multiH"]), XA, YA, XB, YB, matchability_ths=G["ths"])
    assert counts.is_cuda and nb.is_cuda and valid.tolist() == [True, True, False]
    print("golden counts", counts.cpu().numpy().tolist(), "nbAlign", nb.cpu().numpy().tolist())
    assert np.array_equal(nb.cpu().numpy(), g["nbAlign"]), (nb.cpu().numpy().tolist(), g["nbAlign"].tolist())
    assert np.array_equal(counts.cpu().numpy(), g["counts"]), (counts.cpu().numpy().tolist(), g["counts"].tolist())
    prec, tot = assemble.corr_precision(counts, nb)
    assert np.array_equal(prec, g["counts"].sum(axis=1) / g["nbAlign"].sum(axis=1)[:, None]) and tot.tolist() == g["nbAlign"].sum(axis=1).tolist()
    # the pixel grid handed over as the script holds it, (1, T)
    c2, n2, _ = assemble.corr_keypoints_records(R, float(g["th"]), bool(g["multiH"]), XA, YA, XB, YB, matchability_ths=G["ths"],
                                                pixelGrid=g["grid"].reshape(1, -1), sizesA=G["sizeA"])
    assert torch.equal(c2, counts) and torch.equal(n2, nb)


def test_chain_does_not_sync_with_the_host(dev):
    G = golden()
    R = _golden_records(dev)
    XA, YA, XB, YB = ([k[i] for k in G["kp"]] for i in range(4))
    run = lambda: assemble.corr_keypoints_records(R, 0.3, True, XA, YA, XB, YB, matchability_ths=G["ths"])
    want = run()                                                   # the library is loaded, the allocators are warm
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                           # the mode does see a sync on this build
            R.rec[0, 0].item()
        got = run()
        kp = ops.records_keypoints(R, 0.3, True, True, XB, YB)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(t.is_cuda for t in kp[:4])


DRIVER_MIN = 240      # the pairs' shorter side: the smallest size the variant-C driver's own kernels are held to elsewhere in this
                      # suite (the keypoint cases above stay at 48 x 64 maps; here the keypoints are 80 per pair, whatever the maps)


def test_driver_records_to_tallies(dev):
    """Records that multi_h_variant_c(..., want_records=True) filled for two small pairs with ONE candidate each (the evalCorr-like
    use) -> the chain, against today's path: assemble_records, then corr_alignment_error per pair under the script's mask."""
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    pipe = AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=DRIVER_MIN, scaleR=1.2, variant="C", device=dev, seed=5,
                         degenerate="device")
    pairs = [synth.make_pair(DRIVER_MIN, DRIVER_MIN * 4 // 3, seed=s, homography=True) for s in (80, 82)]
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)
    outs, R = pipe.multi_h_variant_c([up(p[0]) for p in pairs], [[up(p[1]) for p in pairs]], maxCoarse=2, pair_ids=[1, 2],
                                     want_records=True)
    assert R.max_h == 3 and R.size_src is not None
    nbH = [o["nbH"] for o in outs]
    print("driver nbH", nbH, "size_src", R.size_src, "h8 w8", R.h8, R.w8)
    assert max(nbH) >= 1, "no pair has a homography: the comparison below would be empty"
    rng = np.random.RandomState(12)
    grid = ops.pck_pixel_grid().reshape(1, -1)
    th = 0.5
    fg, mg, _, valid = ops.assemble_records(R, th, True, True)
    XA, YA, XB, YB = [], [], [], []
    for b in range(2):
        hB, wB = mg[b].shape
        wA, hA = R.size_src[b]
        xb, yb = (rng.rand(80) * wB).astype(np.float32), (rng.rand(80) * hB).astype(np.float32)
        est = ops.sample_points(fg[b], mg[b], xb, yb, (wA, hA))
        XB.append(xb), YB.append(yb)
        XA.append((est[0].cpu().numpy() + rng.randn(80) * 4).astype(np.float32))
        YA.append((est[1].cpu().numpy() + rng.randn(80) * 4).astype(np.float32))
    counts, nb, v = assemble.corr_keypoints_records(R, th, True, XA, YA, XB, YB, matchability_ths=THS)
    assert v.tolist() == valid.tolist() == [n >= 1 for n in nbH]
    counts, nb = counts.cpu().numpy(), nb.cpu().numpy()
    for b in range(2):
        if nbH[b] < 1:
            assert nb[:, b].tolist() == [80] * 3 and not counts[:, b].any()
            continue
        hB, wB = mg[b].shape
        f = fg[b]
        inside = ((f >= -1) & (f <= 1)).all(dim=2).float()
        for t, mt in enumerate(THS):
            mask = (mg[b] >= mt).float() * inside if mt > 0 else torch.ones_like(mg[b])
            c, n = assemble.corr_alignment_error(wB, hB, R.size_src[b][0], R.size_src[b][1], XA[b], YA[b], XB[b], YB[b], f, mask, grid)
            assert n == nb[t, b] and np.array_equal(np.asarray(c, np.int64), counts[t, b]), (b, mt, n, nb[t, b])
        assert 0 < counts[0, b, 3] <= 80
