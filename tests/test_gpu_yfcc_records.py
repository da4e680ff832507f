"""The YFCC path of a batch of pairs of different sizes on the device: driver -> records -> flows -> correspondences.
csrc/points_ragged.hip (rfx_flow_points_ragged_f32; ops.flow_points_ragged / matches_from_flow_ragged) against the per-map op and
the numpy rule of tests/test_yfcc_records_cpu.py (a loop of the rule tests/test_points_cpu.py pins to the reference's outputs);
assemble.yfcc_matches_records against the per-pair chain assemble_yfcc + yfcc_matches; the records multi_h_variant_c(...,
want_records=True) builds against the lists it returns and against every pair run alone.  Integer positions and float32 steps
rounded one by one: everything is compared with torch.equal, pts1 as int32 bit patterns; no tolerance anywhere."""
import warnings

import numpy as np
import pytest
import torch

from rfx import assemble, ops, synth, weights
from rfx.pipeline import AlignPipeline, ragged_candidate_plan, resize_dims
from test_gpu_assemble_records import _fill, _random_pair
from test_points_cpu import golden, sha
from test_yfcc_records_cpu import golden_batch, rule_points_ragged

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _same_points(got1, got2, want1, want2, what):
    """Device rows against numpy rows: shape, pts2 value for value, pts1 bit for bit."""
    assert tuple(got1.shape) == tuple(got2.shape) == (len(want1), 2), (what, tuple(got1.shape), len(want1))
    assert got1.dtype == torch.float32 and got2.dtype == torch.int64
    assert torch.equal(got2.cpu(), torch.from_numpy(want2)), what
    assert torch.equal(_bits(got1), torch.from_numpy(want1.view(np.int32))), what


# ---------------------------------------------------------------- 1. ragged points = the per-map op = the numpy rule

SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41), (17, 241)]      # 1, 63, 64, 65, 1023, 1024, 1025, 4097 px
ANGLES8 = [0, 90, 180, 270, 0, 90, 180, 270]
SIZES_A = [(640 + 3 * b, 480 - 5 * b) for b in range(8)]
SPECIAL = [1.0, -1.0, -0.0, 0.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)),
           np.nextafter(np.float32(-1), np.float32(-2)), np.nextafter(np.float32(-1), np.float32(0)), 2.0 ** -24, -2.0 ** -24,
           2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25]
FAMILIES = ("all", "none", "first", "last", "beside multiples of 64", "seeded")


def _family(name, n, rng):
    p = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": p == 0, "last": p == n - 1,
            "beside multiples of 64": (p % 64 == 0) | (p % 64 == 63), "seeded": rng.rand(n) < 0.4}[name]


def _flows(rng):
    """Seeded float32 flows formed in float64 (their sums with 1 are inexact); +-1, -0.0, the neighbours of +-1 and the half-ulp ties of
    the first step wherever a map has room, in both channels and at both ends."""
    out = []
    for H, W in SHAPES:
        f = (rng.rand(H * W, 2) * 2 - 1).astype(np.float32)
        n = min(len(SPECIAL), H * W)
        f[:n, 0] = f[H * W - n:, 1] = np.asarray(SPECIAL[:n], np.float32)
        out.append(f.reshape(H, W, 2))
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_points_equal_the_per_map_op_and_the_rule(dev, family):
    rng = np.random.RandomState(17 + FAMILIES.index(family))
    flows = _flows(rng)
    keeps = [_family(family, H * W, rng).reshape(H, W) for H, W in SHAPES]
    bgs = [(rng.rand(H, W) < 0.7) | (np.arange(H * W).reshape(H, W) == H * W - 1) for H, W in SHAPES]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pack = lambda maps, tail=(): up(np.concatenate([m.reshape((-1,) + tail) for m in maps]))
    orders = [list(range(8))] + ([list(range(7, -1, -1))] if family in ("seeded", "last") else [])
    for order in orders:
        fl, kp, bg = ([x[b] for b in order] for x in (flows, keeps, bgs))
        sizes, sizesA, angles = ([x[b] for b in order] for x in (SHAPES, SIZES_A, ANGLES8))
        for use_bg in (False, True):
            w1, w2, woff = rule_points_ragged(fl, kp, sizesA, angles, bg if use_bg else None)
            forms = [(pack(fl, (2,)), pack(kp), pack(bg))]                                      # packed, bool
            if family in ("seeded", "beside multiples of 64"):
                forms.append((pack(fl, (2,)), pack(kp).to(torch.uint8) * 7, pack(bg).to(torch.uint8) * 255))   # bytes: non-zero counts
                forms.append(([up(f) for f in fl], [up(k) for k in kp], [up(g) for g in bg]))  # separate maps: concatenated
            for f_d, k_d, b_d in forms:
                p1, p2, off = ops.flow_points_ragged(f_d, k_d, sizes, sizesA, angles, bg=b_d if use_bg else None)
                assert off.is_cuda and off.dtype == torch.int64 and tuple(p1.shape) == tuple(p2.shape) == (sum(h * w for h, w in sizes), 2)
                assert torch.equal(off.cpu(), torch.from_numpy(woff)), (family, order[0], use_bg)
                _same_points(p1[:woff[-1]], p2[:woff[-1]], w1, w2, (family, order[0], use_bg))
            g1, g2, goff = ops.matches_from_flow_ragged(*forms[0][:2], sizes, sizesA, angles, bg=forms[0][2] if use_bg else None)
            assert not goff.is_cuda and torch.equal(goff, torch.from_numpy(woff))
            _same_points(g1, g2, w1, w2, (family, "exact", use_bg))
            # per map: the rows of the batch are the per-map op on that map alone
            for b, (H, W) in enumerate(sizes):
                k = angles[b] // 90
                one = ops.matches_from_flow(up(fl[b]), up(kp[b]), sizesA[b], (W, H) if k % 2 == 0 else (H, W), angles[b],
                                            bg=up(bg[b]) if use_bg else None)
                rows = slice(int(goff[b]), int(goff[b + 1]))
                assert torch.equal(g2[rows], one[1]) and torch.equal(_bits(g1[rows]), _bits(one[0])), (family, b, use_bg)
    if family == "all":
        assert woff.tolist()[-1] == sum((g & np.ones_like(g)).sum() for g in bgs) and np.diff(woff).min() >= 1
    if family == "none":
        assert woff.tolist() == [0] * 9


def test_consecutive_views_of_one_buffer_are_not_copied(dev):
    """Lists of per-pair maps that already lie one behind the other (what assemble_records returns) go to the kernel as they are."""
    rng = np.random.RandomState(5)
    sizes = SHAPES[2:6]
    total = sum(h * w for h, w in sizes)
    f, m = torch.from_numpy((rng.rand(total, 2) * 2 - 1).astype(np.float32)).to(dev), torch.from_numpy(rng.rand(total) < 0.5).to(dev)
    cut = lambda t, tail: [t[o:o + h * w].view((h, w) + tail) for o, (h, w) in zip(np.cumsum([0] + [h * w for h, w in sizes[:-1]]), sizes)]
    assert ops._packed_maps(cut(f, (2,)), "flow").data_ptr() == f.data_ptr() and ops._packed_maps(cut(m, ()), "keep").data_ptr() == m.data_ptr()
    assert ops._packed_maps(cut(f, (2,))[::-1][:1] + cut(f, (2,))[1:], "flow").data_ptr() != f.data_ptr()
    a = ops.matches_from_flow_ragged(cut(f, (2,)), cut(m, ()), sizes, SIZES_A[:4], ANGLES8[:4])
    b = ops.matches_from_flow_ragged(f, m, sizes, SIZES_A[:4], ANGLES8[:4])
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[0]), _bits(b[0])) and len(a[0]) > 0


# ---------------------------------------------------------------- 2. more tiles than the grid cap, more than one scan trip

def test_more_maps_than_the_grid_cap_and_nine_scan_trips(dev):
    """9000 maps alternating 2 x 3 (k = 0) and 3 x 2 (k = 1): one tile each, more tiles than the launches' 8192 workgroups -- they
    stride --, nine trips of the scan, a binary search over 9000 rows; some maps empty."""
    rng = np.random.RandomState(9)
    B = 9000
    keep = rng.rand(B, 6) < 0.5
    keep[rng.rand(B) < 0.1] = False
    keep[[0, 1, B - 1]] = [[False] * 6, [True] * 6, [False] * 5 + [True]]
    flow = (rng.rand(B, 6, 2) * 2 - 1).astype(np.float32)
    sizes = [(2, 3), (3, 2)] * (B // 2)
    angles = [0, 90] * (B // 2)
    sizesA = [(100 + b % 37, 90 + b % 41) for b in range(B)]
    p1, p2, off = ops.matches_from_flow_ragged(torch.from_numpy(flow.reshape(-1, 2)).to(dev), torch.from_numpy(keep.reshape(-1)).to(dev),
                                               sizes, sizesA, angles)
    w1, w2, woff = rule_points_ragged([flow[b].reshape(sizes[b] + (2,)) for b in range(B)], [keep[b].reshape(sizes[b]) for b in range(B)],
                                      sizesA, angles)
    assert (np.diff(woff) == 0).sum() > 100 and woff[-1] > 8192
    assert torch.equal(off, torch.from_numpy(woff))
    _same_points(p1, p2, w1, w2, "9000 maps")


# ---------------------------------------------------------------- 3. the goldens as one ragged batch

def test_goldens_as_one_ragged_batch(dev):
    g = golden()["raw"]
    flows, keeps, sizesA, angles, tags = golden_batch()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pts1, pts2, off = ops.matches_from_flow_ragged([up(f) for f in flows], [up(k) for k in keeps], [k.shape for k in keeps], sizesA, angles)
    for b, (c, a) in enumerate(tags):
        rows = slice(int(off[b]), int(off[b + 1]))
        p1, p2 = pts1[rows].cpu().numpy(), pts2[rows].cpu().numpy()
        assert len(p1) == int(g["case%d_a%d_n" % (c, a)]) and p1.dtype == np.float32 and p2.dtype == np.int64
        assert sha(p1) == str(g["case%d_a%d_sha1" % (c, a)]) and sha(p2) == str(g["case%d_a%d_sha2" % (c, a)]), (c, a)
        if (c, a) == (int(g["full_case"]), int(g["full_angle"])):
            assert torch.equal(_bits(pts1[rows]), torch.from_numpy(g["full_pts1"].view(np.int32)))
            assert torch.equal(pts2[rows].cpu(), torch.from_numpy(g["full_pts2"].astype(np.int64)))


# ---------------------------------------------------------------- 4. hand-filled records -> correspondences, one host sync

HAND = ((30, 40, 3), (40, 30, 0), (32, 38, 11), (3, 5, 1))                       # (h8, w8, nbH)
HAND_ANGLES = [0, 90, 180, 270]
HAND_SRC = [(320, 240), (240, 336), (352, 272), (64, 48)]
HAND_TH = 0.25


def _hand_records(dev):
    g = torch.Generator().manual_seed(40)
    pairs = [_random_pair(g, n, h8, w8) if n else None for h8, w8, n in HAND]
    R = ops.MultiHRecordsRagged([h for h, _, _ in HAND], [w for _, w, _ in HAND], dev, max_h=11)
    for b, pair in enumerate(pairs):
        nbH, _, Hs, f8, m8 = R.views(b)
        _fill((nbH, Hs, f8, m8), pair, dev)
    bgs = [torch.rand(8 * h, 8 * w, generator=g) < (0.6 if b in (0, 2) else 2.0) for b, (h, w, _) in enumerate(HAND)]
    R.candidate, R.candidate_dev = [a // 90 for a in HAND_ANGLES], torch.tensor([a // 90 for a in HAND_ANGLES], dtype=torch.int32, device=dev)
    R.size_src, R.size_tgt, R.angle = list(HAND_SRC), [(8 * w, 8 * h) for h, w, _ in HAND], list(HAND_ANGLES)
    R.bg = torch.cat([m.reshape(-1) for m in bgs]).to(torch.uint8).to(dev)
    return R, pairs, bgs


def _chain(pair, bg, th, sizeA, angle, dev):
    """The per-pair yardstick: assemble_yfcc on the pair's own arrays, then yfcc_matches."""
    fg, binary = assemble.assemble_yfcc(pair[0].to(dev), pair[1].to(dev), pair[2].to(dev), bg.to(dev), th, True, device=dev)
    H, W = binary.shape[1:]
    p1, p2 = assemble.yfcc_matches(fg, binary, sizeA, (W, H) if (angle // 90) % 2 == 0 else (H, W), angle)
    return p1, p2, fg, binary


def test_hand_filled_records_to_correspondences(dev):
    R, pairs, bgs = _hand_records(dev)
    pts1, pts2, off, valid, flows, binaries = assemble.yfcc_matches_records(R, HAND_TH, True, return_maps=True)
    assert not off.is_cuda and valid.is_cuda and valid.tolist() == [True, False, True, True]
    assert int(off[2]) == int(off[1]) and sum(int(off[b + 1] - off[b]) > 0 for b in range(4)) >= 2          # nbH = 0: no rows
    assert not bool(binaries[1].any()) and not bool(flows[1].any())
    for b, pair in enumerate(pairs):
        if pair is None:
            continue
        p1, p2, fg, binary = _chain(pair, bgs[b], HAND_TH, HAND_SRC[b], HAND_ANGLES[b], dev)
        rows = slice(int(off[b]), int(off[b + 1]))
        assert torch.equal(binaries[b], binary[0]) and torch.equal(_bits(flows[b]), _bits(fg[0])), b
        assert torch.equal(pts2[rows], p2) and torch.equal(_bits(pts1[rows]), _bits(p1)), b
    assert int(binaries[0].sum()) < int(assemble.yfcc_matches_records(R, HAND_TH, True, bg=None, return_maps=True)[5][0].sum())
    # explicit arguments in place of the attributes; a slice of the batch
    again = assemble.yfcc_matches_records(R, HAND_TH, True, sizesA=HAND_SRC, sizesB=[(320, 240), (320, 240), (304, 256), (24, 40)],
                                          angles=HAND_ANGLES, bg=[m.to(dev) for m in bgs])
    assert torch.equal(again[2], off) and torch.equal(again[1], pts2) and torch.equal(_bits(again[0]), _bits(pts1))
    part = assemble.yfcc_matches_records(R.rows(2, 4), HAND_TH, True)
    assert torch.equal(part[2], off[2:] - off[2]) and torch.equal(part[1], pts2[int(off[2]):]) and part[3].tolist() == [True, True]


def test_the_batch_form_reads_the_host_once(dev):
    R, _, _ = _hand_records(dev)
    assemble.yfcc_matches_records(R, HAND_TH, True)                  # the library is loaded, the allocators are warm
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            R.rec[0, :5].cpu()
            one = len(seen)
            assert one >= 1                                         # the mode does see a read on this build: ``one`` warnings each
            out = assemble.yfcc_matches_records(R, HAND_TH, True)
            assert len(seen) == 2 * one, [str(w.message) for w in seen]   # exactly one more read: the offsets
            ops.flow_points_ragged(torch.zeros(6, 2, device=dev), torch.ones(6, dtype=torch.bool, device=dev), [(2, 3)], [(5, 5)], 0)
            assert len(seen) == 2 * one                             # the device form: none
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert out[3].is_cuda and len(out[0]) == int(out[2][-1]) > 0


# ---------------------------------------------------------------- 5. the driver

ANGLES = (0, 90, 180, 270)
# (seed, H, W, rows / columns cropped off the target, turn the target is STORED with): the first four pairs, the pipeline settings and
# the accept thresholds of tests/test_gpu_ragged_variant_c.py (measured there: at 0.03 and 0.06 the pairs stop at different rounds)
PAIRS = [(80, 240, 320, 0, 0, 0), (81, 240, 320, 0, 0, 270), (82, 256, 320, 0, 16, 0), (7, 240, 336, 0, 0, 180)]
IDS = [100, 107, 114, 121]
MAX_COARSE = 3


def _up(im, dev):
    return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)


def _lists(pairs, dev):
    src, tgt = [_up(p[0], dev) for p in pairs], [_up(p[1], dev) for p in pairs]
    return src, [[torch.rot90(t, a // 90, (0, 1)).contiguous() for t in tgt] for a in ANGLES]


@pytest.fixture(scope="module")
def driver(dev):
    """The pipeline, the pairs, and every pair run ALONE through the dense driver at both thresholds (computed once)."""
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    pipe = AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=240, scaleR=1.2, variant="C", device=dev, seed=5,
                         degenerate="device")
    pairs = []
    for seed, H, W, dh, dw, turn in PAIRS:
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
        I2 = I2.crop((0, 0, W - dw, H - dh))
        pairs.append((I1, I2.rotate(turn, expand=True) if turn else I2))
    alone = {}
    for th in (0.03, 0.06):
        alone[th] = []
        for p, pid in zip(pairs, IDS):
            src, cands = _lists([p], dev)
            alone[th].append(pipe.multi_h_variant_c(src[0][None], [c[0][None] for c in cands], maxCoarse=MAX_COARSE, maskRegionTh=th,
                                                    pair_ids=[pid])[0])
    return dict(pipe=pipe, pairs=pairs, alone=alone)


def _assert_outs_equal(o, a, tag):
    assert o["candidate"] == a["candidate"] and o["nbInlier"] == a["nbInlier"] and o["nbH"] == a["nbH"], tag
    assert torch.equal(o["mask"], a["mask"]), tag
    for key in ("H", "flowDown8", "matchDown8"):
        assert len(o[key]) == len(a[key]) and all(torch.equal(x, y) for x, y in zip(o[key], a[key])), (tag, key)


def _assert_record(R, b, lists, alone, tag):
    """Pair b's record: nbH, status 0, the first nbH entries equal to the returned lists (if any) and to the pair alone, zeros beyond."""
    nbH, status, Hs, f8, m8 = R.views(b)
    n = alone["nbH"]
    assert float(nbH) == n and float(status) == (0.0 if n else 1.0), (tag, float(nbH), float(status), n)
    for o in ([alone] if lists is None else [lists, alone]) if n else ():
        assert torch.equal(Hs[:n], torch.stack(o["H"])), tag
        assert torch.equal(f8[:n], torch.cat(o["flowDown8"])) and torch.equal(m8[:n], torch.cat(o["matchDown8"])), tag
    assert not bool(Hs[n:].any()) and not bool(f8[n:].any()) and not bool(m8[n:].any()), tag
    assert R.candidate[b] == alone["candidate"] and int(R.candidate_dev[b]) == alone["candidate"], tag
    h, w = alone["mask"].shape
    assert R.size_tgt[b] == (w, h) == (8 * R.w8[b], 8 * R.h8[b]), tag


@pytest.mark.parametrize("th", [0.03, 0.06])
def test_driver_records_equal_the_lists_and_each_pair_alone(dev, driver, th):
    pipe, pairs, alone = driver["pipe"], driver["pairs"], driver["alone"][th]
    nbh, cand, shapes = [o["nbH"] for o in alone], [o["candidate"] for o in alone], [tuple(o["mask"].shape) for o in alone]
    print("alone at %s: nbH %s candidates %s target shapes %s" % (th, nbh, cand, shapes))
    if th == 0.03:                                                  # preconditions on the ALONE results: a trivial batch cannot pass
        assert len(set(cand)) >= 2 and len(set(shapes)) >= 3 and len(set(nbh)) >= 2, (cand, shapes, nbh)
    assert min(nbh) >= 1, nbh
    src, cands = _lists(pairs, dev)
    run = lambda **kw: pipe.multi_h_variant_c(src, cands, maxCoarse=MAX_COARSE, maskRegionTh=th, pair_ids=IDS, **kw)
    plain = run()
    first = None
    for split in (1, 2):
        outs, R = run(want_records=True, split=split)
        assert isinstance(R, ops.MultiHRecordsRagged) and R.max_h == MAX_COARSE + 1 and R.B == 4 and R.bg is None and R.angle is None
        assert R.size_src == [resize_dims(p[0].size[0], p[0].size[1], 240, "min") for p in pairs]
        for b in range(4):
            _assert_outs_equal(outs[b], plain[b], (th, split, b, "outs"))
            _assert_outs_equal(outs[b], alone[b], (th, split, b, "alone"))
            _assert_record(R, b, outs[b], alone[b], (th, split, b))
        first = R.rec.clone() if first is None else first
        assert torch.equal(_bits(R.rec), _bits(first)), split
    outs, R = run(want_records=True, want_lists=False)
    assert torch.equal(_bits(R.rec), _bits(first)) and all(o["H"] == [] and o["nbH"] == a["nbH"] for o, a in zip(outs, alone))
    for b in range(4):
        _assert_record(R, b, None, alone[b], (th, "no lists", b))


def test_driver_pairs_form_same_size_lists_and_backgrounds(dev, driver, monkeypatch):
    pipe, pairs, alone = driver["pipe"], driver["pairs"], driver["alone"][0.03]
    # the PIL entry: the angle of the chosen candidate rides on the records
    outs, R = pipe.multi_h_variant_c_pairs(pairs, angles=ANGLES, maxCoarse=MAX_COARSE, maskRegionTh=0.03, pair_ids=IDS, want_records=True)
    assert R.angle == [ANGLES[a["candidate"]] for a in alone] and len(set(R.angle)) >= 2
    for b in range(4):
        _assert_outs_equal(outs[b], alone[b], ("pairs", b))
        _assert_record(R, b, outs[b], alone[b], ("pairs", b))
    assert R.rows(1, 3).angle == R.angle[1:3] and R.rows(1, 3).size_tgt == R.size_tgt[1:3] and R.rows(1, 3).candidate_dev.tolist() == R.candidate[1:3]
    # a same-size list takes the ragged path and gives each pair's alone result
    calls = []
    real = ops.multih_accept_ragged
    same = [synth.make_pair(240, 320, seed=s, homography=True) for s in (80, 82)]
    src, cands = _lists(same, dev)
    monkeypatch.setattr(ops, "multih_accept_ragged", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    outs, R = pipe.multi_h_variant_c(src, cands, maxCoarse=2, pair_ids=[1, 2], want_records=True)
    n = len(calls)
    assert n >= 1
    dense = pipe.multi_h_variant_c(src, cands, maxCoarse=2, pair_ids=[1, 2])
    assert len(calls) == n                                           # without want_records: today's dense call
    for b in range(2):
        a = pipe.multi_h_variant_c(src[b][None], [c[b][None] for c in cands], maxCoarse=2, pair_ids=[1 + b])[0]
        _assert_outs_equal(outs[b], a, ("same size", b))
        _assert_outs_equal(dense[b], a, ("same size, dense", b))
        _assert_record(R, b, outs[b], a, ("same size", b))
    assert R.max_h == 3
    # background strips: records.bg is the chosen candidates' maps, packed like the assembled maps
    pairs3 = pairs[:3]
    src, cands = _lists(pairs3, dev)
    wh = lambda x: (x.shape[1], x.shape[0])
    sizes = ragged_candidate_plan([wh(x) for x in src], [[wh(x) for x in c] for c in cands], 240, pipe.scaleList, "min")["levels"]
    nS = len(pipe.scaleList)

    def strip(b, k):
        m = torch.ones(sizes[b][nS + k])
        if k % 2 == 0:
            m[:40 + 8 * b] = 0
        else:
            m[:, -(48 + 8 * b):] = 0
        return m
    It_bg = [[strip(b, k) for b in range(3)] for k in range(4)]
    It_bg[3][1] = None
    It_bg[2] = None
    outs, R = pipe.multi_h_variant_c(src, cands, maxCoarse=MAX_COARSE, maskRegionTh=0.03, pair_ids=IDS[:3], It_bg=It_bg, want_records=True)
    plain = pipe.multi_h_variant_c(src, cands, maxCoarse=MAX_COARSE, maskRegionTh=0.03, pair_ids=IDS[:3], It_bg=It_bg)
    want = []
    for b, o in enumerate(outs):
        _assert_outs_equal(o, plain[b], ("bg", b))
        k = o["candidate"]
        m = torch.ones(sizes[b][nS + k]) if It_bg[k] is None or It_bg[k][b] is None else It_bg[k][b]
        assert tuple(m.shape) == tuple(o["mask"].shape)
        want.append(m.reshape(-1))
    assert R.bg.dtype == torch.uint8 and torch.equal(R.bg.cpu(), torch.cat(want).to(torch.uint8)) and 0 < int(R.bg.sum()) < R.bg.numel()
    assert R.rows(1, 3).bg.numel() == want[1].numel() + want[2].numel() and torch.equal(R.rows(1, 2).bg.cpu(), want[1].to(torch.uint8))
    # the driver's records through the batch form = the per-pair chain on the lists
    _assert_matches(R, outs, [m.reshape(o["mask"].shape) for m, o in zip(want, outs)], dev, [ANGLES[o["candidate"]] for o in outs])


def _assert_matches(R, outs, bgs, dev, angles_arg=None):
    """yfcc_matches_records on the driver's records against assemble_yfcc + yfcc_matches on the driver's lists, at the script's 0.95
    and at lower thresholds; at one of them at least two pairs must have points."""
    angles = R.angle if angles_arg is None else angles_arg
    most = 0
    for th in (0.95, 0.5, 0.1):
        pts1, pts2, off, valid = assemble.yfcc_matches_records(R, th, True, angles=angles)
        assert valid.tolist() == [o["nbH"] >= 1 for o in outs]
        for b, o in enumerate(outs):
            if not o["nbH"]:
                assert int(off[b + 1]) == int(off[b])
                continue
            pair = (torch.cat(o["flowDown8"]), torch.stack(o["H"]), torch.cat(o["matchDown8"]))
            p1, p2, _, _ = _chain(pair, bgs[b], th, R.size_src[b], angles[b], dev)
            rows = slice(int(off[b]), int(off[b + 1]))
            assert torch.equal(pts2[rows], p2) and torch.equal(_bits(pts1[rows]), _bits(p1)), (th, b)
        most = max(most, sum(int(off[b + 1] - off[b]) > 0 for b in range(len(outs))))
        print("th %s: points per pair %s" % (th, np.diff(off.numpy()).tolist()))
    assert most >= 2


def test_driver_records_to_correspondences(dev, driver):
    pipe, pairs = driver["pipe"], driver["pairs"]
    outs, R = pipe.multi_h_variant_c_pairs(pairs, angles=ANGLES, maxCoarse=MAX_COARSE, maskRegionTh=0.03, pair_ids=IDS, want_records=True)
    _assert_matches(R, outs, [torch.ones(o["mask"].shape, dtype=torch.bool) for o in outs], dev)
