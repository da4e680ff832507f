"""The YFCC (variant C) multi-homography driver on pairs of different sizes in one call: every pair's results equal, bit for bit
(torch.equal, no tolerance), what the pair gives ALONE through the dense driver -- multi_h_variant_c on stacked tensors at batch 1 with
pair_ids=[id] -- which tests/test_gpu_dropin.py pins to the reference's script.

Kernel level: rfx_keep_mask_ragged_f32 against rfx_keep_mask_f32 called per pair, and the round's matching (keep map -> masked ragged
mutual matching of the active pairs only) against ops.mutual_nn per pair.  Driver level: device draws (split 1 and 2, both degenerate
modes, a shuffled order), explicit draws, background maps, and multi_h_variant_c_pairs.

The driver pairs (PAIRS below; 240x320-class sizes, heights and widths varied by multiples of 8, one target cropped, one stored turned
by 270 and one by 180 degrees; seeds chosen on the MI355X): alone, on the dense driver, they end with nbH = NBH_ALONE[threshold] and
choose the candidates CANDIDATE_ALONE in both degenerate modes (checked by the test), so the chosen target shapes differ, every pair
accepts a homography and the active list of the lock-step rounds shrinks unevenly (see TH for the accept threshold)."""
import numpy as np
import pytest
import torch

from rfx import ops, weights, synth
from rfx.pipeline import AlignPipeline, ragged_candidate_plan

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = -7.0


# ------------------------------------------------------------------------------------------------ kernels
def _packed(ts):
    off = np.cumsum([0] + [t.numel() for t in ts[:-1]]).tolist()
    return torch.cat([t.reshape(-1) for t in ts]).contiguous(), off


def _blob(h, w, g):
    blob = torch.nn.functional.avg_pool2d(torch.rand(1, 1, h + 16, w + 16, generator=g), 17, 1)[0, 0]
    return (blob > blob.median()).float().to(DEV).contiguous()


t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
t32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)

# (h, w, rt, ct): cell counts below (12, 80), across (300, 330) and far above (8250) one 256-thread workgroup, odd ratios
KEEP_SHAPES = [(240, 320, 15, 20), (96, 312, 10, 33), (376, 1242, 50, 165), (64, 48, 4, 3), (128, 168, 8, 10)]


def test_keep_mask_ragged_equals_keep_mask_per_pair():
    g = torch.Generator().manual_seed(11)
    B = len(KEEP_SHAPES)
    cells = [rt * ct for _, _, rt, ct in KEEP_SHAPES]
    ldB = (max(cells) + 3) // 4 * 4
    masks = [_blob(h, w, g) for h, w, _, _ in KEEP_SHAPES]
    bgs = [(torch.rand(h, w, generator=g) > 0.2).float().to(DEV) for h, w, _, _ in KEEP_SHAPES]
    Mask, moff = _packed(masks)
    BG, _ = _packed(bgs)
    geom = t32([[h, w, rt, ct, h // 8, w // 8] for h, w, rt, ct in KEEP_SHAPES])
    mixed = 0
    for mask in (None, Mask):
        for bg in (None, BG):
            for active in (None, [3, 0, 4], [2], [4, 1, 3, 2]):             # lists that skip pairs, out of order
                act = None if active is None else t32(active)
                rows = list(range(B)) if active is None else active
                keep = torch.full((B, ldB), SENTINEL, dtype=torch.float32, device=DEV)
                nB_round = torch.zeros(B, dtype=torch.int32, device=DEV)
                out = ops.keep_mask_ragged(mask, bg, t64(moff), geom, act, ldB, max(cells[b] for b in rows), keep=keep, nB_round=nB_round)
                assert out is keep
                assert nB_round.tolist() == [cells[b] if b in rows else 0 for b in range(B)], (active, nB_round.tolist())
                for b in range(B):
                    if b not in rows:
                        assert bool((keep[b] == SENTINEL).all()), (b, active)                  # an inactive pair's row: untouched
                        continue
                    h, w, rt, ct = KEEP_SHAPES[b]
                    ref = ops.keep_mask(None if mask is None else masks[b][None], None if bg is None else bgs[b][None], None, rt, ct,
                                        n=1, hw=(h, w), device=DEV)[0]
                    assert torch.equal(keep[b, :cells[b]], ref), (b, active, mask is None, bg is None)
                    assert bool((keep[b, cells[b]:] == SENTINEL).all()), (b, active)           # columns past the pair's cells: untouched
                    assert bool(((ref == 0) | (ref == 1)).all())
                    mixed += int(0 < float(ref.sum()) < cells[b])
                    if mask is None and bg is None:
                        assert float(ref.sum()) == cells[b]
    assert mixed >= 3 * 4                                                   # the maps really mix kept and dropped cells
    fresh = ops.keep_mask_ragged(Mask, BG, t64(moff), geom, t32([1]), ldB, cells[1])
    assert tuple(fresh.shape) == (B, ldB) and float(fresh[[0, 2, 3, 4]].abs().sum()) == 0 and torch.equal(fresh[1], keep[1].clamp(min=0))
    with pytest.raises(ValueError):
        ops.keep_mask_ragged(Mask, BG, t64(moff), geom, None, ldB, ldB + 1)
    with pytest.raises(ValueError):
        ops.keep_mask_ragged(Mask, BG, t64(moff), geom[:3], None, ldB, 100)
    with pytest.raises(ValueError):
        ops.keep_mask_ragged(Mask, BG[:-1], t64(moff), geom, None, ldB, max(cells))
    with pytest.raises(RuntimeError):
        ops.keep_mask_ragged(Mask.cpu(), None, t64(moff), geom, None, ldB, max(cells))


# (nA, (h, w, rt, ct)) with nB = rt * ct = 165 / 80 / 12
ROUND_PAIRS = [(300, (176, 240, 11, 15)), (260, (128, 160, 8, 10)), (48, (48, 64, 3, 4))]


def test_round_matching_equals_mutual_nn_per_active_pair():
    g = torch.Generator().manual_seed(23)
    B, C = len(ROUND_PAIRS), 64
    nA = [p[0] for p in ROUND_PAIRS]
    nB = [p[1][2] * p[1][3] for p in ROUND_PAIRS]
    assert nB == [165, 80, 12]
    ldA, ldB, cap = max(nA), (max(nB) + 3) // 4 * 4, max(min(a, b) for a, b in zip(nA, nB))
    unit = lambda n: torch.nn.functional.normalize(torch.randn(C, n, generator=g), dim=0).to(DEV)
    fA, fB = [unit(n) for n in nA], [unit(n) for n in nB]
    featA = torch.zeros((B, C, ldA), device=DEV)
    featB = torch.zeros((B, C, ldB), device=DEV)
    for b in range(B):
        featA[b, :, :nA[b]], featB[b, :, :nB[b]] = fA[b], fB[b]
    masks = [_blob(h, w, g) for _, (h, w, _, _) in ROUND_PAIRS]
    Mask, moff = _packed(masks)
    geom = t32([[h, w, rt, ct, h // 8, w // 8] for _, (h, w, rt, ct) in ROUND_PAIRS])
    keep = torch.zeros((B, ldB), device=DEV)
    for active in ([2, 0], None, [1]):
        rows = list(range(B)) if active is None else active
        nB_round = torch.zeros(B, dtype=torch.int32, device=DEV)
        ops.keep_mask_ragged(Mask, None, t64(moff), geom, None if active is None else t32(active), ldB, max(nB[b] for b in rows),
                             keep=keep, nB_round=nB_round)
        idx1, idx2, cnt = ops.mutual_nn_ragged(featA, featB, t32(nA), nB_round, max(nA[b] for b in rows), max(nB[b] for b in rows),
                                               maskB=keep, cap=cap)
        for b in range(B):
            if b not in rows:
                assert int(cnt[b]) == 0, (b, active)                        # skipped on the round's nB table
                continue
            _, (h, w, rt, ct) = ROUND_PAIRS[b]
            keep_b = ops.keep_mask(masks[b][None], None, None, rt, ct)[0]
            assert 0 < float(keep_b.sum()) < nB[b]
            r1, r2 = ops.mutual_nn(fA[b].contiguous(), fB[b].contiguous(), maskB=keep_b)
            n = int(cnt[b])
            assert n == r1.numel() and n > 0, (b, active, n, r1.numel())
            assert torch.equal(idx1[b, :n], r1) and torch.equal(idx2[b, :n], r2), (b, active)


# ------------------------------------------------------------------------------------------------ driver
ANGLES = (0, 90, 180, 270)
# (seed, H, W, rows / columns cropped off the target, turn the target is STORED with): source H x W
PAIRS = [(80, 240, 320, 0, 0, 0), (81, 240, 320, 0, 0, 270), (82, 256, 320, 0, 16, 0), (7, 240, 336, 0, 0, 180), (8, 272, 352, 8, 0, 0),
         (9, 320, 240, 0, 0, 0)]
# The accept threshold.  At the script's 0.01 the cycle-checked matchability of the synthetic networks keeps every gain above the
# threshold: 62 synthetic pairs tried on the MI355X (these seeds and sizes, with and without perspective, unrelated and grey-padded
# targets) ALL ran the maxCoarse + 1 = 4 rounds, so no active list ever shrank.  At 0.03 and 0.06 the pairs below stop at different
# rounds (measured, pair alone on the dense driver, the same in both degenerate modes):
TH = 0.03
NBH_ALONE = {0.03: [2, 3, 3, 3, 2, 2], 0.06: [1, 2, 1, 2, 2, 2]}
CANDIDATE_ALONE = [0, 1, 0, 2, 0, 0]


def _pairs():
    out = []
    for seed, H, W, dh, dw, turn in PAIRS:
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
        I2 = I2.crop((0, 0, W - dw, H - dh))
        out.append((I1, I2.rotate(turn, expand=True) if turn else I2))
    return out


def _pipe(degenerate="lapack", nbIter=300):
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    return AlignPipeline(sds, nbScale=3, nbIter=nbIter, tolerance=0.05, minSize=240, scaleR=1.2, variant="C", device=DEV, seed=5,
                         degenerate=degenerate)


def _up(im):
    return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(DEV)


def _lists(pairs):
    src, tgt = [_up(p[0]) for p in pairs], [_up(p[1]) for p in pairs]
    return src, [[torch.rot90(t, a // 90, (0, 1)).contiguous() for t in tgt] for a in ANGLES]


def _alone(pipe, pair, pid, sample_fn=None, It_bg=None, th=TH):
    src, cands = _lists([pair])
    return pipe.multi_h_variant_c(src[0][None], [c[0][None] for c in cands], maxCoarse=3, maskRegionTh=th, pair_ids=[pid],
                                  sample_fn=sample_fn, It_bg=It_bg)[0]


def _ragged(pipe, pairs, ids, th=TH, **kw):
    src, cands = _lists(pairs)
    return pipe.multi_h_variant_c(src, cands, maxCoarse=3, maskRegionTh=th, pair_ids=ids, **kw)


def _assert_pair_equal(o, alone, tag):
    assert o["candidate"] == alone["candidate"] and o["nbInlier"] == alone["nbInlier"], (tag, o["nbInlier"], alone["nbInlier"])
    assert o["nbH"] == alone["nbH"] == len(o["H"]), (tag, o["nbH"], alone["nbH"])
    assert o["mask"].shape == alone["mask"].shape and torch.equal(o["mask"], alone["mask"]), tag
    for key in ("H", "flowDown8", "matchDown8"):
        assert len(o[key]) == len(alone[key]) == o["nbH"], (tag, key)
        assert all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(o[key], alone[key])), (tag, key)


@pytest.mark.parametrize("degenerate", ["device", "lapack"])
def test_variant_c_lists_device_draw_equals_each_pair_alone(degenerate):
    pairs = _pairs()
    ids = [100 + 7 * b for b in range(len(pairs))]
    pipe = _pipe(degenerate)
    alone = [_alone(pipe, p, pid) for p, pid in zip(pairs, ids)]
    nbh, cand = [o["nbH"] for o in alone], [o["candidate"] for o in alone]
    shapes = [tuple(o["mask"].shape) for o in alone]
    print("alone (%s): nbH %s candidates %s target shapes %s inliers %s" % (degenerate, nbh, cand, shapes, [o["nbInlier"] for o in alone]))
    # preconditions on the ALONE results: a trivial batch cannot pass
    assert len(set(cand)) >= 2 and len(set(shapes)) >= 3, (cand, shapes)
    assert min(nbh) >= 1 and sum(n >= 2 for n in nbh) >= 2 and len(set(nbh)) >= 2, nbh
    assert len({tuple(p[0].size) for p in pairs}) >= 3 and any(p[0].size != p[1].size and p[0].size != p[1].size[::-1] for p in pairs)
    for split in (1, 2):
        outs = _ragged(pipe, pairs, ids, split=split)
        for b in range(len(pairs)):
            _assert_pair_equal(outs[b], alone[b], (degenerate, split, b))
    order = [4, 1, 5, 0, 3, 2]
    outs = _ragged(pipe, [pairs[i] for i in order], [ids[i] for i in order], split=2)
    for k, i in enumerate(order):
        _assert_pair_equal(outs[k], alone[i], (degenerate, "shuffled", i))
    assert nbh == NBH_ALONE[TH] and cand == CANDIDATE_ALONE
    # a second threshold: some pairs stop after their first homography, the active list shrinks in every round
    alone6 = [_alone(pipe, p, pid, th=0.06) for p, pid in zip(pairs, ids)]
    for split in (1, 2):
        outs = _ragged(pipe, pairs, ids, th=0.06, split=split)
        for b in range(len(pairs)):
            _assert_pair_equal(outs[b], alone6[b], (degenerate, 0.06, split, b))
    assert [o["nbH"] for o in alone6] == NBH_ALONE[0.06]


def test_variant_c_lists_explicit_draws_equal_each_pair_alone():
    pairs = _pairs()[:4]
    ids = [31, 5, 77, 12]
    pipe = _pipe("lapack")

    def draws(pid_of):                                                       # keyed by (pair, call): candidates first, then rounds
        calls = {}

        def fn(b, n, it):
            pid = pid_of(b)
            calls[pid] = calls.get(pid, 0) + 1
            return torch.randint(n, (it, 4), generator=torch.Generator().manual_seed(7000 + 100 * pid + calls[pid] - 1))
        return fn
    outs = _ragged(pipe, pairs, ids, sample_fn=draws(lambda b: ids[b]), split=2)                # split is forced to 1 by explicit draws
    assert min(o["nbH"] for o in outs) >= 1 and len({tuple(o["mask"].shape) for o in outs}) >= 2
    for b, (p, pid) in enumerate(zip(pairs, ids)):
        _assert_pair_equal(outs[b], _alone(pipe, p, pid, sample_fn=draws(lambda _b, pid=pid: pid)), ("explicit", b))


def test_variant_c_lists_background_maps():
    pairs = _pairs()[:3]
    ids = [3, 4, 5]
    pipe = _pipe("device")
    src, cands = _lists(pairs)
    wh = lambda x: (x.shape[1], x.shape[0])
    sizes = ragged_candidate_plan([wh(x) for x in src], [[wh(x) for x in c] for c in cands], 240, pipe.scaleList, "min")["levels"]
    nS = len(pipe.scaleList)                                                 # sizes[b][nS + k] = (h, w) of candidate k after the resize

    def strip(b, k):                                                         # a blank border strip: rows for even k, columns for odd
        m = torch.ones(sizes[b][nS + k])
        if k % 2 == 0:
            m[:40 + 8 * b] = 0
        else:
            m[:, -(48 + 8 * b):] = 0
        return m
    It_bg = [[strip(b, k) for b in range(3)] for k in range(4)]
    It_bg[3][1] = None                                                       # all ones
    It_bg[2] = None                                                          # a candidate without maps
    outs = _ragged(pipe, pairs, ids, It_bg=It_bg)
    plain = _ragged(pipe, pairs, ids)
    assert any(o["nbInlier"] != q["nbInlier"] or not torch.equal(o["mask"], q["mask"]) for o, q in zip(outs, plain))   # the maps matter
    assert max(o["nbH"] for o in outs) >= 1
    for b, (p, pid) in enumerate(zip(pairs, ids)):
        bg1 = [None if g is None or g[b] is None else g[b][None] for g in It_bg]
        a = _alone(pipe, p, pid, It_bg=bg1)
        _assert_pair_equal(outs[b], a, ("bg", b))
        k = a["candidate"]
        if It_bg[k] is not None and It_bg[k][b] is not None and a["nbH"]:
            assert float((a["mask"] * (1 - It_bg[k][b].to(DEV))).sum()) == 0   # nothing is explained inside the blank strip
    with pytest.raises(ValueError):
        _ragged(pipe, pairs, ids, It_bg=[[torch.ones(3, 3)] * 3] * 4)
    with pytest.raises(ValueError):
        _ragged(pipe, pairs, ids, records=ops.MultiHRecords(3, 30, 40, DEV))


def test_multi_h_variant_c_pairs(monkeypatch):
    pipe = _pipe("device")
    calls = dict(dense=0, ragged=0)
    for name, kind in (("keep_mask", "dense"), ("multih_accept", "dense"), ("keep_mask_ragged", "ragged"), ("multih_accept_ragged", "ragged")):
        def counted(*a, _f=getattr(ops, name), _k=kind, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    mixed = _pairs()[:3]
    outs = pipe.multi_h_variant_c_pairs(mixed, maxCoarse=2, pair_ids=[1, 2, 3])
    assert calls["ragged"] >= 2 and calls["dense"] == 0
    src, cands = _lists(mixed)
    ref = pipe.multi_h_variant_c(src, cands, maxCoarse=2, pair_ids=[1, 2, 3])
    for x, y in zip(outs, ref):
        _assert_pair_equal(x, y, "pairs")
    assert len({tuple(o["mask"].shape) for o in outs}) >= 2 and max(o["nbH"] for o in outs) >= 1
    # a same-size list: today's dense call, no ragged entry point
    same = [synth.make_pair(240, 320, seed=s, homography=True) for s in (80, 82)]
    n_ragged = calls["ragged"]
    a = pipe.multi_h_variant_c_pairs(same, maxCoarse=2, pair_ids=[1, 2])
    src, cands = _lists(same)
    b = pipe.multi_h_variant_c(src, cands, maxCoarse=2, pair_ids=[1, 2])                       # lists of one size
    c = pipe.multi_h_variant_c(torch.stack(src), [torch.stack(x) for x in cands], maxCoarse=2, pair_ids=[1, 2])
    assert calls["ragged"] == n_ragged and calls["dense"] >= 3
    for x, y, z in zip(a, b, c):
        _assert_pair_equal(x, z, "same-size pairs")
        _assert_pair_equal(y, z, "same-size lists")
    assert a[0]["nbH"] >= 1
