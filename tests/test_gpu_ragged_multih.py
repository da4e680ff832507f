"""Multi-homography alignment of a ragged batch (pairs of different sizes in one multi_h_batched call): every pair's results equal,
bit for bit (torch.equal, no tolerance), what the pair gives ALONE through the dense path --
multi_h_batched(prepare_device(*upload_raw([pair])), pair_ids=[id]) -- which the parity tests pin to the reference.

Kernel level: rfx_filter_matches_ragged_f32 / rfx_multih_accept_ragged_f32 against the dense entry points called per pair on the
pair's own tensors.  Driver level: device draws (split 1 and 3, both degenerate modes, a shuffled order), explicit draws, background
maps, and the routing of multi_h_pairs.

The driver pairs (PAIRS below; chosen on the MI355X from the 240x320-class sizes and seeds 7-10 of tests/test_gpu_multih.py, heights
and widths varied by multiples of 8, two targets cropped so that source and target shapes differ inside a pair): alone, on the dense
path, they end with nbH = NBH_ALONE = [2, 4, 2, 4, 4, 3, 2] in both degenerate modes (checked by the test) -- every pair accepts two
or more homographies and the pairs stop at three different rounds, so the active list of the lock-step rounds shrinks unevenly."""
import numpy as np
import pytest
import torch
import PIL.Image as Image

from rfx import ops, weights, synth
from rfx.pipeline import AlignPipeline, cell_coords, ragged_multih_tables

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ kernels
def _packed(ts):
    off = np.cumsum([0] + [t.numel() for t in ts[:-1]]).tolist()
    return torch.cat([t.reshape(-1) for t in ts]).contiguous(), off


# (h, w, rt, ct): the three shapes of test_filter_matches_equals_the_aten_glue, a tiny pair that keeps fewer than 4 matches, one more
FILTER_SHAPES = [(240, 320, 15, 20), (96, 312, 10, 33), (376, 1242, 50, 165), (64, 48, 4, 3), (128, 168, 8, 10)]


def test_filter_matches_ragged_equals_filter_matches_per_pair():
    g = torch.Generator().manual_seed(11)
    B = len(FILTER_SHAPES)
    cap = max(rt * ct for _, _, rt, ct in FILTER_SHAPES)
    HA, WA, Ht, Wt, masks, bgs, i1, i2, cnt = [], [], [], [], [], [], [], [], []
    for b, (h, w, rt, ct) in enumerate(FILTER_SHAPES):
        nB, nA = rt * ct, 3 * rt * ct
        W_, H_ = cell_coords(rt, ct, DEV)
        Wt.append(W_); Ht.append(H_)
        WA.append(torch.rand(nA, generator=g).to(DEV)); HA.append(torch.rand(nA, generator=g).to(DEV))
        blob = torch.nn.functional.avg_pool2d(torch.rand(1, 1, h + 16, w + 16, generator=g), 17, 1)[0, 0]
        masks.append((blob > blob.median()).float().to(DEV).contiguous())
        bgs.append((torch.rand(h, w, generator=g) > 0.2).float().to(DEV))
        r1 = torch.zeros(cap, dtype=torch.int64); r2 = torch.zeros(cap, dtype=torch.int64)
        r1[:nB] = torch.sort(torch.randperm(nA, generator=g)[:nB]).values
        r2[:nB] = torch.randperm(nB, generator=g)
        i1.append(r1); i2.append(r2)
        cnt.append([nB, nB // 2, nB - 1, 3, nB][b])
    idx1, idx2 = torch.stack(i1).to(DEV), torch.stack(i2).to(DEV)
    count = torch.tensor(cnt, dtype=torch.int32, device=DEV)
    Mask, moff = _packed(masks)
    BG, _ = _packed(bgs)
    xa, offA = _packed(HA); ya, _ = _packed(WA)
    xb, offB = _packed(Ht); yb, _ = _packed(Wt)
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    geom = torch.tensor([[h, w, rt, ct, h // 8, w // 8] for h, w, rt, ct in FILTER_SHAPES], dtype=torch.int32, device=DEV)
    seen_small = False
    for bg in (None, BG):
        for active in (None, [3, 0, 4], [2], [4, 1, 3, 2]):                 # lists that skip pairs, out of order
            act = None if active is None else torch.tensor(active, dtype=torch.int32, device=DEV)
            M1, M2, n, kept = ops.filter_matches_ragged(idx1, idx2, count, act, Mask, bg, t64(moff), geom, xa, ya, t64(offA), xb, yb,
                                                        t64(offB), want_kept=True)
            for k, b in enumerate(range(B) if active is None else active):
                h, w, rt, ct = FILTER_SHAPES[b]
                r1, r2, rn, rk = ops.filter_matches(idx1[b:b + 1], idx2[b:b + 1], count[b:b + 1], None, masks[b][None],
                                                    None if bg is None else bgs[b][None], rt, ct, HA[b], WA[b], Ht[b], Wt[b],
                                                    want_kept=True)
                assert int(n[k]) == int(rn[0]), (b, active)
                assert torch.equal(M1[k], r1[0]) and torch.equal(M2[k], r2[0]) and torch.equal(kept[k], rk[0]), (b, active)
                seen_small |= int(rn[0]) < 4
                if b == 0 and bg is None:
                    assert 4 < int(rn[0]) < cnt[0]                          # the mask really filters
    assert seen_small


ACCEPT_SHAPES = [((96, 136), (12, 17)), ((50, 70), (6, 8)), ((33, 47), (4, 5)), ((64, 64), (8, 8)), ((120, 90), (15, 11))]


@pytest.mark.parametrize("mode", [0, 1])
def test_multih_accept_ragged_equals_multih_accept_per_pair(mode):
    g = torch.Generator().manual_seed(50 + mode)
    B, max_h = len(ACCEPT_SHAPES), 2
    hw = [h * w for (h, w), _ in ACCEPT_SHAPES]
    assert any(x % 64 for x in hw) and any(x % 256 == 0 for x in hw)
    active = [4, 0, 2, 3]                                                   # pair 1 is not in the round
    a = len(active)
    act = torch.tensor(active, dtype=torch.int32, device=DEV)
    match = [torch.sigmoid(torch.randn(ACCEPT_SHAPES[b][0], generator=g) * 12).to(DEV) for b in active]
    match[2] = torch.zeros_like(match[2])                                   # k = 2 (pair 2): gain 0, accepted only as a first homography
    masks0 = [(torch.rand(s, generator=g) > 0.7).float().to(DEV) for s, _ in ACCEPT_SHAPES]
    bgs = [(torch.rand(s, generator=g) > 0.1).float().to(DEV) for s, _ in ACCEPT_SHAPES]
    # k = 0 (pair 4): accepted on its gain; k = 1 (pair 0): record at capacity; k = 2 (pair 2): first round; k = 3 (pair 3): rejected
    res = torch.tensor([[0, 50, 3, 280], [0, 9, 1, 290], [0, 30, 2, 290], [1, 0, -1, 300]], dtype=torch.int32, device=DEV)
    n_match = torch.tensor([300, 40, 200, 40], dtype=torch.int32, device=DEV)
    nbH0 = torch.tensor([2, 0, 0, 1, 1], dtype=torch.int32, device=DEV)
    bestH = torch.randn(a, 3, 3, generator=g).to(DEV)
    f8 = [torch.randn((2,) + ACCEPT_SHAPES[b][1], generator=g).to(DEV) for b in active]
    m12 = [torch.rand((1,) + ACCEPT_SHAPES[b][1], generator=g).to(DEV) for b in active]
    m21 = [torch.rand((1,) + ACCEPT_SHAPES[b][1], generator=g).to(DEV) for b in active]
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    geom = torch.tensor([[h, w, 1, 1, h8, w8] for (h, w), (h8, w8) in ACCEPT_SHAPES], dtype=torch.int32, device=DEV)
    Match, match_off = _packed(match)
    F8, _ = _packed(f8)
    M12, off8 = _packed(m12)
    M21, _ = _packed(m21)
    th = 0.02
    for use_bg in (True, False):
        Mask, moff = _packed(masks0)
        BG = _packed(bgs)[0] if use_bg else None
        nbH = nbH0.clone()
        R = ops.MultiHRecords.ragged([s[1][0] for s in ACCEPT_SHAPES], [s[1][1] for s in ACCEPT_SHAPES], DEV, max_h=max_h)
        acc, gain = ops.multih_accept_ragged(Match, t64(match_off), Mask, BG, t64(moff), geom, act, res, n_match, nbH, th, mode,
                                             max(hw[b] for b in active), bestH=bestH, flowDown8=F8, match12Down8=M12,
                                             match21Down8=M21, off8=t64(off8), records=R)
        for k, b in enumerate(active):
            (h, w), (h8, w8) = ACCEPT_SHAPES[b]
            m1, n1 = masks0[b][None].clone(), nbH0[b:b + 1].clone()
            R1 = ops.MultiHRecords(1, h8, w8, DEV, max_h=max_h)
            acc1, gain1 = ops.multih_accept(match[k][None], m1, bgs[b][None] if use_bg else None, None, res[k:k + 1], n_match[k:k + 1],
                                            n1, th, mode, bestH=bestH[k:k + 1], flowDown8=f8[k][None], match12Down8=m12[k][None],
                                            match21Down8=m21[k][None], records=R1)
            assert int(acc[k]) == int(acc1[0]), (k, b)
            assert torch.equal(gain[k:k + 1], gain1), (k, b, float(gain[k]), float(gain1[0]))           # bit-equal
            assert torch.equal(Mask[moff[b]:moff[b] + h * w].view(h, w), m1[0]) and int(nbH[b]) == int(n1[0]), (k, b)
            assert torch.equal(R.rec[b, :2], R1.rec[0, :2]) and R.rec[b, 2:4].tolist() == [h8, w8]
            assert torch.equal(R.rec[b, 4:R1.width], R1.rec[0, 4:]) and float(R.rec[b, R1.width:].abs().sum()) == 0
            for x, y in zip(R.views(b), [v[0] for v in R1.views()[:5]]):
                assert torch.equal(x, y)
        # the untouched pair, and the three cases the rule must cover
        assert torch.equal(Mask[moff[1]:moff[1] + hw[1]], masks0[1].reshape(-1)) and int(nbH[1]) == 0 and float(R.rec[1, 1]) == 1
        assert acc.tolist() == [1, 1, 1, 0]
        assert float(gain[2]) <= th and int(nbH[2]) == 1 and float(R.views(2)[1]) == 0                   # first round, gain below th
        assert float(R.views(0)[1]) == 3 and float(R.views(0)[0]) == max_h and int(nbH[0]) == 3          # record at capacity
        assert int(nbH[3]) == 1 and float(R.views(3)[1]) == 1                                            # rejected
    with pytest.raises(ValueError):
        ops.multih_accept_ragged(Match, t64(match_off), torch.zeros(2 * Mask.numel(), device=DEV)[::2], None, t64(moff), geom, act, res,
                                 n_match, nbH, th, mode, max(hw))


# ------------------------------------------------------------------------------------------------ driver
# (seed, H, W, rows / columns cropped off the target): source H x W, target (H - dh) x (W - dw)
PAIRS = [(7, 240, 320, 0, 0), (8, 256, 320, 0, 16), (9, 240, 336, 0, 0), (10, 272, 352, 8, 0), (7, 320, 240, 0, 0), (10, 240, 304, 0, 16)]
NBH_ALONE = [2, 4, 2, 4, 4, 3, 2]        # measured on the MI355X, pair alone on the dense path (the last one: the flat grey pair)


def _pairs():
    out = []
    for seed, H, W, dh, dw in PAIRS:
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
        out.append((I1, I2.crop((0, 0, W - dw, H - dh))))
    out.append((Image.new("RGB", (296, 248), (128, 128, 128)), Image.new("RGB", (328, 240), (128, 128, 128))))     # flat grey
    return out


def _pipe(degenerate="lapack", nbIter=300):
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3, last_std=3.0))
    return AlignPipeline(sds, nbScale=3, nbIter=nbIter, tolerance=0.05, minSize=240, scaleR=1.2, variant="B", device=DEV, seed=5,
                         degenerate=degenerate)


def _up(im):
    return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(DEV)


def _alone(pipe, pair, pid, sample_fn=None, It_bg=None):
    prep = pipe.prepare_device(*pipe.upload_raw([pair]))
    h, w = prep["ItTensor"].shape[2:]
    R = ops.MultiHRecords(1, h // 8, w // 8, DEV)
    out = pipe.multi_h_batched(prep, maxCoarse=3, maskRegionTh=0.01, records=R, pair_ids=[pid], sample_fn=sample_fn, It_bg=It_bg)[0]
    return out, R


def _ragged(pipe, pairs, ids, device_prep=True, **kw):
    prep = pipe.prepare_ragged_device([_up(p[0]) for p in pairs], [_up(p[1]) for p in pairs]) if device_prep else pipe.prepare_ragged(pairs)
    geom = ragged_multih_tables(prep["plan"])["geom"]
    R = ops.MultiHRecords.ragged([g[4] for g in geom], [g[5] for g in geom], DEV)
    outs = pipe.multi_h_batched(prep, maxCoarse=3, maskRegionTh=0.01, records=R, pair_ids=ids, **kw)
    return outs, R, prep


def _assert_pair_equal(o, Rr, b, alone, R1, tag):
    assert o["nbH"] == alone["nbH"] == len(o["H"]), (tag, o["nbH"], alone["nbH"])
    assert torch.equal(o["mask"], alone["mask"]), tag
    for key in ("H", "flowDown8", "matchDown8"):
        assert len(o[key]) == len(alone[key]) and all(torch.equal(x, y) for x, y in zip(o[key], alone[key])), (tag, key)
    n = int(alone["matches"][2])
    assert int(o["matches"][2]) == n and torch.equal(o["matches"][0][:n], alone["matches"][0][:n]), tag
    for x, y in zip(Rr.views(b), [v[0] for v in R1.views()[:5]]):                   # nbH, status, H, flowDown8, matchDown8
        assert torch.equal(x, y), tag
    assert float(Rr.views(b)[1]) == (0.0 if o["nbH"] else 1.0)


@pytest.mark.parametrize("degenerate", ["device", "lapack"])
def test_multi_h_ragged_device_draw_equals_each_pair_alone(degenerate):
    pairs = _pairs()
    ids = [100 + 7 * b for b in range(len(pairs))]
    pipe = _pipe(degenerate)
    alone = [_alone(pipe, p, pid) for p, pid in zip(pairs, ids)]
    nbh = [o["nbH"] for o, _ in alone]
    print("nbH alone (%s):" % degenerate, nbh)
    for split in (1, 3):
        outs, R, prep = _ragged(pipe, pairs, ids, split=split)
        geom = ragged_multih_tables(prep["plan"])["geom"]
        # preconditions: the batch is really ragged and really iterates
        assert len({g[:2] for g in geom}) >= 4 and len({tuple(x.shape) for x in prep["IsTensor"]}) >= 4
        assert max(nbh) >= 2 and len(set(nbh)) >= 2, nbh
        for b in range(len(pairs)):
            _assert_pair_equal(outs[b], R, b, alone[b][0], alone[b][1], (degenerate, split, b))
    order = [4, 6, 1, 0, 5, 3, 2]
    outs, R, _ = _ragged(pipe, [pairs[i] for i in order], [ids[i] for i in order], device_prep=False, split=3)
    for k, i in enumerate(order):
        _assert_pair_equal(outs[k], R, k, alone[i][0], alone[i][1], (degenerate, "shuffled", i))
    assert outs[order.index(6)]["nbH"] == alone[6][0]["nbH"]
    assert nbh == NBH_ALONE


def test_multi_h_ragged_explicit_draws_equal_each_pair_alone():
    pairs = _pairs()[:5]
    ids = [31, 5, 77, 12, 40]
    pipe = _pipe("lapack")

    def draws(pid_of):
        gens = {}

        def fn(b, n, it):
            g = gens.setdefault(b, torch.Generator().manual_seed(1000 + pid_of(b)))
            return torch.randint(n, (it, 4), generator=g)
        return fn
    outs, R, _ = _ragged(pipe, pairs, ids, sample_fn=draws(lambda b: ids[b]), split=3)        # split is forced to 1 by explicit draws
    assert max(o["nbH"] for o in outs) >= 1
    for b, (p, pid) in enumerate(zip(pairs, ids)):
        o1, R1 = _alone(pipe, p, pid, sample_fn=draws(lambda _b, pid=pid: pid))
        _assert_pair_equal(outs[b], R, b, o1, R1, ("explicit", b))


def test_multi_h_ragged_background_maps():
    pairs = _pairs()[:4]
    ids = [3, 4, 5, 6]
    pipe = _pipe("device")
    prep = pipe.prepare_ragged(pairs)
    geom = ragged_multih_tables(prep["plan"])["geom"]
    bg = [None, torch.zeros(geom[1][:2]), torch.ones(geom[2][:2]), None]
    outs, R, _ = _ragged(pipe, pairs, ids, It_bg=bg)
    assert outs[1]["nbH"] == 0 and float(outs[1]["mask"].sum()) == 0
    nb, status, RH, Rf, Rm = R.views(1)
    assert float(nb) == 0 and float(status) == 1 and float(RH.abs().sum() + Rf.abs().sum() + Rm.abs().sum()) == 0
    rest = [0, 2, 3]
    outs2, R2, _ = _ragged(pipe, [pairs[i] for i in rest], [ids[i] for i in rest])             # the same pairs without the blank one
    for k, i in enumerate(rest):
        assert outs[i]["nbH"] == outs2[k]["nbH"] and torch.equal(outs[i]["mask"], outs2[k]["mask"])
        for x, y in zip(R.views(i), R2.views(k)):
            assert torch.equal(x, y), i
    assert max(o["nbH"] for o in outs) >= 1
    with pytest.raises(ValueError):
        pipe.multi_h_batched(prep, maxCoarse=1, It_bg=[torch.ones(3, 3)] * 4)


def test_multi_h_pairs_routing(monkeypatch):
    pipe = _pipe("device")
    calls = dict(dense=0, ragged=0)
    for name, kind in (("filter_matches", "dense"), ("multih_accept", "dense"), ("filter_matches_ragged", "ragged"),
                       ("multih_accept_ragged", "ragged")):
        def counted(*a, _f=getattr(ops, name), _k=kind, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    same = [synth.make_pair(240, 320, seed=s, homography=True) for s in (7, 8)]
    Ra, Rb = ops.MultiHRecords(2, 30, 40, DEV), ops.MultiHRecords(2, 30, 40, DEV)
    a = pipe.multi_h_pairs(same, maxCoarse=2, records=Ra, pair_ids=[1, 2])
    assert calls["ragged"] == 0 and calls["dense"] >= 2                       # a same-size list: the dense path, no ragged entry point
    pipe.multi_h_batched(pipe.prepare(same), maxCoarse=2, records=Rb, pair_ids=[1, 2])
    assert calls["ragged"] == 0 and torch.equal(Ra.rec, Rb.rec) and a[0]["nbH"] >= 1
    mixed = _pairs()[:3]
    n_dense = calls["dense"]
    outs = pipe.multi_h_pairs(mixed, maxCoarse=2, pair_ids=[1, 2, 3])
    assert calls["ragged"] >= 2 and calls["dense"] == n_dense
    ref = pipe.multi_h_batched(pipe.prepare_ragged(mixed), maxCoarse=2, pair_ids=[1, 2, 3])
    for x, y in zip(outs, ref):
        assert x["nbH"] == y["nbH"] and torch.equal(x["mask"], y["mask"]) and all(torch.equal(p, q) for p, q in zip(x["H"], y["H"]))
    assert tuple(outs[0]["mask"].shape) != tuple(outs[1]["mask"].shape)
