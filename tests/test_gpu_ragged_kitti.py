"""The KITTI multi-homography driver on a ragged batch (pairs of different sizes in one multi_h_kitti_batched call): every pair's
results equal, bit for bit (torch.equal, no tolerance), what the pair gives ALONE through the dense driver with the same pair id.

Kernel level: rfx_remove_small_cc_ragged_f32 against the dense filter called on each map alone and against the host labelling;
the flowD2 record store of rfx_multih_accept_ragged_d2_f32 against rfx_multih_accept_f32 on each pair alone.  Driver level: device
draws (both degenerate modes, split 1 and 2, the capacity stop), explicit draws with an injected host filter, background maps,
refusals and routing.

The driver pairs (PAIRS below) are 96x312-class synthetic pairs of three original sizes; two share a size, and (96,312) / (97,315)
resize to the same coarse (160,512), fine (200,648) and half-resolution (96,328) shapes while their originals differ.  The CPU port
(oracle/restate.multi_h_loop_kitti, same parameters, CPU draws seeded with torch.manual_seed(101) per pair) gives pair 1 three
homographies, pair 2 one and the others two, i.e. both preconditions the driver test asserts -- a pair with two or more homographies,
pairs that stop in different rounds -- hold there already; with the device draws keyed by IDS the MI355X gives the same counts,
NBH_ALONE, in both degenerate modes (checked by the test)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import restate
from rfx import ops, rounds, weights, synth
from rfx.pipeline import AlignPipeline, ragged_kitti_tables

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _packed(ts, lead=0):
    off = (np.cumsum([0] + [t.numel() for t in ts[:-1]]) + lead).tolist()
    return torch.cat([torch.zeros(lead, device=ts[0].device)] + [t.reshape(-1) for t in ts]).contiguous(), off


def _t64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------ the ragged filter
# the (7,9) map first: 63 pixels, so that no later offset is a multiple of 64
CC_SHAPES = [(7, 9), (96, 136), (50, 70), (33, 47), (64, 64), (120, 90)]


def _blob_maps():
    g = torch.Generator().manual_seed(5)
    maps = []
    for k, (H, W) in enumerate(CC_SHAPES):
        sigma = (1.0, 3.0, 2.0, 1.0, 3.0, 6.0)[k]
        n = torch.randn(1, 1, H, W, generator=g)
        kk = int(4 * sigma) | 1
        ax = torch.arange(kk) - kk // 2
        ker = torch.exp(-ax.float() ** 2 / (2 * sigma ** 2))
        ker = (ker[:, None] * ker[None, :]) / ker.sum() ** 2
        sm = F.conv2d(n, ker[None, None], padding=kk // 2)[0, 0]
        maps.append((torch.sigmoid(40 * sm / sm.std()) * 0.999999).contiguous())
    return maps


def _constructed_maps():
    m = [torch.zeros(s) for s in CC_SHAPES]
    m[0][:] = 1.0                                    # (b) entirely foreground: never removed; its last row touches ...
    m[1][0, :] = 1.0                                 # (a) ... the entirely-foreground first row of the next map (w 9 != 136)
    m[1][40:45, 20:28] = 0.995                       # (c) a 40-pixel blob: removed at cc_th 0.01 in 96x136 (130 px pass) ...
    m[2][20:25, 20:28] = 0.995                       #     ... kept in 50x70 (35 px pass)
    m[1][60, 3:134] = 1.0                            # (d) a 131-pixel run over three 64-pixel segments, width 136
    m[2][49, :] = 1.0                                # (a) last row of 50x70 (70 px) against the first row of 33x47 (47 px): at
    m[3][0, :] = 1.0                                 #     cc_th 0.05 each is removed alone (175 / 77 px pass), merged neither would be
    for i in range(30):                              # (e) chains that only 8-connectivity joins (NW / NE neighbours)
        m[4][i, i] = 1.0
        m[4][63 - i, i] = 0.995 if i < 12 else 0.0
    m[5][50:52, :] = 1.0                             # (d) two full rows of a 90-wide map: runs that start anywhere in a segment
    m[5][100, 7:83] = 0.9901
    return m


def _check_pack(maps, order, cc_ths):
    """Pack ``maps`` in their order with a 0-element lead, filter the maps listed in ``order`` in one call, compare each with the dense
    filter and the host labelling on that map alone; maps not listed stay as they were."""
    dev_maps = [x.to(DEV) for x in maps]
    buf, off = _packed(dev_maps)
    assert all(o % 64 for o in off[1:])
    hw = [tuple(x.shape) for x in maps]
    for cc_th in cc_ths:
        out = ops.remove_small_cc_ragged(buf, _t64([off[k] for k in order]), [hw[k] for k in order], cc_th, 0.99)
        assert out.data_ptr() != buf.data_ptr() and torch.equal(buf, _packed(dev_maps)[0])                 # the input is untouched
        for k, (h, w) in enumerate(hw):
            got = out[off[k]:off[k] + h * w].view(h, w)
            if k not in order:
                assert torch.equal(got, dev_maps[k]), (k, cc_th)
                continue
            assert torch.equal(got, ops.remove_small_cc(dev_maps[k], cc_th, 0.99)), (k, cc_th)
            assert np.array_equal(got.cpu().numpy(), restate.remove_small_cc_eval(maps[k].numpy().copy(), 0.99, cc_th)), (k, cc_th)
        inpl = buf.clone()
        assert ops.remove_small_cc_ragged(inpl, _t64([off[k] for k in order]), [hw[k] for k in order], cc_th, 0.99, inplace=True) is inpl
        assert torch.equal(inpl, out), cc_th
    return buf, off


def test_remove_small_cc_ragged_equals_the_dense_filter_and_the_host_labelling_per_map():
    allk = list(range(len(CC_SHAPES)))
    _check_pack(_blob_maps(), allk, (0.01, 0.05, 0.3))
    con = _constructed_maps()
    buf, off = _check_pack(con, allk, (0.01, 0.05))
    # the constructed cases do what they were built for (on the dense filter, which the ragged one equals)
    alone = lambda k, th: ops.remove_small_cc(con[k].to(DEV), th, 0.99)
    assert ops.cc_max_area(96 * 136, 0.01) == 130 and ops.cc_max_area(50 * 70, 0.01) == 35
    assert float(alone(1, 0.01)[40, 20]) == 0 and float(alone(2, 0.01)[20, 20]) > 0                          # (c) per-map max_area
    assert float(alone(2, 0.05)[49, 0]) == 0 and float(alone(3, 0.05)[0, 0]) == 0                            # (a) removed alone
    assert torch.equal(alone(0, 1.0), con[0].to(DEV))                                                        # (b) the whole image stays
    assert float(alone(4, 0.01)[0, 0]) == 0 and float(alone(4, 0.0005)[5, 5]) > 0       # (e) ONE 30-pixel component: 40 px pass / 2 px pass
    # a subset of the maps in permuted order
    _check_pack(con, [4, 1, 5], (0.01, 0.05))
    _check_pack(_blob_maps(), [5, 0, 3, 2], (0.05,))
    # the identity, the device-table form, and the refusals every op has
    o = _t64(off)
    assert ops.remove_small_cc_ragged(buf, o, [tuple(x.shape) for x in con], 0) is buf
    rows = ops.cc_dims_table([tuple(x.shape) for x in con], 0.05)
    tab = torch.tensor(rows, dtype=torch.int32, device=DEV)
    assert torch.equal(ops.remove_small_cc_ragged(buf, o, tab, 0.05, max_hw=max(h * w for h, w, _ in rows)),
                       ops.remove_small_cc_ragged(buf, o, [tuple(x.shape) for x in con], 0.05))
    with pytest.raises(RuntimeError):
        ops.remove_small_cc_ragged(buf.cpu(), o, [tuple(x.shape) for x in con], 0.05)
    with pytest.raises(ValueError):
        ops.remove_small_cc_ragged(buf, o[:3], [tuple(x.shape) for x in con], 0.05)
    # a table row that does not fit the buffer is skipped, not followed
    bad = ops.remove_small_cc_ragged(buf, _t64([off[0], buf.numel() - 10]), [CC_SHAPES[0], (50, 70)], 0.05)
    assert torch.equal(bad, buf)


# ------------------------------------------------------------------------------------------------ the flowD2 record store
from test_gpu_ragged_multih import ACCEPT_SHAPES  # noqa: E402

D2_SHAPES = [(6, 9), (3, 4), (2, 3), (4, 4), (8, 6)]


def test_ragged_accept_stores_flowD2_like_the_dense_kernel_per_pair():
    g = torch.Generator().manual_seed(61)
    B, max_h, mode, th = len(ACCEPT_SHAPES), 3, 1, 0.02
    active = [4, 0, 2, 3]                                                   # pair 1 is not in the round
    a = len(active)
    act = torch.tensor(active, dtype=torch.int32, device=DEV)
    match = [torch.sigmoid(torch.randn(ACCEPT_SHAPES[b][0], generator=g) * 12).to(DEV) for b in active]
    masks0 = [(torch.rand(s, generator=g) > 0.7).float().to(DEV) for s, _ in ACCEPT_SHAPES]
    bgs = [(torch.rand(s, generator=g) > 0.1).float().to(DEV) for s, _ in ACCEPT_SHAPES]
    # k = 0 (pair 4): nbH 1; k = 1 (pair 0): nbH max_h - 1, the last slot; k = 2 (pair 2): nbH 0; k = 3 (pair 3): rejected (status 1)
    res = torch.tensor([[0, 50, 3, 280], [0, 9, 1, 290], [0, 30, 2, 290], [1, 0, -1, 300]], dtype=torch.int32, device=DEV)
    n_match = torch.tensor([300, 40, 200, 40], dtype=torch.int32, device=DEV)
    nbH0 = torch.tensor([max_h - 1, 0, 0, 1, 1], dtype=torch.int32, device=DEV)
    bestH = torch.randn(a, 3, 3, generator=g).to(DEV)
    f8 = [torch.randn((2,) + ACCEPT_SHAPES[b][1], generator=g).to(DEV) for b in active]
    m12 = [torch.rand((1,) + ACCEPT_SHAPES[b][1], generator=g).to(DEV) for b in active]
    m21 = [torch.rand((1,) + ACCEPT_SHAPES[b][1], generator=g).to(DEV) for b in active]
    fd2 = [torch.randn((2,) + D2_SHAPES[b], generator=g).to(DEV) for b in active]
    geom = torch.tensor([[h, w, 1, 1, h8, w8] for (h, w), (h8, w8) in ACCEPT_SHAPES], dtype=torch.int32, device=DEV)
    Match, match_off = _packed(match)
    F8, _ = _packed(f8)
    M12, off8 = _packed(m12)
    M21, _ = _packed(m21)
    FD2, offd2 = _packed(fd2)
    offd2 = [o // 2 for o in offd2]
    hw = [h * w for (h, w), _ in ACCEPT_SHAPES]
    for use_bg in (True, False):
        Mask, moff = _packed(masks0)
        BG = _packed(bgs)[0] if use_bg else None
        nbH = nbH0.clone()
        R = ops.MultiHRecords.ragged([s[1][0] for s in ACCEPT_SHAPES], [s[1][1] for s in ACCEPT_SHAPES], DEV, max_h=max_h,
                                     hd2_list=[d[0] for d in D2_SHAPES], wd2_list=[d[1] for d in D2_SHAPES])
        acc, gain = ops.multih_accept_ragged(Match, _t64(match_off), Mask, BG, _t64(moff), geom, act, res, n_match, nbH, th, mode,
                                             max(hw[b] for b in active), bestH=bestH, flowDown8=F8, match12Down8=M12, match21Down8=M21,
                                             off8=_t64(off8), records=R, flowD2=FD2, offd2=_t64(offd2))
        for k, b in enumerate(active):
            (h, w), (h8, w8) = ACCEPT_SHAPES[b]
            hd2, wd2 = D2_SHAPES[b]
            m1, n1 = masks0[b][None].clone(), nbH0[b:b + 1].clone()
            R1 = ops.MultiHRecords(1, h8, w8, DEV, max_h=max_h, hd2=hd2, wd2=wd2)
            acc1, gain1 = ops.multih_accept(match[k][None], m1, bgs[b][None] if use_bg else None, None, res[k:k + 1], n_match[k:k + 1],
                                            n1, th, mode, bestH=bestH[k:k + 1], flowDown8=f8[k][None], match12Down8=m12[k][None],
                                            match21Down8=m21[k][None], flowD2=fd2[k][None], records=R1)
            assert int(acc[k]) == int(acc1[0]) and torch.equal(gain[k:k + 1], gain1), (k, b)
            assert torch.equal(Mask[moff[b]:moff[b] + h * w].view(h, w), m1[0]) and int(nbH[b]) == int(n1[0]), (k, b)
            # the row of one pair IS the dense row: same offsets, same floats, zeros behind
            assert (R.off_match[b], R.off_d2[b]) == (R1.off_match, R1.off_d2)
            assert torch.equal(R.rec[b, :2], R1.rec[0, :2]) and R.rec[b, 2:4].tolist() == [h8, w8]
            assert torch.equal(R.rec[b, 4:R1.width], R1.rec[0, 4:]) and float(R.rec[b, R1.width:].abs().sum()) == 0, (k, b)
            v, v1 = R.views(b), R1.views()
            assert len(v) == 6 and all(torch.equal(x, y[0]) for x, y in zip(v, v1))
        assert acc.tolist() == [1, 1, 1, 0]
        slot = {4: 1, 0: max_h - 1, 2: 0}
        for k, b in enumerate(active[:3]):                                  # the flowD2 slot the pair filled, and only that one
            d2 = R.views(b)[5]
            assert torch.equal(d2[slot[b]], fd2[k]) and float(d2.abs().sum()) == float(fd2[k].abs().sum())
        assert float(R.views(3)[5].abs().sum()) == 0 and float(R.views(1)[5].abs().sum()) == 0      # rejected / not in the round
        assert float(R.views(0)[0]) == max_h and float(R.views(0)[1]) == 0                           # filled to capacity, no overflow
    # records and operands must agree
    R0 = ops.MultiHRecords.ragged([s[1][0] for s in ACCEPT_SHAPES], [s[1][1] for s in ACCEPT_SHAPES], DEV, max_h=max_h)
    args = (Match, _t64(match_off), Mask, None, _t64(moff), geom, act, res, n_match, nbH0.clone(), th, mode, max(hw))
    with pytest.raises(ValueError):
        ops.multih_accept_ragged(*args, bestH=bestH, records=R0, flowD2=FD2, offd2=_t64(offd2))
    with pytest.raises(ValueError):
        ops.multih_accept_ragged(*args, bestH=bestH, records=R)


# ------------------------------------------------------------------------------------------------ driver
# (seed, H, W, rows cropped off the target, amp of the synthetic homography): source H x W, target (H - dh) x W.  Pairs 0 and 1 share their shapes; pairs 0 / 1 and 4
# resize to the same coarse, fine and half-resolution shapes but differ in their originals; pair 3's source and target differ.
PAIRS = [(11, 96, 312, 0, 0.03), (33, 96, 312, 0, 0.08), (30, 94, 311, 0, 0.08), (14, 104, 320, 4, 0.03), (15, 97, 315, 0, 0.03)]
IDS = [40, 33, 30, 3, 28]
NBH_ALONE = [2, 3, 1, 2, 2]
KW = dict(fineSize=200, maskRegionTh=0.005, cc_th=0.01)
_PIPES, _ALONE = {}, {}


def _pairs():
    out = []
    for seed, H, W, dh, amp in PAIRS:
        I1, I2 = synth.make_pair(H, W, seed=seed, homography=True, amp=amp)
        out.append((I1, I2.crop((0, 0, W, H - dh))))
    return out


def _up(im):
    return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(DEV)


def _pipe(degenerate):
    if degenerate not in _PIPES:
        sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
                   match=weights.net_matchability_sd(3, last_std=3.0))
        _PIPES[degenerate] = AlignPipeline(sds, nbScale=3, nbIter=300, tolerance=0.05, minSize=160, scaleR=1.2, variant="B", device=DEV,
                                           seed=7, degenerate=degenerate)
    return _PIPES[degenerate]


def _tables(pipe, pairs):
    plan = pipe._ragged_plan([p[0].size for p in pairs], [p[1].size for p in pairs])
    return ragged_kitti_tables(plan, [p[1].size for p in pairs], KW["fineSize"])


def _records(tabs, max_h):
    return ops.MultiHRecords.ragged([g[4] for g in tabs["geom"]], [g[5] for g in tabs["geom"]], DEV, max_h=max_h,
                                    hd2_list=[d[0] for d in tabs["d2"]], wd2_list=[d[1] for d in tabs["d2"]])


def _alone(degenerate, max_h=8):
    """Every pair ALONE through the dense driver (computed once per mode and record capacity, shared by the tests)."""
    key = (degenerate, max_h)
    if key not in _ALONE:
        pipe, pairs = _pipe(degenerate), _pairs()
        tabs = _tables(pipe, pairs)
        res = []
        for b, (p, pid) in enumerate(zip(pairs, IDS)):
            (h8, w8), (hd2, wd2) = tabs["geom"][b][4:6], tabs["d2"][b]
            R1 = ops.MultiHRecords(1, h8, w8, DEV, max_h=max_h, hd2=hd2, wd2=wd2)
            out = pipe.multi_h_kitti_batched(_up(p[0])[None], _up(p[1])[None], records=R1, pair_ids=[pid], **KW)[0]
            res.append((out, R1))
        _ALONE[key] = res
    return _ALONE[key]


def _assert_pair_equal(o, Rr, b, alone, R1, tag):
    assert o["nbH"] == alone["nbH"] == len(o["H"]), (tag, o["nbH"], alone["nbH"])
    assert torch.equal(o["mask"], alone["mask"]), tag
    for key in ("H", "flowD2", "flowDown8", "matchDown8"):
        assert len(o[key]) == len(alone[key]) and all(torch.equal(x, y) for x, y in zip(o[key], alone[key])), (tag, key)
    v, v1 = Rr.views(b), R1.views()
    assert len(v) == 6 and all(torch.equal(x, y[0]) for x, y in zip(v, v1)), tag
    assert torch.equal(Rr.rec[b, :2], R1.rec[0, :2]) and torch.equal(Rr.rec[b, 4:R1.width], R1.rec[0, 4:]), tag
    assert float(Rr.rec[b, R1.width:].abs().sum()) == 0, tag


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("degenerate", ["lapack", "device"])
def test_kitti_ragged_device_draws_equal_each_pair_alone(degenerate, split):
    pipe, pairs = _pipe(degenerate), _pairs()
    tabs = _tables(pipe, pairs)
    # preconditions on the batch: three original-shape combinations, a shared one, and equal resized shapes over different originals
    assert len({(p[0].size, p[1].size) for p in pairs}) >= 3 and pairs[0][1].size == pairs[1][1].size
    assert tabs["org"][0] != tabs["org"][4] and tabs["resize"][0] == tabs["resize"][4] and tabs["half"][0] == tabs["half"][4]
    assert tabs["geom"][0][2:] == tabs["geom"][4][2:]
    alone = _alone(degenerate)
    nbh = [o["nbH"] for o, _ in alone]
    print("nbH alone (%s):" % degenerate, nbh)
    assert max(nbh) >= 2 and len(set(nbh)) >= 2, nbh             # a pair iterates, and the active list shrinks before the last round
    assert nbh == NBH_ALONE, nbh
    src, tgt = [_up(p[0]) for p in pairs], [_up(p[1])[None] for p in pairs]             # (H,W,3) and (1,H,W,3) entries
    R = _records(tabs, 8)
    outs = pipe.multi_h_kitti_batched(src, tgt, records=R, pair_ids=IDS, split=split, **KW)
    for b in range(len(pairs)):
        _assert_pair_equal(outs[b], R, b, alone[b][0], alone[b][1], (degenerate, split, b))
        assert tuple(outs[b]["mask"].shape) == tabs["org"][b]
    # the capacity stop: a record of one slot ends every pair that accepts after one round, status 4
    alone1 = _alone(degenerate, 1)
    Rc = _records(tabs, 1)
    outc = pipe.multi_h_kitti_batched(src, tgt, records=Rc, pair_ids=IDS, split=split, **KW)
    for b in range(len(pairs)):
        _assert_pair_equal(outc[b], Rc, b, alone1[b][0], alone1[b][1], (degenerate, split, b, "capped"))
    assert bool((Rc.rec[:, 1] == 4.0).any()) and max(o["nbH"] for o in outc) == 1


def test_kitti_ragged_explicit_draws_and_a_host_filter_equal_the_per_pair_driver():
    """Tolerances: those of test_kitti_lock_step_driver_equals_the_per_pair_driver (tests/test_gpu_pipeline.py)."""
    pipe, pairs = _pipe("lapack"), _pairs()

    def draws(b, k, n, it):
        return torch.randint(n, (it, 4), generator=torch.Generator().manual_seed(1000 * b + k))
    order = []

    def host_filter(m, match_th, cc_th):
        order.append(m.shape)
        return restate.remove_small_cc_eval(m, match_th, cc_th)
    single = []
    for b, p in enumerate(pairs):
        calls = [0]

        def fn(n, it, b=b, calls=calls):
            calls[0] += 1
            return draws(b, calls[0], n, it)
        single.append(pipe.multi_h_kitti(_up(p[0])[None], _up(p[1])[None], sample_fn=fn, remove_small_cc=restate.remove_small_cc_eval, **KW))
    ncall = [0] * len(pairs)

    def fnb(b, n, it):
        ncall[b] += 1
        return draws(b, ncall[b], n, it)
    batched = pipe.multi_h_kitti_batched([_up(p[0]) for p in pairs], [_up(p[1]) for p in pairs], sample_fn=fnb, remove_small_cc=host_filter,
                                         split=2, **KW)                                  # explicit draws / a host filter force one group
    assert max(len(o["H"]) for o in single) >= 2
    assert order[:len(pairs)] == [(p[1].size[1], p[1].size[0]) for p in pairs]           # the host filter is called in pair order
    for b, (s1, m) in enumerate(zip(single, batched)):
        assert len(s1["H"]) == len(m["H"]), (b, len(s1["H"]), len(m["H"]))
        for k in range(len(s1["H"])):
            assert (s1["H"][k] - m["H"][k]).abs().max() < 1e-6
            assert (s1["flowD2"][k] - m["flowD2"][k]).abs().max() < 1e-5
            assert (s1["flowDown8"][k] - m["flowDown8"][k]).abs().max() < 1e-5
            assert (s1["matchDown8"][k] - m["matchDown8"][k]).abs().max() < 1e-5
        assert float((s1["mask"] != m["mask"]).float().mean()) < 1e-4


def test_kitti_ragged_background_maps_refusals_and_routing(monkeypatch):
    pipe, pairs = _pipe("device"), _pairs()
    two, ids = [pairs[2], pairs[3]], [IDS[2], IDS[3]]
    tabs = _tables(pipe, two)
    h, w = tabs["org"][0]
    bg0 = torch.ones(h, w)
    bg0[:, : w // 2] = 0                                                     # the left half of pair 0's target is background
    src, tgt = [_up(p[0]) for p in two], [_up(p[1]) for p in two]
    R = _records(tabs, 8)
    outs = pipe.multi_h_kitti_batched(src, tgt, It_bg=[bg0, None], records=R, pair_ids=ids, **KW)
    for b, bg in enumerate((bg0[None], None)):
        (h8, w8), (hd2, wd2) = tabs["geom"][b][4:6], tabs["d2"][b]
        R1 = ops.MultiHRecords(1, h8, w8, DEV, max_h=8, hd2=hd2, wd2=wd2)
        o1 = pipe.multi_h_kitti_batched(src[b][None], tgt[b][None], It_bg=bg, records=R1, pair_ids=[ids[b]], **KW)[0]
        _assert_pair_equal(outs[b], R, b, o1, R1, ("bg", b))
    assert torch.equal(outs[1]["mask"], _alone("device")[3][0]["mask"])      # the pair without a map: as with no maps at all
    with pytest.raises(ValueError):
        pipe.multi_h_kitti_batched(src, tgt, It_bg=[torch.ones(3, 3), None], **KW)
    with pytest.raises(ValueError):
        pipe.multi_h_kitti_batched(src, tgt, It_bg=[bg0], **KW)
    with pytest.raises(ValueError, match="MultiHRecordsRagged"):
        pipe.multi_h_kitti_batched(src, tgt, records=ops.MultiHRecords(2, tabs["geom"][0][4], tabs["geom"][0][5], DEV, hd2=tabs["d2"][0][0],
                                                                       wd2=tabs["d2"][0][1]), **KW)
    with pytest.raises(ValueError, match="MultiHRecordsRagged"):             # ragged records without the d2 lists
        pipe.multi_h_kitti_batched(src, tgt, records=ops.MultiHRecords.ragged([g[4] for g in tabs["geom"]], [g[5] for g in tabs["geom"]], DEV),
                                   **KW)
    # a same-shape list takes the dense path: the ragged group is never built, and the result is the stacked call's
    built = []
    real = rounds.RaggedKittiGroup
    monkeypatch.setattr(rounds, "RaggedKittiGroup", lambda *a, **k: built.append(1) or real(*a, **k))
    same = pairs[:2]
    s_l, t_l = [_up(p[0]) for p in same], [_up(p[1]) for p in same]
    a = pipe.multi_h_kitti_batched(s_l, t_l, pair_ids=IDS[:2], **KW)
    assert not built
    b = pipe.multi_h_kitti_batched(torch.stack(s_l), torch.stack(t_l), pair_ids=IDS[:2], **KW)
    for x, y in zip(a, b):
        assert x["nbH"] == y["nbH"] and torch.equal(x["mask"], y["mask"]) and all(torch.equal(p, q) for p, q in zip(x["H"], y["H"]))
    c = pipe.multi_h_kitti_pairs(same, pair_ids=IDS[:2], **KW)
    assert not built and all(x["nbH"] == y["nbH"] and torch.equal(x["mask"], y["mask"]) for x, y in zip(c, b))
    pipe.multi_h_kitti_pairs(two, pair_ids=ids, **KW)
    assert built
