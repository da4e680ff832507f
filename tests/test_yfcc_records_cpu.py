"""Host side of the YFCC path for batches of different sizes (want_records of multi_h_variant_c, csrc/points_ragged.hip:
rfx_flow_points_ragged_f32, ops.flow_points_ragged / matches_from_flow_ragged, assemble.yfcc_matches_records / yfcc_norm_kp): the
table, header and binding, the refusals that need no device, the ragged rule stated in numpy as a loop of the per-map rule of
tests/test_points_cpu.py -- held against the reference's own outputs in tests/golden/points.npz taken as ONE batch -- and
yfcc_norm_kp against a transcription of the script's arithmetic (and the live function where the reference is present).  Nothing
is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rfx import _lib, assemble, ops
from test_points_cpu import TILE, golden, rule_points, sha
from test_ragged_variant_c_cpu import _bare_pipe, _img

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rfx_flow_points_ragged_ws_bytes", "rfx_flow_points_ragged_f32")


# ---------------------------------------------------------------- the rule

def rule_points_ragged(flows, keeps, sizesA, angles, bgs=None):
    """flows[b] (H_b,W_b,2) float32, keeps[b] / bgs[b] (H_b,W_b) -> (pts1, pts2, offsets (B+1,)): the per-map rule, map after map, each
    with its own angle and source size; the unrotated target size is the map's shape turned back."""
    p1, p2, off = [], [], [0]
    for b, (f, m, sizeA, angle) in enumerate(zip(flows, keeps, sizesA, angles)):
        H, W = m.shape
        sizeB = (W, H) if (angle // 90) % 2 == 0 else (H, W)
        a, c, o = rule_points(f[None], m[None], sizeA, sizeB, angle, None if bgs is None else bgs[b][None])
        p1.append(a), p2.append(c), off.append(off[-1] + int(o[1]))
    return np.concatenate(p1), np.concatenate(p2), np.asarray(off, np.int64)


def golden_batch():
    """The goldens as ONE ragged batch: the (th, multiH) cases times the four angles, each map with its own k -- for odd k the same
    pixels laid out as the turned map.  -> (flows, keeps, sizesA, angles, [(case, angle index)])."""
    G = golden()
    H, W = G["hw"]
    flows, keeps, sizesA, angles, tags = [], [], [], [], []
    for c, (_, _, flow, binary) in enumerate(G["cases"]):
        for a, angle in enumerate(G["angles"]):
            wB, hB = G["sizeB"][a]
            shape = (hB, wB) if (angle // 90) % 2 == 0 else (wB, hB)
            assert shape[0] * shape[1] == H * W
            flows.append(flow.reshape(shape + (2,))), keeps.append(binary.reshape(shape))
            sizesA.append(G["sizeA"][a]), angles.append(angle), tags.append((c, a))
    return flows, keeps, sizesA, angles, tags


def test_ragged_rule_gives_the_reference_outputs_of_the_goldens_as_one_batch():
    g = golden()["raw"]
    flows, keeps, sizesA, angles, tags = golden_batch()
    assert len(flows) == 12 and len({k.shape for k in keeps}) >= 1
    pts1, pts2, off = rule_points_ragged(flows, keeps, sizesA, angles)
    assert off[0] == 0 and off[-1] == len(pts1) == len(pts2)
    for b, (c, a) in enumerate(tags):
        rows = slice(off[b], off[b + 1])
        assert off[b + 1] - off[b] == int(g["case%d_a%d_n" % (c, a)])
        assert sha(pts1[rows]) == str(g["case%d_a%d_sha1" % (c, a)]) and sha(pts2[rows]) == str(g["case%d_a%d_sha2" % (c, a)]), (c, a)
        if (c, a) == (int(g["full_case"]), int(g["full_angle"])):
            assert np.array_equal(pts1[rows].view(np.int32), g["full_pts1"].view(np.int32))
            assert np.array_equal(pts2[rows], g["full_pts2"].astype(np.int64))


# ---------------------------------------------------------------- the table

def test_table_is_a_pure_function_of_the_size_lists():
    sizes = [(1, 1), (31, 33), (32, 32), (25, 41), (17, 241)]                  # 1, 1023, 1024, 1025, 4097 pixels
    assert [h * w for h, w in sizes] == [1, TILE - 1, TILE, TILE + 1, 4 * TILE + 1]
    sizesA = [(640 + b, 480 - b) for b in range(5)]
    rows, total, tiles = ops.flow_points_ragged_table(sizes, sizesA, [0, 90, 180, 270, 450])
    assert total == 7170 and tiles == 1 + 1 + 1 + 2 + 5
    assert [r[0] for r in rows] == [0, 1, 1024, 2048, 3073]                    # pixel offsets: no gaps
    assert [r[6] for r in rows] == [0, 1, 2, 3, 5]                             # first tiles: ceil(H W / 1024) each
    assert [r[3] for r in rows] == [0, 1, 2, 3, 1] and [(r[1], r[2]) for r in rows] == sizes
    assert [(r[4], r[5]) for r in rows] == sizesA and all(r[7] == 0 and len(r) == 8 for r in rows)
    assert ops.flow_points_ragged_table(sizes, sizesA, [0, 90, 180, 270, 450]) == (rows, total, tiles)
    assert ops.flow_points_ragged_table(sizes, sizesA, 180)[0][3][3] == 2     # one angle for all
    assert ops.flow_points_ragged_table([(2, 3)] * 9000, [(5, 5)] * 9000, 0)[1:] == (54000, 9000)
    for bad in (dict(sizes=sizes[:4]), dict(sizesA=sizesA[:4]), dict(angles=[0] * 4), dict(angles=[0, 0, 45, 0, 0]), dict(sizes=[]),
                dict(angles=[0, 0, 0, 0, 90.5]), dict(sizesA=[(0, 5)] + sizesA[1:]), dict(sizesA=sizesA[:4] + [(5, -1)]),
                dict(sizes=[(0, 3)] + sizes[1:]), dict(sizes=sizes[:4] + [(3, -2)])):
        kw = dict(dict(sizes=sizes, sizesA=sizesA, angles=[0] * 5), **bad)
        if bad == dict(sizes=[]):
            kw.update(sizesA=[], angles=[])
        with pytest.raises(ValueError):
            ops.flow_points_ragged_table(**kw)


def test_odd_turns_swap_the_target_size():
    """(wB, hB) follows from (H, W, k): the numpy rule on a (H, W) map at odd k is the per-map rule with sizeB = (H, W)."""
    rng = np.random.RandomState(4)
    H, W = 3, 5
    flow, keep = (rng.rand(H, W, 2) * 2 - 1).astype(np.float32), rng.rand(H, W) < 0.6
    gx, gy = np.meshgrid(np.arange(H), np.arange(W))                           # the unrotated target is (hB, wB) = (W, H)
    turned = np.rot90(np.stack((gx, gy), axis=2), 1)
    assert turned.shape[:2] == (H, W)
    _, pts2, off = rule_points_ragged([flow, flow], [keep, np.ones_like(keep)], [(7, 9), (7, 9)], [90, 0])
    assert np.array_equal(pts2[:off[1]], turned[keep]) and pts2[off[1]:].max(axis=0).tolist() == [W - 1, H - 1]


# ---------------------------------------------------------------- header, binding, library

def test_header_and_binding_declare_the_two_entries_under_abi_17():
    C = ctypes
    text = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.search(r"#define RFX_ABI_VERSION 17\b", text) and _lib.ABI_VERSION == 17
    kinds = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "size_t": C.c_size_t}
    for name in NAMES:
        ret, args = re.search(r"\b(int|size_t)\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S).groups()
        res, argtypes = _lib.SIGNATURES[name]
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[ret], name
        params = [" ".join(p.split()) for p in args.split(",")]
        assert [C.c_void_p if "*" in p else kinds[p.rsplit(" ", 1)[0].replace("const ", "")] for p in params] == argtypes, (name, params)
    assert len(_lib.SIGNATURES["rfx_flow_points_ragged_f32"][1]) == 12
    block = text[text.index("rfx_flow_points_f32 for B maps"):text.index("size_t rfx_flow_points_ragged_ws_bytes")]
    assert "evaluation/evalYFCC/getResults.py:53-71" in block and "ADDED" in block and "ABI 17" in block
    lib = _lib.load()
    assert lib.rfx_abi_version() == 17
    ws = lib.rfx_flow_points_ragged_ws_bytes
    assert ws(10) == 40 and ws(1) == 4 and ws(0) == ws(-3) == 0 and ws(1 << 31) == 4 << 31
    raw = ctypes.CDLL(_lib.LIB_PATH)                                             # the library itself, without the binding's table
    assert all(hasattr(raw, name) for name in NAMES + ("rfx_flow_points_f32",)) and not hasattr(raw, "rfx_flow_points_ragged")


def test_argument_checks_answer_before_any_device_call():
    """Every call carries at least one defect and returns from the opening checks; the fake, aligned pointers are never followed."""
    lib = _lib.load()
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]
    null = ctypes.c_void_p(0)
    E_ARG, E_LIMIT = -1, -2

    def points(flow=P[0], keep=P[1], bg=P[2], table=P[3], B=1, total_px=0, total_tiles=1, pts1=P[4], pts2=P[5], offsets=P[6], ws=P[7]):
        return lib.rfx_flow_points_ragged_f32(flow, keep, bg, table, B, total_px, total_tiles, pts1, pts2, offsets, ws, null)
    assert points() == E_ARG                                                    # total_px = 0: the defect every call below adds to
    for name in ("flow", "keep", "table", "pts1", "pts2", "offsets", "ws"):
        assert points(**{name: null, "total_px": 48}) == E_ARG, name
        assert points(**{name: null, "bg": null, "total_px": 48}) == E_ARG, name
    for bad in (dict(B=0), dict(B=-1), dict(total_px=-5), dict(total_tiles=0), dict(total_tiles=-1), dict(total_tiles=49)):
        assert points(**dict(dict(total_px=48), **bad)) == E_ARG, bad
    for name, addr in (("flow", 0x10004), ("table", 0x40004), ("pts1", 0x50004), ("pts2", 0x60008), ("offsets", 0x70004), ("ws", 0x80002)):
        assert points(**{name: ctypes.c_void_p(addr), "total_px": 48}) == E_ARG, name
    assert points(total_px=1 << 31) == E_LIMIT and points(total_px=48, B=65536, total_tiles=48) == E_LIMIT
    assert points(total_px=1 << 31, ws=null) == E_ARG and points(total_px=1 << 31, B=0) == E_ARG    # a bad argument before the limit


# ---------------------------------------------------------------- Python-level refusals

def test_flow_points_ragged_refusals():
    sizes, sizesA = [(2, 3), (3, 2)], [(640, 480), (320, 240)]
    f, m = torch.zeros(12, 2), torch.ones(12, dtype=torch.bool)
    fl, ml = [f[:6].view(2, 3, 2), f[6:].view(3, 2, 2)], [m[:6].view(2, 3), m[6:].view(3, 2)]
    for op in (ops.flow_points_ragged, ops.matches_from_flow_ragged):
        for flow, keep in ((f, m), (fl, ml), (fl, m)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):          # everything fits: the device is what is wrong
                op(flow, keep, sizes, sizesA, [0, 90])
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                op(flow, keep, sizes, sizesA, 180, bg=keep)
        for bad in (dict(sizes=sizes[:1]), dict(sizesA=sizesA[:1]), dict(angles=[0]), dict(angles=[0, 45]), dict(sizesA=[(0, 1), (1, 1)]),
                    dict(sizes=[(2, 3), (0, 2)]), dict(sizes=[(2, 3), (-3, -2)])):
            with pytest.raises(ValueError):
                op(f, m, **dict(dict(sizes=sizes, sizesA=sizesA, angles=[0, 0]), **bad))
        with pytest.raises(ValueError):                                         # a packed buffer of another batch
            op(f[:11], m, sizes, sizesA, 0)
        with pytest.raises(ValueError):
            op(f, m, sizes, sizesA, 0, bg=m[:11])
        with pytest.raises(ValueError):                                         # a list of B - 1 maps, a map of another pair's shape
            op(fl[:1], ml, sizes, sizesA, 0)
        with pytest.raises(ValueError):
            op(fl, ml[::-1], sizes, sizesA, 0)


class _Rec:
    """What yfcc_matches_records reads of records before it touches a device."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_yfcc_matches_records_refusals():
    R = ops.MultiHRecordsRagged([3, 4], [4, 3], torch.device("cpu"), max_h=2)
    assert R.candidate is R.candidate_dev is R.size_src is R.size_tgt is R.bg is R.angle is None
    with pytest.raises(ValueError, match="sizesA"):
        assemble.yfcc_matches_records(R, 0.5, True)
    with pytest.raises(ValueError, match="angles"):
        assemble.yfcc_matches_records(R, 0.5, True, sizesA=[(640, 480)] * 2)
    with pytest.raises(ValueError, match="sizesB"):
        assemble.yfcc_matches_records(R, 0.5, True, sizesA=[(640, 480)] * 2, angles=[0, 90])
    R.size_src, R.size_tgt, R.angle = [(320, 240), (320, 256)], [(32, 24), (24, 32)], [0, 90]
    with pytest.raises(ValueError, match="multiples of 90"):
        assemble.yfcc_matches_records(R, 0.5, True, angles=[0, 30])
    with pytest.raises(ValueError):
        assemble.yfcc_matches_records(R, 0.5, True, sizesA=[(320, 240)])
    with pytest.raises(ValueError, match="does not fit"):                       # pair 1's map is 32 x 24: at 90 degrees sizeB = (32, 24)
        assemble.yfcc_matches_records(R, 0.5, True, sizesB=[(32, 24), (24, 32)])
    with pytest.raises(ValueError, match="sizesB"):
        assemble.yfcc_matches_records(R, 0.5, True, sizesB=[(32, 24)])
    with pytest.raises(ValueError, match="bg"):
        assemble.yfcc_matches_records(R, 0.5, True, bg="none")
    # rows() slices what the search left on the records
    R.candidate, R.bg = [0, 1], torch.arange(2 * 768, dtype=torch.int64).to(torch.uint8)
    r = R.rows(1, 2)
    assert r.candidate == [1] and r.size_src == [(320, 256)] and r.size_tgt == [(24, 32)] and r.angle == [90] and r.candidate_dev is None
    assert r.bg.numel() == 768 and r.bg.data_ptr() == R.bg.data_ptr() + 768 and R.rows(0, 2).bg.numel() == 1536


def test_want_records_refusals_on_a_bare_pipeline():
    pipe = _bare_pipe()
    u8 = lambda h, w: torch.zeros((h, w, 3), dtype=torch.uint8)
    src = [u8(240, 320), u8(256, 320)]
    cands = [[u8(240, 320), u8(256, 304)], [u8(320, 240), u8(304, 256)]]
    with pytest.raises(ValueError, match=r"records="):                           # stacked tensors fill the records handed in
        pipe.multi_h_variant_c(torch.stack([src[0]] * 2), [torch.stack([cands[0][0]] * 2)], want_records=True)
    with pytest.raises(ValueError, match="records"):                            # unchanged: no records= on a mixed-size list
        pipe.multi_h_variant_c(src, cands, records=object())
    with pytest.raises(ValueError, match="records"):
        pipe.multi_h_variant_c(src, cands, records=object(), want_records=True)
    with pytest.raises(ValueError, match="want_lists"):                         # unchanged: nothing would come back
        pipe.multi_h_variant_c(src, cands, want_lists=False)
    # want_records passes both gates -- with and without the lists, same sizes included -- and stops at the device check
    same = [u8(240, 320)] * 2
    for s, c, kw in ((src, cands, {}), (src, cands, dict(want_lists=False)), (same, [same, same], {}), (same, [same], dict(want_lists=False))):
        with pytest.raises(ValueError, match="HIP device"):
            pipe.multi_h_variant_c(s, c, want_records=True, **kw)
    # the PIL entry hands lists on, also for pairs of one size, and sets the angles on what comes back
    seen = []

    def fake(s, c, **kw):
        seen.append((s, c, kw))
        return ["outs"], _Rec(candidate=[1, 0], angle=None)
    pipe.multi_h_variant_c = fake
    pairs = [(_img(40, 24, 0), _img(32, 24, 1)), (_img(40, 24, 2), _img(32, 24, 3))]
    outs, rec = pipe.multi_h_variant_c_pairs(pairs, angles=(0, 270), want_records=True)
    s, c, kw = seen.pop()
    assert isinstance(s, list) and all(isinstance(x, list) for x in c) and kw["want_records"] is True
    assert outs == ["outs"] and rec.angle == [270, 0]


# ---------------------------------------------------------------- yfcc_norm_kp

def _norm_kp_script(org_size, new_size, K, kp):
    """The arithmetic of evaluation/evalYFCC/getResults.py:29-50 in its order, one axis after the other: half of (size - 1); plus
    K's principal point; the focal length from K's diagonal; both times (new size / size) -- the quotient formed first --; then
    (kp - centres) / focals on (1,2) float64 rows."""
    centre, focal = [], []
    for axis in (0, 1):
        c = (org_size[axis] - 1.0) * 0.5
        c += K[axis, 2]
        f = K[axis, axis]
        c *= (new_size[axis] / org_size[axis])
        f *= (new_size[axis] / org_size[axis])
        centre.append(c), focal.append(f)
    return (kp - np.array([centre])) / np.array([focal])


def _norm_kp_cases():
    for seed in range(8):
        rng = np.random.RandomState(300 + seed)
        org = (int(rng.randint(200, 3000)), int(rng.randint(200, 3000)))
        new = (int(rng.randint(10, 60)) * 16, int(rng.randint(10, 60)) * 16)
        K = np.array([[rng.uniform(300, 3000), 0, rng.uniform(-40, 40)], [0, rng.uniform(300, 3000), rng.uniform(-40, 40)], [0, 0, 1]])
        n = (0, 1, 7, 500)[seed % 4]
        kp = (rng.rand(n, 2) * new).astype(np.float32) if seed % 2 else rng.randint(0, min(new), size=(n, 2)).astype(np.int64)
        yield org, new, K, kp


def test_norm_kp_equals_the_scripts_arithmetic():
    for org, new, K, kp in _norm_kp_cases():
        got, want = assemble.yfcc_norm_kp(org, new, K, kp), _norm_kp_script(org, new, K.copy(), kp)
        assert got.dtype == want.dtype == np.float64 and got.shape == kp.shape
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    org, new, K, kp = next(_norm_kp_cases())
    again = K.copy()
    assemble.yfcc_norm_kp(org, new, again, kp)
    assert np.array_equal(again, K)                                             # K is read, not scaled in place


@pytest.mark.reference
def test_norm_kp_equals_the_live_reference():
    """The reference's own norm_kp, reached like matches_from_flow in tests/test_points_cpu.py: the script's module imports cv2 and
    h5py, so only the named function is compiled from where it lies."""
    import ref_loader
    if ref_loader.staged():
        pytest.skip("the YFCC results script is not part of the staged reference")
    fn = ref_loader.script_functions("evaluation/evalYFCC/getResults.py", ["norm_kp"])["norm_kp"]
    for org, new, K, kp in _norm_kp_cases():
        want = fn(org, new, K.copy(), kp)
        got = assemble.yfcc_norm_kp(org, new, K, kp)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.int64), want.view(np.int64))


def test_ragged_points_kernels_need_no_scratch_and_a_few_words_of_lds():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {r["kernel"]: r for r in kr.table(_lib.LIB_PATH) if r["unit"] == "points_ragged"}
    assert set(rows) == {"points_ragged_count_kernel", "points_ragged_scan_kernel", "points_ragged_scatter_kernel"}
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["waves_per_simd"] == 8, r
    # the tallies only, as in the one-size kernels: one int32 per wavefront (count, scan), two per wavefront (the scatter's double buffer)
    assert {k: (r["lds"], r["wg"]) for k, r in rows.items()} == {"points_ragged_count_kernel": (16, 256), "points_ragged_scan_kernel": (64, 1024),
                                                                 "points_ragged_scatter_kernel": (32, 256)}
