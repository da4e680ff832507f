"""Host side of the Corr results step of a batch of device records (csrc/keypoints.hip; ops.records_keypoints / pck_tally;
assemble.corr_keypoints_records / corr_precision / corr_resize_keypoints; the drop-in's corr namespace).

The yardstick first: the tally rule the kernel is held to, stated in numpy in this file's own words (rule_tally, shared with
tests/test_gpu_corr_records.py), equals what the reference's own alignmentError under the masks of evaluation/evalCorr/getResults.py
:281-282 returned for tests/golden/corr_records.npz.  Then the surface: the keypoint table as a pure function, the refusals, header
and binding, the resize rule, the precision table, the static resources of the two kernels.  Nothing is launched."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from rfx import assemble, ops, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---------------------------------------------------------------- the rule

def rule_tally(xa, ya, m, flag, xs, ys, koff, ths, grid, valid=None):
    """xa, ya, m float32 and flag uint8 of K_total keypoints, xs / ys integer source keypoints, koff (B+1,) -> (counts (M,B,T) int64,
    nb (M,B) int64, dist (M,K_total) float64, NaN where a keypoint is not kept).  A threshold above 0 keeps m >= t (both float32)
    with bit 1 of the flag set; a threshold of 0 or below keeps everything.  The distance is numpy float64 from the float32
    estimates on, as the reference's expression promotes.  A pair with valid 0: nb = its keypoints, nothing measured."""
    ths, grid = np.asarray(ths, np.float32), np.asarray(grid, np.float64)
    B, K = len(koff) - 1, koff[-1]
    counts, nb = np.zeros((len(ths), B, len(grid)), np.int64), np.zeros((len(ths), B), np.int64)
    dist = np.full((len(ths), K), np.nan)
    for t, th in enumerate(ths):
        keep = (m >= th) & ((flag & 2) != 0) if th > 0 else np.ones(K, bool)
        with np.errstate(invalid="ignore"):
            d = ((xa.astype(np.float64) - xs) ** 2 + (ya.astype(np.float64) - ys) ** 2) ** 0.5
        for b in range(B):
            lo, hi = koff[b], koff[b + 1]
            if valid is not None and not valid[b]:
                nb[t, b] = hi - lo
                continue
            k = keep[lo:hi]
            dist[t, lo:hi][k] = d[lo:hi][k]
            nb[t, b] = k.sum()
            with np.errstate(invalid="ignore"):
                counts[t, b] = (d[lo:hi][k][:, None] <= grid).sum(axis=0)
    return counts, nb, dist


_gold = {}


def golden():
    """tests/golden/corr_records.npz, decoded once."""
    if not _gold:
        g = np.load(os.path.join(GOLD, "corr_records.npz"))
        B = len(g["h8"])
        _gold.update(raw=g, B=B, sizes8=[(int(a), int(b)) for a, b in zip(g["h8"], g["w8"])], nbH=[int(n) for n in g["nbH"]],
                     sizeA=[tuple(int(v) for v in s) for s in g["sizeA"]], ths=[float(t) for t in g["ths"]], grid=g["grid"],
                     kp=[tuple(g["p%d_%s" % (b, k)] for k in ("XA", "YA", "XB", "YB")) for b in range(B)])
    return _gold


def test_rule_equals_the_reference_outputs_in_the_golden_file():
    G = golden()
    g = G["raw"]
    assert G["sizes8"] == [(3, 4), (5, 4), (6, 8)] and G["nbH"] == [1, 3, 0] and G["ths"] == [0.0, 0.5, 0.9]
    assert np.array_equal(G["grid"], [1, 2, 3, 5, 8, 13, 22, 36]) and np.array_equal(G["grid"], ops.pck_pixel_grid())
    K = [len(k[0]) for k in G["kp"]]
    koff = [0] + list(np.cumsum(K))
    cat = lambda key, fill: np.concatenate([g["p%d_%s" % (b, key)] if G["nbH"][b] else np.full(K[b], fill, np.float32) for b in range(3)])
    xa, ya, m = cat("xa", 0), cat("ya", 0), cat("m", 0)
    flag = np.full(koff[-1], 3, np.uint8)                          # the golden flows are finite
    xs = np.concatenate([k[0] for k in G["kp"]]).astype(np.int64)
    ys = np.concatenate([k[1] for k in G["kp"]]).astype(np.int64)
    counts, nb, dist = rule_tally(xa, ya, m, flag, xs, ys, koff, G["ths"], G["grid"], valid=[n >= 1 for n in G["nbH"]])
    assert np.array_equal(counts, g["counts"]) and np.array_equal(nb, g["nbAlign"])
    assert nb[:, 2].tolist() == [60, 60, 60] and not counts[:, 2].any()              # the pair without files
    assert nb[0, 0] == 60 and 0 < nb[2, 0] < nb[1, 0] <= 60 and 0 < counts[2, 1, 2] < counts[2, 1, -1]
    assert np.isnan(dist[:, koff[2]:]).all() and not np.isnan(dist[0, :koff[2]]).any()
    # the precision table of the script's last lines, from the same tallies
    prec, tot = assemble.corr_precision(torch.from_numpy(counts), torch.from_numpy(nb))
    assert np.array_equal(tot, g["nbAlign"].sum(axis=1)) and np.array_equal(prec, g["counts"].sum(axis=1) / g["nbAlign"].sum(axis=1)[:, None])


def test_rule_details():
    """Pieces of the rule on cases small enough to read."""
    one = lambda v, dt: np.asarray(v, dt)
    # 3-4-5 lands on 5 and 5-12-13 on 13: <= counts them, < would not
    xa, ya = one([13, 15], np.float32), one([24, 32], np.float32)
    c, nb, d = rule_tally(xa, ya, one([1, 1], np.float32), one([3, 3], np.uint8), one([10, 10], np.int64), one([20, 20], np.int64),
                          [0, 2], [0.0], [4, 5, 12, 13])
    assert d.tolist() == [[5.0, 13.0]] and c.tolist() == [[[0, 1, 1, 2]]] and nb.tolist() == [[2]]
    # m exactly on the threshold is kept; bit 1 clear drops a keypoint only above 0; a NaN is kept at 0 and counts under no threshold
    m = one([0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.9, 0.7], np.float32)
    flag = one([3, 3, 1, 2], np.uint8)
    xa = one([1, 1, np.nan, 1], np.float32)
    c, nb, d = rule_tally(xa, xa, m, flag, np.ones(4, np.int64), np.ones(4, np.int64), [0, 4], [0.0, 0.5, -1.0], [0.0, 1.0])
    assert nb.tolist() == [[4], [2], [4]] and c.tolist() == [[[3, 3]], [[2, 2]], [[3, 3]]]
    assert np.isnan(d[0, 2]) and np.isnan(d[1, 1:3]).all() and d[1, 0] == 0 and d[1, 3] == 0
    # valid = 0: every keypoint counts, none is measured
    c, nb, d = rule_tally(xa, xa, m, flag, np.ones(4, np.int64), np.ones(4, np.int64), [0, 1, 4], [0.0], [1.0], valid=[True, False])
    assert nb.tolist() == [[1, 3]] and c.tolist() == [[[1], [0]]] and np.isnan(d[0, 1:]).all()
    # float64 from the float32 estimate on: not the float32 difference
    x = np.float32(1234.5678)
    assert rule_tally(one([x], np.float32), one([0], np.float32), one([1], np.float32), one([3], np.uint8), one([1000], np.int64),
                      one([0], np.int64), [0, 1], [0.0], [1.0])[2][0, 0] == float(x) - 1000.0


# ---------------------------------------------------------------- the surface

def _records(ragged=True, size_src=None, **kw):
    R = ops.MultiHRecordsRagged([3, 5, 6], [4, 4, 8], "cpu", max_h=4, **kw) if ragged else ops.MultiHRecords(3, 3, 4, "cpu", max_h=4, **kw)
    R.size_src = size_src
    return R


def test_keypoint_table_is_a_pure_function_of_sizes_and_keypoints():
    R = _records(size_src=[(301, 200), (97, 211), (640, 480)])
    xb = [np.asarray([0.0, 31.99, 5.5]), [], np.asarray([63, 1], np.int64)]
    yb = [np.asarray([23.9, 0.2, 7.0]), np.zeros(0, np.float32), [47, 2]]
    rows, total, krows, x, y, koff = ops.records_keypoints_table(R, xb, yb)
    assert (rows, total) == ops.assemble_records_table(R)[::2] and total == 24 * 32 + 40 * 32 + 48 * 64
    assert krows == [(0, 3, 301, 200), (3, 0, 97, 211), (3, 2, 640, 480)] and koff == [0, 3, 3, 5]
    assert x.dtype == y.dtype == np.int32 and x.tolist() == [0, 31, 5, 63, 1] and y.tolist() == [23, 0, 7, 47, 2]
    # truncation toward zero, like astype(np.int64): -0.7 is pixel 0, 31.99 is pixel 31 (rounding would leave the 32-wide map)
    assert ops.records_keypoints_table(R, [[-0.7], [], []], [[-0.2], [], []])[3].tolist() == [0]
    # an empty pair first / last, explicit sizesA and out_hw
    r2 = ops.records_keypoints_table(R, [[], [1], []], [[], [2], []], sizesA=[(5, 6), (7, 8), (9, 10)], out_hw=[(10, 11), (12, 13), (1, 9)])
    assert r2[2] == [(0, 0, 5, 6), (0, 1, 7, 8), (1, 0, 9, 10)] and r2[5] == [0, 0, 1, 1] and r2[1] == 110 + 156 + 9
    # dense records, and a rows() slice of ragged ones
    D = _records(ragged=False)
    assert ops.records_keypoints_table(D, [[1]] * 3, [[2]] * 3, sizesA=[(4, 4)] * 3)[2] == [(0, 1, 4, 4), (1, 1, 4, 4), (2, 1, 4, 4)]
    S = R.rows(1, 3)
    rows, total, krows, *_ = ops.records_keypoints_table(S, [[31], [63]], [[39], [47]])
    assert krows == [(0, 1, 97, 211), (1, 1, 640, 480)] and total == 40 * 32 + 48 * 64 and [r[4:6] for r in rows] == [(40, 32), (48, 64)]


def test_refusals_answer_on_the_host():
    R = _records(size_src=[(301, 200), (97, 211), (640, 480)])
    ok = [[1], [1], [1]]
    with pytest.raises(ValueError, match="per pair"):
        ops.records_keypoints_table(R, ok[:2], ok)
    with pytest.raises(ValueError, match="per pair"):
        ops.records_keypoints_table(R, ok, ok, sizesA=[(1, 1)] * 2)
    with pytest.raises(ValueError, match="xb for"):
        ops.records_keypoints_table(R, [[1, 2], [1], [1]], ok)
    for xb, yb in (([[32], [1], [1]], ok), (ok, [[1], [40], [1]]), ([[1], [1], [-1]], ok), (ok, [[1], [1], [48.0]])):
        with pytest.raises(_lib.RfxError, match="outside"):
            ops.records_keypoints_table(R, xb, yb)
    with pytest.raises(_lib.RfxError):
        ops.records_keypoints_table(R, ok, ok, sizesA=[(0, 5), (5, 5), (5, 5)])
    with pytest.raises(ValueError, match="size_src"):
        ops.records_keypoints_table(_records(), ok, ok)
    with pytest.raises(ValueError, match="size_src"):
        assemble.corr_keypoints_records(_records(), 0.5, True, ok, ok, ok, ok)
    for kitti in (_records(hd2_list=[2, 3, 3], wd2_list=[2, 2, 4]), _records(ragged=False, hd2=2, wd2=2)):
        with pytest.raises(ValueError, match="flowD2"):
            ops.records_keypoints_table(kitti, ok, ok, sizesA=[(5, 5)] * 3)
    with pytest.raises(TypeError):
        ops.records_keypoints_table(object(), ok, ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # everything on the host fits: the device is what is wrong
        ops.records_keypoints(R, 0.5, True, True, ok, ok)
    z = lambda dt: torch.zeros(3, dtype=dt)
    args = (z(torch.float32), z(torch.float32), z(torch.float32), z(torch.uint8), ok, ok, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="1 to 16"):                # T > 16
        ops.pck_tally(*args, pixel_grid=np.arange(17))
    with pytest.raises(ValueError, match="1 to 16"):
        ops.pck_tally(*args, match_ths=())
    with pytest.raises(ValueError, match="per pair"):
        ops.pck_tally(*args[:4], ok[:2], ok, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="keypoints, got"):
        ops.pck_tally(*args[:4], [[1, 2], [1], [1]], ok, [0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pck_tally(*args)
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    assert getResults.corr.keypoints_records is assemble.corr_keypoints_records and getResults.corr.precision is assemble.corr_precision
    assert getResults.corr.alignmentError is assemble.corr_alignment_error


NAMES = ("rfx_records_keypoints_f32", "rfx_pck_tally_f64")


def test_header_and_binding_declare_the_entry_points():
    C = ctypes
    text = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert int(re.search(r"#define RFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 17
    kinds = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float}
    for name in NAMES:
        ret, args = re.search(r"\b(int|size_t)\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S).groups()
        res, argtypes = _lib.SIGNATURES[name]
        assert ret == "int" and res is C.c_int
        params = [" ".join(p.split()) for p in args.split(",")]
        assert [C.c_void_p if "*" in p else kinds[p.rsplit(" ", 1)[0]] for p in params] == argtypes, (name, params)
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 22 and len(_lib.SIGNATURES[NAMES[1]][1]) == 18
    # each entry's comment cites the reference lines it replaces
    assert "evaluation/evalCorr/getResults.py:78-136" in text and "evaluation/evalCorr/getResults.py:281-282" in text
    lib = _lib.load()
    assert lib.rfx_abi_version() == 17


def test_argument_checks_answer_before_any_device_call():
    """Every call below carries at least one defect and returns from the entry point's opening checks; the (fake, aligned) pointers
    are never followed."""
    lib = _lib.load()
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(13)]
    null = ctypes.c_void_p(0)
    E_ARG, E_LIMIT = -1, -2

    def kp(rec=P[0], rec_elems=3000, width=1000, max_h=4, off_H=4, off_flow=40, table=P[1], B=3, total_px=5000, bg=P[2], ktable=P[3],
           xb=P[4], yb=P[5], K=10, xa=P[6], ya=P[7], m=P[8], flag=P[9]):
        return lib.rfx_records_keypoints_f32(rec, rec_elems, width, max_h, off_H, off_flow, table, B, total_px, 0.5, 1, 1, bg, ktable,
                                             xb, yb, K, xa, ya, m, flag, null)
    for name in ("rec", "table", "ktable", "xb", "yb", "xa", "ya", "m", "flag"):
        assert kp(**{name: null}) == E_ARG, name
        assert kp(**{name: null, "bg": null}) == E_ARG, name        # bg is optional, the others are not
    for bad in (dict(B=0), dict(K=0), dict(K=-1), dict(width=0), dict(max_h=0), dict(off_H=0), dict(off_flow=39), dict(off_flow=1001),
                dict(rec_elems=2999), dict(total_px=0), dict(table=ctypes.c_void_p(0x20004)), dict(ktable=ctypes.c_void_p(0x40004))):
        assert kp(**bad) == E_ARG, bad
    assert kp(B=65536, rec_elems=65536000) == E_LIMIT and kp(total_px=1 << 31) == E_LIMIT and kp(K=1 << 31) == E_LIMIT
    assert kp(K=1 << 31, xb=null) == E_ARG                          # a bad argument is named before the limit

    def tally(xa=P[0], ya=P[1], m=P[2], flag=P[3], xs=P[4], ys=P[5], ktable=P[6], B=3, K=10, ths=P[7], M=2, grid=P[8], T=8, valid=P[9],
              counts=P[10], nb=P[11], dist=P[12]):
        return lib.rfx_pck_tally_f64(xa, ya, m, flag, xs, ys, ktable, B, K, ths, M, grid, T, valid, counts, nb, dist, null)
    for name in ("xa", "ya", "m", "flag", "xs", "ys", "ktable", "ths", "grid", "counts", "nb"):
        assert tally(**{name: null}) == E_ARG, name
        assert tally(**{name: null, "valid": null, "dist": null}) == E_ARG, name
    for bad in (dict(B=0), dict(M=0), dict(T=0), dict(T=17), dict(K=-1), dict(grid=ctypes.c_void_p(0x90004)),
                dict(counts=ctypes.c_void_p(0xb0004)), dict(nb=ctypes.c_void_p(0xc0004)), dict(dist=ctypes.c_void_p(0xd0004)),
                dict(ktable=ctypes.c_void_p(0x70004))):
        assert tally(**bad) == E_ARG, bad
    assert tally(B=65536) == E_LIMIT and tally(K=1 << 31) == E_LIMIT and tally(K=1 << 31, T=17) == E_ARG


def test_resize_keypoints_equals_the_golden():
    g = golden()["raw"]
    for i, ((w, h), ms) in enumerate(zip(g["rs_sizes"], g["rs_min"])):
        new, x, y, valid = assemble.corr_resize_keypoints(int(ms), (int(w), int(h)), g["rs_x"][i], g["rs_y"][i], megadepth=True)
        assert new == tuple(int(v) for v in g["rs_new"][i]) and new[0] % 16 == 0 and new[1] % 16 == 0, (w, h)
        assert x.dtype == y.dtype == np.float32 and valid.dtype == bool
        assert np.array_equal(x.view(np.int32), g["rs_outx"][i].view(np.int32)) and np.array_equal(y.view(np.int32), g["rs_outy"][i].view(np.int32))
        assert np.array_equal(valid, g["rs_valid"][i]) and 0 < valid.sum() < len(valid)
        sx = ";".join(repr(float(v)) for v in g["rs_x"][i])          # the CSV's strings
        sy = ";".join(repr(float(v)) for v in g["rs_y"][i])
        new2, x2, y2 = assemble.corr_resize_keypoints(int(ms), (int(w), int(h)), sx, sy)
        assert new2 == new and np.array_equal(x2, x) and np.array_equal(y2, y)
    assert assemble.corr_resize_keypoints(480, (1024, 768), [1.0], [1.0], strideNet=32)[0] == (640, 480)


@pytest.mark.reference
def test_resize_keypoints_equals_the_live_reference():
    import ref_loader
    from PIL import Image
    if not ref_loader.available():
        pytest.skip("the reference's source tree is not present")
    if ref_loader.staged():
        pytest.skip("the Corr results script's resize functions are not part of the staged reference")
    f = ref_loader.script_functions("evaluation/evalCorr/getResults.py", ["ResizeMinResolution", "ResizeMinResolution_megadepth"])
    f["ResizeMinResolution"].__globals__["Image"] = Image           # the script's own import
    rng = np.random.RandomState(3)
    for _ in range(20):
        w, h, ms, stride = int(rng.randint(200, 3000)), int(rng.randint(200, 3000)), int(rng.choice([240, 480, 512])), int(rng.choice([8, 16]))
        x, y = rng.rand(9) * (w + 10) - 5, rng.rand(9) * (h + 10) - 5
        sx, sy = ";".join(repr(float(v)) for v in x), ";".join(repr(float(v)) for v in y)
        I, rx, ry, rv = f["ResizeMinResolution_megadepth"](ms, Image.new("L", (w, h)), sx, sy, stride)
        new, gx, gy, gv = assemble.corr_resize_keypoints(ms, (w, h), sx, sy, strideNet=stride, megadepth=True)
        assert new == I.size and gx.dtype == rx.dtype and np.array_equal(gx, rx) and np.array_equal(gy, ry) and np.array_equal(gv, rv)
        assert f["ResizeMinResolution"](ms, Image.new("L", (w, h)), sx, sy, stride)[0].size == new


def test_precision_on_a_hand_table():
    counts = torch.tensor([[[1, 2, 4], [3, 4, 4]], [[0, 0, 1], [0, 1, 1]]])       # (M=2, B=2, T=3)
    nb = torch.tensor([[4, 4], [1, 3]])
    prec, tot = assemble.corr_precision(counts, nb)
    assert prec.dtype == np.float64 and tot.tolist() == [8, 4]
    assert np.array_equal(prec, np.asarray([[4, 6, 8], [0, 1, 2]]) / np.asarray([[8.0], [4.0]]))
    prec, tot = assemble.corr_precision(np.zeros((1, 2, 2), np.int64), np.zeros((1, 2), np.int64))
    assert np.isnan(prec).all() and tot.tolist() == [0]             # the script's 0 / 0


def test_keypoint_kernels_need_no_scratch_and_a_few_words_of_lds():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {r["kernel"]: r for r in kr.table(_lib.LIB_PATH) if r["unit"] == "keypoints"}
    assert set(rows) == {"records_keypoints_kernel", "pck_tally_kernel"}
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["wg"] == 256, r
    # no LDS in the keypoint transfer; the tally's one pass: 17 int32 per wavefront
    assert rows["records_keypoints_kernel"]["lds"] == 0 and rows["pck_tally_kernel"]["lds"] == 4 * 17 * 4
    mk = open(os.path.join(ROOT, "ransac-flow_amd", "csrc", "Makefile")).read()
    assert re.search(r"^EXTRA_keypoints\s*=.*-ffp-contract=off", mk, flags=re.M) and " keypoints.hip " in mk
