"""Host side of the aligned source images of a batch (csrc/warp_image.hip; ops.warp_records_u8 / warp_flow_u8 / warp_image_table;
assemble.aligned_images_records / aligned_image; AlignPipeline.align_pairs(want_u8=True)).

The yardstick first: the per-pixel rule the kernels are held to, stated in numpy in this file's own words (rule_warp_u8 /
rule_overlay, shared with tests/test_gpu_warp_image.py), against what the reference's own functions returned for
tests/golden/warp_image.npz.  Then the surface: the image table as a pure function, the refusals, header and binding, the entry
points' opening checks, the static resources of the two kernels.  Nothing is launched."""
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
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- the rule

def fma_f32(a, b, c):
    """round_to_float32(a * b + c) for float32 arrays, rounded ONCE: a * b is exact in float64; where the float64 sum with c is not,
    its error term (two-sum) says on which side the true value lies and the sum is made odd in its last bit before the rounding to
    float32 (round to odd), so that no float32 tie is decided by the first rounding."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p, c = a.astype(f64) * b.astype(f64), c.astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def rule_corners(g, size):
    """One axis of the bilinear sample (align_corners = False) in float32 steps: the un-normalised coordinate ((g + 1) * size - 1) / 2
    with the product and the subtraction fused, its floor, the weights of the floor and of its neighbour, and whether either lies in
    the image.  A NaN, an infinity or a huge value lies nowhere."""
    g = np.asarray(g, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        i = fma_f32(g + f32(1), f32(size), f32(-1)) * f32(0.5)
        lo = np.floor(i)
        hi_w = i - lo
        lo_w = f32(1) - hi_w
        in0 = (lo >= 0) & (lo <= size - 1)
        in1 = (lo + f32(1) >= 0) & (lo + f32(1) <= size - 1)
    base = np.where(in0 | in1, lo, 0).astype(np.int64)
    return base, lo_w.astype(f32), hi_w.astype(f32), in0, in1


def rule_warp_u8(flow, src):
    """flow (H,W,2) float32 normalised sampling points, src (Hs,Ws,3) uint8 -> (H,W,3) uint8: per channel v = 0, then for the corners
    nw, ne, sw, se that lie in the source v = fma(byte / 255, weight, v); the result is trunc(clamp(v, 0, 1) * 255), the product
    rounded to float32."""
    Hs, Ws = src.shape[:2]
    x0, ex, wx, xin0, xin1 = rule_corners(flow[..., 0], Ws)
    y0, sy, ny, yin0, yin1 = rule_corners(flow[..., 1], Hs)
    t = src.astype(f32) / f32(255)
    v = np.zeros(flow.shape[:2] + (3,), f32)
    with np.errstate(invalid="ignore"):
        for dy, dx, w, m in ((0, 0, sy * ex, yin0 & xin0), (0, 1, sy * wx, yin0 & xin1), (1, 0, ny * ex, yin1 & xin0), (1, 1, ny * wx, yin1 & xin1)):
            yy, xx = np.clip(y0 + dy, 0, Hs - 1), np.clip(x0 + dx, 0, Ws - 1)
            w = np.where(m, w, f32(0)).astype(f32)               # a corner outside is never read: its (possibly NaN) weight is not used
            v = np.where(m[..., None], fma_f32(t[yy, xx], w[..., None], v), v)
    return (np.clip(v, f32(0), f32(1)) * f32(255)).astype(np.uint8)


def rule_overlay(img, tgt):
    """The 50 % overlay as the reference forms it: float64 a * 0.5 + b * 0.5, truncated."""
    return (img.astype(f64) * 0.5 + tgt.astype(f64) * 0.5).astype(np.uint8)


_gold = {}


def golden():
    if not _gold:
        _gold["g"] = np.load(os.path.join(GOLD, "warp_image.npz"))
    return _gold["g"]


CASES = ["%s_%s" % (k, t) for k in ("hpatch", "corr") for t in "abc"]


def test_rule_equals_the_reference_outputs_in_the_golden_file():
    """Where the flow is the golden's, the rule gives the reference's bytes exactly -- both sources, all six flows -- and the integer
    overlay (a + b) >> 1 is the reference's float64 average, truncated."""
    g = golden()
    assert g["src0"].shape == (20, 28, 3) and g["src1"].shape == (31, 17, 3) and g["tgt"].shape == (24, 32, 3)
    assert os.path.getsize(os.path.join(GOLD, "warp_image.npz")) < 200 * 1024
    seen = set()
    for k in CASES:
        flow = g[k + "_flow"]
        assert flow.shape == (24, 32, 2) and flow.dtype == np.float32
        for s in range(2):
            img = rule_warp_u8(flow, g["src%d" % s])
            want = g["%s_img%d" % (k, s)]
            assert np.array_equal(img, want), (k, s, int((img != want).sum()))
            avg = g["%s_avg%d" % (k, s)]
            assert np.array_equal(rule_overlay(want, g["tgt"]), avg), (k, s)
            assert np.array_equal(((want.astype(np.int32) + g["tgt"]) >> 1).astype(np.uint8), avg), (k, s)
            seen.update(np.unique(want).tolist())
    assert len(seen) == 256                                         # every level occurs in the reference's images
    # the multi-homography settings differ from the single-homography ones
    assert not np.array_equal(g["hpatch_a_img0"], g["hpatch_b_img0"]) and not np.array_equal(g["corr_a_img1"], g["corr_b_img1"])


def test_exact_families_of_the_rule():
    lv = np.arange(256, dtype=np.uint8)
    t = lv.astype(f32) / f32(255)
    assert np.array_equal((t * f32(255)).astype(np.uint8), lv)    # trunc((x / 255) * 255) == x for every level
    rng = np.random.RandomState(7)
    a, b = rng.randint(0, 256, 100000), rng.randint(0, 256, 100000)
    half = f32(0.5)
    for first, second in ((a, b), (b, a)):                         # half-weight blends, either corner first
        v = fma_f32(t[second], half, fma_f32(t[first], half, f32(0)))
        assert np.array_equal((np.clip(v, 0, 1) * f32(255)).astype(np.int64), (a + b) >> 1)
    # all 256 x 256 overlays: the shift is the float64 average, truncated
    A, B = np.meshgrid(lv, lv, indexing="ij")
    assert np.array_equal(rule_overlay(A, B), ((A.astype(np.int32) + B) >> 1).astype(np.uint8))
    # the rule on a sample that falls on integer source pixels reproduces the source; borders, NaN and far outside give 0
    src = (np.arange(2 * 3 * 3).reshape(2, 3, 3) * 14 + 3).astype(np.uint8)
    gx = (2.0 * np.arange(3) + 1.0) / 3 - 1.0
    gy = (2.0 * np.arange(2) + 1.0) / 2 - 1.0
    flow = np.stack(np.meshgrid(gx, gy, indexing="xy"), axis=-1).astype(f32)
    assert np.array_equal(rule_warp_u8(flow, src), src)
    bad = np.asarray([[[np.nan, 0.0], [0.0, np.inf], [-4.0, 0.0], [3e9, -3e9]]], f32)
    assert not rule_warp_u8(bad, src).any()
    # one pixel left of the image's first column: only the two east corners lie inside, with weight 1/2 -> half the value
    edge = np.asarray([[[-1.0, gy[0]]]], f32)
    assert np.array_equal(rule_warp_u8(edge, src)[0, 0], src[0, 0] // 2)


# ---------------------------------------------------------------- the table

def _records(ragged=True, **kw):
    return ops.MultiHRecordsRagged([3, 5, 6], [4, 4, 8], "cpu", max_h=4, **kw) if ragged else ops.MultiHRecords(3, 3, 4, "cpu", max_h=4, **kw)


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_image_table_is_a_pure_function_of_the_images():
    sizes = [(24, 32), (40, 32), (48, 64)]
    srcs = [_u8(13, 17, 3), _u8(2, 3, 3), _u8(1, 1, 3)]
    rows, keep = ops.warp_image_table(sizes, srcs)
    assert rows == [(srcs[0].data_ptr(), 13, 17, 0), (srcs[1].data_ptr(), 2, 3, 0), (srcs[2].data_ptr(), 1, 1, 0)]
    assert len(keep) == 3 and all(a is b for a, b in zip(keep, srcs))
    tgts = [_u8(h, w, 3) for h, w in sizes]
    rows, keep = ops.warp_image_table(sizes, srcs, tgts, device="cpu")
    assert [r[3] for r in rows] == [t.data_ptr() for t in tgts] and len(keep) == 6
    # a dense tensor: the pairs' addresses are one image apart
    S = _u8(3, 5, 7, 3)
    rows, keep = ops.warp_image_table([(8, 8)] * 3, S)
    assert rows == [(S.data_ptr() + b * 105, 5, 7, 0) for b in range(3)]
    assert all(k.untyped_storage().data_ptr() == S.untyped_storage().data_ptr() for k in keep)
    # a tuple works like a list; the sizes of the records' table are what a target is held to
    R = _records()
    trows, max_hw, total = ops.assemble_records_table(R)
    assert [(r[4], r[5]) for r in trows] == sizes and [r[6] for r in trows] == [0, 768, 768 + 1280] and total == 768 + 1280 + 3072
    assert ops.warp_image_table([(r[4], r[5]) for r in trows], tuple(srcs), tuple(tgts))[0] == rows[:0] + \
        [(s.data_ptr(), s.shape[0], s.shape[1], t.data_ptr()) for s, t in zip(srcs, tgts)]
    # out_hw forms: one size for a dense batch, one per pair for a ragged one; the packed offsets follow
    trows, max_hw, total = ops.assemble_records_table(R, [(1, 1), (5, 7), (9, 11)])
    assert [r[6] for r in trows] == [0, 1, 36] and (max_hw, total) == (99, 135)
    D = _records(ragged=False)
    trows, max_hw, total = ops.assemble_records_table(D, (27, 30))
    assert [r[6] for r in trows] == [0, 810, 1620] and [r[0] for r in trows] == [0, D.width, 2 * D.width] and max_hw == 810
    # a rows() slice starts again at 0, over the same storage
    S2 = R.rows(1, 3)
    trows, _, total = ops.assemble_records_table(S2)
    assert [r[6] for r in trows] == [0, 1280] and total == 1280 + 3072 and S2.rec.data_ptr() == R.rec.data_ptr() + 4 * R.width


# ---------------------------------------------------------------- refusals

def test_refusals_answer_on_the_host():
    sizes = [(24, 32), (40, 32), (48, 64)]
    ok = [_u8(4, 5, 3) for _ in range(3)]
    tg = [_u8(h, w, 3) for h, w in sizes]
    T = ops.warp_image_table
    with pytest.raises(ValueError, match="per pair"):
        T(sizes, ok[:2])
    with pytest.raises(ValueError, match="per pair"):
        T(sizes, _u8(2, 4, 5, 3))
    with pytest.raises(ValueError, match="per pair"):
        T(sizes, [o.numpy() for o in ok])
    with pytest.raises(ValueError, match="uint8"):
        T(sizes, [ok[0], ok[1].float(), ok[2]])
    for bad in (_u8(4, 5, 4), _u8(4, 5), _u8(0, 5, 3), _u8(1, 4, 5, 3)):
        with pytest.raises(ValueError, match=r"\(H,W,3\)"):
            T(sizes, [ok[0], bad, ok[2]])
    with pytest.raises(ValueError, match="contiguous"):
        T(sizes, [ok[0], _u8(5, 4, 3).transpose(0, 1), ok[2]])
    with pytest.raises(ValueError, match="contiguous"):
        T(sizes, _u8(3, 4, 10, 3)[:, :, ::2])
    with pytest.raises(ValueError, match="output size"):
        T(sizes, ok, [tg[0], _u8(32, 40, 3), tg[2]])
    with pytest.raises(ValueError, match="uint8"):
        T(sizes, ok, [t.float() for t in tg])
    with pytest.raises(RuntimeError, match="runs on"):
        T(sizes, ok, device="cuda:0")
    R = _records()
    with pytest.raises(TypeError):
        ops.warp_records_u8(object(), ok, 0.5, True, True)
    for kitti in (_records(hd2_list=[2, 3, 3], wd2_list=[2, 2, 4]), _records(ragged=False, hd2=2, wd2=2)):
        with pytest.raises(ValueError, match="flowD2"):
            ops.warp_records_u8(kitti, ok, 0.5, True, True)
        with pytest.raises(ValueError, match="flowD2"):
            assemble.aligned_images_records(kitti, ok, 0.5, True, True)
    with pytest.raises(ValueError, match="out_hw"):
        ops.warp_records_u8(R, ok, 0.5, True, True, out_hw=(24, 32))
    with pytest.raises(ValueError, match="output size"):
        ops.warp_records_u8(R, ok, 0.5, True, True, out_hw=[(8, 8)] * 3, tgt=tg)
    with pytest.raises(ValueError, match="bg is"):
        ops.warp_records_u8(R, ok, 0.5, True, True, bg=torch.zeros(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or uint8"):
        ops.warp_records_u8(R, ok, 0.5, True, True, bg=[torch.zeros(s) for s in sizes])
    total = sum(h * w for h, w in sizes)
    for out in ((_u8(total, 3),), (_u8(total, 4), None, None), (_u8(total, 3).float(), None, None), (_u8(total, 3), None, None)):
        with pytest.raises(ValueError, match="out"):                # the last: a mask is wanted and none is given
            ops.warp_records_u8(R, ok, 0.5, True, True, want_mask=True, out=out)
    with pytest.raises(ValueError, match="out overlay"):
        ops.warp_records_u8(R, ok, 0.5, True, True, tgt=tg, out=(_u8(total, 3), _u8(total), None))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # everything on the host fits: the device is what is wrong
        ops.warp_records_u8(R, ok, 0.5, True, True, tgt=tg, want_mask=True, bg=[torch.ones(s, dtype=torch.bool) for s in sizes])
    # the flow form
    F = ops.warp_flow_u8
    flow = torch.zeros(2, 6, 7, 2)
    two = [_u8(4, 5, 3)] * 2
    for bad in (flow.double(), torch.zeros(2, 6, 7, 3), torch.zeros(6, 7), [torch.zeros(6, 7, 3)], [], flow.numpy()):
        with pytest.raises(ValueError, match="flow"):
            F(bad, two)
    with pytest.raises(ValueError, match="contiguous"):
        F(torch.zeros(2, 6, 2, 7).transpose(2, 3), two)
    with pytest.raises(ValueError, match="8-byte aligned"):
        F(torch.zeros(2 * 42 + 1)[1:].view(6, 7, 2), _u8(4, 5, 3))
    with pytest.raises(ValueError, match="per pair"):
        F(flow, ok)
    with pytest.raises(ValueError, match="output size"):
        F(flow, two, tgt=[_u8(7, 6, 3)] * 2)
    with pytest.raises(ValueError, match="binary has"):
        F(flow, two, binary=torch.zeros(2, 7, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or uint8"):
        F(flow, two, binary=torch.zeros(2, 6, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F(flow, two, tgt=[_u8(6, 7, 3)] * 2, binary=torch.zeros(2, 6, 7, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F([flow[0], flow[1]], two)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        assemble.aligned_image(flow[0], two[0])
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    assert getResults.corr.aligned_images_records is assemble.aligned_images_records is getResults.aligned_images_records
    assert getResults.corr.aligned_image is assemble.aligned_image is getResults.aligned_image
    assert getResults.corr.keypoints_records is assemble.corr_keypoints_records


def test_pipeline_wants_the_uint8_source_for_want_u8():
    from rfx.pipeline import AlignPipeline
    import inspect
    for fn in (AlignPipeline.align_pairs, AlignPipeline.align_prepared):
        assert inspect.signature(fn).parameters["want_u8"].default is False
    with pytest.raises(ValueError, match="Is_u8"):                  # before any device work
        AlignPipeline.align_prepared(None, dict(B=1), fine=True, want_u8=True)


# ---------------------------------------------------------------- header, binding, entry checks

NAMES = ("rfx_warp_records_u8", "rfx_warp_flow_u8")


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
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 19 and len(_lib.SIGNATURES[NAMES[1]][1]) == 11
    # the entries' comment cites the reference lines they replace
    assert "quick_start/align2images.py:97-98,117" in text and ":25-28,112" in text
    # appended: every earlier prototype still stands before them, in its place
    order = re.findall(r"\b(?:int|size_t)\s+(rfx_[a-z0-9_]+)\s*\(", hdr)
    assert order[-2:] == list(NAMES) and order.index("rfx_records_keypoints_f32") < order.index("rfx_less_than_u8_f32") < len(order) - 2
    lib = _lib.load()
    assert lib.rfx_abi_version() == 17
    for name in NAMES:
        assert hasattr(lib, name)


def test_argument_checks_answer_before_any_device_call():
    """Every call below carries at least one defect and returns from the entry point's opening checks; the (fake, aligned) pointers
    are never followed."""
    lib = _lib.load()
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]
    null = ctypes.c_void_p(0)
    E_ARG, E_LIMIT = -1, -2

    def rec(rec=P[0], rec_elems=3000, width=1000, max_h=4, off_H=4, off_flow=40, table=P[1], B=3, max_hw=100, bg=P[2], itable=P[3],
            img=P[4], overlay=P[5], mask=P[6], total_px=300):
        return lib.rfx_warp_records_u8(rec, rec_elems, width, max_h, off_H, off_flow, table, B, max_hw, 0.5, 1, 1, bg, itable, img,
                                       overlay, mask, total_px, null)
    for name in ("rec", "table", "itable", "img"):
        assert rec(**{name: null}) == E_ARG, name
        assert rec(**{name: null, "bg": null, "overlay": null, "mask": null}) == E_ARG, name      # those three are optional
    for bad in (dict(B=0), dict(width=0), dict(max_h=0), dict(off_H=0), dict(off_flow=39), dict(off_flow=1001), dict(rec_elems=2999),
                dict(max_hw=0), dict(total_px=99), dict(table=ctypes.c_void_p(0x20004)), dict(itable=ctypes.c_void_p(0x40004))):
        assert rec(**bad) == E_ARG, bad
    assert rec(B=65536, rec_elems=65536000) == E_LIMIT and rec(max_hw=1 << 31, total_px=1 << 31) == E_LIMIT
    assert rec(max_hw=1 << 31, total_px=1 << 31, img=null) == E_ARG                                # a bad argument is named before the limit

    def flo(flow=P[0], table=P[1], B=3, max_hw=100, binary=P[2], itable=P[3], img=P[4], overlay=P[5], mask=P[6], total_px=300):
        return lib.rfx_warp_flow_u8(flow, table, B, max_hw, binary, itable, img, overlay, mask, total_px, null)
    for name in ("flow", "table", "itable", "img"):
        assert flo(**{name: null}) == E_ARG, name
    assert flo(binary=null) == E_ARG                                # a mask without a binary to pass through
    for bad in (dict(B=0), dict(max_hw=0), dict(total_px=99), dict(flow=ctypes.c_void_p(0x10004)), dict(table=ctypes.c_void_p(0x20004)),
                dict(itable=ctypes.c_void_p(0x40004))):
        assert flo(**bad) == E_ARG, bad
    assert flo(B=65536) == E_LIMIT and flo(max_hw=1 << 31, total_px=1 << 31) == E_LIMIT


def test_warp_image_kernels_need_no_scratch_no_lds_and_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {r["kernel"]: r for r in kr.table(_lib.LIB_PATH) if r["unit"] == "warp_image"}
    assert set(rows) == {"warp_records_u8_kernel", "warp_flow_u8_kernel"}
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["wg"] == 256 and r["lds"] == 0, r
        assert r["vgpr"] <= 128 and r["agpr"] == 0, r               # at least four wavefronts per SIMD
    mk = open(os.path.join(ROOT, "ransac-flow_amd", "csrc", "Makefile")).read()
    assert re.search(r"^EXTRA_warp_image\s*=.*-ffp-contract=off", mk, flags=re.M) and re.search(r"^SRCS\s*=.*\swarp_image\.hip\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "ransac-flow_amd", "csrc", "warp_image.hip")).read()
    assert src.index('#include "assemble_pixel.h"') < src.index("#pragma clang fp contract(off)")
    lines = [l.rstrip("\n").split("\t") for l in open(os.path.join(ROOT, "profiles", "r06_kernel_resources.tsv")) if not l.startswith("#")]
    committed = {l[1]: dict(zip(lines[0], l)) for l in lines[1:] if l[0] == "warp_image"}
    assert set(committed) == set(rows)
    for k, r in rows.items():
        assert all(str(r[c]) == committed[k][c] for c in ("wg", "vgpr", "sgpr", "lds", "scratch")), (k, r, committed[k])
