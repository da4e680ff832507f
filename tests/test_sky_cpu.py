"""Sky masks for a batch of targets, host side: the BILINEAR coefficient tables against Pillow itself, the filter argument of
rfx/lanczos.py, the C ABI surface of the new entry points, and a numpy statement of ops.sky_background against the scripts'
``imresize(mask, (h, w)) < 128`` (the scipy 1.2.3 stand-in of dropin/run_reference_script.py).  Nothing is launched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import PIL.Image as Image

from rfx import _lib, lanczos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rfx_seg_vote_f32", "rfx_sky_bytes_ws_bytes", "rfx_sky_bytes_u8", "rfx_less_than_u8_f32")

# (channels, in (h, w), out (h, w)): RGB up in both directions, up from another aspect, KITTI down, 0/255 maps down, one pass only,
# 8x up, 8x down, transposed size
BILINEAR_CASES = [(3, (96, 128), (304, 400)), (3, (200, 264), (304, 400)), (3, (375, 1242), (152, 504)), (1, (97, 131), (48, 64)),
                  (1, (97, 131), (200, 131)), (1, (60, 80), (480, 640)), (1, (480, 640), (60, 80)), (1, (33, 47), (47, 33))]


def case_image(c, hw, seed):
    rng = np.random.default_rng(seed)
    if c == 3:
        return rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
    # a 0/255 map with structure at several scales: blocks, a thin line, single pixels
    m = (rng.random((hw[0] // 8 + 1, hw[1] // 8 + 1)) > 0.5).repeat(8, 0).repeat(8, 1)[:hw[0], :hw[1]].copy()
    m[hw[0] // 3] = True
    m[rng.integers(0, hw[0], 20), rng.integers(0, hw[1], 20)] ^= True
    return (m.astype(np.uint8) * 255)[:, :, None]


def pil_resize(a, out_hw, resample):
    im = Image.fromarray(a if a.shape[2] == 3 else a[:, :, 0])
    return np.asarray(im.resize((out_hw[1], out_hw[0]), resample)).reshape(out_hw[0], out_hw[1], a.shape[2])


def imresize_standin(arr, size):
    """The launcher's stand-in for scipy.misc.imresize (dropin/run_reference_script.py, restated from scipy 1.2.3), interp="bilinear";
    test_restated_imresize_is_the_launchers pins this copy on it."""
    data = np.asarray(arr)
    if data.dtype != np.uint8:
        cmin, cmax = data.min(), data.max()
        cscale = (cmax - cmin) or 1
        data = (((data - cmin) * (255.0 / cscale)).clip(0, 255) + 0.5).astype(np.uint8)
    im = Image.frombytes("L", (data.shape[1], data.shape[0]), data.tobytes())
    return np.asarray(im.resize((int(size[1]), int(size[0])), resample=Image.BILINEAR))


def script_background(mask, out_hw, k=0):
    """evaluation/evalYFCC/evaluation.py:193,200 on one 0 / 1 float mask."""
    return (imresize_standin(np.rot90(mask, k), out_hw) < 128).astype(np.float32)


def sky_background_numpy(mask, out_hw, k=0):
    """What ops.sky_background computes, per map: the byte form (255 where non-zero if the map holds both a zero and a non-zero value,
    else all zeros), k quarter turns, Pillow BILINEAR as the two table-driven integer passes with C = 1, < 128."""
    nz = mask != 0
    b = (nz.astype(np.uint8) * 255) if (nz.any() and not nz.all()) else np.zeros(mask.shape, np.uint8)
    b = np.ascontiguousarray(np.rot90(b, k))
    r = lanczos.apply_numpy(b[:, :, None], int(out_hw[1]), int(out_hw[0]), "bilinear")[:, :, 0]
    return (r < 128).astype(np.float32)


def sky_maps(hw, seed=0):
    """name -> 0 / 1 float32 mask: mixed, all-zero, all-one, a single non-zero pixel."""
    rng = np.random.default_rng(seed)
    mixed = (case_image(1, hw, seed)[:, :, 0] > 0).astype(np.float32)
    one_px = np.zeros(hw, np.float32)
    one_px[int(rng.integers(0, hw[0])), int(rng.integers(0, hw[1]))] = 1.0
    return dict(mixed=mixed, zeros=np.zeros(hw, np.float32), ones=np.ones(hw, np.float32), one_px=one_px)


@pytest.mark.parametrize("c,in_hw,out_hw", BILINEAR_CASES)
def test_bilinear_tables_equal_pillow_byte_for_byte(c, in_hw, out_hw):
    a = case_image(c, in_hw, seed=in_hw[0] + out_hw[1])
    got = lanczos.apply_numpy(a, out_hw[1], out_hw[0], "bilinear")
    assert got.dtype == np.uint8 and np.array_equal(got, pil_resize(a, out_hw, Image.BILINEAR))
    # and the filter it always had is still what the default names
    if in_hw[0] * in_hw[1] <= 200 * 264:
        assert np.array_equal(lanczos.apply_numpy(a, out_hw[1], out_hw[0]), pil_resize(a, out_hw, Image.LANCZOS))


def test_default_filter_is_lanczos_and_shares_its_cache_entry():
    for a, b in ((128, 400), (1242, 504), (97, 97)):
        d, l = lanczos.coeffs(a, b), lanczos.coeffs(a, b, "lanczos")
        assert d is l and d[2] == l[2] and np.array_equal(d[0], l[0]) and np.array_equal(d[1], l[1])
        t = lanczos.coeffs(a, b, "bilinear")
        assert t is lanczos.coeffs(a, b, "bilinear") and t is not d
        assert t[2] == int(np.ceil(max(a / b, 1.0))) * 2 + 1 and t[2] <= d[2]                 # support 1.0 against 3.0
    p, q = lanczos.plan(128, 96, 400, 304), lanczos.plan(128, 96, 400, 304, "lanczos")
    assert p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) for k in p)
    assert lanczos.plan(128, 96, 128, 96, "bilinear") is None
    with pytest.raises(ValueError):
        lanczos.coeffs(10, 20, "bicubic")
    # the triangle of libImaging/Resample.c: 1 - |x| inside (-1, 1)
    assert [lanczos._bilinear(x) for x in (-1.5, -1.0, -0.25, 0.0, 0.5, 1.0)] == [0.0, 0.0, 0.75, 1.0, 0.5, 0.0]


def test_new_entry_points_agree_between_header_binding_and_ops():
    hdr = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    assert re.search(r"#define\s+RFX_ABI_VERSION\s+17\b", hdr) and _lib.ABI_VERSION == 17
    bare = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = {n: (r, a) for r, n, a in re.findall(r"\b(int|size_t)\s+(rfx_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)}
    kinds = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}
    for name in NEW_SYMBOLS:
        assert name in protos and name in _lib.SIGNATURES, name
        ret, args = protos[name]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t)
        want = []
        for p in args.split(","):
            d = " ".join(p.split())
            want.append(ctypes.c_void_p if "*" in d else kinds[d.rsplit(" ", 1)[0].replace("const ", "").strip()])
        assert want == list(argtypes), (name, want, argtypes)
    assert len(_lib.SIGNATURES["rfx_seg_vote_f32"][1]) == 14 and len(_lib.SIGNATURES["rfx_sky_bytes_u8"][1]) == 8
    # each entry cites the reference lines it replaces
    for cite in ("segNet/segEval.py:27-43", "evaluation/evalYFCC/evaluation.py:193", "evalKITTI/evaluation.py:247-248",
                 "evalHpatch/evaluation.py:180"):
        assert cite in hdr, cite
    from rfx import ops, segnet, pipeline
    for fn in ("pil_resize_u8", "lanczos_resize_u8", "seg_vote", "sky_bytes", "less_than_u8", "sky_background"):
        assert callable(getattr(ops, fn)), fn
    assert callable(segnet.SegNetDevice.get_sky_batch) and callable(pipeline.AlignPipeline.sky_backgrounds)
    import inspect
    for drv in ("multi_h_pairs", "multi_h_kitti_pairs", "multi_h_variant_c_pairs"):
        assert inspect.signature(getattr(pipeline.AlignPipeline, drv)).parameters["seg"].default is None
    assert inspect.signature(ops.pil_resize_u8).parameters["resample"].default == "lanczos"
    assert list(inspect.signature(ops.lanczos_resize_u8).parameters) == ["img", "out_w", "out_h"]
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rfx_abi_version() == 17 and all(hasattr(lib, n) for n in NEW_SYMBOLS)
        # refusals that are answered before any HIP call
        assert lib.rfx_sky_bytes_ws_bytes(3) == 12 and lib.rfx_sky_bytes_ws_bytes(0) == 0
        one = (ctypes.c_void_p * 1)(64)
        hs, ws = (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 1)(4)
        vote = lambda *a: lib.rfx_seg_vote_f32(*a, None)
        assert vote(None, hs, ws, 1, 1, 2, 4, 4, 1.0, 0, 0, 64, None) == -1
        assert vote(one, hs, ws, 0, 1, 2, 4, 4, 1.0, 0, 0, 64, None) == -1 and vote(one, hs, ws, 9, 1, 2, 4, 4, 1.0, 0, 0, 64, None) == -1
        assert vote(one, hs, ws, 1, 1, 2, 0, 4, 1.0, 0, 0, 64, None) == -1 and vote(one, hs, ws, 1, 1, 2, 4, 4, 1.0, 0, 0, None, None) == -1
        assert vote(one, hs, ws, 1, 1, 2, 4, 4, 0.0, 0, 0, 64, None) == -1
        assert vote((ctypes.c_void_p * 1)(None), hs, ws, 1, 1, 2, 4, 4, 1.0, 0, 0, 64, None) == -1
        assert vote(one, hs, ws, 1, 4, 2, 32768, 32768, 1.0, 0, 0, 64, None) == -2                   # N*H*W = 2^32
        assert lib.rfx_sky_bytes_u8(64, 1, 4, 4, 4, 64, 64, None) == -1 and lib.rfx_sky_bytes_u8(None, 1, 4, 4, 0, 64, 64, None) == -1
        assert lib.rfx_sky_bytes_u8(64, 4, 32768, 32768, 0, 64, 64, None) == -2
        assert lib.rfx_less_than_u8_f32(64, 0, 128, 64, None) == -1 and lib.rfx_less_than_u8_f32(None, 4, 128, 64, None) == -1


def test_restated_imresize_is_the_launchers():
    """imresize_standin above against the function dropin/run_reference_script.py installs as scipy.misc.imresize (looked up in its
    source: installing it would replace modules for the rest of the session)."""
    src = open(os.path.join(ROOT, "ransac-flow_amd", "dropin", "run_reference_script.py")).read()
    body = src[src.index("        def imresize("):src.index("        sm.imresize = imresize")]
    ns = {}
    exec("\n".join(l[8:] for l in body.splitlines()), ns)
    rng = np.random.default_rng(1)
    for m in list(sky_maps((37, 53)).values()) + [rng.random((20, 31)).astype(np.float32), rng.integers(0, 256, (20, 31), dtype=np.uint8)]:
        for size in ((48, 64), (19, 40)):
            assert np.array_equal(ns["imresize"](m, size), imresize_standin(m, size))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_numpy_statement_of_sky_background_equals_the_scripts(k):
    for hw in ((61, 83), (97, 131)):
        for name, m in sky_maps(hw, seed=k).items():
            for out in ((48, 64), (200, 131), hw, (hw[0] * 3 + 1, hw[1] * 2 + 3), (9, 7)):     # down, mixed, unchanged, up, far down
                out = out[::-1] if k & 1 else out
                got, ref = sky_background_numpy(m, out, k), script_background(m, out, k)
                assert got.shape == ref.shape == tuple(out) and got.dtype == ref.dtype and np.array_equal(got, ref), (name, hw, out, k)
                if name in ("zeros", "ones"):
                    assert got.min() == 1.0                   # a constant map: bytescale gives zeros, every pixel is below 128
    # the byte rule is per map: a mixed map next to constant ones keeps its own scale
    m = sky_maps((61, 83))["mixed"]
    assert 0.0 < sky_background_numpy(m, (48, 64)).mean() < 1.0
