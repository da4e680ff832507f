"""Host side of the point correspondences and the keypoint transfer (csrc/points.hip; ops.flow_points / matches_from_flow /
sample_points; assemble.assemble_yfcc / yfcc_matches / corr_alignment_error; the drop-in's yfcc namespace).

The yardstick first: the rule the kernels are held to, stated in numpy in this file's own words (rule_points, rule_sample, shared
with tests/test_gpu_points.py), equals what the reference's own matches_from_flow (evaluation/evalYFCC/getResults.py:53-71) and
alignmentError (evaluation/evalCorr/getResults.py:15-38) returned for tests/golden/points.npz, exactly -- and, where the reference's
source tree is present, what they return on fresh seeds.  Then the surface: header, binding, workspace sizes, the argument checks
that answer before any HIP call, the Python-level refusals, the static resources of the four kernels.  Nothing is launched."""
import ctypes
import hashlib
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
TILE = 1024                                                        # pixels of one workgroup's tile (csrc/points.hip)


# ---------------------------------------------------------------- the rule

def rule_points(flow, keep, sizeA, sizeB, angle, bg=None):
    """flow (N,H,W,2) float32, keep / bg (N,H,W) -> (pts1 (n,2) float32, pts2 (n,2) int64, offsets (N+1,) int64).
    Order: map after map, row-major inside a map (np.nonzero lists its hits in exactly that order).  pts1: add 1, times (size - 1),
    halve, every step a float32 operation.  pts2: the entry (i, j) of the target's pixel grid turned k quarter turns
    counter-clockwise, written out for the four k."""
    (wA, hA), (wB, hB), k = sizeA, sizeB, (angle // 90) % 4
    m = keep != 0
    if bg is not None:
        m = m & (bg != 0)
    assert flow.dtype == np.float32 and m.shape[1:] == ((hB, wB) if k % 2 == 0 else (wB, hB))
    n, i, j = np.nonzero(m)
    one, two = np.float32(1), np.float32(2)
    pts1 = np.empty((len(n), 2), np.float32)
    for c, size in ((0, wA), (1, hA)):
        t = flow[n, i, j, c] + one
        t = t * np.float32(size - 1)
        pts1[:, c] = t / two
    x, y = ((j, i), (wB - 1 - i, j), (wB - 1 - j, hB - 1 - i), (i, hB - 1 - j))[k]
    pts2 = np.stack((x, y), axis=1).astype(np.int64)
    offsets = np.concatenate(([0], np.cumsum(m.reshape(len(m), -1).sum(axis=1)))).astype(np.int64)
    return pts1, pts2, offsets


def rule_sample(flow, match, xb, yb, sizeA):
    """flow (H,W,2), match (H,W) float32; integer pixels -> (xa, ya float32, keep bool): add 1, halve, times (size - 1), in float32."""
    one, half = np.float32(1), np.float32(0.5)
    xa = ((flow[yb, xb, 0] + one) * half) * np.float32(sizeA[0] - 1)
    ya = ((flow[yb, xb, 1] + one) * half) * np.float32(sizeA[1] - 1)
    return xa, ya, match[yb, xb] > half


def rule_alignment_error(wB, hB, wA, hA, XA, YA, XB, YB, flow, match, pixelGrid):
    """The tally over the kept keypoints, float64 from the float32 estimates on, zeros when none is kept."""
    xa, ya, xb, yb = (np.asarray(v).astype(np.int64) for v in (XA, YA, XB, YB))
    ex, ey, keep = rule_sample(flow.reshape(hB, wB, 2), match.reshape(hB, wB), xb, yb, (wA, hA))
    if not keep.any():
        return np.zeros(pixelGrid.shape[1]), 0
    d = ((ex[keep].astype(np.float64) - xa[keep]) ** 2 + (ey[keep].astype(np.float64) - ya[keep]) ** 2) ** 0.5
    return (d[:, None] <= pixelGrid).sum(axis=0), int(keep.sum())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_gold = {}


def golden():
    """tests/golden/points.npz, decoded once: dict(bg, cases=[(th, multiH, flow (H,W,2), binary (H,W))], angles, sizeA, sizeB, raw)."""
    if not _gold:
        g = np.load(os.path.join(GOLD, "points.npz"))
        H, W = int(g["hd"]) * 8, int(g["wd"]) * 8
        unpack = lambda a: np.unpackbits(a)[:H * W].reshape(H, W).astype(bool)
        last = g["case2_flow"]
        cases = []
        for c in range(3):
            flow = last if c == 2 else (g["case%d_flow_xor" % c] ^ last.view(np.int32)).view(np.float32)
            cases.append((float(g["case%d_cfg" % c][0]), bool(g["case%d_cfg" % c][1]), flow, unpack(g["case%d_binary" % c])))
        _gold.update(bg=unpack(g["bg"]), cases=cases, angles=[int(a) for a in g["angles"]],
                     sizeA=[tuple(int(v) for v in s) for s in g["sizeA"]], sizeB=[tuple(int(v) for v in s) for s in g["sizeB"]],
                     raw=g, hw=(H, W))
    return _gold


def test_rule_equals_the_reference_outputs_in_the_golden_file():
    G = golden()
    g = G["raw"]
    assert [c[3].sum() for c in G["cases"]] == [7072, 2845, 6227] and G["bg"].mean() < 0.85
    for c, (th, multiH, flow, binary) in enumerate(G["cases"]):
        assert not binary[~G["bg"]].any()                           # the reference's mask already carries matchBG
        for a, angle in enumerate(G["angles"]):
            pts1, pts2, off = rule_points(flow[None], binary[None], G["sizeA"][a], G["sizeB"][a], angle)
            assert len(pts1) == int(g["case%d_a%d_n" % (c, a)]) == off[1] and off[0] == 0
            assert sha(pts1) == str(g["case%d_a%d_sha1" % (c, a)]), (c, angle)
            assert sha(pts2) == str(g["case%d_a%d_sha2" % (c, a)]), (c, angle)
            if (c, a) == (int(g["full_case"]), int(g["full_angle"])):
                assert np.array_equal(pts1.view(np.int32), g["full_pts1"].view(np.int32))
                assert np.array_equal(pts2, g["full_pts2"].astype(np.int64))
    wB, hB, wA, hA = (int(v) for v in g["ae_dims"])
    args = (wB, hB, wA, hA, g["ae_XA"], g["ae_YA"], g["ae_XB"], g["ae_YB"])
    counts, nb = rule_alignment_error(*args, g["ae_flow"], g["ae_match"], g["ae_grid"])
    assert nb == int(g["ae_nb"]) == 22 and np.array_equal(counts, g["ae_counts"]) and counts.dtype == g["ae_counts"].dtype
    counts, nb = rule_alignment_error(*args, g["ae_flow"], g["ae_match"] * np.float32(0.5), g["ae_grid"])
    assert nb == int(g["ae_none_nb"]) == 0 and np.array_equal(counts, g["ae_none_counts"]) and counts.dtype == np.float64
    assert np.array_equal(g["ae_grid"], np.around(np.logspace(0, np.log10(36), 8).reshape(-1, 8)))


def test_rule_details():
    """The pieces of the rule, each on a case small enough to read: the four quarter turns against np.rot90 itself, the order, the
    empty map, bg, and the float32 steps on values where a fused or reordered step shows."""
    hB, wB = 3, 5
    gx, gy = np.meshgrid(np.arange(wB), np.arange(hB))
    grid = np.stack((gx, gy), axis=2)
    for k in range(4):
        turned = np.rot90(grid, k)
        shape = turned.shape[:2]
        assert shape == ((hB, wB) if k % 2 == 0 else (wB, hB))
        keep = np.ones((1,) + shape, bool)
        for angle in (90 * k, 90 * k + 360, 90 * k + 45):           # k = (angle // 90) % 4, as np.rot90 reduces it
            _, pts2, off = rule_points(np.zeros(shape + (2,), np.float32)[None], keep, (7, 9), (wB, hB), angle)
            assert np.array_equal(pts2, turned.reshape(-1, 2)) and pts2.dtype == np.int64 and list(off) == [0, hB * wB]
    keep = np.zeros((3, 2, 3), bool)                               # map 1 empty
    keep[0, 1, 2] = keep[0, 0, 1] = keep[2, 1, 0] = keep[2, 0, 0] = True
    flow = np.arange(36, dtype=np.float32).reshape(3, 2, 3, 2) / 64 - np.float32(0.25)
    pts1, pts2, off = rule_points(flow, keep, (3, 5), (3, 2), 0)
    assert list(off) == [0, 2, 2, 4] and pts2.tolist() == [[1, 0], [2, 1], [0, 0], [0, 1]]
    assert np.array_equal(pts1, ((flow[keep] + 1) * np.array([2, 4], np.float32)) / 2)
    bg = np.ones_like(keep)
    bg[0, 0, 1] = False
    assert list(rule_points(flow, keep, (3, 5), (3, 2), 0, bg)[2]) == [0, 1, 1, 3]
    e = rule_points(flow, np.zeros_like(keep), (3, 5), (3, 2), 0)
    assert e[0].shape == (0, 2) and e[1].shape == (0, 2) and list(e[2]) == [0, 0, 0, 0]
    # (x + 1) * 639 / 2 in float32 steps differs from the float64 value rounded once, and from x * 319.5 + 319.5
    # (on x whose sum with 1 is inexact: a float32 formed as 2 u - 1 from a float32 u adds to 1 exactly, and then nothing shows)
    x = (np.random.RandomState(0).rand(4096) * 2 - 1).astype(np.float32)
    f = np.stack((x, x), axis=1).reshape(1, 1, 4096, 2)
    p = rule_points(f, np.ones((1, 1, 4096), bool), (640, 640), (4096, 1), 0)[0][:, 0]
    assert (p != ((x.astype(np.float64) + 1) * 639 / 2).astype(np.float32)).any()
    assert (p != x * np.float32(319.5) + np.float32(319.5)).any()
    assert np.array_equal(p, ((x + np.float32(1)) * np.float32(639)) / np.float32(2))


@pytest.mark.reference
def test_rule_equals_the_live_reference_on_fresh_seeds():
    import ref_loader
    if ref_loader.staged():
        pytest.skip("the YFCC results script is not part of the staged reference")
    fy = ref_loader.script_functions("evaluation/evalYFCC/getResults.py", ["matches_from_flow"])["matches_from_flow"]
    fc = ref_loader.script_functions("evaluation/evalCorr/getResults.py", ["alignmentError"])["alignmentError"]
    for seed in range(6):
        rng = np.random.RandomState(100 + seed)
        hB, wB = int(rng.randint(2, 40)), int(rng.randint(2, 40))     # (alignmentError squeezes a size-1 axis away)
        sizeA = (int(rng.randint(1, 5000)), int(rng.randint(1, 5000)))
        for angle in (0, 90, 180, 270, 450):
            shape = (hB, wB) if (angle // 90) % 2 == 0 else (wB, hB)
            flow = (rng.rand(*shape, 2) * 2.2 - 1.1).astype(np.float32)
            keep = rng.rand(*shape) < (0.0, 0.3, 0.5, 0.9, 1.0, 0.05)[seed]
            want1, want2 = fy(flow.copy(), keep.astype(np.float32), sizeA, (wB, hB), angle)
            got1, got2, _ = rule_points(flow[None], keep[None], sizeA, (wB, hB), angle)
            assert want1.dtype == got1.dtype and want2.dtype == got2.dtype
            assert np.array_equal(want1.view(np.int32), got1.view(np.int32)) and np.array_equal(want2, got2), (seed, angle)
        K, wA, hA = 50, sizeA[0], sizeA[1]
        flow = (rng.rand(1, hB, wB, 2) * 2 - 1).astype(np.float32)
        match = rng.rand(1, hB, wB, 1).astype(np.float32)
        XB, YB = (rng.rand(K) * wB).astype(np.float32), (rng.rand(K) * hB).astype(np.float32)
        XA, YA = (rng.rand(K) * wA).astype(np.float32), (rng.rand(K) * hA).astype(np.float32)
        grid = np.around(np.logspace(0, np.log10(max(wA, hA)), 8).reshape(-1, 8))
        for mm in (match, match * np.float32(0.5)):
            want, nb = fc(wB, hB, wA, hA, XA, YA, XB, YB, torch.from_numpy(flow), torch.from_numpy(mm), grid)
            got, gnb = rule_alignment_error(wB, hB, wA, hA, XA, YA, XB, YB, flow, mm, grid)
            assert nb == gnb and np.array_equal(want, got) and want.dtype == got.dtype, seed


# ---------------------------------------------------------------- the surface

NAMES = ("rfx_flow_points_ws_bytes", "rfx_flow_points_f32", "rfx_sample_points_f32")


def test_header_and_binding_declare_the_entry_points():
    C = ctypes
    text = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert int(re.search(r"#define RFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 17
    kinds = {"int": C.c_int, "int32_t": C.c_int, "long long": C.c_longlong, "float": C.c_float, "size_t": C.c_size_t}
    for name in NAMES:
        ret, args = re.search(r"\b(int|size_t)\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S).groups()
        res, argtypes = _lib.SIGNATURES[name]
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[ret], name
        params = [" ".join(p.split()) for p in args.split(",")]
        want = [C.c_void_p if "*" in p else kinds[p.rsplit(" ", 1)[0].replace("const ", "")] for p in params]
        assert want == argtypes, (name, params)
    assert len(_lib.SIGNATURES["rfx_flow_points_f32"][1]) == 16 and len(_lib.SIGNATURES["rfx_sample_points_f32"][1]) == 13
    # each entry's comment cites the reference lines it replaces
    assert "evaluation/evalYFCC/getResults.py:53-71" in text and "evaluation/evalCorr/getResults.py:15-31" in text
    lib = _lib.load()
    assert lib.rfx_abi_version() == 17
    ws = lib.rfx_flow_points_ws_bytes
    assert ws(1, 480, 720) == 4 * 338 and ws(16, 480, 720) == 16 * 4 * 338           # ceil(345600 / 1024) = 338 tiles per map
    assert ws(1, 1, 1) == 4 and ws(3, 1, TILE) == 12 and ws(3, 1, TILE + 1) == 24 and ws(9000, 2, 3) == 36000
    assert ws(0, 4, 4) == ws(4, 0, 4) == ws(4, 4, -1) == 0
    assert ws(1 << 30, 1, 1) == 4 << 30 and ws(2, 46341, 46341) == 2 * 4 * ((46341 * 46341 + TILE - 1) // TILE)   # past 2^31


def test_argument_checks_answer_before_any_device_call():
    """Every call below carries at least one defect and returns from the entry point's opening checks; the pointers (fake, aligned
    as the entry asks) are never followed."""
    lib = _lib.load()
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]
    null = ctypes.c_void_p(0)
    E_ARG, E_LIMIT = -1, -2

    def points(flow=P[0], keep=P[1], bg=P[2], N=1, H=6, W=8, k=0, wA=640, hA=480, wB=8, hB=6, pts1=P[3], pts2=P[4], offsets=P[5],
               ws=P[6]):
        return lib.rfx_flow_points_f32(flow, keep, bg, N, H, W, k, wA, hA, wB, hB, pts1, pts2, offsets, ws, null)
    for name in ("flow", "keep", "pts1", "pts2", "offsets", "ws"):
        assert points(**{name: null}) == E_ARG, name
        assert points(**{name: null, "bg": null}) == E_ARG, name     # bg is optional, the others are not
    for bad in (dict(N=0), dict(N=-1), dict(H=0, hB=0), dict(W=-3, wB=-3), dict(k=-1), dict(k=4), dict(wA=0), dict(hA=0), dict(wA=-5)):
        assert points(**bad) == E_ARG, bad
    # the map's shape is (hB, wB) for even k, (wB, hB) for odd k
    assert points(k=1) == E_ARG and points(k=3) == E_ARG and points(k=2, wB=6, hB=8) == E_ARG and points(k=0, wB=6, hB=8) == E_ARG
    assert points(k=1, wB=6, hB=8, N=0) == E_ARG and points(k=2, N=0) == E_ARG       # (these shapes fit: only N is wrong)
    assert points(H=7) == E_ARG and points(W=9) == E_ARG
    # one 8-byte store per pts1 row, one 16-byte store per pts2 row, 8-byte flow reads
    assert points(pts2=ctypes.c_void_p(0x50008)) == E_ARG and points(pts1=ctypes.c_void_p(0x40004)) == E_ARG
    assert points(flow=ctypes.c_void_p(0x10004)) == E_ARG and points(offsets=ctypes.c_void_p(0x60004)) == E_ARG
    # N * H * W = 2^31 is one too many; a bad argument is named before the limit
    assert points(N=32768, H=256, W=256, wB=256, hB=256) == E_LIMIT
    assert points(N=2, H=32768, W=32768, wB=32768, hB=32768, k=3) == E_LIMIT
    assert points(N=32768, H=256, W=256, wB=256, hB=256, ws=null) == E_ARG
    assert points(N=32768, H=256, W=256, wB=256, hB=256, k=5) == E_ARG

    def sample(flow=P[0], match=P[1], xb=P[2], yb=P[3], K=4, H=6, W=8, wA=640, hA=480, xa=P[4], ya=P[5], keep=P[6]):
        return lib.rfx_sample_points_f32(flow, match, xb, yb, K, H, W, wA, hA, xa, ya, keep, null)
    for name in ("flow", "match", "xb", "yb", "xa", "ya", "keep"):
        assert sample(**{name: null}) == E_ARG, name
    for bad in (dict(K=0), dict(K=-2), dict(H=0), dict(W=0), dict(wA=0), dict(hA=0), dict(flow=ctypes.c_void_p(0x10004))):
        assert sample(**bad) == E_ARG, bad
    assert sample(H=65536, W=32768) == E_LIMIT and sample(H=65536, W=32768, K=0) == E_ARG


def test_python_level_refusals():
    f, m = torch.zeros(6, 8, 2), torch.ones(6, 8, dtype=torch.bool)
    for op in (ops.flow_points, ops.matches_from_flow):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # the shapes fit: the device is what is wrong
            op(f, m, (640, 480), (8, 6))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            op(f[None], m[None], (640, 480), (6, 8), angle=270, bg=m[None])
        for bad in (dict(sizeB=(6, 8)), dict(sizeB=(8, 6), angle=90), dict(sizeB=(8, 7)), dict(sizeB=(8, 6), angle=-90)):
            with pytest.raises(ValueError, match="do not fit"):     # numpy raises IndexError there
                op(f, m, (640, 480), **bad)
        with pytest.raises(ValueError):
            op(f, m[:5], (640, 480), (8, 6))
        with pytest.raises(ValueError):
            op(f, m, (640, 480), (8, 6), bg=m[:, :7])
        with pytest.raises(ValueError):
            op(f, m, (0, 480), (8, 6))
        with pytest.raises(ValueError):
            op(torch.zeros(6, 8, 3), m, (640, 480), (8, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_points(f, torch.ones(6, 8), [1, 2], [3, 4], (640, 480))
    # missing files: the reference's sentinel, before anything touches a device
    assert assemble.yfcc_getFlow(8, "/nonexistent", ["flow_7_3H.npy"], "/nonexistent", "/nonexistent", True, 0.5) == ([], [])
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    assert sorted(vars(getResults.yfcc)) == ["_getFlow", "getFlow", "matches_from_flow"]
    assert callable(getResults.corr.alignmentError) and callable(getResults.corr.getFlow) and callable(getResults.kitti.getFlow_all)
    assert getResults.yfcc.getFlow(8, "/nonexistent", ["flow_7_3H.npy"], "/nonexistent", "/nonexistent", True, 0.5) == ([], [])


def test_points_kernels_need_no_scratch_and_a_few_words_of_lds():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {r["kernel"]: r for r in kr.table(_lib.LIB_PATH) if r["unit"] == "points"}
    assert set(rows) == {"points_count_kernel", "points_scan_kernel", "points_scatter_kernel", "sample_points_kernel"}
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["waves_per_simd"] == 8, r
    # the tallies only: one int32 per wavefront (count, scan), two per wavefront (the scatter's double buffer), none (sample)
    lds = {k: r["lds"] for k, r in rows.items()}
    assert lds == {"points_count_kernel": 16, "points_scan_kernel": 64, "points_scatter_kernel": 32, "sample_points_kernel": 0}
    assert {k: r["wg"] for k, r in rows.items()} == {"points_count_kernel": 256, "points_scan_kernel": 1024,
                                                     "points_scatter_kernel": 256, "sample_points_kernel": 256}
