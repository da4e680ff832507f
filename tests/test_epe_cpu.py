"""Host side of the end-point error on the device (csrc/epe.hip: rfx_epe_homography_f32, rfx_epe_flow_f32; ops.epe_homography /
epe_flow; assemble.hpatch_gt_homography / hpatch_epe / kitti_epe; the drop-in's hpatch.epe_from_homography and kitti.epe).

The yardstick first: the rule the kernels are held to, stated in numpy in this file's own words (rule_grid_gt, rule_epe_homography,
rule_epe_flow, shared with tests/test_gpu_epe.py).  The reference has the HPatches part in two functions, getGT
(evaluation/evalHpatch/getResults.py:83-144) and epe (:147-156), joined by module-level statements (:221-250): keep the pixels whose
ground-truth coordinates both lie in [-1, 1], turn both maps into pixels by (x + 1) * (minSize - 1) / 2, take the mean length of the
difference.  The KITTI part is module-level only (evaluation/evalKITTI/getResults.py:221-228): the flow minus the linspace grid,
times (size - 1), halved, in float32; its float64 distance to the ground truth u, v; the sum over valid divided by the number of
valid pixels.  The rule equals what getGT returned for tests/golden/epe.npz bit for bit and, where the reference's source tree is
present, what getGT and epe return on fresh seeds.  Then the surface: header, binding, workspace sizes, the argument checks that
answer before any HIP call, the Python-level refusals, the static resources of the kernels.  Nothing is launched."""
import ctypes
import fractions
import hashlib
import importlib.util
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from rfx import assemble, ops, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TILE = 1024                                                        # pixels of one workgroup's tile (csrc/epe.hip)
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- the rule

def fma_f32(a, b, c):
    """round_to_float32(a * b + c) for float32 arrays, rounded ONCE.  a * b is exact in float64; the float64 sum with c may not be,
    and rounding it twice could miss a float32 tie: the sum's error term (two-sum) says on which side the true value lies, and a sum
    that is inexact is made odd in its last bit (round to odd), after which the rounding to float32 is the rounding of the true value."""
    p, c = a.astype(f64) * b.astype(f64), c.astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):                # inf - inf where an input is not finite
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def rule_grid_gt(Hinv, Sh, Sw):
    """Hinv (9,) or (N,9) float64 -> (gx, gy) float32 (Sh,Sw) or (N,Sh,Sw): Hinv (j, i, 1) in float64 as (h0 * j + h1 * i) + h2 per
    row, the three results rounded to float32, then ((2 * x) / (z + 1e-8)) / (size - 1) - 1 in float32 steps."""
    h = np.asarray(Hinv, f64)
    h = h.reshape((9, 1, 1) if h.size == 9 else (-1, 9, 1, 1))
    Y, X = np.mgrid[0:Sh, 0:Sw].astype(f64)
    xw, yw, zw = (((h[..., 3 * r, :, :] * X + h[..., 3 * r + 1, :, :] * Y) + h[..., 3 * r + 2, :, :]).astype(f32) for r in range(3))
    z = zw + f32(1e-8)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        gx = ((f32(2) * xw) / z) / f32(Sw - 1) - f32(1)
        gy = ((f32(2) * yw) / z) / f32(Sh - 1) - f32(1)
    return gx, gy


def to_pixels(v, size):
    t = v + f32(1)
    t = t * f32(size - 1)
    return t / f32(2)


def rule_epe_homography(flow, Hinv):
    """flow (N,Sh,Sw,2) float32, Hinv (N,9) float64 -> (err (N,Sh,Sw) float32 with NaN outside, count (N,) int64)."""
    N, Sh, Sw, _ = flow.shape
    gx, gy = rule_grid_gt(np.asarray(Hinv).reshape(N, 9), Sh, Sw)
    inside = (gx >= -1) & (gx <= 1) & (gy >= -1) & (gy <= 1)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = to_pixels(gx, Sw) - to_pixels(flow[..., 0], Sw)
        dy = to_pixels(gy, Sh) - to_pixels(flow[..., 1], Sh)
        e = np.sqrt(fma_f32(dy, dy, dx * dx))
    err = np.where(inside, e, f32(np.nan)).astype(f32)
    return err, inside.reshape(N, -1).sum(axis=1)


def rule_lin(n):
    """torch.linspace(-1, 1, n) as float32: step = 2 / (n - 1); the lower half step * i - 1, the upper half 1 - step * (n - 1 - i),
    each one fused multiply-add (exact in float64 for these sizes, then rounded once)."""
    if n <= 1:
        return np.full(n, -1, f32)
    step, i = f64(f32(2) / f32(n - 1)), np.arange(n)
    return np.where(i < n // 2, step * i - 1.0, 1.0 - step * (n - 1 - i)).astype(f32)


def rule_epe_flow(flow, u, v, valid):
    """flow (N,H,W,2), u, v (N,H,W) float32, valid (N,H,W) -> (err (N,H,W) float64 with NaN where not valid, count (N,))."""
    N, H, W, _ = flow.shape
    up = ((flow[..., 0] - rule_lin(W)[None, None, :]) * f32(W - 1)) / f32(2)
    vp = ((flow[..., 1] - rule_lin(H)[None, :, None]) * f32(H - 1)) / f32(2)
    assert up.dtype == f32 and vp.dtype == f32
    dx, dy = up.astype(f64) - u.astype(f64), vp.astype(f64) - v.astype(f64)
    err = np.sqrt(dx * dx + dy * dy)
    err[valid == 0] = np.nan
    return err, (valid != 0).reshape(N, -1).sum(axis=1)


def fsum_of(err):
    """(the exact sum of the errors that are not NaN, rounded once; their number)."""
    e = err[~np.isnan(err)]
    return math.fsum(e.astype(f64).tolist()), int(e.size)


def ulp32(x):
    return float(np.spacing(f32(abs(x))))


def flow_est_for(seed, S):
    """The seeded estimate the golden AEPEs were taken of."""
    return (np.random.RandomState(seed).rand(S, S, 2) * 2.2 - 1.1).astype(f32)


_gold = []


def golden():
    """tests/golden/epe.npz decoded once: [dict(kind, H, ref_hw, trg_hw, S, Hinv, sha, grid, seed, aepe, inside)]; sha = the SHA-256
    of getGT's (S,S,2) float32 map, grid = the map itself for the cases stored in full (S = 17), else None."""
    if not _gold:
        g = np.load(os.path.join(GOLD, "epe.npz"))
        full = iter(g["grid17"])
        for c in range(len(g["kind"])):
            sh = [int(x) for x in g["shapes"][c]]
            _gold.append(dict(kind=str(g["kind"][c]), H=g["H"][c], ref_hw=tuple(sh[0:2]), trg_hw=tuple(sh[2:4]), S=sh[4],
                              Hinv=g["Hinv"][c], sha=str(g["sha"][c]), grid=next(full) if sh[4] == 17 else None,
                              seed=int(g["seed"][c]), aepe=f32(g["aepe"][c]), inside=int(g["inside"][c])))
    return _gold


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == f32 else np.int64)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_rule_equals_the_reference_outputs_in_the_golden_file():
    G = golden()
    assert len(G) >= 18 and {c["S"] for c in G} == {17, 24, 33}
    assert {c["kind"] for c in G} == {"identity", "shift", "dyadic", "perspective"}
    for c in G:
        S = c["S"]
        gx, gy = rule_grid_gt(c["Hinv"], S, S)
        assert gx.dtype == f32 and sha(np.stack((gx, gy), axis=2)) == c["sha"], (c["kind"], S)
        assert (c["grid"] is not None) == (S == 17)
        if c["grid"] is not None:                                      # stored in full: a failing digest has a map to look at
            assert c["grid"].dtype == f32 and c["grid"].shape == (S, S, 2) and sha(c["grid"]) == c["sha"]
            assert np.array_equal(bits(gx), bits(c["grid"][..., 0])) and np.array_equal(bits(gy), bits(c["grid"][..., 1])), c["kind"]
        err, count = rule_epe_homography(flow_est_for(c["seed"], S)[None], c["Hinv"][None])
        assert count[0] == c["inside"]
        if c["kind"] == "identity":
            assert count[0] == S * S                                  # the border sits AT +-1 and is inside
        if c["kind"] == "perspective":
            assert S * S / 3 <= count[0] <= 2 * S * S / 3
        # the reference's float32 mean against the rule's float32(sum / count): both round the same exact value
        total, n = fsum_of(err)
        exact = total / n
        assert abs(float(f32(exact)) - float(c["aepe"])) <= abs(float(c["aepe"]) - exact) + ulp32(exact), c["kind"]
        # the nine numbers: the reference's own calls on the host
        Hs, Hinv = assemble.hpatch_gt_homography(c["H"], c["ref_hw"], c["trg_hw"], S)
        assert Hinv.dtype == f64 and np.allclose(Hinv, c["Hinv"].reshape(3, 3), rtol=1e-12, atol=1e-12 * np.abs(c["Hinv"]).max())
        assert np.allclose(Hs @ Hinv, np.eye(3), atol=1e-12)
        if c["kind"] != "perspective":                                 # exact arithmetic: the same bits on any BLAS
            assert np.array_equal(Hinv, c["Hinv"].reshape(3, 3))


def test_rule_details():
    """The pieces of the rule on cases small enough to read."""
    # the fused step, against exact rational arithmetic rounded once; inputs on which the unfused and the other fused form differ
    rng = np.random.RandomState(0)
    a, b = (rng.randn(4000) * 3).astype(f32), (rng.randn(4000) * 3).astype(f32)
    a[:4], b[:4] = [1 + 2.0 ** -12, 3, 2.0 ** -70, 1], [2.0 ** -13, 2.0 ** -40, 1, 2.0 ** -12 + 2.0 ** -23]
    got = fma_f32(b, b, a * a)

    def once(x, y, z):
        v = fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z))
        lo = f32(float(v))                                            # float(v) rounds correctly to float64; then find the nearest float32
        cands = [np.nextafter(lo, f32(-np.inf)), lo, np.nextafter(lo, f32(np.inf))]
        d = [abs(fractions.Fraction(float(q)) - v) for q in cands]
        best = min(d)
        near = [q for q, dd in zip(cands, d) if dd == best]
        return near[0] if len(near) == 1 else [q for q in near if (int(f32(q).view(np.int32)) & 1) == 0][0]
    want = np.array([once(y, y, x * x) for x, y in zip(a, b)], f32)
    assert np.array_equal(bits(got), bits(want))
    assert (got != a * a + b * b).any() and (got != fma_f32(a, a, b * b)).any()
    # step 6 itself: the root of that fused sum is what torch.norm(p=2, dim=1) gives a two-element row; the two other orders are not
    dx, dy = (rng.randn(57600) * 20).astype(f32), (rng.randn(57600) * 20).astype(f32)
    rows = torch.norm(torch.from_numpy(np.stack((dx, dy), axis=1)), p=2, dim=1).numpy()
    assert np.array_equal(bits(np.sqrt(fma_f32(dy, dy, dx * dx))), bits(rows))
    assert (np.sqrt(dx * dx + dy * dy) != rows).sum() > 1000 and (np.sqrt(fma_f32(dx, dx, dy * dy)) != rows).sum() > 1000
    # the grid: torch.linspace itself
    for n in (1, 2, 3, 17, 24, 33, 240, 375, 1242, 4097):
        assert np.array_equal(bits(rule_lin(n)), bits(torch.linspace(-1, 1, n).numpy())), n
    # the identity: the ground truth is the pixel grid, the border is inside, the error of the identity grid is 0 up to rounding
    S = 9
    gx, gy = rule_grid_gt(np.eye(3).ravel(), S, S)
    assert gx[0, 0] == -1 and gx[0, -1] == 1 and gy[-1, 0] == 1 and np.array_equal(gx[0], f32(2) * np.arange(S, dtype=f32) / f32(S - 1) - 1)
    ident = np.stack(np.broadcast_arrays(rule_lin(S)[None, :], rule_lin(S)[:, None]), axis=2).astype(f32)
    err, count = rule_epe_homography(ident[None], np.eye(3).reshape(1, 9))
    assert count[0] == S * S and err.max() < 1e-5
    # a shift by one pixel to the right: the last column maps outside, every kept pixel is one pixel off
    Hinv = np.array([1, 0, 1, 0, 1, 0, 0, 0, 1], f64)
    err, count = rule_epe_homography(ident[None], Hinv[None])
    assert count[0] == S * (S - 1) and np.isnan(err[0, :, -1]).all() and np.allclose(err[0, :, :-1], 1, atol=1e-5)
    # a degenerate row: z = -1e-8f makes the denominator 0 -> inf or NaN -> outside
    err, count = rule_epe_homography(ident[None], np.array([[1, 0, 0, 0, 1, 0, 0, 0, -float(f32(1e-8))]]))
    assert count[0] == 0 and np.isnan(err).all()
    # KITTI: a flow equal to the grid plus 2 d / (size - 1) is d pixels off
    H, W = 5, 9
    flow = np.stack(np.broadcast_arrays(rule_lin(W)[None, :], rule_lin(H)[:, None]), axis=2).astype(f32)[None].copy()
    flow[0, :, :, 0] += f32(2 * 3 / (W - 1))
    u, v = np.zeros((1, H, W), f32), np.zeros((1, H, W), f32)
    valid = np.zeros((1, H, W), bool)
    valid[0, 1, 2] = valid[0, 4, 8] = True
    err, count = rule_epe_flow(flow, u, v, valid)
    assert count[0] == 2 and np.isnan(err).sum() == H * W - 2 and np.allclose(err[0, 1, 2], 3, atol=1e-6) and err.dtype == f64
    u[0, 1, 2], v[0, 1, 2] = 3, 4
    assert np.allclose(rule_epe_flow(flow, u, v, valid)[0][0, 1, 2], 4, atol=1e-6)
    # KITTI's ground truth, (uint16 - 32768) / 64, is exact in float32 for every uint16
    g = (np.arange(65536, dtype=np.uint16).astype(float) - 32768) / 64.0
    assert np.array_equal(g.astype(f32).astype(f64), g)


def seat_cv2(fn, image):
    """getGT and readFlow read an image file through cv2 (absent here): a stand-in whose imread returns ``image``."""
    fn.__globals__["cv2"] = types.SimpleNamespace(imread=lambda path, flag: image, IMREAD_UNCHANGED=-1)


def reference_row(H, ref_hw):
    """A one-row table like the HPatches csv files: obj, im1, im2, Him, Wim, then the nine entries of H."""
    import pandas as pd
    row = dict(obj="v_scene", im1=1, im2=2, Him=int(ref_hw[0]), Wim=int(ref_hw[1]))
    row.update({"H%d%d" % (r + 1, c + 1): float(np.asarray(H).reshape(3, 3)[r, c]) for r in range(3) for c in range(3)})
    return pd.DataFrame([row])


def reference_aepe(fn_epe, grid_gt, flow_est):
    """The statements between getGT and epe (evaluation/evalHpatch/getResults.py:221-250) around the reference's own epe: keep the
    pixels whose ground truth lies in [-1,1]^2, un-normalise, hand the (n,2) rows to epe.  -> (aepe float32 tensor, n)."""
    S = grid_gt.shape[1]
    t, e = grid_gt[0], torch.from_numpy(flow_est)
    keep = (t[..., 0] >= -1) & (t[..., 0] <= 1) & (t[..., 1] >= -1) & (t[..., 1] <= 1)
    t, e = (t + 1) * (S - 1) / 2, (e + 1) * (S - 1) / 2
    return fn_epe(e[keep], t[keep]), int(keep.sum())


@pytest.mark.reference
def test_rule_equals_the_live_reference_on_fresh_seeds():
    import ref_loader
    fh = ref_loader.script_functions("evaluation/evalHpatch/getResults.py", ["getGT", "epe"])      # both scripts are staged in full
    fk = ref_loader.script_functions("evaluation/evalKITTI/getResults.py", ["readFlow"])
    for seed in range(8):
        rng = np.random.RandomState(200 + seed)
        S = int(rng.randint(5, 40))
        ref_hw, trg_hw = tuple(int(x) for x in rng.randint(100, 900, 2)), tuple(int(x) for x in rng.randint(100, 900, 2))
        H = np.eye(3) + rng.randn(3, 3) * np.array([[0.2, 0.2, 40], [0.2, 0.2, 40], [2e-4, 2e-4, 0]])
        seat_cv2(fh["getGT"], np.empty(trg_hw + (3,), np.uint8))
        grid = fh["getGT"](reference_row(H, ref_hw), 0, S, "/nowhere")
        Hinv = assemble.hpatch_gt_homography(H, ref_hw, trg_hw, S)[1]
        gx, gy = rule_grid_gt(Hinv, S, S)
        assert tuple(grid.shape) == (1, S, S, 2) and grid.dtype == torch.float32
        assert np.array_equal(bits(gx), bits(grid[0, :, :, 0].numpy())) and np.array_equal(bits(gy), bits(grid[0, :, :, 1].numpy())), seed
        est = flow_est_for(seed, S)
        err, count = rule_epe_homography(est[None], Hinv.reshape(1, 9))
        aepe, n = reference_aepe(fh["epe"], grid, est)
        assert n == count[0]
        if n:
            # row by row: torch.norm(p=2, dim=1), the expression epe averages
            keep = ~np.isnan(err[0])
            t, e = (grid[0] + 1) * (S - 1) / 2, (torch.from_numpy(est) + 1) * (S - 1) / 2
            rows = torch.norm(t[torch.from_numpy(keep)] - e[torch.from_numpy(keep)], p=2, dim=1).numpy()
            assert np.array_equal(bits(err[0][keep]), bits(rows)), seed
            total, _ = fsum_of(err)
            exact = total / n
            assert abs(float(f32(exact)) - float(aepe)) <= abs(float(aepe) - exact) + ulp32(exact)
        else:
            assert torch.isnan(aepe)
    # readFlow: float64 arrays that float32 holds exactly
    png = np.random.RandomState(1).randint(0, 65536, (6, 7, 3)).astype(np.uint16)
    seat_cv2(fk["readFlow"], png)
    u, v, valid = fk["readFlow"]("/nowhere")
    assert u.dtype == f64 and valid.dtype == bool and np.array_equal(u.astype(f32).astype(f64), u) and np.array_equal(v.astype(f32).astype(f64), v)
    assert np.array_equal(assemble._exact_f32(u, "u").numpy(), u.astype(f32))


# ---------------------------------------------------------------- the surface

NAMES = ("rfx_epe_ws_bytes", "rfx_epe_homography_f32", "rfx_epe_flow_f32")


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
    assert len(_lib.SIGNATURES["rfx_epe_homography_f32"][1]) == 10 and len(_lib.SIGNATURES["rfx_epe_flow_f32"][1]) == 12
    # each entry's comment cites the reference lines it replaces
    assert "evaluation/evalHpatch/getResults.py:83-144" in text and "evaluation/evalKITTI/getResults.py:221-228" in text
    lib = _lib.load()
    assert lib.rfx_abi_version() == 17
    ws = lib.rfx_epe_ws_bytes
    assert ws(1, 240, 240) == 12 * 57 and ws(16, 240, 240) == 16 * 12 * 57            # ceil(57600 / 1024) = 57 tiles per map
    assert ws(1, 375, 1242) == 12 * 455
    assert ws(1, 1, 1) == 12 and ws(3, 1, TILE) == 36 and ws(3, 1, TILE + 1) == 72 and ws(9000, 2, 3) == 108000
    assert ws(0, 4, 4) == ws(4, 0, 4) == ws(4, 4, -1) == 0
    assert ws(2, 46341, 46341) == 2 * 12 * ((46341 * 46341 + TILE - 1) // TILE)       # past 2^31: size_t arithmetic


def test_argument_checks_answer_before_any_device_call():
    """Every call below carries at least one defect and returns from the entry point's opening checks; the pointers (fake, aligned
    as the entry asks) are never followed."""
    lib = _lib.load()
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(9)]
    null = ctypes.c_void_p(0)
    E_ARG, E_LIMIT = -1, -2

    def hom(flow=P[0], Hinv=P[1], N=1, Sh=6, Sw=8, total=P[2], count=P[3], err=P[4], ws=P[5]):
        return lib.rfx_epe_homography_f32(flow, Hinv, N, Sh, Sw, total, count, err, ws, null)
    for name in ("flow", "Hinv", "total", "count", "ws"):
        assert hom(**{name: null}) == E_ARG, name
        assert hom(**{name: null, "err": null}) == E_ARG, name       # err is optional, the others are not
    for bad in (dict(N=0), dict(N=-1), dict(Sh=0), dict(Sw=-3), dict(Sh=1), dict(Sw=1), dict(Sh=1, Sw=1)):
        assert hom(**bad) == E_ARG, bad
    for name in ("flow", "Hinv", "total", "ws"):                     # 8-byte reads and writes
        assert hom(**{name: ctypes.c_void_p(0x70004)}) == E_ARG, name
    assert hom(err=ctypes.c_void_p(0x50002)) == E_ARG
    assert hom(N=32768, Sh=256, Sw=256) == E_LIMIT and hom(N=2, Sh=32768, Sw=32768) == E_LIMIT
    assert hom(N=32768, Sh=256, Sw=256, ws=null) == E_ARG and hom(N=32768 * 256, Sh=256, Sw=1) == E_ARG   # a bad argument is named first

    def flo(flow=P[0], u=P[1], v=P[2], valid=P[3], N=1, H=6, W=8, total=P[4], count=P[5], err=P[6], ws=P[7]):
        return lib.rfx_epe_flow_f32(flow, u, v, valid, N, H, W, total, count, err, ws, null)
    for name in ("flow", "u", "v", "valid", "total", "count", "ws"):
        assert flo(**{name: null}) == E_ARG, name
        assert flo(**{name: null, "err": null}) == E_ARG, name
    for bad in (dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(W=-1)):
        assert flo(**bad) == E_ARG, bad
    for name in ("flow", "total", "err", "ws"):
        assert flo(**{name: ctypes.c_void_p(0x70004)}) == E_ARG, name
    assert flo(N=32768, H=256, W=256) == E_LIMIT and flo(N=1, H=65536, W=32768) == E_LIMIT
    assert flo(N=32768, H=256, W=256, valid=null) == E_ARG


def test_python_level_refusals():
    f, h = torch.zeros(6, 8, 2), torch.eye(3, dtype=torch.float64)
    for args in ((f, h), (f, h.reshape(9)), (f[None], h[None]), (f[None].repeat(3, 1, 1, 1), h.reshape(1, 9).repeat(3, 1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):   # the shapes fit: the device is what is wrong
            ops.epe_homography(*args)
    for bad in ((f, h[None]), (f[None], h), (f[None], h[None].repeat(2, 1, 1)), (torch.zeros(6, 8, 3), h), (torch.zeros(6, 8), h),
                (f, torch.zeros(3, 4, dtype=torch.float64)), (torch.zeros(1, 8, 2), h), (torch.zeros(6, 1, 2), h),
                (torch.zeros(0, 6, 8, 2), torch.zeros(0, 9, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops.epe_homography(*bad)
    u, m = torch.zeros(6, 8), torch.ones(6, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epe_flow(f, u, u, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epe_flow(f[None], u[None], u[None], m[None], want_err=True)
    for bad in ((f, u[:5], u, m), (f, u, u[:, :7], m), (f, u, u, m[None]), (f[None], u, u, m), (torch.zeros(6, 8, 3), u, u, m),
                (torch.zeros(0, 6, 8, 2), torch.zeros(0, 6, 8), torch.zeros(0, 6, 8), torch.zeros(0, 6, 8, dtype=torch.bool))):
        with pytest.raises(ValueError):
            ops.epe_flow(*bad)
    with pytest.raises(TypeError):
        ops.epe_flow(f.numpy(), u, u, m)
    # a ground truth that float32 would change is refused on the host; a missing flow needs the identity grid's size
    with pytest.raises(ValueError, match="float32 does not hold"):
        assemble.kitti_epe(f[None], np.full((6, 8), 0.1), np.zeros((6, 8)), np.ones((6, 8), bool))
    with pytest.raises(ValueError, match="float32 does not hold"):     # a float64 tensor is held to the same check as an array
        assemble.kitti_epe(f[None], torch.zeros(6, 8, dtype=torch.float64), torch.full((6, 8), 0.1, dtype=torch.float64), np.ones((6, 8), bool))
    assert assemble._exact_f32(torch.full((2, 3), 0.25, dtype=torch.float64), "u").dtype == torch.float32
    with pytest.raises(ValueError, match="needs size"):
        assemble.hpatch_epe([], np.eye(3))
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    assert getResults.hpatch.epe_from_homography is assemble.hpatch_epe and getResults.kitti.epe is assemble.kitti_epe
    assert sorted(vars(getResults.hpatch)) == ["epe_from_homography", "getFlow_all", "getFlow_onlyCoarse"]
    assert sorted(vars(getResults.kitti)) == ["epe", "getFlow_all", "getFlow_onlyCoarse"]
    # the scaled homography, on numbers one can check by hand: halving both images halves the translation
    Hs, Hinv = assemble.hpatch_gt_homography([[1, 0, 8], [0, 1, -4], [0, 0, 1]], (64, 128), (64, 128), (32, 64))
    assert np.array_equal(Hs, [[1, 0, 4], [0, 1, -2], [0, 0, 1]]) and np.array_equal(Hinv, [[1, 0, -4], [0, 1, 2], [0, 0, 1]])


def test_epe_kernels_need_no_scratch_and_a_few_words_of_lds():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {r["kernel"]: r for r in kr.table(_lib.LIB_PATH) if r["unit"] == "epe"}
    assert set(rows) == {"epe_tiles_kernel<HomographyRule>", "epe_tiles_kernel<FlowRule>", "epe_finish_kernel"}
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["waves_per_simd"] == 8, r
    # a float64 and an int32 per wavefront (tiles); 64 staged partials of each (finish)
    assert {k: r["lds"] for k, r in rows.items()} == {"epe_tiles_kernel<HomographyRule>": 48, "epe_tiles_kernel<FlowRule>": 48,
                                                      "epe_finish_kernel": 768}
    assert {k: r["wg"] for k, r in rows.items()} == {"epe_tiles_kernel<HomographyRule>": 256, "epe_tiles_kernel<FlowRule>": 256,
                                                     "epe_finish_kernel": 64}
    # the shared linspace header did not change the warp kernels: their committed rows are this build's
    lines = [l.rstrip("\n").split("\t") for l in open(os.path.join(ROOT, "profiles", "r06_kernel_resources.tsv")) if not l.startswith("#")]
    committed = {l[1]: dict(zip(kr.COLS, l)) for l in lines[1:]}
    for r in kr.table(_lib.LIB_PATH):
        if r["unit"] == "warp":
            assert all(str(r[c]) == committed[r["kernel"]][c] for c in ("vgpr", "sgpr", "lds", "scratch")), r
