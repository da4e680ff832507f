"""Host side of the nearest-explained-pixel fill (csrc/fill.hip, ops.nearest_fill, assemble.interpolate_flow_match(fill="device")).

The yardstick first: the tie rule the kernels are held to -- squared distance, then the smallest column, then the smallest row; an
empty map gives (-1, 0) -- stated by brute force (rule_indices, shared with tests/test_gpu_nearest_fill.py) and checked against
scipy.ndimage.distance_transform_edt(return_indices=True), the call of evaluation/evalKITTI/getResults.py:87-93, on masks where at
least a tenth of the pixels are tied.  Then the surface: header, binding, the argument checks that answer before any HIP call, the
Python-level refusals, and the static resources of the two kernels.  Nothing is launched."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from rfx import assemble, ops, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_indices(explained):
    """(2,H,W) int32: what interpolate_flow_match indexes the flow with."""
    return ndimage.distance_transform_edt(~explained, return_distances=False, return_indices=True)


def rule_indices(explained, want_tied=False):
    """The rule by brute force: every explained pixel is a candidate of every pixel; candidates are listed by (column, row), so the
    first minimum of the exact integer distance is the smallest column, then the smallest row.  -> (2,H,W) int32[, tied (H,W) bool =
    more than one candidate at the minimum]."""
    H, W = explained.shape
    rr, cc = np.nonzero(explained)
    if rr.size == 0:
        idx = np.zeros((2, H, W), np.int32)
        idx[0] = -1
        return (idx, np.zeros((H, W), bool)) if want_tied else idx
    order = np.lexsort((rr, cc))                                   # last key first: column, then row
    rr, cc = rr[order].astype(np.int64), cc[order].astype(np.int64)
    R, X = np.mgrid[0:H, 0:W]
    d = (rr[None, None, :] - R[:, :, None]) ** 2 + (cc[None, None, :] - X[:, :, None]) ** 2
    j = d.argmin(axis=2)
    idx = np.stack([rr[j], cc[j]]).astype(np.int32)
    return (idx, (d == d.min(axis=2, keepdims=True)).sum(axis=2) > 1) if want_tied else idx


def structured_masks(H, W):
    """name -> (H,W) bool: the tie-rich families (also the GPU test's)."""
    out = {}
    m = np.zeros((H, W), bool)
    m[H // 3, :] = True
    m[:, (2 * W) // 3] = True
    m[H - 1, 0] = True
    out["row+column+point"] = m
    out["checkerboard"] = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)
    m = np.zeros((H, W), bool)
    m[H // 4, W // 4] = m[H - 1 - H // 4, W - 1 - W // 4] = True
    out["mirror pair"] = m
    m = np.zeros((H, W), bool)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
    out["four corners"] = m
    for name, (r, c) in dict(tl=(0, 0), tr=(0, W - 1), bl=(H - 1, 0), br=(H - 1, W - 1)).items():
        m = np.zeros((H, W), bool)
        m[r, c] = True
        out["corner " + name] = m
    return out


def test_tie_rule_is_scipys():
    rng = np.random.RandomState(7)
    masks = []
    for H, W in ((1, 1), (1, 17), (17, 1), (12, 19), (23, 16), (20, 20)):
        masks += [rng.rand(H, W) < p for p in (0.5, 0.2, 0.05, 0.01) for _ in range(3)]
        masks += list(structured_masks(H, W).values())
        masks.append(np.ones((H, W), bool))
    pixels = tied = 0
    for m in masks:
        want = scipy_indices(m)
        got, t = rule_indices(m, want_tied=True)
        assert got.dtype == want.dtype == np.int32 and np.array_equal(got, want), m.astype(int)
        pixels, tied = pixels + m.size, tied + int(t.sum())
    assert tied >= 0.10 * pixels, (tied, pixels)                   # the rule is exercised, not just the unique nearest pixel
    for H, W in ((1, 1), (3, 4), (9, 5)):                          # no explained pixel: (-1, 0), which numpy reads as pixel (H-1, 0)
        idx = scipy_indices(np.zeros((H, W), bool))
        assert np.array_equal(idx, rule_indices(np.zeros((H, W), bool))) and (idx[0] == -1).all() and (idx[1] == 0).all()
        v = np.arange(H * W * 2, dtype=np.float32).reshape(H, W, 2)
        assert np.array_equal(v[tuple(idx)], np.broadcast_to(v[H - 1, 0], (H, W, 2)))


def test_header_and_binding_declare_the_entry_points():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rfx_api.h")).read(), flags=re.S)
    assert int(re.search(r"#define RFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 17
    assert re.search(r"\bsize_t\s+rfx_nearest_fill_ws_bytes\s*\(\s*int\s+N\s*,\s*int\s+H\s*,\s*int\s+W\s*\)\s*;", hdr)
    args = re.search(r"\bint\s+rfx_nearest_fill_f32\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S).group(1).split(",")
    assert [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args] == _lib.SIGNATURES["rfx_nearest_fill_f32"][1]
    assert _lib.SIGNATURES["rfx_nearest_fill_f32"][0] is ctypes.c_int and len(args) == 10
    assert _lib.SIGNATURES["rfx_nearest_fill_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    lib = _lib.load()
    assert lib.rfx_abi_version() == _lib.ABI_VERSION
    assert lib.rfx_nearest_fill_ws_bytes(1, 375, 1242) == 4 * 375 * 1242 > 0
    assert lib.rfx_nearest_fill_ws_bytes(3, 8192, 8192) == 4 * 3 * 8192 * 8192          # beyond 2^31 bytes
    assert lib.rfx_nearest_fill_ws_bytes(0, 375, 1242) == 0


def test_argument_checks_answer_before_any_device_call():
    """Every refusal below returns from the entry point's first two lines; the pointers are never followed."""
    lib = _lib.load()
    P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(5)]       # values, explained, out, index, ws
    null = ctypes.c_void_p(0)

    def call(values=P[0], explained=P[1], out=P[2], index=P[3], N=1, H=16, W=16, C=2, ws=P[4]):
        return lib.rfx_nearest_fill_f32(values, explained, out, index, N, H, W, C, ws, null)
    E_ARG, E_LIMIT = -1, -2
    assert call(W=8193) == E_LIMIT and call(H=31729) == E_LIMIT
    assert call(C=9) == E_LIMIT and call(C=0) == E_ARG              # C = 0 is a non-positive size
    for k in ("values", "explained", "out", "ws"):
        assert call(**{k: null}) == E_ARG, k
    assert call(out=P[0]) == E_ARG                                  # out == values: the kernel reads other pixels while it writes
    assert call(N=0) == E_ARG and call(H=0) == E_ARG and call(W=-3) == E_ARG
    assert call(values=null, W=8193) == E_ARG                       # a bad argument is named before a limit


def test_python_level_refusals():
    with pytest.raises(RuntimeError):
        ops.nearest_fill(torch.zeros(4, 5, 2), torch.ones(4, 5, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        ops.nearest_fill(torch.zeros(1, 4, 5, 2), torch.ones(1, 4, 5, dtype=torch.bool), want_index=True)
    z = np.zeros((1, 2, 2, 2), np.float32)
    with pytest.raises(ValueError, match="fill"):                   # before anything is moved to a device ("cuda" does not exist here)
        assemble.assemble_kitti(z, z, np.eye(3, dtype=np.float32)[None], z, (16, 16), 0.5, True, fill="bogus")
    with pytest.raises(ValueError, match="fill"):
        assemble.interpolate_flow_match(torch.zeros(1, 4, 5, 2), torch.ones(1, 4, 5, dtype=torch.bool), fill="gpu")
    assert assemble.FILLS == ("host", "device")
    # the default is the host path of the reference, tensors of any device: a CPU call works and fills by scipy's indices
    f = torch.arange(40, dtype=torch.float32).reshape(1, 4, 5, 2)
    b = torch.zeros(1, 4, 5, dtype=torch.bool)
    b[0, 1, 3] = True
    assert torch.equal(assemble.interpolate_flow_match(f, b), f[:, 1:2, 3:4].expand(1, 4, 5, 2))


def test_fill_kernels_need_no_scratch_and_at_most_32k_of_lds():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {r["kernel"]: r for r in kr.table(_lib.LIB_PATH) if r["unit"] == "fill"}
    assert set(rows) == {"fill_columns_kernel", "fill_rows_kernel"}
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["lds"] <= 32 * 1024, r
        assert r["wg"] == 256 and r["waves_per_simd"] >= 2, r
    assert rows["fill_rows_kernel"]["lds"] == 4 * 8192             # the staged row at the width limit
