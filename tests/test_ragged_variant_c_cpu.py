"""The YFCC (variant C) multi-homography driver on pairs of different sizes: what can be held without a GPU -- the C ABI surface of
rfx_keep_mask_ragged_f32, the byte-equality of torch.rot90 with PIL's right-angle rotations (the candidates of
multi_h_variant_c_pairs), the plan / geometry tables of candidates, the routing of multi_h_variant_c_pairs and the argument errors of
the list entry."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import PIL.Image as Image

from rfx import _lib, pipeline
from rfx.pipeline import AlignPipeline, ragged_plan, ragged_multih_tables, ragged_candidate_plan, ragged_variant_c_tables, scale_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keep_mask_ragged_is_declared_and_mirrored_under_abi_17():
    hdr = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"\bint\s+rfx_keep_mask_ragged_f32\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, "rfx_keep_mask_ragged_f32 is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* mask", "const float* bg", "const long long* moff", "const int32_t* geom", "const int32_t* active",
                      "int n_active", "int ldB", "int max_cells", "float* keep", "int32_t* nB_round", "void* stream"]
    res, args = _lib.SIGNATURES["rfx_keep_mask_ragged_f32"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    assert "evaluation/evalYFCC/coarseAlignFeatMatch.py:158-166" in hdr[hdr.index("rfx_keep_mask_f32 for ACTIVE"):hdr.index("int rfx_keep_mask_ragged_f32")]
    assert re.search(r"#define\s+RFX_ABI_VERSION\s+17\b", hdr) and _lib.ABI_VERSION == 17


def test_rot90_is_the_pil_right_angle_rotation_byte_for_byte():
    rng = np.random.RandomState(3)
    arr = rng.randint(0, 256, size=(37, 53, 3), dtype=np.uint8)                # odd sizes, height != width
    im = Image.fromarray(arr)
    t = torch.from_numpy(arr)
    for angle in (0, 90, 180, 270):
        ref = np.asarray(im.rotate(angle, expand=True) if angle else im, dtype=np.uint8)
        got = torch.rot90(t, angle // 90, (0, 1)).contiguous().numpy()
        assert got.shape == ref.shape == ((37, 53, 3) if angle % 180 == 0 else (53, 37, 3))
        assert np.array_equal(got, ref), angle


def test_candidate_plan_and_the_tables_of_chosen_candidates():
    scales = scale_list(3, 1.2)
    src = [(320, 240), (500, 375), (240, 336)]
    tgt = [(320, 240), (500, 375), (304, 240)]                                   # (w, h); 500x375 resizes to 320x240 at minSize 240
    cands = [tgt, [(h, w) for w, h in tgt]]                                      # candidate 1: the 90-degree turn
    plan = ragged_candidate_plan(src, cands, 240, scales, "min")
    assert (plan["K"], plan["B"], plan["nS"]) == (2, 3, 3)
    # hand-computed: the landscape target and its turn give transposed rows
    land, port = (240, 320, 15, 20, 30, 40), (320, 240, 20, 15, 40, 30)
    t0, t1 = ragged_variant_c_tables(plan, [0, 0, 0]), ragged_variant_c_tables(plan, [1, 1, 1])
    assert t0["geom"][0] == t0["geom"][1] == land and t1["geom"][0] == t1["geom"][1] == port
    assert t0["geom"][2] == (240, 304, 15, 19, 30, 38) and t1["geom"][2] == (304, 240, 19, 15, 38, 30)
    for a, b in zip(t0["geom"], t1["geom"]):
        assert (a[1], a[0], a[3], a[2], a[5], a[4]) == b
    mixed = ragged_variant_c_tables(plan, [1, 0, 1])
    assert mixed["geom"] == [port, land, (304, 240, 19, 15, 38, 30)]
    assert mixed["moff"] == [0, 320 * 240, 2 * 320 * 240] and mixed["total"] == 2 * 320 * 240 + 304 * 240
    assert plan["nB"] == [[300, 300, 285], [300, 300, 285]] and plan["ldB"] == 300
    # every image sits in exactly one bucket, sources before targets
    seen = sorted(m for mem in plan["buckets"].values() for m in mem)
    assert seen == [(b, i) for b in range(3) for i in range(5)]
    for shp, mem in plan["buckets"].items():
        assert all(plan["levels"][b][i] == shp for b, i in mem)
        kinds = [i >= 3 for _, i in mem]
        assert kinds == sorted(kinds)
    assert (240, 320) in plan["buckets"] and (320, 240) in plan["buckets"]
    # one candidate per pair: the one-target plan and its tables
    one = ragged_candidate_plan(src, [tgt], 240, scales, "min")
    ref = ragged_plan(src, tgt, 240, scales, "min")
    for key in ("levels", "cells", "nA", "offs", "ldA", "ldB", "cap", "nS", "B"):
        assert one[key] == ref[key], key
    assert one["nB"] == [ref["nB"]] and list(one["buckets"].items()) == list(ref["buckets"].items())
    assert ragged_variant_c_tables(one, [0, 0, 0]) == ragged_multih_tables(ref)


def _bare_pipe():
    pipe = AlignPipeline.__new__(AlignPipeline)                                  # no networks, no device: argument handling only
    pipe.dev, pipe.variant, pipe.minSize, pipe.scaleList = torch.device("cpu"), "C", 240, scale_list(3, 1.2)
    return pipe


def _img(w, h, seed):
    return Image.fromarray(np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8))


def test_multi_h_variant_c_pairs_routes_same_sizes_dense_and_mixed_sizes_ragged(monkeypatch):
    pipe = _bare_pipe()
    seen = []

    def fake(src, cands, **kw):
        seen.append((src, cands, kw))
        return "out"
    monkeypatch.setattr(pipe, "multi_h_variant_c", fake)
    same = [(_img(40, 24, 0), _img(32, 24, 1)), (_img(40, 24, 2), _img(32, 24, 3))]
    assert pipe.multi_h_variant_c_pairs(same, maxCoarse=2, pair_ids=[4, 5]) == "out"
    src, cands, kw = seen.pop()
    assert isinstance(src, torch.Tensor) and tuple(src.shape) == (2, 24, 40, 3) and src.dtype == torch.uint8
    assert [tuple(c.shape) for c in cands] == [(2, 24, 32, 3), (2, 32, 24, 3), (2, 24, 32, 3), (2, 32, 24, 3)]
    assert kw["maxCoarse"] == 2 and kw["pair_ids"] == [4, 5]
    for k, angle in enumerate((0, 90, 180, 270)):
        for b in range(2):
            ref = same[b][1].rotate(angle, expand=True) if angle else same[b][1]
            assert np.array_equal(cands[k][b].numpy(), np.asarray(ref))
    mixed = [same[0], (_img(40, 24, 4), _img(24, 32, 5))]                        # one target stored portrait
    pipe.multi_h_variant_c_pairs(mixed, angles=(0, 270))
    src, cands, kw = seen.pop()
    assert isinstance(src, list) and len(cands) == 2 and all(isinstance(c, list) and len(c) == 2 for c in cands)
    assert [tuple(x.shape) for x in cands[0]] == [(24, 32, 3), (32, 24, 3)] and [tuple(x.shape) for x in cands[1]] == [(32, 24, 3), (24, 32, 3)]
    assert np.array_equal(cands[1][1].numpy(), np.asarray(mixed[1][1].rotate(270, expand=True)))
    with pytest.raises(ValueError, match="multiples of 90"):
        pipe.multi_h_variant_c_pairs(same, angles=(0, 45))


def test_list_entry_refuses_what_it_cannot_run():
    pipe = _bare_pipe()
    u8 = lambda h, w: torch.zeros((h, w, 3), dtype=torch.uint8)
    src = [u8(240, 320), u8(256, 320)]
    cands = [[u8(240, 320), u8(256, 304)], [u8(320, 240), u8(304, 256)]]
    with pytest.raises(ValueError, match="same number K"):                       # a different K per pair
        pipe.multi_h_variant_c(src, [cands[0], cands[1][:1]])
    with pytest.raises(ValueError, match=r"uint8 \(H,W,3\)"):
        pipe.multi_h_variant_c(src, [[cands[0][0].float(), cands[0][1]]])
    with pytest.raises(ValueError, match="It_bg"):                               # one entry per candidate
        pipe.multi_h_variant_c(src, cands, It_bg=[None])
    with pytest.raises(ValueError, match="It_bg"):                               # one map per pair
        pipe.multi_h_variant_c(src, cands, It_bg=[[None], None])
    with pytest.raises(ValueError, match=r"It_bg\[1\]\[0\]"):                    # candidate 1 of pair 0 is 320x240 after the resize
        pipe.multi_h_variant_c(src, cands, It_bg=[None, [torch.ones(240, 320), None]])
    with pytest.raises(ValueError, match="records"):
        pipe.multi_h_variant_c(src, cands, records=object())
    with pytest.raises(ValueError, match="want_lists"):
        pipe.multi_h_variant_c(src, cands, want_lists=False)
    with pytest.raises(ValueError, match="HIP device"):                          # well-formed lists of host tensors
        pipe.multi_h_variant_c(src, cands, It_bg=[None, [torch.ones(320, 240), None]])
    with pytest.raises(ValueError, match="HIP device"):                          # same sizes: refused before anything is stacked
        pipe.multi_h_variant_c([src[0], src[0]], [[cands[0][0]] * 2])
