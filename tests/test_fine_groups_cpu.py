"""Host-side pieces of the grouped fine stage that need no device: the ABI revision and the rfx_group_stats prototype, the packed
layout of AlignPipeline.pred_flow_mask_groups, and the RFX_FINE_GROUPS switch."""
import ctypes
import os
import re

import pytest

from rfx import _lib, ops
from rfx.pipeline import packed_group_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_16_and_group_stats_prototype():
    hdr = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    assert int(re.search(r"#define RFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 17
    assert re.search(r"int rfx_group_stats\(long long\* groups, long long\* launches\);", hdr)
    assert _lib.SIGNATURES["rfx_group_stats"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])


def test_packed_group_offsets_of_the_test_shapes():
    # (B, h, w) of tests/test_gpu_fine_groups.py: 48x64 (B=2), 64x80 (B=1), 80x48 (B=1), 56x72 (B=3)
    lay = packed_group_offsets([(2, 48, 64), (1, 64, 80), (1, 80, 48), (3, 56, 72)])
    assert lay["off"] == [0, 6144, 11264, 15104] and lay["total"] == 15104 + 3 * 56 * 72
    assert lay["off8"] == [0, 96, 176, 236] and lay["total8"] == 236 + 3 * 7 * 9
    assert lay["shapes"] == [(2, 48, 64, 6, 8), (1, 64, 80, 8, 10), (1, 80, 48, 10, 6), (3, 56, 72, 7, 9)]
    # groups stay in the order given, and a pair's maps follow each other inside its group: pair j of group g sits at
    # off[g] + j * h * w -- the per-pair offsets rounds.RaggedGroup.matches lays out (fine-group order, members ascending)
    per_pair, t = [], 0
    for B, h, w, _, _ in lay["shapes"]:
        for _ in range(B):
            per_pair.append(t)
            t += h * w
    assert [lay["off"][g] + j * s[1] * s[2] for g, s in enumerate(lay["shapes"]) for j in range(s[0])] == per_pair
    # explicit /8 sizes (feature maps that are not h // 8) and more than 8 groups (the library chunks the launches, not the layout)
    assert packed_group_offsets([(1, 20, 30, 3, 4), (2, 8, 8, 1, 1)])["off8"] == [0, 12]
    many = packed_group_offsets([(1, 8 * (k + 1), 16) for k in range(11)])
    assert many["off"] == [sum(8 * (j + 1) * 16 for j in range(k)) for k in range(11)] and len(many["off8"]) == 11
    with pytest.raises(ValueError):
        packed_group_offsets([(0, 8, 8)])


def test_rfx_fine_groups_parsing():
    assert ops.fine_groups_enabled({"RFX_FINE_GROUPS": "1"}) is True
    assert ops.fine_groups_enabled({"RFX_FINE_GROUPS": "0"}) is False
    assert ops.fine_groups_enabled({"RFX_FINE_GROUPS": " 0 "}) is False
    assert ops.fine_groups_enabled({}) is ops.FINE_GROUPS_DEFAULT
    assert ops.fine_groups_enabled({"RFX_FINE_GROUPS": ""}) is ops.FINE_GROUPS_DEFAULT
