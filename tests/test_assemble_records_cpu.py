"""Host side of the batched flow assembly from device records (csrc/warp.hip: rfx_assemble_records_f32; ops.assemble_records,
ops.assemble_records_table; assemble.assemble_records / assemble_yfcc_records): the size table against hand-written layouts and the
records' own offsets, every refusal that answers before a HIP call, header and binding.  Nothing is launched: the records live on
the CPU, where an accepted call ends in the "no CPU fallback" RuntimeError."""
import ctypes
import os
import re

import pytest
import torch

from rfx import assemble, ops, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_of_dense_records_by_hand():
    R = ops.MultiHRecords(3, 3, 4, "cpu")                      # max_h 11: H from 4, flow from 4 + 100, match 264 floats later
    assert (R.off_H, R.off_flow, R.off_match, R.width) == (4, 104, 368, 632)
    rows, max_hw, total = ops.assemble_records_table(R)
    assert rows == [(0, 3, 4, 368, 24, 32, 0, 0), (632, 3, 4, 368, 24, 32, 768, 0), (1264, 3, 4, 368, 24, 32, 1536, 0)]
    assert (max_hw, total) == (768, 2304)
    rows, max_hw, total = ops.assemble_records_table(R, (27, 30))
    assert [r[4:7] for r in rows] == [(27, 30, 0), (27, 30, 810), (27, 30, 1620)] and (max_hw, total) == (810, 2430)
    rows, _, _ = ops.assemble_records_table(R.rows(1, 3), (1, 257))      # a group of the batch: its rows count from its own first
    assert rows == [(0, 3, 4, 368, 1, 257, 0, 0), (632, 3, 4, 368, 1, 257, 257, 0)]
    R5 = ops.MultiHRecords(2, 2, 2, "cpu", max_h=5)            # 45 -> 48 floats of H, 2 x 40 floats of maps: 132 a row
    assert ops.assemble_records_table(R5)[0] == [(0, 2, 2, 4 + 48 + 40, 16, 16, 0, 0), (132, 2, 2, 92, 16, 16, 256, 0)]


def test_table_of_ragged_records_by_hand_and_against_their_own_offsets():
    h8, w8 = [3, 5, 2], [4, 3, 2]
    R = ops.MultiHRecordsRagged(h8, w8, "cpu")
    assert R.width == 104 + 2 * 2 * 15 * 11 == 764
    rows, max_hw, total = ops.assemble_records_table(R)
    assert rows == [(0, 3, 4, 104 + 264, 24, 32, 0, 0), (764, 5, 3, 104 + 330, 40, 24, 768, 0), (1528, 2, 2, 104 + 88, 16, 16, 1728, 0)]
    assert (max_hw, total) == (960, 1984)
    for b, r in enumerate(rows):
        assert r[3] == R.off_match[b] and r[0] == b * R.width and (r[1], r[2]) == (R.h8[b], R.w8[b])
        assert R.off_flow + 2 * r[1] * r[2] * R.max_h == r[3] and r[3] + 2 * r[1] * r[2] * R.max_h <= R.width
    rows, max_hw, total = ops.assemble_records_table(R, [(10, 11), (3, 4), (1, 257)])
    assert [r[4:7] for r in rows] == [(10, 11, 0), (3, 4, 110), (1, 257, 122)] and (max_hw, total) == (257, 379)
    sub = ops.assemble_records_table(R.rows(1, 3))[0]
    assert sub == [(0, 5, 3, 434, 40, 24, 0, 0), (764, 2, 2, 192, 16, 16, 960, 0)]
    # the dense layout is the ragged one of equal sizes
    D = ops.MultiHRecords(2, 3, 4, "cpu")
    assert ops.assemble_records_table(D) == ops.assemble_records_table(ops.MultiHRecordsRagged([3, 3], [4, 4], "cpu"))


def test_refusals_answer_before_anything_touches_a_device():
    D = ops.MultiHRecords(2, 3, 4, "cpu")
    R = ops.MultiHRecordsRagged([3, 2], [4, 2], "cpu")
    call = lambda rec, **kw: ops.assemble_records(rec, 0.5, True, kw.pop("cycle", False), **kw)
    # size lists of the wrong length or form
    for rec, out_hw in ((R, [(24, 32)]), (R, [(24, 32)] * 3), (R, (24, 32)), (R, [(24, 32), (16,)]), (D, [(24, 32), (24, 32)]),
                        (D, (24, 32, 1))):
        with pytest.raises(ValueError, match="out_hw"):
            call(rec, out_hw=out_hw)
    # output sizes <= 0
    for rec, out_hw in ((D, (0, 32)), (D, (24, -1)), (R, [(24, 32), (0, 16)])):
        with pytest.raises(ValueError, match="positive"):
            call(rec, out_hw=out_hw)
    # bg of the wrong shape, dtype or device
    ok = torch.ones((2, 24, 32), dtype=torch.bool)
    for rec, bg in ((D, ok[:1]), (D, ok[:, :, :31]), (D, [ok[0], ok[1]]), (R, [ok[0]]), (R, [ok[0], ok[1]]), (R, ok.reshape(-1))):
        with pytest.raises(ValueError, match="bg"):
            call(rec, bg=bg, cycle=True)
    with pytest.raises(ValueError, match="bool or uint8"):
        call(D, bg=ok.float())
    with pytest.raises(ValueError, match="device"):
        call(D, bg=torch.empty((2, 24, 32), dtype=torch.bool, device="meta"))
    with pytest.raises(ValueError, match="device"):
        call(R, bg=[ok[0], torch.empty((16, 16), dtype=torch.bool, device="meta")])
    # records of the KITTI driver
    for rec in (ops.MultiHRecords(2, 3, 4, "cpu", hd2=2, wd2=2), ops.MultiHRecordsRagged([3, 2], [4, 2], "cpu", hd2_list=[2, 1], wd2_list=[2, 1])):
        with pytest.raises(ValueError, match="KITTI"):
            call(rec)
        with pytest.raises(ValueError, match="KITTI"):
            assemble.assemble_yfcc_records(rec, ok, 0.5, True)
    # outputs: shapes, and a flow buffer that float2 accesses would split
    total = 2 * 24 * 32
    fg, mg, b = torch.empty((total, 2)), torch.empty(total), torch.empty(total, dtype=torch.bool)
    odd = torch.empty(2 * total + 1)[1:].view(total, 2)
    assert odd.data_ptr() % 8 == 4 and odd.is_contiguous()
    with pytest.raises(ValueError, match="8-byte aligned"):
        call(D, out=(odd, mg, b))
    for out in ((fg[:-1], mg, b), (fg, mg[:-1], b), (fg, mg, b.float()), (fg.double(), mg, b), (fg, mg.view(2, -1), b)):
        with pytest.raises(ValueError, match="out "):
            call(D, out=out)
    with pytest.raises(TypeError):
        ops.assemble_records(D.rec, 0.5, True, False)
    # ... and a call that passes all of them reaches the device check: there is no CPU path
    for kw in (dict(), dict(out_hw=(27, 30)), dict(bg=ok, cycle=True), dict(out=(fg, mg, b))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(D, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(R, bg=[ok[0], ok[0, :16, :16]], cycle=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        assemble.assemble_yfcc_records(D, ok.numpy(), 0.5, True)


def test_header_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    assert int(re.search(r"#define\s+RFX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 17
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"\bint\s+rfx_assemble_records_f32\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m, "rfx_assemble_records_f32 is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["rfx_assemble_records_f32"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == 18
    want = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}
    for p, t in zip(params, argtypes):
        assert t is (ctypes.c_void_p if "*" in p else want[p.rsplit(" ", 1)[0]]), (p, t)
    for name in ("assemble_records", "assemble_yfcc_records", "assemble", "assemble_yfcc", "assemble_kitti"):
        assert callable(getattr(assemble, name)), name
    assert callable(ops.assemble_records) and callable(ops.assemble_records_table)
    assert "assemble_records" in assemble.__doc__ and "rfx_assemble_records_f32" in assemble.__doc__
