"""Host side of the batched KITTI flow assembly from device records (csrc/warp.hip: rfx_assemble_kitti_records_f32,
rfx_kitti_scores_records_f32; ops.assemble_kitti_records, ops.assemble_kitti_records_table, ops.assemble_kitti_records_plan;
assemble.assemble_kitti_records): the size table against hand-written layouts, the chunk plan, every refusal that answers before a
HIP call, header and binding, and the entry points' own argument checks through ctypes.  Nothing is launched: the records live on
the CPU, where an accepted call ends in the "no CPU fallback" RuntimeError."""
import ctypes
import os
import re

import pytest
import torch

from rfx import assemble, ops, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rfx_kitti_scores_records_f32", "rfx_assemble_kitti_records_f32")


def test_table_of_dense_records_by_hand():
    R = ops.MultiHRecords(2, 4, 6, "cpu", hd2=2, wd2=3)        # max_h 11: H from 4, flow from 104, 528 floats per /8 list, 132 of d2
    assert (R.off_H, R.off_flow, R.off_match, R.off_d2, R.width) == (4, 104, 632, 1160, 1292)
    rows, max_hw, total = ops.assemble_kitti_records_table(R)
    assert rows == [(0, 4, 6, 632, 1160, 2, 3, 32, 48, 0, 0, 0), (1292, 4, 6, 632, 1160, 2, 3, 32, 48, 1536, 11 * 1536, 0)]
    assert (max_hw, total) == (1536, 3072)
    rows, max_hw, total = ops.assemble_kitti_records_table(R, (27, 50), cc_th=0.01)
    assert [r[7:] for r in rows] == [(27, 50, 0, 0, 13), (27, 50, 1350, 11 * 1350, 13)] and (max_hw, total) == (1350, 2700)
    assert ops.cc_max_area(1350, 0.01) == 13
    rows, _, _ = ops.assemble_kitti_records_table(R.rows(1, 2), (1, 257), cc_th=0.5)   # a group of the batch counts from its own first
    assert rows == [(0, 4, 6, 632, 1160, 2, 3, 1, 257, 0, 0, 128)]
    R5 = ops.MultiHRecords(2, 2, 2, "cpu", max_h=5, hd2=1, wd2=1)   # 48 floats of H, 2 x 40 of /8 maps, 10 of d2: 142 -> 144 a row
    assert ops.assemble_kitti_records_table(R5)[0] == [(0, 2, 2, 92, 132, 1, 1, 16, 16, 0, 0, 0),
                                                       (144, 2, 2, 92, 132, 1, 1, 16, 16, 256, 5 * 256, 0)]


def test_table_of_ragged_records_by_hand_and_against_their_own_offsets():
    h8, w8, hd2, wd2 = [5, 4, 2], [7, 6, 2], [3, 2, 1], [4, 3, 1]
    R = ops.MultiHRecordsRagged(h8, w8, "cpu", hd2_list=hd2, wd2_list=wd2)
    assert R.width == 104 + 2 * 2 * 35 * 11 + 2 * 12 * 11 == 1908
    sizes = [(40, 56), (32, 48), (16, 16)]
    rows, max_hw, total = ops.assemble_kitti_records_table(R, cc_th=0.05)
    assert rows == [(0, 5, 7, 104 + 770, 104 + 1540, 3, 4, 40, 56, 0, 0, 112),
                    (1908, 4, 6, 104 + 528, 104 + 1056, 2, 3, 32, 48, 2240, 11 * 2240, 76),
                    (3816, 2, 2, 104 + 88, 104 + 176, 1, 1, 16, 16, 3776, 11 * 3776, 12)]
    assert (max_hw, total) == (2240, 4032)
    for b, r in enumerate(rows):
        assert (r[3], r[4]) == (R.off_match[b], R.off_d2[b]) and r[0] == b * R.width and r[5:7] == (R.hd2[b], R.wd2[b])
        assert r[4] + 2 * r[5] * r[6] * R.max_h <= R.width and r[7:9] == sizes[b]
        assert r[11] == ops.cc_max_area(r[7] * r[8], 0.05)
    rows, max_hw, total = ops.assemble_kitti_records_table(R, [(10, 11), (3, 4), (1, 257)], cc_th=0.01)
    assert [r[7:] for r in rows] == [(10, 11, 0, 0, 1), (3, 4, 110, 1210, 0), (1, 257, 122, 1342, 2)] and (max_hw, total) == (257, 379)
    sub = ops.assemble_kitti_records_table(R.rows(1, 3))[0]
    assert [r[:1] + r[9:] for r in sub] == [(0, 0, 0, 0), (1908, 1536, 11 * 1536, 0)]
    # the dense layout is the ragged one of equal sizes
    D = ops.MultiHRecords(2, 4, 6, "cpu", hd2=2, wd2=3)
    E = ops.MultiHRecordsRagged([4, 4], [6, 6], "cpu", hd2_list=[2, 2], wd2_list=[3, 3])
    assert ops.assemble_kitti_records_table(D, cc_th=0.01) == ops.assemble_kitti_records_table(E, cc_th=0.01)


def test_chunk_plan():
    R = ops.MultiHRecordsRagged([5, 4, 2, 4], [7, 6, 2, 6], "cpu", hd2_list=[3, 2, 1, 2], wd2_list=[4, 3, 1, 3])
    need = [16 * 11 * hw for hw in (2240, 1536, 256, 1536)]     # bytes of scores + filter workspace per pair
    plan = ops.assemble_kitti_records_plan
    assert plan(R, cc_th=0.01) == [(0, 4)]                      # the default holds a small batch
    assert plan(R, cc_th=0.0, ws_bytes=1) == [(0, 4)]           # no filter: no workspace, one launch
    assert plan(R, cc_th=0.01, ws_bytes=1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert plan(R, cc_th=0.01, ws_bytes=min(need) - 1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert plan(R, cc_th=0.01, ws_bytes=need[0] + need[1]) == [(0, 2), (2, 4)]
    assert plan(R, cc_th=0.01, ws_bytes=need[0] + need[1] - 1) == [(0, 1), (1, 4)]
    assert plan(R, cc_th=0.01, ws_bytes=sum(need)) == [(0, 4)] and plan(R, cc_th=0.01, ws_bytes=sum(need) - 1) == [(0, 3), (3, 4)]
    for ws in (1, 100000, 300000, 500000, 700000, 1 << 30):     # every pair once and in order, each chunk within the bound or alone
        p = plan(R, cc_th=0.01, ws_bytes=ws)
        assert p[0][0] == 0 and p[-1][1] == 4 and all(a[1] == b[0] for a, b in zip(p, p[1:])) and all(lo < hi for lo, hi in p)
        assert all(hi - lo == 1 or sum(need[lo:hi]) <= ws for lo, hi in p)
    assert plan(R, [(375, 1242)] * 4, cc_th=0.01, ws_bytes=200 << 20) == [(0, 2), (2, 4)]        # 82 MB a pair at KITTI's size
    # blockIdx.y of the score kernel is (pair, homography): at most 65535 // max_h pairs a chunk
    D = ops.MultiHRecords(7000, 1, 1, "cpu", hd2=1, wd2=1)
    assert plan(D, (1, 1)) == [(0, 5957), (5957, 7000)]
    for ws in (0, -1, 1.5, "1G", True):
        with pytest.raises(ValueError, match="ws_bytes"):
            plan(R, cc_th=0.01, ws_bytes=ws)


def test_refusals_answer_before_anything_touches_a_device():
    D = ops.MultiHRecords(2, 4, 6, "cpu", hd2=2, wd2=3)
    R = ops.MultiHRecordsRagged([4, 2], [6, 2], "cpu", hd2_list=[2, 1], wd2_list=[3, 1])
    call = lambda rec, **kw: ops.assemble_kitti_records(rec, 0.5, True, **kw)
    # records of the other drivers
    for rec in (ops.MultiHRecords(2, 4, 6, "cpu"), ops.MultiHRecordsRagged([4, 2], [6, 2], "cpu")):
        with pytest.raises(ValueError, match="use assemble_records"):
            call(rec)
        with pytest.raises(ValueError, match="use assemble_records"):
            assemble.assemble_kitti_records(rec, None, 0.5, True)
        with pytest.raises(ValueError, match="use assemble_records"):
            ops.assemble_kitti_records_table(rec)
    with pytest.raises(TypeError):
        call(D.rec)
    # ... while assemble_records keeps refusing KITTI's
    with pytest.raises(ValueError, match="KITTI"):
        ops.assemble_records(D, 0.5, True, True)
    # size lists of the wrong length or form, sizes <= 0
    for rec, out_hw in ((R, [(32, 48)]), (R, [(32, 48)] * 3), (R, (32, 48)), (R, [(32, 48), (16,)]), (D, [(32, 48), (32, 48)]),
                        (D, (32, 48, 1))):
        with pytest.raises(ValueError, match="out_hw"):
            call(rec, out_hw=out_hw)
    for rec, out_hw in ((D, (0, 32)), (D, (24, -1)), (R, [(24, 32), (0, 16)])):
        with pytest.raises(ValueError, match="positive"):
            call(rec, out_hw=out_hw)
    for cc in (-0.01, -1, float("nan")):
        with pytest.raises(ValueError, match="cc_th"):
            call(D, cc_th=cc)
    with pytest.raises(ValueError, match="ws_bytes"):
        call(D, cc_th=0.01, ws_bytes=0)
    # outputs: shapes, and a flow buffer that float2 accesses would split
    total = 2 * 32 * 48
    fg, mg, b = torch.empty((total, 2)), torch.empty(total), torch.empty(total, dtype=torch.bool)
    odd = torch.empty(2 * total + 1)[1:].view(total, 2)
    assert odd.data_ptr() % 8 == 4 and odd.is_contiguous()
    with pytest.raises(ValueError, match="8-byte aligned"):
        call(D, out=(odd, mg, b))
    for out in ((fg[:-1], mg, b), (fg, mg[:-1], b), (fg, mg, b.float()), (fg.double(), mg, b), (fg, mg.view(2, -1), b)):
        with pytest.raises(ValueError, match="out "):
            call(D, out=out)
    # ... and a call that passes all of them reaches the device check: there is no CPU path
    for kw in (dict(), dict(out_hw=(27, 50)), dict(cc_th=0.01, interpolate=True), dict(out=(fg, mg, b)), dict(cc_th=0.01, ws_bytes=1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(D, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(R, out_hw=[(27, 50), (3, 85)], cc_th=0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        assemble.assemble_kitti_records(D, (27, 50), 0.5, True, cc_th=0.01, interpolate=True)


def test_header_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "rfx_api.h")).read()
    assert int(re.search(r"#define\s+RFX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.rfx_abi_version() == 17
    head = hdr[:hdr.index("#define RFX_ABI_VERSION")]
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    want = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}
    for name, count in zip(NEW, (16, 19)):
        assert hasattr(lib, name) and name in head, name       # exported, and named among the additions under 17
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, name + " is not declared"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(params) == len(argtypes) == count
        for p, t in zip(params, argtypes):
            assert t is (ctypes.c_void_p if "*" in p else want[p.rsplit(" ", 1)[0]]), (name, p, t)
    assert callable(assemble.assemble_kitti_records) and callable(assemble.assemble_kitti)
    assert all(callable(getattr(ops, n)) for n in ("assemble_kitti_records", "assemble_kitti_records_table", "assemble_kitti_records_plan"))
    assert all(n in assemble.__doc__ for n in ("assemble_kitti_records",) + NEW)


def test_entry_points_check_their_arguments_without_a_device():
    """Every refusal answers before a HIP call: fake non-null pointers are never dereferenced."""
    lib = _lib.load()
    p, null, st = ctypes.c_void_p(4096), ctypes.c_void_p(0), ctypes.c_void_p(0)
    E_ARG, E_LIMIT = -1, -2
    # rec, rec_elems, width, max_h, off_H, off_flow, table, B, max_hw
    good = dict(rec=p, rec_elems=2 * 1292, width=1292, max_h=11, off_H=4, off_flow=104, table=p, B=2, max_hw=1536)

    def scores(multiH=1, scores=p, base=0, elems=2 * 11 * 1536, dims=p, total_px=3072, **kw):
        a = dict(good, **kw)
        return lib.rfx_kitti_scores_records_f32(a["rec"], a["rec_elems"], a["width"], a["max_h"], a["off_H"], a["off_flow"], a["table"],
                                                a["B"], a["max_hw"], multiH, scores, base, elems, dims, total_px, st)

    def merge(th=0.5, multiH=1, scores=null, base=0, elems=0, fg=p, mg=p, binary=p, total_px=3072, **kw):
        a = dict(good, **kw)
        return lib.rfx_assemble_kitti_records_f32(a["rec"], a["rec_elems"], a["width"], a["max_h"], a["off_H"], a["off_flow"],
                                                  a["table"], a["B"], a["max_hw"], th, multiH, scores, base, elems, fg, mg, binary,
                                                  total_px, st)

    for f in (scores, merge):
        for bad in (dict(rec=null), dict(table=null), dict(B=0), dict(B=-1), dict(width=0), dict(max_h=0), dict(off_H=0),
                    dict(off_flow=102), dict(off_flow=1293), dict(rec_elems=2 * 1292 - 1), dict(max_hw=0), dict(max_hw=3073),
                    dict(total_px=0), dict(base=-1)):
            assert f(**bad) == E_ARG, (f.__name__, bad)
        for bad in (dict(max_hw=1 << 31, total_px=1 << 31), dict(max_hw=1536, total_px=1 << 31),
                    dict(B=5958, rec_elems=5958 * 1292, total_px=5958 * 1536)):                     # 5958 * 11 = 65538 rows of the grid
            assert f(**bad) == E_LIMIT, (f.__name__, bad)
    for bad in (dict(scores=null), dict(dims=null), dict(elems=0), dict(elems=-5)):
        assert scores(**bad) == E_ARG, bad
    assert scores(elems=1 << 31) == E_LIMIT
    for bad in (dict(fg=null), dict(mg=null), dict(binary=null), dict(fg=ctypes.c_void_p(4100)), dict(scores=p, elems=0)):
        assert merge(**bad) == E_ARG, bad
    assert merge(scores=p, elems=1 << 31) == E_LIMIT
