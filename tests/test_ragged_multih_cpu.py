"""The host-side layouts of the ragged multi-homography path, pure functions of the size lists: the ragged result records
(rfx.ops.MultiHRecordsRagged) and the packed-mask offset / geometry tables (rfx.pipeline.ragged_multih_tables).  No GPU."""
import torch

from rfx.ops import MultiHRecords, MultiHRecordsRagged
from rfx.pipeline import ragged_plan, ragged_multih_tables, scale_list

H8 = [30, 30, 40, 7]
W8 = [40, 36, 30, 9]


def test_ragged_records_layout_is_a_function_of_the_sizes():
    max_h = 5
    R = MultiHRecords.ragged(H8, W8, "cpu", max_h=max_h)
    assert isinstance(R, MultiHRecordsRagged) and R.B == 4 and R.rec.shape == (4, R.width) and R.rec.dtype == torch.float32
    assert R.off_H == 4 and R.off_flow == 4 + (9 * max_h + 3) // 4 * 4
    big = max(a * b for a, b in zip(H8, W8))
    assert R.width % 4 == 0 and R.off_flow + 4 * big * max_h <= R.width < R.off_flow + 4 * big * max_h + 4
    for b, (h8, w8) in enumerate(zip(H8, W8)):
        assert R.off_match[b] == R.off_flow + 2 * h8 * w8 * max_h and R.off_match[b] + 2 * h8 * w8 * max_h <= R.width
        nb, status, RH, Rf, Rm = R.views(b)
        assert RH.shape == (max_h, 3, 3) and Rf.shape == (max_h, 2, h8, w8) and Rm.shape == (max_h, 2, h8, w8)
        assert float(nb) == 0 and float(status) == 1 and R.rec[b, 2:4].tolist() == [h8, w8]
        # the views alias the row: header | H | flowDown8 | matchDown8, in this order, without overlap
        base = R.rec[b].data_ptr()
        offs = [(v.data_ptr() - base) // 4 for v in (RH, Rf, Rm)]
        assert offs == [R.off_H, R.off_flow, R.off_match[b]]
    # a lock-step group: rows [1, 3) over the same storage
    sub = R.rows(1, 3)
    assert sub.B == 2 and sub.h8 == H8[1:3] and sub.off_match == R.off_match[1:3] and sub.width == R.width
    sub.views(0)[2][1, 0, 0] = 7.0
    assert float(R.views(1)[2][1, 0, 0]) == 7.0 and sub.rec.data_ptr() == R.rec[1].data_ptr()


def test_ragged_record_of_one_pair_is_the_dense_record():
    h8, w8, max_h = 12, 17, 3
    Rr, Rd = MultiHRecords.ragged([h8], [w8], "cpu", max_h=max_h), MultiHRecords(1, h8, w8, "cpu", max_h=max_h)
    assert (Rr.off_H, Rr.off_flow, Rr.off_match[0], Rr.width) == (Rd.off_H, Rd.off_flow, Rd.off_match, Rd.width)
    # the same numbers written through the views land in the same floats of the row
    g = torch.Generator().manual_seed(1)
    vals = [torch.randn(max_h, 3, 3, generator=g), torch.randn(max_h, 2, h8, w8, generator=g), torch.randn(max_h, 2, h8, w8, generator=g)]
    for dst, v in zip(Rr.views(0)[2:], vals):
        dst.copy_(v)
    for dst, v in zip(Rd.views()[2:5], vals):
        dst[0].copy_(v)
    assert torch.equal(Rr.rec[0, 4:], Rd.rec[0, 4:]) and torch.equal(Rr.rec[0, :2], Rd.rec[0, :2])
    assert Rr.rec[0, 2:4].tolist() == [h8, w8] and Rd.rec[0, 2:4].tolist() == [0, 0]      # the dense header leaves [2], [3] unused


SRC = [(640, 480), (480, 640), (384, 512), (640, 480), (800, 600), (517, 389)]
TGT = [(640, 480), (480, 640), (512, 384), (600, 450), (800, 500), (389, 517)]


def test_packed_mask_tables_of_a_plan():
    for mode in ("max", "min"):
        plan = ragged_plan(SRC, TGT, 480, scale_list(7, 1.2), mode)
        t = ragged_multih_tables(plan)
        nS = plan["nS"]
        assert len(t["moff"]) == len(t["geom"]) == plan["B"]
        pos = 0
        for b, (off, (h, w, rt, ct, h8, w8)) in enumerate(zip(t["moff"], t["geom"])):
            assert off == pos                                   # monotone, disjoint, no gaps (the kernels use scalar loads: no alignment needed)
            assert (h, w) == plan["levels"][b][nS] and (rt, ct) == plan["cells"][b][nS]
            assert (h8, w8) == (h // 8, w // 8) and h % 16 == 0 and w % 16 == 0 and (rt, ct) == (h // 16, w // 16)
            pos += h * w
        assert t["total"] == pos
        assert len({g[:2] for g in t["geom"]}) >= 3
