"""Host-side pieces of the KITTI driver for ragged batches: the geometry tables, the record layout with a flowD2 part, the routing of
lists of images.  No GPU."""
import numpy as np
import PIL.Image as Image
import pytest
import torch

from rfx import ops
from rfx.pipeline import AlignPipeline, ragged_kitti_tables, ragged_plan, resize_img_dims, scale_list

# the five frame sizes of KITTI 2012 / 2015 (w, h)
KITTI_SIZES = [(1242, 375), (1241, 376), (1238, 374), (1226, 370), (1224, 370)]


def test_kitti_geometry_tables_on_hand_computed_sizes():
    sizes = KITTI_SIZES
    plan = ragged_plan(sizes, sizes, 800, scale_list(3, 1.2), "min")              # coarseSize 800, variant B
    t = ragged_kitti_tables(plan, sizes, 650)
    # outil.resizeImg by hand: smaller side -> 650 (325), both sides rounded to multiples of 8.  1242x375: 1242 * 650 / 375 = 2152.8
    # -> 269 * 8; 650 -> 81 * 8 = 648; half: 1242 * 325 / 375 = 1076.4 -> 135 * 8, 325 -> 41 * 8.  1241x376: 2145.3 -> 268 * 8 ...
    assert t["org"] == [(375, 1242), (376, 1241), (374, 1238), (370, 1226), (370, 1224)]
    assert t["resize"] == [(648, 2152), (648, 2144), (648, 2152), (648, 2152), (648, 2152)]
    assert t["half"] == [(328, 1080), (328, 1072), (328, 1072), (328, 1080), (328, 1072)]
    assert t["d2"] == [(41, 135), (41, 134), (41, 134), (41, 135), (41, 134)]
    # the coarse target feature map: smaller side -> 800, sides floored to multiples of 16: 2640 x 800 for all five -> 50 x 165 cells
    assert t["geom"] == [(375, 1242, 50, 165, 81, 269), (376, 1241, 50, 165, 81, 268), (374, 1238, 50, 165, 81, 269),
                         (370, 1226, 50, 165, 81, 269), (370, 1224, 50, 165, 81, 269)]
    # masks at the ORIGINAL target size, pair after pair without gaps
    assert t["moff"] == [0, 465750, 465750 + 466616, 465750 + 466616 + 463012, 465750 + 466616 + 463012 + 453620]
    assert t["total"] == t["moff"][4] + 370 * 1224
    # the sizes are the dense driver's own
    for (w, h), r, d in zip(sizes, t["resize"], t["half"]):
        assert AlignPipeline.resize_img_dims(w, h, 8, 650) == (r[1], r[0]) == resize_img_dims(w, h, 8, 650)
        assert AlignPipeline.resize_img_dims(w, h, 8, 325) == (d[1], d[0])


def test_kitti_geometry_tables_small_pairs_and_mixed_source_sizes():
    # (w, h): the test pairs of the GPU suite at coarse 160 / fine 200.  312x96: 312 * 200 / 96 = 650 -> 81.25 -> 81 * 8 = 648;
    # half: 325 -> 40.6 -> 41 * 8 = 328, 100 -> 12.5 -> 12 * 8 = 96 (round half to even) for every pair.  315x97: 649.5 -> 648; 324.7
    # -> 328.  311x94: 661.7 -> 83 * 8 = 664; 330.9 -> 328.  320x100: 640; 320.
    tgt = [(312, 96), (315, 97), (311, 94), (320, 100)]
    src = [(312, 96), (315, 97), (311, 94), (320, 104)]
    plan = ragged_plan(src, tgt, 160, scale_list(3, 1.2), "min")
    t = ragged_kitti_tables(plan, tgt, 200)
    assert t["resize"] == [(200, 648), (200, 648), (200, 664), (200, 640)]
    assert t["half"] == [(96, 328), (96, 328), (96, 328), (96, 320)]
    assert t["d2"] == [(12, 41), (12, 41), (12, 41), (12, 40)]
    assert t["geom"][0] == (96, 312, 10, 32, 25, 81) and t["geom"][1] == (97, 315, 10, 32, 25, 81)
    assert t["geom"][2] == (94, 311, 10, 33, 25, 83) and t["geom"][3] == (100, 320, 10, 32, 25, 80)
    assert t["moff"] == [0, 96 * 312, 96 * 312 + 97 * 315, 96 * 312 + 97 * 315 + 94 * 311]


def test_ragged_records_with_a_flowD2_part():
    h8, w8, hd2, wd2, max_h = [25, 25, 12], [81, 83, 17], [12, 13, 6], [41, 41, 8], 3
    R = ops.MultiHRecordsRagged(h8, w8, "cpu", max_h=max_h, hd2_list=hd2, wd2_list=wd2)
    r4 = lambda x: (x + 3) // 4 * 4
    assert R.off_H == 4 and R.off_flow == 4 + r4(9 * max_h)
    for b in range(3):
        R1 = ops.MultiHRecords(1, h8[b], w8[b], "cpu", max_h=max_h, hd2=hd2[b], wd2=wd2[b])
        # a row of one pair is the dense row
        assert (R.off_H, R.off_flow, R.off_match[b], R.off_d2[b]) == (R1.off_H, R1.off_flow, R1.off_match, R1.off_d2)
        assert R.off_d2[b] == R.off_match[b] + 2 * h8[b] * w8[b] * max_h
        assert R.width >= R1.width
        R.rec[b, 4:R1.width] = torch.arange(4, R1.width, dtype=torch.float32)
        R1.rec[0, 4:] = torch.arange(4, R1.width, dtype=torch.float32)
        v, v1 = R.views(b), R1.views()
        assert len(v) == 6 and all(torch.equal(x, y[0]) for x, y in zip(v, v1))
        assert tuple(v[5].shape) == (max_h, 2, hd2[b], wd2[b])
    assert R.width == max(ops.MultiHRecords(1, a, b, "cpu", max_h=max_h, hd2=c, wd2=d).width for a, b, c, d in zip(h8, w8, hd2, wd2))
    assert R.rec[:, 1].tolist() == [1, 1, 1] and R.rec[:, 2].tolist() == h8 and R.rec[:, 3].tolist() == w8
    assert R.d2dims.tolist() == [list(x) for x in zip(hd2, wd2)] and R.d2dims.dtype == torch.int32
    sub = R.rows(1, 3)
    assert (sub.B, sub.h8, sub.hd2, sub.wd2, sub.off_d2) == (2, h8[1:], hd2[1:], wd2[1:], R.off_d2[1:])
    assert sub.rec.data_ptr() == R.rec[1:].data_ptr() and sub.d2dims.tolist() == R.d2dims[1:].tolist()
    assert torch.equal(sub.views(0)[5], R.views(1)[5])
    same = ops.MultiHRecords.ragged(h8, w8, "cpu", max_h=max_h, hd2_list=hd2, wd2_list=wd2)
    assert (same.width, same.off_d2) == (R.width, R.off_d2)
    for bad in (dict(hd2_list=hd2), dict(wd2_list=wd2), dict(hd2_list=hd2[:2], wd2_list=wd2[:2])):
        with pytest.raises(ValueError):
            ops.MultiHRecordsRagged(h8, w8, "cpu", max_h=max_h, **bad)


def test_ragged_records_without_d2_lists_keep_their_layout():
    h8, w8, max_h = [30, 32, 12], [40, 40, 17], 11
    R = ops.MultiHRecordsRagged(h8, w8, "cpu", max_h=max_h)
    # the layout of the records before they could hold flowD2: header 4, H slots padded to 4, two /8 parts of the pair's own size
    assert R.off_H == 4 and R.off_flow == 104
    assert R.off_match == [104 + 2 * a * b * max_h for a, b in zip(h8, w8)]
    assert R.width == 104 + 4 * 32 * 40 * max_h and tuple(R.rec.shape) == (3, R.width)
    assert R.hd2 is None and R.off_d2 is None and len(R.views(0)) == 5
    assert tuple(R.views(2)[4].shape) == (max_h, 2, 12, 17)
    sub = R.rows(0, 2)
    assert sub.hd2 is None and len(sub.views(1)) == 5


def test_cc_dims_table_uses_each_maps_own_size():
    rows = ops.cc_dims_table([(96, 136), (50, 70), (7, 9)], 0.01)
    assert rows == [(96, 136, 130), (50, 70, 35), (7, 9, 0)]
    assert [r[2] for r in rows] == [ops.cc_max_area(h * w, 0.01) for h, w, _ in rows]


def _bare_pipe():
    pipe = object.__new__(AlignPipeline)                 # no networks: only the routing is exercised
    pipe.dev = torch.device("cpu")
    return pipe


def test_multi_h_kitti_pairs_routing(monkeypatch):
    pipe = _bare_pipe()
    seen = {}

    def batched(src, tgt, **kw):
        seen.update(src=src, tgt=tgt, kw=kw)
        return "out"
    monkeypatch.setattr(pipe, "multi_h_kitti_batched", batched, raising=False)
    im = lambda w, h, v: Image.fromarray(np.full((h, w, 3), v, dtype=np.uint8))
    same = [(im(312, 96, 1), im(312, 96, 2)), (im(312, 96, 3), im(312, 96, 4))]
    assert pipe.multi_h_kitti_pairs(same, fineSize=200, pair_ids=[5, 6]) == "out"
    assert isinstance(seen["src"], torch.Tensor) and tuple(seen["src"].shape) == (2, 96, 312, 3) and tuple(seen["tgt"].shape) == (2, 96, 312, 3)
    assert seen["kw"]["fineSize"] == 200 and seen["kw"]["pair_ids"] == [5, 6] and seen["kw"]["cc_th"] == 0.01
    mixed = [(im(312, 96, 1), im(312, 96, 2)), (im(311, 94, 3), im(311, 94, 4)), (im(320, 104, 5), im(320, 100, 6))]
    pipe.multi_h_kitti_pairs(mixed, records="R", split=2)
    assert isinstance(seen["src"], list) and [tuple(x.shape) for x in seen["src"]] == [(96, 312, 3), (94, 311, 3), (104, 320, 3)]
    assert [tuple(x.shape) for x in seen["tgt"]] == [(96, 312, 3), (94, 311, 3), (100, 320, 3)] and seen["tgt"][2].dtype == torch.uint8
    assert int(seen["tgt"][2][0, 0, 0]) == 6 and seen["kw"]["records"] == "R" and seen["kw"]["split"] == 2


def test_multi_h_kitti_batched_routes_lists(monkeypatch):
    pipe = _bare_pipe()
    calls = []

    class Dense(Exception):
        pass

    def prepare_device(src, tgt):
        calls.append(("dense", tuple(src.shape), tuple(tgt.shape)))
        raise Dense()
    monkeypatch.setattr(pipe, "prepare_device", prepare_device, raising=False)
    monkeypatch.setattr(pipe, "_multi_h_kitti_batched_ragged", lambda src, tgt, *a: calls.append(("ragged", [tuple(x.shape) for x in src],
                                                                                                 [tuple(x.shape) for x in tgt])) or "r",
                        raising=False)
    u8 = lambda h, w: torch.zeros((h, w, 3), dtype=torch.uint8)
    with pytest.raises(Dense):                           # one shape per side, (H,W,3) and (1,H,W,3) entries mixed: stacked, the dense path
        pipe.multi_h_kitti_batched([u8(96, 312), u8(96, 312)[None]], [u8(90, 300)[None], u8(90, 300)])
    assert calls == [("dense", (2, 96, 312, 3), (2, 90, 300, 3))]
    assert pipe.multi_h_kitti_batched([u8(96, 312), u8(96, 312)], [u8(96, 312)[None], u8(94, 311)]) == "r"     # targets differ
    assert calls[-1] == ("ragged", [(96, 312, 3), (96, 312, 3)], [(96, 312, 3), (94, 311, 3)])
    assert pipe.multi_h_kitti_batched([u8(96, 312), u8(97, 315)], [u8(96, 312), u8(96, 312)]) == "r"           # sources differ
    with pytest.raises(ValueError):
        pipe.multi_h_kitti_batched([u8(96, 312)], [u8(96, 312), u8(94, 311)])
