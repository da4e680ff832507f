"""The bucket / offset plan of a ragged batch (rfx.pipeline.ragged_plan), a pure function of the image sizes: no GPU."""
from rfx.pipeline import ragged_plan, resize_dims, scale_list

SRC = [(640, 480), (480, 640), (384, 512), (640, 480), (800, 600), (517, 389)]
TGT = [(640, 480), (480, 640), (512, 384), (600, 450), (800, 600), (389, 517)]


def _plan(mode="max", min_size=480, nb_scale=7):
    return ragged_plan(SRC, TGT, min_size, scale_list(nb_scale, 1.2), mode), scale_list(nb_scale, 1.2)


def test_level_shapes_are_resize_dims():
    for mode in ("max", "min"):
        plan, scales = _plan(mode)
        nS = len(scales)
        for b, ((sw, sh), (tw, th)) in enumerate(zip(SRC, TGT)):
            for i, s in enumerate(scales):
                nw, nh = resize_dims(sw, sh, int(480 * s), mode)
                assert plan["levels"][b][i] == (nh, nw)
                assert plan["cells"][b][i] == (nh // 16, nw // 16)
            nw, nh = resize_dims(tw, th, 480, mode)
            assert plan["levels"][b][nS] == (nh, nw)
            assert plan["nB"][b] == (nh // 16) * (nw // 16)


def test_equal_shapes_share_one_bucket_and_every_image_is_in_one():
    plan, scales = _plan()
    nS = len(scales)
    seen = []
    for shp, mem in plan["buckets"].items():
        assert mem, shp
        for b, i in mem:
            assert plan["levels"][b][i] == shp
        seen += mem
        # sources first, then targets (one scatter per destination)
        kinds = [i == nS for _, i in mem]
        assert kinds == sorted(kinds)
    assert sorted(seen) == sorted((b, i) for b in range(len(SRC)) for i in range(nS + 1))
    assert len(set(plan["buckets"])) == len(plan["buckets"])
    # pairs 0 and 3 have one source size: all their levels ride in the same buckets
    for i in range(nS):
        assert any((0, i) in m and (3, i) in m for m in plan["buckets"].values())
    assert len(plan["buckets"]) < len(SRC) * (nS + 1)


def test_offsets_tile_each_pair_without_overlap_and_ld_is_padded():
    plan, scales = _plan()
    for b in range(len(SRC)):
        spans = sorted((plan["offs"][b][i], r * c) for i, (r, c) in enumerate(plan["cells"][b][:len(scales)]))
        pos = 0
        for off, n in spans:
            assert off == pos and n > 0
            pos += n
        assert pos == plan["nA"][b]
    assert plan["ldA"] % 4 == 0 and max(plan["nA"]) <= plan["ldA"] < max(plan["nA"]) + 4
    assert plan["ldB"] % 4 == 0 and max(plan["nB"]) <= plan["ldB"] < max(plan["nB"]) + 4
    assert plan["cap"] == max(min(a, b) for a, b in zip(plan["nA"], plan["nB"]))
    assert plan["B"] == len(SRC)
