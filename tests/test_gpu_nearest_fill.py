"""The nearest-explained-pixel fill on the device (csrc/fill.hip: rfx_nearest_fill_f32, ops.nearest_fill) against the call it
replaces, scipy.ndimage.distance_transform_edt(~explained, return_indices=True) of evaluation/evalKITTI/getResults.py:87-93:
the indices are held to scipy's index for index -- ties (13-16 % of the pixels of a typical mask) and the empty map included --,
the values to a bit-exact gather by those indices, and assemble_kitti(fill="device") to torch.equal with fill="host".
Integer work: no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

from rfx import assemble, ops, synth
from test_nearest_fill_cpu import scipy_indices, structured_masks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fill(values, masks, dev, want_index=True):
    return ops.nearest_fill(torch.from_numpy(values).to(dev), torch.from_numpy(masks).to(dev), want_index=want_index)


def _gather(values, masks, idx):
    """values[n, idx0, idx1] as 32-bit words: what interpolate_flow_match computes on the host (a row of -1 wraps to H-1)."""
    bits = values.view(np.int32)
    return np.stack([bits[n][idx[n, 0], idx[n, 1]] for n in range(len(masks))])


def _check(values, masks, dev, what):
    """One batch: indices equal to scipy's per map, out a bit-exact gather by them, explained pixels untouched."""
    out, idx = _fill(values, masks, dev)
    out, idx = out.cpu().numpy(), idx.cpu().numpy()
    want = np.stack([scipy_indices(m) for m in masks])
    assert idx.dtype == np.int32 and idx.shape == want.shape
    bad = np.argwhere(idx != want)
    assert bad.size == 0, "%s: %d indices differ from scipy's, first at (n, plane, r, x) = %s: %d, scipy %d" % (
        what, len(bad), tuple(bad[0]), idx[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(out.view(np.int32), _gather(values, masks, want)), what
    assert np.array_equal(out.view(np.int32)[masks], values.view(np.int32)[masks]), what
    return out, idx


def test_every_mask_of_a_3x4_map_in_one_batch(dev):
    """All 4096 masks of a 3 x 4 map as ONE batch, the empty one (map 0) included: a wrong tie, a wrong batch offset or a wrong
    empty-map answer has nowhere to hide.  12288 rows: the row pass walks past its grid cap."""
    bits = (np.arange(4096)[:, None] >> np.arange(12)[None, :]) & 1
    masks = bits.reshape(4096, 3, 4).astype(bool)
    values = np.random.RandomState(0).randn(4096, 3, 4, 2).astype(np.float32)
    _, idx = _check(values, masks, dev, "3x4 exhaustive")
    assert (idx[0, 0] == -1).all() and (idx[0, 1] == 0).all() and not masks[0].any()


def _family(H, W, seed):
    rng = np.random.RandomState(seed)
    fam = {"density %g" % p: rng.rand(H, W) < p for p in (0.5, 0.05, 0.001)}
    fam.update(structured_masks(H, W))
    fam["all explained"] = np.ones((H, W), bool)
    return fam


# 96 x 312: the suite's KITTI test size; 3 x 2100: wider than a workgroup's segment (9 segments of one staged row)
@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1), (37, 53), (64, 64), (65, 129), (96, 312), (3, 2100)])
def test_seeded_families_equal_scipy_everywhere(dev, H, W):
    fam = _family(H, W, 1000 * H + W)
    masks = np.stack(list(fam.values()))                            # one batch, a different mask per map
    values = np.random.RandomState(H + W).randn(len(masks), H, W, 2).astype(np.float32)
    out, idx = _check(values, masks, dev, "%dx%d batch of %s" % (H, W, list(fam)))
    k = list(fam).index("all explained")
    assert np.array_equal(out[k].view(np.int32), values[k].view(np.int32))
    # three maps of the batch on their own, in the (H,W,C) / (H,W) form: map n of a batch is the single call
    for name in ("density 0.05", "row+column+point", "checkerboard"):
        n = list(fam).index(name)
        o1, i1 = _fill(values[n], masks[n], dev)
        assert tuple(o1.shape) == (H, W, 2) and tuple(i1.shape) == (2, H, W)
        assert np.array_equal(i1.cpu().numpy(), idx[n]) and np.array_equal(o1.cpu().numpy().view(np.int32), out[n].view(np.int32)), name
    o2 = _fill(values[:3], masks[:3], dev, want_index=False)        # without the index output
    assert isinstance(o2, torch.Tensor) and np.array_equal(o2.cpu().numpy().view(np.int32), out[:3].view(np.int32))


def test_beyond_the_launch_cap(dev):
    """N*H*W = 2 099 200 > 8192 x 256, 8200 row segments > the row pass's 8192 workgroups."""
    masks = np.random.RandomState(5).rand(2, 1025, 1024) < 0.1
    values = np.random.RandomState(6).randn(2, 1025, 1024, 1).astype(np.float32)
    _check(values, masks, dev, "2x1025x1024")


def test_column_pass_beyond_its_launch_cap(dev):
    """N*W = 2 097 300 columns > 8192 x 256 threads: the column pass strides its grid.  Every map is one of the 256 masks of a
    2 x 4 map, so scipy is asked 256 times, not N times."""
    N = (1 << 19) + 37
    which = np.random.RandomState(8).randint(0, 256, N)
    table = ((np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1).reshape(256, 2, 4).astype(bool)
    want = np.stack([scipy_indices(m) for m in table])[which]
    masks = table[which]
    values = np.arange(N * 8, dtype=np.float32).reshape(N, 2, 4, 1)          # every pixel of the batch its own value (< 2^24)
    out, idx = _fill(values, masks, dev)
    assert np.array_equal(idx.cpu().numpy(), want)
    src = (np.arange(N)[:, None, None] * 2 + want[:, 0] % 2) * 4 + want[:, 1]   # % 2: the row -1 of an empty map is row H-1
    assert np.array_equal(out.cpu().numpy()[..., 0], src.astype(np.float32))


@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_values_move_bit_for_bit(dev, C):
    H, W = 37, 53
    rng = np.random.RandomState(40 + C)
    masks = np.stack([rng.rand(H, W) < 0.05, np.zeros((H, W), bool), structured_masks(H, W)["row+column+point"],
                      rng.rand(H, W) < 0.5])
    values = rng.randn(len(masks), H, W, C).astype(np.float32)
    bits = values.view(np.int32)
    special = np.array([0x7fc12345, 0x7f800001, -0x3fedcb, 0x7f800000, -0x800000, -0x80000000], np.int64).astype(np.int32)
    assert np.isnan(special[:3].view(np.float32)).all() and np.isinf(special[3:5].view(np.float32)).all()   # NaNs with payloads, +-inf, -0.0
    for n in (0, 2, 3):                                             # planted at explained pixels: they spread to their neighbours
        rr, cc = np.nonzero(masks[n])
        for j in range(len(special) * 2):
            bits[n, rr[j * 3 % len(rr)], cc[j * 3 % len(rr)], j % C] = special[j % len(special)]
    bits[1, H - 1, 0, :] = special[np.arange(C) % len(special)]     # the empty map reads pixel (H-1, 0) ...
    assert not np.array_equal(bits[1, H - 1, 0], bits[1, 0, 0])     # ... which is not pixel (0, 0)
    out, idx = _check(values, masks, dev, "C = %d" % C)
    assert np.array_equal(out.view(np.int32)[1], np.broadcast_to(bits[1, H - 1, 0], (H, W, C)))
    for s in special:
        assert (out.view(np.int32) == s).sum() > (bits == s).sum()  # each special value reached pixels beyond its own
    with pytest.raises(RuntimeError):
        _fill(np.zeros((1, 4, 4, 9), np.float32), np.ones((1, 4, 4), bool), dev)          # C above the limit
    with pytest.raises(RuntimeError):
        _fill(values, masks[:, :-1], dev)                           # shapes that do not belong together


def _kitti_both(args, dev):
    host = assemble.assemble_kitti(*args, device=dev, fill="host")
    device = assemble.assemble_kitti(*args, device=dev, fill="device")
    for h, d, what in zip(host, device, ("flow", "match", "binary")):
        assert h.dtype == d.dtype and h.shape == d.shape and h.device == d.device and torch.equal(h, d), what
    return host


def test_assemble_kitti_device_fill_equals_host_fill(dev):
    """Both paths share every device step before the fill, so the results are equal, not close."""
    g = np.load(os.path.join(GOLD, "assemble.npz"))
    n, hd, wd = int(g["n"]), int(g["hd"]), int(g["wd"])
    fd, fd2, pm, md = synth.assembly_arrays(int(g["seed"]), n, hd, wd)
    for tag in "cd":
        th, cc, interp, multiH = g["kitti_%s_cfg" % tag]
        # (configuration c explains every pixel of its 80 x 112 map: there the fill has to be the identity)
        _kitti_both((fd2, fd, pm, md, (hd * 8, wd * 8), float(th), bool(multiH), float(cc), True), dev)
    n, hd, wd = 11, 60, 80                                          # the 480 x 640 case of the full-size property test
    fd, fd2, pm, md = synth.assembly_arrays(31, n, hd, wd)
    fg, _, b = _kitti_both((fd2, fd, pm, md, (480, 640), 0.5, True, 0.0, True), dev)
    assert bool(b.any()) and not bool(b.all())
    # nothing explained at all (no score reaches 2.0): both paths read pixel (H-1, 0)
    fg, _, b = _kitti_both((fd2, fd, pm, md, (480, 640), 2.0, True, 0.0, True), dev)
    assert not bool(b.any()) and torch.equal(fg, fg[:, -1:, :1].expand_as(fg))
    calls = []
    real = ops.nearest_fill
    ops.nearest_fill = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        assemble.assemble_kitti(fd2, fd, pm, md, (480, 640), 0.5, True, 0.0, True, dev)                    # the default is "host"
        assert not calls
        assemble.assemble_kitti(fd2, fd, pm, md, (480, 640), 0.5, True, 0.0, True, dev, fill="device")
        assert len(calls) == 1
    finally:
        ops.nearest_fill = real


def test_dropin_reads_the_fill_switch(dev, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd", "dropin"))
    import getResults
    n, hd, wd = 3, 8, 10
    fd, fd2, pm, md = synth.assembly_arrays(41, n, hd, wd)
    np.save(tmp_path / "Homograpy_3_3.npy", pm)
    np.save(tmp_path / "Finetune_D2_3_3.npy", fd2)
    np.save(tmp_path / "Finetune_3_3.npy", fd)
    np.save(tmp_path / "Finetune_Mask_3_3.npy", md)
    grid_org = torch.zeros(1, hd * 8, wd * 8, 2)
    args = (3, str(tmp_path), 3, "Finetune", None, True, grid_org, 0.25, 0.01, True)
    calls = []
    real = ops.nearest_fill
    monkeypatch.setattr(ops, "nearest_fill", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.delenv("RFX_KITTI_FILL", raising=False)
    plain = getResults.kitti.getFlow_all(*args)
    assert not calls and plain.device.type == "cpu" and tuple(plain.shape) == (1, hd * 8, wd * 8, 2)
    monkeypatch.setenv("RFX_KITTI_FILL", "host")
    assert torch.equal(getResults.kitti.getFlow_all(*args), plain) and not calls
    monkeypatch.setenv("RFX_KITTI_FILL", "device")
    on_device = getResults.kitti.getFlow_all(*args)
    assert len(calls) == 1 and on_device.device.type == "cpu" and torch.equal(on_device, plain)
    monkeypatch.setenv("RFX_KITTI_FILL", "gpu")
    with pytest.raises(ValueError, match="fill"):
        getResults.kitti.getFlow_all(*args)
