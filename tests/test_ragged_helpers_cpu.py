"""The host helpers the drivers for pairs of different sizes share (rfx.ragged): grouping by shape, stacking and handing rows back,
the first-maximum choice of the candidate search, and the packing of per-pair background maps.  No device involved."""
import numpy as np
import pytest
import torch

from rfx import ragged


def test_by_shape_keeps_first_appearance_order_and_ascending_members():
    keys = [(3, 4), (5, 6), (3, 4), (1, 2), (5, 6), (3, 4)]
    groups = ragged.by_shape(keys)
    assert list(groups.items()) == [((3, 4), [0, 2, 5]), ((5, 6), [1, 4]), ((1, 2), [3])]
    assert list(ragged.by_shape([("src", (8, 8, 3))] * 4).items()) == [(("src", (8, 8, 3)), [0, 1, 2, 3])]     # one key: one group
    assert list(ragged.by_shape([])) == []
    assert ragged.mixed([(1, 2), (1, 2)], [(3, 4)]) is False and ragged.mixed([(1, 2), (1, 2)], [(3, 4), (4, 3)]) is True


def test_rows_returns_the_one_member_itself_and_the_cat_of_several():
    ts = [torch.arange(6.0).view(1, 2, 3) + 10 * k for k in range(4)]
    assert ragged.rows(ts, [2]) is ts[2]
    got = ragged.rows(ts, [1, 3])
    assert got.shape == (2, 2, 3) and torch.equal(got, torch.cat([ts[1], ts[3]]))
    by_key = {(0, 1): ts[0], (2, 0): ts[1]}                                     # a dict of images by (pair, level) works the same
    assert ragged.rows(by_key, [(2, 0)]) is ts[1] and torch.equal(ragged.rows(by_key, [(2, 0), (0, 1)]), torch.cat([ts[1], ts[0]]))


def test_hand_back_gives_item_mem_k_row_k_as_a_view():
    t = torch.arange(12.0).view(3, 4)
    dst = [None] * 5
    ragged.hand_back(dst, [4, 0, 2], t)
    assert dst[1] is None and dst[3] is None
    for k, m in enumerate([4, 0, 2]):
        assert dst[m].shape == (1, 4) and torch.equal(dst[m], t[k:k + 1]) and dst[m].data_ptr() == t[k].data_ptr()
    out = {}
    ragged.hand_back(out, ["a", "b"], dict(x=t[:2], y=t[1:]))
    assert set(out["b"]) == {"x", "y"} and torch.equal(out["b"]["x"], t[1:2]) and torch.equal(out["a"]["y"], t[1:2])


def test_choose_candidates_is_the_first_maximum():
    assert ragged.choose_candidates(torch.tensor([[3, 9, 4, 1], [7, 0, 2, 6]])) == [1, 0]          # a unique maximum
    assert ragged.choose_candidates(torch.tensor([[5, 8, 8, 2], [4, 4, 4, 4]])) == [1, 0]          # a tie goes to the lower index
    assert ragged.choose_candidates(torch.zeros((3, 4), dtype=torch.int32)) == [0, 0, 0]           # nothing found anywhere
    assert ragged.choose_candidates(torch.tensor([[0], [12], [3]])) == [0, 0, 0]                   # K = 1
    rng = np.random.RandomState(1)
    table = torch.from_numpy(rng.randint(0, 3, size=(50, 4)))
    assert ragged.choose_candidates(table) == [int(max(range(4), key=lambda k: (int(table[b, k]), -k))) for b in range(50)]
    assert all(isinstance(c, int) for c in ragged.choose_candidates(table))


def test_pack_bg_on_the_cpu():
    sizes = [(2, 3), (4, 2), (1, 5)]
    a, c = torch.arange(6.0).view(2, 3) / 8, torch.tensor([[1, 0, 1, 0, 1]], dtype=torch.uint8)
    bg = ragged.pack_bg([a, None, c], sizes, "cpu")
    assert bg.dtype == torch.float32 and bg.shape == (6 + 8 + 5,)
    assert torch.equal(bg[:6], a.reshape(-1)) and torch.equal(bg[6:14], torch.ones(8)) and torch.equal(bg[14:], c.float().reshape(-1))
    assert ragged.pack_bg(None, sizes, "cpu") is None
    assert ragged.pack_bg([None, None, None], sizes, "cpu") is None            # no background at all: what the kernels take as all ones
    with pytest.raises(ValueError, match="It_bg"):                              # one entry per pair
        ragged.pack_bg([a, None], sizes, "cpu")
    with pytest.raises(ValueError, match="It_bg"):                              # the target's own size
        ragged.pack_bg([a.t(), None, None], sizes, "cpu")
    with pytest.raises(ValueError, match="It_bg"):                              # the shape is checked where the rest is None too
        ragged.pack_bg([None, None, torch.ones(5, 1)], sizes, "cpu")
