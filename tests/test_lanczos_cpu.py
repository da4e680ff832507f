"""rfx/lanczos.py on the host: the coefficient tables and their integer two-pass application against Pillow itself, byte for
byte.  The device kernels (tests/test_gpu_preproc_exact.py) are then held to ``apply_numpy``, so a table error and a kernel error
show up in different tests, and a change of the host libm, of Pillow or of the tables' operation order is noticed without a GPU."""
import numpy as np
import pytest

import lanczos_cases as L
from rfx import lanczos

# Where the uint8 clamp must be hit at BOTH ends in every pass that runs.  Lanczos-3 has negative lobes: next to a 0 -> 255 step it
# under- and overshoots by several per cent of the step unless the filter is stretched over many pixels (a strong downscale averages
# the step away) -- so these are the upscales and the near-unit scales.  A one-pixel checkerboard sits at the Nyquist frequency and
# is flattened by any scale <= 1 and by the near-unit ones; only its upscales overshoot.
CLAMP_CASES = {
    "binary": [(5, 7, 333, 217), (640, 480, 641, 479), (33, 31, 32, 32), (16, 16, 15, 17), (17, 9, 17, 40), (17, 9, 40, 9)],
    "checker": [(2, 3, 64, 48), (5, 7, 333, 217), (17, 9, 17, 40), (17, 9, 40, 9)],
}


@pytest.mark.parametrize("size", L.SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_apply_numpy_equals_pillow_byte_for_byte(size):
    w, h, ow, oh = size
    for fam in L.FAMILIES:
        for c in (1, 2, 3, 4):
            img = L.image(fam, h, w, c, seed=w + ow)
            got = lanczos.apply_numpy(img, ow, oh)
            ref = L.pillow(img, ow, oh)
            assert got.dtype == np.uint8 and got.shape == (oh, ow, c)
            assert np.array_equal(got, ref), (size, fam, c, int(np.abs(got.astype(int) - ref.astype(int)).max()))
            if (w, h) == (ow, oh):
                assert got is not img and not np.shares_memory(got, img)


@pytest.mark.parametrize("family", sorted(CLAMP_CASES))
def test_both_ends_of_the_clamp_are_reached_in_each_pass(family):
    for (w, h, ow, oh) in CLAMP_CASES[family]:
        img = L.image(family, h, w, 3, seed=w + ow)
        passes = L.unclamped(img, ow, oh)
        assert set(passes) == {k for k, on in (("h", ow != w), ("v", oh != h)) if on}
        for name, v in passes.items():
            assert int(v.min()) < 0 and int(v.max()) > 255, (family, (w, h, ow, oh), name, int(v.min()), int(v.max()))
        # ... and the clamped recomputation is what apply_numpy and Pillow give
        last = np.clip(passes["v" if "v" in passes else "h"], 0, 255).astype(np.uint8)
        assert np.array_equal(last, lanczos.apply_numpy(img, ow, oh)) and np.array_equal(last, L.pillow(img, ow, oh))


def test_the_device_inputs_reach_both_ends_of_the_clamp():
    """The inputs of tests/test_gpu_preproc_exact.py: without the clamp the accumulator leaves 0..255 at both ends, in a horizontal and in a
    vertical pass, for the 0/255 and the checkerboard family and for C = 3 as well as C = 2."""
    for fam, sizes in (("binary", [(33, 31, 32, 32), (17, 9, 17, 40), (17, 9, 40, 9)]), ("checker", [(2, 3, 64, 48)])):
        for c in (2, 3):
            seen = set()
            for (w, h, ow, oh) in sizes:
                assert (w, h, ow, oh) in L.SMALL
                for name, v in L.unclamped(L.image(fam, h, w, c, seed=c), ow, oh).items():
                    if int(v.min()) < 0 and int(v.max()) > 255:
                        seen.add(name)
            assert seen == {"h", "v"}, (fam, c, seen)


def _axis_pairs():
    return sorted({(w, ow) for (w, h, ow, oh) in L.SIZES} | {(h, oh) for (w, h, ow, oh) in L.SIZES})


@pytest.mark.parametrize("pair", _axis_pairs(), ids=lambda p: "%d-%d" % p)
def test_table_invariants(pair):
    n_in, n_out = pair
    bounds, kk, ksize = lanczos.coeffs(n_in, n_out)
    assert bounds.shape == (n_out, 2) and kk.shape == (n_out, ksize) and bounds.dtype == np.int32 and kk.dtype == np.int32
    xmin, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (xmin >= 0).all() and (xmin + count <= n_in).all()
    assert (count >= 1).all() and (count <= ksize).all()
    beyond = np.arange(ksize)[None, :] >= count[:, None]
    assert not kk[beyond].any()
    # every weight is rounded to the nearest integer: the sum moves by at most 0.5 per weight
    assert (np.abs(kk.astype(np.int64).sum(1) - (1 << lanczos.PRECISION_BITS)) <= count).all()


def test_ksize_of_the_long_downscale():
    assert lanczos.coeffs(1200, 37)[2] == 197


@pytest.mark.parametrize("size", L.SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_plan_never_windows_the_rows_of_a_full_image(size):
    """For a full-image box the first output row's window starts at source row 0 and the last one's ends at the last source row,
    so the horizontal pass always runs over all rows with row_offset 0: the row-window path of rfx_lanczos_pass_u8
    (row_offset > 0) is unreachable from ops.lanczos_resize_u8 and is tested by calling the entry point directly."""
    w, h, ow, oh = size
    p = lanczos.plan(w, h, ow, oh)
    if (w, h) == (ow, oh):
        assert p is None
        return
    assert p["y_first"] == 0 and p["rows_h"] == h
    assert p["need_h"] == (ow != w) and p["need_v"] == (oh != h)
    assert int(p["bounds_v"][0, 0]) == 0 and int(p["bounds_v"][-1].sum()) == h
