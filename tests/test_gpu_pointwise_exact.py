"""The gather / stencil kernels of csrc/warp.hip, csrc/pool.hip and csrc/seg.hip against float64, at their edges.

The idea is tests/test_gpu_conv_exact.py's.  Tier 1: operands are drawn from families in which every value a kernel can form
(coordinate, weight, product, partial sum) is a multiple of one quantum and stays below 2^24 quanta, so float32 arithmetic is
exact and a correct kernel returns the float64 result BIT FOR BIT whatever its operation order or fma contraction; a misrouted
tap / corner / channel / image, a wrong weight or border rule, or a stale index on a later grid-stride trip (grids are capped at
8192 x 256 = 2^21 threads) is a bit difference.  Every family checks its own invariant on the host before it is trusted: the
float64 reference is representable in float32 and ATen's float32 kernel returns the same bits (``_exact`` below; the unmarked
``test_family_invariants_hold_on_the_host`` runs all of it without a device).  Tier 2: where exactness cannot hold (arbitrary
grids, non-dyadic resizes, projective grids, exp) the bound is derived from the count of roundings, stated in the test's docstring
and computed from the test's own inputs.  Tier 3: index images with integral coordinates against pure numpy indexing, for the
kernels that gather or move data (the reductions -- l2norm, softmax_accum, argmax_mask -- are routed by their Tier 1 / 2 data).

References are plain float64 torch / numpy written here.  u = 2^-24 is the unit round-off of float32."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rfx import ops

gpu = pytest.mark.gpu
U = 2.0 ** -24
CAP = 8192 * 256
F64 = torch.float64


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _ints(g, shape, lo, hi, q=1.0):
    """multiples of q in [lo*q, hi*q]"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float() * q


def _exact(ref64, aten32=None, what=""):
    """The family's invariant: the float64 result is a float32 number, and (where given) ATen's float32 kernel returns its bits."""
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64), "family not exact: float64 reference is not representable in float32 " + what
    if aten32 is not None:
        assert torch.equal(aten32, ref32), "family not exact: ATen float32 differs from float64 " + what
    return ref32


def _same(a, b):
    """torch.equal that also holds NaN == NaN (payloads aside)."""
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape or not torch.equal(a.isnan(), b.isnan()):
        return False
    z = torch.zeros((), dtype=a.dtype)
    return torch.equal(torch.where(a.isnan(), z, a), torch.where(b.isnan(), z, b))


def _where_bad(got, ref):
    d = (got.cpu() != ref.cpu()).nonzero()
    return "%d mismatches, first at %s" % (d.shape[0], d[:4].tolist())


# ====================================================================== grid_sample
GS_SHAPES = [(2, 3, 17, 23, 9, 11), (1, 2, 1, 1, 4, 5), (1, 1, 2, 7, 3, 3), (1, 1, 13, 1, 5, 5), (3, 2, 16, 32, 33, 20),
             (1, 1, 60, 80, 7, 7)]
GS_BORDER = [(False, 16, 32), (False, 2, 8), (False, 1, 4), (True, 17, 33), (True, 2, 9)]
GS_CASES = [("rand", ac) + s for ac in (False, True) for s in GS_SHAPES] + [("border",) + b for b in GS_BORDER] + \
           [("cap", False, 2, 1, 16, 32, 1025, 1024)]


def _norm_coord(p, size, ac):
    """normalised coordinate (float64) whose un-normalised value is the pixel coordinate p"""
    return 2.0 * p / (size - 1) - 1.0 if ac else (2.0 * p + 1.0) / size - 1.0


def gs_build(case):
    kind, ac = case[0], case[1]
    g = _gen(1, ac, *case[2:])
    if kind == "border":
        Hi, Wi = case[2], case[3]
        N, C = 2, 2
        ky = torch.arange(-16, 8 * Hi + 9, dtype=F64) / 8
        kx = torch.arange(-16, 8 * Wi + 9, dtype=F64) / 8
        gy, gx = torch.meshgrid(_norm_coord(ky, Hi, ac), _norm_coord(kx, Wi, ac), indexing="ij")
        grid = _exact(torch.stack((gx, gy), -1)[None].repeat(N, 1, 1, 1), what="(border grid)")
        grid[1] = grid[1].flip(0, 1)
    else:
        N, C, Hi, Wi, Ho, Wo = case[2:]
        grid = _ints(g, (N, Ho, Wo, 2), -128, 128, 2.0 ** -6)
    img = _ints(g, (N, C, Hi, Wi), -8, 8)
    ref64 = F.grid_sample(img.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=ac)
    ref = _exact(ref64, F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=ac), str(case))
    return img, grid, ac, ref


@gpu
@pytest.mark.parametrize("case", GS_CASES, ids=str)
def test_grid_sample_is_float64_bit_for_bit(dev, case):
    """Tier 1.  Image: integers in [-8, 8]; grid: multiples of 2^-6 in [-2, 2] (un-normalised coordinate exact for any size, weights
    multiples of 2^-14), or -- at power-of-two sizes -- built from the pixel coordinates k/8, k in [-16, 8 size + 8], so that samples
    land exactly on pixel -1, 0, size-1, size and beyond on both axes and in all four corners.  One case beyond the launch cap."""
    img, grid, ac, ref = gs_build(case)
    got = ops.grid_sample(img.to(dev), grid.to(dev), ac)
    assert torch.equal(got.cpu(), ref), _where_bad(got, ref)


BAD = [float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 3e9, -3e9]


def gs_nonfinite_build(ac):
    g = _gen(2, ac)
    N, C, Hi, Wi, Ho, Wo = 2, 2, 16, 32, 9, 12
    img = _ints(g, (N, C, Hi, Wi), 1, 8)
    grid = _ints(g, (N, Ho, Wo, 2), -56, 56, 2.0 ** -6)          # |g| <= 0.875: every sample inside the image, value > 0
    bad = torch.zeros(N, Ho, Wo, dtype=torch.bool)
    clean = grid.clone()
    for i, v in enumerate(BAD):                                  # isolated pixels: x only, y only, both
        for n, (y, x, ch) in enumerate(((1, 1 + i, (0,)), (4, 1 + i, (1,)), (7, 1 + i, (0, 1)))):
            b = (n + i) % N
            for c in ch:
                grid[b, y, x, c] = v
            bad[b, y, x] = True
            clean[b, y, x, :] = -4.0                             # far outside: all four corners masked
    ref = _exact(F.grid_sample(img.double(), clean.double(), mode="bilinear", padding_mode="zeros", align_corners=ac))
    assert bool((ref[bad[:, None].expand_as(ref)] == 0).all()) and bool((ref[~bad[:, None].expand_as(ref)] > 0).all())
    return img, grid, bad, ref


@gpu
@pytest.mark.parametrize("ac", [False, True])
def test_grid_sample_non_finite_and_huge_coordinates_give_zero(dev, ac):
    """NaN, +-inf, +-1e30 and +-3e9 (beyond int) in x, in y or in both: the pixel is 0 in every channel and every other pixel keeps
    its float64 value (positive here, so an unchanged neighbour is told from a zeroed one) -- the huge finite values guard the
    (int) conversion of the floor.  This follows ATen's CUDA grid_sampler, whose in-bounds masks are all false for such a
    coordinate; ATen's CPU kernel returns NaN for NaN and +-inf coordinates, and is NOT the model here."""
    img, grid, bad, ref = gs_nonfinite_build(ac)
    got = ops.grid_sample(img.to(dev), grid.to(dev), ac).cpu()
    assert torch.equal(got, ref), _where_bad(got, ref)


def gs_tier2_build(case):
    ac, N, C, Hi, Wi, Ho, Wo = case
    g = _gen(3, *case)
    img = torch.rand(N, C, Hi, Wi, generator=g) * 2 - 1
    grid = torch.rand(N, Ho, Wo, 2, generator=g) * 2.6 - 1.3
    ref = F.grid_sample(img.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=ac)
    pad = F.pad(img.double(), (1, 1, 1, 1))
    L = max(float((pad[..., 1:] - pad[..., :-1]).abs().max()), float((pad[..., 1:, :] - pad[..., :-1, :]).abs().max()))
    gd = grid.double()
    dx = 1.5 * U * ((gd[..., 0].abs() + 1) * Wi + 1)
    dy = 1.5 * U * ((gd[..., 1].abs() + 1) * Hi + 1)
    bound = (L * (dx + dy) + 8 * U * float(img.abs().max()))[:, None].expand_as(ref)
    aten32 = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=ac)
    assert bool(((aten32.double() - ref).abs() <= bound).all())
    return img, grid, ac, ref, bound


GS_T2 = [(False, 2, 3, 17, 23, 9, 11), (True, 2, 3, 17, 23, 9, 11), (False, 1, 2, 5, 3, 31, 29), (True, 1, 1, 7, 61, 40, 40)]


@gpu
@pytest.mark.parametrize("case", GS_T2, ids=str)
def test_grid_sample_odd_sizes_arbitrary_grids_within_the_derived_bound(dev, case):
    """Tier 2.  Bilinear sampling with zero padding is continuous and piecewise bilinear, so per pixel
    |err| <= L (dx + dy) + 8 u max|v|:  L = largest difference of adjacent pixels (zero border included);  dx = 1.5 u ((|gx| + 1) W
    + 1) is the un-normalised coordinate's own rounding (three roundings -- add, multiply, subtract, fewer under fma contraction --
    of magnitude <= (|gx| + 1) W + 1, halved by the final * 0.5), dy alike;  8 = roundings of the two complements 1 - w, the weight
    products, the four value products and three additions, each relative to <= max|v|."""
    img, grid, ac, ref, bound = gs_tier2_build(case)
    got = ops.grid_sample(img.to(dev), grid.to(dev), ac).cpu().double()
    err = (got - ref).abs()
    print("grid_sample tier 2 %s: max err %.3e, min slack %.3e" % (case, float(err.max()), float((bound - err).min())))
    assert bool((err <= bound).all())


# ====================================================================== resize_bilinear
RS_CASES = [(False, 2, 3, 6, 8, 48, 64), (False, 2, 3, 5, 3, 20, 24), (False, 2, 3, 1, 1, 8, 8), (False, 2, 3, 16, 16, 8, 4),
            (False, 2, 3, 1, 5, 4, 5), (True, 2, 3, 5, 9, 17, 33), (True, 2, 3, 2, 2, 9, 5), (True, 2, 3, 3, 3, 1, 1),
            (False, 7, 100, 6, 8, 48, 64)]
assert 7 * 100 * 48 * 64 > CAP


def rs_build(case):
    ac, N, C, Hi, Wi, Ho, Wo = case
    x = _ints(_gen(4, *case), (N, C, Hi, Wi), -8, 8)
    ref64 = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=ac)
    return x, (Ho, Wo), ac, _exact(ref64, F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=ac), str(case))


@gpu
@pytest.mark.parametrize("case", RS_CASES, ids=str)
def test_resize_bilinear_dyadic_ratios_are_float64_bit_for_bit(dev, case):
    """Tier 1.  Integer input, dyadic ratios only (scale, source index and both weights exact): x8 (the product's), x4 / x8 mixed,
    1x1 source, x1/2 / x1/4 down, a 1-row source; align_corners on 5x9 -> 17x33, 2x2 -> 9x5 and 3x3 -> 1x1; one case beyond the cap."""
    x, size, ac, ref = rs_build(case)
    got = ops.resize_bilinear(x.to(dev), size, ac)
    assert torch.equal(got.cpu(), ref), _where_bad(got, ref)


def rs_tier2_build(case):
    Hi, Wi, Ho, Wo = case
    x = torch.rand(2, 3, Hi, Wi, generator=_gen(5, *case)) * 2 - 1
    ref = F.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=False)
    xd = x.double()
    L = max(float((xd[..., 1:] - xd[..., :-1]).abs().max()), float((xd[..., 1:, :] - xd[..., :-1, :]).abs().max()))
    bound = L * 3 * U * (Hi + Wi) + 6 * U * float(x.abs().max())
    aten32 = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False)
    assert float((aten32.double() - ref).abs().max()) <= bound
    return x, (Ho, Wo), ref, bound


@gpu
@pytest.mark.parametrize("case", [(6, 8, 41, 67), (7, 5, 3, 11)], ids=str)
def test_resize_bilinear_non_dyadic_within_the_derived_bound(dev, case):
    """Tier 2.  Bilinear resizing (edge-clamped) is continuous: |err| <= L 3 u (Hin + Win) + 6 u max|v|.  The source index
    scale * (dst + 0.5) - 0.5 carries three roundings (the float32 scale, the product, the subtraction) of magnitude <= the input
    extent against float64's exact ratio; L = largest difference of adjacent pixels; 6 = the complements, products and sums of the
    two-stage interpolation, each relative to <= max|v|."""
    x, size, ref, bound = rs_tier2_build(case)
    err = float((ops.resize_bilinear(x.to(dev), size, False).cpu().double() - ref).abs().max())
    print("resize tier 2 %s: max err %.3e, bound %.3e" % (case, err, bound))
    assert err <= bound


# ====================================================================== maxpool2d
MP_CFG = [(3, 2, 1), (2, 1, 0), (3, 1, 1)]
MP_CASES = [(2, 3, 19, 26) + c for c in MP_CFG] + [(2, 2, 3, 3) + c for c in MP_CFG] + [(2, 2, 2, 2, 2, 1, 0), (2, 2, 1, 7, 3, 1, 1),
                                                                                          (2, 2, 1, 7, 3, 2, 1), (1, 3, 701, 1000, 3, 1, 1)]
assert 3 * 701 * 1000 > CAP


def mp_build(case):
    N, C, H, W, k, s, p = case
    x = torch.randn(N, C, H, W, generator=_gen(6, *case))
    x[0, 0, H // 3, W // 3] = float("nan")
    x[0, C - 1, H // 2, W // 2] = -float("inf")
    x[N - 1, 0, H // 2:H // 2 + 4, W // 2:W // 2 + 4] = -float("inf")     # whole windows of -inf
    if H <= 3:
        x[N - 1, C - 1] = -float("inf")
    ref64 = F.max_pool2d(x.double(), k, s, p)
    ref = ref64.float()
    assert _same(ref.double(), ref64) and _same(F.max_pool2d(x, k, s, p), ref)
    assert bool(ref.isnan().any()) and bool((ref == -float("inf")).any())
    return x, (k, s, p), ref


@gpu
@pytest.mark.parametrize("case", MP_CASES, ids=str)
def test_maxpool2d_equals_float64_for_any_input(dev, case):
    """Tier 1 (a maximum is exact for any input): random floats with a NaN (propagates), a -inf, and windows that hold only -inf,
    at (k, stride, pad) = (3,2,1), (2,1,0), (3,1,1); 19x26, 3x3, 2x2 (k = 2), 1x7 (k = 3, pad 1); one case beyond the cap."""
    x, (k, s, p), ref = mp_build(case)
    got = ops.maxpool2d(x.to(dev), k, s, p)
    assert _same(got, ref), _where_bad(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(ref, nan=7.0))


# ====================================================================== blurpool2d / maxblurpool2d
def blur64(x, stride):
    """reflect-pad 1, depthwise [1 2 1]^T [1 2 1] / 16, stride -- float64"""
    C = x.shape[1]
    a = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype)
    k = (a[:, None] * a[None, :] / 16)[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), k, stride=stride, groups=C)


BP_CASES = [(s, 2, 2, H, W) for s in (1, 2) for (H, W) in ((2, 2), (2, 9), (19, 26))] + [(1, 1, 3, 701, 1000)]
assert 3 * 701 * 1000 > CAP
MB_SIZES = [(3, 3), (3, 4), (4, 3), (8, 8), (12, 16), (37, 40), (10, 44), (19, 26)]
MB_CASES = [(s, 2, 2, H, W) for s in (1, 2, 3) for (H, W) in MB_SIZES] + [(1, 1, 3, 702, 1001)]
assert 3 * 701 * 1000 > CAP                                         # the per-output kernel's outputs at stride 1


def bp_build(case, fused):
    s, N, C, H, W = case
    x = _ints(_gen(7, fused, *case), (N, C, H, W), -64, 64, 0.125)
    x64 = F.max_pool2d(x.double(), 2, 1) if fused else x.double()
    x32 = F.max_pool2d(x, 2, 1) if fused else x
    return x, s, _exact(blur64(x64, s), blur64(x32, s), str(case))


@gpu
@pytest.mark.parametrize("case", BP_CASES, ids=str)
def test_blurpool2d_is_float64_bit_for_bit(dev, case):
    """Tier 1.  Input: integers in [-64, 64] / 8, weights 1/16, 1/8, 1/4: every product and partial sum is a multiple of 2^-7.
    2x2 and 2x9 are all reflected border; 3 x 701 x 1000 at stride 1 is beyond the cap."""
    x, s, ref = bp_build(case, False)
    got = ops.blurpool2d(x.to(dev), s)
    assert torch.equal(got.cpu(), ref), _where_bad(got, ref)


@gpu
@pytest.mark.parametrize("case", MB_CASES, ids=str)
def test_maxblurpool2d_is_float64_bit_for_bit_aligned_and_not(dev, case):
    """Tier 1, against float64 directly (MaxPool2d(2, 1) then the blur).  3x3, 3x4, 4x3: the smallest legal maps, all reflected
    border; 8x8: Win % 4 == 0 but no interior block yet (that needs Hin >= 9 and Win >= 12), so every 2x2 block of the
    register-blocked stride-2 kernel takes its border path; 12x16: the first size with interior blocks (two); 37x40 and 10x44:
    Win % 4 == 0 with odd Hout / odd Wout; 19x26: the per-output kernel; 3 x 702 x 1001 at stride 1: that kernel beyond the cap.  The same input as a view whose data pointer is not
    16-byte aligned (one element off a flat buffer) takes the per-output fall-back and must give the same bits."""
    x, s, ref = bp_build(case, True)
    got = ops.maxblurpool2d(x.to(dev), s)
    assert torch.equal(got.cpu(), ref), _where_bad(got, ref)
    flat = torch.empty(x.numel() + 1, device=dev)
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    got = ops.maxblurpool2d(view, s)
    assert torch.equal(got.cpu(), ref), _where_bad(got, ref)


def mb_cap_build():
    """2049 planes of 128x128 -> 64x64 outputs = 32x32 blocks each: 2049 * 1024 > 2^21 blocks.  The planes are 8 distinct ones in a
    random assignment, so that the float64 reference is 8 planes' work on the host."""
    g = _gen(8)
    base = _ints(g, (1, 8, 128, 128), -64, 64, 0.125)
    pick = torch.randint(0, 8, (2049,), generator=g)
    ref = _exact(blur64(F.max_pool2d(base.double(), 2, 1), 2), blur64(F.max_pool2d(base, 2, 1), 2))
    assert 2049 * 32 * 32 > CAP
    return base, pick, ref


@gpu
def test_maxblurpool2d_block_kernel_beyond_the_cap(dev):
    """Tier 1: N C ceil(Hout/2) ceil(Wout/2) > 2^21 -- the register-blocked kernel's grid-stride loop takes a second trip; the same
    planes one element off a flat buffer take the per-output fall-back, four times beyond the cap."""
    base, pick, ref = mb_cap_build()
    x = base.to(dev)[0][pick.to(dev)][None]
    got = ops.maxblurpool2d(x, 2)
    want = ref.to(dev)[0][pick.to(dev)][None]
    assert got.shape == want.shape and torch.equal(got, want)
    flat = torch.empty(x.numel() + 1, device=dev)       # (``got`` stays alive: a freed block would hand its right values to the next output)
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    assert torch.equal(ops.maxblurpool2d(view, 2), want)


# ====================================================================== warp_grid
WG_SIZES = [(17, 33), (5, 9), (2, 2), (1, 1), (1, 9)]


def warp_grid64(M, h, w, lin32=False):
    """(x', y', z') = M (x, y, 1) on the linspace(-1, 1) grid, (x'/z', y'/z'); numpy float64.  A size-1 axis sits at -1."""
    M = M.double().numpy()
    dt = torch.float32 if lin32 else F64
    xs = torch.linspace(-1, 1, w, dtype=dt).double().numpy()
    ys = torch.linspace(-1, 1, h, dtype=dt).double().numpy()
    X, Y = np.meshgrid(xs, ys)
    P = np.stack((X, Y, np.ones_like(X)), -1)                        # (h, w, 3)
    Q = np.einsum("bij,hwj->bhwi", M, P)
    S = np.einsum("bij,hwj->bhwi", np.abs(M), np.abs(P))             # sum |terms| of each chain
    A = np.broadcast_to((np.abs(M[:, :, 0]) + np.abs(M[:, :, 1]))[:, None, None, :], S.shape)
    return torch.from_numpy(Q[..., :2] / Q[..., 2:]), (S, A, Q)


def wg_build(h, w, B=3):
    g = _gen(9, h, w, B)
    M = _ints(g, (B, 3, 3), -16, 16, 0.125)
    M[:, 2, :2] = 0
    M[:, 2, 2] = torch.tensor([1.0, 2.0, 0.5, 1.0, 2.0])[:B]
    for n, dt in ((h, F64), (w, F64)):
        assert torch.equal(torch.linspace(-1, 1, n).double(), torch.linspace(-1, 1, n, dtype=dt)), "linspace not exact"
    assert float(torch.linspace(-1, 1, 1)[0]) == -1.0
    return M, _exact(warp_grid64(M, h, w)[0])


@gpu
@pytest.mark.parametrize("hw", WG_SIZES + [(513, 1025)], ids=str)
def test_warp_grid_affine_dyadic_is_float64_bit_for_bit(dev, hw):
    """Tier 1.  h - 1, w - 1 powers of two (linspace exact), affine matrices with entries k/8 and M[2][2] in {1, 2, 1/2} (the division
    is exact), a batch of different matrices; 5 x 513 x 1025 is beyond the cap."""
    B = 5 if hw[0] > 100 else 3
    assert hw[0] < 100 or B * hw[0] * hw[1] > CAP
    M, ref = wg_build(hw[0], hw[1], B)
    got = ops.warp_grid(M.to(dev), hw[0], hw[1])
    assert torch.equal(got.cpu(), ref), _where_bad(got, ref)


def wg_tier2_build(h, w):
    g = _gen(10, h, w)
    M = torch.randn(3, 3, 3, generator=g)
    M[:, 2, :2] = (torch.rand(3, 2, generator=g) - 0.5) * 0.5           # |a| + |b| <= 1/2
    M[:, 2, 2] = 1.0
    ref, (S, A, Q) = warp_grid64(M, h, w)
    zs = Q[..., 2]
    assert np.abs(zs).min() >= 0.5
    q = np.abs(Q[..., :2] / Q[..., 2:])
    E = U * (3 * S + 2 * A)                                          # per chain: its own roundings + the grid coordinates'
    bound = (E[..., :2] + q * E[..., 2:]) / np.abs(Q[..., 2:]) * 1.001 + U * q
    return M, ref, torch.from_numpy(bound)


@gpu
@pytest.mark.parametrize("hw", [(48, 64), (7, 5), (17, 33)], ids=str)
def test_warp_grid_projective_within_the_derived_bound(dev, hw):
    """Tier 2.  Per coordinate |err| <= (En + |q| Ed) / |zs| + u |q|, q = numerator / zs, with E = u (3 S + 2 A) per chain: three
    roundings relative to S = sum |terms|; the float32 linspace coordinate is within 2 u of float64's (the rounded step times the
    index, then one fused add -- an ABSOLUTE error: near the grid's centre the coordinate is small and its error is not), which
    enters through A = |M[i][0]| + |M[i][1]|; the division adds one rounding.  Matrices are drawn with |zs| >= 1/2 over the grid
    (asserted on the host)."""
    M, ref, bound = wg_tier2_build(*hw)
    err = (ops.warp_grid(M.to(dev), hw[0], hw[1]).cpu().double() - ref).abs()
    print("warp_grid tier 2 %s: max err %.3e, min slack %.3e" % (hw, float(err.max()), float((bound - err).min())))
    assert bool((err <= bound).all())


# ====================================================================== compose_flow
def compose64(fd, coarse, H, W, clamp, dt=F64):
    """F.interpolate + identity grid (+ clamp) + F.grid_sample of the coarse grid + the in-bounds flag, in ``dt``.  The identity
    grid holds the float32 linspace values (widened)."""
    up = F.interpolate(fd.to(dt), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    gx = torch.linspace(-1, 1, W).to(dt).view(1, 1, W).expand(1, H, W)
    gy = torch.linspace(-1, 1, H).to(dt).view(1, H, 1).expand(1, H, W)
    up = up + torch.stack((gx, gy), -1)
    if clamp:
        up = up.clamp(-1, 1)
    return up


def sample64(coarse, up):
    f12 = F.grid_sample(coarse.permute(0, 3, 1, 2).to(up.dtype), up, mode="bilinear", padding_mode="zeros",
                        align_corners=False).permute(0, 2, 3, 1)
    inb = ((f12 >= -1) & (f12 <= 1)).all(-1).to(up.dtype)
    return f12, inb


CF_CASES = [(H, W, Hc, Wc, clamp, huge) for (H, W, Hc, Wc) in ((17, 33, 17, 33), (5, 9, 5, 9), (17, 33, 9, 20))
            for clamp in (False, True) for huge in (False,)] + [(17, 33, 17, 33, False, True), (17, 33, 9, 20, False, True),
                                                                (513, 2049, 9, 20, True, False)]
assert 2 * 513 * 2049 > CAP


def cf_build(case):
    H, W, Hc, Wc, clamp, huge = case
    N = 2
    g = _gen(11, *case)
    fd = _ints(g, (N, 2, H, W), -96, 96, 2.0 ** -6)                   # +-1.5 on top of the +-1 identity grid: leaves on all sides
    coarse = _ints(g, (N, Hc, Wc, 2), -2, 2)
    ph, pw = (Hc + 2) // 3, (Wc + 2) // 3
    coarse[:, :ph, :pw] = 1.0                                        # constant patches sampled with zero flow: exactly +-1
    coarse[:, Hc - ph:, Wc - pw:] = -1.0
    fd[:, :, 1, 1] = 0.0
    fd[:, :, H - 2, W - 2] = 0.0
    bad = torch.zeros(N, H, W, dtype=torch.bool)
    clean = fd.clone()
    if huge:                                                         # finite but far beyond int, on isolated pixels
        for i, v in enumerate((1e30, -1e30, 3e9, -3e9)):
            n, c, y, x = i % 2, (i // 2) % 2, 3, 2 + 2 * i
            fd[n, c, y, x] = v
            clean[n, c, y, x] = 0.0
            bad[n, y, x] = True
    for n_ in (H, W):
        assert torch.equal(torch.linspace(-1, 1, n_).double(), torch.linspace(-1, 1, n_, dtype=F64))
    up = compose64(fd, coarse, H, W, clamp)
    up_s = compose64(clean, coarse, H, W, clamp)
    up_s[bad] = -4.0
    f12, inb = sample64(coarse, up_s)
    f12_32, inb32 = sample64(coarse, up_s.float())
    ref12, refup = _exact(f12, f12_32, str(case)), up.float()        # at a huge flow the sum rounds once, in float32 as in float64
    assert torch.equal(refup[~bad].double(), up[~bad])
    assert torch.equal(inb.float(), inb32)
    if huge:
        assert bool((ref12[bad] == 0).all())
    ok = ~bad
    assert bool((ref12[ok] == 1).any()) and bool((ref12[ok] == -1).any()) and bool((inb == 0).any())
    on_edge = ((ref12.abs() == 1).any(-1)) & (ref12.abs() <= 1).all(-1)
    assert bool(on_edge.any()) and bool((inb[on_edge] == 1).all())
    raw = compose64(clean, coarse, H, W, False)                      # before the clamp: out on all four sides and in the corners
    assert float(raw.abs().min(dim=-1).values.max()) > 1 and bool((raw[..., 0] < -1).any()) and bool((raw[..., 0] > 1).any()) \
        and bool((raw[..., 1] < -1).any()) and bool((raw[..., 1] > 1).any())
    return fd, coarse, (H, W), clamp, ref12, refup, inb.float()


@gpu
@pytest.mark.parametrize("case", CF_CASES, ids=str)
def test_compose_flow_is_float64_bit_for_bit(dev, case):
    """Tier 1.  hd x wd = H x W in {17x33, 5x9} (the up-sampling is the identity and the identity grid exact), flowDown multiples of
    2^-6 that leave the image on all four sides, an integer coarse grid of the output's size or of another one (9x20 against 17x33:
    the KITTI full-resolution pass; 2 x 513 x 2049 against 9x20 is beyond the cap), clamp on and off: flow12, flowUp and the
    in-bounds flag are all bit-equal to float64, values
    exactly +-1 (flag = 1) included.  ``huge``: +-1e30 and +-3e9 residual flows on isolated pixels give 0 there -- as ATen's CUDA
    grid_sampler does, see test_grid_sample_non_finite_and_huge_coordinates_give_zero -- and leave every neighbour's bits alone."""
    fd, coarse, hw, clamp, ref12, refup, refinb = cf_build(case)
    f12, inb, fup = ops.compose_flow(fd.to(dev), coarse.to(dev), clamp=clamp, want_inb=True, want_flow_up=True, out_hw=hw)
    assert torch.equal(fup.cpu(), refup), _where_bad(fup, refup)
    assert torch.equal(f12.cpu(), ref12), _where_bad(f12, ref12)
    assert torch.equal(inb.cpu(), refinb), _where_bad(inb, refinb)
    f12b, inbb, fupb = ops.compose_flow(fd.to(dev), coarse.to(dev), clamp=clamp, out_hw=hw)
    assert inbb is None and fupb is None and torch.equal(f12b, f12)


def cf_up_build(clamp):
    g = _gen(12, clamp)
    fd = _ints(g, (2, 2, 6, 8), -32, 32, 2.0 ** -6)
    coarse = _ints(g, (2, 48, 64, 2), -2, 2)
    up64 = compose64(fd, coarse, 48, 64, clamp)
    up32 = compose64(fd, coarse, 48, 64, clamp, torch.float32)
    ref = up64.float()                    # one rounding of an exact sum: the float32 addition's
    assert torch.equal(ref, up32), "F.interpolate + identity grid is not the rounded float64 sum"
    return fd, coarse, ref


@gpu
@pytest.mark.parametrize("clamp", [False, True])
def test_compose_flow_flow_up_x8_equals_resize_plus_grid(dev, clamp):
    """6x8 -> 48x64 (the product's x8): the up-sampled dyadic flow is exact, and linspace(-1, 1, 64) -- inexact, but the same float32
    value, added once -- makes flowUp bit-equal to F.interpolate(...) + identity grid in float32 (= the float64 sum rounded once)."""
    fd, coarse, ref = cf_up_build(clamp)
    _, _, fup = ops.compose_flow(fd.to(dev), coarse.to(dev), clamp=clamp, want_flow_up=True)
    assert torch.equal(fup.cpu(), ref), _where_bad(fup, ref)


def cf_nonfinite_build():
    g = _gen(13)
    fd = _ints(g, (2, 2, 6, 8), -16, 16, 2.0 ** -6)                   # |flow| <= 1/4
    coarse = _ints(g, (2, 48, 64, 2), 1, 2)
    clean = fd.clone()
    cells = [(0, 0, 2, 2), (0, 1, 2, 5), (0, 0, 4, 3), (1, 1, 2, 3), (1, 0, 4, 2), (1, 1, 4, 5), (0, 1, 4, 6)]   # isolated, >= 2
    for v, (n, c, y, x) in zip(BAD, cells):
        fd[n, c, y, x] = v
    up = compose64(fd, coarse, 48, 64, False)
    bad = (~torch.isfinite(up) | (up.abs() > 3)).any(-1)
    up_c = compose64(clean, coarse, 48, 64, False)
    assert float(up_c.abs().max()) <= 1.25 and bool((up[~bad] == up_c[~bad]).all()) and 0.05 < float(bad.float().mean()) < 0.5
    assert float(up[bad].abs().nan_to_num(nan=1e38).max(dim=-1).values.min()) > 1e6       # far outside, never a near miss
    return fd, clean, coarse, bad


@gpu
def test_compose_flow_non_finite_flow_gives_zero_and_spares_the_rest(dev):
    """NaN, +-inf, +-1e30, +-3e9 in isolated cells of a 6x8 residual flow, up-sampled x8 (clamp off): wherever the float64 up-sampled
    flow is non-finite or far outside, flow12 is 0 (and the flag 1: 0 is in bounds) -- ATen's CUDA grid_sampler rule, not its CPU
    kernel's NaN; every other pixel has the bits of the same call on the flow without those cells.  (With hd x wd = H x W a
    non-finite cell would also spoil its left / upper neighbours through a zero-weight tap, where ATen copies the map: the bad
    cells sit at rows / columns >= 2 of a true up-sampling, away from every zero-weight tap.)"""
    fd, clean, coarse, bad = cf_nonfinite_build()
    f12, inb, fup = ops.compose_flow(fd.to(dev), coarse.to(dev), want_inb=True, want_flow_up=True)
    c12, cinb, cup = ops.compose_flow(clean.to(dev), coarse.to(dev), want_inb=True, want_flow_up=True)
    f12, inb, fup, c12, cinb, cup = (t.cpu() for t in (f12, inb, fup, c12, cinb, cup))
    assert bool((f12[bad] == 0).all()) and bool((inb[bad] == 1).all())
    assert float((c12[bad].abs().sum(-1) > 0).float().mean()) > 0.9  # ... where the clean flow samples a positive grid
    assert torch.equal(f12[~bad], c12[~bad]) and torch.equal(inb[~bad], cinb[~bad]) and torch.equal(fup[~bad], cup[~bad])
    assert bool((~torch.isfinite(fup[bad]) | (fup[bad].abs() > 3)).any(-1).all())


def cf_clamp_nonfinite_build():
    g = _gen(23)
    fd = _ints(g, (2, 2, 6, 8), -16, 16, 2.0 ** -6)
    coarse = _ints(g, (2, 48, 64, 2), 1, 2)
    cells = [(0, 0, 2, 2), (0, 1, 2, 5), (0, 0, 4, 3), (1, 1, 2, 3), (1, 0, 4, 2), (1, 1, 4, 5), (0, 1, 4, 6)]
    twin = fd.clone()
    for v, (n, c, y, x) in zip(BAD, cells):
        fd[n, c, y, x] = v
        twin[n, c, y, x] = 1e6 if v == float("inf") else (-1e6 if v != v or v == -float("inf") else v)
    nan_up = torch.isnan(compose64(fd, coarse, 48, 64, False))
    assert 0 < int(nan_up.sum()) < nan_up.numel() // 8
    return fd, twin, coarse, nan_up


@gpu
def test_compose_flow_pins_non_finite_flow_under_clamp_and_at_identity_size(dev):
    """Two behaviours of compose_flow on a non-finite residual flow that are NOT ATen's, pinned as they are so that a change is
    noticed (the product never feeds one; DESIGN_LOG.md):
    (1) clamp on -- what every product call but one passes: fminf(fmaxf(NaN, -1), 1) = -1 where torch.clamp keeps the NaN, so the
        pixel does not become 0 but samples the coarse grid's border at -1.  The whole result (flowUp, flow12, flag) is bit-equal
        to the call on the same flow with NaN -> -1e6 (and +-inf -> +-1e6, which clamp like torch's), and flowUp is exactly -1
        wherever the float64 up-sampled flow is NaN.
    (2) hd x wd = H x W, clamp off: ATen copies the map (only the cell itself is non-finite); the kernel still interpolates, and
        0 * NaN / 0 * inf through the zero-weight taps spoils the cell's left, upper and upper-left neighbours too: those four pixels
        are 0, every other pixel has its float64 bits."""
    fd, twin, coarse, nan_up = cf_clamp_nonfinite_build()
    a = ops.compose_flow(fd.to(dev), coarse.to(dev), clamp=True, want_inb=True, want_flow_up=True)
    b = ops.compose_flow(twin.to(dev), coarse.to(dev), clamp=True, want_inb=True, want_flow_up=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert bool((a[2].cpu()[nan_up] == -1).all())
    fd, coarse, hw, clamp, ref12, refup, refinb = cf_build((17, 33, 17, 33, False, False))
    want = ref12.clone()
    for (n, c, y, x, v) in ((0, 0, 5, 7, float("nan")), (1, 1, 9, 20, float("inf")), (1, 0, 12, 3, -float("inf"))):
        fd[n, c, y, x] = v
        want[n, y - 1:y + 1, x - 1:x + 1] = 0.0
    f12, _, _ = ops.compose_flow(fd.to(dev), coarse.to(dev), out_hw=hw)
    assert torch.equal(f12.cpu(), want), _where_bad(f12, want)


# ====================================================================== flow_grad_clamp
FG_CASES = [(2, 2, 9, 1), (2, 7, 2, 2), (1, 2, 2, 1), (3, 6, 5, 3), (2, 1025, 1026, 1)]
assert 2 * 1025 * 1026 > CAP


def fg_build(case):
    B, H, W, gb = case
    g = _gen(14, *case)
    a = _ints(g, (B, 1, H, W), -20, 20)
    trip = torch.tensor([[3.0, 4.0], [5.0, 12.0], [4.0, 3.0]])[torch.arange(B) % 3] * 2.0 ** -torch.arange(5, 5 + B)[:, None]
    f = a * trip.view(B, 2, 1, 1)                                   # diagonal differences (3, 4) 2^-k |da|: the norm is 5 2^-k |da|
    grid = _ints(g, (gb, H, W, 2), -80, 80, 2.0 ** -6)
    flow = (f.double().permute(0, 2, 3, 1) + grid.double()).clamp(-1, 1)
    fgrad = torch.norm(f.double()[:, :, 1:, 1:] - f.double()[:, :, :-1, :-1], dim=1, keepdim=True)
    aten_flow = torch.clamp(f.permute(0, 2, 3, 1) + grid, min=-1, max=1)
    return f, grid, _exact(flow, aten_flow, str(case)), _exact(fgrad, None, str(case))


@gpu
@pytest.mark.parametrize("case", FG_CASES, ids=str)
def test_flow_grad_clamp_pythagorean_differences_are_exact(dev, case):
    """Tier 1.  Flows whose diagonal differences are Pythagorean multiples (3,4,5) 2^-k / (5,12,13) 2^-k: squares, sum and root are
    exact, so flowGrad is torch.equal to float64's norm (and the clamped sum with a dyadic grid to float64's); H = 2, W = 2, both,
    a per-sample grid, and a case beyond the cap."""
    f, grid, ref_flow, ref_fg = fg_build(case)
    fg, flow = ops.flow_grad_clamp(f.to(dev), grid.to(dev))
    assert torch.equal(flow.cpu(), ref_flow), _where_bad(flow, ref_flow)
    assert fg.shape == ref_fg.shape and torch.equal(fg.cpu(), ref_fg), _where_bad(fg, ref_fg)


# ====================================================================== adaptive_avgpool2d
AP_CASES = [(H, W, s) for (H, W) in ((12, 12), (13, 17), (6, 6), (1, 1)) for s in (1, 2, 3, 6)]


def ap_counts(H, W, s):
    ch = [-(-(o + 1) * H // s) - (o * H) // s for o in range(s)]
    cw = [-(-(o + 1) * W // s) - (o * W) // s for o in range(s)]
    return [a * b for a in ch for b in cw]


def ap_build(case):
    H, W, s = case
    g = _gen(15, *case)
    x = _ints(g, (2, 3, H, W), -8, 8)
    ref64 = F.adaptive_avg_pool2d(x.double(), s)
    pow2 = all(c & (c - 1) == 0 for c in ap_counts(H, W, s))
    if pow2:
        _exact(ref64, F.adaptive_avg_pool2d(x, s), str(case))
    xr = torch.randn(2, 3, H, W, generator=g)
    refr = F.adaptive_avg_pool2d(xr.double(), s)
    n = torch.tensor(ap_counts(H, W, s), dtype=F64).view(1, 1, s, s)
    boundr = n * U * F.adaptive_avg_pool2d(xr.double().abs(), s)
    assert bool(((F.adaptive_avg_pool2d(xr, s).double() - refr).abs() <= boundr).all())
    return x, s, ref64, pow2, xr, refr, boundr


@gpu
@pytest.mark.parametrize("case", AP_CASES, ids=str)
def test_adaptive_avgpool2d_integer_inputs_and_the_rounding_bound(dev, case):
    """Integer inputs, the PPM's output sizes 1, 2, 3, 6 on 12x12, 13x17 (overlapping windows), 6x6 and 1x1.  Tier 1 where every
    window's element count is a power of two (sum and division exact): torch.equal.  Tier 2 elsewhere: the integer sum is still
    exact, so |err| <= u |ref| -- the one rounding of the division; and for random floats |err| <= n u mean|v| over the window of n
    elements (n - 1 additions and the division, each relative to <= sum|v| / n after the division)."""
    x, s, ref64, pow2, xr, refr, boundr = ap_build(case)
    got = ops.adaptive_avgpool2d(x.to(dev), s).cpu()
    if pow2:
        assert torch.equal(got, ref64.float()), _where_bad(got, ref64.float())
    assert bool(((got.double() - ref64).abs() <= U * ref64.abs()).all())
    err = (ops.adaptive_avgpool2d(xr.to(dev), s).cpu().double() - refr).abs()
    assert bool((err <= boundr).all())


@gpu
def test_adaptive_avgpool2d_beyond_the_cap(dev):
    """Tier 1: 2 x 29200 planes of 12x12 -> 6x6 (windows of 4 integers: exact), 2 102 400 outputs."""
    x = _ints(_gen(24), (2, 29200, 12, 12), -8, 8)
    assert x.numel() // 4 > CAP
    ref = _exact(F.adaptive_avg_pool2d(x.double(), 6), F.adaptive_avg_pool2d(x, 6))
    got = ops.adaptive_avgpool2d(x.to(dev), 6)
    assert torch.equal(got.cpu(), ref), _where_bad(got, ref)


# ====================================================================== argmax_mask / copy_cols
@gpu
@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (3, 1, 2, 3), (2, 2, 1025, 1030)], ids=str)
def test_argmax_mask_first_index_wins_ties(dev, shape):
    """Scores are integers in [0, 3]: exact ties between classes at most pixels, the FIRST index must win as torch.max / numpy.argmax
    do; both ``complement`` settings; N HW beyond the cap."""
    N, C, H, W = shape
    sc = _ints(_gen(16, *shape), shape, 0, 3)
    pred_ref = torch.from_numpy(np.argmax(sc.numpy(), axis=1))
    assert torch.equal(pred_ref, sc.double().max(dim=1)[1]) and (C == 1 or bool((sc[:, 0] == sc[:, 1]).any()))
    for cid in (0, C - 1):
        m, pred = ops.argmax_mask(sc.to(dev), cid, complement=False, want_pred=True)
        assert torch.equal(pred.cpu().long(), pred_ref)
        assert torch.equal(m.cpu(), (pred_ref == cid).float())
        assert torch.equal(ops.argmax_mask(sc.to(dev), cid, complement=True).cpu(), (pred_ref != cid).float())


@gpu
@pytest.mark.parametrize("case", [(7, 5, 8), (7, 5, 5), (7, 8, 5), (9, 1, 4), (9, 4, 1), (5, 1, 1), (2100, 1000, 1001)], ids=str)
def test_copy_cols_index_image(dev, case):
    """w_dst <, = and > w_src, width 1 on either side, beyond the cap: an index image against numpy slicing."""
    rows, ws, wd = case
    src = (torch.arange(rows * ws, dtype=torch.float32) + 1).view(rows, ws)
    ref = np.zeros((rows, wd), np.float32)
    ref[:, :min(ws, wd)] = src.numpy()[:, :min(ws, wd)]
    assert torch.equal(ops.copy_cols(src.to(dev), wd).cpu(), torch.from_numpy(ref))


# ====================================================================== l2norm
@gpu
@pytest.mark.parametrize("shape", [(2, 17, 7, 5), (1, 31, 9, 11), (3, 33, 5, 5), (1, 36, 5, 13), (2, 16, 3, 3), (1, 1, 2, 2),
                                   (2, 3, 513, 512)], ids=str)
def test_l2norm_remainder_loops_equal_torch_normalize_bit_for_bit(dev, shape):
    """As test_gpu_kernels.py::test_l2norm_equals_torch_normalize_bit_for_bit (one fma chain in ATen's order): the one-thread-per-pixel
    kernel's remainder loop at C = 17, 31, 33 (around its 16-unroll, not multiples of 4), C = 16 and 1, and the four-wavefront kernel
    at C = 36 with N HW = 65, not a multiple of 64; 2 x 3 x 513 x 512 is beyond the one-thread-per-pixel kernel's own cap
    (64 x 8192 pixels)."""
    g = _gen(17, *shape)
    x = torch.relu(torch.randn(*shape, generator=g)) * torch.rand(1, shape[1], 1, 1, generator=g)
    x[0, :, 0, 0] = 0.0
    assert shape[2] < 100 or shape[0] * shape[2] * shape[3] > 64 * 8192
    assert torch.equal(ops.l2norm(x.to(dev)).cpu(), F.normalize(x))


@gpu
def test_l2norm_scatter_two_images_out_of_order(dev):
    """l2norm_scatter: two images written in non-monotone order (dst_off[0] > dst_off[1]) with a channel stride > HW: bit-equal to
    F.normalize, every untouched column stays zero."""
    N, C, H, W = 2, 36, 5, 7
    HW, ld = H * W, 3 * H * W + 11
    g = _gen(18)
    x = torch.randn(N, C, H, W, generator=g)
    want = F.normalize(x).view(N, C, HW)
    out = torch.zeros(C, ld, device=dev)
    off = torch.tensor([2 * HW + 5, 3], dtype=torch.int64)
    ops.l2norm_scatter(x.to(dev), out, off.to(dev), ld)
    out = out.cpu()
    keep = torch.ones(ld, dtype=torch.bool)
    for n in range(N):
        assert torch.equal(out[:, off[n]:off[n] + HW], want[n])
        keep[off[n]:off[n] + HW] = False
    assert int(keep.sum()) == ld - 2 * HW and bool((out[:, keep] == 0).all())


# ====================================================================== flow_head / softmax_accum
# Largest |device - float64| of flow_head on each of the three cases below, measured on an MI355X (ROCm 7.0 device library expf)
# against the float64 softmax expectation on 2026-10-17; see test_flow_head_within_four_times_the_measured_error.
FLOW_HEAD_MEASURED = {3: 1.437e-9, 5: 8.254e-8, 7: 2.484e-7}
FH_CASES = [(3, 1, 600, 900), (5, 2, 13, 22), (7, 2, 6, 9)]
assert 600 * 900 > 64 * 8192


def flow_head64(lg, K):
    N, KK, R, Cc = lg.shape
    p = F.softmax(lg.double(), dim=1)
    off = torch.arange(K, dtype=F64) - K // 2
    ox = off.view(1, K).expand(K, K).reshape(1, KK, 1, 1)
    oy = off.view(K, 1).expand(K, K).reshape(1, KK, 1, 1)
    ref = torch.cat(((p * ox).sum(1, keepdim=True) / Cc * 2, (p * oy).sum(1, keepdim=True) / R * 2), 1)
    # accumulation part of the bound (expf taken as exact): per tap the subtraction l - max (u |l - max|, relative on e), the
    # sum of KK terms, the division, the product and the KK additions of the expectation, the final division
    a = (lg.double() - lg.double().max(dim=1, keepdim=True).values).abs() * U
    A = (p * a).sum(1, keepdim=True) + (2 * KK + 3) * U
    acc = torch.cat(((p * ox.abs() * (a + A)).sum(1, keepdim=True) / Cc * 2, (p * oy.abs() * (a + A)).sum(1, keepdim=True) / R * 2), 1)
    return ref, acc


def fh_build(case):
    K, N, R, Cc = case
    g = _gen(19, *case)
    lg = torch.randn(N, K * K, R, Cc, generator=g) * torch.tensor([1.0, 3.0, 10.0, 30.0])[torch.randint(0, 4, (N, 1, R, Cc), generator=g)]
    lg = lg.clamp(-30, 30)
    dom = torch.randint(0, K * K, (N, R, Cc), generator=g)
    sel = torch.rand(N, R, Cc, generator=g)
    is_dom, is_flat = sel < 0.2, sel > 0.9
    lg = torch.where(is_dom[:, None], -30.0 * torch.ones_like(lg), lg)
    lg.scatter_(1, dom[:, None], torch.where(is_dom, torch.tensor(30.0), lg.gather(1, dom[:, None])[:, 0])[:, None])
    lg = torch.where(is_flat[:, None], lg[:, :1].expand_as(lg), lg).contiguous()
    ref, acc = flow_head64(lg, K)
    return lg, K, ref, acc, dom, is_dom, is_flat


@gpu
@pytest.mark.parametrize("case", FH_CASES, ids=str)
def test_flow_head_within_four_times_the_measured_error(dev, case):
    """Tier 2.  K in {3, 5, 7}, non-square maps, logits scaled up to +-30, NP = 540 000 > 64 * 8192 (this kernel's own cap).  A pixel
    with one dominant logit (+30 against -30: the others weigh e^-60) answers its tap's offset to a relative 1e-6 -- which is also
    the routing check: every pixel has another dominant tap; a pixel with all logits equal answers 0 (|.| <= 1e-7, the existing
    known-answer bound).  Everywhere: the accumulation part is derived (``flow_head64``: per tap u |l - max| from the subtraction,
    then 2 K^2 + 3 roundings of sum, division, products and additions, weighted by p |offset|); expf's own error is the vendor's
    and no ulp bound of the device library is documented in the ROCm installation, so the whole error is bounded at 4x the largest
    |device - float64| measured on these very inputs (FLOW_HEAD_MEASURED, with its date: 1.4e-9 / 8.3e-8 / 2.5e-7 for K = 3 / 5 / 7,
    each below the derived accumulation part alone, 4e-9 / 1e-6 / 6e-6 at worst).  The existing 1e-6 absolute check stays."""
    lg, K, ref, acc, dom, is_dom, is_flat = fh_build(case)
    got = ops.flow_head(lg.to(dev), K).cpu().double()
    N, _, R, Cc = lg.shape
    err = (got - ref).abs()
    print("flow_head K=%d: max err %.3e (accumulation part of the bound at that pixel %.3e, max %.3e)"
          % (K, float(err.max()), float(acc.flatten()[err.argmax()]), float(acc.max())))
    want = torch.stack(((dom % K - K // 2).double() / Cc * 2, (dom // K - K // 2).double() / R * 2), 1)
    d = is_dom[:, None].expand_as(got)
    assert bool(((got - want).abs()[d] <= 1e-6 * want.abs()[d] + 1e-20).all())       # (+ the other taps' e^-60)
    assert float(got[is_flat[:, None].expand_as(got)].abs().max()) <= 1e-7
    assert float(err.max()) < 1e-6
    assert float(err.max()) <= 4 * FLOW_HEAD_MEASURED[K]


# Largest |device - float64| of softmax_accum after the first / the second accumulation on the inputs below, measured on an MI355X
# (ROCm 7.0 device library expf) on 2026-10-17; see test_softmax_accum_twice_within_four_times_the_measured_error.
SOFTMAX_MEASURED = {2: (2.056e-8, 4.049e-8), 150: (1.113e-7, 1.412e-7)}


def sm_build(C):
    g = _gen(20, C)
    lgs = [torch.randn(2, C, 9, 13, generator=g) * 3, torch.randn(2, C, 9, 13, generator=g) * 8]
    div = 5.0
    refs, accs, tot, tota = [], [], 0.0, 0.0
    for lg in lgs:
        p = F.softmax(lg.double(), dim=1)
        a = (lg.double() - lg.double().max(dim=1, keepdim=True).values).abs() * U      # the subtraction, carried through exp
        rel = a + (p * a).sum(1, keepdim=True) + (C - 1) * U + 2 * U
        tot = tot + p / div
        tota = tota + p / div * rel * 1.001
        refs.append(tot)
        accs.append(tota + (U * tot if len(refs) > 1 else 0.0))
    return lgs, div, refs, accs


@gpu
@pytest.mark.parametrize("C", [2, 150])
def test_softmax_accum_twice_within_four_times_the_measured_error(dev, C):
    """Tier 2.  C in {2, 150}, div = 5, accumulated twice into one buffer.  The accumulation part is derived (``sm_build``), per
    element relative to p / div: a_c + sum_c' p_c' a_c' + (C - 1) u + 2 u with a_c = u |l_c - max| (the subtraction's rounding
    carried through exp), the sum of C terms and the two divisions; the second accumulation adds u |total| for its one addition.
    expf's own error is the vendor's and -- as for flow_head -- no ulp bound of the device library is documented in the ROCm
    installation, so the whole error is bounded at 4x the largest |device - float64| measured on these very inputs
    (SOFTMAX_MEASURED, with its date: 2.1e-8 / 4.0e-8 for C = 2, 1.1e-7 / 1.4e-7 for C = 150, after the first / second call)."""
    lgs, div, refs, accs = sm_build(C)
    sc = ops.softmax_accum(lgs[0].to(dev), None, div=div)
    e0 = float((sc.cpu().double() - refs[0]).abs().max())
    assert ops.softmax_accum(lgs[1].to(dev), sc, div=div) is sc
    e1 = float((sc.cpu().double() - refs[1]).abs().max())
    print("softmax_accum C=%d: max err %.3e / %.3e (derived accumulation part, max %.3e / %.3e)"
          % (C, e0, e1, float(accs[0].max()), float(accs[1].max())))
    assert e0 <= 4 * SOFTMAX_MEASURED[C][0] and e1 <= 4 * SOFTMAX_MEASURED[C][1]


# ====================================================================== Tier 3: index images, integral coordinates, numpy indexing
def _index_image(*shape):
    n = int(np.prod(shape))
    assert n < 2 ** 24
    return (torch.arange(n, dtype=torch.float32) + 1).view(*shape)


@gpu
@pytest.mark.parametrize("case", [(False, 2, 3, 4, 8, 6, 5), (True, 2, 3, 5, 9, 6, 5), (False, 2, 1, 4, 8, 1024, 1025)], ids=str)
def test_index_image_grid_sample(dev, case):
    """Tier 3: out[n, c, i, j] = img[n, c, py, px] (0 outside) for integral sample positions, H != W, N > 1, C > 1, beyond the cap."""
    ac, N, C, Hi, Wi, Ho, Wo = case
    g = _gen(21, *case)
    img = _index_image(N, C, Hi, Wi)
    py = torch.randint(-1, Hi + 1, (N, Ho, Wo), generator=g)
    px = torch.randint(-1, Wi + 1, (N, Ho, Wo), generator=g)
    grid = _exact(torch.stack((_norm_coord(px.double(), Wi, ac), _norm_coord(py.double(), Hi, ac)), -1))
    padded = np.zeros((N, C, Hi + 2, Wi + 2), np.float32)
    padded[:, :, 1:-1, 1:-1] = img.numpy()
    n_idx = np.arange(N)[:, None, None]
    ref = np.moveaxis(padded[n_idx, :, py.numpy() + 1, px.numpy() + 1], -1, 1)
    assert N * Ho * Wo > CAP or Ho < 100
    got = ops.grid_sample(img.to(dev), grid.to(dev), ac).cpu().numpy()
    assert np.array_equal(got, ref)


@gpu
def test_index_image_compose_flow(dev):
    """Tier 3: a 4x8 coarse index grid sampled at integral positions from a 5x9 output (Hc x Wc != H x W): pure indexing."""
    N, H, W, Hc, Wc = 2, 5, 9, 4, 8
    g = _gen(22)
    coarse = _index_image(N, Hc, Wc, 2)
    py = torch.randint(-1, Hc + 1, (N, H, W), generator=g)
    px = torch.randint(-1, Wc + 1, (N, H, W), generator=g)
    lx = torch.linspace(-1, 1, W, dtype=F64).view(1, 1, W)
    ly = torch.linspace(-1, 1, H, dtype=F64).view(1, H, 1)
    fd = _exact(torch.stack((_norm_coord(px.double(), Wc, False) - lx, _norm_coord(py.double(), Hc, False) - ly), 1))
    padded = np.zeros((N, Hc + 2, Wc + 2, 2), np.float32)
    padded[:, 1:-1, 1:-1] = coarse.numpy()
    ref = padded[np.arange(N)[:, None, None], py.numpy() + 1, px.numpy() + 1]
    f12, _, _ = ops.compose_flow(fd.to(dev), coarse.to(dev), out_hw=(H, W))
    assert np.array_equal(f12.cpu().numpy(), ref)


@gpu
@pytest.mark.parametrize("case", [(2, 3, 9, 17, 5, 9), (2, 175000, 3, 5, 2, 3)], ids=str)
def test_index_image_resize(dev, case):
    """Tier 3: align_corners with an integral scale 2: out[y, x] = in[2y, 2x]; N C Hout Wout beyond the cap in the second case."""
    N, C, Hi, Wi, Ho, Wo = case
    x = _index_image(N, C, Hi, Wi)
    assert N * C * Ho * Wo > CAP or C < 10
    got = ops.resize_bilinear(x.to(dev), (Ho, Wo), True).cpu().numpy()
    assert np.array_equal(got, x.numpy()[:, :, ::2, ::2])


@gpu
@pytest.mark.parametrize("cfg", MP_CFG, ids=str)
def test_index_image_maxpool(dev, cfg):
    """Tier 3: on an increasing index image the maximum is the window's last in-bounds element."""
    k, s, p = cfg
    N, C, H, W = 2, 3, 11, 14
    x = _index_image(N, C, H, W)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    iy = np.minimum(np.arange(Ho) * s - p + k - 1, H - 1)
    ix = np.minimum(np.arange(Wo) * s - p + k - 1, W - 1)
    assert np.array_equal(ops.maxpool2d(x.to(dev), k, s, p).cpu().numpy(), x.numpy()[:, :, iy[:, None], ix[None, :]])


def _np_blur(x, stride):
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")
    H, W = x.shape[2:]
    w = (0.25, 0.5, 0.25)
    acc = sum(w[i] * w[j] * xp[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3))
    return acc[:, :, ::stride, ::stride]


@gpu
@pytest.mark.parametrize("case", [(1, 11, 14), (2, 11, 14), (2, 10, 16), (3, 7, 12)], ids=str)
def test_index_image_blur_and_maxblur(dev, case):
    """Tier 3: nine shifted slices of the reflect-padded index image in numpy (exact: indices < 2^10, weights 2^-4); the max-pool of
    an increasing image is its lower-right neighbour.  H != W, N > 1, C > 1; 10x16 at stride 2 takes the register-blocked kernel."""
    s, H, W = case
    x = _index_image(2, 3, H, W)
    ref = _np_blur(x.numpy(), s)
    assert np.array_equal(ops.blurpool2d(x.to(dev), s).cpu().numpy().astype(np.float64), ref)
    refm = _np_blur(x.numpy()[:, :, 1:, 1:], s)
    aligned = ops.maxblurpool2d(x.to(dev), s)            # kept alive: the next output must not inherit its block
    assert np.array_equal(aligned.cpu().numpy().astype(np.float64), refm)
    flat = torch.empty(x.numel() + 1, device=dev)
    view = flat[1:].view(x.shape)
    view.copy_(x)                                                    # not 16-byte aligned: the per-output fall-back
    assert np.array_equal(ops.maxblurpool2d(view, s).cpu().numpy().astype(np.float64), refm)


@gpu
def test_index_image_avgpool_flow_grad_clamp_warp_grid(dev):
    """Tier 3 for the kernels without a gather: adaptive_avgpool2d to the input's own size is the identity; flow_grad_clamp with a
    zero grid is a (B,2,H,W) -> (B,H,W,2) transposition; warp_grid with pure translations is the identity grid shifted per image."""
    x = _index_image(2, 3, 5, 7)
    assert torch.equal(ops.adaptive_avgpool2d(x.to(dev), (5, 7)).cpu(), x)
    f = _index_image(3, 2, 5, 7) * 2.0 ** -8
    _, flow = ops.flow_grad_clamp(f.to(dev), torch.zeros(1, 5, 7, 2, device=dev), want_grad=False)
    assert np.array_equal(flow.cpu().numpy(), np.transpose(f.numpy(), (0, 2, 3, 1)))
    M = torch.eye(3).repeat(3, 1, 1)
    M[:, 0, 2] = torch.tensor([0.0, 1.0, -2.0])
    M[:, 1, 2] = torch.tensor([3.0, -1.0, 0.5])
    got = ops.warp_grid(M.to(dev), 5, 9).cpu().numpy()
    xs, ys = np.linspace(-1, 1, 9), np.linspace(-1, 1, 5)
    for b in range(3):
        assert np.array_equal(got[b, :, :, 0], np.broadcast_to(xs[None, :] + float(M[b, 0, 2]), (5, 9)))
        assert np.array_equal(got[b, :, :, 1], np.broadcast_to(ys[:, None] + float(M[b, 1, 2]), (5, 9)))


# ====================================================================== the families' invariants, without a device
def test_family_invariants_hold_on_the_host():
    """Every Tier 1 family and shape above: the float64 reference is a float32 number and ATen's float32 kernel returns its bits;
    every Tier 2 bound also holds for ATen's own float32 kernel.  A wrong family is found here and not on the device."""
    for c in GS_CASES:
        gs_build(c)
    for ac in (False, True):
        gs_nonfinite_build(ac)
    for c in GS_T2:
        gs_tier2_build(c)
    for c in RS_CASES:
        rs_build(c)
    for c in ((6, 8, 41, 67), (7, 5, 3, 11)):
        rs_tier2_build(c)
    for c in MP_CASES:
        mp_build(c)
    for c in BP_CASES:
        bp_build(c, False)
    for c in MB_CASES:
        bp_build(c, True)
    mb_cap_build()
    for hw in WG_SIZES + [(513, 1025)]:
        wg_build(hw[0], hw[1], 5 if hw[0] > 100 else 3)
    for hw in ((48, 64), (7, 5), (17, 33)):
        wg_tier2_build(*hw)
    for c in CF_CASES:
        cf_build(c)
    for clamp in (False, True):
        cf_up_build(clamp)
    cf_nonfinite_build()
    cf_clamp_nonfinite_build()
    for c in FG_CASES:
        fg_build(c)
    for c in AP_CASES:
        ap_build(c)
    for c in FH_CASES[1:]:
        lg, K, ref, acc, dom, is_dom, is_flat = fh_build(c)
        assert bool(is_dom.any()) and bool(is_flat.any()) and float(lg.abs().max()) == 30.0
    for C in (2, 150):
        sm_build(C)
