"""The two kernel families that decide every match -- csrc/corr.hip and csrc/mutual_nn.hip -- against float64, bit for bit, at
their tile edges, short channel counts and exact ties.

The idea is tests/test_gpu_pointwise_exact.py's Tier 1: operands come from families in which every product and every partial sum
is a multiple of one quantum below 2^24 quanta, so float32 arithmetic is exact and a correct kernel returns the float64 result
BIT FOR BIT whatever its summation order, chunking or fma contraction.  A dropped, duplicated or too-early-read channel chunk, a
wrong tap, plane, pixel or image, a border value that is not zero, or a tie resolved to another index is then a bit difference:
every comparison below is torch.equal, on values and on index lists, with no tolerance and no share of cases left out.

Each family checks its own invariant on the host before it is trusted (``_exact``): the float64 reference is representable in
float32 and the float32 CPU evaluation of the same formula returns the same bits.  The unmarked
``test_family_invariants_hold_on_the_host`` runs all of these checks, the non-vacuity counts of the tie family and the agreement
of this file's mutual-NN reference with oracle/restate.py::mutual_matching, without a device.

References are plain float64 torch / numpy written here; they call nothing in rfx and nothing in oracle/restate.py."""

import functools

import numpy as np
import pytest
import torch

from rfx import ops

gpu = pytest.mark.gpu
F64 = torch.float64
CAP = 8192 * 256                       # the plain correlation kernel's grid: 8192 workgroups of 256 threads, one pixel each
NAN = float("nan")


# ---------------------------------------------------------------------- helpers (as in tests/test_gpu_pointwise_exact.py)
def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _ints(g, shape, lo, hi, q=1.0):
    """multiples of q in [lo*q, hi*q]"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float() * q


def _exact(ref64, cpu32=None, what=""):
    """The family's invariant: the float64 result is a float32 number, and (where given) the float32 CPU evaluation returns its bits."""
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64), "family not exact: float64 reference is not representable in float32 " + what
    if cpu32 is not None:
        assert torch.equal(cpu32, ref32), "family not exact: float32 CPU evaluation differs from float64 " + what
    return ref32


def _where_bad(got, ref):
    d = (got.cpu() != ref.cpu()).nonzero()
    return "%d mismatches, first at %s" % (d.shape[0], d[:4].tolist())


def _same(got, ref, what):
    """torch.equal against the host reference.  The device result is then overwritten with NaN: a freed block is handed to the next
    output of its size with its values, and a kernel that writes nothing (or not everything) must not inherit right ones.  For the
    same reason no reference is ever copied to the device."""
    g = got.cpu()
    got.fill_(NAN)
    assert g.shape == ref.shape, (what, tuple(g.shape), tuple(ref.shape))
    assert torch.equal(g, ref), "%s: %s" % (what, _where_bad(g, ref))


# ====================================================================== A. correlation
def _corr64(x, y, dtype=F64):
    """out[n, i*7+j, r, c] = sum_ch x[n,ch,r,c] * y[n,ch,r+i-3,c+j-3], y zero outside the image: 49 shifted slice products."""
    x, y = x.to(dtype), y.to(dtype)
    N, C, H, W = x.shape
    out = torch.zeros(N, 49, H, W, dtype=dtype)
    for i in range(7):
        for j in range(7):
            dy, dx = i - 3, j - 3
            r0, r1, c0, c1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if r0 < r1 and c0 < c1:
                out[:, i * 7 + j, r0:r1, c0:c1] = (x[:, :, r0:r1, c0:c1] * y[:, :, r0 + dy:r1 + dy, c0 + dx:c1 + dx]).sum(1)
    return out


def _corr64_at(x, y, n, r, c, dtype=F64):
    """_corr64 at the pixels (n[k], r[k], c[k]) only -> (P, 49); for the one case whose whole volume is too large for the host."""
    N, C, H, W = x.shape
    xv = x[n, :, r, c].to(dtype)
    out = torch.zeros(n.numel(), 49, dtype=dtype)
    for i in range(7):
        for j in range(7):
            rr, cc = r + (i - 3), c + (j - 3)
            ok = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
            out[ok, i * 7 + j] = (xv[ok] * y[n[ok], :, rr[ok], cc[ok]].to(dtype)).sum(1)
    return out


def corr_inputs(kind, N, C, H, W):
    """taps: x = (1, 0, 0 ..), y[:, 0] = 1 + the pixel's flat index over the whole batch (< 2^24), the other y channels random
    integers that must not leak: the volume is a pure gather that pins every plane, pixel, border zero and image index.
    sums: every channel of x and y holds integers in [-4, 4] / 8: products are multiples of 2^-6, |sum| <= C / 4."""
    g = _gen(31, kind == "taps", N, C, H, W)
    if kind == "taps":
        assert N * H * W < 2 ** 24
        x = torch.zeros(N, C, H, W)
        x[:, 0] = 1.0
        y = _ints(g, (N, C, H, W), -8, 8)
        y[:, 0] = (torch.arange(N * H * W, dtype=torch.float32) + 1).view(N, H, W)
        return x, y
    assert kind == "sums"
    return _ints(g, (N, C, H, W), -4, 4, 0.125), _ints(g, (N, C, H, W), -4, 4, 0.125)


@functools.lru_cache(maxsize=24)
def corr_case(kind, N, C, H, W, both=False):
    """(x, y, corr(x, y)[, corr(y, x)]) -- the references checked by ``_exact``"""
    x, y = corr_inputs(kind, N, C, H, W)
    what = "(%s %s)" % (kind, (N, C, H, W))
    ref12 = _exact(_corr64(x, y), _corr64(x, y, torch.float32), what)
    if kind == "taps":                                               # the gather it is meant to be
        assert torch.equal(ref12[:, 24], y[:, 0]) and torch.equal(ref12[:, 0, 3:, 3:], y[:, 0, :H - 3, :W - 3])
        assert H < 4 or bool((ref12[:, 0, :3] == 0).all())
    if not both:
        return x, y, ref12
    return x, y, ref12, _exact(_corr64(y, x), _corr64(y, x, torch.float32), what + " reversed")


VARIANTS = (1, 2, 3, 5, 7, 8)          # 64x16, 32x16, 16x16 plain tiles; 16x80, 16x48, 16x64 tuned tiles
ONE_SHAPES = [(1, 1, 4), (3, 15, 12), (2, 17, 20), (1, 33, 52), (3, 16, 48), (1, 65, 84), (2, 7, 164), (11, 9, 100)]
FULL_C = ((2, 17, 20), (1, 33, 52))
SUM_C = (2, 4, 6, 8, 10, 256)          # 1 .. 5 chunks of 2 channels against ring depths 3 (plain) and 4 (tuned), + the product's


def one_dir_inputs(shape):
    return [("taps", 2), ("sums", 6)] + ([("sums", C) for C in SUM_C if C != 6] if shape in FULL_C else [])


@gpu
@pytest.mark.parametrize("shape", ONE_SHAPES, ids=str)
def test_corr_neigh_every_variant_is_float64_bit_for_bit(dev, shape):
    """Every tile configuration forced on every shape: one pixel row of one quad; maps smaller than, equal to and ragged against
    the 16 / 32 / 64-row and 16 / 48 / 64 / 80-column tiles in both directions; several images; workgroup counts that are no
    multiple of 8 (the XCD remap must stay a bijection).  taps pins the routing; sums with C = 6 (3 chunks = the plain ring's
    depth), and at two shapes with C = 2 .. 10 and 256, pins the ring: 1 .. 5 chunks against depths 3 and 4 -- shorter than,
    equal to and longer than the prologue -- where a chunk that is dropped, doubled or read before it landed changes an exact sum."""
    N, H, W = shape
    for kind, C in one_dir_inputs(shape):
        x, y, ref = corr_case(kind, N, C, H, W)
        xd, yd = x.to(dev), y.to(dev)
        for v in VARIANTS:
            _same(ops.corr_neigh(xd, yd, variant=v), ref, "%s C=%d variant %d" % (kind, C, v))


# auto_variant() of csrc/corr.hip, restated: with r16 = ceil(H / 16), a map wider than 32 columns whose launch would have
# N * r16 * ceil(W / 80) >= 128 workgroups takes the tuned tile -- 80, 64 or 48 columns wide, whichever pads W least, the widest
# on ties (variants 5, 8, 7).  Every other map takes 16-column plain tiles, as tall as still gives 1024 workgroups: 64 rows
# (variant 1) if N * ceil(H / 64) * ceil(W / 16) >= 1024, else 32 rows (2) under the same test, else 16 rows (3).
def _auto_variant(N, H, W):
    up = lambda a, b: -(-a // b)
    if W > 32 and N * up(H, 16) * up(W, 80) >= 128:
        best, best_w = 5, 1 << 30
        for ncb in (5, 4, 3):
            if up(W, 16 * ncb) * 16 * ncb < best_w:
                best, best_w = ncb, up(W, 16 * ncb) * 16 * ncb
        return {5: 5, 4: 8, 3: 7}[best]
    tc = up(W, 16)
    return 1 if N * up(H, 64) * tc >= 1024 else (2 if N * up(H, 32) * tc >= 1024 else 3)


# (N, H, W) -> the variant the two-direction entry (which has no variant argument) picks
BIDIR_SHAPES = {(32, 17, 156): 5, (32, 17, 100): 8, (32, 17, 84): 7, (512, 5, 20): 1, (512, 33, 8): 2, (2, 17, 24): 3}
BIDIR_INPUTS = (("taps", 2), ("sums", 6))


def _bidir(dev, x, y):
    N, _, H, W = x.shape
    out = torch.full((2 * N, 49, H, W), NAN, device=dev)            # NaN: an element that is not written cannot compare equal
    o12, o21 = ops.corr_neigh_bidir(x.to(dev), y.to(dev), out=out)
    assert o12.data_ptr() == out.data_ptr() and o21.data_ptr() == out[N:].data_ptr()
    return out[:N], out[N:]


@gpu
@pytest.mark.parametrize("shape", list(BIDIR_SHAPES), ids=str)
def test_corr_neigh_bidir_both_directions_are_float64_bit_for_bit(dev, shape):
    """The two-direction form of all six configurations (shapes chosen from the restated auto_variant rule; the host test asserts
    the map): out12 == corr64(x, y) and out21 == corr64(y, x), into a buffer that starts as NaN, so every element of the mirrored
    store -- shifted pixels, mirrored planes and the zeros its owner lane writes -- is shown to be written, and written once with
    the right value.  taps runs in both operand orders: as (x, y) it pins out12's gather, as (y, x) out21's."""
    N, H, W = shape
    for kind, C in BIDIR_INPUTS:
        x, y, ref12, ref21 = corr_case(kind, N, C, H, W, True)
        o12, o21 = _bidir(dev, x, y)
        _same(o12, ref12, "%s out12" % kind)
        _same(o21, ref21, "%s out21" % kind)
        if kind == "taps":
            o12, o21 = _bidir(dev, y, x)
            _same(o12, ref21, "taps swapped out12")
            _same(o21, ref12, "taps swapped out21")


# The plain one-thread-per-pixel kernel serves whatever the 16-byte DMA path cannot (dma_ok in csrc/corr.hip): an odd channel
# count, a width that is no multiple of 4 (reached through an explicit variant: without one ops.corr_neigh pads the width), or a
# base pointer that is not 16-byte aligned.
PLAIN_CASES = [("odd-C", 2, 3, 9, 12), ("W%4", 2, 4, 9, 11), ("x-misaligned", 1, 4, 9, 12), ("y-misaligned", 1, 4, 9, 12)]


def _off_by_one_float(t, dev):
    flat = torch.empty(t.numel() + 1, device=dev)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@gpu
@pytest.mark.parametrize("case", PLAIN_CASES, ids=str)
def test_corr_neigh_plain_fallback_is_float64_bit_for_bit(dev, case):
    """C = 3; W = 11 with an explicit variant; x, then y, as a view one float (4 bytes) off a 16-byte aligned buffer: each alone
    sends the call to the plain kernel.  Both families."""
    what, N, C, H, W = case
    for kind in ("taps", "sums"):
        x, y, ref = corr_case(kind, N, C, H, W)
        xd, yd = x.to(dev), y.to(dev)
        if what == "x-misaligned":
            xd = _off_by_one_float(x, dev)
        if what == "y-misaligned":
            yd = _off_by_one_float(y, dev)
        got = ops.corr_neigh(xd, yd, variant=3 if what == "W%4" else None)
        _same(got, ref, "%s %s" % (what, kind))


CAP_SHAPE = (2, 1, 1025, 1028)
assert CAP < CAP_SHAPE[0] * CAP_SHAPE[2] * CAP_SHAPE[3] < 2 ** 24


@functools.lru_cache(maxsize=1)
def corr_cap_case():
    """taps with C = 1 on 2 x 1025 x 1028 = 2 107 400 pixels.  Reference at: the first and last 4 rows and columns of both images,
    the 16 pixels around flat index 2^21 (where the grid-stride loop starts its second trip) and 4096 seeded pixels."""
    N, C, H, W = CAP_SHAPE
    x, y = corr_inputs("taps", N, C, H, W)
    edge_r = torch.cat((torch.arange(4), torch.arange(H - 4, H)))
    edge_c = torch.cat((torch.arange(4), torch.arange(W - 4, W)))
    pts = [torch.cartesian_prod(torch.arange(N), edge_r, torch.arange(W)), torch.cartesian_prod(torch.arange(N), torch.arange(H), edge_c)]
    flat = torch.cat((torch.arange(CAP - 8, CAP + 8), torch.randint(0, N * H * W, (4096,), generator=_gen(32))))
    pts.append(torch.stack((flat // (H * W), flat % (H * W) // W, flat % W), 1))
    n, r, c = torch.cat(pts).unbind(1)
    ref = _exact(_corr64_at(x, y, n, r, c), _corr64_at(x, y, n, r, c, torch.float32), "(cap)")
    return x, y, (n, r, c), ref


@gpu
def test_corr_neigh_plain_fallback_beyond_its_grid_cap(dev):
    """C = 1 is odd: the plain kernel, whose grid is capped at 8192 x 256 threads -- the last 10 248 pixels are a thread's second
    trip of the grid-stride loop, where a stale image, row or column index would show.  The volume (413 MB) stays on the device;
    the sampled pixels are gathered there."""
    x, y, (n, r, c), ref = corr_cap_case()
    got = ops.corr_neigh(x.to(dev), y.to(dev))
    assert tuple(got.shape) == (CAP_SHAPE[0], 49) + CAP_SHAPE[2:]
    _same(got[n.to(dev), :, r.to(dev), c.to(dev)], ref, "cap")


GROUP_BIDIR = [(2, 17, 24), (32, 17, 100), (32, 17, 84)]             # variants 3, 8, 7 in one recorded group
GROUP_ONE = [("sums", 2, 4, 9, 11), ("sums", 3, 6, 15, 12), ("taps", 1, 2, 33, 52), ("sums", 2, 6, 7, 164)]   # W = 11: padded, cropped


@gpu
def test_corr_neigh_groups_are_float64_bit_for_bit(dev):
    """corr_neigh_bidir_group: three problems of three variants recorded in one launch group (blockIdx.y selects the problem, the
    XCD remap runs on the problem's own workgroup count), into NaN-filled buffers; corr_neigh_group: four problems, one of them
    of width 11, which is zero-padded before the group and cropped after it.  All against float64."""
    for kind, C in BIDIR_INPUTS:
        cases = [corr_case(kind, N, C, H, W, True) for (N, H, W) in GROUP_BIDIR]
        outs = [torch.full((2 * c[0].shape[0], 49) + tuple(c[0].shape[2:]), NAN, device=dev) for c in cases]
        res = ops.corr_neigh_bidir_group([c[0].to(dev) for c in cases], [c[1].to(dev) for c in cases], outs=outs)
        for k, ((o12, o21), c) in enumerate(zip(res, cases)):
            assert o12.data_ptr() == outs[k].data_ptr()
            _same(o12, c[2], "group %s problem %d out12" % (kind, k))
            _same(o21, c[3], "group %s problem %d out21" % (kind, k))
    cases = [corr_case(*g) for g in GROUP_ONE]
    res = ops.corr_neigh_group([c[0].to(dev) for c in cases], [c[1].to(dev) for c in cases])
    for k, (o, c) in enumerate(zip(res, cases)):
        _same(o, c[2], "one-direction group problem %d" % k)


# ====================================================================== B. mutual nearest neighbours
def _mnn64(A, B, mask=None):
    """S = A^T (B mask) in float64; row and column arg-max with the FIRST index on ties (numpy.argmax); (i, j = row_arg[i]) is
    kept iff col_arg[j] == i and float32(S[i, j])^2 > 0 evaluated in float32; pairs listed by ascending i."""
    Bm = B.double() if mask is None else B.double() * mask.double()[None, :]
    S = (A.double().t() @ Bm).numpy()
    if S.shape[0] == 0 or S.shape[1] == 0:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    row_arg, col_arg = S.argmax(axis=1), S.argmax(axis=0)
    i = np.arange(S.shape[0])
    v = S[i, row_arg].astype(np.float32)
    keep = (col_arg[row_arg] == i) & (v * v > np.float32(0))
    return torch.from_numpy(i[keep]).long(), torch.from_numpy(row_arg[keep]).long()


DUP_A, DUP_B = (1, 4, 32, 64, 128, 129), (1, 32, 128, 200)


def _pm1(g, shape):
    return (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1).float()


def mnn_inputs(C, nA, nB, seed=0):
    """rademacher: entries +-1 -- every column has squared norm exactly C, a copy scores exactly C, every score is an integer of
    magnitude <= C.  B = copies of random A columns, 30 % of them replaced by unrelated columns.  Exact ties come from duplicated
    columns: A[:, i+d] = A[:, i] for d in DUP_A at every 37th i, B[:, j+d] = B[:, j] for d in DUP_B at every 29th j -- strides that
    put the two tied indices into the same lane's registers (4: rows; 32: the lane's second column), into neighbouring lanes (1),
    across the xor-32 lanes and the two wave rows / columns (32, 64) and across 128-wide tiles (128, 129, 200).  A few all-zero
    columns on both sides tie whole rows / columns at score 0.  mask: 0/1, 70 % ones."""
    g = _gen(41, C, nA, nB, seed)
    A = _pm1(g, (C, nA))
    for d in DUP_A:
        for i in range(0, nA - d, 37):
            A[:, i + d] = A[:, i]
    B = A[:, torch.randint(nA, (nB,), generator=g)].clone()
    noise = torch.rand(nB, generator=g) < 0.3
    B[:, noise] = _pm1(g, (C, int(noise.sum())))
    for d in DUP_B:
        for j in range(0, nB - d, 29):
            B[:, j + d] = B[:, j]
    if nA >= 64:
        A[:, 11::61] = 0.0
    if nB >= 64:
        B[:, 17::47] = 0.0
    mask = (torch.rand(nB, generator=g) < 0.7).float()
    return A, B, mask


def _mnn_exact(A, B, mask, what):
    """The family's invariant for one (A, B, mask): float32 scores are the float64 scores, and the float32 list is the float64 list."""
    Bm32 = B if mask is None else B * mask[None, :]
    S64 = A.double().t() @ Bm32.double()
    _exact(S64, A.t() @ Bm32, what)
    ref = _mnn64(A, B, mask)
    S32 = (A.t() @ Bm32).numpy()
    if S32.size:
        ra, ca, i = S32.argmax(1), S32.argmax(0), np.arange(S32.shape[0])
        v = S32[i, ra]
        keep = (ca[ra] == i) & (v * v > np.float32(0))
        assert np.array_equal(i[keep], ref[0].numpy()) and np.array_equal(ra[keep], ref[1].numpy()), "float32 list differs " + what
    return ref


@functools.lru_cache(maxsize=64)
def mnn_case(C, nA, nB, seed=0):
    """A, B, mask and the three reference lists (no mask, the 0/1 mask, the all-zero mask).  Non-vacuity: with nA, nB >= 127 at
    least 5 matches of the unmasked list lie on a row whose maximum is tied and at least 5 on a column whose maximum is tied."""
    A, B, mask = mnn_inputs(C, nA, nB, seed)
    what = "(mnn %s)" % ((C, nA, nB, seed),)
    zero = torch.zeros(nB)
    refs = {"none": _mnn_exact(A, B, None, what), "mask": _mnn_exact(A, B, mask, what + " masked"),
            "zero": _mnn_exact(A, B, zero, what + " all-zero mask")}
    assert len(refs["zero"][0]) == 0
    S = A.double().t() @ B.double()
    tied_r = (S == S.max(1, keepdim=True).values).sum(1) > 1
    tied_c = (S == S.max(0, keepdim=True).values).sum(0) > 1
    i1, i2 = refs["none"]
    counts = (len(i1), int(tied_r[i1].sum()), int(tied_c[i2].sum()))
    if nA >= 127 and nB >= 127:
        assert counts[1] >= 5 and counts[2] >= 5, "tie family is vacuous %s: %s" % (what, counts)
    return dict(A=A, B=B, mask=mask, zero=zero, refs=refs, counts=counts)


MNN_SIZES = [(64, 300, 260), (1024, 531, 300), (96, 130, 129), (40, 257, 127), (32, 1, 5), (64, 5, 1), (64, 127, 128), (64, 128, 129),
             (64, 2107, 300), (64, 300, 1100)]
FORMS = ("0", "1")                     # RFX_MNN_FORM: 0 = k-major tile kernel where C % 32 == 0 and C >= 64; 1 = transposed-image kernel


def _list_equal(got, ref, what):
    """Both index lists equal the float64 ones.  Device lists are overwritten afterwards, as in ``_same``: the next call of the
    same size gets the same blocks for its index buffers."""
    g1, g2 = got[0].cpu(), got[1].cpu()
    for t in got:
        if t.is_cuda:
            t.fill_(-1)
    assert torch.equal(g1, ref[0]) and torch.equal(g2, ref[1]), \
        "%s: got %d matches, float64 has %d; first differing %s" % (what, len(g1), len(ref[0]), _first_diff(g1, g2, ref))


def _first_diff(g1, g2, ref):
    a, b = list(zip(g1.tolist(), g2.tolist())), list(zip(ref[0].tolist(), ref[1].tolist()))
    return next(((k, x, y) for k, (x, y) in enumerate(zip(a + [None] * len(b), b + [None] * len(a))) if x != y), None)


@gpu
@pytest.mark.parametrize("size", MNN_SIZES, ids=str)
def test_mutual_nn_exact_ties_resolve_to_the_first_index(dev, size, monkeypatch):
    """Both kernel forms, without a mask, with a 0/1 mask and with an all-zero mask (no match: every score ties at 0 and the
    v * v > 0 test drops the one mutual pair).  C = 64, 96, 1024: k-major form under RFX_MNN_FORM=0; C = 40 and 32: the
    transposed-image form under either setting, with its C % 32 != 0 tail at 40.  Unpadded matrices: float4 staging where nA and
    nB are multiples of 4 (300 x 260, 300 x 1100), scalar staging elsewhere.  1 x 5 and 5 x 1: a single row / column;
    127 / 128 / 129: a tile edge; 2107 x 300 and 300 x 1100: 17 and 9 tiles whose partial maxima the reduction joins."""
    C, nA, nB = size
    c = mnn_case(C, nA, nB)
    Ad, Bd = c["A"].to(dev), c["B"].to(dev)
    for form in FORMS:
        monkeypatch.setenv("RFX_MNN_FORM", form)
        for key, m in (("none", None), ("mask", c["mask"]), ("zero", c["zero"])):
            got = ops.mutual_nn(Ad, Bd, None if m is None else m.to(dev))
            _list_equal(got, c["refs"][key], "form %s, mask %s" % (form, key))


def _ld(n, vec):
    """a padded leading dimension: the next multiple of 4 plus 4 (float4 staging) or an n + 3 / n + 1 that is no multiple of 4"""
    return (n + 3) // 4 * 4 + 4 if vec else (n + 3 if (n + 3) % 4 else n + 1)


def _padded(M, ld, dev):
    P = torch.full((M.shape[0], ld), NAN, device=dev)
    P[:, :M.shape[1]] = M.to(dev)
    return P


@gpu
@pytest.mark.parametrize("vec", [True, False], ids=["pad4-float4", "pad3-scalar"])
@pytest.mark.parametrize("size", [(64, 300, 260), (96, 130, 129)], ids=str)
def test_mutual_nn_padded_leading_dimension_with_nan_padding(dev, size, vec, monkeypatch):
    """Both matrices in (C, ld) storage whose padding columns hold NaN -- they may only reach rows / columns the arg-max skips.
    float4 staging needs both leading dimensions to be multiples of 4: 304 / 264 (pad 4) and 136 / 136; scalar staging takes the
    others: 303 / 263 (pad 3) and 133 / 130."""
    C, nA, nB = size
    c = mnn_case(C, nA, nB)
    ldA, ldB = _ld(nA, vec), _ld(nB, vec)
    assert (ldA % 4 == 0 and ldB % 4 == 0) if vec else (ldA % 4 != 0 and ldB % 4 != 0)
    Ap, Bp = _padded(c["A"], ldA, dev), _padded(c["B"], ldB, dev)
    for form in FORMS:
        monkeypatch.setenv("RFX_MNN_FORM", form)
        for key, m in (("none", None), ("mask", c["mask"])):
            got = ops.mutual_nn(Ap, Bp, None if m is None else m.to(dev), ldA=ldA, ldB=ldB, nA=nA, nB=nB)
            _list_equal(got, c["refs"][key], "form %s, mask %s, ld %d / %d" % (form, key, ldA, ldB))


@gpu
@pytest.mark.parametrize("size", [(96, 130, 129), (1024, 531, 300)], ids=str)
def test_mutual_nn_every_score_chunk_returns_the_float64_list(dev, size, monkeypatch):
    """score_chunk 0 (256 products), -1 (one chain), 32, 64, 1024: the sums are exact, so every chunking of both forms returns the
    same list -- a chunk that is closed twice or not at all does not."""
    C, nA, nB = size
    c = mnn_case(C, nA, nB)
    Ad, Bd, md = c["A"].to(dev), c["B"].to(dev), c["mask"].to(dev)
    for form in FORMS:
        monkeypatch.setenv("RFX_MNN_FORM", form)
        for chunk in (0, -1, 32, 64, 1024):
            _list_equal(ops.mutual_nn(Ad, Bd, score_chunk=chunk), c["refs"]["none"], "form %s chunk %d" % (form, chunk))
            _list_equal(ops.mutual_nn(Ad, Bd, md, score_chunk=chunk), c["refs"]["mask"], "form %s chunk %d masked" % (form, chunk))


@functools.lru_cache(maxsize=1)
def mnn_sign_cases():
    """(name, A, B, reference list) for the v * v > 0 rule.  A score whose square is subnormal is deliberately not pinned."""
    a = _pm1(_gen(42), (64, 1))
    neg = _mnn_exact(a, -a, None, "(negative)")
    assert neg[0].tolist() == [0] and neg[1].tolist() == [0]                   # the score is -64: kept, its square is positive
    c = mnn_case(64, 300, 260)
    A, B = c["A"], c["B"]
    tiny = _mnn_exact(A * 2.0 ** -50, B * 2.0 ** -50, None, "(2^-50)")
    assert len(tiny[0]) == 0 and float((A.double().t() @ B.double()).abs().max()) * 2.0 ** -100 == 2.0 ** -94
    small = _mnn_exact(A * 2.0 ** -20, B * 2.0 ** -20, None, "(2^-20)")
    assert torch.equal(small[0], c["refs"]["none"][0]) and torch.equal(small[1], c["refs"]["none"][1]) and len(small[0]) > 10
    S = (A.double().t() @ B.double())[small[0], small[1]]
    assert float(S.abs().min()) >= 1 and (float(S.abs().min()) * 2.0 ** -40) ** 2 >= 2.0 ** -126     # the squares are normal
    return [("negative", a, -a, neg), ("2^-50", A * 2.0 ** -50, B * 2.0 ** -50, tiny), ("2^-20", A * 2.0 ** -20, B * 2.0 ** -20, small)]


@gpu
def test_mutual_nn_sign_and_underflow_of_the_square_test(dev, monkeypatch):
    """nA = nB = 1 with B = -A: the score is -C and the match is kept (the rule is v * v > 0, not v > 0).  Features scaled by
    2^-50: the largest score is 2^-94, every square underflows to 0, no match.  Scaled by 2^-20: squares are normal numbers and
    the list is the unscaled one."""
    for name, A, B, ref in mnn_sign_cases():
        for form in FORMS:
            monkeypatch.setenv("RFX_MNN_FORM", form)
            _list_equal(ops.mutual_nn(A.to(dev), B.to(dev)), ref, "%s form %s" % (name, form))


def _batched(dev, fA, ldA, nA, fB, nB, C, mask, batch):
    """rfx_mutual_nn_batched_f32 with the argument layout of rfx/pipeline.py::_mutual_batched"""
    from rfx import _lib
    ws = torch.empty(batch * _lib.load().rfx_mutual_nn_ws_bytes(nA, nB), dtype=torch.uint8, device=dev)
    cap = min(nA, nB)
    idx1 = torch.full((batch, cap), -1, dtype=torch.int64, device=dev)
    idx2 = torch.full((batch, cap), -1, dtype=torch.int64, device=dev)
    count = torch.zeros(batch, dtype=torch.int32, device=dev)
    ops._call("rfx_mutual_nn_batched_f32", ops._one_device(fA, fB, mask), ops._p(fA), ldA, nA, C * ldA, ops._p(fB), nB, nB, C * nB, C,
              ops._p(mask), ops._p(idx1), ops._p(idx2), ops._p(count), ops._p(ws), batch, 0)
    return idx1.cpu(), idx2.cpu(), count.cpu()


@gpu
@pytest.mark.parametrize("size", [(64, 257, 130), (64, 260, 132)], ids=str)
def test_mutual_nn_batched_dense_entry_equals_float64_per_pair(dev, size, monkeypatch):
    """The entry the production pipeline calls: three pairs of one size in one launch (blockIdx.y = the pair), features (3, C, n)
    and a (3, nB) mask; 257 x 130 stages with scalar loads, 260 x 132 with float4; both forms, with and without the mask."""
    C, nA, nB = size
    cs = [mnn_case(C, nA, nB, seed) for seed in (1, 2, 3)]
    fA, fB = torch.stack([c["A"] for c in cs]).to(dev), torch.stack([c["B"] for c in cs]).to(dev)
    mask = torch.stack([c["mask"] for c in cs]).to(dev)
    for form in FORMS:
        monkeypatch.setenv("RFX_MNN_FORM", form)
        for key, m in (("none", None), ("mask", mask)):
            idx1, idx2, count = _batched(dev, fA, nA, nA, fB, nB, C, m, 3)
            for b, c in enumerate(cs):
                n = int(count[b])
                _list_equal((idx1[b, :n], idx2[b, :n]), c["refs"][key], "pair %d form %s mask %s" % (b, form, key))


RAGGED_PAIRS = [(300, 260), (129, 128), (1, 5), (0, 7)]


@gpu
@pytest.mark.parametrize("vec", [True, False], ids=["float4", "scalar"])
def test_mutual_nn_ragged_entry_equals_float64_per_pair(dev, vec):
    """Four pairs of different sizes on one padded layout (everything beyond a pair's own columns is NaN, the mask's padding
    too), C = 64, with and without a mask; a pair with nA = 0 gives count 0."""
    C = 64
    ldA, ldB = _ld(300, vec), _ld(260, vec)
    cs = [mnn_case(C, nA, nB) if nA else None for nA, nB in RAGGED_PAIRS]
    fA = torch.full((len(cs), C, ldA), NAN, device=dev)
    fB = torch.full((len(cs), C, ldB), NAN, device=dev)
    mask = torch.full((len(cs), ldB), NAN, device=dev)
    for b, (c, (nA, nB)) in enumerate(zip(cs, RAGGED_PAIRS)):
        if c is not None:
            fA[b, :, :nA], fB[b, :, :nB], mask[b, :nB] = c["A"].to(dev), c["B"].to(dev), c["mask"].to(dev)
    nA = torch.tensor([p[0] for p in RAGGED_PAIRS], dtype=torch.int32, device=dev)
    nB = torch.tensor([p[1] for p in RAGGED_PAIRS], dtype=torch.int32, device=dev)
    for key, m in (("none", None), ("mask", mask)):
        d1, d2, count = ops.mutual_nn_ragged(fA, fB, nA, nB, maxNA=300, maxNB=260, maskB=m)
        idx1, idx2, count = d1.cpu(), d2.cpu(), count.cpu()
        d1.fill_(-1), d2.fill_(-1)                                   # (see _list_equal)
        for b, c in enumerate(cs):
            n = int(count[b])
            if c is None:
                assert n == 0
            else:
                _list_equal((idx1[b, :n], idx2[b, :n]), c["refs"][key], "pair %d mask %s" % (b, key))


# ====================================================================== every family's invariants, without a device
def test_family_invariants_hold_on_the_host():
    """Builds every input family of this file: each builder asserts that its float64 reference is a float32 number and that the
    float32 CPU evaluation returns the same bits; the mutual-NN builders also assert the non-vacuity counts.  Further: the shapes
    of the two-direction test reach all six configurations under the restated auto_variant rule; the pointwise correlation
    reference agrees with the full one; and this file's mutual-NN reference agrees with oracle/restate.py::mutual_matching -- the
    function pinned on the reference project -- on every mutual-NN input, exact ties included."""
    for shape in ONE_SHAPES:
        for kind, C in one_dir_inputs(shape):
            corr_case(kind, shape[0], C, shape[1], shape[2])
    assert {(_auto_variant(*s)) for s in BIDIR_SHAPES} == set(VARIANTS)
    for shape, v in BIDIR_SHAPES.items():
        assert _auto_variant(*shape) == v and shape[2] % 4 == 0
        for kind, C in BIDIR_INPUTS:
            corr_case(kind, shape[0], C, shape[1], shape[2], True)
    assert len({_auto_variant(*s) for s in GROUP_BIDIR}) >= 2 and all(s in BIDIR_SHAPES for s in GROUP_BIDIR)
    for what, N, C, H, W in PLAIN_CASES:
        assert C % 2 == 1 or W % 4 != 0 or "misaligned" in what
        for kind in ("taps", "sums"):
            corr_case(kind, N, C, H, W)
    for g in GROUP_ONE:
        corr_case(*g)
    x, y, (n, r, c), ref = corr_cap_case()
    assert bool((n * CAP_SHAPE[2] * CAP_SHAPE[3] + r * CAP_SHAPE[3] + c >= CAP).any())
    xs, ys, full = corr_case("sums", 2, 3, 9, 12)
    pts = torch.cartesian_prod(torch.arange(2), torch.arange(9), torch.arange(12))
    assert torch.equal(_corr64_at(xs, ys, *pts.unbind(1)), full.double().permute(0, 2, 3, 1).reshape(-1, 49))

    import restate
    seen = []
    for size in MNN_SIZES + [(64, nA, nB) for nA, nB in RAGGED_PAIRS if nA]:
        seen.append(mnn_case(*size))
    for size in ((64, 257, 130), (64, 260, 132)):
        seen.extend(mnn_case(*size, seed) for seed in (1, 2, 3))
    for c in seen:
        for key, m in (("none", None), ("mask", c["mask"]), ("zero", c["zero"])):
            Bm = c["B"] if m is None else c["B"] * m[None, :]
            r1, r2 = restate.mutual_matching(c["A"], Bm)
            assert torch.equal(r1, c["refs"][key][0]) and torch.equal(r2, c["refs"][key][1]), key
    for name, A, B, ref in mnn_sign_cases():
        r1, r2 = restate.mutual_matching(A, B)
        assert torch.equal(r1, ref[0]) and torch.equal(r2, ref[1]), name
    print("matches / on a tied row / on a tied column:", {s: mnn_case(*s)["counts"] for s in MNN_SIZES})
