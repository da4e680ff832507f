"""The kernels that turn matches into a result -- csrc/ransac.hip (with dlt.h), csrc/cc.hip and csrc/multih.hip -- against plain
numpy / float64 references written here, at their edges, ties and thresholds.

A. ransac.hip.  The reprojection error is emulated in float32 STEP BY STEP (``err_ref``): fl32(x2*H0), two fused multiply-adds per
   row (``fma32``: the product formed exactly in float64, added with TwoSum, the error term deciding a float32 halfway case -- an
   exact fma, checked against rationals), the IEEE divide, two subtractions, two squares, one add, and numpy's correctly rounded
   float32 sqrt.  The kernel's root is the bare v_sqrt_f32, whose documented accuracy is 1 ulp: ops.prediction must lie within
   1 ulp(e) of the reference e, NaN and +-inf as the reference has them.  Inlier counts, masks, winners and statuses are compared
   EXACTLY, on families that hold no error within 2 ulp(tol) of tol (``no_band``: asserted, no case left out), with H the device's
   own float32 H read back and the determinant gate taken from the host build of dlt.h -- DLT precision is not mixed in.  The search
   (duplicate filter, chunks of 100 in filtered order, zero-chunk abort, first maximum) is ``search_ref``, a dozen lines over the
   reference counts.  An equality family (a pure translation, whose unit-norm H is dyadic; matches on a lattice; offsets from
   Pythagorean triples) makes every step exact and puts ``e`` at, two ulps above and two ulps below tol.  The device DLT must be
   the host build of the same header bit for bit.
B. cc.hip against label propagation (``cc_ref``): label = flat index, a 3x3 minimum over the foreground until nothing changes.
   Outputs are compared as bit patterns.
C. multih.hip: keep_cell against ATen's align_corners=False formula in float64 on binary maps with power-of-two ratios (exact),
   and against a float32 emulation elsewhere (no cell within 4 ulp of 0.5, asserted); the ordered compaction across 1024-item
   trips; the accept gain bit-equal to float32(float64(sum) / HW) on sums that are exact; every comparison placed at equality.

Each family checks its own preconditions on the host before it is trusted; the unmarked ``test_family_invariants_hold_on_the_host``
runs all of them without a device.  References call nothing in rfx and nothing in oracle/restate.py (the host test alone compares
``cc_ref`` with restate, and reads ops.cc_max_area, which is host code).  ``_same`` overwrites every device result after comparing
it, and no reference is ever copied to the device."""

import ctypes
import functools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from rfx import ops

gpu = pytest.mark.gpu
F32 = np.float32
NAN = float("nan")
VP = ctypes.c_void_p


# ---------------------------------------------------------------------- helpers (as in tests/test_gpu_match_exact.py)
def _where_bad(g, ref):
    d = (g != ref).nonzero()
    return "%d mismatches, first at %s" % (d.shape[0], d[:4].tolist())


def _same(got, ref, what):
    """torch.equal against the host reference.  The device result is then overwritten (NaN, or -1 / 1 in integer and boolean
    tensors): a freed block is handed to the next output of its size with its values, and a kernel that writes nothing (or not
    everything) must not inherit right ones.  For the same reason no reference is ever copied to the device."""
    g = got.cpu()
    if got.is_floating_point():
        got.fill_(NAN)
    elif got.dtype == torch.bool:
        got.fill_(True)
    else:
        got.fill_(-1)
    ref = torch.as_tensor(ref)
    assert g.shape == ref.shape and g.dtype == ref.dtype, (what, tuple(g.shape), g.dtype, tuple(ref.shape), ref.dtype)
    assert torch.equal(g, ref), "%s: %s" % (what, _where_bad(g, ref))


def _same_bits(got, ref_bits, what):
    """float32 device tensor against a reference given as int32 bit patterns (NaN payloads and the sign of zero included)"""
    _same(got.view(torch.int32), torch.from_numpy(np.ascontiguousarray(ref_bits).view(np.int32)), what)


def _exact(ref64, cpu32, what):
    """The invariant of an exact family: the float64 evaluation is a float32 number, and the float32 evaluation returns its bits."""
    ref64, cpu32 = np.asarray(ref64, np.float64), np.asarray(cpu32)
    assert cpu32.dtype == F32 and np.array_equal(cpu32.astype(np.float64), ref64), "family not exact " + what
    return cpu32


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    """dlt.h compiled for the host (tests/host/host_dlt.cpp): the CPU suite pins it against numpy's SVD and torch.det"""
    from test_oracle import _host_dlt_lib
    return _host_dlt_lib(tmp_path_factory)


def host_dlt(lib, X, Y):
    X, Y = np.ascontiguousarray(X, F32), np.ascontiguousarray(Y, F32)
    N = len(X)
    h, Hf = np.zeros((N, 9)), np.zeros((N, 9), F32)
    lib.rfx_host_dlt4(X.ctypes.data_as(VP), Y.ctypes.data_as(VP), N, h.ctypes.data_as(VP), Hf.ctypes.data_as(VP))
    return Hf


def host_rank(lib, X, Y):
    X, Y = np.ascontiguousarray(X, F32), np.ascontiguousarray(Y, F32)
    fl = np.zeros(len(X), np.uint8)
    lib.rfx_host_dlt4_rank(X.ctypes.data_as(VP), Y.ctypes.data_as(VP), len(X), fl.ctypes.data_as(VP))
    return fl


def host_gate(lib, H):
    """det(H) > 1e-6 with the kernel's own determinant (rfx_det3_lu_f32), NaN -> False"""
    H = np.ascontiguousarray(H, F32).reshape(-1, 9)
    d = np.zeros(len(H), F32)
    lib.rfx_host_det3(H.ctypes.data_as(VP), len(H), d.ctypes.data_as(VP))
    with np.errstate(invalid="ignore"):
        return d > F32(1e-6)


# ====================================================================== A. ransac.hip
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays.  a * b is exact in float64 (48 bits); s = fl64(p + c) and TwoSum's
    error term t give p + c = s + t exactly.  fl32(s) is the answer unless s lies exactly half way between two float32 numbers
    and t != 0: then the true sum lies on t's side of the tie, and the neighbour on that side is the correctly rounded result."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        t = (p - (s - bb)) + (c - bb)
        r = s.astype(F32)
        r64 = r.astype(np.float64)
        other = np.where(r64 > s, np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))).astype(np.float64)
        tie = np.isfinite(s) & np.isfinite(other) & (r64 != s) & ((r64 + other) * 0.5 == s)
        fix = tie & (t * (other - r64) > 0)
        return np.where(fix, other, r64).astype(F32)


def _round_f32(x):
    """a Fraction rounded to the nearest float32, ties to even (normal range)"""
    if x == 0:
        return F32(0)
    e = 0
    ax = abs(x)
    while ax >= 2:
        ax /= 2
        e += 1
    while ax < 1:
        ax *= 2
        e -= 1
    q = Fraction(2) ** (e - 23)
    n = x / q
    fl = n.numerator // n.denominator
    rem = n - fl
    k = fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1) else 0)
    return F32(float(k * q))                               # k * q has <= 25 significant bits: float() is exact, F32() too


def fma_triples(n, seed):
    """cancellation-heavy triples (c within a few ulps of -a*b), plain random ones, and triples whose float64 sum is an exact
    float32 tie that only the error term resolves (the double-rounding case)"""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-2, 2, n).astype(F32)
    b = rng.uniform(-2, 2, n).astype(F32)
    c = rng.uniform(-2, 2, n).astype(F32)
    k = n // 3
    prod = (a[:k] * b[:k]).astype(F32)
    c[:k] = -(prod.view(np.int32) + rng.randint(-3, 4, k).astype(np.int32)).view(F32)
    j = n - n // 4
    sgn = rng.choice([-1.0, 1.0], n - j)
    a[j:] = F32(128) * (F32(1) + sgn.astype(F32) * F32(2.0 ** -23))     # a * b = 128 * (1 - 2^-46) or the like: half an ulp of c
    b[j:] = F32(1) - sgn.astype(F32) * F32(2.0 ** -23)                  # ... minus a term below float64's resolution
    c[j:] = (rng.randint(2 ** 23, 2 ** 24, n - j).astype(np.float64) * 256).astype(F32)
    return a, b, c


def err_ref(m1, m2, H):
    """float32 reprojection error of every (hypothesis, match): m1, m2 (n,3), H (N,9) float32 -> d2, e (N,n) float32.
    m1[:, 2] is never read."""
    m1, m2, H = np.asarray(m1, F32), np.asarray(m2, F32), np.asarray(H, F32).reshape(-1, 9)
    x2, y2, z2 = m2[None, :, 0], m2[None, :, 1], m2[None, :, 2]
    with np.errstate(all="ignore"):
        def row(k):
            return fma32(z2, H[:, k + 2, None], fma32(y2, H[:, k + 1, None], x2 * H[:, k, None]))
        px, py, pz = row(0), row(3), row(6)
        ex, ey = px / pz, py / pz
        dx, dy = m1[None, :, 0] - ex, m1[None, :, 1] - ey
        d2 = dx * dx + dy * dy
        assert d2.dtype == F32
        return d2, np.sqrt(d2)


def no_band(e, tol, band=2):
    """no finite error lies within ``band`` ulp(tol) of tol: a root that is 1 ulp off cannot change a decision.  The random
    families keep 2 ulps clear; the equality family sits at exactly 2 ulps and asks for more than 1."""
    t = F32(tol)
    fin = np.isfinite(e)
    gap = np.abs(e[fin].astype(np.float64) - np.float64(t))
    return bool((gap > band * np.float64(np.spacing(t))).all())


def counts_ref(e, tol, gate):
    with np.errstate(invalid="ignore"):
        return (e < F32(tol)).sum(1).astype(np.int64) * gate.astype(np.int64)


def search_ref(samples, counts):
    """outil.RANSAC over the reference counts -> (status, best count, winner, hypotheses after the duplicate filter)"""
    keep = [i for i, r in enumerate(np.asarray(samples).tolist()) if len(set(r)) == 4]        # the duplicate filter (raw values)
    nu = len(keep)
    for c in range(nu // 100):                                                                 # full chunks only, filtered order
        if max(int(counts[i]) for i in keep[c * 100:(c + 1) * 100]) == 0:
            return 1, 0, -1, nu
    best, bc = -1, 0
    for i in keep:
        if int(counts[i]) > bc:                                                                # the first maximum wins
            best, bc = i, int(counts[i])
    return (2, 0, -1, nu) if best < 0 else (0, bc, best, nu)


HM = np.array([[1.05, .02, .03], [-.01, .97, -.02], [.01, .02, 1.]])


@functools.lru_cache(maxsize=None)
def scene(n, seed, z_one=False):
    """n matches: 65 % follow one homography, the rest are unrelated.  m2[:, 2] = 1 + k/128 (k = -4 .. 4, never 0 unless z_one):
    the error divides by it although the DLT never sees it, so errors scatter on both sides of the tolerances used here.
    m1[:, 2] is NaN or arbitrary: nothing may read it."""
    rng = np.random.RandomState(1000 * n + seed)
    m2 = np.ones((n, 3))
    m2[:, :2] = rng.uniform(-1, 1, (n, 2))
    p = m2 @ HM.T
    m1 = np.concatenate([p[:, :2] / p[:, 2:], np.full((n, 1), NAN)], 1)
    out = rng.rand(n) < 0.35
    m1[out, :2] = rng.uniform(-1, 1, (int(out.sum()), 2))
    m1[::3, 2] = rng.uniform(-5, 5, len(m1[::3]))
    if not z_one:
        m2[:, 2] = 1 + rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], n) / 128.0
    return m1.astype(F32), m2.astype(F32)


def draw(n, N, seed, dup_every=0):
    """(N,4) indices; rows of distinct indices where n >= 4, except every ``dup_every``-th (a repeated index); some entries are
    written python-style negative (-1 = n-1, ...), never next to their positive twin; row 0 holds a literal -1"""
    rng = np.random.RandomState(77 * n + 13 * N + seed)
    if n < 4:
        return rng.randint(0, n, (N, 4)).astype(np.int64)
    s = np.stack([rng.permutation(n)[:4] for _ in range(N)]).astype(np.int64)
    if dup_every:
        s[dup_every - 1::dup_every, 3] = s[dup_every - 1::dup_every, 1]
    neg = rng.rand(N, 4) < 0.1
    s[neg] -= n
    if n - 1 in s[0, 1:] % n:                          # row 0 (never a repeated-index row) starts with a literal -1 = n-1
        s[0, 1:][s[0, 1:] % n == n - 1] = s[0, 0] % n
    s[0, 0] = -1
    return s


TOL = 0.02
# n: the ballot tail (63 / 64 / 65, 127 / 129) and the select kernel's 1024-stride mask loop; N: four hypotheses per workgroup,
# chunks of 100, the select kernel's 1024-stride rank loop
COUNT_CASES = [(1, 5), (3, 101), (4, 1), (63, 3), (64, 4), (65, 99), (127, 100), (129, 1023), (1025, 1025), (64, 1025), (1025, 3)]
COUNT_SEEDS = {}          # (n, N) -> seed, where 0 would put an error into the band (none needed so far: see the host test)


def count_case(n, N):
    m1, m2 = scene(n, COUNT_SEEDS.get((n, N), 0))
    return m1, m2, draw(n, N, 0, dup_every=7 if N > 7 else 0)


def hyp_ref(lib, m1, m2, H, tol, band=2):
    """reference errors, counts and the gate for the float32 hypotheses H (N,9)"""
    H = np.ascontiguousarray(H, F32).reshape(-1, 9)
    _, e = err_ref(m1, m2, H)
    assert no_band(e, tol, band), "an error within %d ulp of tol: pick another seed" % band
    gate = host_gate(lib, H)
    return e, counts_ref(e, tol, gate), gate


def ulp_close(got, e):
    """|got - e| <= 1 ulp(e); NaN where e is NaN; +-inf equal"""
    got, e = np.asarray(got), np.asarray(e)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(e)
        ok = np.where(fin, np.abs(got.astype(np.float64) - e.astype(np.float64)) <= np.spacing(np.abs(e)).astype(np.float64),
                      (got == e) | (np.isnan(got) & np.isnan(e)))
    return ok & (np.isfinite(got) == fin)


def _dev_search(dev, m1, m2, s, tol):
    """(H (N,9), counts, prediction errors, bestH, mask, result) of the device, each poisoned after it is read"""
    m1d, m2d, sd = (torch.from_numpy(v).to(dev) for v in (m1, m2, s))
    H, cnt = ops.score_hypotheses(m1d, m2d, sd, tol)
    err = ops.prediction(m1d, m2d, H) if len(s) <= 65535 else None
    Hh, ch = H.cpu().numpy().reshape(-1, 9), cnt.cpu().numpy()
    eh = err.cpu().numpy() if err is not None else None
    for t in (H, cnt) + ((err,) if err is not None else ()):
        t.fill_(-1)
    bH, inl, res = ops.ransac_h4(m1d, m2d, sd, tol)
    out = Hh, ch, eh, bH.cpu().numpy().reshape(9), inl.cpu().numpy(), res.cpu().numpy().tolist()
    bH.fill_(NAN)
    res.fill_(-7)
    return out


def check_search(lib, dev, m1, m2, s, tol, what, expect=None, band=2):
    """score_hypotheses, prediction and ransac_h4 on one input against the references; returns the reference result"""
    Hh, cnt, err, bH, inl, res = _dev_search(dev, m1, m2, s, tol)
    # which matches a sample row means: numpy's own indexing (-1 = n-1) into the host build of the DLT, bit for bit, on every row
    # whose four matches are distinct.  Everything below takes the device's H; this line is what ties H to the samples.
    real = np.array([len(set(r)) == 4 for r in (s % len(m1)).tolist()])
    assert np.array_equal(Hh[real].view(np.int32), host_dlt(lib, m1[s[real]], m2[s[real]]).view(np.int32)), \
        what + ": the device H is not the host DLT of m1[samples], m2[samples]"
    e, ref, gate = hyp_ref(lib, m1, m2, Hh, tol, band)
    assert np.array_equal(cnt, ref), "%s: counts %s" % (what, _where_bad(torch.from_numpy(cnt), torch.from_numpy(ref)))
    if err is not None:
        ok = ulp_close(err, e)
        assert ok.all(), "%s: %d errors off by more than 1 ulp, first %s" % (what, (~ok).sum(), np.argwhere(~ok)[:3].tolist())
        with np.errstate(invalid="ignore"):
            assert np.array_equal((err < F32(tol)).sum(1) * gate, cnt), what + ": count and prediction kernels disagree"
    st, bc, win, nu = want = search_ref(s, ref)
    assert res == [st, bc, win, nu], (what, res, want)
    if expect is not None:
        assert (st, win) == expect, (what, want, expect)
    if st == 0:
        assert np.array_equal(bH.view(np.int32), Hh[win].view(np.int32)), what + ": bestH is not the winner's H"
        with np.errstate(invalid="ignore"):
            assert np.array_equal(inl, e[win] < F32(tol)), what + ": inlier mask"
        assert int(inl.sum()) == bc
    else:
        assert not inl.any() and not bH.any(), what
    return want, Hh, ref


@gpu
@pytest.mark.parametrize("n,N", COUNT_CASES, ids=str)
def test_error_counts_and_search_equal_the_float32_emulation(dev, hostlib, n, N):
    """score_hypotheses, prediction and ransac_h4 on the same matches and samples: m2[:, 2] != 1, m1[:, 2] NaN or arbitrary,
    a repeated index in every 7th row, and negative sample indices (a literal -1 in row 0, about a tenth of the rest): the device H
    must be the host DLT of numpy's m1[samples], m2[samples] (check_search), so -1 can only mean n-1.  n < 4: every row repeats an index, nothing survives the filter
    (status 2) while score_hypotheses, which does not filter, still counts what its H gives."""
    m1, m2, s = count_case(n, N)
    assert n < 4 or (s[0, 0] == -1 and len(set((s[0] % n).tolist())) == 4)
    (st, _, _, nu), _, ref = check_search(hostlib, dev, m1, m2, s, TOL, "n=%d N=%d" % (n, N))
    if n < 4:
        assert (st, nu) == (2, 0)
    elif N >= 99 and n >= 63:
        assert st == 0 and 0 < ref.max() < n and nu < N          # not vacuous: a real winner, some matches in, some out


def pred_case():
    """1025 matches x 9 hand-written H (not from the DLT): near the scene's homography (inlier scale: p.x - ex cancels), far from
    it, affine with m2[:, 2] = 0 rows (pz = 0: +-inf and, where px = 0 too, NaN), and the zero matrix (NaN everywhere)"""
    m1, m2 = (v.copy() for v in scene(1025, 3, z_one=True))
    rng = np.random.RandomState(5)
    m2[9::16, 2] = (1 + rng.randint(-4, 5, len(m2[9::16])) / 128.0).astype(F32)
    Hs = [HM / np.linalg.norm(HM), HM * 3, HM + 1e-4 * rng.randn(3, 3), HM + 0.3 * rng.randn(3, 3), -HM,
          np.array([[1, 0.25, -0.5], [-0.5, 1, 0.25], [0, 0, 1.0]]), np.array([[0, 0, 1.0], [0, 0, 0], [0, 0, 2.0]]),
          np.zeros((3, 3)), rng.randn(3, 3)]
    m2[5::64, 2] = 0
    m2[5, :2] = 0          # with the translation-free row of the 7th H: px = pz = 0
    return m1, m2, np.stack(Hs).astype(F32).reshape(-1, 9)


@gpu
def test_prediction_is_the_emulated_chain_within_one_ulp_of_the_root(dev):
    """ops.prediction on hand-written H.  A chain in another order, an un-fused multiply-add or a reciprocal in place of the
    divide changes ex in its last place, which p.x - ex turns into tens of ulps of e at inlier scale: one ulp cannot hide it."""
    m1, m2, Hs = pred_case()
    _, e = err_ref(m1, m2, Hs)
    err = ops.prediction(*(torch.from_numpy(v).to(dev) for v in (m1, m2, Hs.reshape(-1, 3, 3))))
    got = err.cpu().numpy()
    err.fill_(NAN)
    ok = ulp_close(got, e)
    assert ok.all(), "%d of %d off by more than 1 ulp, first at %s" % ((~ok).sum(), ok.size, np.argwhere(~ok)[:3].tolist())


# ---- the equality family
TRIPLES = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29))
S_EQ = 2.0 ** -9
EQ_ROWS = [0, 1, 2, 4]


def equal_case(triple, n=129):
    """A pure translation by (1, 0): its unit-norm homography is +-0.5 * [[1,0,1],[0,1,0],[0,0,1]] -- dyadic -- so with matches on
    the k/64 lattice and m2[:, 2] a power of two every product, sum and quotient of the error is exact; the offsets
    (+-a, +-b) * 2^-9 make d2 = (c * 2^-9)^2 a perfect square and e = c * 2^-9 exact.  Matches 0 .. 3 are the sample (e = 0)."""
    a, b, c = triple
    rng = np.random.RandomState(c)
    m2 = np.ones((n + 4, 3))
    m2[:4, :2] = np.array([[-48, -40], [44, -36], [40, 52], [-36, 44]]) / 64.0
    z = rng.choice([0.5, 1.0, 2.0], n)
    m2[4:, :2] = rng.randint(-64, 65, (n, 2)) / 64.0 * z[:, None]
    m2[4:, 2] = z
    off = np.array([(a, b), (-a, b), (a, -b), (-a, -b), (b, a), (-b, a), (b, -a), (-b, -a), (c, 0), (0, -c)])[np.arange(n) % 10]
    m1 = np.full((n + 4, 3), NAN)
    m1[:, :2] = m2[:, :2] / m2[:, 2:] + np.array([1.0, 0.0])
    m1[4:, :2] += off * S_EQ
    s = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [0, 1, 2, 2], [2, 0, 3, 1]], np.int64)
    return m1.astype(F32), m2.astype(F32), s, F32(c * S_EQ)


def equal_family_holds(m1, m2, H, e0):
    """on the hypotheses of rows EQ_ROWS (row 3 repeats an index): every match has e == 0 (the sample) or e == e0 exactly, d2 a
    perfect square"""
    d2, e = err_ref(m1, m2, H)
    want = np.where(np.arange(len(m1)) < 4, F32(0), e0).astype(F32)[None].repeat(4, 0)
    return np.array_equal(e[EQ_ROWS], want) and np.array_equal(d2[EQ_ROWS].astype(np.float64), want.astype(np.float64) ** 2)


def _ulps(x, k):
    return (F32(x).view(np.int32) + k).view(F32)


@gpu
@pytest.mark.parametrize("triple", TRIPLES, ids=str)
def test_inlier_decision_two_ulps_either_side_of_an_exact_error(dev, hostlib, triple):
    """tol two ulps above the exact e: every match is an inlier; two ulps below: only the four sample points (e = 0)."""
    m1, m2, s, e0 = equal_case(triple)
    n = len(m1)
    for k, cnt in ((2, n), (-2, 4)):
        tol = float(_ulps(e0, k))
        (st, bc, win, nu), Hh, ref = check_search(hostlib, dev, m1, m2, s, tol, "%s %+d ulp" % (triple, k), expect=(0, 0), band=1)
        assert equal_family_holds(m1, m2, Hh, e0)
        assert (bc, nu) == (cnt, 4) and ref.tolist() == [cnt, cnt, cnt, ref[3], cnt]


@gpu
@pytest.mark.parametrize("triple", TRIPLES, ids=str)
def test_inlier_decision_is_strict_at_an_exact_error(dev, hostlib, triple):
    """v_sqrt_f32 returns the exact root of these perfect squares (read on an MI355X, DESIGN_LOG section 4): prediction returns e
    itself, ``tol == e`` is not an inlier -- the comparison is ``<`` -- and the next float32 above is."""
    m1, m2, s, e0 = equal_case(triple)
    n = len(m1)
    m1d, m2d, sd = (torch.from_numpy(v).to(dev) for v in (m1, m2, s))
    H, cnt_eq = ops.score_hypotheses(m1d, m2d, sd, float(e0))
    Hh = H.cpu().numpy().reshape(-1, 9)
    assert equal_family_holds(m1, m2, Hh, e0)
    _, e = err_ref(m1, m2, Hh)
    err = ops.prediction(m1d, m2d, H)
    _same(err[EQ_ROWS], torch.from_numpy(e[EQ_ROWS]), "prediction on perfect squares")
    assert host_gate(hostlib, Hh)[EQ_ROWS].all()
    for tol, cnt in ((e0, 4), (_ulps(e0, 1), n)):
        c = ops.score_hypotheses(m1d, m2d, sd, float(tol))[1]
        assert c.cpu()[EQ_ROWS].tolist() == [cnt] * 4, (triple, float(tol), c.cpu().tolist())
        bH, inl, res = ops.ransac_h4(m1d, m2d, sd, float(tol))
        assert res.cpu().tolist() == [0, cnt, 0, 4]
        _same(inl, torch.from_numpy(e[0] < tol), "mask at tol = e%s" % ("" if cnt == 4 else " + 1 ulp"))


# ---- the search
def search_scene():
    """40 matches under one homography (z = 1), 16 unrelated ones, and four extra matches (56 .. 59) whose hypotheses have full
    rank but |det H| sixteen times below the gate: dead hypotheses (count 0) that no filter drops"""
    rows, cols, eps = 15, 20, 1e-4
    xs, ys = ((np.arange(cols) + 0.5) / cols - 0.5) * 2, ((np.arange(rows) + 0.5) / rows - 0.5) * 2
    xb, yb = np.tile(xs, rows), np.repeat(ys, cols)
    rng = np.random.RandomState(3)
    cells = rng.permutation(rows * cols)[:56]
    m2 = np.stack((xb[cells], yb[cells], np.ones(56)), 1)
    p = m2 @ HM.T
    m1 = np.concatenate([p[:, :2] / p[:, 2:], np.ones((56, 1))], 1)
    m1[40:, :2] = rng.uniform(-1, 1, (16, 2))
    m1 = np.concatenate([m1, [[-.5, -.5, 1.], [.5, -.5, 1.], [.5, .5, 1.], [-.5, .5, 1.]]])
    m2 = np.concatenate([m2, [[-.6, eps, 1.], [-.1, -2 * eps, 1.], [.3, 3 * eps, 1.], [.7, -eps, 1.]]])
    return m1.astype(F32), m2.astype(F32)


def _rows(rng, k, kind):
    """live: four distinct of the 40 good matches; weak: at least one of the 16 unrelated ones; dead: a permutation of 56 .. 59;
    dup: a repeated index (the filter drops it)"""
    if k == 0:
        return np.zeros((0, 4), np.int64)
    if kind == "live":
        return np.stack([rng.permutation(40)[:4] for _ in range(k)]).reshape(k, 4)
    if kind == "weak":
        r = np.stack([rng.permutation(40)[:4] for _ in range(k)]).reshape(k, 4)
        r[np.arange(k), rng.randint(0, 4, k)] = rng.randint(40, 56, k)
        return r
    if kind == "dead":
        return np.stack([56 + rng.permutation(4) for _ in range(k)]).reshape(k, 4)
    return np.tile(rng.randint(0, 40, (k, 1)), (1, 4))


def _with_dups(rng, parts, every=9):
    """the rows of ``parts`` in order, a dropped row put in after every ``every`` rows: rank != index"""
    rows = np.concatenate(parts)
    out = []
    for i, r in enumerate(rows):
        out.append(r)
        if i % every == every - 1:
            out.append(_rows(rng, 1, "dup")[0])
    return np.stack(out).astype(np.int64)


WIN_ROW = np.array([0, 13, 27, 38], np.int64)
# name -> (kind, expected status, expected winner or None)
SEARCH_CASES = {
    "ties 700 1023 1024 2047 2100": ("tie", (700, 1023, 1024, 2047, 2100), 0, 700),
    "ties 1024 1500": ("tie", (1024, 1500), 0, 1024),
    "ties 1023 1024": ("tie", (1023, 1024), 0, 1023),
    "dead ranks 200-249 of 250": ("dead", (200, 50, 0), 0, None),
    "dead ranks 150-249 of 300": ("dead", (150, 100, 50), 0, None),
    "dead ranks 100-199 of 300": ("dead", (100, 100, 100), 1, -1),
    "dead all of 100": ("dead", (0, 100, 0), 1, -1),
    "dead all of 99": ("dead", (0, 99, 0), 2, -1),
}


@functools.lru_cache(maxsize=None)
def search_case(name):
    kind, spec, status, winner = SEARCH_CASES[name]
    rng = np.random.RandomState(len(name))
    if kind == "tie":
        s = _rows(rng, 2150, "weak")
        s[5:600:7] = _rows(rng, len(s[5:600:7]), "dup")               # dropped rows in front of the ties
        s[list(spec)] = WIN_ROW
        return s.astype(np.int64), status, winner
    live0, dead, live1 = spec
    return _with_dups(rng, [_rows(rng, live0, "live"), _rows(rng, dead, "dead"), _rows(rng, live1, "live")]), status, winner


def search_case_holds(lib, name, H=None):
    """the case does what its name says -- on the host build's H (bit-equal to the device's, test_device_dlt_...) or the device's"""
    m1, m2 = search_scene()
    s, status, winner = search_case(name)
    if H is None:
        H = host_dlt(lib, m1[s], m2[s])
    _, ref, gate = hyp_ref(lib, m1, m2, H, TOL)
    st, bc, win, nu = search_ref(s, ref)
    dead = (s >= 56).all(1)
    ok = st == status and (winner is None or win == winner) and not gate[dead].any() and (ref[dead] == 0).all()
    if SEARCH_CASES[name][0] == "tie":
        tied = [i for i in range(len(s)) if ref[i] == bc and len(set(s[i].tolist())) == 4]
        ok = ok and tied == sorted(SEARCH_CASES[name][1]) and nu < len(s) and bc == 40
    else:
        ok = ok and nu == sum(SEARCH_CASES[name][1]) and nu < len(s)
    return ok


@gpu
@pytest.mark.parametrize("name", list(SEARCH_CASES), ids=str)
def test_search_ties_and_zero_chunk_abort_equal_the_stated_search(dev, hostlib, name):
    """Exact ties (the winning sample row repeated on both sides of the select kernel's 1024-hypothesis trips: the first wins) with
    dropped rows in front of them; dead hypotheses in the partial last chunk (never aborts), across two chunks (neither is all
    dead), filling one full chunk (abort), and alone (100: abort; 99: nothing found)."""
    m1, m2 = search_scene()
    s, status, winner = search_case(name)
    want, Hh, _ = check_search(hostlib, dev, m1, m2, s, TOL, name)
    assert search_case_holds(hostlib, name, Hh), (name, want)


BATCH_N = (0, 3, 4, 65)


def batch_case():
    cap, N = max(BATCH_N), 230
    pairs = []
    for b, n in enumerate(BATCH_N):
        m1, m2 = scene(max(n, 1), 40 + b, z_one=(b == 3))
        s = draw(n, N, b, dup_every=5) if n else np.zeros((N, 4), np.int64)
        pairs.append((m1[:n], m2[:n], s))
    return cap, N, pairs


@gpu
def test_batched_search_equals_single_pair_calls_and_the_reference(dev, hostlib):
    """n = (0, 3, 4, 65) in one launch, the padding rows of match1 / match2 NaN.  n < 4: status 3, nothing evaluated; padding mask
    rows 0; every pair with n >= 4 equals its single-pair call and the reference."""
    cap, N, pairs = batch_case()
    B = len(pairs)
    M1, M2 = np.full((B, cap, 3), NAN, F32), np.full((B, cap, 3), NAN, F32)
    for b, (a, c, _) in enumerate(pairs):
        M1[b, :len(a)], M2[b, :len(a)] = a, c
    nd = torch.tensor(BATCH_N, dtype=torch.int32, device=dev)
    S = torch.from_numpy(np.stack([p[2] for p in pairs])).to(dev)
    bH, bI, bR = ops.ransac_h4_batched(torch.from_numpy(M1).to(dev), torch.from_numpy(M2).to(dev), nd, S, TOL)
    H_, I_, R_ = bH.cpu().numpy().reshape(B, 9), bI.cpu().numpy(), bR.cpu().numpy().tolist()
    bH.fill_(NAN)
    bR.fill_(-7)
    for b, (m1, m2, s) in enumerate(pairs):
        n = len(m1)
        assert not I_[b, n:].any(), b
        if n < 4:
            assert R_[b] == [3, 0, -1, 0] and not I_[b].any() and not H_[b].any(), (b, R_[b])
            continue
        Hh, cnt, _, sH, sI, sR = _dev_search(dev, m1, m2, s, TOL)
        e, ref, _ = hyp_ref(hostlib, m1, m2, Hh, TOL)
        st, bc, win, nu = search_ref(s, ref)
        assert R_[b] == [st, bc, win, nu] == sR and st == 0, (b, R_[b], sR)
        assert np.array_equal(H_[b].view(np.int32), Hh[win].view(np.int32)) and np.array_equal(H_[b].view(np.int32), sH.view(np.int32))
        assert np.array_equal(I_[b, :n], e[win] < F32(TOL)) and np.array_equal(I_[b, :n], sI), b


# ---- the DLT on the device
def dlt_case(N):
    """N 4-point systems: samples of a scene, and the det-gate family of tests/test_oracle.py among them"""
    from test_oracle import det_gate_cases
    m1, m2 = (np.nan_to_num(v, nan=1.0) for v in scene(200, 9))
    rng = np.random.RandomState(N)
    s = np.stack([rng.permutation(200)[:4] for _ in range(N)])
    X, Y = m1[s].copy(), m2[s].copy()
    k = N // 3
    if k:
        X[:k], Y[:k] = det_gate_cases(k, seed=N)
        # rank-deficient systems (the flag): three of the four target points on one row of a 30 x 40 cell lattice, the source
        # points the same cells one column on -- collinear in both images, a 2-D null space
        xs, ys = ((np.arange(40) + 0.5) / 40 - 0.5) * 2, ((np.arange(30) + 0.5) / 30 - 0.5) * 2
        for j in range(k, 2 * k):
            r, r2 = rng.permutation(30)[:2]
            c = rng.permutation(39)[:4]
            Y[j, :, 0], Y[j, :, 1], Y[j, :, 2] = xs[c], ys[[r, r, r, r2]], 1
            X[j] = Y[j]
            X[j, :, 0] = xs[c + 1]
            p = rng.permutation(4)
            X[j], Y[j] = X[j, p], Y[j, p]
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


@gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4000])
def test_device_dlt_is_the_host_build_of_the_same_header_bit_for_bit(dev, hostlib, N):
    """ops.dlt4_homography, the H of score_hypotheses and the rank flags against tests/host/host_dlt.cpp: the device compile of the
    float64 Householder code is the host's.  (That the algorithm is right is the CPU suite's matter.)"""
    X, Y = dlt_case(N)
    ref = torch.from_numpy(host_dlt(hostlib, X, Y).view(np.int32).reshape(N, 3, 3))
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    _same(ops.dlt4_homography(Xd, Yd).view(torch.int32), ref, "dlt4_homography")
    H = torch.empty((N, 3, 3), dtype=torch.float32, device=dev)
    fl = torch.empty(N, dtype=torch.uint8, device=dev)
    ops._call("rfx_dlt4_homography_flags", dev, ops._p(Xd), ops._p(Yd), N, ops._p(H), ops._p(fl))
    rank = torch.from_numpy(host_rank(hostlib, X, Y))
    assert N < 63 or (rank[N // 3:2 * (N // 3)].all() and not rank[:N // 3].any() and not rank[2 * (N // 3):].all())   # both occur
    _same((fl & 4) // 4, rank, "rank flags")
    _same(H.view(torch.int32), ref, "dlt4_homography_flags")
    m1d, m2d = Xd.reshape(-1, 3), Yd.reshape(-1, 3)
    Hs, cnt = ops.score_hypotheses(m1d, m2d, torch.arange(4 * N, device=dev).view(N, 4), TOL)
    # the gate of the same hypotheses: count > 0 <=> it passed (the four sample points are inliers of their own H where it is
    # well conditioned; a count of 0 behind a passed gate is possible and not asserted)
    gate = host_gate(hostlib, ref.numpy().view(F32))
    assert not cnt.cpu().numpy()[~gate].any()
    assert N < 4000 or (0.2 < gate[:N // 3].mean() < 0.8)
    _same(Hs.view(torch.int32), ref, "H of score_hypotheses")


# ====================================================================== B. cc.hip
def cc_areas(m, th):
    """m (N,H,W) float32 -> (foreground, area of each pixel's 8-connected component).  Foreground = m > th (NaN is background);
    label = flat index, then a 3x3 minimum over the foreground until nothing changes."""
    m = np.asarray(m, F32)
    N, H, W = m.shape
    with np.errstate(invalid="ignore"):
        fg = m > F32(th)
    BIG = H * W
    lab = np.where(fg, np.arange(BIG, dtype=np.int64).reshape(1, H, W), BIG)
    while True:
        p = np.pad(lab, ((0, 0), (1, 1), (1, 1)), constant_values=BIG)
        new = lab
        for dy in range(3):
            for dx in range(3):
                new = np.minimum(new, p[:, dy:dy + H, dx:dx + W])
        new = np.where(fg, new, BIG)
        if np.array_equal(new, lab):
            break
        lab = new
    flat = (lab + np.arange(N).reshape(N, 1, 1) * (BIG + 1)).ravel()
    return fg, np.bincount(flat, minlength=N * (BIG + 1))[flat].reshape(N, H, W)


def cc_apply(m, fg, area, max_area):
    """a foreground pixel whose component has area <= max_area and < H*W becomes +0.0, everything else keeps its bits (int32)"""
    m = np.asarray(m, F32)
    kill = fg & (area <= max_area) & (area < m.shape[1] * m.shape[2])
    return np.where(kill, np.int32(0), m.view(np.int32))


def cc_ref(m, th, max_area):
    return cc_apply(m, *cc_areas(m, th), max_area)


TH = 0.5
FG_VALS = np.array([np.nextafter(F32(TH), F32(1)), 0.75, 1.0, 3e38, np.inf, 0.5000001], F32)
BG_VALS = np.array([TH, NAN, -1.0, 0.0, -0.0, np.nextafter(F32(TH), F32(0)), -np.inf], F32)


def paint(P):
    """a boolean pattern as a map: foreground from FG_VALS (the float32 next above the threshold among them), background from
    BG_VALS (the threshold itself, NaN and -0.0 among them), varied by position"""
    P = np.asarray(P, bool)
    i = np.arange(P.size).reshape(P.shape)
    return np.where(P, FG_VALS[i % len(FG_VALS)], BG_VALS[(i // 3) % len(BG_VALS)]).astype(F32)


def th_for(size, a):
    """a cc_th whose integer bound on a map of ``size`` pixels is ``a`` (checked against ops.cc_max_area on the host)"""
    return (a + 0.5) / size


def _cc_dev(dev, m, max_area):
    m = np.asarray(m, F32)
    m3 = m if m.ndim == 3 else m[None]
    return ops.remove_small_cc(torch.from_numpy(m3).to(dev), th_for(m3.shape[1] * m3.shape[2], max_area), TH)


def all_4x4():
    k = np.arange(65536, dtype=np.int64)
    return ((k[:, None] >> np.arange(16)) & 1).astype(bool).reshape(65536, 4, 4)


@gpu
@pytest.mark.parametrize("max_area", [0, 1, 3, 15, 16])
def test_cc_all_binary_4x4_maps_in_one_launch(dev, max_area):
    """Every neighbourhood of the three union rules, 16 rows per 64-lane segment, four maps per segment: maps must not see each
    other.  The all-ones map survives max_area = 16 (a component that is the whole image is never removed)."""
    m = paint(all_4x4())
    ref = cc_ref(m, TH, max_area)
    assert max_area < 16 or np.array_equal(ref[65535], m[65535].view(np.int32))
    _same_bits(_cc_dev(dev, m, max_area), ref, "4x4 exhaustive, max_area %d" % max_area)


def serpentine(H, W):
    P = np.zeros((H, W), bool)
    P[::2] = True
    P[1::4, W - 1] = True
    P[3::4, 0] = True
    return P


def spiral(n):
    """a one-pixel-wide square spiral: a walk that turns right whenever the cell two ahead is already taken"""
    P = np.zeros((n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    P[0, 0] = True
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        ny2, nx2 = ny + dy, nx + dx
        if not (0 <= ny < n and 0 <= nx < n) or P[ny, nx] or (0 <= ny2 < n and 0 <= nx2 < n and P[ny2, nx2]):
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            ny2, nx2 = ny + dy, nx + dx
            if not (0 <= ny < n and 0 <= nx < n) or P[ny, nx] or (0 <= ny2 < n and 0 <= nx2 < n and P[ny2, nx2]):
                break
        y, x = ny, nx
        P[y, x] = True
    return P


def comb(H, W):
    P = np.zeros((H, W), bool)
    P[:, ::2] = True
    P[H - 1] = True
    return P


def row_wrap(H, W):
    """a run that ends at x = W-1 while the next row starts with foreground at x = 0: lone pixels unless a row link crosses the
    row end (for W = 2 they touch diagonally)"""
    P = np.zeros((H, W), bool)
    P[0::3, W - 1] = True
    P[1::3, 0] = True
    return P


def seg_cross(H, W):
    """runs of 11 pixels that straddle flat indices 64, 128, ..: lane 0's look into the previous segment"""
    P = np.zeros(H * W, bool)
    for b in range(64, H * W - 6, 64):
        if (b - 5) // W == (b + 5) // W:
            P[b - 5:b + 6] = True
    P = P.reshape(H, W)
    P[1::2] = False
    return P


def checker(H, W):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)


PATTERNS = {
    "serpentine 65x129": lambda: serpentine(65, 129),
    "spiral 67": lambda: spiral(67),
    "comb 9x257": lambda: comb(9, 257),
    "checkerboard 33x65": lambda: checker(33, 65),
    "diagonal 65": lambda: np.eye(65, dtype=bool),
    "anti-diagonal 65": lambda: np.eye(65, dtype=bool)[:, ::-1].copy(),
    "row wrap 6x2": lambda: row_wrap(6, 2), "row wrap 7x3": lambda: row_wrap(7, 3), "row wrap 9x5": lambda: row_wrap(9, 5),
    "row wrap 9x13": lambda: row_wrap(9, 13), "row wrap 5x63": lambda: row_wrap(5, 63), "row wrap 5x64": lambda: row_wrap(5, 64),
    "row wrap 5x65": lambda: row_wrap(5, 65),
    "segment crossing 8x130": lambda: seg_cross(8, 130), "segment crossing 6x191": lambda: seg_cross(6, 191),
}
ONE_COMPONENT = ("serpentine 65x129", "spiral 67", "comb 9x257", "checkerboard 33x65", "diagonal 65", "anti-diagonal 65")


@functools.lru_cache(maxsize=None)
def pattern_case(name):
    """(map, [(max_area, reference bits)], area of the largest component): the threshold that removes it and the one that keeps it"""
    m = paint(PATTERNS[name]())[None]
    fg, area = cc_areas(m, TH)
    big = int(area[fg].max())
    return m, [(a, cc_apply(m, fg, area, a)) for a in (big, big - 1)], big


@gpu
@pytest.mark.parametrize("name", list(PATTERNS), ids=str)
def test_cc_constructed_patterns_removed_and_kept(dev, name):
    """Deep find chains and many CAS unions (serpentine, spiral, comb, checkerboard), the NW and NE rules alone (the two
    diagonals), runs that end a row while the next row begins inside the same 64-pixel segment, runs across a segment boundary."""
    m, cases, area = pattern_case(name)
    if name in ONE_COMPONENT:
        assert area == int(PATTERNS[name]().sum())
    for a, ref in cases:
        _same_bits(_cc_dev(dev, m, a), ref, "%s, max_area %d" % (name, a))


CC_W, CC_H = (1, 2, 63, 64, 65, 127, 128, 129, 191), (1, 2, 5)


@functools.lru_cache(maxsize=None)
def random_maps(H, W):
    rng = np.random.RandomState(H * 1000 + W)
    return paint(np.stack([rng.rand(H, W) < d for d in (0.3, 0.45, 0.6, 0.75, 0.9)]))


@gpu
@pytest.mark.parametrize("W", CC_W)
def test_cc_random_maps_at_widths_next_to_the_segment_size(dev, W):
    for H in CC_H:
        m = random_maps(H, W)
        for a in (1, 4, H * W):
            _same_bits(_cc_dev(dev, m, a), cc_ref(m, TH, a), "%dx%d random, max_area %d" % (H, W, a))


def beyond_cap_case():
    """2049 x 2050 (more pixels than the 16384 x 256 threads of the launch): 8x8 cells, each with a solid square of side
    1 + (cell index mod 5) in its lower right corner (three background pixels between squares), one lone pixel in the last
    corner.  max_area = 9 removes sides 1 .. 3 and the lone pixel; built by construction, no labelling."""
    H, W = 2049, 2050
    yy, xx = np.arange(2048)[:, None], np.arange(2048)[None, :]
    side = 1 + ((yy // 8) * 256 + (xx // 8)) % 5
    sq = (yy % 8 >= 8 - side) & (xx % 8 >= 8 - side)
    P = np.zeros((H, W), bool)
    P[:2048, :2048] = sq
    P[2048, 2049] = True
    m = np.where(P, F32(1.0), F32(0.25)).astype(F32)
    m[::7, ::5] = np.where(P[::7, ::5], F32(np.nextafter(F32(TH), F32(1))), F32(TH))
    keep = np.zeros((H, W), bool)
    keep[:2048, :2048] = sq & (side >= 4)
    return m, np.where(P & ~keep, np.int32(0), m.view(np.int32))


@gpu
def test_cc_stride_loop_beyond_the_launch_cap(dev):
    m, ref = beyond_cap_case()
    assert m.size > 16384 * 256 and (ref.ravel()[16384 * 256:] != m.view(np.int32).ravel()[16384 * 256:]).any()
    _same_bits(_cc_dev(dev, m, 9)[0], ref, "2049x2050")


RAGGED = ((3, 5, 0), (7, 9, 15), (1, 1, 78), (5, 64, 83))          # h, w, offset: 15, 78 and 83 are no multiples of 64
RAGGED_TOTAL = 83 + 320 + 10 + 320          # a gap of 10, then a tail gap as long as the row that does not fit
RAGGED_MISFIT = (5, 64, RAGGED_TOTAL - 319)  # one element too long for the buffer; its slice lies in the tail gap alone


def ragged_case():
    rng = np.random.RandomState(11)
    buf = np.full(RAGGED_TOTAL, F32(0.875))                                 # the gaps hold foreground values
    maps = []
    for h, w, off in RAGGED:
        P = rng.rand(h, w) < 0.6
        if h == 5:
            P[:, 63] = True
            P[:, 0] = True                                                  # runs that end a row / begin the next
        m = paint(P)
        buf[off:off + h * w] = m.ravel()
        maps.append(m)
    return buf.astype(F32), maps


@gpu
@pytest.mark.parametrize("max_area", [1, 3, 400])
def test_cc_ragged_maps_equal_the_reference_and_the_dense_call(dev, max_area):
    """Maps 3x5, 7x9, 1x1 and 5x64 packed at offsets 0, 15, 78 and 83 with foreground-valued gaps: the gaps neither change nor
    connect anything.  A table row that does not fit the buffer is skipped: with a NaN-filled output, its slice and the gaps stay
    NaN.  Then each map alone (n_active = 1), and the public entry point, whose gaps pass through."""
    buf, maps = ragged_case()
    refs = [cc_ref(m[None], TH, max_area)[0] for m in maps]
    for m, r in zip(maps, refs):
        _same_bits(_cc_dev(dev, m, max_area)[0], r, "dense %s" % (m.shape,))
    bd = torch.from_numpy(buf).to(dev)

    def run(rows):
        n = len(rows)
        off = torch.tensor([r[2] for r in rows], dtype=torch.int64, device=dev)
        dims = torch.tensor([[r[0], r[1], max_area] for r in rows], dtype=torch.int32, device=dev)
        out = torch.full_like(bd, NAN)
        ws = torch.empty(3 * 4 * RAGGED_TOTAL, dtype=torch.uint8, device=dev)
        ops._call("rfx_remove_small_cc_ragged_f32", dev, ops._p(bd), ops._p(out), ops._p(off), ops._p(dims), n, RAGGED_TOTAL,
                  max(r[0] * r[1] for r in rows if r[2] + r[0] * r[1] <= RAGGED_TOTAL), float(TH), ops._p(ws))
        return out
    want = np.full(RAGGED_TOTAL, NAN, F32).view(np.int32)
    nan_bits = want[0]
    for (h, w, off), r in zip(RAGGED, refs):
        want[off:off + h * w] = r.ravel()
    assert RAGGED_MISFIT[2] > 83 + 320 + 10 and RAGGED_MISFIT[2] + 320 == RAGGED_TOTAL + 1
    _same_bits(run(RAGGED + (RAGGED_MISFIT,)), want, "ragged + a row that does not fit")
    for (h, w, off), r in zip(RAGGED, refs):
        one = np.full(RAGGED_TOTAL, nan_bits, np.int32)
        one[off:off + h * w] = r.ravel()
        _same_bits(run(((h, w, off),)), one, "ragged, n_active = 1, %dx%d" % (h, w))
    pub = buf.view(np.int32).copy()
    for (h, w, off), m in zip(RAGGED, maps):
        a = ops.cc_max_area(h * w, 0.3)
        pub[off:off + h * w] = cc_ref(m[None], TH, a).ravel()
    got = ops.remove_small_cc_ragged(bd, torch.tensor([r[2] for r in RAGGED], device=dev), [(r[0], r[1]) for r in RAGGED], 0.3, TH)
    _same_bits(got, pub, "remove_small_cc_ragged")


def cc_max_area_brute(size, th):
    return max(a for a in range(size + 1) if np.float64(a) / np.float64(size) <= np.float64(th))


# ====================================================================== C. multih.hip
def fg32(mask, bg):
    """((mask + (1 - bg)) > 0.5) in float32 steps"""
    mask = np.asarray(mask, F32)
    bgv = np.ones_like(mask) if bg is None else np.asarray(bg, F32)
    return (mask + (F32(1) - bgv)) > F32(0.5)


def keep64(mask, bg, rt, ct):
    """ATen's upsample_bilinear2d (align_corners=False) of (1 - fg) to (rt, ct) in float64, thresholded at 0.5 -> (value, keep)"""
    v = 1.0 - fg32(mask, bg).astype(np.float64)
    h, w = v.shape

    def axis(n_in, n_out):
        s = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = s.astype(np.int64)
        return i0, i0 + (i0 < n_in - 1), s - i0
    y0, y1, ly = axis(h, rt)
    x0, x1, lx = axis(w, ct)
    ly, lx = ly[:, None], lx[None, :]
    r0 = v[y0][:, x0] * (1 - lx) + v[y0][:, x1] * lx
    r1 = v[y1][:, x0] * (1 - lx) + v[y1][:, x1] * lx
    val = r0 * (1 - ly) + r1 * ly
    return val, val > 0.5


def keep32(mask, bg, rt, ct, contract):
    """the same in float32 steps: scale = fl(h / rt); src = scale * (dst + 0.5) - 0.5 rounded after each step, or
    (``contract``) as one fused multiply-add -- a compiler may do either -- then the written order: fl(v00 * hx), fma, fma"""
    v = (F32(1) - fg32(mask, bg).astype(F32)).astype(F32)
    h, w = v.shape

    def axis(n_in, n_out):
        sc = F32(n_in) / F32(n_out)
        d = (np.arange(n_out).astype(F32) + F32(0.5)).astype(F32)
        s = fma32(np.full_like(d, sc), d, np.full_like(d, F32(-0.5))) if contract else (sc * d).astype(F32) - F32(0.5)
        s = np.where(s < 0, F32(0), s).astype(F32)
        i0 = s.astype(np.int64)
        lam = (s - i0.astype(F32)).astype(F32)
        return i0, i0 + (i0 < n_in - 1), lam, (F32(1) - lam).astype(F32)
    y0, y1, ly, hy = axis(h, rt)
    x0, x1, lx, hx = axis(w, ct)
    ly, hy, lx, hx = ly[:, None], hy[:, None], lx[None, :], hx[None, :]
    shape = (rt, ct)
    B = lambda a: np.broadcast_to(a, shape).astype(F32)
    r0 = fma32(v[y0][:, x1], B(lx), (v[y0][:, x0] * hx).astype(F32))
    r1 = fma32(v[y1][:, x1], B(lx), (v[y1][:, x0] * hx).astype(F32))
    val = fma32(r1, B(ly), (r0 * hy).astype(F32))
    return val, val > F32(0.5)


def keep_nondyadic(mask, bg, rt, ct):
    """the keep map where the ratio is no power of two: both float32 forms of the source index agree on every cell, and no cell
    lies within 4 ulp of 0.5 (asserted: the maps are chosen accordingly)"""
    va, ka = keep32(mask, bg, rt, ct, False)
    vb, kb = keep32(mask, bg, rt, ct, True)
    _, k64 = keep64(mask, bg, rt, ct)
    margin = 4 * np.spacing(F32(0.5))
    assert np.array_equal(ka, kb) and np.array_equal(ka, k64)
    assert (np.abs(va - F32(0.5)) > margin).all() and (np.abs(vb - F32(0.5)) > margin).all(), "a cell within 4 ulp of 0.5"
    return ka


def settle(mask, rt, ct):
    """binary mask with the 2x2 source blocks of every cell that would land within 1e-3 of 0.5 made uniform"""
    mask = mask.copy()
    h, w = mask.shape
    for _ in range(20):
        val, _ = keep64(mask, None, rt, ct)
        bad = np.argwhere(np.abs(val - 0.5) < 1e-3)
        if not len(bad):
            return mask
        for r, c in bad:
            y0 = int(max((h / rt) * (r + 0.5) - 0.5, 0))
            x0 = int(max((w / ct) * (c + 0.5) - 0.5, 0))
            mask[y0:y0 + 2, x0:x0 + 2] = mask[y0, x0]
    raise AssertionError("could not settle the map")


@functools.lru_cache(maxsize=None)
def keep_case(name):
    """(mask (B,h,w), bg or None, rt, ct, keep (B, rt*ct) float32)"""
    rng = np.random.RandomState(len(name) * 7 + 1)
    if name in ("scale 2", "scale 16"):
        (h, w, rt, ct) = (32, 48, 16, 24) if name == "scale 2" else (240, 320, 15, 20)
        B = 4
        mask = (rng.rand(B, h, w) < 0.5).astype(F32)
        bg = np.ones((B, h, w), F32)
        k = (h // rt) // 2 - 1                                  # the 2x2 block that cell (r, c) averages starts at (k, k) of its tile
        blk = lambda b, r, c: (b, slice(r * (h // rt) + k, r * (h // rt) + k + 2), slice(c * (w // ct) + k, c * (w // ct) + k + 2))
        # explained = 1 -> keep_px = 0.  Cells 0 .. 5 of pair 0: the interpolated value at 0, 1/4, 1/2 (two ways), 3/4, 1
        for c, pat in enumerate(([1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 1], [1, 0, 0, 0], [0, 0, 0, 0])):
            mask[blk(0, 0, c)] = np.array(pat, F32).reshape(2, 2)
        # pair 1: non-binary mask / bg with mask + (1 - bg) exactly 0.5 (not explained: kept) and just above (explained)
        half_up = np.nextafter(F32(0.5), F32(1))
        for c, (mv, bv) in enumerate(((0.5, 1.0), (half_up, 1.0), (0.25, 0.75), (0.25 + 2.0 ** -24, 0.75), (0.0, 0.5),
                                      (2.0 ** -24, 0.5))):
            mask[blk(1, 0, c)] = mv
            bg[blk(1, 0, c)] = bv
        bg[2] = (rng.rand(h, w) < 0.8).astype(F32)
        exact = True
    elif name == "non-dyadic":
        h, w, rt, ct, B = 96, 312, 10, 33, 2
        mask = np.stack([settle((rng.rand(h, w) < p).astype(F32), rt, ct) for p in (0.5, 0.3)])
        bg, exact = None, False
    elif name == "upsample":
        h, w, rt, ct, B = 3, 5, 7, 9, 2
        mask = np.stack([settle((rng.rand(h, w) < p).astype(F32), rt, ct) for p in (0.5, 0.3)])
        bg, exact = None, False
    else:
        assert name == "one pixel"
        h, w, rt, ct, B = 1, 1, 7, 9, 2
        mask = np.array([0.0, 1.0], F32).reshape(2, 1, 1)
        bg, exact = None, False
    keep = []
    for b in range(B):
        g = None if bg is None else bg[b]
        if exact:
            val, k = keep64(mask[b], g, rt, ct)
            v32, k32 = keep32(mask[b], g, rt, ct, False)
            _exact(val, v32, name)
            assert np.array_equal(k, k32) and np.array_equal(k, keep32(mask[b], g, rt, ct, True)[1])
        else:
            k = keep_nondyadic(mask[b], g, rt, ct)
        keep.append(k.ravel())
    keep = np.stack(keep).astype(F32)
    if exact:
        assert keep[0, :6].tolist() == [0, 0, 0, 0, 1, 1] and keep[1, :6].tolist() == [1, 0, 1, 0, 1, 0]
        val0 = keep64(mask[0], bg[0], rt, ct)[0].ravel()[:6]
        assert val0.tolist() == [0, 0.25, 0.5, 0.5, 0.75, 1.0]
    return mask, bg, rt, ct, keep


KEEP_CASES = ("scale 2", "scale 16", "non-dyadic", "upsample", "one pixel")


@gpu
@pytest.mark.parametrize("name", KEEP_CASES, ids=str)
def test_keep_mask_equals_the_float64_interpolation(dev, name):
    """ops.keep_mask against ATen's formula: interpolated values exactly at 0.5 (not kept), a quarter above and below,
    mask + (1 - bg) exactly at 0.5 and one ulp above; a non-dyadic ratio; upsampling with the clamp at 0; a 1x1 mask.  With and
    without an ``active`` list."""
    mask, bg, rt, ct, keep = keep_case(name)
    md = torch.from_numpy(mask).to(dev)
    bd = torch.from_numpy(bg).to(dev) if bg is not None else None
    _same(ops.keep_mask(md, bd, None, rt, ct), torch.from_numpy(keep), name)
    act = list(range(len(mask)))[::-1] + [0]
    _same(ops.keep_mask(md, bd, torch.tensor(act, dtype=torch.int32, device=dev), rt, ct), torch.from_numpy(keep[act]),
          name + ", active list")


FILTER_N = (0, 1, 1023, 1024, 1025, 2049)
FILTER_PATTERNS = ("all", "none", "alternate", "last lane", "one in trip 2", "random")


def filter_case(n):
    """One launch: a pair per keep pattern, cap = n + 7 > n.  The keep map is keep_case('scale 2') of pair 0 .. 3 (cycled); idx2
    points into kept / dropped cells as the pattern says, cells repeat; the coordinate tables hold distinct dyadic values."""
    mask, bg, rt, ct, keep = keep_case("scale 2")
    B, cap = len(FILTER_PATTERNS), n + 7
    rng = np.random.RandomState(n)
    i = np.arange(n)
    want = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternate": i % 2 == 1, "last lane": i % 64 == 63,
            "one in trip 2": i == 1024, "random": rng.rand(n) < 0.5}
    nc = rt * ct
    masks = np.stack([mask[b % len(mask)] for b in range(B)])
    bgs = np.stack([bg[b % len(bg)] for b in range(B)])
    idx1 = rng.randint(0, nc, (B, cap)).astype(np.int64)
    idx2 = np.full((B, cap), -12345, np.int64)                       # beyond count: never read
    for b, p in enumerate(FILTER_PATTERNS):
        k = keep[b % len(keep)] > 0
        on, off = np.flatnonzero(k), np.flatnonzero(~k)
        idx2[b, :n] = np.where(want[p], on[rng.randint(0, len(on), n)], off[rng.randint(0, len(off), n)])
    idx1[:, n:] = -12345
    xa, ya = np.arange(nc, dtype=F32) + F32(0.25), -np.arange(nc, dtype=F32) - F32(0.5)
    xb, yb = np.arange(nc, dtype=F32) * F32(2) + F32(0.125), np.arange(nc, dtype=F32) * F32(-4) - F32(0.75)
    count = np.full(B, n, np.int32)
    ref = []
    for b, p in enumerate(FILTER_PATTERNS):
        kept = np.flatnonzero(keep[b % len(keep)][idx2[b, :n]] > 0)
        assert np.array_equal(kept, np.flatnonzero(want[p]))
        m1, m2, kp = np.zeros((cap, 3), F32), np.zeros((cap, 3), F32), np.full(cap, -1, np.int32)
        a, c = idx1[b, kept], idx2[b, kept]
        m1[:len(kept)] = np.stack((xa[a], ya[a], np.ones(len(kept), F32)), 1)
        m2[:len(kept)] = np.stack((xb[c], yb[c], np.ones(len(kept), F32)), 1)
        kp[:len(kept)] = kept
        ref.append((m1, m2, len(kept), kp))
    return dict(masks=masks, bgs=bgs, rt=rt, ct=ct, idx1=idx1, idx2=idx2, count=count, xa=xa, ya=ya, xb=xb, yb=yb, ref=ref, cap=cap)


@gpu
@pytest.mark.parametrize("n", FILTER_N)
def test_filter_matches_keeps_the_reference_list_in_order(dev, n):
    """The ordered compaction over zero, one, exactly one and more than one 1024-item trip: all, none, every other item, only the
    last lane of each wavefront, only the first item of the second trip (n = 1025 and 2049), a random half.  Order, kept indices, count, zeroed padding and
    -1 in ``kept``; through an ``active`` list; and the ragged entry point on the same data."""
    c = filter_case(n)
    t = lambda v, dt=None: torch.from_numpy(np.ascontiguousarray(v)).to(dev) if dt is None else torch.tensor(v, dtype=dt, device=dev)
    B = len(FILTER_PATTERNS)
    act = [4, 2, 0, 5, 1, 3]
    args = (t(c["idx1"]), t(c["idx2"]), t(c["count"]))
    tabs = (t(c["xa"]), t(c["ya"]), t(c["xb"]), t(c["yb"]))

    def check(out, order, what):
        m1, m2, no, kept = out
        for k, b in enumerate(order):
            r1, r2, rn, rk = c["ref"][b]
            assert int(no[k]) == rn, (what, b, int(no[k]), rn)
            assert torch.equal(m1[k].cpu(), torch.from_numpy(r1)) and torch.equal(m2[k].cpu(), torch.from_numpy(r2)), (what, b)
            assert torch.equal(kept[k].cpu(), torch.from_numpy(rk)), (what, b)
        for o in out:
            o.fill_(-3)
    check(ops.filter_matches(*args, None, t(c["masks"]), t(c["bgs"]), c["rt"], c["ct"], *tabs, want_kept=True), range(B), "dense")
    check(ops.filter_matches(*args, t(act, torch.int32), t(c["masks"]), t(c["bgs"]), c["rt"], c["ct"], *tabs, want_kept=True), act,
          "dense, active list")
    h, w = c["masks"].shape[1:]
    nc = c["rt"] * c["ct"]
    geom = t([[h, w, c["rt"], c["ct"], 1, 1]] * B, torch.int32)
    moff, toff = t([b * h * w for b in range(B)], torch.int64), t([b * nc for b in range(B)], torch.int64)
    rep = lambda v: t(np.tile(v, B))
    check(ops.filter_matches_ragged(*args, t(act, torch.int32), t(c["masks"].ravel()), t(c["bgs"].ravel()), moff, geom, rep(c["xa"]),
                                    rep(c["ya"]), toff, rep(c["xb"]), rep(c["yb"]), toff, want_kept=True), act, "ragged")


ACCEPT_HW = ((1, 1), (7, 9), (8, 8), (5, 13), (5, 3277))          # HW = 1, 63, 64, 65, 64 * 256 + 1 against NPART = 64
P9999 = F32(0.9999)


def accept_case(hw, mode):
    """Six pairs.  Matchability: multiples of 2^-10 in [0, 1] with the values the comparisons turn on sprinkled in (1.0 and the
    float32 below it; float32(0.9999) and the float32 above it): every value is a multiple of 2^-24 and the sum of HW <= 2^15
    of them is exact in float64 in any order.  mask 0 / 1, bg 0 / 1 (pair 2: no pixel is background).
    pairs 0 .. 2 ordinary; 3: fewer than 4 matches; 4: RANSAC status 1; 5: nbH = 0 (accepted whatever the gain)."""
    h, w = hw
    HW, B = h * w, 6
    rng = np.random.RandomState(HW + mode)
    match = (rng.randint(0, 1025, (B, h, w)) / 1024.0).astype(F32)
    edge = np.array([1.0, np.nextafter(F32(1), F32(0)), P9999, np.nextafter(P9999, F32(1)), np.nextafter(P9999, F32(0))], F32)
    sel = rng.rand(B, h, w) < 0.3
    match[sel] = edge[rng.randint(0, len(edge), int(sel.sum()))]
    mask = (rng.rand(B, h, w) < 0.3).astype(F32)
    bg = (rng.rand(B, h, w) < 0.85).astype(F32)
    bg[2] = 1
    if HW == 1:
        mask[:], bg[:] = 0, 1
        match[:, 0, 0] = edge[[0, 1, 2, 3, 0, 3]]
    res = np.zeros((B, 4), np.int32)
    res[4, 0] = 1
    n_match = np.array([10, 4, 99, 3, 50, 4], np.int32)
    nbH = np.array([1, 2, 1, 1, 1, 0], np.int32)
    return match, mask, bg, res, n_match, nbH


def accept_ref(match, mask, bg, res, n_match, nbH, th, mode, act):
    """-> accept, gain, the updated masks.  act[k] = batch row of active pair k (match / res / n_match are per active pair)"""
    new = mask.copy()
    acc, gain = [], []
    for k, b in enumerate(act):
        HW = mask[b].size
        nf = (F32(1) - fg32(mask[b], bg[b]).astype(F32)).astype(F32)
        stat = ((match[k] > P9999).astype(F32) if mode else match[k]) * nf
        q = stat.astype(np.float64) * 2.0 ** 24
        assert np.array_equal(q, np.round(q)) and HW <= 2 ** 15            # exact in float64 whatever the order
        g = F32(np.float64(stat.astype(np.float64).sum()) / np.float64(HW))
        ok = n_match[k] >= 4 and res[k, 0] == 0 and (np.float64(g) > th or nbH[b] == 0)
        acc.append(int(ok))
        gain.append(g)
        if ok:
            v = (mask[b] + (match[k] * nf).astype(F32)).astype(F32)
            new[b] = ((v > P9999) if mode else (v >= F32(1))).astype(F32)
    return np.array(acc, np.int32), np.array(gain, F32), new


@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hw", ACCEPT_HW, ids=str)
def test_multih_accept_gain_rule_and_mask_update_at_equality(dev, hw, mode):
    """gain bit-equal to float32(float64(sum) / HW) with empty partials among the 64; th exactly the gain of a pair: not accepted;
    one float64 ulp below: accepted; the mask update at exactly 1.0 / one ulp below (mode 0) and at float32(0.9999) / one ulp
    above (mode 1); rejected pairs keep their masks.  Through an ``active`` list, and the ragged entry point on the same data."""
    match, mask, bg, res, n_match, nbH = accept_case(hw, mode)
    h, w = hw
    B = len(mask)
    act = [2, 0, 5, 3, 4, 1]
    mk = match[act]                                                    # the round's tensors are per ACTIVE pair
    rk, nk = res[act], n_match[act]
    _, gains, _ = accept_ref(mk, mask, bg, rk, nk, nbH, 0.0, mode, act)
    g0 = float(gains[1])                                               # pair 0's gain (active slot 1)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    for th in (g0, float(np.nextafter(np.float64(g0), -np.inf)), 0.0, 2.0):
        acc, gain, new = accept_ref(mk, mask, bg, rk, nk, nbH, th, mode, act)
        if g0 > 0:
            assert acc[1] == (0 if th >= g0 else 1)
        assert acc[2] == 1 and acc[3] == 0 and acc[4] == 0            # nbH = 0; too few matches; failed RANSAC
        for ragged in (False, True):
            md, nd = t(mask.copy()), t(nbH.copy())
            common = (t(act).int(), t(rk), t(nk), nd, th, mode)
            if not ragged:
                a_, g_ = ops.multih_accept(t(mk), md, t(bg), *common)
            else:
                geom = torch.tensor([[h, w, 1, 1, 1, 1]] * B, dtype=torch.int32, device=dev)
                moff = torch.arange(B, device=dev) * (h * w)
                a_, g_ = ops.multih_accept_ragged(t(mk.ravel()), torch.arange(B, device=dev) * (h * w), md.view(-1), t(bg.ravel()),
                                                  moff, geom, *common, h * w)
            what = "%s mode %d th %r%s" % (hw, mode, th, " ragged" if ragged else "")
            _same(g_.view(torch.int32), torch.from_numpy(gain.view(np.int32)), what + ": gain")
            _same(a_, torch.from_numpy(acc), what + ": accept")
            _same(md.view(B, h, w), torch.from_numpy(new), what + ": mask")
            _same(nd, torch.from_numpy(nbH + np.bincount(np.array(act)[acc == 1], minlength=B).astype(np.int32)), what + ": nbH")


# ====================================================================== the host side of every family
def test_family_invariants_hold_on_the_host(tmp_path_factory):
    """Everything the GPU tests take for granted, without a device: the exact fma against rationals; the band condition of every
    random RANSAC family and the expectations of the search cases (on the host build's H, which the device must reproduce bit
    for bit); the equality family; the cc reference against oracle/restate.py and the constructed patterns; ops.cc_max_area
    against brute force; the 0.5 margins of the keep maps; the exact sums of the accept family."""
    from test_oracle import _host_dlt_lib
    import restate
    lib = _host_dlt_lib(tmp_path_factory)
    # -- fma32 is one rounding: against exact rationals, and the double-rounded form is NOT (the tie family bites)
    a, b, c = fma_triples(3000, 1)
    got = fma32(a, b, c)
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got, want), "fma32: %d of %d differ from the rationals" % ((got != want).sum(), len(a))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (naive != want).sum() > 100
    # -- A: band condition and non-vacuity of the count cases, on the host build's H
    for n, N in COUNT_CASES:
        m1, m2, s = count_case(n, N)
        e, ref, gate = hyp_ref(lib, m1, m2, host_dlt(lib, m1[s], m2[s]), TOL)
        st, bc, win, nu = search_ref(s, ref)
        if n >= 63 and N >= 99:
            assert st == 0 and 0 < ref.max() < n and nu < N, (n, N)
            assert (s < 0).any() and s.min() >= -n
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac.npz"))
    e = err_ref(gold["m1_2"], gold["m2_2"], gold["score_H_2"])[1]           # what tests/test_gpu_kernels.py compares prediction with
    assert e.size == 360000 and no_band(e, 0.05)
    m1, m2, Hs = pred_case()
    _, e = err_ref(m1, m2, Hs)
    assert np.isnan(e).any() and np.isposinf(e).any() and np.isfinite(e).mean() > 0.8
    assert (e[0][np.isfinite(e[0])] < 1e-5).mean() > 0.5                        # inlier scale: the cancellation is there
    # a chain in the other order, or with its first multiply-add un-fused, is NOT within one ulp of the root at that scale
    x2, y2, z2 = (m2[None, :, k] for k in range(3))
    H0 = Hs[:1]
    rev = lambda k: fma32(x2, H0[:, k, None], fma32(y2, H0[:, k + 1, None], z2 * H0[:, k + 2, None]))
    unf = lambda k: fma32(z2, H0[:, k + 2, None], (y2 * H0[:, k + 1, None]).astype(F32) + (x2 * H0[:, k, None]).astype(F32))
    for alt in (rev, unf):
        with np.errstate(all="ignore"):
            px, py, pz = alt(0), alt(3), alt(6)
            dx, dy = m1[None, :, 0] - px / pz, m1[None, :, 1] - py / pz
            e_alt = np.sqrt(dx * dx + dy * dy)
        assert (~ulp_close(e_alt, e[:1])).sum() > 50
    for name in SEARCH_CASES:
        assert search_case_holds(lib, name), name
    cap, N, pairs = batch_case()
    for m1, m2, s in pairs[2:]:
        _, ref, _ = hyp_ref(lib, m1, m2, host_dlt(lib, m1[s], m2[s]), TOL)
        assert search_ref(s, ref)[0] == 0
    for tr in TRIPLES:
        m1, m2, s, e0 = equal_case(tr)
        H = host_dlt(lib, m1[s], m2[s])
        assert equal_family_holds(m1, m2, H, e0) and host_gate(lib, H)[EQ_ROWS].all(), tr
        for k in (-2, 2):
            assert no_band(err_ref(m1, m2, H)[1], _ulps(e0, k), 1), tr
    X, Y = dlt_case(4000)
    assert 0.2 < host_gate(lib, host_dlt(lib, X, Y))[:1333].mean() < 0.8
    for N in (63, 64, 65, 4000):                                          # flagged and unflagged systems in every DLT case
        fl = host_rank(lib, *dlt_case(N))
        assert fl[N // 3:2 * (N // 3)].all() and not fl[:N // 3].any() and not fl[2 * (N // 3):].all(), N
    # -- B: cc_ref against restate on a few maps; the patterns are what they are called; cc_max_area
    rng = np.random.RandomState(0)
    for H, W, a in ((5, 7, 2), (9, 13, 5), (4, 65, 3), (6, 6, 36), (3, 3, 9)):
        for dens in (0.4, 0.7, 1.1):
            m = paint(rng.rand(H, W) < dens)
            want = restate.remove_small_cc_eval(np.nan_to_num(m.copy(), nan=-2.0), TH, th_for(H * W, a))
            got = cc_ref(m[None], TH, a)[0].view(F32)
            assert np.array_equal(np.nan_to_num(got, nan=-2.0), want), (H, W, a, dens)
    for name in PATTERNS:
        m, cases, area = pattern_case(name)
        (a1, removed), (a0, kept) = cases
        with np.errstate(invalid="ignore"):
            fg = m > F32(TH)
        assert not (removed[fg] != 0).any() and (kept[fg] != 0).sum() >= area and a0 == a1 - 1, name
        if name in ONE_COMPONENT:
            assert area == int(fg.sum()), name
        if name.startswith("row wrap") and not name.endswith("x2"):
            assert area == 1, name
        for a in (a0, a1):
            assert ops.cc_max_area(m[0].size, th_for(m[0].size, a)) == a
    for size, areas in ((16, (0, 1, 3, 15, 16)), (2049 * 2050, (9,)), (15, (1, 3, 400)), (320, (1, 3, 400))):
        for a in areas:
            assert ops.cc_max_area(size, th_for(size, a)) == a
    for H in CC_H:
        for W in CC_W:
            for a in (1, 4, H * W):
                assert ops.cc_max_area(H * W, th_for(H * W, a)) == a
    for size in (1200, 465750, 1):
        for th in (0.0099, 0.01, 1 / 3, 0.0, 1e-7, 0.5, 0.999999, 1.0, 2.5e-6):
            assert ops.cc_max_area(size, th) == cc_max_area_brute(size, th), (size, th)
    m, ref = beyond_cap_case()
    small = cc_ref(m[None, 2000:, 1984:], TH, 9)[0]                   # the construction against the labelling on a corner crop
    assert np.array_equal(small, ref[2000:, 1984:])
    buf, maps = ragged_case()
    assert all(off % 64 for _, _, off in RAGGED[1:]) and len(buf) == RAGGED_TOTAL
    # -- C: the keep families (their own assertions run inside keep_case), the filter and the accept families
    for name in KEEP_CASES:
        mask, bg, rt, ct, keep = keep_case(name)
        assert 0 < keep.mean() < 1, name
    for n in FILTER_N:
        filter_case(n)
    for hw in ACCEPT_HW:
        for mode in (0, 1):
            match, mask, bg, res, n_match, nbH = accept_case(hw, mode)
            act = [2, 0, 5, 3, 4, 1]
            acc, gain, new = accept_ref(match[act], mask, bg, res[act], n_match[act], nbH, 0.0, mode, act)
            assert acc[2:].tolist() == [1, 0, 0, 1]
            if hw[0] * hw[1] >= 63:
                assert acc.tolist() == [1, 1, 1, 0, 0, 1]
                assert (gain > 0).all() and (new != mask).any()
                assert (match == P9999).any() and (match == 1).any()
