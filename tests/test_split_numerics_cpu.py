"""The operand splitting of the split convolution kernels (csrc/conv1x1s.hip, csrc/conv3x3s.hip), on the host: ops.split_weights'
round-to-nearest-even pieces sum back exactly, and the three products the kernels drop (wm*xl + wl*xm + wl*xl) stay below
2^-24 (1 + 2^-10) |w x| -- the figure the kernel comments cite.

Analysis (normal float32 w, x; scale so that 1 <= |w| < 2): hi = bf16(w) leaves |w - hi| <= 2^-8 (half a bf16 ulp of 2^-7), so
|wm| <= 2^-8; mid = bf16(w - hi) has an ulp of at most 2^-16 (its magnitude is below 2^-8), so |wl| <= 2^-17.  Hence
|wm xl| + |wl xm| + |wl xl| <= 2 * 2^-8 * 2^-17 + 2^-34 = 2^-24 (1 + 2^-10) with |w|, |x| >= 1.  The bound is nearly attained:
w = x = 1 + 2^-8 - 2^-17 has hi = 1, mid = 2^-8 (a tie rounded to even), lo = -2^-17, and a dropped sum of 2^-24 (1 - 2^-10) against
|w x| = (1 + 2^-8 - 2^-17)^2: a ratio of 2^-24.013."""
import numpy as np
import torch

from rfx import ops


def _pieces_via_split_weights(v):
    """hi, mid, lo of a 1-D float32 tensor, through ops.split_weights' packing (one row of Cin = len(v) weights)."""
    n = v.numel()
    assert n % 16 == 0
    wS = ops.split_weights(v.view(1, n))
    pc = wS.view(torch.bfloat16).float().view(n // 16, 3, 2, 128, 8)[:, :, :, 0, :]   # [kb][piece][h][8], row m = 0
    return pc.permute(1, 0, 2, 3).reshape(3, n)


def _test_values():
    g = np.random.default_rng(5)
    rnd = (g.standard_normal(4096) * np.exp2(g.integers(-60, 60, 4096))).astype(np.float32)
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -23)
    edges = []
    for e in (-30, -1, 0, 1, 7, 40):
        b = np.float32(2.0 ** e)
        for k in range(0, 40):
            edges += [b + np.float32(k) * ulp * b, b - np.float32(k) * ulp * b / 2]
    # ties of every rounding step: hi + half a bf16 ulp (2^-8), mid's ties (2^-17 next to a multiple of 2^-16), both signs
    ties = []
    for m in range(0, 256, 7):
        base = one + np.float32(m) * np.float32(2.0 ** -7)
        for t in (2.0 ** -8, 2.0 ** -8 - 2.0 ** -17, 2.0 ** -9 + 2.0 ** -17, 2.0 ** -8 - 2.0 ** -16 + 2.0 ** -17, 2.0 ** -8 + 2.0 ** -17):
            ties += [base + np.float32(t), base - np.float32(t)]
    v = np.concatenate([rnd, np.array(edges, np.float32), np.array(ties, np.float32)])
    v = np.concatenate([v, -v])
    return torch.from_numpy(v[: v.size // 16 * 16].copy())


def test_split_weights_pieces_are_rne_and_sum_back_exactly():
    v = _test_values()
    hi, mid, lo = _pieces_via_split_weights(v)
    assert torch.equal(hi.double() + mid.double() + lo.double(), v.double())
    # each piece is the round-to-nearest-even bf16 of what the previous ones leave
    assert torch.equal(hi, v.bfloat16().float())
    assert torch.equal(mid, (v - hi).bfloat16().float())
    assert torch.equal(lo, (v - hi - mid).bfloat16().float())
    # the per-piece bounds the analysis uses, relative to the binade of v
    e = torch.floor(torch.log2(v.double().abs()))
    assert bool((mid.double().abs() <= torch.exp2(e - 8)).all())
    assert bool((lo.double().abs() <= torch.exp2(e - 17)).all())


def _dropped_ratio(w, x):
    wh, wm, wl = (p.double() for p in _pieces_via_split_weights(w))
    xh, xm, xl = (p.double() for p in _pieces_via_split_weights(x))
    return (wm * xl + wl * xm + wl * xl).abs() / (w.double() * x.double()).abs()


def _structured_pool(rng, n):
    """Values whose pieces are near their maximal sizes, over many binades and both signs: hi rounded down (v = 1 + r1) or up
    (v = 1 + 2^-7 - r1) by r1 = mid + lo, with mid anywhere in [2^-9, 2^-8] on its 2^-16 grid and lo a tie or a random
    remainder below 2^-17 -- mixed freely, so that the pool also holds many values far from the worst case."""
    mid = rng.integers(128, 257, n) * 2.0 ** -16
    lo = np.where(rng.random(n) < 0.5, rng.choice([-1.0, 1.0], n) * 2.0 ** -17, rng.integers(-15, 16, n) * 2.0 ** -21)
    r1 = np.minimum(mid + lo, 2.0 ** -8)
    sig = np.where(rng.random(n) < 0.5, 1.0 + r1, 1.0 + 2.0 ** -7 - r1)
    v = sig * np.exp2(rng.integers(-40, 41, n)) * rng.choice([-1.0, 1.0], n)
    return torch.from_numpy(v.astype(np.float32))


def test_dropped_cross_terms_bound():
    """Worst |wm xl + wl xm + wl xl| / |w x| by analysis (module docstring) and by a search: below 2^-24 (1 + 2^-10) everywhere.
    The search pairs two independent pools of structured values (other binades, mixed significands, both rounding directions of
    hi, every sign) at random and still comes within 2 % of the bound; random normal data over many binades stays lower."""
    bound = 2.0 ** -24 * (1 + 2.0 ** -10)
    # the analytic near-worst case
    a = torch.full((16,), 1 + 2.0 ** -8 - 2.0 ** -17, dtype=torch.float32)
    r_analytic = float(_dropped_ratio(a, a).max())
    assert 2.0 ** -24.02 < r_analytic < bound
    # search: 2^18 random (w, x) pairs of independent structured pools
    rng = np.random.default_rng(11)
    n = 1 << 18
    w, x = _structured_pool(rng, n), _structured_pool(rng, n)
    r_search = _dropped_ratio(w, x)
    worst = float(r_search.max())
    # random data, many binades
    g = torch.Generator().manual_seed(0)
    wr = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=g).float())
    xr = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=g).float())
    r_rand = float(_dropped_ratio(wr, xr).max())
    print("dropped cross terms / |w x|: analytic 2^%.3f, search 2^%.3f (%d pairs), random 2^%.3f, bound 2^%.4f"
          % (np.log2(r_analytic), np.log2(worst), n, np.log2(r_rand), np.log2(bound)))
    assert worst < bound and r_rand < bound
    assert worst > 2.0 ** -24 * 0.98            # the search reaches the analytic regime: the bound is tight, not just safe
