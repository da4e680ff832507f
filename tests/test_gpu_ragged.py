"""Ragged batches (pairs of different sizes in one call): every pair's results equal, bit for bit, what the pair gives alone.

Kernel level: rfx_mutual_nn_ragged_f32 against rfx_mutual_nn_f32 per pair, rfx_l2norm_nchw_scatter_f32 against rfx_l2norm_nchw_f32
per image, rfx_gather_matches_ragged_f32 against rfx_gather_matches_f32 per pair.  Pipeline level: coarse() and align_pairs(fine=True)
on a mixed-size batch against the same pairs run one at a time through today's path."""
import numpy as np
import pytest
import torch

from rfx import ops, weights, synth
from rfx.pipeline import AlignPipeline

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
C = 1024


def _unit_features(n, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.rand((C, n), generator=g) ** 4            # non-negative like post-ReLU trunk features, with clear maxima
    return (f / f.norm(dim=0, keepdim=True)).to(DEV)


def _padded(feats, ld):
    out = torch.zeros((len(feats), C, ld), dtype=torch.float32, device=DEV)
    for b, f in enumerate(feats):
        out[b, :, :f.shape[1]] = f
    return out


# nA / nB not multiples of 4 or of 128; pair 1 below one tile on both axes; pair 2 far larger than the rest
SIZES = [(301, 250), (37, 61), (1531, 1203), (205, 3), (130, 129)]


@pytest.mark.parametrize("chunk", [0, "host", -1])
@pytest.mark.parametrize("masked", [False, True])
def test_mutual_nn_ragged_equals_single_pair_calls(chunk, masked):
    score_chunk = ops.resolve_score_chunk(chunk)[0]
    fa = [_unit_features(nA, 10 + b) for b, (nA, _) in enumerate(SIZES)]
    # targets: a permuted, slightly perturbed copy of part of the source, so that every pair has many mutual matches
    fb = []
    for b, (nA, nB) in enumerate(SIZES):
        g = torch.Generator().manual_seed(100 + b)
        src = fa[b][:, torch.randint(nA, (nB,), generator=g).to(DEV)]
        noisy = src + 0.02 * torch.rand(src.shape, generator=g).to(DEV)
        fb.append(noisy / noisy.norm(dim=0, keepdim=True))
    nA = [s[0] for s in SIZES]
    nB = [s[1] for s in SIZES]
    ldA, ldB = (max(nA) + 3) // 4 * 4, (max(nB) + 3) // 4 * 4
    masks = None
    if masked:
        masks = [torch.ones(n, device=DEV) for n in nB]
        for b, m in enumerate(masks):
            m[b % 3::5] = 0.0                            # zeroed target columns
    mask = _padded([m[None] for m in masks], ldB)[:, 0] if masked else None
    cap = max(min(a, b) for a, b in SIZES)
    idx1, idx2, cnt = ops.mutual_nn_ragged(_padded(fa, ldA), _padded(fb, ldB), torch.tensor(nA, dtype=torch.int32, device=DEV),
                                           torch.tensor(nB, dtype=torch.int32, device=DEV), max(nA), max(nB), maskB=mask,
                                           score_chunk=score_chunk, cap=cap)
    assert idx1.shape == (len(SIZES), cap)
    cnt = cnt.cpu().tolist()
    for b in range(len(SIZES)):
        # the single-pair call on the UNPADDED features (ld = n: the scalar k-major instance where n % 4 != 0)
        r1, r2 = ops.mutual_nn(fa[b].contiguous(), fb[b].contiguous(), maskB=masks[b] if masked else None, score_chunk=score_chunk)
        assert cnt[b] == r1.numel(), (b, cnt[b], r1.numel())
        assert torch.equal(idx1[b, :cnt[b]], r1) and torch.equal(idx2[b, :cnt[b]], r2), b
    assert cnt[3] <= 3 and max(cnt) > 100


def test_l2norm_scatter_and_gather_ragged_equal_the_dense_ops():
    g = torch.Generator().manual_seed(7)
    x = torch.relu(torch.randn((3, C, 5, 7), generator=g)).to(DEV)
    ld, B = 103, 3
    out = torch.full((B, C, ld), -1.0, device=DEV)
    offs = [0 * C * ld + 11, 2 * C * ld + 0, 1 * C * ld + 60]
    ops.l2norm_scatter(x, out, torch.tensor(offs, dtype=torch.int64, device=DEV), ld)
    for n, o in enumerate(offs):
        ref = ops.l2norm(x[n:n + 1])[0].reshape(C, 35)
        b, col = divmod(o, C * ld)
        assert torch.equal(out[b, :, col:col + 35], ref), n

    # gather: per-pair coordinate tables packed pair after pair
    nA, nB, cap = [40, 17, 90], [33, 50, 12], 30
    xa = [torch.rand(n, generator=g) for n in nA]
    ya = [torch.rand(n, generator=g) for n in nA]
    xb = [torch.rand(n, generator=g) for n in nB]
    yb = [torch.rand(n, generator=g) for n in nB]
    idx1 = torch.stack([torch.randint(n, (cap,), generator=g) for n in nA]).to(DEV)
    idx2 = torch.stack([torch.randint(n, (cap,), generator=g) for n in nB]).to(DEV)
    n = torch.tensor([30, 0, 12], dtype=torch.int32, device=DEV)
    offA = torch.tensor(np.cumsum([0] + nA[:-1]), dtype=torch.int64, device=DEV)
    offB = torch.tensor(np.cumsum([0] + nB[:-1]), dtype=torch.int64, device=DEV)
    cat = lambda t: torch.cat(t).to(DEV)
    M1, M2 = ops.gather_matches_ragged(idx1, idx2, n, cat(xa), cat(ya), offA, cat(xb), cat(yb), offB)
    for b in range(3):
        r1, r2 = ops.gather_matches(idx1[b:b + 1], idx2[b:b + 1], n[b:b + 1], xa[b].to(DEV), ya[b].to(DEV), xb[b].to(DEV),
                                    yb[b].to(DEV))
        assert torch.equal(M1[b], r1[0]) and torch.equal(M2[b], r2[0]), b


def _pairs():
    """6 pairs of 5 source sizes (pairs 0 and 3 share theirs), targets of their own size, plus a flat pair."""
    import PIL.Image as Image
    sizes = [(120, 160), (160, 120), (96, 128), (120, 160), (150, 200), (100, 140)]
    pairs = []
    for b, (h, w) in enumerate(sizes):
        I1, _ = synth.make_pair(h, w, seed=20 + b)
        _, I2 = synth.make_pair(h + 8 * (b % 2), w - 8 * (b % 3), seed=20 + b)
        pairs.append((I1, I2))
    flat = Image.new("RGB", (136, 104), (128, 128, 128))
    pairs.append((flat, flat.copy()))
    return pairs


def _pipe(degenerate, fine=False):
    sds = dict(trunk=weights.resnet50_trunk_sd(0))
    if fine:
        sds.update(feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2))
    return AlignPipeline(sds, nbScale=3, nbIter=200, tolerance=0.05, minSize=160, scaleR=1.2, device=DEV, degenerate=degenerate)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, torch.Tensor):
        return torch.equal(a.cpu(), b.cpu())
    return a == b


KEYS = ("index1", "index2", "n", "status", "count", "winner", "H", "inlier", "samples")


@pytest.mark.parametrize("mode", ["device_draw", "host_samples_lapack"])
def test_coarse_ragged_equals_each_pair_alone(mode):
    pairs = _pairs()
    ids = list(range(100, 100 + len(pairs)))
    pipe = _pipe("device" if mode == "device_draw" else "lapack")
    prep = pipe.prepare_ragged(pairs)
    plan = prep["plan"]
    assert len(plan["buckets"]) < 4 * len(pairs) and len({tuple(map(tuple, l)) for l in plan["levels"]}) >= 4

    def sample_fn_for(pid):
        return lambda b, n, it: torch.randint(n, (it, 4), generator=torch.Generator().manual_seed(pid))

    if mode == "device_draw":
        res = pipe.coarse(prep, pair_ids=ids)
    else:
        res = pipe.coarse(prep, sample_fn=lambda b, n, it: sample_fn_for(ids[b])(b, n, it))
    assert len(res) == len(pairs)
    for b, (p, pid) in enumerate(zip(pairs, ids)):
        one = pipe.prepare([p])
        alone = (pipe.coarse(one, pair_ids=[pid]) if mode == "device_draw" else pipe.coarse(one, sample_fn=sample_fn_for(pid)))[0]
        for k in KEYS:
            assert _same(res[b].get(k), alone.get(k)), (b, k)
        if alone["n"] < 4:
            assert res[b]["H"] is None
    assert sum(r["H"] is not None for r in res) >= len(pairs) - 1


def test_align_pairs_ragged_fine_equals_each_pair_alone():
    pairs = _pairs()[:5]
    ids = list(range(len(pairs)))
    pipe = _pipe("device", fine=True)
    res = pipe.align_pairs(pairs, fine=True, pair_ids=ids)
    for b, p in enumerate(pairs):
        alone = pipe.align_pairs([p], fine=True, pair_ids=[b])[0]
        for k in ("index1", "H", "flow12", "flowDown", "img1_fine"):
            assert _same(res[b][k], alone[k]), (b, k)


def test_prepare_ragged_device_equals_prepare_ragged():
    pairs = _pairs()
    pipe = _pipe("device")
    a = pipe.prepare_ragged(pairs)
    up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(DEV)
    d = pipe.prepare_ragged_device([up(p[0]) for p in pairs], [up(p[1]) for p in pairs])
    assert list(a["plan"]["buckets"]) == list(d["plan"]["buckets"])
    for x, y in zip(a["bucket_x"], d["bucket_x"]):
        assert torch.equal(x, y)
    for k in ("IsTensor", "ItTensor"):
        for x, y in zip(a[k], d[k]):
            assert torch.equal(x, y), k


def test_same_size_batches_keep_the_dense_path():
    pipe = _pipe("device")
    I1, I2 = synth.make_pair(120, 160, seed=3)
    J1, J2 = synth.make_pair(120, 160, seed=4)
    assert "ragged" not in pipe.prepare([(I1, I2), (J1, J2)])
    assert pipe.prepare_ragged([(I1, I2), (J1, J2)])["ragged"]
