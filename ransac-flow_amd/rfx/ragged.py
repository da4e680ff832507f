"""What the drivers for batches of pairs of DIFFERENT sizes share on the host: the pure planners (which image goes into which bucket,
where a pair's masks sit in a packed buffer), the group-by-shape idiom (by_shape / rows / hand_back), the first-maximum choice of the
YFCC candidate search, and the packed explained-region masks of a batch's rounds (pack_bg, PackedBatch).  Imports neither pipeline
nor rounds: both use it.
"""
import collections

import numpy as np
import torch


def resize_dims(w, h, min_size, mode, stride=16):
    """ResizeMaxSize (quick_start/coarseAlignFeatMatch.py:80-90) / ResizeMinSize
    (evaluation/evalHpatch/coarseAlignFeatMatch.py:90-100)."""
    f = max if mode == "max" else min
    ratio = f(w / float(min_size), h / float(min_size))
    nw, nh = int(round(w / ratio)), int(round(h / ratio))
    return nw // stride * stride, nh // stride * stride


# ---------------------------------------------------------------- group by shape, stack, hand the rows back
def by_shape(keys):
    """OrderedDict key -> [indices i with keys[i] == key]: keys in order of first appearance, members ascending."""
    groups = collections.OrderedDict()
    for i, key in enumerate(keys):
        groups.setdefault(key, []).append(i)
    return groups


def mixed(*key_lists):
    """Does any of the lists hold more than one distinct key (sizes of the sources, of the targets, ...)?  True: the ragged path."""
    return any(len(set(keys)) > 1 for keys in key_lists)


def rows(ts, mem):
    """ts[m] for m in mem (each with a leading dimension) stacked along dimension 0; one member: that tensor itself, no copy."""
    return torch.cat([ts[m] for m in mem]) if len(mem) > 1 else ts[mem[0]]


def hand_back(dst, mem, t):
    """dst[mem[k]] = row k of ``t`` as a [k:k + 1] view (``t``: a tensor, or a dict of tensors -> a dict of views)."""
    for k, m in enumerate(mem):
        dst[m] = {key: v[k:k + 1] for key, v in t.items()} if isinstance(t, dict) else t[k:k + 1]


def choose_candidates(table):
    """The (B, K) host table of inlier counts -> per pair the FIRST maximum (np.argmax, evaluation/evalYFCC/evaluation.py:210)."""
    return np.asarray(table).argmax(axis=1).tolist()


# ---------------------------------------------------------------- planners: pure functions of the sizes
def packed_group_offsets(bhw_list):
    """Where the shape groups of a grouped fine stage sit in its packed buffers.  ``bhw_list``: one (B, h, w[, h8, w8]) per group, in
    group order (h8, w8: the /8 map size, default h // 8, w // 8).  Returns dict(off, off8, total, total8, shapes): group g's full-
    resolution maps start at element off[g] (B*h*w elements, one plane per pair), its /8 maps at off8[g] (B*h8*w8; the two-channel
    /8 flow at 2 * off8[g]); total / total8 are the buffer sizes.  Pure Python: no device involved."""
    off, off8, shapes, t, t8 = [], [], [], 0, 0
    for e in bhw_list:
        B, h, w = int(e[0]), int(e[1]), int(e[2])
        h8, w8 = (int(e[3]), int(e[4])) if len(e) > 3 else (h // 8, w // 8)
        if B <= 0 or h <= 0 or w <= 0 or h8 <= 0 or w8 <= 0:
            raise ValueError("packed_group_offsets: empty group %r" % (tuple(e),))
        off.append(t)
        off8.append(t8)
        shapes.append((B, h, w, h8, w8))
        t += B * h * w
        t8 += B * h8 * w8
    return dict(off=off, off8=off8, total=t, total8=t8, shapes=shapes)


def ragged_plan(src_sizes, tgt_sizes, min_size, scales, mode="max"):
    """Bucket / offset plan of a ragged batch: pair b's source of size src_sizes[b] = (w, h) gives len(scales) pyramid levels and its
    target of size tgt_sizes[b] one more image, each resized by resize_dims exactly as the one-pair path does (multiples of 16).
    Images of EQUAL shape -- any level, any pair, sources and targets alike -- form one bucket: one dense problem of the grouped trunk
    pass.  Level index len(scales) stands for the target.  Pure function of the sizes (no tensors).
    Returns dict(levels[b][i] = (h, w) of image i of pair b, cells[b][i] = (h // 16, w // 16), nA[b], nB[b], offs[b][i] = column
    of level i in pair b's (C, nA) block, ldA / ldB = the largest nA / nB padded to a multiple of 4, cap = max_b min(nA, nB),
    buckets = {(h, w): [(b, i), ...]} in order of first appearance, members ordered sources first (by pair, level), then targets)."""
    nS = len(scales)
    levels, cells, nA, nB, offs = [], [], [], [], []
    for (sw, sh), (tw, th) in zip(src_sizes, tgt_sizes):
        lv = []
        for sc in scales:
            nw, nh = resize_dims(sw, sh, int(min_size * sc), mode)
            lv.append((nh, nw))
        nw, nh = resize_dims(tw, th, min_size, mode)
        lv.append((nh, nw))
        cl = [(h // 16, w // 16) for h, w in lv]
        o, off = [], 0
        for r, c in cl[:nS]:
            o.append(off)
            off += r * c
        levels.append(lv)
        cells.append(cl)
        offs.append(o)
        nA.append(off)
        nB.append(cl[nS][0] * cl[nS][1])
    buckets = collections.OrderedDict()
    for b, lv in enumerate(levels):
        for i, shp in enumerate(lv):
            buckets.setdefault(shp, [])
    for shp in buckets:
        mem = [(b, i) for b, lv in enumerate(levels) for i, x in enumerate(lv) if x == shp]
        buckets[shp] = sorted(mem, key=lambda m: (m[1] == nS, m[0], m[1]))
    pad4 = lambda n: (n + 3) // 4 * 4
    return dict(levels=levels, cells=cells, nA=nA, nB=nB, offs=offs, ldA=pad4(max(nA)), ldB=pad4(max(nB)),
                cap=max(min(a, b) for a, b in zip(nA, nB)), buckets=buckets, nS=nS, B=len(levels))


def ragged_multih_tables(plan):
    """The packed-mask tables of a ragged batch's multi-homography rounds, a pure function of the plan: pair b's explained-region mask
    (and background map) are the h*w floats at element ``moff[b]`` of one buffer of ``total`` floats, pair after pair without gaps,
    and ``geom[b]`` = (h, w, rt, ct, h8, w8): the resized target image (plan["levels"][b][nS]), its feature map
    (plan["cells"][b][nS]) and the /8 maps of the fine stage.  What rfx_filter_matches_ragged_f32 / rfx_multih_accept_ragged_f32 read."""
    nS = plan["nS"]
    moff, geom, pos = [], [], 0
    for b in range(plan["B"]):
        h, w = plan["levels"][b][nS]
        rt, ct = plan["cells"][b][nS]
        moff.append(pos)
        geom.append((h, w, rt, ct, h // 8, w // 8))
        pos += h * w
    return dict(moff=moff, geom=geom, total=pos)


def ragged_candidate_plan(src_sizes, cand_sizes, min_size, scales, mode="min"):
    """ragged_plan for pairs with K candidate targets each (the YFCC driver's rotations): ``cand_sizes[k][b]`` = (w, h) of candidate k
    of pair b.  Image index i < nS is pyramid level i of the source, nS + k is candidate k.  Returns ragged_plan's dict with
    levels[b] / cells[b] of nS + K entries, nB[k][b] (per candidate), ldB over all candidates, cap = max over (b, k) of
    min(nA[b], nB[k][b]), K, and buckets over ALL images (sources first, then targets by pair and candidate).  With K = 1 every
    entry but nB (one more list level) equals ragged_plan's.  Pure function of the sizes."""
    K = len(cand_sizes)
    plans = [ragged_plan(src_sizes, ts, min_size, scales, mode) for ts in cand_sizes]
    p0, nS, B = plans[0], plans[0]["nS"], plans[0]["B"]
    levels = [p0["levels"][b][:nS] + [p["levels"][b][nS] for p in plans] for b in range(B)]
    cells = [p0["cells"][b][:nS] + [p["cells"][b][nS] for p in plans] for b in range(B)]
    nB = [p["nB"] for p in plans]
    buckets = collections.OrderedDict()
    for lv in levels:
        for shp in lv:
            buckets.setdefault(shp, [])
    for shp in buckets:
        mem = [(b, i) for b, lv in enumerate(levels) for i, x in enumerate(lv) if x == shp]
        buckets[shp] = sorted(mem, key=lambda m: (m[1] >= nS, m[0], m[1]))
    return dict(levels=levels, cells=cells, nA=p0["nA"], nB=nB, offs=p0["offs"], ldA=p0["ldA"], ldB=max(p["ldB"] for p in plans),
                cap=max(p["cap"] for p in plans), buckets=buckets, nS=nS, B=B, K=K)


def ragged_variant_c_tables(plan, chosen):
    """ragged_multih_tables for a ragged_candidate_plan and the candidate ``chosen[b]`` of every pair: the packed-mask tables of the
    YFCC driver's rounds (moff, geom = (h, w, rt, ct, h8, w8) of the CHOSEN candidate's resized image, total)."""
    nS = plan["nS"]
    pick = lambda key: [plan[key][b][:nS] + [plan[key][b][nS + c]] for b, c in enumerate(chosen)]
    return ragged_multih_tables(dict(plan, levels=pick("levels"), cells=pick("cells")))


def resize_img_dims(w, h, stride, min_size):
    """outil.resizeImg (utils/outil.py:6-19): smaller side -> min_size, each side ROUNDED to a multiple of stride."""
    ratio = min(w / min_size, h / min_size)
    return int(round(w / ratio / stride) * stride), int(round(h / ratio / stride) * stride)


def ragged_kitti_tables(plan, tgt_sizes, fineSize):
    """The tables of a ragged batch's KITTI rounds, a pure function of the plan, the targets' ORIGINAL sizes ``tgt_sizes[b]`` = (w, h)
    and ``fineSize``: per pair org[b] = (h_org, w_org), resize[b] = (h_r, w_r) and half[b] = (h_d2, w_d2) = resize_img_dims at fineSize
    and fineSize // 2 (stride 8), d2[b] = (h_d2 // 8, w_d2 // 8) = the size of the half-resolution /8 flow.  The explained-region
    masks (and background maps) live at the ORIGINAL target size: pair b's h_org * w_org floats at ``moff[b]`` of one buffer of
    ``total`` floats, and geom[b] = (h_org, w_org, rt, ct, h_r // 8, w_r // 8) -- the mask's size, the coarse target feature map
    (plan["cells"][b][nS]) and the /8 maps of the full-resolution pass: what rfx_filter_matches_ragged_f32 /
    rfx_multih_accept_ragged_d2_f32 read."""
    nS = plan["nS"]
    out = dict(moff=[], geom=[], org=[], resize=[], half=[], d2=[])
    pos = 0
    for b, (w_org, h_org) in enumerate(tgt_sizes):
        w_r, h_r = resize_img_dims(w_org, h_org, 8, fineSize)
        w_d2, h_d2 = resize_img_dims(w_org, h_org, 8, fineSize // 2)
        rt, ct = plan["cells"][b][nS]
        out["moff"].append(pos)
        out["geom"].append((h_org, w_org, rt, ct, h_r // 8, w_r // 8))
        out["org"].append((h_org, w_org))
        out["resize"].append((h_r, w_r))
        out["half"].append((h_d2, w_d2))
        out["d2"].append((h_d2 // 8, w_d2 // 8))
        pos += h_org * w_org
    out["total"] = pos
    return out


# ---------------------------------------------------------------- the packed masks of a batch's rounds
def pack_bg(It_bg, sizes, device):
    """The background maps of a ragged batch as ONE float buffer, pair after pair like the masks: ``It_bg[b]`` = an (h, w) tensor of
    ``sizes[b]`` = (h, w), or None = all ones.  None, or a list of nothing but None: no background, None."""
    if It_bg is None:
        return None
    if len(It_bg) != len(sizes):
        raise ValueError("It_bg of a ragged batch: one (h, w) tensor (or None) per pair, got %d for %d pairs" % (len(It_bg), len(sizes)))
    for x, hw in zip(It_bg, sizes):
        if x is not None and tuple(x.shape) != tuple(hw):
            raise ValueError("It_bg entry of shape %s for a target of %s" % (tuple(x.shape), tuple(hw)))
    if all(x is None for x in It_bg):
        return None
    return torch.cat([torch.ones(h * w, dtype=torch.float32, device=device) if x is None else x.to(device).float().reshape(-1)
                      for x, (h, w) in zip(It_bg, sizes)])


class PackedBatch:
    """What the rounds of a ragged batch read besides its features, made from the tables ``tabs`` of a planner (moff, geom, total):
    ONE pinned upload cut into ``moff`` (B,) int64, ``geom`` (B,6) int32 and ``extra`` (B,.) int32 (``extra_rows``: further integers
    per pair, KITTI's d2 sizes); the packed background ``bg`` (pack_bg over the mask sizes geom[b][:2]); and, with ``masks``, the
    packed explained-region ``Mask`` (all zero) and the homography counts ``nbH``."""

    def __init__(self, tabs, It_bg, device, extra_rows=None, masks=True):
        B = len(tabs["moff"])
        self.tabs = tabs
        self.bg = pack_bg(It_bg, [g[:2] for g in tabs["geom"]], device)
        host = tabs["moff"] + [v for g in tabs["geom"] for v in g] + [v for r in extra_rows or () for v in r]
        tab = torch.tensor(host, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        self.moff, self.geom = tab[:B], tab[B:7 * B].to(torch.int32).view(B, 6)
        self.extra = tab[7 * B:].to(torch.int32).view(B, -1) if extra_rows else None
        if masks:
            self.Mask = torch.zeros(tabs["total"], dtype=torch.float32, device=device)
            self.nbH = torch.zeros(B, dtype=torch.int32, device=device)

    def fields(self):
        """The entries of a round group's ``batch`` dict."""
        return dict(tabs=self.tabs, bg=self.bg, moff=self.moff, geom=self.geom, Mask=self.Mask, nbH=self.nbH)

    def mask_of(self, b):
        o, (h, w) = self.tabs["moff"][b], self.tabs["geom"][b][:2]
        return self.Mask[o:o + h * w].view(h, w)
