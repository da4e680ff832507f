"""Batched coarse-to-fine alignment of image pairs on one MI355X.

Restructures the reference's per-pair, host-driven flow (quick_start/align2images.py:53-97 on top of
quick_start/coarseAlignFeatMatch.py:92-173) for throughput: all pairs of a batch go through every
network layer in ONE launch per layer and pyramid scale (batch dimension = pairs), normalised features
are written straight into the concatenated (1024, nA) match matrix, and the host synchronises twice per
batch (match counts -> RANSAC index draw; final results) instead of >= 3 times per 100 RANSAC
hypotheses.  Semantics per pair are the reference's (variant A: ResizeMaxSize, or B: ResizeMinSize).

Host-side work that stays on the CPU: PIL LANCZOS pyramid + ToTensor/Normalize.
``prepare()`` does it and uploads; everything after runs on the device.
"""
import functools
import os

import numpy as np
import torch
import PIL.Image as Image

from . import ops, ragged, rounds, trunk_pass
from .cache import BoundedCache
from .nets import ResNet50Trunk, FeatureExtractorNet, NetFlowCoarseNet, NetMatchabilityNet
from .ragged import (packed_group_offsets, ragged_candidate_plan, ragged_kitti_tables, ragged_multih_tables,      # noqa: F401
                     ragged_plan, ragged_variant_c_tables, resize_dims, resize_img_dims)     # importable from here by name too

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def scale_list(nb_scale, scale_r):
    """quick_start/coarseAlignFeatMatch.py:70-74."""
    if nb_scale == 1:
        return [1]
    half = nb_scale // 2 + 1
    return np.linspace(scale_r, 1, half).tolist() + np.linspace(1, 1 / scale_r, half).tolist()[1:]


def pil_to_tensor(pil):
    arr = np.asarray(pil, dtype=np.uint8)
    return torch.from_numpy(arr.copy()).permute(2, 0, 1).contiguous().float().div(255)


def backgrounds_of_masks(masks, out_hw_list, k_list=None):
    """ops.sky_background per group of masks that share (shape, output size, turns) -> one (h, w) map per mask, in order."""
    k_list = [0] * len(masks) if k_list is None else [int(k) % 4 for k in k_list]
    keys = [(tuple(m.shape), (int(hw[0]), int(hw[1])), k) for m, hw, k in zip(masks, out_hw_list, k_list)]
    out = [None] * len(masks)
    for (_, hw, k), mem in ragged.by_shape(keys).items():
        bg = ops.sky_background(torch.stack([masks[j] for j in mem]), hw, k)
        for row, j in enumerate(mem):
            out[j] = bg[row]
    return out


def sky_backgrounds(seg, tgt_u8_list, out_hw_list, k_list=None, max_batch=None):
    """The scripts' --segNet step for a list of targets, on the device: ``It_bg = imresize(np.rot90(skyFromSeg(target), k), (h, w))
    < 128`` (evaluation/evalHpatch/evaluation.py:177-180, evalYFCC/evaluation.py:185-200) per target.  seg: a segnet.SegNetDevice;
    tgt_u8_list: (H, W, 3) uint8 device tensors (or PIL images); out_hw_list: the (h, w) of each map; k_list: quarter turns of
    each mask before the resize (default none); max_batch: get_sky_batch's (default: its own).  get_sky_batch, then
    ops.sky_background per (shape, size, turns) group: no host resize, no mask download, no (N, 150, H, W) tensor.
    -> list of (h, w) float32 device maps, what the drivers take as It_bg."""
    if len(out_hw_list) != len(tgt_u8_list) or (k_list is not None and len(k_list) != len(tgt_u8_list)):
        raise ValueError("one output size (and one number of turns) per target")
    masks = seg.get_sky_batch(tgt_u8_list) if max_batch is None else seg.get_sky_batch(tgt_u8_list, max_batch=max_batch)
    return backgrounds_of_masks(masks, out_hw_list, k_list)


_CELL_COORDS = BoundedCache(64)


def cell_coords_cached(n_rows, n_cols, device):
    """cell_coords() memoised per (shape, device): the grids are constants of the map size (a dozen tiny ATen launches per
    pyramid level and step otherwise).  LRU-bounded (64 shapes: a stream of variable-size pairs must not grow it for ever); a
    captured HIP graph that read an entry holds it by lease (trunk_pass.graphed)."""
    return _CELL_COORDS.get((n_rows, n_cols, str(device)), lambda: cell_coords(n_rows, n_cols, device))


def cell_coords(n_rows, n_cols, device):
    """outil.getWHTensor (utils/outil.py:21-24): (W = row coordinate, H = column coordinate).
    Evaluated on the CPU and uploaded: ``(i + 0.5) / n`` is a true IEEE division there, while ATen's device kernel for
    tensor / python-scalar multiplies by the rounded reciprocal -- 40 % of the cell centres come out one float32 ulp
    (1.2e-7) away (scripts/dbg/cell_coords_check.py).  The CPU reference is the parity target: with its coordinates the
    RANSAC inputs are the oracle's bit for bit (the 1-ulp offset used to reach H as up to 4e-7, and as 4e-6 through an
    ill-conditioned 4-point sample)."""
    r = (torch.arange(n_rows, dtype=torch.float32) + 0.5) / n_rows
    c = (torch.arange(n_cols, dtype=torch.float32) + 0.5) / n_cols
    W = r.view(-1, 1).expand(n_rows, n_cols).reshape(-1)
    Hh = c.view(1, -1).expand(n_rows, n_cols).reshape(-1)
    return ((W - 0.5) * 2).to(device), ((Hh - 0.5) * 2).to(device)


class AlignPipeline:
    def __init__(self, sds, nbScale=7, nbIter=1000, tolerance=0.05, minSize=640, scaleR=1.2, variant="A",
                 device="cuda", kernelSize=7, draw="device", seed=0, degenerate="lapack", score_chunk=None):
        """``draw``: where the RANSAC index draw of utils/outil.py:120 happens when no explicit ``samples`` / ``sample_fn`` is
        given.  "device" (default; the reference draws on ``match1.device``, i.e. on the GPU in a GPU run): Philox4x32-10 on
        the device keyed by (``seed``, call counter, pair, hypothesis) -- no host sync for nbMatch, no CPU draw + upload.
        "host": ``torch.randint`` on the CPU generator per pair in pair order = what a CPU run of the reference draws
        (the parity mode: the oracle can replay it from ``torch.manual_seed``).
        ``score_chunk``: how the mutual-NN scores are summed (ops.resolve_score_chunk, resolved HERE, once): None = RFX_SCORE_CHUNK
        or the fixed default of 256 products per chunk; an int; "host" = the K blocking of this host's sgemm (scores bit-equal to
        the reference's torch.mm on this host: the parity modes).  The resolved value and its origin are attributes
        (``score_chunk``, ``score_chunk_source``) and an explicit argument of every mutual-NN launch of THIS pipeline."""
        self.score_chunk, self.score_chunk_source = ops.resolve_score_chunk(score_chunk)
        if draw not in ("device", "host"):
            raise ValueError("draw must be 'device' or 'host'")
        if degenerate not in ("auto", "device", "lapack"):
            raise ValueError("degenerate must be 'auto', 'device' or 'lapack'")
        # rank-deficient 4-point samples (ops.ransac_h4_batched): "lapack" (default since round 6: the EXACT mode) = re-solved by the
        # host's LAPACK like the reference does for every hypothesis -- the flagged samples go to pinned memory, librfxhost.so runs
        # numpy's own dgesdd on them on std::threads, one more host wait per RANSAC call, hidden under other device work by the
        # lock-step drivers (multi_h_batched: 0.985x of the "device" mode on BASELINE config 3); "device" = the Householder sweep's own
        # null vector for those samples (no host round trip; a valid vector of the 2-D null space, not LAPACK's pick);
        # "auto" (rounds 4-5's default) = lapack whenever the draw comes from the host, device otherwise
        self.degenerate = degenerate
        if degenerate == "lapack" or (degenerate == "auto" and draw == "host"):
            from . import _lapack
            _lapack.start()           # the exact mode's host LAPACK workers: started here, not inside the first round
        self.draw, self.seed, self._draw_calls = draw, int(seed), 0
        self.dev = torch.device(device)
        self.trunk = ResNet50Trunk(sds["trunk"], self.dev)
        self.feat = FeatureExtractorNet(sds["feat"], self.dev) if "feat" in sds else None
        self.flow = NetFlowCoarseNet(sds["flow"], kernelSize, self.dev) if "flow" in sds else None
        self.match = NetMatchabilityNet(sds["match"], kernelSize, self.dev) if "match" in sds else None
        self.nbIter, self.tol, self.minSize = nbIter, tolerance, minSize
        self.variant = variant
        self.scaleList = scale_list(nbScale, scaleR)
        self.mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)
        self.std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
        self._capture = trunk_pass.CapturePolicy(self.MAX_GRAPHS)       # which trunk-pass shapes replay a HIP graph
        self._graphs = self._capture.entries
        self._ids_cache = BoundedCache(16)      # pair-id tuple -> its device tensor (_draw_epoch)
        self._stream_pools = {}                 # purpose -> the side streams of _side_streams

    def _side_streams(self, purpose, n, exact=False):
        """``n`` pipeline-owned side streams for ``purpose``, the same ones call after call.  A pool grows on demand; with
        ``exact`` one of another size is rebuilt."""
        pool = self._stream_pools.setdefault(purpose, [])
        if exact and len(pool) != n:
            del pool[:]
        while len(pool) < n:
            pool.append(torch.cuda.Stream(device=self.dev))
        return pool[:n]

    def _degenerate_mode(self, host_draw):
        if self.degenerate == "auto":
            return "lapack" if host_draw else "device"
        return self.degenerate

    def reseed(self, seed):
        """Restart the device-side index-draw stream (same seed + same call sequence -> same draws)."""
        self.seed, self._draw_calls = int(seed), 0

    def _pair_draw(self, n, it):
        """Index draw of the per-pair drivers: the pipeline's draw mode for one pair with n matches."""
        if self.draw == "device":
            ids, epoch = self._draw_epoch(None)
            return self._device_draw(torch.tensor([n], dtype=torch.int32, device=self.dev), ids, epoch, 0)[0]
        return torch.randint(n, (it, 4))

    # which driver draws: part of the Philox stream id when pair_ids are given
    DRAW_TAG = dict(multi_h=0, coarse=1, kitti=2, variant_c_select=3, variant_c=4)

    def _draw_epoch(self, pair_ids, driver="multi_h", draw_epoch=0):
        """The key of a driver call's device draws besides (seed, round): ``pair_ids`` given (the caller's ABSOLUTE pair ids,
        one per pair of the batch) -> (ids on the device, epoch): a pair's hypotheses depend on (seed, its id, the driver, the
        caller's ``draw_epoch``, the round) only -- not on the batch it rides in, on which other pairs are still active, or on how
        a stream is sharded over ranks.  epoch = draw_epoch * 16 + the driver's tag: the quick_start search (coarse) and round 0 of
        a multi-homography loop work on the same match list and must not share their samples, and a caller that retries a pair
        passes another ``draw_epoch`` to draw afresh (draw_epoch 0 + multi_h = epoch 0: the keys of rounds 3-4 are unchanged).
        The id tensor is cached per id tuple and uploaded from pinned memory without blocking.
        ``None`` -> ids = positions in the batch and a per-pipeline call counter as the epoch (calls draw afresh)."""
        if pair_ids is None:
            self._draw_calls += 1
            return None, self._draw_calls
        key = tuple(int(i) for i in pair_ids)
        ids = self._ids_cache.get(key, lambda: torch.tensor(key, dtype=torch.int32).pin_memory().to(self.dev, non_blocking=True))
        return ids, int(draw_epoch) * 16 + self.DRAW_TAG[driver]

    def _device_draw(self, n_dev, ids=None, epoch=0, rnd=0):
        return ops.draw_samples(n_dev, self.nbIter, self.seed, (int(epoch) << 32) | int(rnd), ids)

    # ---------------------------------------------------------------- host pre-processing
    def _resize(self, I, size):
        w, h = I.size
        nw, nh = resize_dims(w, h, size, "max" if self.variant == "A" else "min")
        return I.resize((nw, nh), resample=Image.LANCZOS)

    def prepare(self, pairs, want_u8=False):
        """pairs: list of (Is, It) PIL images, all of one size.  Returns device-resident inputs.  ``want_u8``: also ``Is_u8``
        (B,h,w,3), the bytes IsTensor is x / 255 of (align_prepared(want_u8=True) samples them)."""
        nS = len(self.scaleList)
        src = [[] for _ in range(nS)]
        tgt, IsT, ItT, Is8 = [], [], [], []
        for Is_org, It_org in pairs:
            pyr = [self._resize(Is_org, int(self.minSize * s)) for s in self.scaleList]
            for i, im in enumerate(pyr):
                src[i].append(pil_to_tensor(im))
            IsT.append(src[nS // 2][-1])
            if want_u8:
                Is8.append(torch.from_numpy(np.asarray(pyr[nS // 2], dtype=np.uint8).copy()))
            It = self._resize(It_org, self.minSize)
            tgt.append(pil_to_tensor(It))
        norm = lambda lst: ((torch.stack(lst) - self.mean) / self.std).to(self.dev)
        return dict(src=[norm(s) for s in src], tgt=norm(tgt), IsTensor=torch.stack(IsT).to(self.dev),
                    ItTensor=torch.stack(tgt).to(self.dev), B=len(pairs), Is_u8=torch.stack(Is8).to(self.dev) if want_u8 else None)

    @staticmethod
    def _mixed_sizes(pairs):
        """Pairs of PIL images: do the sources, or the targets, come in more than one size?  (Then the ragged path.)"""
        return ragged.mixed([p[0].size for p in pairs], [p[1].size for p in pairs])

    def _upload_lists(self, pairs):
        """Pairs of PIL images -> (sources, targets): per side a list of uint8 (H,W,3) device tensors, every image uploaded once."""
        up = lambda im: torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(self.dev)
        return [up(p[0]) for p in pairs], [up(p[1]) for p in pairs]

    def upload_raw(self, pairs):
        """Raw uint8 images of a batch -> device (N,H,W,3) tensors (what a decoder would leave in HBM)."""
        src = torch.from_numpy(np.stack([np.asarray(p[0].convert("RGB"), dtype=np.uint8) for p in pairs])).to(self.dev)
        tgt = torch.from_numpy(np.stack([np.asarray(p[1].convert("RGB"), dtype=np.uint8) for p in pairs])).to(self.dev)
        return src, tgt

    def prepare_device(self, src_u8, tgt_u8):
        """Same result as ``prepare`` -- bit for bit -- with the LANCZOS pyramid, ToTensor and Normalize computed on
        the device from raw uint8 (N,H,W,3) images: Pillow's fixed-point resampler and the float
        conversions are reproduced exactly by rfx_lanczos_pass_u8 / rfx_u8_to_f32_chw."""
        mode = "max" if self.variant == "A" else "min"
        B, h, w, _ = src_u8.shape
        srcs, IsT, Is8 = [], None, None
        mid = len(self.scaleList) // 2
        for i, sc in enumerate(self.scaleList):
            nw, nh = resize_dims(w, h, int(self.minSize * sc), mode)
            im = ops.lanczos_resize_u8(src_u8, nw, nh)
            raw, norm = ops.u8_to_f32(im, IMAGENET_MEAN, IMAGENET_STD, want_raw=(i == mid))
            srcs.append(norm)
            if i == mid:
                IsT, Is8 = raw, im
        ItT, tnorm = self.prepare_target_device(tgt_u8)
        return dict(src=srcs, tgt=tnorm, IsTensor=IsT, ItTensor=ItT, B=B, Is_u8=Is8)

    def prepare_target_device(self, tgt_u8):
        """The target half of prepare_device: raw uint8 (N,H,W,3) -> (ItTensor raw, normalised), resized like setTarget does."""
        mode = "max" if self.variant == "A" else "min"
        th, tw = tgt_u8.shape[1], tgt_u8.shape[2]
        nw, nh = resize_dims(tw, th, self.minSize, mode)
        return ops.u8_to_f32(ops.lanczos_resize_u8(tgt_u8, nw, nh), IMAGENET_MEAN, IMAGENET_STD)

    # ---------------------------------------------------------------- sky masks (the scripts' --segNet)
    def _upload_targets(self, pairs):
        return [torch.from_numpy(np.asarray(p[1].convert("RGB"), dtype=np.uint8).copy()).to(self.dev) for p in pairs]

    def _target_resized_hw(self, h, w):
        """(rows, columns) of a target of (h, w) pixels after setTarget's resize: the size the drivers' It_bg has."""
        nw, nh = resize_dims(w, h, self.minSize, "max" if self.variant == "A" else "min")
        return nh, nw

    _backgrounds_of_masks = staticmethod(backgrounds_of_masks)
    sky_backgrounds = staticmethod(sky_backgrounds)      # pipe.sky_backgrounds(seg, targets, sizes[, turns])

    @staticmethod
    def _seg_or_bg(seg, It_bg):
        if seg is not None and It_bg is not None:
            raise ValueError("give either seg (It_bg is formed from the targets) or It_bg, not both")
        return seg is not None

    # ---------------------------------------------------------------- ragged batches (pairs of different sizes)
    def _ragged_prep(self, plan, norm, IsT, ItT):
        """norm[(b, i)]: (1,3,h,w) normalised image i of pair b (i >= nS: the targets) -> the ragged prep: one (N,3,h,w) tensor per
        bucket of the plan (members in the plan's order), the per-pair raw IsTensor / ItTensor (1,3,h,w) of the fine stage."""
        xs = [torch.cat([norm[m] for m in mem], dim=0) for mem in plan["buckets"].values()]         # always a copy: a bucket of its own
        return dict(ragged=True, plan=plan, B=plan["B"], bucket_x=xs, IsTensor=IsT, ItTensor=ItT)

    def _ragged_plan(self, src_sizes, tgt_sizes):
        return ragged_plan(src_sizes, tgt_sizes, self.minSize, self.scaleList, "max" if self.variant == "A" else "min")

    def prepare_ragged(self, pairs, want_u8=False):
        """prepare() for pairs of different sizes (PIL path).  Every image is resized, converted and normalised exactly as prepare()
        does it for its pair alone; images of one shape are stacked into one bucket (ragged_plan).  Returns a ragged prep, which
        features / coarse / fine_quickstart / align_prepared accept."""
        plan = self._ragged_plan([p[0].size for p in pairs], [p[1].size for p in pairs])
        nS, mid = plan["nS"], plan["nS"] // 2
        mean, std = self.mean, self.std
        norm, IsT, ItT, Is8 = {}, [], [], []
        for b, (Is_org, It_org) in enumerate(pairs):
            for i, s in enumerate(self.scaleList):
                im = self._resize(Is_org, int(self.minSize * s))
                t = pil_to_tensor(im)[None]
                norm[(b, i)] = ((t - mean) / std).to(self.dev)
                if i == mid:
                    IsT.append(t.to(self.dev))
                    if want_u8:                                  # the bytes IsTensor is x / 255 of, one (h,w,3) tensor per pair
                        Is8.append(torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).to(self.dev))
            t = pil_to_tensor(self._resize(It_org, self.minSize))[None]
            norm[(b, nS)] = ((t - mean) / std).to(self.dev)
            ItT.append(t.to(self.dev))
        return dict(self._ragged_prep(plan, norm, IsT, ItT), Is_u8=Is8 if want_u8 else None)

    def _prepare_lists_device(self, plan, src_list, cands, u8_out=None):
        """The device pre-processing of B sources and K lists of B targets (uint8 (H,W,3) device tensors) over ``plan`` (image nS + k
        of a pair = its target k): the LANCZOS pyramid and the float conversions run once per input shape and level -- one
        rfx_lanczos_pass_u8 / rfx_u8_to_f32_chw chain for all images that share both, whatever pair or list they belong to.
        Returns (norm[(b, i)], IsTensor[b], ItTensor[k][b]): the normalised images and the raw ones of the fine stage, (1,3,h,w).
        ``u8_out``: a list of B entries that receives each source's resized mid-level bytes (h,w,3), which the pass forms anyway."""
        nS, mid, B = plan["nS"], plan["nS"] // 2, plan["B"]
        norm, IsT, ItT = {}, [None] * B, [[None] * B for _ in cands]
        imgs = [(x, b, None) for b, x in enumerate(src_list)] + [(x, b, k) for k, c in enumerate(cands) for b, x in enumerate(c)]
        for (is_tgt, _), mem in ragged.by_shape([(k is not None, tuple(x.shape)) for x, _, k in imgs]).items():
            u8 = torch.stack([imgs[j][0] for j in mem])
            who = [imgs[j][1:] for j in mem]
            for i in ([nS + who[0][1]] if is_tgt else range(nS)):
                nh, nw = plan["levels"][who[0][0]][i]
                small = ops.lanczos_resize_u8(u8, nw, nh)
                raw, nrm = ops.u8_to_f32(small, IMAGENET_MEAN, IMAGENET_STD, want_raw=(i == mid or is_tgt))
                ragged.hand_back(norm, [(b, i if k is None else nS + k) for b, k in who], nrm)
                if is_tgt:
                    for j, (b, k) in enumerate(who):
                        ItT[k][b] = raw[j:j + 1]
                elif i == mid:
                    ragged.hand_back(IsT, [b for b, _ in who], raw)
                    if u8_out is not None:
                        for j, (b, _) in enumerate(who):
                            u8_out[b] = small[j]
        return norm, IsT, ItT

    def prepare_ragged_device(self, src_list, tgt_list):
        """prepare_device() for pairs of different sizes: src_list / tgt_list = uint8 (H,W,3) device tensors, one per pair
        (_prepare_lists_device with one list of targets); equals prepare_ragged() bit for bit."""
        plan = self._ragged_plan([(x.shape[1], x.shape[0]) for x in src_list], [(x.shape[1], x.shape[0]) for x in tgt_list])
        Is8 = [None] * len(src_list)
        norm, IsT, ItT = self._prepare_lists_device(plan, src_list, [tgt_list], u8_out=Is8)
        return dict(self._ragged_prep(plan, norm, IsT, ItT[0]), Is_u8=Is8)

    def prepare_candidates_device(self, src_list, cands):
        """prepare_ragged_device for pairs with K candidate targets each (cands[k][b]: uint8 (H,W,3) device tensors).  Returns a
        ragged prep over a ragged_candidate_plan: bucket_x, K, IsTensor[b], ItTensor[k][b] (raw, (1,3,h,w))."""
        size = lambda x: (x.shape[1], x.shape[0])
        plan = ragged_candidate_plan([size(x) for x in src_list], [[size(x) for x in c] for c in cands], self.minSize, self.scaleList,
                                     "max" if self.variant == "A" else "min")
        return dict(self._ragged_prep(plan, *self._prepare_lists_device(plan, src_list, cands)), K=plan["K"])

    def _features_ragged(self, prep):
        """features() of a ragged prep: ONE grouped trunk pass over all buckets (nets.forward_group: one launch per kernel instance
        and layer for up to RFX_MAX_GROUP buckets) -- the sources' pyramid levels and every target -- then one
        rfx_l2norm_nchw_scatter_f32 per bucket and destination: sources into the padded featA (B,1024,ldA), target k of pair b into
        featB (K,B,1024,ldB).  Cell coordinates: per image, the tables of the one-pair path, packed pair after pair for the sources
        and list after list, pair after pair for the targets (offA / offB = where they begin, nB_dev / offB (K,B)).  A prep of two
        images per pair (no ``K``) is the K = 1 case with featB / nB / nB_dev / offB of its one list."""
        plan, B, K, dev = prep["plan"], prep["B"], prep.get("K", 1), self.dev
        nS, ldA, ldB = plan["nS"], plan["ldA"], plan["ldB"]
        nB = plan["nB"] if "K" in prep else [plan["nB"]]
        featA = torch.zeros((B, 1024, ldA), dtype=torch.float32, device=dev)
        featB = torch.zeros((K, B, 1024, ldB), dtype=torch.float32, device=dev)
        fs = self.trunk.forward_group(prep["bucket_x"])
        # all destination tables in one upload
        offs_host, spans = [], []
        for mem in plan["buckets"].values():
            k = sum(1 for m in mem if m[1] < nS)
            spans.append((k, len(offs_host), len(mem)))
            offs_host += [b * 1024 * ldA + plan["offs"][b][i] for b, i in mem[:k]] + [((i - nS) * B + b) * 1024 * ldB for b, i in mem[k:]]
        nB_flat = [n for per_k in nB for n in per_k]
        offA = np.cumsum([0] + plan["nA"][:-1]).tolist()
        offB = np.cumsum([0] + nB_flat[:-1]).tolist()
        tab = torch.tensor(offs_host + offA + offB, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        for f, (k, o, n) in zip(fs, spans):
            if k:
                ops.l2norm_scatter(f[:k], featA, tab[o:o + k], ldA)
            if k < n:
                ops.l2norm_scatter(f[k:], featB, tab[o + k:o + n], ldB)
        coords = lambda cells: [torch.cat(t) for t in zip(*[cell_coords_cached(r, c, dev) for r, c in cells])]
        WA, HA = coords([rc for b in range(B) for rc in plan["cells"][b][:nS]])
        Wt, Ht = coords([plan["cells"][b][nS + k] for k in range(K) for b in range(B)])
        no = len(offs_host)
        sizes = torch.tensor(plan["nA"] + nB_flat, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        out = dict(ragged=True, featA=featA, featB=featB, ldA=ldA, ldB=ldB, nA=plan["nA"], nB=nB, cap=plan["cap"], nA_dev=sizes[:B],
                   nB_dev=sizes[B:].view(K, B), WA=WA, HA=HA, Wt=Wt, Ht=Ht, offA=tab[no:no + B], offB=tab[no + B:].view(K, B),
                   offA_host=offA, offB_host=offB, _refs=(fs, tab))
        if "K" not in prep:
            out.update({key: out[key][0] for key in ("featB", "nB", "nB_dev", "offB")})
        return out

    def _mutual_ragged(self, feats, maskB=None):
        mask = None
        if maskB is not None:
            mask = (torch.stack(list(maskB)) if not isinstance(maskB, torch.Tensor) else maskB).float().contiguous()
        return ops.mutual_nn_ragged(feats["featA"], feats["featB"], feats["nA_dev"], feats["nB_dev"], max(feats["nA"]),
                                    max(feats["nB"]), maskB=mask, score_chunk=self.score_chunk, cap=feats["cap"])

    def _ragged_pair_feats(self, feats):
        """Per-pair views of a ragged feats dict's cell-coordinate tables (the keys _coarse_per_pair reads)."""
        out = []
        for b, (oA, oB) in enumerate(zip(feats["offA_host"], feats["offB_host"])):
            nA, nB = feats["nA"][b], feats["nB"][b]
            out.append(dict(HA=feats["HA"][oA:oA + nA], WA=feats["WA"][oA:oA + nA], Ht=feats["Ht"][oB:oB + nB],
                            Wt=feats["Wt"][oB:oB + nB]))
        return out

    def _fine_ragged(self, prep, Hs):
        """fine_quickstart of a ragged prep: the pairs grouped by (source, target) image shape, each group through today's dense
        batch kernels -- all groups as one chain of grouped launches (fine_quickstart_groups) with RFX_FINE_GROUPS on, one chain per
        group otherwise.  Returns one dict per pair, every tensor with a leading batch dimension of 1."""
        IsT, ItT = prep["IsTensor"], prep["ItTensor"]
        groups = list(ragged.by_shape([(tuple(s.shape), tuple(t.shape)) for s, t in zip(IsT, ItT)]).values())
        out = [None] * prep["B"]
        subs = [dict(IsTensor=torch.cat([IsT[b] for b in bs]), ItTensor=torch.cat([ItT[b] for b in bs])) for bs in groups]
        hs = [Hs[bs] for bs in groups]
        if ops.fine_groups_enabled():
            fs = self.fine_quickstart_groups(subs, hs)
        else:
            fs = [self.fine_quickstart(sub, h) for sub, h in zip(subs, hs)]
        for bs, f in zip(groups, fs):
            ragged.hand_back(out, bs, f)
        return out

    # ---------------------------------------------------------------- coarse stage
    def features(self, prep):
        """ResNet-50 conv4 features of every pyramid level and of the target, L2-normalised, written into
        featA (B,1024,nA) / featB (B,1024,nB) (quick_start/coarseAlignFeatMatch.py:92-125).

        Small batches (B <= 4) are launch-bound: ~900 kernel launches of a few workgroups each per pair cost more host time
        (Python + allocator + launch) than GPU time.  There the whole multi-stream trunk pass is captured ONCE per input
        shape into a HIP graph (``torch.cuda.CUDAGraph``: our ctypes launches go to torch's current stream, which is the
        capture stream) and replayed: one graph launch instead of ~900 (RFX_GRAPH=0 disables; never under ops.Profiler,
        whose per-launch events cannot be recorded into a graph)."""
        if prep.get("ragged"):
            return self._features_ragged(prep)
        if trunk_pass.graph_eligible(prep["B"]):
            return self._features_graphed(prep)
        return self._features_eager(prep)

    MAX_GRAPHS = 4      # captured shapes kept (LRU): each pins a private memory pool + static input / output buffers

    def _cell_coords(self, n_rows, n_cols):
        return cell_coords_cached(n_rows, n_cols, self.dev)

    def _features_eager(self, prep):
        return trunk_pass.features_eager(self, prep)

    def _features_graphed(self, prep):
        """HIP-graph replay of the trunk pass over the pyramid levels and the target (trunk_pass.graphed: captured at the SECOND
        sighting of a shape, at most MAX_GRAPHS captures kept)."""
        B = prep["B"]
        key = (tuple(tuple(x.shape) for x in prep["src"]), tuple(prep["tgt"].shape))
        body = lambda t: (None, self._features_eager(dict(src=list(t[:-1]), tgt=t[-1], B=B)))
        return trunk_pass.graphed(self, key, (*prep["src"], prep["tgt"]), body)[1]

    def prepare_and_features(self, src_u8, tgt_u8):
        """prepare_device + features -> (prep, feats).  Small batches (B <= 4): ONE HIP graph from the raw uint8 images to the
        normalised features -- the device pyramid (24 launches of tiny kernels per pair) is as launch-bound as the trunk pass, and
        a graph that starts at the raw images needs 2 input copies instead of 8.  Same capture policy and cache as _features_graphed;
        the returned ``prep`` tensors belong to the graph and are valid until its next replay.  Larger batches, RFX_GRAPH=0 or an
        active Profiler: the two eager calls."""
        if not trunk_pass.graph_eligible(src_u8.shape[0]):
            prep = self.prepare_device(src_u8, tgt_u8)
            return prep, self.features(prep)
        key = ("raw", tuple(src_u8.shape), tuple(tgt_u8.shape))

        def body(t):
            prep = self.prepare_device(*t)
            return prep, self._features_eager(prep)
        return trunk_pass.graphed(self, key, (src_u8, tgt_u8), body, what="pyramid + trunk pass")

    def coarse(self, prep, feats=None, samples=None, maskB=None, sample_fn=None, pair_ids=None, draw_epoch=0):
        """Per pair: mutual NN -> matches -> RANSAC.  Index draw (utils/outil.py:120): ``samples`` = list of (nbIter,4) int64
        CPU tensors, or ``sample_fn(b, nMatch, nbIter)`` -> such a tensor; otherwise the pipeline's ``draw`` mode -- "device":
        Philox on the device from the device-side match counts, ONE host sync per batch (the result records); "host":
        torch.randint on the CPU generator per pair, in pair order (what a CPU run of the reference draws), which needs the
        match counts on the host first (a second sync).  Returns a list of per-pair dicts (device tensors)."""
        feats = feats or self.features(prep)
        B = prep["B"]
        lib_out = []
        ragged = bool(feats.get("ragged"))
        # ONE batched mutual-NN launch chain for all pairs
        idx1, idx2, cnt = self._mutual_ragged(feats, maskB) if ragged else self._mutual_batched(feats, B, maskB)
        host_draw = not (samples is None and sample_fn is None and self.draw == "device")
        self._last_degenerate = {}
        if not host_draw:
            ids, epoch = self._draw_epoch(pair_ids, "coarse", draw_epoch)
            smp = self._device_draw(cnt, ids, epoch, 0)
            counts, draws = None, smp
        else:
            counts = cnt.cpu().tolist()  # <- sync: the host-side index draw needs nbMatch
            draws = []
            for b in range(B):
                n = counts[b]
                if n >= 4:
                    draws.append(samples[b] if samples is not None else
                                 (sample_fn(b, n, self.nbIter) if sample_fn is not None else torch.randint(n, (self.nbIter, 4))))
                else:
                    draws.append(torch.zeros((self.nbIter, 4), dtype=torch.int64))
            if len({tuple(d.shape) for d in draws}) != 1:       # explicit draws of different lengths: one launch chain per pair
                return self._coarse_per_pair(self._ragged_pair_feats(feats) if ragged else feats, idx1, idx2, counts, draws,
                                             self._degenerate_mode(True))
            smp = torch.stack(draws).to(self.dev, non_blocking=True)
        if ragged:
            M1, M2 = ops.gather_matches_ragged(idx1, idx2, cnt, feats["HA"], feats["WA"], feats["offA"], feats["Ht"], feats["Wt"],
                                               feats["offB"])
        else:
            M1, M2 = ops.gather_matches(idx1, idx2, cnt, feats["HA"], feats["WA"], feats["Ht"], feats["Wt"])
        bestH, inl, resd = ops.ransac_h4_batched(M1, M2, cnt, smp, self.tol, degenerate=self._degenerate_mode(host_draw),
                                                 info=self._last_degenerate)
        host = torch.cat((cnt[:, None], resd), dim=1).cpu().tolist()  # <- sync: result records (+ the match counts)
        for b in range(B):
            n, status, c, widx, nuniq = host[b]
            res = dict(index1=idx1[b, :n], index2=idx2[b, :n], H=None, inlier=None, samples=None, n=n)
            if n >= 4:
                res.update(match1=M1[b, :n], match2=M2[b, :n], samples=draws[b], status=status, count=c, winner=widx,
                           nUnique=nuniq)
                if status == 0:
                    res["H"], res["inlier"] = bestH[b], inl[b, :n]
            lib_out.append(res)
        return lib_out

    def _coarse_per_pair(self, feats, idx1, idx2, counts, draws, degenerate="device"):
        out = []
        for b, n in enumerate(counts):
            i1, i2 = idx1[b, :n], idx2[b, :n]
            res = dict(index1=i1, index2=i2, H=None, inlier=None, samples=None, n=n)
            if n >= 4:
                fb = feats[b] if isinstance(feats, list) else feats          # a list: per-pair tables of a ragged batch
                ones = torch.ones(n, dtype=torch.float32, device=self.dev)
                m1 = torch.stack((fb["HA"][i1], fb["WA"][i1], ones), dim=1)
                m2 = torch.stack((fb["Ht"][i2], fb["Wt"][i2], ones), dim=1)
                bestH, inl, r = ops.ransac_h4(m1, m2, draws[b].to(self.dev), self.tol, degenerate=degenerate)
                status, c, widx, nuniq = r.cpu().tolist()
                res.update(match1=m1, match2=m2, samples=draws[b], status=status, count=c, winner=widx, nUnique=nuniq)
                if status == 0:
                    res["H"], res["inlier"] = bestH, inl
            out.append(res)
        return out

    def _mutual_batched(self, feats, B, maskB=None):
        from . import _lib
        lib = _lib.load()
        nA, nB = feats["nA"], feats["nB"]
        ws = torch.empty(B * lib.rfx_mutual_nn_ws_bytes(nA, nB), dtype=torch.uint8, device=self.dev)
        cap = min(nA, nB)
        idx1 = torch.empty((B, cap), dtype=torch.int64, device=self.dev)
        idx2 = torch.empty((B, cap), dtype=torch.int64, device=self.dev)
        count = torch.zeros(B, dtype=torch.int32, device=self.dev)
        mask = None
        if maskB is not None:
            mask = (torch.stack(list(maskB)) if not isinstance(maskB, torch.Tensor) else maskB).float().contiguous()
        ldA = feats.get("ldA", nA)
        ops._call("rfx_mutual_nn_batched_f32", ops._one_device(feats["featA"], feats["featB"], mask), ops._p(feats["featA"]),
                  ldA, nA, 1024 * ldA, ops._p(feats["featB"]), nB, nB, 1024 * nB, 1024, ops._p(mask), ops._p(idx1),
                  ops._p(idx2), ops._p(count), ops._p(ws), B, int(self.score_chunk))
        return idx1, idx2, count

    # ---------------------------------------------------------------- fine stage
    def _stage(self, fn, *lists):
        """ops.stage on this pipeline's device, without side streams: the lock-step groups of the round drivers run on streams of
        their own."""
        return ops.stage(fn, *lists, device=self.dev, side_streams=False)

    def feat_l2norm(self, xs):
        """[l2norm(feat(x)) for x in xs] for image batches of different sizes, as one chain of stages."""
        return self._stage(ops.l2norm, self.feat.forward_group(xs, False))

    def _features_both(self, a_list, b_list):
        """Per group, both image batches through the FeatureExtractor as ONE batch -> (features of a, features of b)."""
        fs = self.feat_l2norm([torch.cat((a, b), dim=0) for a, b in zip(a_list, b_list)])
        return [f[:a.shape[0]] for f, a in zip(fs, a_list)], [f[a.shape[0]:] for f, a in zip(fs, a_list)]

    def fine_quickstart(self, prep, Hs):
        """quick_start/align2images.py:61-97 for a batch: Hs (B,3,3) device tensor."""
        return self.fine_quickstart_groups([prep], [Hs])[0]

    def fine_quickstart_groups(self, preps, Hs_list):
        """fine_quickstart for shape groups of different sizes: every stage is ONE ops.stage over the groups (one group: the eager
        launches; more than 8 groups: chunked by the library), bit-identical per group."""
        st = self._stage
        Is, It = [p["IsTensor"] for p in preps], [p["ItTensor"] for p in preps]
        fcs = st(lambda Hs, t: ops.warp_grid(Hs, t.shape[2], t.shape[3]), Hs_list, It)
        coarse = st(ops.grid_sample, Is, fcs)
        f1, f2 = self._features_both(coarse, It)
        corr = ops.corr_neigh_group(f1, f2)
        down = self.flow.forward_group(corr, False, False)
        f12 = st(lambda d, fc: ops.compose_flow(d, fc, clamp=False)[0], down, fcs)
        fine = st(ops.grid_sample, Is, f12)
        return [dict(flowCoarse=fcs[g], img1_coarse=coarse[g], feat1=f1[g], feat2=f2[g], corr12=corr[g], flowDown=down[g],
                     flow12=f12[g], img1_fine=fine[g]) for g in range(len(preps))]

    @staticmethod
    def _corr_both(featt, feats):
        """Per group (2B,49,h,w) = corr(featt, feats) | corr(feats, featt) (evaluation/evalHpatch/evaluation.py:29,34): both directions
        from ONE pass over the features (the reverse volume is the forward one at mirrored taps / shifted pixels:
        ops.corr_neigh_bidir).  RFX_CORR_BIDIR=0: the two directions as one launch over a doubled batch (each re-reads both feature
        maps), bit-identical."""
        if os.environ.get("RFX_CORR_BIDIR", "1") == "0":
            return ops.corr_neigh_group([torch.cat((ft, fs), dim=0) for ft, fs in zip(featt, feats)],
                                        [torch.cat((fs, ft), dim=0) for ft, fs in zip(featt, feats)])
        cs = [torch.empty((2 * ft.shape[0], 49, ft.shape[2], ft.shape[3]), dtype=torch.float32, device=ft.device) for ft in featt]
        ops.corr_neigh_bidir_group(featt, feats, outs=cs)
        return cs

    def _pred_heads(self, feats, featt, fcs, hw_list):
        """The part of the PredFlowMask chain that the plain and the cycle-checked forms share, over G shape groups: both correlation
        directions, the flow head and the matchability head (both matchability passes in one batch).  ``hw_list``: the size the
        group's full-resolution outputs have.  Returns (layout, new, cut, packed /8 flow, its per-group views, the one group's whole
        (2B,1,h/8,w/8) matchability or None, per-group (match12Down8, match21Down8), packed match12Down8, packed match21Down8);
        ``new(n)`` makes a flat buffer, ``cut(t)`` the per-group (B,1,h,w) views of a packed full-resolution buffer."""
        lay = packed_group_offsets([(fc.shape[0], hw[0], hw[1], ft.shape[2], ft.shape[3]) for fc, hw, ft in zip(fcs, hw_list, featt)])
        new = lambda n: torch.empty(n, dtype=torch.float32, device=self.dev)
        cut = lambda t: [t[o:o + B * h * w].view(B, 1, h, w) for (B, h, w, _, _), o in zip(lay["shapes"], lay["off"])]
        cut8 = lambda t, c=1: [t[c * o8:c * (o8 + B * h8 * w8)].view(B, c, h8, w8) for (B, _, _, h8, w8), o8 in zip(lay["shapes"], lay["off8"])]
        cs = self._corr_both(featt, feats)
        f8 = new(2 * lay["total8"])
        fd8 = self.flow.forward_group([c[:c.shape[0] // 2] for c in cs], False, False, outs=cut8(f8, 2))
        if len(fcs) == 1:
            # one group's batch is written as a whole: the last convolution is one launch over its 2B volumes
            md = self.match.forward_group(cs, False, False)[0]
            halves = [(md[:md.shape[0] // 2], md[md.shape[0] // 2:])]
            m12, m21 = halves[0][0].reshape(-1), halves[0][1].reshape(-1)
        else:
            md, m12, m21 = None, new(lay["total8"]), new(lay["total8"])
            halves = self.match.trunk.forward_group(cs, False, halves_out=list(zip(cut8(m12), cut8(m21))))
        return lay, new, cut, f8, fd8, md, halves, m12, m21

    def _pred_flow_mask_cycle_lists(self, feats, featt, fcs, out_hw_list=None, out=None):
        """The cycle-checked PredFlowMask chain after the features over G shape groups (pred_flow_mask_lists' ``cycle`` form takes one):
        the shared heads, then ONE stage of ops.cycle_tail, which writes every group's match straight into the packed buffer.  Group g's
        outputs live at out_hw_list[g] (default: its coarse grid's size).  Per group bit-identical to the one-group form; returns and
        ``out`` as pred_flow_mask_lists' plain form."""
        hws = [tuple(fc.shape[1:3]) if hw is None else (int(hw[0]), int(hw[1])) for fc, hw in zip(fcs, out_hw_list or [None] * len(fcs))]
        lay, new, cut, f8, fd8, _, halves, m12, m21 = self._pred_heads(feats, featt, fcs, hws)
        packed = new(lay["total"])
        match = cut(packed)
        tails = self._stage(lambda d, h, fc, hw, m_out: ops.cycle_tail(d, h[0], h[1], fc, out_hw=hw, match_out=m_out[:, 0]),
                            fd8, halves, fcs, hws, match)
        if out is not None:
            out.update(match=packed, flowDown8=f8, match12Down8=m12, match21Down8=m21, layout=lay)
        return [dict(flow12=tails[g][0], match=match[g], flowDown8=fd8[g], match12Down8=halves[g][0], match21Down8=halves[g][1])
                for g in range(len(fcs))]

    def pred_flow_mask_lists(self, feats, featt, fcs, cycle=False, out_hw=None, out=None):
        """The PredFlowMask chain after the features, written once, over G shape groups: group g = normalised source features
        feats[g] and target features featt[g] (B_g,256,h/8,w/8) and the coarse grid fcs[g] (B_g,h,w,2).  Both correlation directions,
        the flow head and the matchability head (both matchability passes in one batch), then one of two tails:
          * plain (evaluation/evalHpatch/evaluation.py:23-55): match = match12 * in-bounds(flow12);
          * ``cycle`` (evalYFCC/evaluation.py:32-58, evalKITTI/evaluation.py:49-81): match = match12 * grid_sample(match21, flowUp) *
            in-bounds(flow12), at ``out_hw`` (default: the coarse grid's size).  One group per call (ValueError otherwise).
        Every step is ONE ops.stage over the groups, so one group issues the eager launches.  Returns one dict per group (flow12,
        match, flowDown8, match12Down8, match21Down8).  flowDown8 -- and, in the plain form, match, match12Down8 and match21Down8 --
        are views of ONE packed buffer each, groups in order (packed_group_offsets; one group: the group's own tensors); ``out``
        (plain form): a dict that receives those buffers under the same keys (what rfx_multih_accept_ragged_f32 reads), plus
        ``layout``."""
        G = len(fcs)
        if cycle and G > 1:
            raise ValueError("the cycle-checked PredFlowMask forms take one shape group per call, got %d" % G)
        lay, new, cut, f8, fd8, md, halves, m12, m21 = self._pred_heads(feats, featt, fcs, [fc.shape[1:3] for fc in fcs])
        if cycle:
            B = fcs[0].shape[0]
            H, W = fcs[0].shape[1:3] if out_hw is None else out_hw
            m = ops.resize_bilinear(md, (H, W), align_corners=False)
            flow12, inb, flowUp = ops.compose_flow(fd8[0], fcs[0], clamp=True, want_inb=True, want_flow_up=True, out_hw=(H, W))
            # (match12 * cycle) * in-bounds, left to right like the reference expression (evalKITTI/evaluation.py:75-77), one kernel
            f12, match = [flow12], [ops.match_score(m[:B, 0], ops.grid_sample(m[B:], flowUp)[:, 0], inb).unsqueeze(1)]
        else:
            match12, inb = new(lay["total"]), new(lay["total"])

            def tail(m, d, fc, m_out, inb_out):                 # the resize reads match12Down8, compose_flow the /8 flow: independent
                ops.resize_bilinear(m, fc.shape[1:3], align_corners=False, out=m_out)
                return ops.compose_flow(d, fc, clamp=True, want_inb=True, inb_out=inb_out[:, 0])[0]
            f12 = self._stage(tail, [h[0] for h in halves], fd8, fcs, cut(match12), cut(inb))
            packed = torch.mul(match12, inb)                    # match12 * inb of all groups: one multiply over the packed buffers
            match = cut(packed)
            if out is not None:
                out.update(match=packed, flowDown8=f8, match12Down8=m12, match21Down8=m21, layout=lay)
        return [dict(flow12=f12[g], match=match[g], flowDown8=fd8[g], match12Down8=halves[g][0], match21Down8=halves[g][1])
                for g in range(G)]

    def _sampled_features(self, Is_list, fcs):
        """Per group: the sources sampled at the coarse grids -> normalised features."""
        return self.feat_l2norm(self._stage(ops.grid_sample, Is_list, fcs))

    def pred_flow_mask(self, IsTensor, featt, flowCoarse):
        """evaluation/evalHpatch/evaluation.py:23-55 (PredFlowMask) for a batch."""
        return self.pred_flow_mask_lists(self._sampled_features([IsTensor], [flowCoarse]), [featt], [flowCoarse])[0]

    def pred_flow_mask_groups(self, Is_list, featt_list, Hs_list, hw_list, out=None):
        """warp_grid + pred_flow_mask for G shape groups in one call: group g = sources Is_list[g] (B_g,3,.,.), normalised target
        features featt_list[g] (B_g,256,h/8,w/8), homographies Hs_list[g] (B_g,3,3), target size hw_list[g] = (h, w).  Returns one
        dict per group with pred_flow_mask's keys, each tensor bit-identical to pred_flow_mask on that group alone; the packed
        buffers and ``out``: pred_flow_mask_lists."""
        fcs = self._stage(lambda Hs, hw: ops.warp_grid(Hs, hw[0], hw[1]), Hs_list, hw_list)
        return self.pred_flow_mask_lists(self._sampled_features(Is_list, fcs), featt_list, fcs, out=out)

    def pred_flow_mask_kitti(self, IsSample, ItSample, flowCoarse, out_hw=None):
        """evaluation/evalKITTI/evaluation.py:49-81: both images go through the FeatureExtractor here (one batch), and the
        matchability is cycle-checked.  ``out_hw``: resolution of the identity grid the reference passes (``grid``): the coarse
        grid's own by default; the ORIGINAL image size in the full-resolution pass of the KITTI driver (:302), where flowCoarse has
        the fine size."""
        feats, featt = self._features_both([IsSample], [ItSample])
        return self.pred_flow_mask_lists(feats, featt, [flowCoarse], cycle=True, out_hw=out_hw)[0]

    def pred_flow_mask_kitti_groups(self, IsSample_list, ItSample_list, fcs, out_hw_list=None, out=None):
        """pred_flow_mask_kitti for G shape groups in one call: group g = sampled sources IsSample_list[g] and targets ItSample_list[g]
        (B_g,3,h,w), coarse grid fcs[g] (B_g,h,w,2), outputs at out_hw_list[g] (None: the grid's size).  Every step is one ops.stage
        over the groups and the tail is ops.cycle_tail.  Returns one dict per group with pred_flow_mask_kitti's keys, each tensor
        bit-identical to pred_flow_mask_kitti on that group alone; the packed buffers and ``out``: pred_flow_mask_lists."""
        feats, featt = self._features_both(IsSample_list, ItSample_list)
        return self._pred_flow_mask_cycle_lists(feats, featt, fcs, out_hw_list, out)

    # ---------------------------------------------------------------- multi-homography driver
    def multi_h(self, prep, b=0, maxCoarse=10, maskRegionTh=0.01, It_bg=None, feats=None, sample_fn=None):
        """The per-pair multi-homography loop of evaluation/evalHpatch/evaluation.py:184-243 (variant B: matches
        computed once, filtered by the explained-region mask) with every mask kept on the device: per accepted
        homography the host reads back two scalars (surviving-match count for the index draw, acceptance
        statistic) instead of round-tripping h x w masks through numpy as the reference does (:53,212,225,238).
        Returns dict(H=[(3,3)...], flowDown8=[...], matchDown8=[...], mask=final explained mask (h,w))."""
        feats = feats or self.features(prep)
        dev = self.dev
        h, w = prep["ItTensor"].shape[2], prep["ItTensor"].shape[3]
        IsT, ItT = prep["IsTensor"][b:b + 1], prep["ItTensor"][b:b + 1]
        i1, i2 = ops.mutual_nn(feats["featA"][b], feats["featB"][b], ldA=feats.get("ldA"), nA=feats["nA"], score_chunk=self.score_chunk)
        W1, H1 = feats["WA"][i1], feats["HA"][i1]
        W2, H2 = feats["Wt"][i2], feats["Ht"][i2]
        rt, ct = feats["rt"], feats["ct"]
        r2, c2 = i2 // ct, i2 % ct                       # integer cell coordinates (getWHTensor_Int)
        featt = ops.l2norm(self.feat(ItT))
        bg = torch.ones((h, w), dtype=torch.float32, device=dev) if It_bg is None else It_bg.to(dev).float()
        Mask = torch.zeros((h, w), dtype=torch.float32, device=dev)
        out = dict(H=[], flowDown8=[], matchDown8=[])
        draw = sample_fn or self._pair_draw
        nb = 0
        while nb <= maxCoarse:
            fg = ((Mask + (1 - bg)) > 0.5).float()
            keep = ops.resize_bilinear((1 - fg)[None, None], (rt, ct), align_corners=False)[0, 0] > 0.5
            valid = keep[r2, c2]
            n = int(valid.sum().item())                                       # sync: size of the index draw
            if n < 4:
                break
            ones = torch.ones(n, dtype=torch.float32, device=dev)
            m1 = torch.stack((H1[valid], W1[valid], ones), dim=1)
            m2 = torch.stack((H2[valid], W2[valid], ones), dim=1)
            bestH, inl, res = ops.ransac_h4(m1, m2, draw(n, self.nbIter).to(dev), self.tol,
                                            degenerate=self._degenerate_mode(sample_fn is not None or self.draw == "host"))
            flowCoarse = ops.warp_grid(bestH[None], h, w)
            pm = self.pred_flow_mask(IsT, featt, flowCoarse)
            stat = torch.stack(((pm["match"][0, 0] * (1 - fg)).mean(), res[0].float()))
            gain, status = stat.cpu().tolist()                                # sync: acceptance statistic + status
            if status != 0:
                break
            if gain > maskRegionTh or nb == 0:
                out["H"].append(bestH)
                out["flowDown8"].append(pm["flowDown8"])
                out["matchDown8"].append(torch.cat((pm["match12Down8"], pm["match21Down8"]), dim=1))
                nb += 1
                Mask = ((Mask + pm["match"][0, 0] * (1 - fg)) >= 1.0).float()
            else:
                break
        out["mask"] = Mask
        return out

    def _round_draws(self, active, n_dev, sample_fn, A=None, ids=None, epoch=0, rnd=0):
        """Index draws of one lock-step round -> (a,nbIter,4) int64 device tensor.  Device mode: Philox from the device-side
        counts keyed by (seed, epoch, round, pair id) -- the id of the k-th active pair is ids[active[k]] (the caller's absolute
        ids) or its position active[k] in the batch -- no sync.  Host mode / explicit sample_fn: one sync for the counts, CPU
        draws for the active pairs in ascending order, one upload."""
        if sample_fn is None and self.draw == "device":
            if ids is not None:
                key = ids if A is None else ids.index_select(0, A)
            else:
                key = A                                                   # None = the whole batch in order = positions 0..B-1
            return self._device_draw(n_dev, key, epoch, rnd)
        n_host = n_dev.cpu().tolist()                                                   # sync: sizes of the index draws
        draw = sample_fn or (lambda b, n, it: torch.randint(n, (it, 4)))
        return torch.stack([draw(b, n, self.nbIter) if n >= 4 else torch.zeros((self.nbIter, 4), dtype=torch.int64)
                            for b, n in zip(active, n_host)]).to(self.dev, non_blocking=True)

    def multi_h_batched(self, prep, maxCoarse=10, maskRegionTh=0.01, It_bg=None, feats=None, sample_fn=None, records=None,
                        want_lists=True, trace=None, pair_ids=None, draw_epoch=0, split=None):
        """multi_h() for every pair of the batch in lock-step: round k computes the k-th homography of all pairs that are
        still active.  A round is device work end to end -- rfx_filter_matches_f32 (mask -> keep map -> ordered compaction of
        the cached matches), the index draw (device mode), rfx_ransac_h4_batched, the warp, PredFlowMask over the active
        pairs, rfx_multih_accept_f32 (gain, accept rule, mask update, result-record store) -- and ONE host readback: the
        accept flags, from which the host builds the next round's active list (the exact mode, degenerate="lapack", has a second
        wait per round: the flagged 4-point samples, re-solved by the host's LAPACK).  Semantics per pair =
        evaluation/evalHpatch/evaluation.py:184-243.
        ``split``: the rounds of the batch as this many independent lock-step groups (contiguous slices of the batch), each on its
        own HIP stream, driven from this one host thread as coroutines (rounds.lockstep_rounds yields at its host waits;
        rounds.drive_rounds resumes the group whose event is due): while one group waits for the host -- accept flags, the LAPACK
        stage -- the other groups' kernels keep the GPU busy, and the small launches of one group's late rounds share the chip with
        another's.  Per pair the arithmetic is unchanged (every kernel computes a pair independently; device draws are keyed by
        absolute pair position / id).  None = RFX_MULTIH_SPLIT or, for device draws, 4 groups from 32 pairs on, 3 from 12, 2 from 8
        (rounds.HPATCH_SPLIT), else 1; forced to 1 with host draws / ``sample_fn`` (the CPU generator is consumed in pair order),
        with ``trace`` and under an ops.Profiler (per-launch events): rounds.split_policy.
        ``sample_fn(b, n, nbIter)`` -> (nbIter,4) int64 CPU tensor: explicit draws (parity mode; costs a second sync per round).
        ``pair_ids``: absolute ids of the batch's pairs for the device draw (see _draw_epoch): with them a pair's homographies
        are the same alone, in any batch and under any sharding.
        ``records``: an ops.MultiHRecords to fill (the fixed-size rows one all_gather moves); ``want_lists=False`` skips the
        per-pair Python lists (throughput drivers that only ship the records).  ``trace``: a list that receives one dict per
        round with the round's state (mask before the round, counts, H, PredFlowMask outputs, accept flags) -- the parity
        sweeps replay every round on the oracle from it.
        A ragged prep (prepare_ragged / prepare_ragged_device: pairs of different sizes) takes the same rounds with packed masks
        (_multi_h_batched_ragged): per pair the results are, bit for bit, the pair's alone; ``It_bg`` is then a list of per-pair
        (h_b, w_b) tensors (None entries = all ones) and ``records`` an ops.MultiHRecordsRagged.
        Returns a list of dicts like multi_h() (H / flowDown8 / matchDown8 lists are views of per-round tensors)."""
        if prep.get("ragged"):
            return self._multi_h_batched_ragged(prep, maxCoarse, maskRegionTh, It_bg, feats, sample_fn, records, want_lists, trace,
                                                pair_ids, draw_epoch, split)
        feats = feats or self.features(prep)
        dev = self.dev
        B = prep["B"]
        h, w = prep["ItTensor"].shape[2], prep["ItTensor"].shape[3]
        idx1, idx2, cnt = self._mutual_batched(feats, B)
        st = rounds.RoundState(self, [dict(H=[], flowDown8=[], matchDown8=[]) for _ in range(B)], "multi_h", rounds.HPATCH_SPLIT, split,
                               sample_fn, records, want_lists, trace, pair_ids, draw_epoch, maskRegionTh, maxCoarse)
        batch = dict(feats=feats, idx1=idx1, idx2=idx2, cnt=cnt, IsTensor=prep["IsTensor"], ItTensor=prep["ItTensor"],
                     bg=None if It_bg is None else It_bg.to(dev).float().contiguous(),
                     Mask=torch.zeros((B, h, w), dtype=torch.float32, device=dev), nbH=torch.zeros(B, dtype=torch.int32, device=dev))
        groups = [rounds.DenseGroup(st, batch, lo, hi) for lo, hi in st.bounds]
        if st.split == 1 and st.degenerate != "lapack":
            groups[0].target_features()       # one group and no host stage to put it behind: ahead of the rounds
        rounds.drive_rounds(self, [rounds.lockstep_rounds(g) for g in groups])
        return st.close(lambda b: batch["Mask"][b], (idx1, idx2, cnt))

    # ---------------------------------------------------------------- multi-homography rounds of a ragged batch
    def _multi_h_batched_ragged(self, prep, maxCoarse, maskRegionTh, It_bg, feats, sample_fn, records, want_lists, trace, pair_ids,
                                draw_epoch, split):
        """multi_h_batched for a ragged prep.  One grouped trunk pass (_features_ragged), one ragged mutual matching, then the
        lock-step rounds of rounds.RaggedGroup under the dense driver's coroutine / stream machinery (rounds.drive_rounds, ``split``).
        The explained-region masks (and background maps) of all pairs live in ONE packed buffer (ragged_multih_tables, ragged.PackedBatch:
        offsets and geometry uploaded once), so a round is one filter launch, one draw, one RANSAC search and one accept launch for all active
        pairs of a group whatever their sizes, and one host readback.  Only the fine stage of a round (warp_grid, PredFlowMask)
        runs per group of active pairs that share (source shape, target shape), on the dense kernels."""
        feats = feats or self.features(prep)
        B, tabs = prep["B"], ragged_multih_tables(prep["plan"])
        idx1, idx2, cnt = self._mutual_ragged(feats)
        st = rounds.RoundState(self, [dict(H=[], flowDown8=[], matchDown8=[]) for _ in range(B)], "multi_h", rounds.HPATCH_SPLIT, split,
                               sample_fn, records, want_lists, trace, pair_ids, draw_epoch, maskRegionTh, maxCoarse)
        if records is not None:
            ops.MultiHRecordsRagged.require(records, [g[4:6] for g in tabs["geom"]])
        pb = ragged.PackedBatch(tabs, It_bg, self.dev)
        batch = dict(pb.fields(), prep=prep, feats=feats, idx1=idx1, idx2=idx2, cnt=cnt)
        rounds.drive_rounds(self, [rounds.lockstep_rounds(rounds.RaggedGroup(st, batch, lo, hi)) for lo, hi in st.bounds])
        return st.close(pb.mask_of, (idx1, idx2, cnt))

    # ---------------------------------------------------------------- YFCC / Corr driver shape (variant C)
    def pred_flow_mask_cycle(self, IsTensor, featt, flowCoarse):
        """PredFlowMask of evaluation/evalYFCC/evaluation.py:32-58 (= evalCorr/evaluation.py:29-56) for a batch: the Hpatch form
        (pred_flow_mask) with the CYCLE-CHECKED matchability, all at the target's resolution, target features handed in."""
        return self.pred_flow_mask_lists(self._sampled_features([IsTensor], [flowCoarse]), [featt], [flowCoarse], cycle=True)[0]

    def pred_flow_mask_cycle_groups(self, Is_list, featt_list, Hs_list, hw_list, out=None):
        """warp_grid + pred_flow_mask_cycle for G shape groups in one call (arguments as pred_flow_mask_groups): every step one ops.stage
        over the groups, the tail ops.cycle_tail.  Returns one dict per group with pred_flow_mask_cycle's keys, each tensor
        bit-identical to pred_flow_mask_cycle on that group alone; the packed buffers and ``out``: pred_flow_mask_lists."""
        fcs = self._stage(lambda Hs, hw: ops.warp_grid(Hs, hw[0], hw[1]), Hs_list, hw_list)
        return self._pred_flow_mask_cycle_lists(self._sampled_features(Is_list, fcs), featt_list, fcs, out=out)

    def multi_h_variant_c(self, src_u8, tgt_candidates_u8, maxCoarse=10, maskRegionTh=0.01, It_bg=None, sample_fn=None, records=None,
                          want_lists=True, pair_ids=None, draw_epoch=0, split=None, want_records=False):
        """The driver of evaluation/evalYFCC/evaluation.py:176-292 for a batch of B pairs in lock-step, everything on the device.

        ``src_u8`` (B,H,W,3) uint8: the sources; ``tgt_candidates_u8``: K tensors (B,Hk,Wk,3) -- candidate k of every pair (the
        script's four rotations of the target, :189; K = 1 = evalCorr-like use without a search).
        1. *candidate search* (:191-208): source pyramid features once; per candidate: target features, the variant-C getCoarse --
           keep map of the candidate's background (ops.keep_mask) -> mutual matching against the MASKED target features (the 0/1
           column mask of rfx_mutual_nn_batched_f32) -> RANSAC -- and nbInlier = the winner's inlier count (0 for the (None, [])
           sentinel: np.sum(InlierMask) counts distinct target cells, and mutual matches have distinct target cells); the chosen
           candidate is the FIRST maximum (np.argmax, :210).  One host sync: the (B,K) count table, from which the pairs are
           grouped by the shape of their chosen candidate.
        2. *multi-homography loop* (:238-275) per shape group: every round RE-MATCHES -- keep map of the explained-region mask ->
           masked mutual matching -> RANSAC -> warp -> pred_flow_mask_cycle -> accept rule / mask update / record store
           (rfx_multih_accept_f32 mode 0: the same rule as the Hpatch loop) -- with ONE host readback per round (accept flags).
        ``It_bg``: K tensors (B,Hk,Wk) (1 = foreground to explain, as the script's It_bg after :212) at the candidates' RESIZED
        target size, or None (all ones).  ``sample_fn(b, n, nbIter)``: explicit draws (parity mode), called per pair in ascending
        order, first for the candidates k = 0..K-1 with >= 4 matches, then per round.  Device draws are keyed by (seed, pair id,
        candidate / round) with their own driver tags.
        Lists of images -- ``src_u8``: B uint8 (H,W,3) device tensors, ``tgt_candidates_u8``: K lists of B uint8 (Hk_b,Wk_b,3) tensors
        (YFCC100M images come in arbitrary sizes, and the rotations swap height and width): all sources of one shape and, per
        candidate, all targets of one shape are stacked and take the dense path unchanged; otherwise the ragged path
        (_multi_h_variant_c_ragged) -- per pair the results are, bit for bit, the pair's alone.  ``It_bg`` is then K lists (or None)
        of B per-pair (h,w) tensors at the candidates' resized sizes (None entries = all ones); ``split``: lock-step groups of the
        rounds as in multi_h_batched (default 1; the dense path runs its shape groups one after the other).  The geometry of a
        ragged batch's records depends on the chosen candidates, known only after the search, so the ragged path takes no
        ``records=``; it BUILDS them: ``want_records=True`` (list inputs only; such a call always takes the ragged path, also when all
        sizes agree -- per pair it is bit-identical) makes an ops.MultiHRecordsRagged over the chosen candidates' /8 sizes with
        max_h = maxCoarse + 1 after the search, has the rounds' accept kernel fill it, hangs the search's decisions on it (candidate,
        candidate_dev, size_src, size_tgt, bg: see the class) and returns (outs, records); ``want_lists=False`` is allowed with it.
        Returns a list of B dicts: H / flowDown8 / matchDown8 lists, mask, nbH, candidate (the chosen k), nbInlier (K counts)."""
        lists = isinstance(src_u8, (list, tuple)) or any(isinstance(c, (list, tuple)) for c in tgt_candidates_u8)
        if want_records and not lists:
            raise ValueError("multi_h_variant_c: want_records=True builds the records of a LIST of pairs; a batch of stacked tensors "
                             "fills the ops.MultiHRecords handed in as records=")
        if lists:
            src_l, cands, It_bg, mixed = self._variant_c_lists(src_u8, tgt_candidates_u8, It_bg, records, want_lists, want_records)
            if mixed:
                return self._multi_h_variant_c_ragged(src_l, cands, maxCoarse, maskRegionTh, It_bg, sample_fn, pair_ids, draw_epoch, split,
                                                      want_lists, want_records)
            src_u8, tgt_candidates_u8 = src_l, cands
        dev = self.dev
        B, K = src_u8.shape[0], len(tgt_candidates_u8)
        prep = self.prepare_device(src_u8, tgt_candidates_u8[0])
        feats = self.features(prep)
        featA, nA, ldA = feats["featA"], feats["nA"], feats.get("ldA", feats["nA"])
        cand = []                                                         # per candidate: ItTensor, featB, rt, ct, Wt, Ht
        for k, t8 in enumerate(tgt_candidates_u8):
            if k == 0:
                ItT, fB, rt, ct, Wt, Ht = prep["ItTensor"], feats["featB"], feats["rt"], feats["ct"], feats["Wt"], feats["Ht"]
            else:
                ItT, tn = self.prepare_target_device(t8)
                ft = ops.l2norm(self.trunk(tn))
                rt, ct = ft.shape[2], ft.shape[3]
                Wt, Ht = cell_coords_cached(rt, ct, dev)
                fB = ft.view(B, 1024, rt * ct)
            cand.append(dict(ItT=ItT, featB=fB, rt=rt, ct=ct, Wt=Wt, Ht=Ht,
                             bg=None if It_bg is None or It_bg[k] is None else It_bg[k].to(dev).float().contiguous()))

        def matches(c, fA, fB, maskB, n_pairs):
            """The matching half of variant C's getCoarse for a batch: masked mutual matching -> matches."""
            f = dict(featA=fA, featB=fB, nA=nA, ldA=ldA, nB=c["rt"] * c["ct"])
            idx1, idx2, cnt = self._mutual_batched(f, n_pairs, maskB)
            M1, M2 = ops.gather_matches(idx1, idx2, cnt, feats["HA"], feats["WA"], c["Ht"], c["Wt"])
            return M1, M2, cnt

        def matches_of(k):
            c = cand[k]
            keep = None if c["bg"] is None else ops.keep_mask(None, c["bg"], None, c["rt"], c["ct"])
            return matches(c, featA, c["featB"], keep, B)
        chosen, _, outs = self._variant_c_select(K, B, matches_of, sample_fn, pair_ids, draw_epoch)
        if records is not None:
            records.rec[:, 3] = torch.tensor(chosen, dtype=torch.float32).to(dev)
        groups = ragged.by_shape([tuple(cand[c]["ItT"].shape[2:]) for c in chosen])
        # the shape groups one after the other, each as ONE lock-step group of its own (no split, no trace)
        st = rounds.RoundState(self, outs, "variant_c", (), 1, sample_fn, records, want_lists, None, pair_ids, draw_epoch, maskRegionTh,
                               maxCoarse)
        masks = {}

        def shape_groups():
            for (h, w), members in groups.items():
                # the group's tensors: pair m of the group = pair members[m] of the batch with ITS chosen candidate
                G = len(members)
                gi = torch.tensor(members, dtype=torch.int64, device=dev)
                ref_c = cand[chosen[members[0]]]
                pick = lambda key: torch.stack([cand[chosen[b]][key][b] for b in members])
                bg = None if all(cand[chosen[b]]["bg"] is None for b in members) else torch.stack(
                    [cand[chosen[b]]["bg"][b] if cand[chosen[b]]["bg"] is not None else torch.ones((h, w), device=dev) for b in members])
                batch = dict(ItTensor=pick("ItT"), featB=pick("featB"), bg=bg, featA=featA.index_select(0, gi),
                             IsTensor=prep["IsTensor"].index_select(0, gi), rt=ref_c["rt"], ct=ref_c["ct"], gi=gi,
                             Mask=torch.zeros((G, h, w), dtype=torch.float32, device=dev), nbH=torch.zeros(G, dtype=torch.int32, device=dev))
                g = rounds.VariantCGroup(st, batch, members, functools.partial(matches, ref_c))
                for m, b in enumerate(members):
                    masks[b] = g.Mask[m]
                yield from rounds.lockstep_rounds(g)
                g.store_records()

        rounds.drive_rounds(self, [shape_groups()])
        return st.close(lambda b: masks[b])

    def _variant_c_select(self, K, B, matches_of, sample_fn, pair_ids, draw_epoch):
        """The candidate search of the YFCC driver (evaluation/evalYFCC/evaluation.py:191-210) for B pairs and K candidates:
        ``matches_of(k)`` -> (M1, M2, n_k), the matches of every pair with its candidate k; per candidate the draws (tag
        variant_c_select, round k), the RANSAC search and nbInlier = the winner's inlier count (0 unless the status is 0 and n >= 4);
        ONE host sync, the (B,K) count table; the chosen candidate is the first maximum.  Returns (chosen, table, outs): outs[b] = the
        pair's result dict with ``candidate`` and ``nbInlier`` filled in."""
        degen = self._degenerate_mode(sample_fn is not None or self.draw == "host")
        ids, ep_sel = self._draw_epoch(pair_ids, "variant_c_select", draw_epoch)
        all_b = list(range(B))
        counts = []
        for k in range(K):
            M1, M2, n_k = matches_of(k)
            smp = self._round_draws(all_b, n_k, sample_fn, None, ids, ep_sel, k)
            _, _, res = ops.ransac_h4_batched(M1, M2, n_k, smp, self.tol, degenerate=degen)
            counts.append(torch.where((res[:, 0] == 0) & (n_k >= 4), res[:, 1], torch.zeros_like(res[:, 1])))
        table = torch.stack(counts, dim=1).cpu()                          # the ONE sync of the search: (B,K) inlier counts
        chosen = ragged.choose_candidates(table)
        outs = [dict(H=[], flowDown8=[], matchDown8=[], nbH=0, candidate=chosen[b], nbInlier=table[b].tolist()) for b in range(B)]
        return chosen, table, outs

    # ---------------------------------------------------------------- the YFCC driver on pairs of different sizes
    def _variant_c_lists(self, src, cands, It_bg, records, want_lists, want_records=False):
        """The list inputs of multi_h_variant_c, checked -> (src, cands, It_bg, mixed).  Same shapes throughout (``mixed`` False):
        everything stacked into the dense driver's tensors.  Otherwise -- and always with ``want_records`` -- per-pair lists, It_bg
        as K lists of B entries or None."""
        dev = self.dev
        src_l = list(src)
        cands = [list(c) for c in cands]
        B, K = len(src_l), len(cands)
        if B == 0 or K == 0:
            raise ValueError("one source per pair and at least one list of candidate targets")
        if any(len(c) != B for c in cands):
            raise ValueError("every pair needs the same number K of candidates: K lists of B = %d targets each, got lengths %s"
                             % (B, [len(c) for c in cands]))
        imgs = src_l + [x for c in cands for x in c]
        if any(not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2] != 3 for x in imgs):
            raise ValueError("sources and candidate targets are uint8 (H,W,3) tensors, one per pair")
        mixed = want_records or ragged.mixed(*([tuple(x.shape) for x in lst] for lst in [src_l] + cands))
        if It_bg is not None:
            if len(It_bg) != K or any(g is not None and len(g) != B for g in It_bg):
                raise ValueError("It_bg: one entry per candidate (K = %d), each None or B = %d per-pair maps" % (K, B))
            mode = "max" if self.variant == "A" else "min"
            for k, g in enumerate(It_bg):
                for b, x in enumerate(g if g is not None else ()):
                    nw, nh = resize_dims(cands[k][b].shape[1], cands[k][b].shape[0], self.minSize, mode)
                    if x is not None and tuple(x.shape) != (nh, nw):
                        raise ValueError("It_bg[%d][%d] of shape %s for a candidate resized to %s" % (k, b, tuple(x.shape), (nh, nw)))
        if mixed and records is not None:
            raise ValueError("multi_h_variant_c on pairs of different sizes fills no records= handed in: their geometry depends on the "
                             "chosen candidate, which is known only after the search (want_records=True builds and returns them)")
        if mixed and not want_lists and not want_records:
            raise ValueError("multi_h_variant_c on pairs of different sizes without want_records=True has no records to fill, so "
                             "want_lists=False would return nothing")
        if any(not x.is_cuda or x.device != imgs[0].device for x in imgs):
            raise ValueError("sources and candidate targets must live on one HIP device (no CPU fallback)")
        if mixed:
            return src_l, cands, It_bg, True
        if It_bg is not None:                                # per-pair maps -> the dense driver's (B,h,w) tensor per candidate
            dense_bg = []
            for g in It_bg:
                if g is None or isinstance(g, torch.Tensor) or all(x is None for x in g):
                    dense_bg.append(g if isinstance(g, torch.Tensor) else None)
                    continue
                hw = next(tuple(x.shape) for x in g if x is not None)
                dense_bg.append(torch.stack([torch.ones(hw, device=dev) if x is None else x.to(dev).float() for x in g]))
            It_bg = dense_bg
        return torch.stack(src_l), [torch.stack(c) for c in cands], It_bg, False

    def _multi_h_variant_c_ragged(self, src_l, cands, maxCoarse, maskRegionTh, It_bg, sample_fn, pair_ids, draw_epoch, split,
                                  want_lists=True, want_records=False):
        """multi_h_variant_c for pairs of different sizes (src_l[b], cands[k][b]: uint8 (H,W,3) device tensors).
        *Search*: the source pyramids and all B * K candidate targets through ONE grouped trunk pass (_features_ragged); per
        candidate index k, for all pairs at once: keep map of the candidate's background (rfx_keep_mask_ragged_f32, mask null) ->
        masked ragged mutual matching -> match gather -> draws (tag variant_c_select, round k) -> RANSAC search; ONE host sync, the
        (B,K) inlier-count table.  *Rounds*: rounds.RaggedVariantCGroup on the CHOSEN candidates' features and packed masks
        (ragged_variant_c_tables) under the lock-step machinery of the other ragged drivers.  ``want_records``: an
        ops.MultiHRecordsRagged over the chosen candidates' /8 sizes, filled by the rounds' accept kernel; -> (outs, records)."""
        dev, B, K = self.dev, len(src_l), len(cands)
        prep = self.prepare_candidates_device(src_l, cands)
        plan, feats = prep["plan"], self.features(prep)
        ldB, maxNA = plan["ldB"], max(plan["nA"])

        def matches_of(k):
            keep, max_nB = None, max(plan["nB"][k])
            if It_bg is not None and It_bg[k] is not None and any(x is not None for x in It_bg[k]):
                pb = ragged.PackedBatch(ragged_variant_c_tables(plan, [k] * B), It_bg[k], dev, masks=False)
                keep = ops.keep_mask_ragged(None, pb.bg, pb.moff, pb.geom, None, ldB, max_nB)
            idx1, idx2, n_k = ops.mutual_nn_ragged(feats["featA"], feats["featB"][k], feats["nA_dev"], feats["nB_dev"][k], maxNA, max_nB,
                                                   maskB=keep, score_chunk=self.score_chunk, cap=plan["cap"])
            M1, M2 = ops.gather_matches_ragged(idx1, idx2, n_k, feats["HA"], feats["WA"], feats["offA"], feats["Ht"], feats["Wt"],
                                               feats["offB"][k])
            return M1, M2, n_k
        chosen, _, outs = self._variant_c_select(K, B, matches_of, sample_fn, pair_ids, draw_epoch)
        # the rounds: the chosen candidates' features, sizes and tables as ONE ragged batch
        tabs = ragged_variant_c_tables(plan, chosen)
        pb = ragged.PackedBatch(tabs, None if It_bg is None else [None if It_bg[c] is None else It_bg[c][b] for b, c in enumerate(chosen)], dev)
        records = None
        if want_records:
            sizes8 = [tuple(g[4:6]) for g in tabs["geom"]]
            records = ops.MultiHRecordsRagged([s[0] for s in sizes8], [s[1] for s in sizes8], dev, max_h=maxCoarse + 1)
            ops.MultiHRecordsRagged.require(records, sizes8)
            records.candidate = list(chosen)
            records.candidate_dev = torch.tensor(chosen, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            records.size_src = [(int(x.shape[3]), int(x.shape[2])) for x in prep["IsTensor"]]
            records.size_tgt = [(g[1], g[0]) for g in tabs["geom"]]           # (h, w) = (8 h8, 8 w8): a packed mask IS a packed map
            records.bg = None if pb.bg is None else (pb.bg != 0).to(torch.uint8)
        pick = torch.tensor([c * B + b for b, c in enumerate(chosen)], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        rf = dict(feats, featB=feats["featB"].view(K * B, 1024, ldB).index_select(0, pick), nB=[plan["nB"][c][b] for b, c in enumerate(chosen)],
                  nB_dev=feats["nB_dev"].reshape(-1).index_select(0, pick), offB=feats["offB"].reshape(-1).index_select(0, pick))
        st = rounds.RoundState(self, outs, "variant_c", (), split, sample_fn, records, want_lists, None, pair_ids, draw_epoch, maskRegionTh,
                               maxCoarse)
        batch = dict(pb.fields(), prep=dict(IsTensor=prep["IsTensor"], ItTensor=[prep["ItTensor"][c][b] for b, c in enumerate(chosen)]),
                     feats=rf, idx1=None, idx2=None, cnt=None)
        rounds.drive_rounds(self, [rounds.lockstep_rounds(rounds.RaggedVariantCGroup(st, batch, lo, hi)) for lo, hi in st.bounds])
        outs = st.close(pb.mask_of)
        return (outs, records) if want_records else outs

    def multi_h_variant_c_pairs(self, pairs, angles=(0, 90, 180, 270), maxCoarse=10, maskRegionTh=0.01, It_bg=None, sample_fn=None,
                                records=None, want_lists=True, pair_ids=None, draw_epoch=0, split=None, seg=None, want_records=False):
        """multi_h_variant_c on pairs of PIL images, the candidates being the target turned by ``angles`` (multiples of 90 degrees,
        counter-clockwise: evaluation/evalYFCC/evaluation.py:189).  Every image is uploaded once; a candidate is torch.rot90 of the
        uploaded target, byte-identical to PIL's rotate(angle, expand=True) for right angles.  All sources of one size and all targets
        of one size: the dense path on stacked tensors (``It_bg``: K tensors (B,h,w), ``records`` an ops.MultiHRecords).  Otherwise the
        ragged path on lists (``It_bg``: K lists of per-pair maps; no ``records=``).  ``seg`` instead of ``It_bg``: one sky mask per
        target (get_sky_batch), and candidate k gets it turned like the candidate, at that candidate's resized size
        (evaluation/evalYFCC/evaluation.py:193-200).  ``want_records=True``: always the ragged path on lists, -> (outs, records) as
        multi_h_variant_c builds them, with ``records.angle`` = angles[candidate] per pair (the script's rotation.json)."""
        if any(int(a) % 90 for a in angles):
            raise ValueError("candidate angles are multiples of 90 degrees, got %s" % (tuple(angles),))
        use_seg = self._seg_or_bg(seg, It_bg)
        src, tgt = self._upload_lists(pairs)
        cands = [[torch.rot90(t, int(a) // 90 % 4, (0, 1)).contiguous() for t in tgt] for a in angles]
        if use_seg:
            masks = seg.get_sky_batch(tgt)
            It_bg = [self._backgrounds_of_masks(masks, [self._target_resized_hw(int(x.shape[0]), int(x.shape[1])) for x in c],
                                                [int(a) // 90] * len(tgt)) for a, c in zip(angles, cands)]
        if not self._mixed_sizes(pairs) and not want_records:
            src, cands = torch.stack(src), [torch.stack(c) for c in cands]
            if use_seg:
                It_bg = [torch.stack(g) for g in It_bg]
        res = self.multi_h_variant_c(src, cands, maxCoarse=maxCoarse, maskRegionTh=maskRegionTh, It_bg=It_bg, sample_fn=sample_fn,
                                     records=records, want_lists=want_lists, pair_ids=pair_ids, draw_epoch=draw_epoch, split=split,
                                     want_records=want_records)
        if want_records:
            res[1].angle = [int(angles[c]) for c in res[1].candidate]
        return res

    # ---------------------------------------------------------------- KITTI two-resolution driver (BASELINE config 5)
    resize_img_dims = staticmethod(resize_img_dims)     # outil.resizeImg's sizes (module level: ragged_kitti_tables uses it too)

    def multi_h_kitti(self, src_u8, tgt_u8, fineSize=650, maskRegionTh=0.005, cc_th=0.01, It_bg=None, feats=None, prep=None,
                      sample_fn=None, remove_small_cc=None):
        """The per-pair driver of evaluation/evalKITTI/evaluation.py:222-336 for ONE pair of raw uint8 (1,H,W,3) device
        images (self must be a variant-B pipeline built with the KITTI coarse parameters: minSize = coarseSize 800,
        nbScale 3, scaleR 1.2, nbIter 50 000).  Per homography: getCoarse on the cached matches filtered by the
        explained-region mask (:273) -> homography grids at the half and the full fine resolution (:281-282) -> source
        (ORIGINAL resolution) warped to the half resolution (:284) -> PredFlowMask there (:290) -> its /8 flow composed
        with the full-resolution homography grid (:294-297) -> source warped by it (:299) -> PredFlowMask whose outputs live
        at the ORIGINAL target resolution (:302) -> small-component filter on the host, like the reference's skimage call
        (:321; on the device, ops.remove_small_cc; ``remove_small_cc(match ndarray, 0.99, cc_th)`` injects a host filter) -> accept iff
        ((match > 0.9999) outside the mask).mean() > maskRegionTh or first homography (:322) -> mask update (:333).
        The loop is the reference's ``while True``: it ends on the accept test or when fewer than 4 matches survive.
        LANCZOS resizes (outil.resizeImg) run on the device, byte-exact vs Pillow.  Host syncs per homography: match count,
        RANSAC status + accept statistic.
        Returns dict(H=[...], flowD2=[...], flowDown8=[...], matchDown8=[...], mask)."""
        dev = self.dev
        if prep is None:
            prep = self.prepare_device(src_u8, tgt_u8)
        feats = feats or self.features(prep)
        h_org, w_org = tgt_u8.shape[1], tgt_u8.shape[2]
        w_r, h_r = self.resize_img_dims(w_org, h_org, 8, fineSize)
        w_d2, h_d2 = self.resize_img_dims(w_org, h_org, 8, fineSize // 2)
        tensor_s, _ = ops.u8_to_f32(src_u8)                                              # source at its ORIGINAL size
        tensor_resize, _ = ops.u8_to_f32(ops.lanczos_resize_u8(tgt_u8, w_r, h_r))
        tensor_d2, _ = ops.u8_to_f32(ops.lanczos_resize_u8(tgt_u8, w_d2, h_d2))
        i1, i2 = ops.mutual_nn(feats["featA"][0], feats["featB"][0], ldA=feats.get("ldA"), nA=feats["nA"], score_chunk=self.score_chunk)
        W1, H1 = feats["WA"][i1], feats["HA"][i1]
        W2, H2 = feats["Wt"][i2], feats["Ht"][i2]
        rt, ct = feats["rt"], feats["ct"]
        r2, c2 = i2 // ct, i2 % ct
        bg = torch.ones((h_org, w_org), dtype=torch.float32, device=dev) if It_bg is None else It_bg.to(dev).float()
        Mask = torch.zeros((h_org, w_org), dtype=torch.float32, device=dev)
        out = dict(H=[], flowD2=[], flowDown8=[], matchDown8=[])
        draw = sample_fn or self._pair_draw
        nb = 0
        while True:
            fg = ((Mask + (1 - bg)) > 0.5).float()
            keep = ops.resize_bilinear((1 - fg)[None, None], (rt, ct), align_corners=False)[0, 0] > 0.5
            valid = keep[r2, c2]
            n = int(valid.sum().item())                                       # sync: size of the index draw
            if n < 4:
                break
            ones = torch.ones(n, dtype=torch.float32, device=dev)
            m1 = torch.stack((H1[valid], W1[valid], ones), dim=1)
            m2 = torch.stack((H2[valid], W2[valid], ones), dim=1)
            bestH, _, res = ops.ransac_h4(m1, m2, draw(n, self.nbIter).to(dev), self.tol,
                                          degenerate=self._degenerate_mode(sample_fn is not None or self.draw == "host"))
            flow_d2, pm, match = self.kitti_fine_round(bestH[None], tensor_s, tensor_d2, tensor_resize, (h_org, w_org), cc_th,
                                                       remove_small_cc)
            match = match[0]
            stat = torch.stack((((match > 0.9999).float() * (1 - fg)).mean(), res[0].float()))
            gain, status = stat.cpu().tolist()                                # sync: acceptance statistic + status
            if status != 0:
                break
            if gain > maskRegionTh or nb == 0:
                out["H"].append(bestH)
                out["flowD2"].append(flow_d2)
                out["flowDown8"].append(pm["flowDown8"])
                out["matchDown8"].append(torch.cat((pm["match12Down8"], pm["match21Down8"]), dim=1))
                nb += 1
                Mask = ((Mask + match * (1 - fg)) > 0.9999).float()
            else:
                break
        out["mask"] = Mask
        return out

    def kitti_fine_round(self, Hs, tensor_s, tensor_d2, tensor_resize, org_hw, cc_th=0.01, remove_small_cc=None):
        """The fine part of one round of the KITTI driver (evaluation/evalKITTI/evaluation.py:279-321) for a batch of
        homographies Hs (a,3,3): homography grids at the half and the full fine resolution -> source warped to the half
        resolution -> PredFlowMask there -> its /8 flow composed with the full-resolution homography grid -> source warped by
        it -> PredFlowMask whose outputs live at the ORIGINAL target resolution ``org_hw`` -> small-component filter
        (device: rfx_remove_small_cc_f32; or an injected host filter ``remove_small_cc(match ndarray, 0.99, cc_th)``).
        Returns (flow_d2 (a,2,hd2,wd2), PredFlowMask dict of the full-resolution pass, match (a,h_org,w_org) after the filter)."""
        h_d2, w_d2 = tensor_d2.shape[2], tensor_d2.shape[3]
        h_r, w_r = tensor_resize.shape[2], tensor_resize.shape[3]
        hom_d2 = ops.warp_grid(Hs, h_d2, w_d2)
        hom_resize = ops.warp_grid(Hs, h_r, w_r)
        Is_d2 = ops.grid_sample(tensor_s, hom_d2)
        flow_d2 = self.pred_flow_mask_kitti(Is_d2, tensor_d2, hom_d2)["flowDown8"]
        flowCoarse, _, _ = ops.compose_flow(flow_d2, hom_resize, clamp=True)
        IsSample = ops.grid_sample(tensor_s, flowCoarse)
        pm = self.pred_flow_mask_kitti(IsSample, tensor_resize, flowCoarse, out_hw=org_hw)
        match = pm["match"][:, 0]
        if cc_th > 0:                                                                   # :321
            if remove_small_cc is None:
                match = ops.remove_small_cc(match, cc_th, 0.99)
            else:                                                                       # an injected host filter: one round trip
                mh = match.cpu().numpy()
                match = torch.from_numpy(np.stack([remove_small_cc(mh[k], 0.99, cc_th) for k in range(mh.shape[0])])).to(self.dev)
        return flow_d2, pm, match

    def kitti_fine_round_groups(self, Hs_list, tensor_s_list, tensor_d2_list, tensor_resize_list, org_hw_list, out=None):
        """kitti_fine_round(..., cc_th=0) for G shape groups in one call: group g = homographies Hs_list[g] (a_g,3,3), sources
        tensor_s_list[g], targets at the half and the full fine resolution tensor_d2_list[g] / tensor_resize_list[g], original target
        size org_hw_list[g].  Every step is one ops.stage over the groups: both warp_grids, the half-resolution warp, the KITTI form
        there, compose_flow of its /8 flow with the full-resolution grid, the full-resolution warp, the KITTI form at the original
        size.  Returns one (flow_d2, PredFlowMask dict of the full-resolution pass, match (a_g,h_org,w_org) -- unfiltered) per group,
        bit-identical to kitti_fine_round on that group alone; ``out`` receives the packed buffers of the full-resolution pass
        (pred_flow_mask_lists) and ``flowD2``, the half-resolution /8 flows packed in group order."""
        st = self._stage
        hom_d2 = st(lambda Hs, t: ops.warp_grid(Hs, t.shape[2], t.shape[3]), Hs_list, tensor_d2_list)
        hom_resize = st(lambda Hs, t: ops.warp_grid(Hs, t.shape[2], t.shape[3]), Hs_list, tensor_resize_list)
        Is_d2 = st(ops.grid_sample, tensor_s_list, hom_d2)
        half = {}
        flow_d2 = [pm["flowDown8"] for pm in self.pred_flow_mask_kitti_groups(Is_d2, tensor_d2_list, hom_d2, out=half)]
        flowCoarse = st(lambda d, fc: ops.compose_flow(d, fc, clamp=True)[0], flow_d2, hom_resize)
        IsSample = st(ops.grid_sample, tensor_s_list, flowCoarse)
        pms = self.pred_flow_mask_kitti_groups(IsSample, tensor_resize_list, flowCoarse, out_hw_list=org_hw_list, out=out)
        if out is not None:
            out["flowD2"] = half["flowDown8"]
        return [(d2, pm, pm["match"][:, 0]) for d2, pm in zip(flow_d2, pms)]

    def multi_h_kitti_batched(self, src_u8, tgt_u8, fineSize=650, maskRegionTh=0.005, cc_th=0.01, It_bg=None, sample_fn=None,
                              remove_small_cc=None, records=None, want_lists=True, trace=None, pair_ids=None, draw_epoch=0, split=None):
        """multi_h_kitti() for B pairs in lock-step (src_u8 / tgt_u8: (B,H,W,3) uint8 on the device, or -- pairs of DIFFERENT sizes
        -- per side a list of (H,W,3) / (1,H,W,3) uint8 device tensors, see below): round k
        computes the k-th homography of every pair that is still active -- one batched launch chain for the trunk features,
        the match filtering (rfx_filter_matches_f32), the index draw (device mode), RANSAC (rfx_ransac_h4_batched), the two
        warps and both PredFlowMask passes over the active pairs, the small-component filter on the device and the accept
        rule / mask update / record store (rfx_multih_accept_f32, mode 1), with ONE host readback per round (the accept
        flags).  Per pair the arithmetic and the accept / stop rule are multi_h_kitti()'s
        (evaluation/evalKITTI/evaluation.py:257-336); batch-1 fine passes become batch-a ones, which is where the time goes
        (the 3x3 kernels run at 0.59 of the matrix peak at batch 1, 0.8 at batch 8).
        ``sample_fn(b, n, nbIter)`` -> (nbIter,4) int64 CPU tensor: explicit draws (parity mode; a second sync per round).
        ``records``: ops.MultiHRecords built with the half-resolution /8 size (hd2, wd2); ``trace``: as in multi_h_batched.
        Lists of images: all sources of one shape and all targets of one shape are stacked and take the dense path unchanged;
        otherwise the ragged path (_multi_h_kitti_batched_ragged: real KITTI lists mix 1242x375, 1241x376, 1238x374, 1226x370 and
        1224x370 frames) -- per pair the results are, bit for bit, the pair's alone; ``It_bg`` is then a list with one (h_org, w_org)
        tensor or None per pair and ``records`` an ops.MultiHRecordsRagged built with the d2 lists.
        Returns a list of dicts like multi_h_kitti()."""
        dev = self.dev
        if isinstance(src_u8, (list, tuple)) or isinstance(tgt_u8, (list, tuple)):
            one = lambda x: x[0] if x.dim() == 4 else x
            src_l, tgt_l = [one(x) for x in src_u8], [one(x) for x in tgt_u8]
            if len(src_l) != len(tgt_l) or not src_l:
                raise ValueError("one source and one target per pair")
            if ragged.mixed([tuple(x.shape) for x in src_l], [tuple(x.shape) for x in tgt_l]):
                return self._multi_h_kitti_batched_ragged(src_l, tgt_l, fineSize, maskRegionTh, cc_th, It_bg, sample_fn, remove_small_cc,
                                                          records, want_lists, trace, pair_ids, draw_epoch, split)
            src_u8, tgt_u8 = torch.stack(src_l), torch.stack(tgt_l)
            if isinstance(It_bg, (list, tuple)):
                It_bg = None if all(x is None for x in It_bg) else torch.stack(
                    [torch.ones(tgt_u8.shape[1:3], device=dev) if x is None else x.to(dev).float() for x in It_bg])
        B, h_org, w_org = tgt_u8.shape[0], tgt_u8.shape[1], tgt_u8.shape[2]
        prep = self.prepare_device(src_u8, tgt_u8)
        feats = self.features(prep)
        w_r, h_r = self.resize_img_dims(w_org, h_org, 8, fineSize)
        w_d2, h_d2 = self.resize_img_dims(w_org, h_org, 8, fineSize // 2)
        tensor_s, _ = ops.u8_to_f32(src_u8)                                              # sources at their ORIGINAL size
        tensor_resize, _ = ops.u8_to_f32(ops.lanczos_resize_u8(tgt_u8, w_r, h_r))
        tensor_d2, _ = ops.u8_to_f32(ops.lanczos_resize_u8(tgt_u8, w_d2, h_d2))
        idx1, idx2, cnt = self._mutual_batched(feats, B)
        # (an injected host filter is called in pair order: one group)
        st = rounds.RoundState(self, [dict(H=[], flowD2=[], flowDown8=[], matchDown8=[]) for _ in range(B)], "kitti", rounds.KITTI_SPLIT,
                               split, sample_fn, records, want_lists, trace, pair_ids, draw_epoch, maskRegionTh,
                               host_filter=remove_small_cc is not None)
        # the rounds are the Hpatch driver's with the KITTI fine pass / accept mode / stop rule (rounds.KittiGroup): lock-step
        # groups on streams, ready-first scheduling, the exact mode's host stage hidden under the other groups' kernels
        batch = dict(feats=feats, idx1=idx1, idx2=idx2, cnt=cnt, bg=None if It_bg is None else It_bg.to(dev).float().contiguous(),
                     Mask=torch.zeros((B, h_org, w_org), dtype=torch.float32, device=dev), nbH=torch.zeros(B, dtype=torch.int32, device=dev),
                     tensor_s=tensor_s, tensor_d2=tensor_d2, tensor_resize=tensor_resize, cc_th=cc_th, remove_small_cc=remove_small_cc)
        rounds.drive_rounds(self, [rounds.lockstep_rounds(rounds.KittiGroup(st, batch, lo, hi)) for lo, hi in st.bounds])
        return st.close(lambda b: batch["Mask"][b], (idx1, idx2, cnt))

    def _multi_h_kitti_batched_ragged(self, src_l, tgt_l, fineSize, maskRegionTh, cc_th, It_bg, sample_fn, remove_small_cc, records,
                                      want_lists, trace, pair_ids, draw_epoch, split):
        """multi_h_kitti_batched for pairs of different sizes (src_l / tgt_l: per-pair (H,W,3) uint8 device tensors).  One grouped
        trunk pass and one ragged mutual matching (prepare_ragged_device, _features_ragged, _mutual_ragged), the fine-stage images
        from one LANCZOS / float-conversion chain per distinct shape, then the lock-step rounds of rounds.RaggedKittiGroup: per round
        and group ONE filter launch, ONE draw, ONE RANSAC search, ONE small-component filter (rfx_remove_small_cc_ragged_f32) and ONE
        accept launch (rfx_multih_accept_ragged_d2_f32) for all active pairs whatever their sizes, and one host readback; only the
        two PredFlowMask passes run per group of active pairs that share (source original shape, target original shape)."""
        B = len(src_l)
        prep = self.prepare_ragged_device(src_l, tgt_l)
        feats = self.features(prep)
        tabs = ragged_kitti_tables(prep["plan"], [(x.shape[1], x.shape[0]) for x in tgt_l], fineSize)
        if records is not None:
            ops.MultiHRecordsRagged.require(records, [g[4:6] for g in tabs["geom"]], tabs["d2"])
        # the fine-stage images: sources at their ORIGINAL size, targets at fineSize and fineSize // 2 -- one chain per distinct shape
        # (image 2 b = the source of pair b, 2 b + 1 its target)
        tensor_s, tensor_resize, tensor_d2 = [None] * B, [None] * B, [None] * B
        imgs = [x for pair in zip(src_l, tgt_l) for x in pair]
        for (is_tgt, _), mem in ragged.by_shape([(j % 2, tuple(x.shape)) for j, x in enumerate(imgs)]).items():
            u8, bs = torch.stack([imgs[j] for j in mem]), [j // 2 for j in mem]
            if is_tgt:
                (h_r, w_r), (h_d2, w_d2) = tabs["resize"][bs[0]], tabs["half"][bs[0]]
                ragged.hand_back(tensor_resize, bs, ops.u8_to_f32(ops.lanczos_resize_u8(u8, w_r, h_r))[0])
                ragged.hand_back(tensor_d2, bs, ops.u8_to_f32(ops.lanczos_resize_u8(u8, w_d2, h_d2))[0])
            else:
                ragged.hand_back(tensor_s, bs, ops.u8_to_f32(u8)[0])
        idx1, idx2, cnt = self._mutual_ragged(feats)
        st = rounds.RoundState(self, [dict(H=[], flowD2=[], flowDown8=[], matchDown8=[]) for _ in range(B)], "kitti", rounds.KITTI_SPLIT,
                               split, sample_fn, records, want_lists, trace, pair_ids, draw_epoch, maskRegionTh,
                               host_filter=remove_small_cc is not None)
        pb = ragged.PackedBatch(tabs, It_bg, self.dev, extra_rows=tabs["d2"])
        batch = dict(pb.fields(), feats=feats, idx1=idx1, idx2=idx2, cnt=cnt, d2dims=pb.extra, d2=tabs["d2"], tensor_s=tensor_s,
                     tensor_d2=tensor_d2, tensor_resize=tensor_resize, cc_th=cc_th, remove_small_cc=remove_small_cc)
        rounds.drive_rounds(self, [rounds.lockstep_rounds(rounds.RaggedKittiGroup(st, batch, lo, hi)) for lo, hi in st.bounds])
        return st.close(pb.mask_of, (idx1, idx2, cnt))

    def multi_h_kitti_pairs(self, pairs, fineSize=650, maskRegionTh=0.005, cc_th=0.01, It_bg=None, sample_fn=None, remove_small_cc=None,
                            records=None, want_lists=True, trace=None, pair_ids=None, draw_epoch=0, split=None, seg=None):
        """multi_h_kitti_batched on pairs of PIL images.  All sources of one size and all targets of one size: upload_raw(), today's
        dense path (``It_bg`` (B,h,w), ``records`` an ops.MultiHRecords).  Otherwise per-pair uploads and the ragged path (``It_bg`` a
        list of per-pair tensors, ``records`` an ops.MultiHRecordsRagged with the d2 lists).  ``seg`` instead of ``It_bg``: It_bg at
        (h_org, w_org) from the uploaded targets (evaluation/evalKITTI/evaluation.py:245-248; sky_backgrounds)."""
        mixed = self._mixed_sizes(pairs)
        src, tgt = self._upload_lists(pairs) if mixed else self.upload_raw(pairs)
        if self._seg_or_bg(seg, It_bg):
            bgs = self.sky_backgrounds(seg, list(tgt), [(int(t.shape[0]), int(t.shape[1])) for t in tgt])
            It_bg = bgs if mixed else torch.stack(bgs)
        return self.multi_h_kitti_batched(src, tgt, fineSize=fineSize, maskRegionTh=maskRegionTh, cc_th=cc_th, It_bg=It_bg,
                                          sample_fn=sample_fn, remove_small_cc=remove_small_cc, records=records, want_lists=want_lists,
                                          trace=trace, pair_ids=pair_ids, draw_epoch=draw_epoch, split=split)

    # ---------------------------------------------------------------- whole path
    def align_prepared(self, prep, fine=True, samples=None, feats=None, pair_ids=None, draw_epoch=0, want_u8=False):
        """coarse() + fine_quickstart() of a prep from prepare / prepare_device or, for pairs of different sizes, prepare_ragged /
        prepare_ragged_device.  A ragged batch gives every pair, bit for bit, what it gives alone (same ``pair_ids`` / draws); it
        runs eagerly (no HIP-graph capture).  multi_h_batched takes ragged preps too (multi_h_pairs), and multi_h_kitti_batched takes
        lists of images of different sizes (multi_h_kitti_pairs), and so does multi_h_variant_c (multi_h_variant_c_pairs; without
        records).  Not covered for ragged batches: the drop-in modules.
        ``want_u8`` (with ``fine``): every result also carries ``img1_fine_u8`` (1,H,W,3) uint8, the aligned source as an image
        (quick_start/align2images.py:97-98: ToPILImage of img1_fine), made in one launch for the batch by ops.warp_flow_u8 from
        flow12 and the prep's uint8 source ``Is_u8``; equal to (img1_fine.clamp(0, 1) * 255).byte() as HWC.  Nothing else changes.
        Preps with ``Is_u8``: prepare_device, prepare_and_features and prepare_ragged_device always (they hold the bytes anyway, at
        no cost), prepare / prepare_ragged when called with want_u8=True (align_pairs does that).  Preps without: prepare /
        prepare_ragged by default, prepare_candidates_device (its fine stage belongs to the multi-homography drivers)."""
        if want_u8 and fine and prep.get("Is_u8") is None:
            raise ValueError("align_prepared: want_u8 needs the prep's uint8 source Is_u8: prepare(pairs, want_u8=True) / "
                             "prepare_ragged(pairs, want_u8=True), or a prep of prepare_device / prepare_ragged_device")
        res = self.coarse(prep, feats=feats, samples=samples, pair_ids=pair_ids, draw_epoch=draw_epoch)
        if fine:
            eye = torch.eye(3, device=self.dev)
            Hs = torch.stack([r["H"] if r["H"] is not None else eye for r in res])
            if prep.get("ragged"):
                for r, f in zip(res, self._fine_ragged(prep, Hs)):
                    r["flow12"], r["img1_fine"], r["flowDown"] = f["flow12"], f["img1_fine"], f["flowDown"]
                if want_u8:
                    imgs = ops.warp_flow_u8([r["flow12"][0] for r in res], list(prep["Is_u8"]))[0]
                    for r, im in zip(res, imgs):
                        r["img1_fine_u8"] = im[None]
                return res
            f = self.fine_quickstart(prep, Hs)
            u8 = ops.warp_flow_u8(f["flow12"], prep["Is_u8"])[0] if want_u8 else None
            for b, r in enumerate(res):
                r["flow12"] = f["flow12"][b:b + 1]
                r["img1_fine"] = f["img1_fine"][b:b + 1]
                r["flowDown"] = f["flowDown"][b:b + 1]
                if want_u8:
                    r["img1_fine_u8"] = u8[b:b + 1]
        return res

    def align_pairs(self, pairs, fine=True, samples=None, pair_ids=None, want_u8=False):
        """Pairs of PIL images.  All sources of one size and all targets of one size: prepare(), today's dense path.  Otherwise the
        ragged path (prepare_ragged).  ``want_u8``: see align_prepared."""
        prep = self.prepare_ragged(pairs, want_u8) if self._mixed_sizes(pairs) else self.prepare(pairs, want_u8)
        return self.align_prepared(prep, fine=fine, samples=samples, pair_ids=pair_ids, want_u8=want_u8)

    def multi_h_pairs(self, pairs, maxCoarse=10, maskRegionTh=0.01, It_bg=None, sample_fn=None, records=None, want_lists=True,
                      trace=None, pair_ids=None, draw_epoch=0, split=None, seg=None):
        """multi_h_batched on pairs of PIL images.  All sources of one size and all targets of one size: prepare(), today's dense
        path (``It_bg`` (B,h,w), ``records`` an ops.MultiHRecords).  Otherwise prepare_ragged() and the ragged path (``It_bg`` a
        list of per-pair tensors, ``records`` an ops.MultiHRecordsRagged).  ``seg`` (a segnet.SegNetDevice) instead of ``It_bg``: the
        scripts' --segNet, It_bg formed on the device from the targets at their resized size (sky_backgrounds)."""
        mixed = self._mixed_sizes(pairs)
        if self._seg_or_bg(seg, It_bg):
            bgs = self.sky_backgrounds(seg, self._upload_targets(pairs), [self._target_resized_hw(p[1].size[1], p[1].size[0]) for p in pairs])
            It_bg = bgs if mixed else torch.stack(bgs)
        prep = self.prepare_ragged(pairs) if mixed else self.prepare(pairs)
        return self.multi_h_batched(prep, maxCoarse=maxCoarse, maskRegionTh=maskRegionTh, It_bg=It_bg, sample_fn=sample_fn,
                                    records=records, want_lists=want_lists, trace=trace, pair_ids=pair_ids, draw_epoch=draw_epoch,
                                    split=split)
