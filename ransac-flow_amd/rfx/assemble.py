"""Offline flow assembly: what the reference's ``getResults.py`` scripts do with the arrays the
evaluation scripts saved -- per pair ``n`` homographies, their stride-8 fine flows and matchability maps -- to obtain
ONE dense flow (and confidence) at the evaluation resolution:

    coarse_i = warp_grid(H_i);  flowUp_i = clamp(up(flowDown_i) + identity, -1, 1);  flow_i = grid_sample(coarse_i, flowUp_i)
    score_i  = up(match12_i) [* grid_sample(up(match21_i), flowUp_i)] * in_bounds(flow_i)
    owner(p) = 0 if score_0(p) >= th else first i >= 1 with score_i(p) >= th (multiH) else 0

Reference: evaluation/evalHpatch/getResults.py:16-63, evaluation/evalCorr/getResults.py:78-136,
evaluation/evalKITTI/getResults.py:95-141, evaluation/evalYFCC/getResults.py:132-190.  Device work = librfx kernels (rfx_warp_grid_f32, rfx_compose_flow_f32,
rfx_resize_bilinear_f32, rfx_grid_sample_f32, rfx_match_score_f32, rfx_merge_multi_h_f32); reading the ``.npy`` files
KITTI's connected-component filter runs on the device (rfx_remove_small_cc_f32).  Its nearest-neighbour fill (--interpolate) runs
where ``fill`` says: "host" (the default) copies flow and mask to the host and calls scipy like the reference; "device" is
rfx_nearest_fill_f32, scipy's indices reproduced index for index, with no host transfer and no sync.
What the YFCC and Corr scripts then READ off the assembled maps stays on the device as well: the correspondences of all explained
pixels (yfcc_matches: rfx_flow_points_f32, evalYFCC/getResults.py:53-71) and the transfer of annotated keypoints
(corr_alignment_error: rfx_sample_points_f32, evalCorr/getResults.py:15-38; 3 K values cross the bus, not the maps).
The end-point error the HPatches and KITTI scripts end in is reduced on the device too (hpatch_epe: rfx_epe_homography_f32,
evalHpatch/getResults.py:83-156,221-250 -- the ground-truth map is formed per pixel from the nine numbers of hpatch_gt_homography;
kitti_epe: rfx_epe_flow_f32, evalKITTI/getResults.py:221-228); one float64 sum and one count per map cross the bus.
A whole BATCH whose arrays still lie on the device as the drivers' records (ops.MultiHRecords / ops.MultiHRecordsRagged) is assembled
by assemble_records / assemble_yfcc_records in ONE launch (rfx_assemble_records_f32): per pair bit for bit what assemble /
assemble_yfcc give on the record's first nbH entries, with nbH read on the device, no (n,H,W) intermediate and no host sync -- the
HPatches, Corr and YFCC forms.  KITTI's records (with flowD2) go through assemble_kitti_records (rfx_assemble_kitti_records_f32, with
cc_th > 0 also rfx_kitti_scores_records_f32 and the ragged component filter): the two-level composition is evaluated per pixel, the
filter runs on one packed score buffer per chunk of pairs, and the --interpolate fill is ops.nearest_fill on the batch.
The YFCC results step has its batch form as well: yfcc_matches_records takes the records multi_h_variant_c(..., want_records=True)
builds for pairs of any sizes to the correspondences of every pair -- one assembly launch, the three launches of
rfx_flow_points_ragged_f32 and ONE host read for the batch; yfcc_norm_kp is the script's norm_kp on the host.

On-disk formats (written by evaluation/evalHpatch/evaluation.py:254-260 and friends):
    <fine>/flow_{id}_{n}H.npy   (n,2,h/8,w/8) float   fine flow, stride 8
    <fine>/mask_{id}_{n}H.npy   (n,2,h/8,w/8) float   matchability 1->2 | 2->1
    <coarse>/flow_{id}_{n}H.npy (n,3,3)        float   homographies
    <mask>/maskBG_{id}_{n}H.npy (h,w) bool              background mask (loaded by evalCorr, unused in its assembly; YFCC ANDs it
                                                        with the explained mask)
    KITTI: Homograpy_{id}_{n}.npy, {res}_D2_{id}_{n}.npy, {res}_{id}_{n}.npy, {res}_Mask_{id}_{n}.npy, BG_{id}_{n}H.npy
"""
import os

import numpy as np
import torch

from . import ops


def find_nbH(pairID, flowList):
    """The reference's lookup (evalHpatch/getResults.py:17-22): first listed name whose second '_' field is the pair
    id; returns the text between the second '_' and 'H', or None."""
    for name in flowList:
        parts = name.split("_")
        if len(parts) > 2 and parts[1] == str(pairID):
            return parts[2].split("H")[0]
    return None


def _to_dev(a, device):
    """numpy array (the saved .npy files) or tensor (the views of an ops.MultiHRecords: no host round trip) -> float32 on ``device``."""
    if torch.is_tensor(a):
        return a.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.float32))).to(device)


def assemble(flowDown, param, matchDown, out_hw, th, multiH, cycle, device="cuda"):
    """-> (flowGlobal (1,H,W,2), matchGlobal (1,H,W), binary (1,H,W) bool) device tensors."""
    H, W = int(out_hw[0]), int(out_hw[1])
    fd, pm, md = _to_dev(flowDown, device), _to_dev(param, device), _to_dev(matchDown, device)
    coarse = ops.warp_grid(pm, H, W)
    flow, inb, fup = ops.compose_flow(fd, coarse, clamp=True, want_inb=True, want_flow_up=cycle)
    m = ops.resize_bilinear(md, (H, W), align_corners=False)
    cyc = ops.grid_sample(m[:, 1:2].contiguous(), fup)[:, 0] if cycle else None
    return ops.merge_multi_h(flow, m[:, 0], th, multiH, cyc=cyc, inb=inb)


def assemble_yfcc(flowDown, param, matchDown, matchBG, th, multiH, device="cuda"):
    """evalYFCC/getResults.py:150-190 (_getFlow): assemble(..., cycle=True) at 8h x 8w, the explained mask ANDed with the background
    mask matchBG (8h,8w) -> (flowGlobal (1,H,W,2), binary (1,H,W) bool) device tensors."""
    h, w = int(flowDown.shape[2]), int(flowDown.shape[3])
    fg, _, binary = assemble(flowDown, param, matchDown, (h * 8, w * 8), th, multiH, True, device)
    bg = matchBG if torch.is_tensor(matchBG) else torch.from_numpy(np.ascontiguousarray(np.asarray(matchBG) != 0))
    return fg, binary & (bg.to(fg.device) != 0).reshape(1, h * 8, w * 8)


def assemble_records(records, th, multiH, cycle, out_hw=None, bg=None):
    """assemble() for every pair of a batch of device records at once (ops.assemble_records): cycle=False at any ``out_hw`` is the
    HPatches form (evalHpatch/getResults.py:16-63), cycle=True at the default 8x size the Corr form (evalCorr/getResults.py:78-136).
    -> (flowGlobal, matchGlobal, binary, valid): (B,H,W,2), (B,H,W), (B,H,W) bool for dense records, lists of per-pair maps for
    ragged ones; valid (B,) bool on the device = the pair has a homography -- where the scripts return [] the maps are zero."""
    return ops.assemble_records(records, th, multiH, cycle, out_hw=out_hw, bg=bg)


def assemble_yfcc_records(records, bg, th, multiH):
    """assemble_yfcc() for every pair of a batch of device records at once: cycle=True at 8h x 8w, the explained mask ANDed with the
    background maps ``bg`` -- (B,8h,8w) for dense records, one (8h_b,8w_b) map per pair for ragged ones; tensors on the records'
    device (bool / uint8; anything else counts as != 0) or numpy arrays, which are uploaded.  -> (flowGlobal, binary, valid)."""
    dev = records.rec.device

    def mask(m):
        t = m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(np.asarray(m) != 0)).to(dev)
        return t if t.dtype in (torch.bool, torch.uint8) else t != 0
    bg = [mask(m) for m in bg] if isinstance(bg, (list, tuple)) else mask(bg)
    fg, _, binary, valid = ops.assemble_records(records, th, multiH, True, bg=bg)
    return fg, binary, valid


def aligned_images_records(records, src_u8, th, multiH, cycle, out_hw=None, bg=None, tgt_u8=None, want_mask=False):
    """The aligned source image of every pair of a batch of device records, as uint8 HWC (ops.warp_records_u8;
    quick_start/align2images.py:97-98,117: F.grid_sample(IsTensor, flow12) -> ToPILImage, and with ``tgt_u8`` get_Avg_Image of
    :25-28,112), in one launch: what assemble_records -> grid_sample -> mul(255).byte() gives per pair, without the flow or any float
    image.  src_u8 / tgt_u8: a (B,H,W,3) uint8 tensor or one (H_b,W_b,3) uint8 device tensor per pair -- sources of any sizes, each
    target at its pair's output size.  -> (img, overlay | None, mask | None, valid): (B,H,W,3) for dense records, lists of per-pair
    images for ragged ones; valid (B,) bool on the device."""
    return ops.warp_records_u8(records, src_u8, th, multiH, cycle, out_hw=out_hw, bg=bg, tgt=tgt_u8, want_mask=want_mask)


def aligned_image(flow, src_u8, tgt_u8=None):
    """The same image from a flow the caller holds (ops.warp_flow_u8): ``flow`` (H,W,2) / (B,H,W,2) float32 or a list of per-pair
    maps -- quick-start's flow12, assemble_kitti_records' flow.  -> img, or (img, overlay) with ``tgt_u8``."""
    img, overlay, _ = ops.warp_flow_u8(flow, src_u8, tgt=tgt_u8)
    return img if tgt_u8 is None else (img, overlay)


def yfcc_matches(flowGlobal, binary, sizeA, sizeB, angle):
    """evalYFCC/getResults.py:53-71 (matches_from_flow) on the maps assemble_yfcc returns, (1,H,W,2) and (1,H,W), or on single
    (H,W,2) / (H,W) maps; numpy arrays are uploaded.  sizeA = (wA, hA), sizeB = (wB, hB) before the rotation by ``angle``.
    -> (pts1 (n,2) float32, pts2 (n,2) int64) device tensors, in numpy's boolean-indexing order."""
    dev = next((t.device for t in (flowGlobal, binary) if torch.is_tensor(t) and t.is_cuda), "cuda")
    f = _to_dev(flowGlobal, dev)
    b = binary.to(dev) if torch.is_tensor(binary) else torch.from_numpy(np.ascontiguousarray(np.asarray(binary))).to(dev)
    b = b if b.dtype in (torch.bool, torch.uint8) else b != 0
    if f.dim() == 4 and f.shape[0] == 1:
        f, b = f[0], b.reshape(f.shape[1], f.shape[2])
    return ops.matches_from_flow(f, b, sizeA, sizeB, angle)[:2]


def yfcc_matches_records(records, th, multiH, sizesA=None, sizesB=None, angles=None, bg="records", return_maps=False):
    """The YFCC results step (evalYFCC/getResults.py:304-318: getFlow, then matches_from_flow) for EVERY pair of a batch of device
    records at once: ops.assemble_records (cycle=True at 8h x 8w, the background ANDed in) into packed buffers allocated here, then
    ops.matches_from_flow_ragged on those buffers -- one assembly launch, three points launches and ONE host read (the offsets) for
    the whole batch, whatever the pairs' sizes.  Per pair bit for bit assemble_yfcc on the record's first nbH entries followed by
    yfcc_matches.  ``sizesA[b]`` = (wA, hA) of the resized source, ``sizesB[b]`` = (wB, hB) of the resized target BEFORE its rotation
    by ``angles[b]``; the defaults are what multi_h_variant_c(_pairs)(..., want_records=True) left on the records: size_src, size_tgt
    turned back by the angle, angle.  ``bg``: "records" (records.bg, possibly None), None, or what ops.assemble_records takes.
    -> (pts1 (n,2) float32, pts2 (n,2) int64, offsets (B+1,) int64 on the HOST, valid (B,) bool on the device); pair b's points are
    rows offsets[b]:offsets[b+1], a pair without a homography (valid False) has none.  ``return_maps``: also the per-pair
    flowGlobal / binary views of the packed buffers."""
    rows, _, total = ops.assemble_records_table(records)
    B, dev = records.B, records.rec.device
    sizes = [(r[4], r[5]) for r in rows]
    sizesA = getattr(records, "size_src", None) if sizesA is None else sizesA
    if sizesA is None:
        raise ValueError("yfcc_matches_records: these records carry no size_src; pass sizesA = one (wA, hA) per pair")
    angles = getattr(records, "angle", None) if angles is None else angles
    if angles is None:
        raise ValueError("yfcc_matches_records: these records carry no angle (multi_h_variant_c_pairs sets it); pass angles")
    ptab = ops.flow_points_ragged_table(sizes, sizesA, angles)[0]                # checks lengths, angles and sizes on the host
    if sizesB is None:
        tgt = getattr(records, "size_tgt", None)
        if tgt is None:
            raise ValueError("yfcc_matches_records: these records carry no size_tgt; pass sizesB = one (wB, hB) per pair")
        sizesB = [(h, w) if r[3] & 1 else (w, h) for (w, h), r in zip(tgt, ptab)]
    if len(sizesB) != B:
        raise ValueError("yfcc_matches_records: %d sizesB for %d pairs" % (len(sizesB), B))
    for b, ((wB, hB), r) in enumerate(zip(sizesB, ptab)):
        want = (int(wB), int(hB)) if r[3] & 1 else (int(hB), int(wB))
        if (r[1], r[2]) != want:
            raise ValueError("yfcc_matches_records: pair %d's map of shape %s does not fit sizeB = %s at angle %s (%s expected)"
                             % (b, (r[1], r[2]), (wB, hB), 90 * r[3], want))
    if isinstance(bg, str):
        if bg != "records":
            raise ValueError("yfcc_matches_records: bg is \"records\", None or background maps, got %r" % bg)
        bg = getattr(records, "bg", None)
    out = (torch.empty((total, 2), dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.float32, device=dev),
           torch.empty(total, dtype=torch.bool, device=dev))
    flows, _, binaries, valid = ops.assemble_records(records, th, multiH, True, bg=bg, out=out)
    pts1, pts2, off = ops.matches_from_flow_ragged(out[0], out[2], sizes, sizesA, [90 * r[3] for r in ptab])
    return (pts1, pts2, off, valid, flows, binaries) if return_maps else (pts1, pts2, off, valid)


def yfcc_norm_kp(org_size, new_size, K, kp):
    """evalYFCC/getResults.py:29-50 (norm_kp): pixel coordinates ``kp`` (n,2) of an image resized from ``org_size`` = (w, h) to
    ``new_size`` = (w_n, h_n) -> image-plane coordinates under the calibration K (3,3), whose principal point is given relative to
    the image centre.  numpy float64 on host arrays, the script's own operations in its order (the points have to cross the bus for
    cv2's pose solver anyway): not a device op."""
    (w, h), (w_n, h_n) = org_size, new_size
    sx, sy = w_n / w, h_n / h                                      # the resize, per axis
    centre = np.array([[((w - 1.0) * 0.5 + K[0, 2]) * sx, ((h - 1.0) * 0.5 + K[1, 2]) * sy]])
    focal = np.array([[K[0, 0] * sx, K[1, 1] * sy]])
    return (kp - centre) / focal


def corr_alignment_error(wB, hB, wA, hA, XA, YA, XB, YB, flow, match2, pixelGrid, device="cuda"):
    """evalCorr/getResults.py:15-38 (alignmentError): flow (1,hB,wB,2) and match2 (1,hB,wB,1) as corr_getFlow returns them (or
    arrays), keypoints XA, YA (source) and XB, YB (target) as numpy arrays -- floats are truncated toward zero, like the reference's
    astype(np.int64) --, pixelGrid (1,T).  The maps are read on the device at the K target keypoints (ops.sample_points); the
    distances of the kept keypoints and their tally under the T thresholds are numpy float64 on the host, where the reference
    promotes too.  -> (counts (T,), nbAlign), zeros when no keypoint is kept."""
    dev = next((t.device for t in (flow, match2) if torch.is_tensor(t) and t.is_cuda), device)
    f = _to_dev(flow, dev).reshape(int(hB), int(wB), 2)
    m = _to_dev(match2, dev).reshape(int(hB), int(wB))
    xa, ya = np.asarray(XA).astype(np.int64), np.asarray(YA).astype(np.int64)
    xaH, yaH, keep = (t.cpu().numpy() for t in ops.sample_points(f, m, XB, YB, (wA, hA)))
    index = np.where(keep)[0]
    nbAlign = len(index)
    if nbAlign == 0:
        return np.zeros(pixelGrid.shape[1]), nbAlign
    pixelDiff = ((xaH[index] - xa[index]) ** 2 + (yaH[index] - ya[index]) ** 2) ** 0.5
    return np.sum(pixelDiff.reshape((-1, 1)) <= pixelGrid, axis=0), nbAlign


def corr_keypoints_records(records, th, multiH, XA, YA, XB, YB, matchability_ths=(0,), pixelGrid=None, sizesA=None, bg=None):
    """The Corr results step (evalCorr/getResults.py:271-285: getFlow, then alignmentError per matchability threshold) for EVERY pair
    of a batch of device records at once, without the dense maps: ops.records_keypoints (cycle=True at the 8x size) reads the
    assembly at the target keypoints only, ops.pck_tally forms the float64 distances and the per-pair tally -- two launches, two
    pinned uploads, no host sync.  XA, YA (source) and XB, YB (target): one host array per pair, floats truncated toward zero like
    the script's astype(np.int64); ``sizesA[b]`` = (wA, hA) of the resized source, by default records.size_src (what
    multi_h_variant_c(..., want_records=True) leaves there).  A pair without a homography follows the script's ``continue`` branch.
    -> (counts (M,B,T) int64, nbAlign (M,B) int64, valid (B,) bool) on the device; corr_precision reads them."""
    xa, ya, m, flag, koff = ops.records_keypoints(records, th, multiH, True, XB, YB, sizesA=sizesA, bg=bg)
    valid = records.rec[:, 0] >= 1                             # the kernels' own test of nbH
    grid = None if pixelGrid is None else np.asarray(pixelGrid, dtype=np.float64).reshape(-1)
    counts, nb = ops.pck_tally(xa, ya, m, flag, XA, YA, koff, match_ths=matchability_ths, pixel_grid=grid, valid=valid)
    return counts, nb, valid


def corr_precision(counts, nbAlign):
    """The table the script prints (evalCorr/getResults.py:287-289) from corr_keypoints_records' device tallies -- the one host read
    of the batch: -> (precision (M,T) float64 = counts summed over the pairs / nbAlign summed over the pairs, total (M,) int64)."""
    c = (counts.cpu() if torch.is_tensor(counts) else torch.as_tensor(np.asarray(counts))).numpy().sum(axis=1)
    n = (nbAlign.cpu() if torch.is_tensor(nbAlign) else torch.as_tensor(np.asarray(nbAlign))).numpy().sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):       # no kept keypoint: the script's 0 / 0
        return c.astype(np.float64) / n[:, None], n


def corr_resize_keypoints(minSize, size, x, y, strideNet=16, megadepth=False):
    """The coordinate half of evalCorr/getResults.py:41-56 (ResizeMinResolution) and :60-76 (ResizeMinResolution_megadepth): an image
    of ``size`` = (w, h) is resized so that its shorter side is about ``minSize``, both sides rounded down to multiples of
    ``strideNet``, and the keypoints move with it.  x, y: arrays, or the CSV's ';'-separated strings; float32 like the script's.
    -> ((new_w, new_h), x, y[, index_valid: megadepth -- the keypoints strictly inside the resized image])."""
    parse = lambda v: np.array([float(t) for t in v.split(";")] if isinstance(v, str) else v).astype(np.float32)
    x, y = parse(x), parse(y)
    w, h = size
    ratio = min(w / float(minSize), h / float(minSize))
    new_w, new_h = round(w / ratio), round(h / ratio)
    new_w, new_h = new_w // strideNet * strideNet, new_h // strideNet * strideNet
    ratioW, ratioH = new_w / float(w), new_h / float(h)
    x, y = x * ratioW, y * ratioH
    if megadepth:
        return (new_w, new_h), x, y, (x > 0) * (x < new_w) * (y > 0) * (y < new_h)
    return (new_w, new_h), x, y


def identity_grid(h, w, device="cuda"):
    """The grid the scripts fall back to when a pair has no saved flow (evalHpatch/getResults.py:191-193,218;
    evalKITTI/getResults.py:209-214): torch.linspace(-1, 1, w) along x and (-1, 1, h) along y, (1,h,w,2).  ops.warp_grid of the
    identity homography gives it exactly (x * 1 + y * 0 + 0, divided by 1)."""
    return ops.warp_grid(torch.eye(3, dtype=torch.float32, device=device)[None], int(h), int(w))


def hpatch_gt_homography(H, ref_hw, trg_hw, size):
    """evalHpatch/getResults.py:107-117 (getGT): the ground-truth homography H (3,3), given for the original images of (h, w) =
    ref_hw and trg_hw, mapped to size x size images (size: an int, the script's minSize, or (h_scale, w_scale)) -- the product
    S2 H inv(S1) with the diagonal scale matrices S1 (source) and S2 (target) -- and its inverse.  numpy float64 on the host, the
    reference's own calls in its order, so the same nine numbers.  -> (H_scale, Hinv)."""
    h_scale, w_scale = (size, size) if np.ndim(size) == 0 else (size[0], size[1])
    (h_ref, w_ref), (h_trg, w_trg) = ref_hw, trg_hw
    S1 = np.array([[w_scale / w_ref, 0, 0], [0, h_scale / h_ref, 0], [0, 0, 1]])
    S2 = np.array([[w_scale / w_trg, 0, 0], [0, h_scale / h_trg, 0], [0, 0, 1]])
    H_scale = np.dot(np.dot(S2, np.asarray(H, dtype=np.float64).reshape(3, 3)), np.linalg.inv(S1))
    return H_scale, np.linalg.inv(H_scale)


def _mean(total, count, as_float32):
    """sum / count per map on the host, after ONE read of both -> a list of Python floats; NaN for a map without a counted pixel
    (the mean of nothing)."""
    both = torch.stack((total.reshape(-1), count.reshape(-1).to(torch.float64))).cpu().tolist()    # a count is exact in float64
    out = []
    for s, c in zip(*both):
        m = s / int(c) if c else float("nan")
        out.append(float(np.float32(m)) if as_float32 else m)
    return out


def hpatch_epe(flow_est, Hinv, size=None, device="cuda"):
    """evalHpatch/getResults.py:218-250: the average end-point error of flow_est -- the (1,S,S,2) device tensor hpatch_getFlow_all
    returns, or its [] for a pair without a saved flow, which stands for the identity grid of ``size`` x ``size`` -- against the
    ground truth Hinv defines (hpatch_gt_homography's second result), over the pixels the ground truth keeps inside [-1,1]^2.  The
    map stays on the device (ops.epe_homography); a sum and a count come back.  -> float32(sum / count) as a Python float, NaN when
    no pixel is inside.  A batch -- flow_est (N,S,S,2) with Hinv (N,3,3) -- gives a list of N."""
    h = np.asarray(Hinv.cpu() if torch.is_tensor(Hinv) else Hinv, dtype=np.float64)
    batch = h.ndim == 3
    h = h.reshape(-1, 9)
    if not torch.is_tensor(flow_est) and len(flow_est) == 0:
        if size is None:
            raise ValueError("hpatch_epe: a pair without a saved flow needs size (the identity grid's)")
        sh, sw = (size, size) if np.ndim(size) == 0 else (size[0], size[1])
        flow_est = identity_grid(sh, sw, device).expand(len(h), -1, -1, -1)
    dev = flow_est.device if torch.is_tensor(flow_est) and flow_est.is_cuda else device
    f = _to_dev(flow_est, dev)
    f = f[None] if f.dim() == 3 else f
    total, count = ops.epe_homography(f, torch.from_numpy(h).to(f.device))
    out = _mean(total, count, True)
    return out if batch else out[0]


def _exact_f32(a, name):
    """A ground-truth array or tensor as a float32 tensor, refused if that changes a value (KITTI's (uint16 - 32768) / 64 never
    does)."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    t32 = t.to(torch.float32)
    if t.dtype != torch.float32 and not torch.equal(t32.to(torch.float64), t.to(torch.float64)):
        raise ValueError("kitti_epe: %s has values that float32 does not hold exactly" % name)
    return t32


def kitti_epe(flowGlobal, u, v, valid, device="cuda"):
    """evalKITTI/getResults.py:221-228: the average end-point error of the assembled flow -- the (1,H,W,2) device tensor
    assemble_kitti / kitti_getFlow_all return, or [] for a pair without prediction (the identity grid) -- against the ground truth
    u, v (H,W) of readFlow (:17-24; arrays or tensors whose values float32 holds exactly: anything else is refused) over the pixels with
    valid set.  The flow stays on the device (ops.epe_flow); u, v, valid go up, a sum and a count come back.  -> sum / count in
    float64 as a Python float, NaN when nothing is valid.  A batch -- (N,H,W,2) with (N,H,W) arrays -- gives a list of N."""
    uh, vh = _exact_f32(u, "u"), _exact_f32(v, "v")                    # refused here, before the flow is touched
    batch = uh.dim() == 3
    H, W = int(uh.shape[-2]), int(uh.shape[-1])
    if not torch.is_tensor(flowGlobal) and len(flowGlobal) == 0:
        flowGlobal = identity_grid(H, W, device).expand(uh.shape[0] if batch else 1, -1, -1, -1)
    dev = flowGlobal.device if torch.is_tensor(flowGlobal) and flowGlobal.is_cuda else device
    f = _to_dev(flowGlobal, dev)
    f = f[None] if f.dim() == 3 else f
    m = valid if torch.is_tensor(valid) else torch.from_numpy(np.ascontiguousarray(np.asarray(valid)))
    m = (m if m.dtype in (torch.bool, torch.uint8) else m != 0).to(dev)
    shape = (f.shape[0], H, W)
    total, count = ops.epe_flow(f, uh.to(dev).reshape(shape).contiguous(), vh.to(dev).reshape(shape).contiguous(), m.reshape(shape))
    out = _mean(total, count, False)
    return out if batch else out[0]


def remove_small_cc(score, cc_th, match_th=0.99):
    """evalKITTI/getResults.py:66-84 (skimage.measure.label on the host there) on the device: rfx_remove_small_cc_f32."""
    return ops.remove_small_cc(score, cc_th, match_th)


FILLS = ("host", "device")


def _check_fill(fill):
    if fill not in FILLS:
        raise ValueError("fill must be one of %s, got %r" % (FILLS, fill))


def interpolate_flow_match(flowGlobal, binary, fill="host"):
    """evalKITTI/getResults.py:87-93: every pixel takes the flow of its nearest explained pixel.  fill="host": scipy on the host,
    like the reference; fill="device": ops.nearest_fill (the same indices, ties included), asynchronous on the current stream."""
    _check_fill(fill)
    if fill == "device":
        return ops.nearest_fill(flowGlobal, binary)
    from scipy import ndimage
    idx = ndimage.distance_transform_edt((~binary[0]).cpu().numpy(), return_distances=False, return_indices=True)
    f = flowGlobal[0].cpu().numpy()[tuple(idx)]
    return torch.from_numpy(f).unsqueeze(0).to(flowGlobal.device)


def assemble_kitti(flowd2Down, flowDown, param, matchDown, out_hw, th, multiH, cc_th=0.0, interpolate=False,
                   device="cuda", fill="host"):
    _check_fill(fill)
    H, W = int(out_hw[0]), int(out_hw[1])
    d2d, fd = _to_dev(flowd2Down, device), _to_dev(flowDown, device)
    pm, md = _to_dev(param, device), _to_dev(matchDown, device)
    hom = ops.warp_grid(pm, H, W)
    d2, _, _ = ops.compose_flow(d2d, hom, clamp=True)
    flow, inb, fup = ops.compose_flow(fd, d2, clamp=True, want_inb=True, want_flow_up=True)
    m = ops.resize_bilinear(md, (H, W), align_corners=False)
    cyc = ops.grid_sample(m[:, 1:2].contiguous(), fup)[:, 0]
    if cc_th == 0:
        fg, mg, binary = ops.merge_multi_h(flow, m[:, 0], th, multiH, cyc=cyc, inb=inb)
    else:
        score = remove_small_cc(ops.match_score(m[:, 0], cyc=cyc, inb=inb), cc_th)
        fg, mg, binary = ops.merge_multi_h(flow, score, th, multiH)
    if interpolate:
        fg = interpolate_flow_match(fg, binary, fill)
    return fg, mg, binary


def assemble_kitti_records(records, out_hw, th, multiH, cc_th=0.0, interpolate=False):
    """assemble_kitti(..., fill="device") for every pair of a batch of KITTI device records at once (ops.assemble_kitti_records):
    ``out_hw`` one (H, W) for dense records, one per pair for ragged ones (None: 8x the /8 size).  -> (flowGlobal, matchGlobal,
    binary, valid) as assemble_records returns them; a pair without a homography (valid False) has zeros in all three maps."""
    return ops.assemble_kitti_records(records, th, multiH, cc_th=cc_th, interpolate=interpolate, out_hw=out_hw)


# ---- file-level entry points with the reference's argument lists -------------------------------------------------

def _load(path):
    return np.load(path).astype(np.float32)


def hpatch_getFlow_all(pairID, finePath, coarsePath, flowList, multiH, warper, grid, th, outW, outH, device="cuda"):
    """evalHpatch/getResults.py:16-63.  ``warper`` / ``grid`` are accepted for signature parity and ignored (the grid
    and the homography warp are generated on the device).  Returns [] when the pair has no saved flow."""
    nbH = find_nbH(pairID, flowList)
    if nbH is None:
        return []
    flow = _load(os.path.join(finePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    param = _load(os.path.join(coarsePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    match = _load(os.path.join(finePath, "mask_{:d}_{}H.npy".format(pairID, nbH)))
    return assemble(flow, param, match, (outH, outW), th, multiH, False, device)[0]


def hpatch_getFlow_onlyCoarse(pairID, finePath, coarsePath, flowList, multiH, warper, grid, th, outW, outH,
                              device="cuda"):
    """evalHpatch/getResults.py:65-80: the first homography's grid."""
    nbH = find_nbH(pairID, flowList)
    if nbH is None:
        return []
    param = _load(os.path.join(coarsePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    return ops.warp_grid(_to_dev(param[:1], device), int(outH), int(outW))


def corr_getFlow(pairID, finePath, flowList, coarsePath, maskPath, multiH, th, device="cuda"):
    """evalCorr/getResults.py:78-136 -> (flowGlobal (1,8h,8w,2), matchGlobal (1,8h,8w,1)) or ([], [])."""
    nbH = find_nbH(pairID, flowList)
    if nbH is None:
        return [], []
    flow = _load(os.path.join(finePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    param = _load(os.path.join(coarsePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    match = _load(os.path.join(finePath, "mask_{:d}_{}H.npy".format(pairID, nbH)))
    h, w = flow.shape[2], flow.shape[3]
    fg, mg, _ = assemble(flow, param, match, (h * 8, w * 8), th, multiH, True, device)
    return fg, mg.unsqueeze(3)


def yfcc_getFlow(pairID, finePath, flowList, coarsePath, maskPath, multiH, th, device="cuda"):
    """evalYFCC/getResults.py:132-148 -> (flowGlobal (1,8h,8w,2), binary (1,8h,8w) bool) or ([], [])."""
    nbH = find_nbH(pairID, flowList)
    if nbH is None:
        return [], []
    flow = _load(os.path.join(finePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    param = _load(os.path.join(coarsePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    match = _load(os.path.join(finePath, "mask_{:d}_{}H.npy".format(pairID, nbH)))
    matchBG = np.load(os.path.join(maskPath, "maskBG_{:d}_{}H.npy".format(pairID, nbH)))
    return assemble_yfcc(flow, param, match, matchBG, th, multiH, device)


def corr_getFlow_Coarse(pairID, flowList, finePath, coarsePath, device="cuda"):
    """evalCorr/getResults.py:138-164 -> (grid of homography 0 at 8x, all-ones confidence)."""
    nbH = find_nbH(pairID, flowList)
    if nbH is None:
        return [], []
    flow = np.load(os.path.join(finePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    param = _load(os.path.join(coarsePath, "flow_{:d}_{}H.npy".format(pairID, nbH)))
    h, w = flow.shape[2], flow.shape[3]
    return (ops.warp_grid(_to_dev(param[:1], device), h * 8, w * 8),
            torch.ones(1, h * 8, w * 8, 1, device=device))


def kitti_getFlow_all(pairID, predDir, nbH, res_name, warper_org, multiH, grid_org, th, cc_th, interpolate,
                      device="cuda", fill="host"):
    """evalKITTI/getResults.py:95-141; the output size is that of ``grid_org`` (1,H,W,2), as in the reference.  ``fill``: where the
    nearest-neighbour fill of ``interpolate`` runs (interpolate_flow_match)."""
    param = _load(os.path.join(predDir, "Homograpy_{}_{}.npy".format(pairID, nbH)))
    flowd2 = _load(os.path.join(predDir, "{}_D2_{}_{}.npy".format(res_name, pairID, nbH)))
    flow = _load(os.path.join(predDir, "{}_{}_{}.npy".format(res_name, pairID, nbH)))
    match = _load(os.path.join(predDir, "{}_Mask_{}_{}.npy".format(res_name, pairID, nbH)))
    H, W = int(grid_org.shape[1]), int(grid_org.shape[2])
    return assemble_kitti(flowd2, flow, param, match, (H, W), th, multiH, cc_th, interpolate, device, fill)[0]


def kitti_getFlow_onlyCoarse(pairID, predDir, nbH, res_name, warper_org, multiH, grid_org, th, cc_th, interpolate,
                             device="cuda"):
    """evalKITTI/getResults.py:144-152."""
    param = _load(os.path.join(predDir, "Homograpy_{}_{}.npy".format(pairID, nbH)))
    return ops.warp_grid(_to_dev(param[:1], device), int(grid_org.shape[1]), int(grid_org.shape[2]))
