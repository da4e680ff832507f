"""Drop-in for the flow-assembly functions of the reference's four ``getResults.py`` scripts (which are scripts,
not modules: their bodies parse argv and walk dataset folders that are out of scope).  Same names, argument lists
and return conventions (CPU tensors, ``[]`` sentinels); the arithmetic runs in librfx on the HIP device:

    from getResults import hpatch, corr, kitti, yfcc
    flow = hpatch.getFlow_all(pairID, finePath, coarsePath, flowList, multiH, warper, grid, th, outW, outH)
    flow, match = corr.getFlow(pairID, finePath, flowList, coarsePath, maskPath, multiH, th)
    flow = kitti.getFlow_all(pairID, predDir, nbH, res_name, warper_org, multiH, grid_org, th, cc_th, interpolate)
    counts, nbAlign = corr.alignmentError(wB, hB, wA, hA, XA, YA, XB, YB, flow, match, pixelGrid)
    counts, nbAlign, valid = corr.keypoints_records(records, th, multiH, XA, YA, XB, YB, matchability_ths)   # a whole batch, on the device
    precision, total = corr.precision(counts, nbAlign)                                                    # the one host read
    img, overlay, mask, valid = corr.aligned_images_records(records, src_u8, th, multiH, cycle)     # uint8 HWC, a whole batch, on the device
    img = aligned_image(flow, src_u8)                              # the same image from a flow the caller holds (KITTI, quick start)
    flow, binary = yfcc.getFlow(pairID, finePath, flowList, coarsePath, maskPath, multiH, th)        # numpy, like the script
    pts1, pts2 = yfcc.matches_from_flow(flow, binary, sizeA, sizeB, angle)                             # numpy float32 / int64
    aepe = hpatch.epe_from_homography(flow_est, Hinv)                  # a float; Hinv: rfx.assemble.hpatch_gt_homography(...)[1]
    avg_error = kitti.epe(flow, u, v, valid)                           # a float; u, v, valid as readFlow returns them

Reference: evaluation/evalHpatch/getResults.py:16-80,83-156,218-250, evaluation/evalCorr/getResults.py:15-38,78-164,
evaluation/evalKITTI/getResults.py:95-152,221-228, evaluation/evalYFCC/getResults.py:53-71,132-190.
"""
import os
import sys
import types

_PKG = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from rfx import assemble as _a  # noqa: E402


def _cpu(x):
    if isinstance(x, tuple):
        return tuple(_cpu(v) for v in x)
    return x.cpu() if hasattr(x, "cpu") else x


def _wrap(fn):
    def call(*args, **kw):
        return _cpu(fn(*args, **kw))
    call.__doc__ = fn.__doc__
    call.__name__ = fn.__name__
    return call


def _kitti_getFlow_all(pairID, predDir, nbH, res_name, warper_org, multiH, grid_org, th, cc_th, interpolate, device="cuda"):
    """evalKITTI/getResults.py:95-141 with the reference's argument list.  RFX_KITTI_FILL=host|device (default host) says where
    the nearest-neighbour fill of ``interpolate`` runs (rfx.assemble.interpolate_flow_match); the result is the same tensor."""
    return _a.kitti_getFlow_all(pairID, predDir, nbH, res_name, warper_org, multiH, grid_org, th, cc_th, interpolate, device,
                                fill=os.environ.get("RFX_KITTI_FILL", "host"))


def _np(x):
    if isinstance(x, tuple):
        return tuple(_np(v) for v in x)
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _yfcc_getFlow(pairID, finePath, flowList, coarsePath, maskPath, multiH, th, device="cuda"):
    """evalYFCC/getResults.py:132-148 -> numpy (flowGlobal (H,W,2) float32, match_binary (H,W) bool), or ([], [])."""
    fg, binary = _a.yfcc_getFlow(pairID, finePath, flowList, coarsePath, maskPath, multiH, th, device)
    return (fg, binary) if isinstance(fg, list) else (fg[0].cpu().numpy(), binary[0].cpu().numpy())


def _yfcc__getFlow(flow, param, match, matchBG, multiH, th, device="cuda"):
    """evalYFCC/getResults.py:150-190, the reference's argument order (multiH before th) -> numpy, squeezed like the reference."""
    fg, binary = _a.assemble_yfcc(flow, param, match, matchBG, th, multiH, device)
    return fg[0].cpu().numpy(), binary[0].cpu().numpy()


def _yfcc_matches_from_flow(flowFine, matchBinary, sizeA, sizeB, angle):
    """evalYFCC/getResults.py:53-71 -> numpy (pts1 (n,2) float32, pts2 (n,2) int64)."""
    return _np(_a.yfcc_matches(flowFine, matchBinary, sizeA, sizeB, angle))


hpatch = types.SimpleNamespace(getFlow_all=_wrap(_a.hpatch_getFlow_all),
                               getFlow_onlyCoarse=_wrap(_a.hpatch_getFlow_onlyCoarse), epe_from_homography=_a.hpatch_epe)
corr = types.SimpleNamespace(getFlow=_wrap(_a.corr_getFlow), getFlow_Coarse=_wrap(_a.corr_getFlow_Coarse),
                             alignmentError=_a.corr_alignment_error, keypoints_records=_a.corr_keypoints_records,
                             precision=_a.corr_precision, aligned_images_records=_a.aligned_images_records,
                             aligned_image=_a.aligned_image)
kitti = types.SimpleNamespace(getFlow_all=_wrap(_kitti_getFlow_all),
                              getFlow_onlyCoarse=_wrap(_a.kitti_getFlow_onlyCoarse), epe=_a.kitti_epe)
yfcc = types.SimpleNamespace(getFlow=_yfcc_getFlow, _getFlow=_yfcc__getFlow, matches_from_flow=_yfcc_matches_from_flow)
# the aligned source images (quick_start/align2images.py:97-98,117 and :25-28,112) of a batch of any driver's records, or of a flow the
# caller holds -- the same two functions whichever protocol the records come from
aligned_images_records, aligned_image = _a.aligned_images_records, _a.aligned_image
