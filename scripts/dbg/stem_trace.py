"""Experiment: per-workgroup phase timing of stem7_conv_maxpool_kernel (library built with `make trace`): s_memtime words per
workgroup (csrc/stem.hip): 0 start | 1 patch in LDS | 2 after the barrier | 3 sum over the channel groups of MFMA phase + tile
stores + barrier | 4 sum of pooling pass + stores + barrier | 5 end | 6 channel groups walked.
Matrix-pipe busy = MFMA cycles of a wave (sub-tiles per wave x 74 MFMAs x 64 cycles, per channel group) / workgroup life x resident
workgroups per CU (--resident, from profiles/r06_kernel_resources.tsv).
usage: RFX_LIB=ransac-flow_amd/librfx_trace.so python scripts/dbg/stem_trace.py [--resident 2]"""
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "ransac-flow_amd"))
import torch
from rfx import _lib, ops, weights
from rfx.ops import ConvPlan, ACT_RELU

ap = argparse.ArgumentParser()
ap.add_argument("--resident", type=int, default=2)
a = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda:0")
sd = weights.resnet50_trunk_sd(0, randomize_bn=True)
plan = ConvPlan(sd["conv1.weight"], {k: sd["bn1." + k] for k in ("weight", "bias", "running_mean", "running_var")}, 2, 3, ACT_RELU, dev)
lib.rfx_debug_trace.argtypes = [ctypes.c_void_p]
for (N, H, W) in ((64, 480, 640), (64, 960, 1280)):
    x = torch.randn(N, 3, H, W, device=dev)
    for _ in range(3):
        ops.stem_conv7_maxpool(x, plan)
    torch.cuda.synchronize()
    trace = torch.zeros(1 << 23, dtype=torch.int64, device=dev)
    lib.rfx_debug_trace(ctypes.c_void_p(trace.data_ptr()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); ops.stem_conv7_maxpool(x, plan); e1.record()
    torch.cuda.synchronize()
    lib.rfx_debug_trace(ctypes.c_void_p(0))
    t = trace.cpu().view(-1, 8)
    t = t[t[:, 5] > 0].double()
    tot = t[:, 5] - t[:, 0]
    groups = t[:, 6].mean()
    phases = [("load+stage", t[:, 2] - t[:, 0]), ("mfma+tile", t[:, 3]), ("pool+store", t[:, 4])]
    print("%dx%dx%d: %d workgroups x %.0f channel groups, event %.3f ms, ticks per workgroup: total %.0f (p90 %.0f)"
          % (N, H, W, t.shape[0], groups, e0.elapsed_time(e1), tot.mean(), tot.quantile(0.9)))
    for nm, d in phases:
        print("   %-12s mean %8.0f  p10 %8.0f  p90 %8.0f  (%.1f %%)" % (nm, d.mean(), d.quantile(0.1), d.quantile(0.9), 100 * d.mean() / tot.mean()))
    # the matrix work of a wave: 3 sub-tile slots x 74 MFMAs x 64 cycles per channel group (ticks taken as shader cycles, as in
    # DESIGN_LOG's round-6 entry, where the figure matched the PMC's)
    mfma_cycles = 3 * 74 * 64 * float(groups)
    print("   MFMA cycles per wave %.0f -> matrix pipe busy %.3f with %d resident workgroups" % (mfma_cycles, a.resident * mfma_cycles / tot.mean(), a.resident))
