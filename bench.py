#!/usr/bin/env python
"""bench.py -- aligned image pairs / s at 480x640 on N MI355X (one process per GPU).

A "step" = one pass of the whole hot path over one batch of synthetic pairs already resident in HBM (raw uint8 images;
the bit-exact LANCZOS pyramid + ToTensor/Normalize run on the device inside the step).  float32 end to end.

Workloads (``--config``; BASELINE.json ``configs``):
  3 (default)   BASELINE config 3 AS WORDED -- the headline: batch of 64 480x640 pairs, each target warped by a seeded random
                homography, evaluation semantics (variant B: minSize 480, 7 scales x2, nA = 13 065, coarseIter 10 000),
                multi-homography loop (maxCoarse 10, maskRegionTh 0.01) with a PredFlowMask per homography
                (evaluation/evalHpatch/evaluation.py:193-243); RANSAC index draw on the device (utils/outil.py:120 on a GPU run).
  qs            batch of 64 480x640 pairs, quick_start semantics (quick_start/align2images.py:53-97): ResNet-50 conv4
                features of the 7-level x1.2 pyramid + target -> mutual NN -> RANSAC (nbIter 1000) -> warp ->
                FeatureExtractor x2 -> 7x7 correlation -> NetFlowCoarse -> flow composition -> final warp (one homography
                per pair; rounds 1-2's headline, now ``extra.quick_start`` of the default run).
  2             ONE 480x640 pair, coarse RANSAC only (nbIter 1000, no fine net): value = 1 / latency.
  4             evalHpatch-shaped stream: 960x720 pairs, minSize 720, 5 scales x2, coarseIter 50 000, multi-H on.
  5             evalKITTI-shaped stream: 1242x376 pairs, coarseSize 800, 3 scales x1.2, coarseIter 50 000, fineSize 650,
                two-resolution fine pass, cycle-checked matchability, cc-filter on the device (evaluation/evalKITTI/evaluation.py).
A plain run sets up, warms up, times ``--steps`` steps (``value`` / ``ms_per_step``), writes the last timed step's outputs if
``--dump-outputs DIR`` is given, and prints the line.  ``--full`` adds everything else the line can carry: the rooflines (for
configs 2 / 3 / 4 a second pass of the same steps under the per-launch events), a quick_start leg (``extra.quick_start``: 10 steps,
own rooflines and parity block), the other exact modes and the fp32-MFMA-only build (config 3), and, on rank 0, the CPU legs below.

N > 1: ``python bench.py --gpus N`` re-launches itself under ``torch.distributed.run`` (one rank per GPU, RCCL); when the
driver launches it that way itself, RANK / LOCAL_RANK / WORLD_SIZE come from the environment.  Every rank aligns its own
shard of the pair stream (pair i -> rank i mod N: weak scaling, no data-path collective) and the per-pair result records
-- nbH | status | rank | H[11] | flowDown8[11] | matchDown8[11], 0.85 MB per 480x640 pair, what
evaluation/evalHpatch/evaluation.py:254-260 saves -- are collected with ONE all_gather per step.

Prints one JSON line on rank 0 (the driver's contract): value = pairs/s over all ranks, plus (``--full``)
  roofline      -- the conv-class kernel instance with the most GPU time (fp32 MFMA bound): algorithmic FLOP per launch /
                   average launch duration, HIP events on the launch stream inside the timed region (ops.Profiler);
  roofline_corr -- the same for the HBM-bound 7x7 correlation kernel, SURVEY 8d algorithmic bytes;
  cpu_baseline  -- the REFERENCE ITSELF on this host's cores (kind "reference": its own classes / functions / loop statement,
                   byte-compiled into oracle/_ref by oracle/make_ref.py so that it exists on the GPU box; "port" =
                   oracle/restate.py only where no reference is present): bounded sample of the SAME workload as ``value``,
                   thread count chosen by a one-pair scan;
  parity        -- oracle/parity_sweep.py over pairs of the timed batch, bounded by a wall-clock budget (pairs not reached
                   are reported): config 3 = every round of the multi-homography loop replayed on the oracle from the
                   device's state + the oracle's own loop end to end ("ev_loop"); extra.quick_start.parity = the oracle end to
                   end on its own homography ("qs").  Child processes: the oracle is the checker, never the thing timed.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))

# the host driver supports only dmabuf IPC: without this RCCL / cross-process tensor sharing fails with
# "hipIpcGetMemHandle: invalid argument" (already exported on the build and GPU boxes; kept for any other launcher)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

PEAK_F32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md (dense fp32 matrix peak)
PEAK_HBM_GBS = 8000.0          # HBM3E spec peak
METRIC = "aligned image-pairs/sec @480×640, 1/2/4/8 MI355X; max-abs flow Δ vs ref"
MULTIH_MATCH_STD = 3.0         # saturating matchability head (random init): the explained-region mask grows, pairs stop at
                               # different homography counts (tests/golden/make_golden.py uses the same value)
T_START = time.perf_counter()
FORCE_DIST = os.environ.get("RFX_BENCH_FORCE_DIST") == "1"


def log(msg):
    sys.stderr.write("[bench %7.1fs] %s\n" % (time.perf_counter() - T_START, msg))
    sys.stderr.flush()


def cpu_threads():
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(1, min(avail, os.cpu_count() or 1, 64))


# ------------------------------------------------------------------------------------------------ CPU legs (children)


def cpu_baseline_subprocess(args):
    """The CPU leg in a child process with a hard wall-clock limit so that it can never stall the bench."""
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--config", args.config, "--height", str(args.height),
           "--width", str(args.width), "--nb-scale", str(args.nb_scale), "--nb-iter", str(args.nb_iter), "--cpu-pairs", str(args.cpu_pairs)]
    have_ref = os.path.isdir(os.path.join(ROOT, "oracle", "_ref")) or os.path.isdir("/root/reference/utils")
    fail = {"value": None, "unit": "pairs/s", "cores": cpu_threads(), "kind": "reference" if have_ref else "port",
            "kind_note": "the leg failed: kind = what WOULD have run (oracle/_ref or /root/reference present: %s)" % have_ref}
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        for ln in out.stdout.splitlines():
            if ln.startswith("{"):
                return json.loads(ln)
        return dict(fail, sample="cpu leg failed: " + out.stderr[-300:])
    except subprocess.TimeoutExpired:
        return dict(fail, sample="cpu leg exceeded its 300 s limit")


def cpu_baseline(args):
    """Bounded CPU sample of the SAME workload as ``value`` on this host's cores.  kind = "reference": the reference itself
    (oracle/ref_oracle.py: its CoarseAlign class, its outil.RANSAC, its nn.Modules, its PredFlowMask and its multi-homography
    ``while`` statement, loaded from /root/reference or from the byte-compiled oracle/_ref that travels to the GPU box);
    kind = "port" (oracle/restate.py) only where neither exists.  The thread count is chosen by a short scan (one pair each at
    8 / 16 / 32 / 64 threads, as many as the box has): oneDNN's small convolutions do not scale to every core of a 2-socket host."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import torch
    import parity_sweep
    from rfx import synth, weights
    O = parity_sweep.oracle_backend()
    kind = "reference" if hasattr(O, "KIND") else "port"
    H, W = args.height, args.width
    if args.config == "3":
        sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
                   match=weights.net_matchability_sd(3, last_std=MULTIH_MATCH_STD))
        ca = O.CoarseAlignOracle(sds["trunk"], 7, 10000, 0.05, min(H, W), 2.0, variant="B")
        nets = dict(feat=sds["feat"], flow=sds["flow"], match=sds["match"])
        nh = []

        def one(seed):
            I1, I2 = synth.make_pair(H, W, seed=seed, homography=True)
            ca.setPair(I1, I2)
            nh.append(len(O.multi_h_loop(ca, nets, max_coarse=10, mask_region_th=0.01)["H"]))
        what = ("BASELINE config 3 as worded (variant B CoarseAlign.setPair, 7 scales x2, coarseIter 10 000, the multi-homography "
                "loop of evaluation/evalHpatch/evaluation.py:211-243 with a PredFlowMask per homography)")
    else:
        sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2))
        ca = O.CoarseAlignOracle(sds["trunk"], args.nb_scale, args.nb_iter, 0.05, max(H, W), 1.2, variant="A")
        nets = dict(feat=sds["feat"], flow=sds["flow"])
        nh = None

        def one(seed):
            I1, I2 = synth.make_pair(H, W, seed=seed)
            ca.setSource(I1)
            ca.setTarget(I2)
            r = ca.getCoarse(np.zeros((ca.It.size[1], ca.It.size[0])))
            with torch.no_grad():
                fc = O.warp_grid(torch.from_numpy(r["H"])[None], ca.It.size[1], ca.It.size[0])
                O.fine_step_quickstart(nets, ca.IsTensor, ca.ItTensor, fc)
        what = "full coarse+fine quick_start path (quick_start/align2images.py:53-97)"

    avail = cpu_threads()
    cand = sorted({t for t in (8, 16, 32, 64) if t <= avail} | ({avail} if avail < 8 else set()))
    torch.set_num_threads(cand[0])
    t0 = time.perf_counter()
    one(1000)  # warm-up (oneDNN primitive caches, lazy imports)
    warm = time.perf_counter() - t0
    scan = {}
    for t in cand:
        torch.set_num_threads(t)
        t0 = time.perf_counter()
        one(1500)
        scan[t] = round(time.perf_counter() - t0, 2)
        if warm > 30:
            break
    fastest = min(scan.values())
    best = min(t for t, v in scan.items() if v <= 1.05 * fastest)       # one-pair timings are noisy: the smallest count within 5 % of the best
    torch.set_num_threads(best)
    if nh:
        nh.clear()
    t0 = time.perf_counter()
    n = 0
    while n < args.cpu_pairs:
        one(2000 + n)
        n += 1
        if time.perf_counter() - t0 > 25 or (n == 1 and warm > 30):
            break
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "pairs/s", "cores": best, "kind": kind, "oracle": parity_sweep.oracle_name(O),
            "threads_scan_s_per_pair": {str(k): v for k, v in scan.items()}, "host_logical_cpus": os.cpu_count(),
            "sample": "%d synthetic %dx%d pairs, %s, executed by %s on %d threads (best of a one-pair scan over %s threads)"
                      "%s, %.1f s" % (n, H, W, what, parity_sweep.oracle_name(O), best, "/".join(str(c) for c in cand),
                                      (", %.1f homographies per pair" % (sum(nh) / len(nh))) if nh else "", dt)}


def parity_subprocess(cfg, dump_dir, seeds, H, W, budget, stability=False):
    """oracle/parity_sweep.py over the dumped GPU results (child process; bounded).  ``stability``: the reference against ITSELF
    under a second CPU execution setting (8 threads + oneDNN vs 1 thread without oneDNN) on the same seeds -- the flip rate two
    executions of the reference show against each other, reported next to the device's."""
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "parity_sweep.py"), "--config", cfg, "--height",
           str(H), "--width", str(W), "--budget", str(budget)] + (["--stability", "--threads", "8"] if stability else ["--dump", dump_dir])
    cmd += ["--seeds"] + [str(s) for s in seeds]
    if os.environ.get("RFX_PARITY_RECORDS"):        # per-pair records for profiles/ (evidence scripts)
        cmd += ["--records", os.environ["RFX_PARITY_RECORDS"] + "_" + cfg + os.environ.get("RFX_PARITY_RECORDS_SUFFIX", "") + ".json"]
    env = dict(os.environ, OMP_WAIT_POLICY="PASSIVE", GOMP_SPINCOUNT="0")     # many oracle workers side by side: no spin-waiting
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=budget + 120, env=env)
        for ln in reversed(out.stdout.splitlines()):
            if ln.startswith("{"):
                return json.loads(ln)
        return {"error": "parity sweep failed: " + out.stderr[-400:]}
    except subprocess.TimeoutExpired:
        return {"error": "parity sweep exceeded its limit"}


# ------------------------------------------------------------------------------------------------ launch


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="3", choices=["qs", "2", "3", "4", "5"])
    ap.add_argument("--batch", type=int, default=None, help="pairs per step per GPU (default: 64 for qs / 3, 1 for 2, 16 for 4, 8 for 5)")
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--nb-scale", type=int, default=7)
    ap.add_argument("--nb-iter", type=int, default=1000)
    ap.add_argument("--multi-h", action="store_true", help="alias of --config 3")
    ap.add_argument("--cpu-pairs", type=int, default=6)
    ap.add_argument("--host-draw", action="store_true", help="RANSAC index draw with torch.randint on the CPU generator (what a "
                    "CPU run of the reference draws) instead of on the device")
    ap.add_argument("--degenerate", default="lapack", choices=["auto", "device", "lapack"],
                    help="rank-deficient 4-point samples (AlignPipeline): lapack (the timed default since round 6) = the EXACT mode: re-solved "
                         "by the host's LAPACK (librfxhost.so: numpy's own dgesdd on std::threads) like the reference does for every sample; "
                         "device = the device's own null vector (no host round trip; rounds 3-5's timed mode); auto = lapack with host draws, "
                         "device with device draws")
    ap.add_argument("--split", type=int, default=None,
                    help="lock-step groups of the multi-homography driver (AlignPipeline.multi_h_batched split=): default = the pipeline's "
                         "rule (2 groups on 2 streams for device draws)")
    ap.add_argument("--score-chunk", default="host",
                    help="how the mutual-NN scores are summed (ops.resolve_score_chunk): 'host' (default here: the K blocking of this host's "
                         "sgemm, probed ONCE on rank 0 before the workload is built and broadcast -- the parity legs compare with this host's "
                         "CPU run of the reference), 'default' (fixed 256 products) or a number of products per chunk")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: rooflines (configs 2 / 3 / 4: a second, profiled pass of the same steps), "
                         "the quick_start / exact-mode / fp32-MFMA-only legs (config 3, N = 1), the CPU baseline and the parity sweeps; "
                         "a plain run only times the steps")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0: write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64): "
                         "records.npy = the gathered per-pair record block, pair_ids.npy = the pair of every row; a fixed, seeded sample "
                         "of the rows where the block exceeds 64 MB")
    ap.add_argument("--no-exact-leg", action="store_true", help="--full run: skip extra.exact_mode (throughput of the exact modes)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full run: skip the CPU legs (cpu_baseline + parity sweep)")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--parity-pairs", type=int, default=None, help="pairs of the batch covered by the parity sweep (default: all)")
    ap.add_argument("--parity-budget", type=float, default=95.0, help="wall-clock bound of the headline's parity sweep, seconds")
    ap.add_argument("--timed-parity-budget", type=float, default=85.0,
                    help="wall-clock bound of the sweep over the TIMED mode (device draws replayed on the reference), seconds")
    ap.add_argument("--qs-parity-budget", type=float, default=50.0, help="wall-clock bound of the quick_start leg's parity sweep")
    ap.add_argument("--stability-budget", type=float, default=55.0, help="wall-clock bound of the reference-vs-reference sweep")
    ap.add_argument("--no-qs-leg", "--no-config3-leg", dest="no_qs_leg", action="store_true",
                    help="--full run: skip the quick_start leg (extra.quick_start)")
    ap.add_argument("--host-prep", action="store_true",
                    help="build the LANCZOS pyramid with PIL on the host before the timed region (default: raw uint8 images "
                         "resident in HBM, pyramid + ToTensor + Normalize on the device inside the timed step)")
    ap.add_argument("--pcie", action="store_true",
                    help="PCIe-inclusive variant (configs qs / 3 / 4; never the headline): the raw uint8 images start in pinned HOST "
                         "memory and are uploaded inside every timed step, and the step ends with the result records copied back to "
                         "pinned host memory")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher rehearsal WITHOUT a GPU: the real rank code (self-spawn, process group, barriers, all_gather, "
                         "max-over-ranks timing, JSON) around a CPU stand-in step that fabricates records; value is meaningless")
    ap.add_argument("--single-stream", action="store_true",
                    help="profiling runs (rocprofv3 --kernel-trace / --pmc): ONE lock-step group and ONE trunk stream, one timed pass under "
                         "the per-launch events -- no kernel overlaps another, so rocprofv3's per-kernel durations are the ones the "
                         "rooflines are computed from (the product path overlaps kernels of different streams, which stretches every "
                         "overlapped kernel's begin-to-end time)")
    ap.add_argument("--dump-records", default=None,
                    help="rank 0: torch.save the last step's gathered record block + the absolute pair id of every row (N-rank vs 1-rank "
                         "equality checks: a pair's record does not depend on the sharding)")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.multi_h:
        args.config = "3"
    dflt = {"qs": (480, 640, 64), "2": (480, 640, 1), "3": (480, 640, 64), "4": (720, 960, 16), "5": (376, 1242, 8)}[args.config]
    args.height = args.height or dflt[0]
    args.width = args.width or dflt[1]
    args.batch = args.batch or dflt[2]
    if args.single_stream:
        args.split = 1
        os.environ["RFX_TRUNK_STREAMS"] = "1"
    return args


def self_spawn(args):
    """``python bench.py --gpus N`` (N > 1) outside any launcher: re-exec under torch.distributed.run, one rank per GPU."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("--gpus %d without WORLD_SIZE: launching %d ranks via torch.distributed.run (port %d)" % (args.gpus, args.gpus, port))
    sys.exit(subprocess.call(cmd))


def preflight(dist, backend, rank, world, dev):
    """Process-group bring-up with a diagnosis instead of a hang: init (RCCL: eager communicator on this rank's GPU) -> a 1 MB
    ``all_gather_into_tensor`` whose content is checked -> barrier, all under a 60 s limit BEFORE the workload is built.  On
    failure every rank prints one line (visible devices, HSA_ENABLE_IPC_MODE_LEGACY, RCCL version, rendezvous) and re-raises."""
    import datetime
    import torch
    t0 = time.perf_counter()
    stage = "init_process_group"
    try:
        kw = dict(backend=backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=int(os.environ.get("RFX_PREFLIGHT_TIMEOUT", "60"))))
        if backend == "nccl":
            kw["device_id"] = dev
        dist.init_process_group(**kw)
        stage = "all_gather_into_tensor (1 MB)"
        n = 262144
        mine = torch.full((n,), float(rank), dtype=torch.float32, device=dev if backend == "nccl" else None)
        allr = torch.empty((world * n,), dtype=torch.float32, device=mine.device)
        dist.all_gather_into_tensor(allr, mine)
        stage = "barrier"
        dist.barrier()
        if dev is not None:
            torch.cuda.synchronize()
        got = allr.view(world, n)[:, 0].tolist()
        if got != [float(r) for r in range(world)]:
            raise RuntimeError("all_gather returned ranks %s" % got)
        log("preflight ok: %s, %d rank(s), 1 MB all_gather + barrier in %.2f s" % (backend, world, time.perf_counter() - t0))
    except Exception as e:  # noqa: BLE001 -- diagnose, then fail
        try:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else "-"
        except Exception:  # noqa: BLE001
            ver = "?"
        sys.stderr.write("[bench preflight FAILED] rank %d/%d at %s after %.1f s: %s: %s | backend=%s rccl=%s visible_devices=%d "
                         "HIP_VISIBLE_DEVICES=%s ROCR_VISIBLE_DEVICES=%s HSA_ENABLE_IPC_MODE_LEGACY=%s MASTER=%s:%s device=%s\n"
                         % (rank, world, stage, time.perf_counter() - t0, type(e).__name__, str(e)[:300], backend, ver,
                            torch.cuda.device_count() if torch.cuda.is_available() else 0, os.environ.get("HIP_VISIBLE_DEVICES"),
                            os.environ.get("ROCR_VISIBLE_DEVICES"), os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
                            os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"), dev))
        sys.stderr.flush()
        raise


# ------------------------------------------------------------------------------------------------ workloads


def _pinned(raw):
    """--pcie: the step's input as the boundary hands it over -- raw uint8 images in pinned host memory."""
    return tuple(t.cpu().pin_memory() for t in raw)


def _upload(raw_h, dev):
    return tuple(t.to(dev, non_blocking=True) for t in raw_h)


def _download(rec, keep):
    """--pcie: the records back in pinned host memory (asynchronous copy on the step's stream; the timed region ends with a
    synchronize).  The device tensor is returned for the gather."""
    if "buf" not in keep or keep["buf"].shape != rec.shape:
        import torch
        keep["buf"] = torch.empty(rec.shape, dtype=rec.dtype).pin_memory()
    keep["buf"].copy_(rec, non_blocking=True)
    return rec


def build_workload(args, dev, rank, world, score_chunk=None):
    """Returns (step() -> (B, width) float32 record tensor on ``dev``, meta dict, extras for the parity leg).  Record columns:
    meta["col"] = dict(status=..., nbh=... or None, rank=...)."""
    import torch
    from rfx import weights, synth, ops
    from rfx.pipeline import AlignPipeline
    from rfx import dist as rdist
    H, W, B, cfg = args.height, args.width, args.batch, args.config
    draw = "host" if args.host_draw else "device"
    pkw = dict(device=dev, draw=draw, seed=1000, degenerate=args.degenerate, score_chunk=score_chunk)
    draw_txt = ("RANSAC index draw: Philox on the device from the device-side match counts, keyed by (seed, absolute pair id, round)" if draw == "device" else
                "RANSAC index draw: torch.randint on the CPU generator per pair and homography")
    sds = dict(trunk=weights.resnet50_trunk_sd(0), feat=weights.feature_extractor_sd(1), flow=weights.net_flow_coarse_sd(2),
               match=weights.net_matchability_sd(3))
    seeds = [rank + world * i for i in range(B)]        # this rank's shard of the synthetic stream: pair i -> rank i mod world
    if cfg in ("qs", "2"):
        pipe = AlignPipeline(sds, nbScale=args.nb_scale, nbIter=args.nb_iter, tolerance=0.05, minSize=max(H, W), scaleR=1.2,
                             variant="A", **pkw)
        pairs = [synth.make_pair(H, W, seed=s) for s in seeds]
        raw = pipe.upload_raw(pairs)
        prep0 = pipe.prepare(pairs) if args.host_prep else None
        fine = cfg == "qs"

        raw_h, rec_h = _pinned(raw) if args.pcie else None, {}

        def step():
            r = _upload(raw_h, dev) if raw_h is not None else raw
            p, feats = (prep0, None) if prep0 is not None else pipe.prepare_and_features(*r)
            res = pipe.align_prepared(p, fine=fine, feats=feats, pair_ids=seeds)
            rec = rdist.pack_records(res, rank=rank) if fine else _coarse_records(res, dev, rank)
            return _download(rec, rec_h) if raw_h is not None else rec
        if fine:
            wl = ("batch of %d %dx%d pairs per GPU per step, full pipeline: ResNet-50 conv4 feat x%d scales + mutual NN + RANSAC("
                  "nbIter=%d, 4-pt DLT) + FeatureExtractor + 7x7 corr + NetFlowCoarse + grid_sample (quick_start semantics, one "
                  "homography per pair: quick_start/align2images.py at the metric's 480x640); %s" % (B, H, W, args.nb_scale, args.nb_iter, draw_txt))
        else:
            wl = ("BASELINE config 2: ONE %dx%d pair per step, coarse RANSAC only (ResNet-50 conv4 feat x%d scales + mutual NN + "
                  "RANSAC nbIter=%d, no fine net): value = 1 / latency; %s" % (H, W, args.nb_scale, args.nb_iter, draw_txt))
        col = dict(status=9, nbh=None, rank=-1 if fine else 10)
        return step, dict(workload=wl, nbIter=args.nb_iter, nbScale=args.nb_scale, col=col), dict(pipe=pipe, seeds=seeds)
    sds["match"] = weights.net_matchability_sd(3, last_std=MULTIH_MATCH_STD)
    col = dict(status=1, nbh=0, rank=2)
    if cfg in ("3", "4"):
        nbScale, nbIter = (7, 10000) if cfg == "3" else (5, 50000)
        pipe = AlignPipeline(sds, nbScale=nbScale, nbIter=nbIter, tolerance=0.05, minSize=min(H, W), scaleR=2.0, variant="B", **pkw)
        raw = pipe.upload_raw([synth.make_pair(H, W, seed=s, homography=True) for s in seeds])

        raw_h, rec_h = _pinned(raw) if args.pcie else None, {}

        def step():
            prep = pipe.prepare_device(*(_upload(raw_h, dev) if raw_h is not None else raw))
            R = ops.MultiHRecords(B, prep["ItTensor"].shape[2] // 8, prep["ItTensor"].shape[3] // 8, dev, max_h=11)
            R.rec[:, 2] = float(rank)
            pipe.multi_h_batched(prep, maxCoarse=10, maskRegionTh=0.01, records=R, want_lists=False, pair_ids=seeds, split=args.split)
            return _download(R.rec, rec_h) if raw_h is not None else R.rec
        wl = ("BASELINE config %s as worded: batch of %d %dx%d pairs per GPU per step, each target warped by a seeded random "
              "homography; evaluation semantics (variant B, minSize %d, %d scales x2, coarseIter %d) + multi-homography loop "
              "(maxCoarse 10, maskRegionTh 0.01, lock-step over the batch, device-resident rounds) with FeatureExtractor + 7x7 corr "
              "(both directions from one pass) + NetFlowCoarse + NetMatchability x2 + flow composition per homography; %s; per-pair "
              "result record = nbH | H[11] | flowDown8[11] | matchDown8[11] (evaluation/evalHpatch/evaluation.py:254-260)"
              % (cfg, B, H, W, min(H, W), nbScale, nbIter, draw_txt))
        return step, dict(workload=wl, nbIter=nbIter, nbScale=nbScale, matchability_init_std=MULTIH_MATCH_STD, col=col), dict(pipe=pipe, seeds=seeds)
    # config 5: KITTI-shaped stream, two-resolution driver
    pipe = AlignPipeline(sds, nbScale=3, nbIter=50000, tolerance=0.05, minSize=800, scaleR=1.2, variant="B", **pkw)
    raws = [pipe.upload_raw([synth.make_pair(H, W, seed=s, homography=True, amp=0.02)]) for s in seeds]

    raw_all = (torch.cat([r[0] for r in raws]), torch.cat([r[1] for r in raws]))
    w_r, h_r = pipe.resize_img_dims(W, H, 8, 650)
    w_d2, h_d2 = pipe.resize_img_dims(W, H, 8, 325)

    def step():
        R = ops.MultiHRecords(B, h_r // 8, w_r // 8, dev, max_h=11, hd2=h_d2 // 8, wd2=w_d2 // 8)
        R.rec[:, 2] = float(rank)
        pipe.multi_h_kitti_batched(raw_all[0], raw_all[1], fineSize=650, maskRegionTh=0.005, cc_th=0.01, records=R, want_lists=False,
                                   pair_ids=seeds, split=args.split)
        return R.rec
    wl = ("BASELINE config 5: %d evalKITTI-shaped %dx%d pairs per GPU per step (coarseSize 800 -> 2640x800 target, 3 scales "
          "x1.2, nA = 25 747, coarseIter 50 000; fineSize 650: two-resolution fine pass, cycle-checked matchability, "
          "cc-filter 0.01 (device union-find labelling), maskRegionTh 0.005), lock-step driver over the batch, device-resident rounds; %s; "
          "per-pair result record = nbH | H[11] | flowDown8[11] | matchDown8[11] | flowD2[11]" % (B, W, H, draw_txt))
    return step, dict(workload=wl, nbIter=50000, nbScale=3, matchability_init_std=MULTIH_MATCH_STD, col=col), dict(pipe=pipe, seeds=seeds)


def _coarse_records(res, dev, rank=0):
    """[H (9) | status | rank] per pair (BASELINE config 2: coarse stage only)."""
    import torch
    rec = torch.zeros((len(res), 11), dtype=torch.float32, device=dev)
    rec[:, 10] = float(rank)
    for b, r in enumerate(res):
        if r["H"] is not None:
            rec[b, :9] = r["H"].reshape(9)
        else:
            rec[b, 9] = 1.0
    return rec


def dry_run_step(args, rank):
    """CPU stand-in for --dry-run: deterministic fake records (rank-tagged) -- exercises everything around the kernels."""
    import torch

    def step():
        rec = torch.zeros((args.batch, 10), dtype=torch.float32)
        rec[:, 0] = float(rank)
        rec[:, 1] = torch.arange(args.batch, dtype=torch.float32)
        time.sleep(0.01)
        return rec
    return step


# ------------------------------------------------------------------------------------------------ timing + rooflines


def timed_loop(step, args, dist, sync, prof_factory):
    """W untimed warm-up steps, then EXACTLY K steps bracketed by barrier + device synchronise on both sides."""
    from rfx import dist as rdist
    for i in range(args.warmup):
        step()
        sync()
        log("warmup step %d done" % i)
    sync()
    if dist is not None:
        dist.barrier()
    sync()
    with prof_factory() as prof:
        t0 = time.perf_counter()
        # ONE all_gather per step (identity when world == 1), overlapped: the collective of step k is in flight while step k+1
        # computes, and is waited for when step k+1 hands in its own records; the last one is flushed INSIDE the timed region
        pg = rdist.PipelinedGather(dist, force=FORCE_DIST)
        for _ in range(args.steps):
            pg.push(step())
        out = pg.flush()
        sync()
        if dist is not None:
            dist.barrier()
        sync()
        elapsed = time.perf_counter() - t0
    return elapsed, out, prof


SPLIT_PRODUCTS = 6            # bf16 MFMA products per float32 product in the split kernels (csrc/conv1x1s.hip, conv3x3s.hip)
PEAK_BF16_MFMA_TFLOPS = 2500.0   # dense bf16 matrix peak (MI355X_MICROARCH.md)


def is_split(kid):
    return bool(kid & (32768 | 65536))


def kernel_name(kid):
    tf = lambda b: "true" if b else "false"
    if kid & 65536:        # float32 3x3 on the bf16 matrix cores by exact operand splitting (conv3x3s.hip)
        # <TM, true>: the weight images by LDS-DMA (the default; RFX_C3S_ADMA=0 runs <TM, false>)
        return "conv3x3_split_s2_kernel" if kid & 4 else "conv3x3_split_kernel<%d, %s>" % (
            1 if kid & 1 else 2, "false" if os.environ.get("RFX_C3S_ADMA", "1") == "0" else "true")
    if kid & 32768:        # ... 1x1 (conv1x1s.hip); 4: strided pixels (the projection shortcuts)
        return "conv1x1_split_kernel<%d>" % (1 if kid & 1 else 2)
    if kid & (32 | 512):   # direct 3x3 kernel; 512 = fused with the 1x1 expansion (Bottleneck tail); 16384 = chunked accumulation (KCH = 4)
        return "conv3x3_direct_kernel<%d, %d, %s, %d, %s, %d>" % (1 if kid & 3 else 2, 4 if kid & 128 else (8 if kid & 64 else 16), tf(kid & 512),
                                                                   4 if kid & 2048 else 2, tf(kid & 4096), 4 if kid & 16384 else 0)
    if kid & 8192:         # direct 3x3 / stride 2 kernel; 16384 = chunked accumulation (KCH = 4, K >= 1152)
        return "conv3x3_s2_kernel<%d, %d>" % (1 if kid & 1 else 2, 4 if kid & 16384 else 0)
    if kid & 1024:         # k-major 1x1 kernel (conv1x1.hip); 16384 = chunked accumulation (KCH = 8)
        return "conv1x1_kmajor_kernel<%d, %s, %d>" % (1 if kid & 3 else 2, tf(kid & 16), 8 if kid & 16384 else 0)
    if kid == 256:
        return "stem_conv_maxblur_kernel"
    if kid == 257:
        return "stem7_conv_maxpool_kernel"
    return "conv2d_mfma_kernel<%s, %s, %s, %s>" % ({0: "2, 2", 1: "1, 2", 2: "1, 1"}[kid & 3], tf(kid & 4), tf(kid & 8), tf(kid & 16))


def pmc_traffic(kernel, cfg):
    """HBM-side bytes per launch of ``kernel`` from the committed PMC summary of the SAME bench command (separate rocprofv3 --pmc
    passes: FETCH_SIZE and WRITE_SIZE cannot share a pass and rocprofv3 cannot wrap the process that is being timed), corrected as
    MI355X_MICROARCH.md prescribes for gfx950 (FETCH_SIZE counts 16-byte/lane reads at half: doubled; WRITE_SIZE raw).  None when
    the summary or the kernel is missing."""
    ks = None
    for rnd in ("r06", "r05", "r04"):     # the newest committed summary of this command
        path = os.path.join(ROOT, "profiles", "%s_pmc_summary_config%s.json" % (rnd, cfg))
        try:
            ks = json.load(open(path))["kernels"]
            break
        except (OSError, ValueError, KeyError):
            continue
    if ks is None:
        return None, None
    norm = lambda t: t.replace(" ", "")
    for name, o in ks.items():
        if norm(name).startswith(norm(kernel)) and "fetch_bytes_per_launch_corrected" in o and "write_size_bytes_per_launch_raw" in o:
            return o["fetch_bytes_per_launch_corrected"] + o["write_size_bytes_per_launch_raw"], os.path.relpath(path, ROOT)
    return None, None


def rooflines(prof, elapsed, rank, cfg="3", dev=None):
    by = {}
    for (v, f, e0, e1, _, nb) in prof.conv:
        g = by.setdefault(v, [0, 0.0, 0.0, 0.0])
        g[0] += 1; g[1] += f; g[2] += e0.elapsed_time(e1) * 1e-3; g[3] += nb
    if os.environ.get("RFX_BENCH_DUMP") and rank == 0:
        agg = {}
        for (v, f, e0, e1, shp, _) in prof.conv:
            a = agg.setdefault((v,) + shp, [0, 0.0, 0.0])
            a[0] += 1; a[1] += f; a[2] += e0.elapsed_time(e1) * 1e-3
        rows = sorted(((k, c, f, t) for k, (c, f, t) in agg.items()), key=lambda r: -r[3])
        def workgroups(key):
            """Workgroups of one launch where the grid is the tile count (the direct 3x3 kernels: kernel-id bit 5; patch shape from
            bits 6-7 / 11, 128-channel tiles unless bits 0-1 say 64); the k-major 1x1 kernel is persistent (512 workgroups)."""
            kid, N, Cin, H, W, Cout, kk, stride = key
            if kid & 1024:
                return 512
            if not (kid & 32) or (kid & 512):
                return None
            ph, pw = (16, 16) if kid & 2048 else {0: (8, 16), 1: (16, 8), 2: (32, 4)}[(kid >> 6) & 3]
            bm = 64 if (kid & 3) else 128
            return N * -(-H // ph) * -(-W // pw) * -(-Cout // bm)
        with open(os.environ["RFX_BENCH_DUMP"], "w") as fh:
            fh.write("# per kernel instance and shape over the profiled pass (one stream): N = images of the launch (64 = a full round or a trunk "
                     "level, smaller = a shrinking multi-homography round); workgroups per launch and their remainder over the 512 resident "
                     "slots (256 CUs x 2) where the grid is the tile count\n")
            fh.write("variant,kernel,N,Cin,H,W,Cout,k,stride,calls,total_ms,TFLOPs,share,workgroups,waves_of_512,last_wave_fill\n")
            tot = sum(r[3] for r in rows)
            for k, c, f, t in rows:
                wg = workgroups(k)
                extra = ",,," if wg is None else ",%d,%.2f,%.2f" % (wg, wg / 512.0, (wg % 512) / 512.0 if wg % 512 else 1.0)
                fh.write("%d,\"%s\"," % (k[0], kernel_name(k[0])) + ",".join(str(x) for x in k[1:]) + ",%d,%.3f,%.1f,%.3f%s\n"
                         % (c, t * 1e3, f / t / 1e12, t / tot, extra))
    dom = max(by, key=lambda k: by[k][2])           # the kernel instance with the most GPU time
    n, f, t, b = by[dom]
    tot_f, tot_t = sum(g[1] for g in by.values()), sum(g[2] for g in by.values())
    ach = f / t / 1e12
    # peak of the dominant kernel: an fp32-MFMA kernel is bounded by the fp32 matrix peak; a split kernel executes SPLIT_PRODUCTS bf16
    # products per float32 product on the bf16 matrix cores, so ITS ceiling in algorithmic (float32) FLOP/s is the dense bf16 peak / 6
    peak = PEAK_BF16_MFMA_TFLOPS / SPLIT_PRODUCTS if is_split(dom) else PEAK_F32_MFMA_TFLOPS
    roof = {"kernel": kernel_name(dom), "bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(ach / peak, 4), "traffic": None,
            "traffic_note": "not measured inside the bench (rocprofv3 cannot wrap itself): the per-launch FETCH_SIZE / WRITE_SIZE "
                            "of this kernel from separate --pmc passes of this command are committed in profiles/ (static)",
            "launches": n, "avg_launch_us": round(t / n * 1e6, 2), "flop_per_launch": f / n, "algorithmic_bytes_per_launch": round(b / n),
            "time_share": round(t / elapsed, 3), "all_conv_tflops": round(tot_f / tot_t / 1e12, 2), "conv_time_share": round(tot_t / elapsed, 3),
            "conv_kernels": {("%d" % k): {"launches": g[0], "tflops": round(g[1] / g[2] / 1e12, 1), "time_share": round(g[2] / elapsed, 3)}
                             for k, g in sorted(by.items())}}
    if is_split(dom):
        roof["peak_note"] = ("algorithmic float32 FLOP/s; the kernel computes every float32 product as %d exact bf16 x bf16 products on the bf16 "
                             "matrix cores (float32 = hi + mid + lo bf16 pieces, csrc/conv3x3s.hip), so its ceiling is the dense bf16 peak "
                             "%.0f / %d = %.1f TFLOP/s; executed bf16 matrix FLOP/s = %d x achieved; against the fp32 matrix peak (%.1f TFLOP/s, "
                             "the bound of the fp32-MFMA kernel it replaced at 0.80) it stands at %.2f"
                             % (SPLIT_PRODUCTS, PEAK_BF16_MFMA_TFLOPS, SPLIT_PRODUCTS, peak, SPLIT_PRODUCTS, PEAK_F32_MFMA_TFLOPS,
                                ach / PEAK_F32_MFMA_TFLOPS))
        roof["executed_bf16_tflops"] = round(ach * SPLIT_PRODUCTS, 1)
        roof["vs_fp32_mfma_peak"] = round(ach / PEAK_F32_MFMA_TFLOPS, 4)
    tr, src = pmc_traffic(roof["kernel"], cfg)
    if tr is not None:
        roof["traffic"] = round(tr)
        roof["traffic_unit"] = "bytes per launch"
        roof["traffic_note"] = ("FETCH_SIZE (x2: gfx950 counts 16-byte/lane reads at half) + WRITE_SIZE of this kernel, averaged per launch over "
                                "separate rocprofv3 --pmc passes of this bench command (%s): static evidence, not this process; "
                                "algorithmic bytes per launch (input + output + weights once) = %d" % (src, round(b / n)))
    corr = None
    if prof.corr:
        cb = sum(x[0] for x in prof.corr) / len(prof.corr)
        cd = sum(e0.elapsed_time(e1) * 1e-3 for _, e0, e1 in prof.corr) / len(prof.corr)
        corr = {"kernel": "corr7_dma_kernel", "bound": "hbm", "achieved": round(cb / cd / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": round(cb / cd / 1e9 / PEAK_HBM_GBS, 4), "traffic": None, "bytes_per_launch": cb, "launches": len(prof.corr),
                "avg_launch_us": round(cd * 1e6, 2),
                "traffic_note": "PMC per-launch traffic of this kernel: profiles/ (static, separate --pmc passes)"}
        kus = prof.corr_durations()[0] if hasattr(prof, "corr_durations") else []
        if len(kus) == len(prof.corr):
            # `achieved` / `frac` by KERNEL duration: the start / stop events hipExtLaunchKernelGGL attaches to the dispatch itself
            # (rfx_corr_timing; the timestamps rocprofv3 reads), same launches, same timed region.  The interval between two events
            # recorded AROUND a launch (event_interval_us) also brackets ~18 us of command-processor work per 150 us kernel.
            kd = sum(kus) / len(kus) * 1e-6
            corr.update(event_interval_us=corr["avg_launch_us"], frac_by_event_interval=corr["frac"], achieved=round(cb / kd / 1e9, 1),
                        frac=round(cb / kd / 1e9 / PEAK_HBM_GBS, 4), avg_launch_us=round(kd * 1e6, 2),
                        duration_source="dispatch-level start/stop events of every launch of the timed region (hipExtLaunchKernelGGL, "
                                        "rfx_corr_timing): the kernel's own duration, as rocprofv3 --kernel-trace reports it")
        trc, srcc = pmc_traffic("corr7_dma_kernel", "qs" if cfg == "qs" else cfg)
        if trc is not None and cfg == "qs":
            corr["traffic"] = round(trc)
            corr["traffic_note"] = "FETCH_SIZE x2 + WRITE_SIZE per launch, separate --pmc passes of this command (%s)" % srcc
    if getattr(prof, "corr_bidir", None):
        # both directions of a pair in ONE launch (evaluation semantics): `achieved` is priced on the bytes that launch must
        # move at minimum -- (2C + 2*49)*4 per pixel: x and y read once, two volumes written -- NOT on twice SURVEY 8d's
        # per-direction figure, which is what the two one-direction launches it replaces would have moved (given below)
        nb = len(prof.corr_bidir)
        mb = sum(x[0] for x in prof.corr_bidir) / nb
        pb = sum(x[1] for x in prof.corr_bidir) / nb
        cd = sum(e0.elapsed_time(e1) * 1e-3 for _, _, e0, e1 in prof.corr_bidir) / nb
        bid = {"kernel": "corr7_dma_kernel, BIDIR epilogue (corr12 and corr21 of a pair from one pass over the features)", "bound": "hbm",
               "achieved": round(mb / cd / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(mb / cd / 1e9 / PEAK_HBM_GBS, 4),
               "traffic": None, "bytes_per_launch": mb, "launches": nb, "avg_launch_us": round(cd * 1e6, 2),
               "per_direction_accounting": {"bytes_per_launch": pb, "achieved": round(pb / cd / 1e9, 1), "frac": round(pb / cd / 1e9 / PEAK_HBM_GBS, 4),
                                            "note": "SURVEY 8d's (2C+49)*4 B per pair-direction x the 2 directions one launch produces"},
               "traffic_note": "PMC per-launch traffic of this kernel: profiles/ (static, separate --pmc passes)"}
        # the rounds of the multi-homography loop shrink the batch (64, 64, ~40, ... active pairs: the late launches are 100-160
        # workgroups on 256 CUs); the launches over the FULL batch separately
        top = max(x[0] for x in prof.corr_bidir)
        full = [x for x in prof.corr_bidir if x[0] == top]
        fd = sum(e0.elapsed_time(e1) * 1e-3 for _, _, e0, e1 in full) / len(full)
        bid["full_batch_launches"] = {"launches": len(full), "bytes_per_launch": top, "avg_launch_us": round(fd * 1e6, 2),
                                      "achieved": round(top / fd / 1e9, 1), "frac": round(top / fd / 1e9 / PEAK_HBM_GBS, 4)}
        kusb = prof.corr_durations()[1] if hasattr(prof, "corr_durations") else []
        if len(kusb) == nb:
            kd = sum(kusb) / nb * 1e-6
            bid.update(event_interval_us=bid["avg_launch_us"], frac_by_event_interval=bid["frac"], achieved=round(mb / kd / 1e9, 1),
                       frac=round(mb / kd / 1e9 / PEAK_HBM_GBS, 4), avg_launch_us=round(kd * 1e6, 2),
                       duration_source="dispatch-level start/stop events (rfx_corr_timing), every launch of the timed region")
            bid["per_direction_accounting"].update(achieved=round(pb / kd / 1e9, 1), frac=round(pb / kd / 1e9 / PEAK_HBM_GBS, 4))
            fk = [u for u, x in zip(kusb, prof.corr_bidir) if x[0] == top]
            fkd = sum(fk) / len(fk) * 1e-6
            bid["full_batch_launches"].update(event_interval_us=bid["full_batch_launches"]["avg_launch_us"],
                                              frac_by_event_interval=bid["full_batch_launches"]["frac"], avg_launch_us=round(fkd * 1e6, 2),
                                              achieved=round(top / fkd / 1e9, 1), frac=round(top / fkd / 1e9 / PEAK_HBM_GBS, 4))
        if corr is None:
            corr = bid
        else:
            corr["bidir"] = bid
    return roof, corr


def dump_outputs(d, rec, pair_ids, limit=64 * 10 ** 6 - 4096):
    """--dump-outputs: the last timed step's gathered record block as ``d/records.npy`` (float32) and the pair id of every row as
    ``d/pair_ids.npy`` (float64).  A block over ``limit`` bytes keeps a fixed, seeded sample of its rows (in order)."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    rec = rec.detach().float().cpu().numpy()
    ids = np.asarray(pair_ids, dtype=np.float64)
    rows = np.arange(rec.shape[0])
    per_row = rec.shape[1] * 4 + 8
    if rec.shape[0] * per_row > limit:
        rows = np.sort(np.random.default_rng(0).choice(rec.shape[0], max(1, limit // per_row), replace=False))
    np.save(os.path.join(d, "records.npy"), np.ascontiguousarray(rec[rows]))
    np.save(os.path.join(d, "pair_ids.npy"), ids[rows])
    log("outputs of the last timed step written to %s (%d of %d rows)" % (d, len(rows), rec.shape[0]))


class _NoProf:
    conv, corr, corr_bidir = [], [], []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def main():
    args = parse_args()
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(args)))
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_spawn(args)
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # RFX_BENCH_DEVICE / RFX_BENCH_BACKEND exist only to rehearse the N>1 control flow on a 1-GPU box (all ranks on one
    # device, gloo instead of RCCL); the driver's multi-GPU runs use the defaults: one GPU per rank, RCCL.
    backend = os.environ.get("RFX_BENCH_BACKEND", "gloo" if args.dry_run else "nccl")
    dev = None
    if not args.dry_run:
        if not torch.cuda.is_available():
            raise RuntimeError("bench.py needs a HIP device (there is no CPU fallback; --dry-run rehearses the launcher only)")
        dev_index = int(os.environ.get("RFX_BENCH_DEVICE", local_rank))
        torch.cuda.set_device(dev_index)
        dev = torch.device("cuda", dev_index)
    dist = None
    force_dist = os.environ.get("RFX_BENCH_FORCE_DIST") == "1"   # world of ONE rank through RCCL anyway (1-GPU box check)
    if world > 1 or force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        preflight(dist, backend, rank, world, dev)
    sync = (lambda: None) if args.dry_run else torch.cuda.synchronize
    if world > 1:
        # N ranks share one host: each gets its share of the cores for the little CPU work a step has (cell-coordinate tables,
        # the host sgemm probe on rank 0, torch's intra-op pool) instead of N full-size thread pools
        torch.set_num_threads(max(1, cpu_threads() // world))
    # the score chunk: resolved ONCE, on rank 0, BEFORE the workload is built (never inside a launch), and broadcast -- every rank
    # must sum its scores the same way, whatever host it would probe
    from rfx import ops
    sc = [None, None]
    if rank == 0:
        sc = list(ops.resolve_score_chunk(args.score_chunk if not args.score_chunk.lstrip("-").isdigit() else int(args.score_chunk)))
    if dist is not None:
        dist.broadcast_object_list(sc, src=0)
    score_chunk, score_chunk_source = int(sc[0]), sc[1]
    log("score chunk: %d products (%s)" % (score_chunk, score_chunk_source))

    if args.dry_run:
        step, meta, extra = dry_run_step(args, rank), dict(workload="DRY RUN (no GPU): launcher / process-group rehearsal"), None
        prof_factory = _NoProf
    else:
        step, meta, extra = build_workload(args, dev, rank, world, score_chunk=score_chunk)
        prof_factory = ops.Profiler
        torch.manual_seed(123 + rank)
    log("workload built (config %s, rank %d/%d)" % (args.config, rank, world))
    unprofiled, prof, out = None, None, None
    if not args.dry_run and args.config in ("2", "3", "4") and not (args.single_stream and args.config != "2"):
        # config 2: single-pair latency is launch-bound: the product path replays the trunk as ONE HIP graph, which cannot carry the
        # profiler's per-launch events.  configs 3 / 4: the multi-homography rounds run as two lock-step groups on two HIP streams
        # (multi_h_batched split=2) whose kernels overlap -- a per-launch event interval would charge a kernel with its neighbour's
        # time.  -> the product path is timed WITHOUT the profiler (value), then (--full) the same steps once more with it (one
        # group, eager launches, per-launch events) for the rooflines
        e_np, out, _ = timed_loop(step, args, dist, sync, _NoProf)
        unprofiled = e_np
        log("%d timed steps without the profiler (the product path): %.3f s" % (args.steps, e_np))
    timed_out = out
    if unprofiled is None or args.full:
        elapsed, out, prof = timed_loop(step, args, dist, sync, prof_factory)
        log("%d timed steps: %.3f s" % (args.steps, elapsed))
        if timed_out is None:
            timed_out = out
    else:
        elapsed = unprofiled
    profiled_elapsed = elapsed
    if unprofiled is not None:
        elapsed = unprofiled
    per_rank_ms = None
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else None)
        allt = torch.empty((world,), dtype=torch.float64, device=t.device)
        dist.all_gather_into_tensor(allt, t)                              # every rank's own clock: a SCALE record explains itself
        per_rank_ms = [round(float(x) / args.steps * 1e3, 3) for x in allt.tolist()]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    B = args.batch
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, timed_out, [r + world * i for r in range(world) for i in range(B)])
    if args.dump_records and rank == 0:
        # rank-major gathered order: row r*B + i = pair (r + world*i) of the stream (pair i -> rank i mod world)
        torch.save({"records": out.cpu(), "pair_ids": [r + world * i for r in range(world) for i in range(B)], "world": world},
                   args.dump_records)
    col = meta.get("col", dict(status=9, nbh=None, rank=0))
    ok_pairs = int((out[:, col["status"]] == 0).sum().item())
    names = {"3": "BASELINE config 3 (configs[2]) as worded", "qs": "quick_start semantics at the metric's size (BASELINE configs 2+3 shape, one homography)",
             "2": "BASELINE config 2 (configs[1])", "4": "BASELINE config 4 (configs[3])", "5": "BASELINE config 5 (configs[4])"}
    line = {"metric": METRIC, "value": round(B * args.steps * world / elapsed, 3), "unit": "pairs/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": dict({k: v for k, v in meta.items() if k != "col"}, config=args.config, baseline_config=names.get(args.config, "dry run"),
                           pairs_per_step_per_gpu=B, weights="random-init",
                           arithmetic=("float32 in and out of every kernel; convolution sums: fp32 matrix cores (v_mfma_f32_32x32x2_f32) or, for the "
                                       "long-K 1x1 and the 3x3 layers, float32 = hi + mid + lo bf16 pieces (exact) multiplied on the bf16 "
                                       "matrix cores (every product exact, float32 accumulators) -- error against float64 not larger than the "
                                       "fp32 kernels'; extra.fp32_mfma_only = the same workload with RFX_CONV_SPLIT=0"
                                       if os.environ.get("RFX_CONV_SPLIT", "1") != "0" else "float32, fp32 matrix cores only (RFX_CONV_SPLIT=0)"),
                           parallelism="pairs sharded over %d rank(s) (pair i -> rank i mod N), one all_gather of result records per step" % world,
                           gathered_records=int(out.shape[0]), record_bytes_per_pair=int(out.shape[1]) * 4, aligned_ok_last_step=ok_pairs,
                           ranks_seen_in_gather=sorted(set(int(x) for x in out[:, col["rank"]].tolist())),
                           collective=("all_gather_into_tensor over %s, %d rank(s)" % (backend, world)) if dist is not None else "none (single process)",
                           score_chunk_products=score_chunk, score_chunk_source=score_chunk_source,
                           ransac_draw="host (torch.randint, CPU generator)" if args.host_draw else "device (Philox4x32-10)",
                           streams=("single stream, one lock-step group (--single-stream: profiling run)" if args.single_stream else
                                    "product path: trunk levels on 4 HIP streams, multi-homography rounds as lock-step groups on streams"),
                           rank_deficient_samples=("host LAPACK (exact mode: librfxhost.so runs numpy's own dgesdd on the flagged samples)"
                                                   if (args.degenerate == "lapack" or (args.degenerate == "auto" and args.host_draw))
                                                   else "device null vector"),
                           preprocessing="host PIL, outside the timed region" if args.host_prep else
                           "device (bit-exact Pillow LANCZOS pyramid + ToTensor/Normalize), inside the timed step")}
    if dist is not None:
        try:
            rv = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None
        except Exception:  # noqa: BLE001
            rv = None
        line["config"].update(n_ranks_in_process_group=int(dist.get_world_size()), backend=backend, rccl_version=rv,
                              ms_per_step_per_rank=per_rank_ms, cpu_threads_per_rank=torch.get_num_threads())
        if backend == "nccl":
            line["config"]["n_ranks_in_rccl"] = int(dist.get_world_size())
    if args.pcie:
        line["config"]["pcie_inclusive"] = ("NOT the headline: raw uint8 images uploaded from pinned host memory and the result records copied "
                                            "back to pinned host memory inside every timed step (%.1f + %.1f MB per step)"
                                            % (2.0 * B * args.height * args.width * 3 / 1e6, out.shape[0] / world * out.shape[1] * 4 / 1e6))
    if not args.dry_run and col["nbh"] is not None:
        nbh = out[:, col["nbh"]]
        line["config"]["homographies_per_pair_last_step"] = {"mean": round(float(nbh.mean()), 2), "min": int(nbh.min()), "max": int(nbh.max())}
        line["config"]["homographies_per_s"] = round(float(nbh.sum()) * args.steps / elapsed, 1)
    if not args.dry_run and args.full:
        roof, corr = rooflines(prof, profiled_elapsed, rank, args.config, dev)
        if unprofiled is not None and args.config == "2":
            roof["note"] = ("value / ms_per_step: HIP-graph trunk, no profiler (%.2f ms per pair); this roofline: a second pass of %d steps "
                            "with the per-launch events (eager launches, %.2f ms per pair)" % (unprofiled / args.steps * 1e3, args.steps,
                                                                                          profiled_elapsed / args.steps * 1e3))
        elif unprofiled is not None:
            roof["note"] = ("value / ms_per_step: the product path, no profiler (multi-homography rounds as lock-step groups on HIP streams, "
                            "%.2f ms per step); this roofline: the same %d steps once more under the per-launch events (one group: "
                            "overlapping streams would charge a kernel with its neighbour's time), %.2f ms per step"
                            % (unprofiled / args.steps * 1e3, args.steps, profiled_elapsed / args.steps * 1e3))
            line["config"]["ms_per_step_profiled_pass"] = round(profiled_elapsed / args.steps * 1e3, 3)
        line["roofline"] = roof
        if corr:
            line["roofline_corr"] = corr

    extras = {}
    if rank == 0 and not args.dry_run and args.full and args.config == "3" and world == 1:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        # ---- quick_start semantics, driver-timed next to the headline: rounds 1-2's headline workload ----
        if not args.no_qs_leg:
            aq = argparse.Namespace(**vars(args))
            aq.config, aq.steps, aq.warmup, aq.nb_iter, aq.nb_scale = "qs", 10, 2, 1000, 7
            stepq, metaq, extraq = build_workload(aq, dev, rank, world, score_chunk=score_chunk)
            torch.manual_seed(123)
            eq, outq, profq = timed_loop(stepq, aq, None, sync, ops.Profiler)
            rq, cq = rooflines(profq, eq, rank, "qs", dev)
            extras["quick_start"] = {"value": round(B * aq.steps / eq, 3), "unit": "pairs/s", "ms_per_step": round(eq / aq.steps * 1e3, 2),
                                     "steps": aq.steps, "warmup": aq.warmup, "workload": metaq["workload"],
                                     "aligned_ok_last_step": int((outq[:, 9] == 0).sum().item()),
                                     "roofline": {k: rq[k] for k in ("kernel", "achieved", "frac", "avg_launch_us", "time_share", "all_conv_tflops", "conv_time_share", "traffic")},
                                     "roofline_corr": cq}
            log("quick_start leg done: %.1f pairs/s" % extras["quick_start"]["value"])
        # ---- the other draw / null-vector modes on the SAME workload: what the exact mode costs ----
        if not args.no_exact_leg:
            ex = {}
            for name, hd, dg in (("host_draw_lapack", True, "lapack"), ("device_draw_device_null_vector", False, "device")):
                ae = argparse.Namespace(**vars(args))
                ae.host_draw, ae.degenerate, ae.steps, ae.warmup = hd, dg, 5, 1
                stepe, _, extrae = build_workload(ae, dev, rank, world, score_chunk=score_chunk)
                torch.manual_seed(123)
                ee, oute, _ = timed_loop(stepe, ae, None, sync, _NoProf)
                ex[name] = {"pairs_per_s": round(B * ae.steps / ee, 3), "ms_per_step": round(ee / ae.steps * 1e3, 2), "steps": ae.steps,
                            "vs_timed_mode": round((B * ae.steps / ee) / line["value"], 4),
                            "aligned_ok_last_step": int((oute[:, col["status"]] == 0).sum().item())}
                del stepe, extrae
                torch.cuda.empty_cache()
            # the timed (exact) mode once more with its host stage logged: flagged samples, dgesdd calls, host milliseconds per step
            pipe_t = extra["pipe"]
            pipe_t.exact_log = []
            step()
            sync()
            L, pipe_t.exact_log = pipe_t.exact_log, None
            from rfx import _lapack
            ex["timed_mode_host_stage"] = {"flagged_samples_per_step": int(sum(sum(r["n_degenerate"]) for r in L)),
                                           "dgesdd_calls_per_step": int(sum(r["n_solved"] for r in L)),
                                           "host_ms_per_step": round(sum(r["host_ms"] for r in L), 2), "ransac_calls_per_step": len(L),
                                           "solver": _lapack.info()}
            ex["timed_mode_vs_device_null_vector"] = round(line["value"] / ex["device_draw_device_null_vector"]["pairs_per_s"], 4)
            ex["note"] = ("value = the EXACT mode (device Philox draws; rank-deficient 4-point samples re-solved by the host's LAPACK through "
                          "librfxhost.so, hidden under the other lock-step group's kernels); device_draw_device_null_vector = rounds 3-5's timed "
                          "mode (no host stage); host_draw_lapack = torch.randint on the CPU generator per pair and round: the mode `parity` is "
                          "measured in (one lock-step group, a second sync per round)")
            extras["exact_mode"] = ex
            # ---- every convolution on the fp32-MFMA kernels (RFX_CONV_SPLIT=0: no bf16-piece kernels, fused Bottleneck tails): the
            # figure to read if one does not accept float32 sums formed from exact bf16 operand pieces as float32 arithmetic
            prev = os.environ.get("RFX_CONV_SPLIT")
            os.environ["RFX_CONV_SPLIT"] = "0"
            try:
                af = argparse.Namespace(**vars(args))
                af.steps, af.warmup = 5, 1
                stepf, _, extraf = build_workload(af, dev, rank, world, score_chunk=score_chunk)
                torch.manual_seed(123)
                ef, outf, _ = timed_loop(stepf, af, None, sync, _NoProf)
                extras["fp32_mfma_only"] = {"pairs_per_s": round(B * af.steps / ef, 3), "ms_per_step": round(ef / af.steps * 1e3, 2), "steps": af.steps,
                                            "vs_value": round((B * af.steps / ef) / line["value"], 4),
                                            "aligned_ok_last_step": int((outf[:, col["status"]] == 0).sum().item()),
                                            "note": "RFX_CONV_SPLIT=0: the same workload with every convolution on the fp32 matrix-core kernels "
                                                    "(v_mfma_f32_32x32x2_f32) of rounds 1-5; `value` runs the long-K 1x1 layers, the stride-2 projections and "
                                                    "every 3x3 layer on rfx_conv1x1_split_* / rfx_conv3x3_split_* (float32 results from exact bf16 operand pieces; "
                                                    "error against float64 not larger than the fp32 kernels': profiles/r06_split_conv_bench.json)"}
                # the fp32-MFMA build's own roofline (3 steps under the per-launch events): the kernel `roofline` named in rounds 3-5
                ap = argparse.Namespace(**vars(af))
                ap.steps, ap.warmup = 3, 0
                ep, _, proff = timed_loop(stepf, ap, None, sync, ops.Profiler)
                rf, _ = rooflines(proff, ep, rank, "3", dev)
                extras["fp32_mfma_only"]["roofline"] = {k: rf[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_us",
                                                                         "time_share", "all_conv_tflops", "conv_time_share")}
                del stepf, extraf, proff
                torch.cuda.empty_cache()
            finally:
                if prev is None:
                    os.environ.pop("RFX_CONV_SPLIT", None)
                else:
                    os.environ["RFX_CONV_SPLIT"] = prev
            log("exact-mode leg done: %s" % {k: v["pairs_per_s"] for k, v in ex.items() if isinstance(v, dict) and "pairs_per_s" in v})
        # ---- CPU legs: bounded oracle baseline, then the parity sweeps over pairs of the timed batches ----
        if not args.no_cpu_baseline:
            log("GPU legs done; timing the CPU oracle (bounded sample, child process)")
            line["cpu_baseline"] = cpu_baseline_subprocess(args)
            if not args.no_parity:
                import parity_sweep   # the CHECKER: dumps the device results, the oracle runs in child processes
                seeds = extra["seeds"][:args.parity_pairs] if args.parity_pairs else extra["seeds"]
                d = tempfile.mkdtemp(prefix="rfx_parity_loop_")
                parity_sweep.dump_gpu_loop("ev_loop", seeds, dev, d, batch=16,
                                           pipe=parity_sweep.gpu_pipeline("ev_loop", args.height, args.width, dev, score_chunk=score_chunk))
                log("parity sweep (config 3, exact mode: every round of the multi-H loop on the oracle), %d pairs dumped, budget %.0f s" % (len(seeds), args.parity_budget))
                line["parity"] = parity_subprocess("ev_loop", d, seeds, args.height, args.width, args.parity_budget)
                # ---- the mode that is TIMED: device Philox draws, device null vectors; every round replayed on the reference with
                # the device's own samples injected at utils/outil.py:120
                d = tempfile.mkdtemp(prefix="rfx_parity_timed_")
                parity_sweep.dump_gpu_loop("ev_loop", seeds, dev, d, batch=16, draw="device",
                                           pipe=parity_sweep.gpu_pipeline("ev_loop", args.height, args.width, dev, draw="device",
                                                                          score_chunk=score_chunk, degenerate=args.degenerate))
                log("parity sweep over the TIMED mode (device draws replayed on the reference), budget %.0f s" % args.timed_parity_budget)
                os.environ["RFX_PARITY_RECORDS_SUFFIX"] = "_timed_mode"
                line["parity_timed_mode"] = parity_subprocess("ev_loop", d, seeds, args.height, args.width, args.timed_parity_budget)
                os.environ.pop("RFX_PARITY_RECORDS_SUFFIX", None)
                # ---- the reference against ITSELF on the evaluation pyramid (first homography, two CPU execution settings): the rate
                # at which the reference's own arg-max near-ties flip, next to config 3's device-vs-reference count
                log("reference vs reference (evaluation pyramid, first homography), budget %.0f s" % args.stability_budget)
                ovo = parity_subprocess("ev", None, seeds, args.height, args.width, args.stability_budget, stability=True)
                line["parity"]["oracle_vs_oracle"] = ovo
                if "pairs" in ovo and ovo["pairs"] and "total_matches" in ovo and line["parity"].get("total_matches"):
                    pz = line["parity"]
                    pz["flipped_matches_per_1e4_device_vs_reference"] = round(1e4 * pz["total_flipped_matches"] / pz["total_matches"], 3)
                    pz["flipped_matches_per_1e4_reference_vs_reference"] = round(1e4 * ovo["total_flipped_matches"] / max(ovo["total_matches"], 1), 3)
                if not args.no_qs_leg:
                    d = tempfile.mkdtemp(prefix="rfx_parity_qs_")
                    parity_sweep.dump_gpu_pairs("qs", seeds, args.height, args.width, dev, d,
                                                pipe=parity_sweep.gpu_pipeline("qs", args.height, args.width, dev, score_chunk=score_chunk))
                    log("parity sweep (quick_start: oracle end to end), budget %.0f s" % args.qs_parity_budget)
                    extras["quick_start"]["parity"] = parity_subprocess("qs", d, seeds, args.height, args.width, args.qs_parity_budget)
                    log("reference vs reference (quick_start: two CPU execution settings), budget %.0f s" % args.stability_budget)
                    ovo = parity_subprocess("qs", None, seeds, args.height, args.width, args.stability_budget, stability=True)
                    extras["quick_start"]["parity"]["oracle_vs_oracle"] = ovo
                    if "pairs" in ovo and ovo["pairs"]:
                        q = extras["quick_start"]["parity"]
                        q["flipped_pairs_device_vs_reference_per_pair"] = round(q["pairs_with_flips"] / max(q["pairs"], 1), 3)
                        q["flipped_pairs_reference_vs_reference_per_pair"] = round(ovo["pairs_with_flips"] / ovo["pairs"], 3)
    elif rank == 0 and not args.dry_run and args.full and args.config == "qs" and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        line["cpu_baseline"] = cpu_baseline_subprocess(args)
        if not args.no_parity:
            import parity_sweep
            seeds = extra["seeds"][:args.parity_pairs] if args.parity_pairs else extra["seeds"]
            d = tempfile.mkdtemp(prefix="rfx_parity_")
            parity_sweep.dump_gpu_pairs("qs", seeds, args.height, args.width, dev, d,
                                        pipe=parity_sweep.gpu_pipeline("qs", args.height, args.width, dev, score_chunk=score_chunk))
            line["parity"] = parity_subprocess("qs", d, seeds, args.height, args.width, args.parity_budget)
    if dist is not None:
        # all collectives are done: leave the group BEFORE rank 0's CPU leg, so that no rank waits in a communicator for it
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and world > 1 and not args.dry_run and args.full and args.config in ("3", "qs") and not args.no_cpu_baseline:
        # N > 1: the line still carries the host baseline (bounded, ~1 min); the parity sweeps stay with the N = 1 run
        log("rank 0: timing the CPU reference (bounded sample, child process)")
        line["cpu_baseline"] = cpu_baseline_subprocess(args)
    if extras:
        line["extra"] = extras
    if rank == 0:
        print(json.dumps(line))


if __name__ == "__main__":
    main()
