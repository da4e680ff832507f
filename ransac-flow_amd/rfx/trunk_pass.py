"""The trunk feature pass every alignment starts with (AlignPipeline.features / prepare_and_features): ResNet-50 conv4 features of all
pyramid levels and of the target, L2-normalised into featA (B,1024,ldA) / featB (B,1024,nB).

Two halves.  The capture policy: ``graph_eligible`` (which batches replay a HIP graph), ``CapturePolicy`` (when a shape is captured and
which captures are kept; pure Python) and ``graphed`` (warm-up, capture, the empty-capture guard and the replay -- the one place that
builds a graph).  The launch forms of the pass itself, ``features_eager``: a layout step, then ``_levels_grouped`` (one grouped launch
per kernel instance and layer for all images of a pair, as one chain or as balanced chains on their own streams) or
``_levels_streamed`` (one trunk pass per level, dealt to N streams), then a shared finish.  ``fork_join`` is the stream choreography both
multi-stream forms use; ``pair_level_with_target``, ``balance_chains`` and ``level_stream_count`` are their pure rules.  Every
environment switch is read at call time.
"""
import collections
import functools
import os

import torch

from . import ops
from .cache import lease


def graph_eligible(B):
    """Small batches are launch-bound and replay a HIP graph; RFX_GRAPH=0 disables; never under an ops.Profiler, whose per-launch
    events cannot be recorded into a graph."""
    return B <= 4 and os.environ.get("RFX_GRAPH", "1") != "0" and ops.Profiler.active() is None


class CapturePolicy:
    """Which keys get a captured graph: a key is captured at its SECOND sighting (a stream of variable-size pairs never pays warm-up +
    capture for shapes it sees once; the seen-set remembers the last 64 keys, oldest forgotten first) and at most ``max_entries``
    captures are kept, least recently used evicted first (an evicted entry releases its graph, pool and static buffers).  All keys
    -- shape keys of the trunk pass, ("raw", ...) keys of the pyramid + trunk pass -- share one cache and one bound."""
    SEEN_MAX = 64

    def __init__(self, max_entries):
        self.max_entries = max_entries
        self.entries = collections.OrderedDict()
        self.seen = collections.OrderedDict()

    def decide(self, key):
        """"replay" (an entry exists; it becomes the most recently used), "capture" (second sighting) or "eager" (first)."""
        if key in self.entries:
            self.entries.move_to_end(key)
            return "replay"
        if key in self.seen:
            return "capture"
        self.seen[key] = True
        while len(self.seen) > self.SEEN_MAX:
            self.seen.popitem(last=False)
        return "eager"

    def store(self, key, entry):
        self.entries[key] = entry
        while len(self.entries) > self.max_entries:
            self.entries.popitem(last=False)


def graphed(pipe, key, inputs, body, what="trunk pass"):
    """``body(inputs)`` -> (prep, feats) through the capture policy of ``pipe``: the eager call at a first sighting, otherwise the
    HIP-graph replay of ``body`` over static copies of the tensors ``inputs``.  Warm-up, capture and replay run under the pipeline's
    own device: ``torch.cuda.graph`` captures the CURRENT device's stream, while the kernels launch on pipe.dev's.  The returned
    featA / featB are clones; everything else ``body`` returned (``prep`` included) belongs to the graph and is valid until its next
    replay."""
    step = pipe._capture.decide(key)
    if step == "eager":
        return body(inputs)
    with torch.cuda.device(pipe.dev):
        if step == "capture":
            # whatever the captured kernels read from a bounded cache (Lanczos tables, cell coordinates: addresses baked into the
            # graph) is held by the lease list, which lives and dies with the cache entry
            with lease() as held:
                body(inputs)                            # warm-up: lazily built state (packed weights ...) must exist
                torch.cuda.synchronize(pipe.dev)
                static = [x.clone() for x in inputs]
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    prep, out = body(static)
            # an empty capture (kernels launched outside the captured stream) would replay stale features for ever:
            # check once that a replay really rewrites the outputs
            out["featA"].zero_()
            g.replay()
            torch.cuda.synchronize(pipe.dev)
            if not bool(out["featA"].abs().sum() > 0):
                raise RuntimeError("HIP-graph capture of the %s is empty (kernels did not go to the capture stream)" % what)
            held = list({id(v): v for v in held}.values())      # warm-up and capture read the same values: keep each once
            pipe._capture.store(key, (g, static, prep, out, held))
        g, static, prep, out, _ = pipe._capture.entries[key]
        for d, x in zip(static, inputs):
            d.copy_(x)
        g.replay()
        res = dict(out)
        res["featA"], res["featB"] = out["featA"].clone(), out["featB"].clone()   # the graph's own buffers are reused by the next replay
    return prep, res


def fork_join(main, jobs):
    """Run ``jobs`` = [(stream, fn)] in list order, each under its stream, and return their results.  A job whose stream is not
    ``main`` (the caller passes ``main`` itself for the ones that are) waits for one ready event recorded on ``main`` before the first
    job and records a done event of its own; ``main`` waits for every done event, in order, after the last job.  A job on ``main``
    neither waits nor records, so jobs that are all on ``main`` create no event at all.  Under capture these events are the fork and
    join edges of the graph.  Tensors that cross streams are the caller's to ``record_stream``."""
    ready = None
    if any(st is not main for st, _ in jobs):
        ready = torch.cuda.Event()
        ready.record(main)
    results, done = [], []
    for st, fn in jobs:
        with torch.cuda.stream(st):
            if st is not main:
                st.wait_event(ready)
            results.append(fn())
            if st is not main:
                ev = torch.cuda.Event()
                ev.record(st)
                done.append(ev)
    for ev in done:
        main.wait_event(ev)
    return results


def pair_level_with_target(src_shapes, tgt_shape):
    """Index of the first pyramid level that has the target's shape (the level of scale 1), or None.  That level and the target
    go through the trunk as ONE problem of 2B images (one launch tail less per layer); every sample is computed independently,
    bit-identical to two passes."""
    return next((i for i, s in enumerate(src_shapes) if tuple(s) == tuple(tgt_shape)), None)


def balance_chains(sizes, nch):
    """Deal items of the given sizes to ``nch`` chains: largest first (equal sizes in index order), each to the lightest chain so
    far (the lowest chain index among equals).  Returns the item indices of every chain; chains may stay empty.  (measured on a
    single 480x640 pair against "the two largest levels vs the rest" 5.63 ms and alternating 5.99 ms: 5.38-5.43 ms)"""
    chains, load = [[] for _ in range(nch)], [0] * nch
    for i in sorted(range(len(sizes)), key=lambda i: -sizes[i]):
        k = load.index(min(load))
        chains[k].append(i)
        load[k] += sizes[i]
    return chains


def level_stream_count(B, n_levels, env, profiled):
    """Streams the per-level trunk passes are dealt to.  ``env`` = RFX_TRUNK_STREAMS: its value, at least 1.  Default: one stream per
    level for small batches (B <= 4: a layer of one level has too few workgroups to fill 256 CUs -- a single 480x640 pair drops from
    15.9 to 10.6 ms), four streams otherwise (round 6, profiles/r06_stream_sweep.txt: 1 / 2 / 4 / 8 streams = 113.6 / 113.0 / 114.6 /
    114.8 pairs/s on config 3 with 3 lock-step groups -- the tail of one level's layer overlaps another level's kernels).  ONE stream
    under an ops.Profiler: overlapping launches would charge one kernel with another's time in the per-launch event timing bench.py's
    rooflines are computed from."""
    if profiled:
        return 1
    if env:
        return max(1, int(env))
    return n_levels if B <= 4 else min(4, n_levels)


Layout = collections.namedtuple("Layout", "B dims nA ldA offs Ws Hs featA")


def _layout(pipe, prep):
    """Where every pyramid level lands in featA: level i of (r, c) cells owns columns offs[i] : offs[i] + r * c."""
    B = prep["B"]
    dims = [(x.shape[2] // 16, x.shape[3] // 16) for x in prep["src"]]
    nA = sum(r * c for r, c in dims)
    ldA = (nA + 3) // 4 * 4      # rows padded to 16 bytes: the mutual-NN kernel then stages with float4 loads
    featA = torch.empty((B, 1024, ldA), dtype=torch.float32, device=pipe.dev)
    Ws, Hs, offs = [], [], []
    off = 0
    for (r, c) in dims:
        W, Hh = pipe._cell_coords(r, c)
        Ws.append(W)
        Hs.append(Hh)
        offs.append(off)
        off += r * c
    return Layout(B, dims, nA, ldA, offs, Ws, Hs, featA)


def _l2norm_level(lay, i, f):
    ops.l2norm(f, out=lay.featA[:, :, lay.offs[i]:], out_batch_stride=1024 * lay.ldA, out_chan_stride=lay.ldA)


def _levels_grouped(pipe, prep, lay):
    """Small batches: the 8 images of a pair (7 pyramid levels + target) have 8 different sizes, so a layer is 8 launches of 2-150
    workgroups on 256 CUs and the pass is bound by one workgroup lifetime per layer AND level.  All levels go through the trunk layer
    by layer with ONE grouped launch per kernel instance and layer (nets.forward_group: blockIdx.y selects the image); bit-identical
    to the per-level passes.  Returns the target's raw features."""
    B, tgt, nL = lay.B, prep["tgt"], len(lay.dims)
    shared = pair_level_with_target([x.shape for x in prep["src"]], tgt.shape)
    xs = [torch.cat((x, tgt), dim=0) if i == shared else x for i, x in enumerate(prep["src"])]
    if shared is None:
        xs.append(tgt)

    def chain(idxs, **kw):
        fs = pipe.trunk.forward_group([xs[i] for i in idxs], **kw)
        for i, f in zip(idxs, fs):
            if i < nL:
                _l2norm_level(lay, i, f[:B] if i == shared else f)
        return fs

    nch = max(1, int(os.environ.get("RFX_GROUP_CHAINS", "2")))
    if nch == 1:
        # one chain + the library's side streams (round 3's first form)
        fs = chain(range(len(xs)))
    else:
        # The images split into k pixel-balanced subsets, each its own grouped chain on its own stream (captured as a fork /
        # join of the graph): the launch tails of one chain overlap the other's kernels.  Single 480x640 pair: 6.08-6.35 -> 5.38-5.70 ms
        # with two chains on the same box (three: 5.7-6.3, four: 5.8), two pairs 10.22 -> 9.54 ms; each chain keeps its kernel
        # instances serial on its stream.
        # (side streams inside a chain, shared or one pool per chain, crash the process on ROCm 7.2: chains stay serial)
        chains = [idxs for idxs in balance_chains([x.numel() for x in xs], nch) if idxs]
        main = torch.cuda.current_stream(pipe.dev)
        streams = [main] + pipe._side_streams("chain", nch - 1, exact=True)
        outs = fork_join(main, [(streams[k], functools.partial(chain, idxs, side_streams=False)) for k, idxs in enumerate(chains)])
        fs = [None] * len(xs)
        for idxs, out in zip(chains, outs):
            for i, f in zip(idxs, out):
                fs[i] = f
        for f in fs:
            f.record_stream(main)
    return fs[shared][B:] if shared is not None else fs[-1]


def _levels_streamed(pipe, prep, lay, nstream):
    """The pyramid levels are independent trunk passes.  With ``nstream`` > 1 they are dealt to that many HIP streams so that the
    launch tails of one level -- the /16 maps of the small levels have few workgroups per layer -- overlap with the next level's
    kernels; every level still writes its own columns of featA.  Returns the target's raw features, or None when no level shares
    its pass with the target.
    (measured, coarse stage of 480x640 pairs: B = 1 7.73 -> 6.83 ms, B = 2 10.15 -> 9.99 ms, B = 4 16.7 -> 18.3 ms: from four
    pairs on the per-level batches are large enough for the 8-stream form to win)"""
    B, tgt = lay.B, prep["tgt"]
    pair = pair_level_with_target([x.shape for x in prep["src"]], tgt.shape)
    main = torch.cuda.current_stream(pipe.dev)
    # (stream priorities for the largest levels -- the critical path of a small-batch pass -- were measured: 7.7 ->
    # 9.1-9.2 ms with one or two high-priority queues; all queues stay equal)
    streams = pipe._side_streams("level", nstream, exact=True) if nstream > 1 else [main]

    def level(i):
        x = prep["src"][i]
        if i != pair:
            _l2norm_level(lay, i, pipe.trunk(x))
            return None
        f2 = pipe.trunk(torch.cat((x, tgt), dim=0))
        _l2norm_level(lay, i, f2[:B])
        return f2[B:]

    outs = fork_join(main, [(streams[i % len(streams)], functools.partial(level, i)) for i in range(len(lay.dims))])
    ft_raw = None if pair is None else outs[pair]
    if ft_raw is not None and nstream > 1:
        ft_raw.record_stream(main)
    return ft_raw


def _finish(pipe, prep, lay, ft_raw):
    """The target's normalised features (from its own trunk pass when no form has run it yet) and the feature dict."""
    B = lay.B
    ft = ops.l2norm(ft_raw if ft_raw is not None else pipe.trunk(prep["tgt"]))
    rt, ct = ft.shape[2], ft.shape[3]
    Wt, Ht = pipe._cell_coords(rt, ct)
    return dict(featA=lay.featA, featB=ft.view(B, 1024, rt * ct), nA=lay.nA, ldA=lay.ldA, nB=rt * ct, WA=torch.cat(lay.Ws),
                HA=torch.cat(lay.Hs), Wt=Wt, Ht=Ht, rt=rt, ct=ct)


def features_eager(pipe, prep):
    """The trunk pass without a graph.  Batches of one or two pairs take the grouped form (RFX_GROUPED=0 disables; never under an
    ops.Profiler; an explicit RFX_TRUNK_STREAMS asks for the per-level form), everything else the per-level passes."""
    lay = _layout(pipe, prep)
    profiled = ops.Profiler.active() is not None
    env = os.environ.get("RFX_TRUNK_STREAMS")
    if lay.B <= 2 and os.environ.get("RFX_GROUPED", "1") != "0" and not profiled and not env:
        ft_raw = _levels_grouped(pipe, prep, lay)
    else:
        ft_raw = _levels_streamed(pipe, prep, lay, level_stream_count(lay.B, len(lay.dims), env, profiled))
    return _finish(pipe, prep, lay, ft_raw)
