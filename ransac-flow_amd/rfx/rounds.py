"""The lock-step rounds of the batched multi-homography drivers: AlignPipeline.multi_h_batched (dense and ragged preps),
multi_h_kitti_batched and multi_h_variant_c.

Round k computes the k-th homography of every pair of a group that is still active.  ``lockstep_rounds`` is the one round loop:
active list -> matches of the round -> index draws -> RANSAC search -> fine stage + accept kernel -> ONE host readback (the accept
flags) -> per-pair outputs and stop rule.  It is a generator that yields a HIP event at every host wait; ``drive_rounds`` runs
one generator per lock-step group, each under its own stream, and resumes the group whose event is due.  What the drivers differ
in -- where a round's matches come from, the fine stage, how a pair's outputs are cut out of the round's tensors, when a pair
stops -- is the group class: DenseGroup (Hpatch), KittiGroup, RaggedGroup (Hpatch, pairs of different sizes), RaggedKittiGroup
(KITTI, pairs of different sizes), VariantCGroup (one target-shape group of the YFCC driver), RaggedVariantCGroup (YFCC, pairs and
chosen candidates of different sizes).  ``split_policy`` decides how many groups a batch is cut into, RoundState holds what the
groups of one call share.
"""
import os

import torch

from . import ops, ragged

# default number of lock-step groups: (from this many pairs on, groups), largest first.
# Hpatch (measured, profiles/r06_stream_sweep.txt: config 3, 64 pairs: 1 / 2 / 3 / 4 / 6 groups = 110.2 / 112.7 / 115.3 / 115.4 / 115.6
# pairs/s; config 4, 16 pairs, 50 000 hypotheses: 2 / 3 / 4 groups = 56.1 / 57.4 / 56.2; 4 groups from 32 pairs since the 16x16-patch
# split 3x3 kernels: 152.6 pairs/s on config 3)
HPATCH_SPLIT = ((32, 4), (12, 3), (8, 2))
# KITTI (measured at config 5, B = 8: two groups of 4 hide the exact mode's host stage but run the fine passes at batch 4 instead of 8
# -- a wash (21.0 vs 21.1 pairs/s, profiles/r06_stream_sweep.txt); groups pay from 8 pairs per group on)
KITTI_SPLIT = ((16, 2),)


def split_policy(B, split, thresholds, host_draw=False, trace=False, host_filter=False, profiled=False, env=None):
    """Number of lock-step groups of a batch of B pairs.  ``split``: the caller's argument; None = RFX_MULTIH_SPLIT or the driver's
    default ``thresholds`` (HPATCH_SPLIT / KITTI_SPLIT).  Forced to 1 with host draws / ``sample_fn`` (the CPU generator is consumed
    in pair order), with a trace, with an injected KITTI host filter (called in pair order) and under an ops.Profiler (per-launch
    events; RFX_MULTIH_SPLIT_PROFILED=1 lifts this one).  Clamped to [1, B].  ``env``: os.environ unless given."""
    env = os.environ if env is None else env
    if split is None:
        split = int(env.get("RFX_MULTIH_SPLIT", "0")) or next((k for n, k in thresholds if B >= n), 1)
    if host_draw or trace or host_filter or (profiled and env.get("RFX_MULTIH_SPLIT_PROFILED", "0") != "1"):
        split = 1
    return max(1, min(int(split), B))


class RoundState:
    """What the lock-step groups of one driver call share, indexed by position in the batch: the per-pair outputs ``outs`` and
    homography counts ``nb``, the key of the device draws (``ids``, ``epoch``: AlignPipeline._draw_epoch), the degenerate mode, the
    number of groups ``split`` with their ``bounds``, and the caller's options."""

    def __init__(self, pipe, outs, driver, thresholds, split, sample_fn, records, want_lists, trace, pair_ids, draw_epoch,
                 maskRegionTh, maxCoarse=None, host_filter=False):
        B = len(outs)
        host_draw = sample_fn is not None or pipe.draw == "host"
        self.pipe, self.outs, self.nb = pipe, outs, [0] * B
        self.sample_fn, self.records, self.want_lists, self.trace = sample_fn, records, want_lists, trace
        self.maskRegionTh, self.maxCoarse = maskRegionTh, maxCoarse
        self.split = split_policy(B, split, thresholds, host_draw, trace is not None, host_filter, ops.Profiler.active() is not None)
        self.bounds = [(B * k // self.split, B * (k + 1) // self.split) for k in range(self.split)]
        self.ids, self.epoch = pipe._draw_epoch(pair_ids, driver, draw_epoch)
        if self.ids is None and self.split > 1:
            self.ids = torch.arange(B, dtype=torch.int32, device=pipe.dev)       # the key of pair b stays its batch position b
        self.eye = torch.eye(3, device=pipe.dev)
        self.degenerate = pipe._degenerate_mode(host_draw)

    def close(self, mask_of, matches=None):
        """The per-pair outputs after the rounds: ``mask`` = mask_of(b), ``nbH`` and, for the drivers that match once, ``matches``."""
        for b, o in enumerate(self.outs):
            o["mask"], o["nbH"] = mask_of(b), self.nb[b]
            if matches is not None:
                idx1, idx2, cnt = matches
                o["matches"] = (idx1[b], idx2[b], cnt[b:b + 1])      # the cached mutual matches (rows beyond the count: undefined)
        return self.outs


def drive_rounds(pipe, gens):
    """Run lock-step round generators to completion from this host thread: generator k runs under stream k (the caller's
    stream for k = 0, pipeline-owned side streams after), yields a HIP event whenever it needs the host to see device results,
    and is resumed once that event has completed -- whichever group is ready first.  One generator: the plain sequential loop."""
    main = torch.cuda.current_stream(pipe.dev)
    streams = [main] + pipe._side_streams("round", max(len(gens) - 1, 0))
    for s in streams[1:]:
        s.wait_stream(main)
    live = [(g, s, None) for g, s in zip(gens, streams)]
    while live:
        # the group whose event has already completed goes first (its host work -- the LAPACK stage, the next round's
        # launches -- then runs under the other groups' queued kernels); none ready: wait for the one that yielded first
        k = next((i for i, (_, _, ev) in enumerate(live) if ev is None or ev.query()), 0)
        g, s, ev = live.pop(k)
        if ev is not None:
            ev.synchronize()
        with torch.cuda.stream(s):
            try:
                ev = next(g)
            except StopIteration:
                continue
        live.append((g, s, ev))
    for s in streams[1:]:
        main.wait_stream(s)


def lockstep_rounds(g):
    """The rounds of one lock-step group ``g`` as a generator (see drive_rounds): yields a recorded HIP event at every host wait.
    All launches go to the stream that is current while the generator runs.  Pair m of the group is pair g.pairs[m] of the batch."""
    st = g.st
    pipe, dev, trace = st.pipe, st.pipe.dev, st.trace
    G = len(g.pairs)
    acc_host = torch.empty(G, dtype=torch.int32).pin_memory()
    active = list(range(G))
    rnd = 0
    while active:
        a = len(active)
        # all pairs active: A = None, and nothing below gathers rows
        A = None if a == G else torch.tensor(active, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        pairs = [g.pairs[m] for m in active]
        M1, M2, n_dev = g.matches(A, active)
        smp = pipe._round_draws(pairs, n_dev, st.sample_fn, A, g.ids, st.epoch, rnd)
        rnd += 1
        if st.degenerate == "lapack":
            # the exact mode: stage 1 + the flagged samples into pinned memory, then -- first round only -- the target's
            # FeatureExtractor pass (independent of the search) BEHIND the gather, so that the host's LAPACK stage runs
            # while the GPU works; the other rounds hide it under another group's kernels (split > 1)
            search = ops.ransac_h4_batched_begin(M1, M2, n_dev, smp, pipe.tol)
            g.target_features()
            yield search.event
            info = {} if getattr(pipe, "exact_log", None) is not None else None
            bestH, inl, res = ops.ransac_h4_batched_finish(search, info=info)
            if info is not None:
                pipe.exact_log.append(dict(info, round=rnd - 1, lo=g.pairs[0], active=a))
        else:
            g.target_features()
            bestH, inl, res = ops.ransac_h4_batched(M1, M2, n_dev, smp, pipe.tol, degenerate=st.degenerate)
        Hs = torch.where((res[:, 0] == 0)[:, None, None], bestH, st.eye)                # failed pairs: any finite warp
        mask_before = g.mask_rows(A, active) if trace is not None else None
        rd = g.fine(A, active, Hs, bestH, res, n_dev)
        if trace is not None:
            trace.append(dict(g.trace_entry(rd, active), active=pairs, mask_before=mask_before, n=n_dev, H=bestH, res=res, inlier=inl,
                              accept=rd["accept"], gain=rd["gain"], mask_after=g.mask_rows(A, active), samples=smp, round=rnd - 1))
        acc_host[:a].copy_(rd["accept"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        yield ev                                                                    # the round's host readback: accept flags
        acc = acc_host[:a].tolist()
        nxt = []
        for k, m in enumerate(active):
            if not acc[k]:
                continue
            b = g.pairs[m]
            if st.want_lists:
                st.outs[b]["H"].append(bestH[k])
                g.collect(st.outs[b], rd, k, m)
            st.nb[b] += 1
            if g.goes_on(b):
                nxt.append(m)
        active = nxt


def _rows(t, A):
    return t if A is None else t.index_select(0, A)


class DenseGroup:
    """Pairs [lo, hi) of a batch of the Hpatch driver whose pairs share one size: the matches are cached and filtered by the
    explained-region mask every round, the fine stage is PredFlowMask (evaluation/evalHpatch/evaluation.py:184-243).  ``batch``:
    the batch's tensors (idx1, idx2, cnt of the mutual matching, Mask (B,h,w), nbH (B,), bg, IsTensor, ItTensor) and ``feats``;
    the group works on views of rows [lo, hi) of the same storage."""
    accept_mode = 0

    def __init__(self, st, batch, lo, hi):
        cut = lambda key: None if batch.get(key) is None else batch[key][lo:hi]
        self.st, self.cut, self.pairs, self.feats = st, cut, range(lo, hi), batch.get("feats")
        self.idx1, self.idx2, self.cnt = cut("idx1"), cut("idx2"), cut("cnt")
        self.Mask, self.nbH, self.bg = cut("Mask"), cut("nbH"), cut("bg")
        self.IsT, self.ItT = cut("IsTensor"), cut("ItTensor")
        self.ids = None if st.ids is None else st.ids[lo:hi]
        self.R = None if st.records is None else st.records.rows(lo, hi)
        self.h, self.w = self.Mask.shape[1], self.Mask.shape[2]
        self.featt = None

    def matches(self, A, active):
        f = self.feats
        return ops.filter_matches(self.idx1, self.idx2, self.cnt, A, self.Mask, self.bg, f["rt"], f["ct"], f["HA"], f["WA"], f["Ht"],
                                  f["Wt"])

    def target_features(self):
        if self.featt is None:
            self.featt = ops.l2norm(self.st.pipe.feat(self.ItT))

    def pred(self, A, Hs):
        """-> (PredFlowMask outputs of the active pairs, their matchability (a,h,w) for the accept kernel, the KITTI driver's flowD2)."""
        flowCoarse = ops.warp_grid(Hs, self.h, self.w)
        pm = self.st.pipe.pred_flow_mask(_rows(self.IsT, A), _rows(self.featt, A), flowCoarse)
        return pm, pm["match"][:, 0], None

    def fine(self, A, active, Hs, bestH, res, n_dev):
        pm, match, flow_d2 = self.pred(A, Hs)
        accept, gain = ops.multih_accept(match, self.Mask, self.bg, A, res, n_dev, self.nbH, self.st.maskRegionTh, self.accept_mode,
                                         bestH=bestH, flowDown8=pm["flowDown8"], match12Down8=pm["match12Down8"],
                                         match21Down8=pm["match21Down8"], flowD2=flow_d2, records=self.R)
        md2 = torch.cat((pm["match12Down8"], pm["match21Down8"]), dim=1) if self.st.want_lists else None
        return dict(pm=pm, match=match, flow_d2=flow_d2, accept=accept, gain=gain, md2=md2)

    def mask_rows(self, A, active):
        return _rows(self.Mask, A).clone()

    def trace_entry(self, rd, active):
        return dict(pm=rd["pm"], match=rd["match"])

    def collect(self, out, rd, k, m):
        out["flowDown8"].append(rd["pm"]["flowDown8"][k:k + 1])
        out["matchDown8"].append(rd["md2"][k:k + 1])

    def goes_on(self, b):
        return self.st.nb[b] <= self.st.maxCoarse


class KittiGroup(DenseGroup):
    """Pairs [lo, hi) of a batch of the KITTI driver: DenseGroup's cached matches with the two-resolution fine pass and the
    small-component filter (evaluation/evalKITTI/evaluation.py:279-336), accept mode 1, and the reference's ``while True``.  ``batch``
    also holds tensor_s / tensor_d2 / tensor_resize (B,...) and cc_th / remove_small_cc."""
    accept_mode = 1

    def __init__(self, st, batch, lo, hi):
        super().__init__(st, batch, lo, hi)
        self.tensor_s, self.tensor_d2, self.tensor_resize = self.cut("tensor_s"), self.cut("tensor_d2"), self.cut("tensor_resize")
        self.cc_th, self.remove_small_cc = batch["cc_th"], batch["remove_small_cc"]

    def target_features(self):
        pass                                             # both PredFlowMask passes of a round compute their own

    def pred(self, A, Hs):
        flow_d2, pm, match = self.st.pipe.kitti_fine_round(Hs, _rows(self.tensor_s, A), _rows(self.tensor_d2, A),
                                                           _rows(self.tensor_resize, A), (self.h, self.w), self.cc_th, self.remove_small_cc)
        return pm, match, flow_d2

    def trace_entry(self, rd, active):
        return dict(super().trace_entry(rd, active), flowD2=rd["flow_d2"])

    def collect(self, out, rd, k, m):
        super().collect(out, rd, k, m)
        out["flowD2"].append(rd["flow_d2"][k:k + 1])

    def goes_on(self, b):
        R = self.st.records
        if R is not None and self.st.nb[b] >= R.max_h:
            # the reference's ``while True`` has no round limit; a fixed-size record has: the pair stops at the record's
            # capacity and its record says so (status 4 = "capped by the driver": the reference might have gone on; a
            # truncated pair is distinguishable from one that ended on the accept test)
            R.rec[b, 1] = 4.0
            return False
        return True


class VariantCGroup(DenseGroup):
    """The pairs ``members`` of a batch of the YFCC driver whose chosen candidate targets share one shape, as a dense batch of
    their own (evaluation/evalYFCC/evaluation.py:238-275): every round RE-MATCHES -- keep map of the explained-region mask -> masked
    mutual matching (``match(fA, fB, keep, n)`` -> M1, M2, n_dev) -> and the fine stage is the cycle-checked PredFlowMask.  ``batch``:
    the group's own tensors (Mask (G,h,w), nbH, bg, IsTensor, ItTensor, featA, featB), rt, ct and gi = members on the device.  The
    slice-derived pairs / ids / records of the base class are replaced by the group's; the caller's records get the group's rows
    back with ``store_records`` after the rounds."""

    def __init__(self, st, batch, members, match):
        super().__init__(st, batch, 0, len(members))
        dev = st.pipe.dev
        self.pairs, self.match, self.rt, self.ct = members, match, batch["rt"], batch["ct"]
        self.fA, self.fB = batch["featA"], batch["featB"]
        self.gi = batch["gi"]                            # the members as an index tensor
        self.ids = self.gi.int() if st.ids is None else st.ids.index_select(0, self.gi)     # absolute batch positions when no ids were given
        self.featt = ops.l2norm(st.pipe.feat(self.ItT))
        R = st.records
        if R is not None:
            if (R.h8, R.w8) != (self.h // 8, self.w // 8):
                raise ValueError("records were built for /8 maps of %dx%d, this group's targets give %dx%d (one MultiHRecords per "
                                 "shape group)" % (R.h8, R.w8, self.h // 8, self.w // 8))
            self.R = ops.MultiHRecords(len(members), R.h8, R.w8, dev, max_h=R.max_h)
            self.R.rec[:, 2:4] = R.rec.index_select(0, self.gi)[:, 2:4]

    def matches(self, A, active):
        keep = ops.keep_mask(self.Mask, self.bg, A, self.rt, self.ct)
        return self.match(_rows(self.fA, A), _rows(self.fB, A), keep, len(active))

    def pred(self, A, Hs):
        pm = self.st.pipe.pred_flow_mask_cycle(_rows(self.IsT, A), _rows(self.featt, A), ops.warp_grid(Hs, self.h, self.w))
        return pm, pm["match"][:, 0], None

    def store_records(self):
        if self.R is not None:
            self.st.records.rec.index_copy_(0, self.gi, self.R.rec)


class RaggedGroup:
    """Pairs [lo, hi) of a ragged batch of the Hpatch driver (pairs of different sizes).  The explained-region masks (and
    background maps) of all pairs live in ONE packed buffer (ragged.ragged_multih_tables), so the filter and the accept kernel
    of a round are one launch each for all active pairs of the group.  Pairs of the slice that share (source shape, target shape)
    form a fine group: their raw images are stacked once, the target features are computed once per target shape, and every round
    runs warp_grid + PredFlowMask over the active members of all fine groups as one chain of grouped launches
    (AlignPipeline.pred_flow_mask_groups; RFX_FINE_GROUPS off: once per fine group, packed with one torch.cat each).  The round's
    matchability and /8 maps are packed in fine-group order and handed to rfx_multih_accept_ragged_f32 with per-active-pair offsets; those offsets
    and the groups' gather indices go up in ONE pinned table per round.  ``batch``: prep, feats, idx1, idx2, cnt and the fields of a
    ragged.PackedBatch: tabs, the packed Mask / bg, nbH (B,), moff (B,), geom (B,6)."""

    def __init__(self, st, batch, lo, hi):
        cut = lambda t: None if t is None else t[lo:hi]
        feats, tabs = batch["feats"], batch["tabs"]
        self.st, self.pairs, self.feats = st, range(lo, hi), feats
        self.idx1, self.idx2, self.cnt = cut(batch["idx1"]), cut(batch["idx2"]), cut(batch["cnt"])
        self.nbH, self.moff, self.geom = cut(batch["nbH"]), cut(batch["moff"]), cut(batch["geom"])
        self.ids, self.offA, self.offB = cut(st.ids), cut(feats["offA"]), cut(feats["offB"])
        self.Mask, self.bg = batch["Mask"], batch["bg"]                  # packed: the offsets are absolute
        self.gm, self.mo = tabs["geom"][lo:hi], tabs["moff"][lo:hi]
        self.R = None if st.records is None else st.records.rows(lo, hi)
        self.fine_setup(batch, lo, hi)

    def fine_setup(self, batch, lo, hi):
        """The fine groups of the slice and their stacked images."""
        IsT, self.ItT = batch["prep"]["IsTensor"][lo:hi], batch["prep"]["ItTensor"][lo:hi]
        self.make_fine_groups([(tuple(s.shape), tuple(t.shape)) for s, t in zip(IsT, self.ItT)], Is=IsT)
        self.tgroups = ragged.by_shape([tuple(t.shape) for t in self.ItT])      # the FeatureExtractor pass of the targets: per target shape
        self.have_featt = False

    def make_fine_groups(self, keys, **images):
        """The fine groups: the pairs of the slice that share ``keys[m]``, members ascending, each with its members' ``images``
        (name -> per-pair (1,3,.,.) list) stacked once."""
        self.fine_groups = [dict(members=mem, pos={m: j for j, m in enumerate(mem)}, hw=self.gm[mem[0]][:2], hw8=self.gm[mem[0]][4:6],
                                 **{name: ragged.rows(ts, mem) for name, ts in images.items()})
                            for mem in ragged.by_shape(keys).values()]

    def round_layout(self, active):
        """The round's layout: fine groups in order, each with its active members; pair k of the active list sits at match_off[k] of
        the packed matchability and at off8[k] of the packed /8 maps.  One pinned table goes up."""
        a = len(active)
        kpos = {m: k for k, m in enumerate(active)}
        rg, table, m_off, o8 = [], [0] * (2 * a), 0, 0
        for g in self.fine_groups:
            mem = [m for m in g["members"] if m in kpos]
            if not mem:
                continue
            (h, w), (h8, w8) = g["hw"], g["hw8"]
            for m in mem:
                table[kpos[m]], table[a + kpos[m]] = m_off, o8
                m_off += h * w
                o8 += h8 * w8
            ent = dict(g=g, mem=mem, kidx=None, sel=None)
            if len(mem) != a or [kpos[m] for m in mem] != list(range(a)):
                ent["kidx"] = (len(table), len(mem))
                table += [kpos[m] for m in mem]
            if len(mem) != len(g["members"]):
                ent["sel"] = (len(table), len(mem))
                table += [g["pos"][m] for m in mem]
            rg.append(ent)
        self.x0 = len(table)
        table += self.extra_table(rg, kpos, a)
        self.rg, self.table, self.T = rg, table, torch.tensor(table, dtype=torch.int64).pin_memory().to(self.st.pipe.dev, non_blocking=True)

    def matches(self, A, active):
        self.round_layout(active)
        f = self.feats
        return ops.filter_matches_ragged(self.idx1, self.idx2, self.cnt, A, self.Mask, self.bg, self.moff, self.geom, f["HA"], f["WA"],
                                         self.offA, f["Ht"], f["Wt"], self.offB)

    def extra_table(self, rg, kpos, a):
        """What a driver's round needs in the pinned table besides the offsets and gather indices (from self.x0 on)."""
        return []

    def target_features(self):
        if self.have_featt:
            return
        self.have_featt = True
        pipe, ItT, ft = self.st.pipe, self.ItT, {}
        xs = [ragged.rows(ItT, mem) for mem in self.tgroups.values()]
        if ops.fine_groups_enabled():
            fs = pipe.feat_l2norm(xs)                    # all target shapes as one chain of stages
        else:
            fs = [ops.l2norm(pipe.feat(x)) for x in xs]
        for f, mem in zip(fs, self.tgroups.values()):
            ragged.hand_back(ft, mem, f)
        for g in self.fine_groups:
            g["featt"] = ragged.rows(ft, g["members"])

    # all fine groups of a round as one chain of grouped launches: the driver's default where RFX_FINE_GROUPS is unset (a driver whose
    # grouped chain measured slower keeps False here; RFX_FINE_GROUPS=1 / 0 selects either way)
    grouped_fine = True

    def use_groups(self):
        """Whether this round's fine stage runs as one grouped chain: RFX_FINE_GROUPS where set, else the driver's ``grouped_fine``;
        never under a Profiler (ops.fine_groups_enabled)."""
        unset = str(os.environ.get("RFX_FINE_GROUPS", "")).strip() == ""
        return ops.fine_groups_enabled() and (self.grouped_fine or not unset)

    def pred_group(self, Is, featt, flowCoarse):
        """The fine pass of one fine group's active members (the per-group form)."""
        return self.st.pipe.pred_flow_mask(Is, featt, flowCoarse)

    def pred_groups(self, Is_list, featt_list, Hs_list, hw_list, out):
        """The fine pass of all fine groups' active members as one chain of grouped launches."""
        return self.st.pipe.pred_flow_mask_groups(Is_list, featt_list, Hs_list, hw_list, out=out)

    def take(self, ent, t, key):
        """The rows of ``t`` that round-group entry ``ent`` works on: key "sel" = its active members out of a fine group's stacked
        tensor, "kidx" = its pairs out of a tensor over the round's active list (None: all rows, ``t`` itself)."""
        return t if ent[key] is None else t.index_select(0, self.T[ent[key][0]:ent[key][0] + ent[key][1]])

    @staticmethod
    def pack(ts):
        """Per-fine-group tensors -> ONE flat buffer in fine-group order (one group: a view of its own tensor)."""
        return ragged.rows([t.reshape(-1) for t in ts], range(len(ts)))

    def max_hw(self, active):
        return max(self.gm[m][0] * self.gm[m][1] for m in active)

    def where(self):
        """After a round's fine stage: pair m -> (its round-group entry, its row there); with ``want_lists`` every entry gets ``md2``,
        both matchability maps as the two channels of matchDown8."""
        where = {}
        for ent in self.rg:
            if self.st.want_lists:
                ent["md2"] = torch.cat((ent["pm"]["match12Down8"], ent["pm"]["match21Down8"]), dim=1)
            for j, m in enumerate(ent["mem"]):
                where[m] = (ent, j)
        return where

    def fine(self, A, active, Hs, bestH, res, n_dev):
        rg, T, a, take = self.rg, self.T, len(active), self.take
        if self.use_groups():
            # fine stage: all fine groups as ONE chain of grouped launches; its packed outputs are in fine-group order, which is the
            # order matches() laid the round's offsets out in -- they go to the accept kernel as they are
            packed = {}
            pms = self.pred_groups([take(e, e["g"]["Is"], "sel") for e in rg], [take(e, e["g"]["featt"], "sel") for e in rg],
                                   [take(e, Hs, "kidx") for e in rg], [e["g"]["hw"] for e in rg], packed)
            for ent, pm in zip(rg, pms):
                ent["pm"] = pm
            pack = lambda key: packed[key]
        else:
            # RFX_FINE_GROUPS off: per fine group, the dense kernels
            for ent in rg:
                g = ent["g"]
                h, w = g["hw"]
                ent["pm"] = self.pred_group(take(ent, g["Is"], "sel"), take(ent, g["featt"], "sel"),
                                            ops.warp_grid(take(ent, Hs, "kidx"), h, w))
            pack = lambda key: self.pack([e["pm"][key] for e in rg])
        accept, gain = ops.multih_accept_ragged(pack("match"), T[:a], self.Mask, self.bg, self.moff, self.geom, A, res, n_dev, self.nbH,
                                                self.st.maskRegionTh, 0, self.max_hw(active), bestH=bestH,
                                                flowDown8=pack("flowDown8"), match12Down8=pack("match12Down8"),
                                                match21Down8=pack("match21Down8"), off8=T[a:2 * a], records=self.R)
        return dict(accept=accept, gain=gain, where=self.where())

    def mask_rows(self, A, active):
        return [self.Mask[self.mo[m]:self.mo[m] + self.gm[m][0] * self.gm[m][1]].view(self.gm[m][:2]).clone() for m in active]

    def trace_entry(self, rd, active):
        where = rd["where"]
        return dict(pm=[{key: v[where[m][1]:where[m][1] + 1] for key, v in where[m][0]["pm"].items()} for m in active])

    def collect(self, out, rd, k, m):
        ent, j = rd["where"][m]
        out["flowDown8"].append(ent["pm"]["flowDown8"][j:j + 1])
        out["matchDown8"].append(ent["md2"][j:j + 1])

    def goes_on(self, b):
        return self.st.nb[b] <= self.st.maxCoarse


class RaggedVariantCGroup(RaggedGroup):
    """Pairs [lo, hi) of a ragged batch of the YFCC driver (pairs -- and chosen candidate targets -- of different sizes): RaggedGroup
    with the differences VariantCGroup has over DenseGroup.  Every round RE-MATCHES: ONE rfx_keep_mask_ragged_f32 for the active pairs
    (keep map of the explained-region mask + background, written into each pair's own row, and the round's nB table: rt * ct at the
    active positions, 0 elsewhere), ONE masked ragged mutual matching that skips the inactive pairs on that table, ONE gather of the
    active pairs' matches.  The fine stage is the cycle-checked PredFlowMask over the active members of all fine groups as one chain
    of grouped launches (AlignPipeline.pred_flow_mask_cycle_groups; RFX_FINE_GROUPS off: once per fine group); its matchability maps
    are packed in fine-group order for the ragged accept kernel (mode 0).  ``batch``: RaggedGroup's (idx1 /
    idx2 / cnt None: nothing is cached) with ``feats`` = the CHOSEN candidates' featB / nB / offB and the tables of
    ragged.ragged_variant_c_tables."""
    def __init__(self, st, batch, lo, hi):
        super().__init__(st, batch, lo, hi)
        f, dev = self.feats, st.pipe.dev
        self.fA, self.fB, self.nA_dev = f["featA"][lo:hi], f["featB"][lo:hi], f["nA_dev"][lo:hi]
        self.nA, self.nB, self.ldB, self.cap = f["nA"][lo:hi], f["nB"][lo:hi], f["ldB"], f["cap"]
        self.keep = torch.zeros((hi - lo, self.ldB), dtype=torch.float32, device=dev)
        self.nB_round = torch.zeros(hi - lo, dtype=torch.int32, device=dev)

    def matches(self, A, active):
        self.round_layout(active)
        f = self.feats
        self.nB_round.zero_()
        max_nB = max(self.nB[m] for m in active)
        ops.keep_mask_ragged(self.Mask, self.bg, self.moff, self.geom, A, self.ldB, max_nB, keep=self.keep, nB_round=self.nB_round)
        idx1, idx2, cnt = ops.mutual_nn_ragged(self.fA, self.fB, self.nA_dev, self.nB_round, max(self.nA[m] for m in active), max_nB,
                                               maskB=self.keep, score_chunk=self.st.pipe.score_chunk, cap=self.cap)
        n_dev = _rows(cnt, A)
        M1, M2 = ops.gather_matches_ragged(_rows(idx1, A), _rows(idx2, A), n_dev, f["HA"], f["WA"], _rows(self.offA, A), f["Ht"], f["Wt"],
                                           _rows(self.offB, A))
        return M1, M2, n_dev

    def pred_group(self, Is, featt, flowCoarse):
        return self.st.pipe.pred_flow_mask_cycle(Is, featt, flowCoarse)

    def pred_groups(self, Is_list, featt_list, Hs_list, hw_list, out):
        return self.st.pipe.pred_flow_mask_cycle_groups(Is_list, featt_list, Hs_list, hw_list, out=out)


class RaggedKittiGroup(RaggedGroup):
    """Pairs [lo, hi) of a ragged batch of the KITTI driver: RaggedGroup with the differences KittiGroup has over DenseGroup -- the
    two-resolution fine pass, the small-component filter, accept mode 1, no cached target features, the reference's ``while True``
    with the capacity stop, flowD2 collected and traced.  The packed masks live at the ORIGINAL target sizes
    (ragged.ragged_kitti_tables).  A fine group is the pairs of the slice that share (source ORIGINAL shape, target ORIGINAL shape):
    the source is sampled at its original size and the outputs live at the original target size, so two pairs whose resized shapes
    coincide but whose originals differ are two groups.  A round runs the two-resolution fine pass over the active members of all fine
    groups as one chain of grouped launches (pipeline.kitti_fine_round_groups; RFX_FINE_GROUPS off: pipeline.kitti_fine_round, without
    its dense filter, once per fine group, the matchability maps packed in fine-group order), then ONE rfx_remove_small_cc_ragged_f32
    on a copy of the packed maps for all active pairs and ONE ragged accept (mode 1) with the flowD2 store.  ``batch``: RaggedGroup's plus tensor_s /
    tensor_d2 / tensor_resize (per-pair (1,3,.,.) lists), d2 (per-pair (hd2, wd2) of the half-resolution /8 flow), d2dims (B,2) on the
    device, cc_th / remove_small_cc."""
    accept_mode = 1
    goes_on = KittiGroup.goes_on

    def fine_setup(self, batch, lo, hi):
        Ts, Td2, Tr = batch["tensor_s"][lo:hi], batch["tensor_d2"][lo:hi], batch["tensor_resize"][lo:hi]
        self.cc_th, self.remove_small_cc = batch["cc_th"], batch["remove_small_cc"]
        self.d2, self.d2dims = batch["d2"][lo:hi], batch["d2dims"][lo:hi]
        self.make_fine_groups([(tuple(t.shape), hw[:2]) for t, hw in zip(Ts, self.gm)], Is=Ts, d2=Td2, resize=Tr)

    def target_features(self):
        pass                                             # both PredFlowMask passes of a round compute their own

    def extra_table(self, rg, kpos, a):
        # flowD2 offsets per active pair (packed in fine-group order like the other maps), then the filter's (h, w, max_area) rows
        offd2, dims, pos = [0] * a, [0] * (3 * a), 0
        for ent in rg:
            for m in ent["mem"]:
                k = kpos[m]
                offd2[k] = pos
                pos += self.d2[m][0] * self.d2[m][1]
                h, w = self.gm[m][:2]
                dims[3 * k:3 * k + 3] = h, w, ops.cc_max_area(h * w, self.cc_th) if self.cc_th > 0 else 0
        return offd2 + dims

    def fine(self, A, active, Hs, bestH, res, n_dev):
        rg, T, a, gm, x0, take = self.rg, self.T, len(active), self.gm, self.x0, self.take
        pipe = self.st.pipe
        if self.use_groups():
            # both resolutions' fine passes: all fine groups as ONE chain of grouped launches, packed in fine-group order
            packed = {}
            per_group = pipe.kitti_fine_round_groups([take(e, Hs, "kidx") for e in rg], [take(e, e["g"]["Is"], "sel") for e in rg],
                                                     [take(e, e["g"]["d2"], "sel") for e in rg], [take(e, e["g"]["resize"], "sel") for e in rg],
                                                     [e["g"]["hw"] for e in rg], out=packed)
            for ent, r in zip(rg, per_group):
                ent["flow_d2"], ent["pm"], ent["match"] = r
            pack, match, flow_d2, shared = (lambda key: packed[key]), packed["match"], packed["flowD2"], True
        else:
            for ent in rg:
                g = ent["g"]
                ent["flow_d2"], ent["pm"], ent["match"] = pipe.kitti_fine_round(take(ent, Hs, "kidx"), take(ent, g["Is"], "sel"),
                                                                                take(ent, g["d2"], "sel"), take(ent, g["resize"], "sel"),
                                                                                g["hw"], cc_th=0)
            pack = lambda key: self.pack([e["pm"][key] for e in rg])
            match, flow_d2, shared = self.pack([e["match"] for e in rg]), self.pack([e["flow_d2"] for e in rg]), len(rg) == 1
        max_hw = self.max_hw(active)
        if self.cc_th > 0:                                                              # evalKITTI/evaluation.py:321
            if self.remove_small_cc is None:
                if shared:
                    match = match.clone()            # the storage of PredFlowMask's own maps: keep its output (trace) as it is
                ops.remove_small_cc_ragged(match, T[:a], T[x0 + a:x0 + 4 * a].to(torch.int32).view(a, 3), self.cc_th, 0.99,
                                           inplace=True, max_hw=max_hw)
            else:                                    # an injected host filter, called in pair order: one round trip
                mh = match.cpu().numpy().copy()
                for k, m in enumerate(active):
                    o, (h, w) = self.table[k], gm[m][:2]
                    mh[o:o + h * w] = self.remove_small_cc(mh[o:o + h * w].reshape(h, w), 0.99, self.cc_th).reshape(-1)
                match = torch.from_numpy(mh).to(pipe.dev)
        accept, gain = ops.multih_accept_ragged(match, T[:a], self.Mask, self.bg, self.moff, self.geom, A, res, n_dev, self.nbH,
                                                self.st.maskRegionTh, self.accept_mode, max_hw, bestH=bestH, flowDown8=pack("flowDown8"),
                                                match12Down8=pack("match12Down8"), match21Down8=pack("match21Down8"), off8=T[a:2 * a],
                                                records=self.R, flowD2=flow_d2, offd2=T[x0:x0 + a],
                                                d2dims=self.d2dims if self.R is None else None)
        return dict(accept=accept, gain=gain, where=self.where(), match=match)

    def trace_entry(self, rd, active):
        where, tab, gm = rd["where"], self.table, self.gm
        cut = lambda k, m: rd["match"][tab[k]:tab[k] + gm[m][0] * gm[m][1]].view(gm[m][:2])
        return dict(super().trace_entry(rd, active), flowD2=[where[m][0]["flow_d2"][where[m][1]:where[m][1] + 1] for m in active],
                    match=[cut(k, m) for k, m in enumerate(active)])

    def collect(self, out, rd, k, m):
        super().collect(out, rd, k, m)
        ent, j = rd["where"][m]
        out["flowD2"].append(ent["flow_d2"][j:j + 1])
