#!/usr/bin/env python
"""Aligned source images (uint8 HWC) of a batch of pairs from their device records, in ONE process:

    (a) chain:    u8_to_f32 of the sources, one ops.assemble_records call, per pair ops.grid_sample and the byte conversion
                  clamp(0, 1).mul(255).byte() -> HWC; with the overlay also (img + tgt) >> 1 in torch
    (b) one call: ops.warp_records_u8 on the whole batch (rfx_warp_records_u8: one launch, no float intermediate)

Two cases.  "16 x 480x640": 16 pairs, 60 x 80 records at 480 x 640, 4..11 homographies per pair, multiH on, with and without the
cycle check (th 0.2 / 0.45) and the overlay; sources one (16,480,640,3) tensor.  "8 mixed": the first eight sizes of the mixed-size
set of the ragged benches (ragged_bench.SIZES), maps at the sizes' multiples of 8, sources at the sizes themselves, ragged records,
cycle check and overlay on.  Record contents: synth.assembly_arrays, as in assemble_records_bench.py.  Wall clock around INNER
consecutive runs between two synchronisations, per run; the two paths alternating, REPS repetitions each: median (min - max),
milliseconds.  Peak allocation of each path above what is allocated before it, in MiB.  Both paths' bytes are compared.
-> profiles/warp_image_bench.json

    python scripts/ubench/warp_image_bench.py [--out profiles/warp_image_bench.json] [--reps 5]

The byte-store / LDS-staged question (scripts/ubench/warp_image_staged.hip, built as its header says): with --staged-lib PATH that
library's rfx_warp_records_u8 is bound beside the product's and timed as a third path, alternating with the other two in the same
process, its bytes compared with the product's; recorded per case under "lds_staged".
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "ransac-flow_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rfx import _lib, ops, synth  # noqa: E402
from ragged_bench import SIZES  # noqa: E402

MAX_H, INNER = 11, 10


def fill(views, seed, n, h8, w8, dev):
    nbH, Hs, f8, m8 = views
    fd, _, pm, md = synth.assembly_arrays(seed, n, h8, w8)
    f8[:n], Hs[:n], m8[:n] = (torch.from_numpy(np.ascontiguousarray(a)).float().to(dev) for a in (fd, pm, md))
    nbH.fill_(float(n))


def dense_records(B, h8, w8, nb, dev):
    R = ops.MultiHRecords(B, h8, w8, dev, max_h=MAX_H)
    nbH, _, Hs, f8, m8, _ = R.views()
    for b, n in enumerate(nb):
        fill((nbH[b], Hs[b], f8[b], m8[b]), 100 + b, n, h8, w8, dev)
    return R


def ragged_records(sizes8, nb, dev):
    R = ops.MultiHRecordsRagged([s[0] for s in sizes8], [s[1] for s in sizes8], dev, max_h=MAX_H)
    for b, n in enumerate(nb):
        v = R.views(b)
        fill((v[0], v[2], v[3], v[4]), 200 + b, n, sizes8[b][0], sizes8[b][1], dev)
    return R


def chain(R, srcs, tgts, th, cycle):
    """srcs: a (B,H,W,3) tensor or a list; -> per pair (img, overlay | None) uint8 HWC."""
    if isinstance(srcs, torch.Tensor):
        raw = ops.u8_to_f32(srcs)[0]
        raws = [raw[b:b + 1] for b in range(R.B)]
    else:
        raws = [ops.u8_to_f32(s[None])[0] for s in srcs]
    fg = ops.assemble_records(R, th, True, cycle)[0]
    out = []
    for b in range(R.B):
        img = ops.grid_sample(raws[b], fg[b][None]).clamp(0, 1).mul(255).byte()[0].permute(1, 2, 0).contiguous()
        ov = ((img.to(torch.int32) + tgts[b].to(torch.int32)) >> 1).to(torch.uint8) if tgts is not None else None
        out.append((img, ov))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / INNER


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def cases(dev):
    g = torch.Generator().manual_seed(11)
    img = lambda *shape: torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev)
    B = 16
    nb = [int(x) for x in np.random.RandomState(7).randint(4, MAX_H + 1, B)]
    R = dense_records(B, 60, 80, nb, dev)
    S, T = img(B, 480, 640, 3), img(B, 480, 640, 3)
    for cycle, th in ((True, 0.2), (False, 0.45)):
        for overlay in (False, True):
            yield ("16 x 480x640, cycle %s, overlay %s" % ("on" if cycle else "off", "on" if overlay else "off"),
                   dict(pairs=B, nbH=nb, cycle=cycle, th=th, overlay=overlay), R, S, T if overlay else None, th, cycle)
    sizes = SIZES[:8]
    sizes8 = [(h // 8, w // 8) for h, w in sizes]
    nb = [int(x) for x in np.random.RandomState(8).randint(1, MAX_H + 1, 8)]
    R = ragged_records(sizes8, nb, dev)
    S = [img(h, w, 3) for h, w in sizes]
    T = [img(8 * h, 8 * w, 3) for h, w in sizes8]
    yield ("8 mixed, cycle on, overlay on", dict(pairs=8, nbH=nb, sizes=sizes, cycle=True, th=0.2, overlay=True), R, S, T, 0.2, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_image_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--staged-lib", help="the library built from scripts/ubench/warp_image_staged.hip: timed as a third path")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    product_fn = lib.rfx_warp_records_u8
    staged_fn = None
    if a.staged_lib:
        staged_fn = ctypes.CDLL(os.path.abspath(a.staged_lib)).rfx_warp_records_u8
        staged_fn.restype, staged_fn.argtypes = _lib.SIGNATURES["rfx_warp_records_u8"]

    def with_fn(fn, run):
        """run() with the binding's rfx_warp_records_u8 set to ``fn`` (ops looks the entry point up by name at every call)."""
        def call():
            lib.rfx_warp_records_u8 = fn
            try:
                return run()
            finally:
                lib.rfx_warp_records_u8 = product_fn
        return call
    rec = dict(what="aligned source images (uint8 HWC) of a batch from its device records: (a) u8_to_f32, one assemble_records call, per pair "
                    "grid_sample and the byte conversion (and the overlay in torch), (b) one ops.warp_records_u8 call; wall clock around %d "
                    "consecutive runs between synchronisations, per run, alternating in one process, %d repetitions each, milliseconds; peak "
                    "allocation above the inputs, MiB" % (INNER, a.reps),
               device=torch.cuda.get_device_name(0), reps=a.reps, cases={})
    for name, info, R, S, T, th, cycle in cases(dev):
        run_b = lambda: ops.warp_records_u8(R, S, th, True, cycle, tgt=T)
        run_c = with_fn(staged_fn, run_b) if staged_fn else None
        got = run_b()
        run_a = lambda: chain(R, S, T, th, cycle)
        want = run_a()
        same = all(torch.equal(w[0], got[0][b]) and (T is None or torch.equal(w[1], got[1][b])) for b, w in enumerate(want))
        del want
        if run_c:
            alt = run_c()
            same_c = all(torch.equal(x, y) for x, y in zip(alt[0], got[0])) and (T is None or all(torch.equal(x, y) for x, y in zip(alt[1], got[1])))
            del alt
        ta, tb, tc = [], [], []
        for _ in range(a.reps):
            ta.append(wall(run_a))
            tb.append(wall(run_b))
            if run_c:
                tc.append(wall(run_c))
        case = dict(info, byte_equal=same, chain_ms=stats(ta), one_call_ms=stats(tb),
                    chain_over_one_call_median=statistics.median(ta) / statistics.median(tb),
                    one_call_slowest_below_chain_fastest=max(tb) < min(ta), chain_peak_mib=peak_mib(run_a), one_call_peak_mib=peak_mib(run_b))
        if run_c:
            case["lds_staged"] = dict(one_call_ms=stats(tc), byte_equal_to_product=same_c,
                                      byte_stores_over_staged_median=statistics.median(tb) / statistics.median(tc),
                                      staged_slowest_below_byte_stores_fastest=max(tc) < min(tb),
                                      byte_stores_slowest_below_staged_fastest=max(tb) < min(tc))
        del got
        rec["cases"][name] = case
        print(name, json.dumps(case))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
