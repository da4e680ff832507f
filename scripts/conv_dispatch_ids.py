"""The kernel-instance ids of the fp32 convolution dispatch (include/rfx_api.h: rfx_conv2d_kernel_id, rfx_conv3x3_kernel_id,
rfx_conv3x3_conv1x1_kernel_id, rfx_conv2d_tile_variant) over a grid of launches, as a table a later build is held to
(tests/test_conv_dispatch_cpu.py, tests/golden/conv_dispatch_ids.json).  Needs no GPU: the id functions are host code.

    python scripts/conv_dispatch_ids.py dump OUT.json       write the table of the library RFX_LIB names (default: the built one)
    python scripts/conv_dispatch_ids.py eval TABLE.json SETTING    print the values of one setting of TABLE as a JSON list
    python scripts/conv_dispatch_ids.py record TABLE.json SETTING  print the return codes of the launch entry points, recording

The library reads its switches once per process, so every setting (the default environment over the full grid, each switch alone at
a non-default value over a reduced grid) is evaluated by an ``eval`` child of its own, which loads nothing but the library."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "ransac-flow_amd", "librfx.so")

MAPS = [(15, 20), (25, 33), (30, 40), (60, 80), (120, 160), (240, 320)]      # the pyramid's map sizes (output H x W)
FULL = dict(N=[1, 2, 4, 16, 64], maps=MAPS)
REDUCED = dict(N=[1, 64], maps=[(25, 33), (240, 320)])
SWITCHES = [("RFX_CONV_FORCE_VARIANT", "0"), ("RFX_CONV_FORCE_VARIANT", "2"), ("RFX_CONV_WS", "1"), ("RFX_CONV_DIRECT", "0"),
            ("RFX_CONV_S2", "0"), ("RFX_CONV_1X1", "0"), ("RFX_C1_CHUNK", "0"), ("RFX_C1_CHUNK", "1024"), ("RFX_CONV_VECB", "0"),
            ("RFX_C3_CHUNK", "0"), ("RFX_C3_S2_CHUNK", "0"), ("RFX_C3_TAIL_CHUNK", "0"), ("RFX_C3_WIDE", "0"),
            ("RFX_GROUP_UNIFORM", "0"),
            ("RFX_S2_TM", "1")]      # read by no source since the dispatch became one function: kept to show the ids never saw it
ALL_SWITCHES = sorted({k for k, _ in SWITCHES})


def net_geometries():
    """Sorted (Cin, Cout, KH, KW, stride, pad) of every convolution of every net (the plans tests/test_conv_routes_cpu.py walks)."""
    sys.path[:0] = [os.path.join(ROOT, "ransac-flow_amd"), os.path.join(ROOT, "tests")]
    from rfx import nets, segnet, weights
    from test_conv_routes_cpu import _walk
    objs = [nets.ResNet50Trunk(weights.resnet50_trunk_sd(0), "cpu"), nets.FeatureExtractorNet(weights.feature_extractor_sd(1), "cpu"),
            nets.NetFlowCoarseNet(weights.net_flow_coarse_sd(2), device="cpu"), nets.NetMatchabilityNet(weights.net_matchability_sd(3), device="cpu"),
            segnet.SegEncoder(weights.seg_encoder_sd(4), "cpu"), segnet.SegDecoder(weights.seg_decoder_sd(5), "cpu")]
    return sorted({(p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad) for o in objs for _, p in _walk(o)})


def queries(geoms, grid):
    """Every (function, arguments) of one setting, in the order of its value list; each is asked not recording, then recording."""
    for N in grid["N"]:
        for H, W in grid["maps"]:
            for Cin, Cout, KH, KW, s, p in geoms:
                yield "rfx_conv2d_kernel_id", (N, Cin, Cout, KH, KW, s, p, H, W)
                if (KH, KW, s, p) == (3, 3, 1, 1) and Cin >= 8:
                    for k_chunk in (0, 4):
                        yield "rfx_conv3x3_kernel_id", (N, Cin, Cout, H, W, k_chunk)
            for Cout in sorted({g[1] for g in geoms}):
                yield "rfx_conv2d_tile_variant", (N, Cout, H, W)
            for Cmid in (64, 128):
                yield "rfx_conv3x3_conv1x1_kernel_id", (N, H, W, Cmid)


def evaluate(table, setting):
    lib = ctypes.CDLL(os.environ.get("RFX_LIB") or DEFAULT_LIB)
    geoms = [tuple(g) for g in table["geometries"]]
    out = []
    for fn, args in queries(geoms, table["settings"][setting]["grid"]):
        out.append(getattr(lib, fn)(*args))
        assert lib.rfx_group_begin() == 0                  # recording: neither call touches HIP
        out.append(getattr(lib, fn)(*args))
        lib.rfx_group_abort()
    return out


def record(table, setting):
    """Return code of every launch entry point over the setting's grid while a grouped launch records: the entry point decides,
    finds the instance in its family's table and records it (no HIP call, the dummy pointers are never read) -- RFX_E_ARG would be a
    decided instance without a table entry.  Called whatever the ids say, as a caller may (RFX_CONV_DIRECT=0 / RFX_CONV_S2=0: against
    the rule); input pointers aligned and not.  The instances without a grouped form (Cin % 8 != 0) launch at once: left out."""
    lib = ctypes.CDLL(os.environ.get("RFX_LIB") or DEFAULT_LIB)
    P, p, grid, out = ctypes.c_void_p, 1 << 20, table["settings"][setting]["grid"], []
    for Cin, Cout, KH, KW, s, pad in (tuple(g) for g in table["geometries"]):
        for N in grid["N"]:
            for H, W in grid["maps"]:
                assert lib.rfx_group_begin() == 0
                Hin, Win = (H - 1) * s + KH - 2 * pad, (W - 1) * s + KW - 2 * pad      # an input that gives an H x W output
                for x in (p, p + 4):
                    out.append(lib.rfx_conv2d_f32(P(x), P(p), P(p), None, None, None, P(p), N, Cin, Hin, Win, Cout, KH, KW, s, pad, 1, None))
                if (KH, KW, pad) == (3, 3, 1) and Cin % 8 == 0 and s == 1:
                    out += [lib.rfx_conv3x3_f32(P(p), P(p), None, None, None, P(p), N, Cin, H, W, Cout, 1, kc, None) for kc in (0, 4)]
                    if Cout in (64, 128):
                        out.append(lib.rfx_conv3x3_conv1x1_f32(P(p), P(p), None, None, 1, P(p), P(p), P(p), None, 1, P(p), N, Cin, H, W,
                                                               Cout, 4 * Cout, None))
                if (KH, KW, pad) == (3, 3, 1) and Cin % 8 == 0 and s == 2:
                    out.append(lib.rfx_conv3x3_s2_f32(P(p), P(p), None, None, None, P(p), N, Cin, Hin, Win, Cout, 1, None))
                lib.rfx_group_abort()
    return out


def run_setting(table_path, setting, env_pairs, mode="eval"):
    env = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
    env.update(env_pairs)
    return json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), mode, table_path, setting], env=env))


def dump(out_path):
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    table = dict(produced_by="scripts/conv_dispatch_ids.py dump", library_commit=commit, geometries=net_geometries(),
                 settings={"default": dict(env={}, grid=FULL)})
    for k, v in SWITCHES:
        table["settings"]["%s=%s" % (k, v)] = dict(env={k: v}, grid=REDUCED)
    with open(out_path, "w") as f:
        json.dump(table, f)
    for name, s in table["settings"].items():
        s["values"] = run_setting(out_path, name, s["env"])
    with open(out_path, "w") as f:
        json.dump(table, f, separators=(",", ":"))
    print("%s: %d settings, %d values, library of %s" % (out_path, len(table["settings"]),
                                                        sum(len(s["values"]) for s in table["settings"].values()), commit))


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        with open(sys.argv[2]) as f:
            print(json.dumps((record if sys.argv[1] == "record" else evaluate)(json.load(f), sys.argv[3])))
