"""The fp32 convolution dispatch (csrc/conv_dispatch.h) against a frozen table of ids: tests/golden/conv_dispatch_ids.json holds what
rfx_conv2d_kernel_id, rfx_conv3x3_kernel_id, rfx_conv3x3_conv1x1_kernel_id and rfx_conv2d_tile_variant answered BEFORE the dispatch
became one decision function (its "library_commit" names the build that produced it; scripts/conv_dispatch_ids.py dump) -- for every
convolution geometry of the nets, N in {1, 2, 4, 16, 64}, the pyramid's six map sizes, k_chunk 0 and 4, not recording and recording,
and a reduced grid under each environment switch alone at a non-default value.  The built library must reproduce every entry.  The
library reads its switches once per process: each setting is evaluated in a child process of its own (host code only, no GPU).

The same table is asked of the header alone, compiled by the host compiler (no HIP) into a stand-alone program
(tests/host/conv_dispatch_walk.cpp) that takes "recording" as the plain argument the decision functions take; built by hand with
-fsanitize=address,undefined the same program is the dispatch's sanitizer run."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PATH = os.path.join(ROOT, "tests", "golden", "conv_dispatch_ids.json")
_spec = importlib.util.spec_from_file_location("conv_dispatch_ids", os.path.join(ROOT, "scripts", "conv_dispatch_ids.py"))
ids = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ids)

with open(TABLE_PATH) as _f:
    TABLE = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def built_library():
    if not os.path.exists(ids.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()


def test_table_covers_the_grid():
    geoms = [tuple(g) for g in TABLE["geometries"]]
    assert geoms == ids.net_geometries()
    assert TABLE["settings"]["default"]["grid"] == dict(N=[1, 2, 4, 16, 64], maps=[list(m) for m in ids.MAPS])
    assert set(TABLE["settings"]) == {"default"} | {"%s=%s" % kv for kv in ids.SWITCHES}
    for name, s in TABLE["settings"].items():
        assert len(s["values"]) == 2 * sum(1 for _ in ids.queries(geoms, s["grid"])), name


@pytest.mark.parametrize("setting", sorted(TABLE["settings"]))
def test_library_reproduces_every_id(setting, monkeypatch):
    monkeypatch.delenv("RFX_LIB", raising=False)
    s = TABLE["settings"][setting]
    got = ids.run_setting(TABLE_PATH, setting, s["env"])
    geoms = [tuple(g) for g in TABLE["geometries"]]
    asked = [(q, rec) for q in ids.queries(geoms, s["grid"]) for rec in ("eager", "recording")]
    wrong = [(q, rec, g, w) for (q, rec), g, w in zip(asked, got, s["values"]) if g != w]
    assert len(got) == len(s["values"]) and not wrong, "%d of %d differ; (query, mode, got, table): %s" % (len(wrong), len(got), wrong[:5])


@pytest.fixture(scope="module")
def walk_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_dispatch") / "conv_dispatch_walk")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "conv_dispatch_walk.cpp")])
    return exe


@pytest.mark.parametrize("setting", sorted(TABLE["settings"]))
def test_header_alone_reproduces_every_id(walk_program, setting):
    s = TABLE["settings"][setting]
    geoms = [tuple(g) for g in TABLE["geometries"]]
    lines = ["%s %d %s" % (fn, rec, " ".join(map(str, args))) for fn, args in ids.queries(geoms, s["grid"]) for rec in (0, 1)]
    env = {k: v for k, v in os.environ.items() if k not in ids.ALL_SWITCHES}
    env.update(s["env"])
    r = subprocess.run([walk_program], input="\n".join(lines) + "\n", env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    assert [int(v) for v in r.stdout.split()] == s["values"]


@pytest.mark.parametrize("setting", ["default", "RFX_CONV_DIRECT=0", "RFX_CONV_S2=0", "RFX_CONV_WS=1", "RFX_CONV_FORCE_VARIANT=2", "RFX_C3_TAIL_CHUNK=0"])
def test_every_decided_instance_has_a_table_entry(setting, monkeypatch):
    """The launch entry points, called while a grouped launch records (host code only: scripts/conv_dispatch_ids.py record), over the
    setting's grid -- also against the library's own rule and on an unaligned input: each finds its decided instance in its family's
    table (RFX_OK, not the RFX_E_ARG of a missing entry)."""
    monkeypatch.delenv("RFX_LIB", raising=False)
    rcs = ids.run_setting(TABLE_PATH, setting, TABLE["settings"][setting]["env"], mode="record")
    assert len(rcs) > 100 and set(rcs) == {0}, {rc: rcs.count(rc) for rc in set(rcs)}
