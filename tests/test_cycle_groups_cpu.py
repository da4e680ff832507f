"""The cycle-checked fine stage for all shape groups, host side: the C ABI surface of rfx_cycle_tail_f32 (header prototype against
the ctypes binding, argument for argument), the ABI revision, and the Python surface (ops.cycle_tail, the three grouped pipeline
methods, the drivers' switch).  Nothing is launched."""
import ctypes
import inspect
import os
import re

import pytest

from rfx import _lib, ops, pipeline, rounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "rfx_api.h")).read()


def test_cycle_tail_prototype_and_binding_agree_argument_for_argument():
    hdr = _header()
    bare = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = {n: (r, a) for r, n, a in re.findall(r"\b(int|size_t)\s+(rfx_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", bare, flags=re.S)}
    assert "rfx_cycle_tail_f32" in protos and "rfx_cycle_tail_f32" in _lib.SIGNATURES
    ret, args = protos["rfx_cycle_tail_f32"]
    res, argtypes = _lib.SIGNATURES["rfx_cycle_tail_f32"]
    assert ret == "int" and res is ctypes.c_int
    kinds = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}
    want, names = [], []
    for p in args.split(","):
        d = " ".join(p.split())
        want.append(ctypes.c_void_p if "*" in d else kinds[d.rsplit(" ", 1)[0].replace("const ", "").strip()])
        names.append(d.rsplit(" ", 1)[1].lstrip("*"))
    assert want == list(argtypes), (want, argtypes)
    assert names == ["flowDown8", "match12Down8", "match12_stride", "match21Down8", "match21_stride", "coarseGrid", "flow12", "match", "N",
                     "hd", "wd", "Hc", "Wc", "H", "W", "stream"]
    # the entry cites the reference lines it replaces
    for cite in ("evalYFCC/evaluation.py:47-58", "evalKITTI/evaluation.py:66-81", "evalKITTI/evaluation.py:302"):
        assert cite in hdr, cite


def test_abi_revision_is_17_an_addition():
    assert int(re.search(r"#define RFX_ABI_VERSION (\d+)", _header()).group(1)) == _lib.ABI_VERSION == 17
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rfx_abi_version() == 17 and hasattr(lib, "rfx_cycle_tail_f32")
        # refusals that are answered before any HIP call
        one = ctypes.c_void_p(8)
        args = lambda **kw: [kw.get("fd", one), one, 35, one, 35, one, one, one, kw.get("N", 1), kw.get("hd", 5), 7, 40, 56, kw.get("H", 40),
                             56, None]
        assert lib.rfx_cycle_tail_f32(*args(fd=None)) != 0
        assert lib.rfx_cycle_tail_f32(*args(N=0)) != 0 and lib.rfx_cycle_tail_f32(*args(hd=0)) != 0 and lib.rfx_cycle_tail_f32(*args(H=-1)) != 0
        a = args(N=2)
        a[2] = 34                                                            # a plane stride below hd * wd with two images
        assert lib.rfx_cycle_tail_f32(*a) != 0


def test_python_surface():
    assert list(inspect.signature(ops.cycle_tail).parameters) == ["flowDown8", "match12Down8", "match21Down8", "coarseGrid", "out_hw",
                                                                  "flow12_out", "match_out"]
    assert all(p.default is None for n, p in inspect.signature(ops.cycle_tail).parameters.items() if n in ("out_hw", "flow12_out", "match_out"))
    P = pipeline.AlignPipeline
    par = lambda f: list(inspect.signature(f).parameters)[1:]
    assert par(P.pred_flow_mask_cycle_groups) == ["Is_list", "featt_list", "Hs_list", "hw_list", "out"]
    assert par(P.pred_flow_mask_kitti_groups) == ["IsSample_list", "ItSample_list", "fcs", "out_hw_list", "out"]
    assert par(P.kitti_fine_round_groups)[:5] == ["Hs_list", "tensor_s_list", "tensor_d2_list", "tensor_resize_list", "org_hw_list"]
    for f, names in ((P.pred_flow_mask_cycle_groups, ("out",)), (P.pred_flow_mask_kitti_groups, ("out_hw_list", "out")),
                     (P.kitti_fine_round_groups, par(P.kitti_fine_round_groups)[5:])):
        assert all(inspect.signature(f).parameters[n].default is None for n in names), f.__name__
    # the one-group methods keep their signatures
    assert par(P.pred_flow_mask_cycle) == ["IsTensor", "featt", "flowCoarse"]
    assert par(P.pred_flow_mask_kitti) == ["IsSample", "ItSample", "flowCoarse", "out_hw"]
    assert par(P.kitti_fine_round) == ["Hs", "tensor_s", "tensor_d2", "tensor_resize", "org_hw", "cc_th", "remove_small_cc"]
    with pytest.raises(TypeError):
        ops.cycle_tail(None, None, None, None)


def test_drivers_select_the_grouped_chain_by_the_switch(monkeypatch):
    """RFX_FINE_GROUPS selects either way; unset, a driver's ``grouped_fine`` decides (where the library default is on)."""
    for cls in (rounds.RaggedGroup, rounds.RaggedVariantCGroup, rounds.RaggedKittiGroup):
        assert isinstance(cls.grouped_fine, bool), cls.__name__
        g = object.__new__(cls)
        monkeypatch.setenv("RFX_FINE_GROUPS", "1")
        assert g.use_groups() is True
        monkeypatch.setenv("RFX_FINE_GROUPS", "0")
        assert g.use_groups() is False
        monkeypatch.delenv("RFX_FINE_GROUPS")
        assert g.use_groups() is (cls.grouped_fine and ops.FINE_GROUPS_DEFAULT)
    assert callable(rounds.RaggedVariantCGroup.pred_groups) and rounds.RaggedVariantCGroup.pred_groups is not rounds.RaggedGroup.pred_groups
