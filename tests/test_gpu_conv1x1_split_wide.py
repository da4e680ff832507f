"""The 256-channel instance of the split 1x1 convolution (csrc/conv1x1s.hip: conv1x1_split_wide_kernel, 8 wavefronts over one staged
128-pixel activation image) against the 128-channel instance it replaces on large launches, and against float64.

Which instance a launch takes is decided by a rule the library reads ONCE per process from RFX_C1S_WIDE (0: never the wide tile; 1:
wherever Cout >= 256; unset: the measured rule of csrc/conv1x1s.hip), so every launch of this module happens in one of three child processes --
``narrow`` (RFX_C1S_WIDE=0), ``wide`` (RFX_C1S_WIDE=1) and ``auto`` (unset) -- started side by side by one module
fixture: ``python tests/test_gpu_conv1x1_split_wide.py MODE OUT`` runs every case below and saves the outputs.  The tests compare the
three files with each other bit for bit, and the wide one with float64:
  * on the exact operand families of tests/test_gpu_conv_exact.py (every product and partial sum representable in float32: any
    correct kernel returns the float64 result bit for bit) for the cases without sigmoid;
  * on realistic data (tests/test_gpu_kernels.py's split section: relu(randn) activations, He weights) by the rms error against the
    float64 convolution, bounded as there (3e-7 of the output rms), printing that module's max-error ratio against the fp32 kernel.
Shapes: the smallest that reach every branch of the kernel -- Cin = 16 / 32 / 48 / 272 (one stage, both LDS buffers, an odd stage count,
a long loop), Cout = 256 / 320 / 1024 (one exact tile, a ragged last tile that ends past the packed weights' 128-row padding, several
tiles), P = 70 (below one pixel tile, columns past the end, two images in one tile), 129 (one column into the second tile), 273 (a tile
that starts in one image and ends in the next), stride 2 from an odd width, every epilogue form, scale / shift present and null."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "ransac-flow_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest  # noqa: E402
import torch  # noqa: E402

from rfx import ops, _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, RELU, SIGMOID = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SIGMOID


def C(name, N, Cin, Cout, H, W, stride=1, res=False, act=NONE, affine=True):
    return dict(name=name, N=N, Cin=Cin, Cout=Cout, H=H, W=W, stride=stride, res=res, act=act, affine=affine)


CASES = [
    C("k16-m256-p70-res-relu", 2, 16, 256, 5, 7, res=True, act=RELU),
    C("k32-m320-p70-plain", 2, 32, 320, 5, 7, affine=False),
    C("k48-m1024-p129-sigmoid", 1, 48, 1024, 3, 43, act=SIGMOID),
    C("k272-m320-p273-res-relu", 3, 272, 320, 7, 13, res=True, act=RELU),
    C("k272-m256-s2-9x11", 2, 272, 256, 9, 11, stride=2),
    C("k48-m1024-s2-9x11-res-relu", 3, 48, 1024, 9, 11, stride=2, res=True, act=RELU, affine=False),
    C("k32-m256-p129-res-sigmoid", 1, 32, 256, 3, 43, res=True, act=SIGMOID, affine=False),
]
# one grouped launch (ops.launch_group) of three inputs of different sizes through one plan
GROUP = C("group-k48-m320", 2, 48, 320, 5, 7, res=True, act=RELU)
GROUP_SIZES = [(2, 5, 7), (1, 3, 43), (3, 7, 13)]
# dispatch: a launch of 200 wide workgroups with Cin = 512 (one round on 256 CUs where the 128-channel tiles double up: the wide
# instance under the default rule) ...
BIG = C("big-k512-m256-p25600", 4, 512, 256, 80, 80, res=True, act=RELU)
# ... and what the rule answers on trunk layers of the flagship configuration: (N, Cin, output pixels per image, Cout)
RULE_SHAPES = [(64, 1024, 4800, 256), (64, 256, 4800, 1024), (64, 512, 4800, 1024), (64, 128, 19200, 512), (64, 512, 19200, 128),
               (64, 256, 76800, 64), (1, 512, 4800, 1024), (2, 512, 4800, 1024), (8, 1024, 4800, 256), (2, 1024, 4800, 256),
               (1, 1024, 300, 256), (64, 1024, 300, 256), (64, 1024, 825, 256), (8, 1024, 3300, 256), (64, 1024, 520, 256)]


def rule(cus, N, Cin, HW, Cout):
    """csrc/conv1x1s.hip's c1s_tile_channels with RFX_C1S_WIDE unset."""
    if Cout <= 64:
        return 64
    if Cout < 256 or Cin < 512:
        return 128
    tp = (N * HW + 127) // 128
    w, n = (Cout + 255) // 256 * tp, (Cout + 127) // 128 * tp
    rest = n % (2 * cus)
    cost_wide, cost_128 = (w + cus - 1) // cus * 81, n // (2 * cus) * 100 + (0 if rest == 0 else 58 if rest <= cus else 100)
    return 256 if cost_wide < cost_128 else 128


def families(case):
    return ("random",) if case["act"] == SIGMOID else ("random", "dense", "apieces", "wpieces")


def make_data(case, fam, sizes=None):
    """CPU operands of one case and family, the same in every process: dict(w, scale, shift, Q, qx, qw, inputs=[(x, res)])."""
    import zlib
    from test_gpu_conv_exact import operands, epilogue
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (case["name"], fam)).encode()))
    Cin, Cout, s = case["Cin"], case["Cout"], case["stride"]
    sizes = sizes or [(case["N"], case["H"], case["W"])]
    d = dict(Q=None, qx=None, qw=None, scale=None, shift=None)
    if fam == "random":
        d["w"] = torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cout) ** 0.5
        if case["affine"]:
            d["scale"], d["shift"] = 1.0 + 0.2 * (torch.rand(Cout, generator=g) - 0.5), 0.1 * torch.randn(Cout, generator=g)
        xs = [torch.relu(torch.randn(N, Cin, H, W, generator=g)) for (N, H, W) in sizes]
    else:
        N0, H0, W0 = sizes[0]
        x0, d["w"], d["qx"], d["qw"] = operands(fam, g, N0, Cin, Cout, H0, W0, 1, 1)
        xs = [x0] + [operands(fam, g, N, Cin, Cout, H, W, 1, 1)[0] for (N, H, W) in sizes[1:]]
        if case["affine"]:
            d["scale"], d["shift"], d["Q"] = epilogue(fam, g, Cout, d["qx"], d["qw"])
        else:
            d["Q"] = d["qx"] * d["qw"]
    d["inputs"] = []
    for x in xs:
        N, _, H, W = x.shape
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        res = None
        if case["res"] and fam == "random":
            res = torch.randn(N, Cout, Ho, Wo, generator=g)
        elif case["res"]:
            span = 2048 if fam == "dense" else 1 << 17            # as tests/test_gpu_conv_exact.py's residuals
            res = torch.randint(-span, span + 1, (N, Cout, Ho, Wo), generator=g).float() * d["Q"]
        d["inputs"].append((x, res))
    return d


def make_plan(case, d, dev, split=True):
    p = ops.ConvPlan(d["w"], None, case["stride"], 0, case["act"], dev, split=split)
    assert (p.wS is not None) == split
    if d["scale"] is not None:
        p.scale, p.shift = d["scale"].to(dev), d["shift"].to(dev)
    return p


def tile_channels(case, N, H, W):
    s = case["stride"]
    return _lib.load().rfx_conv1x1_split_tile_channels(N, case["Cin"], ((H - 1) // s + 1) * ((W - 1) // s + 1), case["Cout"])


# ------------------------------------------------------------------ the child: every launch of this module
def child(out_path):
    dev = torch.device("cuda:0")
    rec = dict(cus=torch.cuda.get_device_properties(0).multi_processor_count, y={}, tile={}, rule={})
    for case in CASES:
        rec["tile"][case["name"]] = tile_channels(case, case["N"], case["H"], case["W"])
        for fam in families(case):
            d = make_data(case, fam)
            x, res = d["inputs"][0]
            y = make_plan(case, d, dev)(x.to(dev), residual=res.to(dev) if res is not None else None)
            rec["y"][case["name"], fam] = y.cpu()
    d = make_data(GROUP, "dense", GROUP_SIZES)
    plan = make_plan(GROUP, d, dev)
    ins = [(x.to(dev), r.to(dev)) for x, r in d["inputs"]]
    with ops.launch_group(dev, False):
        grouped = [plan(x, residual=r) for x, r in ins]
    rec["y"]["group"] = [y.cpu() for y in grouped]
    rec["y"]["group-single"] = [plan(x, residual=r).cpu() for x, r in ins]
    rec["tile"]["group"] = [tile_channels(GROUP, *sz) for sz in GROUP_SIZES]
    d = make_data(BIG, "dense")
    x, res = d["inputs"][0]
    y = make_plan(BIG, d, dev)(x.to(dev), residual=res.to(dev)).cpu()
    rec["tile"]["big"] = tile_channels(BIG, BIG["N"], BIG["H"], BIG["W"])
    rec["big_sha"] = hashlib.sha256(y.numpy().tobytes()).hexdigest()
    rec["big_first"] = y[:1, :, :8].clone()                              # the first 8 rows of image 0, every channel
    lib = _lib.load()
    rec["rule"] = {s: lib.rfx_conv1x1_split_tile_channels(*s) for s in RULE_SHAPES}
    torch.cuda.synchronize()
    torch.save(rec, out_path)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, dev):
    """{"narrow" | "wide" | "auto": the record child() saved under that setting of RFX_C1S_WIDE}"""
    tmp = tmp_path_factory.mktemp("c1s_wide")
    procs = {}
    for mode, val in (("narrow", "0"), ("wide", "1"), ("auto", None)):
        env = dict(os.environ, RFX_CONV_SPLIT="1")
        env.pop("RFX_C1S_WIDE", None)
        if val is not None:
            env["RFX_C1S_WIDE"] = val
        procs[mode] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(tmp / (mode + ".pt"))], env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for mode, p in procs.items():
        try:
            log = p.communicate(timeout=300)[0]
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert p.returncode == 0, "child %s exited with %s:\n%s" % (mode, p.returncode, log[-4000:])
        out[mode] = torch.load(str(tmp / (mode + ".pt")), weights_only=False)
    return out


def _mismatch(y, ref):
    return "%d of %d elements differ" % (int((y != ref).sum()), y.numel())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_wide_instance_equals_the_128_channel_instance_bit_for_bit(runs, case):
    assert runs["wide"]["tile"][case["name"]] == 256 and runs["narrow"]["tile"][case["name"]] == 128
    for fam in families(case):
        yw, yn = runs["wide"]["y"][case["name"], fam], runs["narrow"]["y"][case["name"], fam]
        assert yw.shape == yn.shape and torch.equal(yw, yn), (fam, _mismatch(yw, yn))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_wide_instance_against_float64(runs, case, dev):
    from test_gpu_conv_exact import exact_reference
    from test_gpu_kernels import _split_max_error_ratio
    Cin, Cout, s = case["Cin"], case["Cout"], case["stride"]
    for fam in families(case):
        d = make_data(case, fam)
        x, res = d["inputs"][0]
        yw = runs["wide"]["y"][case["name"], fam].to(dev)
        if fam != "random":
            scale = d["scale"] if d["scale"] is not None else torch.ones(Cout)
            shift = d["shift"] if d["shift"] is not None else torch.zeros(Cout)
            ref = exact_reference(x, d["w"], scale, shift, res, case["act"], d["Q"], d["qx"], d["qw"], s, 0, dev=dev, fam=fam)
            assert torch.equal(yw, ref), (fam, _mismatch(yw, ref))
            continue
        y64 = torch.einsum("mk,nkhw->nmhw", d["w"].view(Cout, Cin).double().to(dev), x[:, :, ::s, ::s].double().to(dev))
        if d["scale"] is not None:
            y64 = y64 * d["scale"].double().to(dev).view(1, -1, 1, 1) + d["shift"].double().to(dev).view(1, -1, 1, 1)
        if res is not None:
            y64 = y64 + res.double().to(dev)
        y64 = torch.relu(y64) if case["act"] == RELU else (torch.sigmoid(y64) if case["act"] == SIGMOID else y64)
        y32 = make_plan(case, d, dev, split=False)(x.to(dev), residual=res.to(dev) if res is not None else None)
        rms = float(y64.pow(2).mean().sqrt())
        esp = float((yw.double() - y64).pow(2).mean().sqrt()) / rms
        print("%s: rms error / output rms = %.3e" % (case["name"], esp))
        _split_max_error_ratio(yw, y32, y64, Cin, "wide split 1x1 %s" % case["name"])
        assert esp < 3e-7 and float((yw - y32).abs().max()) / rms < 2e-5


def test_grouped_launch_of_three_sizes(runs, dev):
    """One recorded launch of three problems of different sizes (the wide family's rfx_group_kernel_w): every member equals its own single
    launch, the 128-channel instance's grouped launch, and float64."""
    from test_gpu_conv_exact import exact_reference
    assert runs["wide"]["tile"]["group"] == [256] * 3 and runs["narrow"]["tile"]["group"] == [128] * 3
    d = make_data(GROUP, "dense", GROUP_SIZES)
    for i, (x, res) in enumerate(d["inputs"]):
        yg = runs["wide"]["y"]["group"][i]
        assert torch.equal(yg, runs["wide"]["y"]["group-single"][i]), (i, "grouped vs single")
        assert torch.equal(yg, runs["narrow"]["y"]["group"][i]), (i, "wide vs 128-channel")
        ref = exact_reference(x, d["w"], d["scale"], d["shift"], res, GROUP["act"], d["Q"], d["qx"], d["qw"], 1, 0, dev=dev, fam="dense")
        assert torch.equal(yg.to(dev), ref), (i, _mismatch(yg.to(dev), ref))


def test_dispatch_rule(runs, dev):
    """Unset, the switch sends a launch to the wide instance exactly where the measured rule says so (Cout >= 256, Cin >= 512, and the
    wide tile's rounds over the CUs shorter than the 128-channel tile's): the small launches above stay on the 128-channel instance
    (the switch changes nothing there), the large one moves, and moves no bit."""
    from test_gpu_conv_exact import exact_reference
    auto, narrow, wide = runs["auto"], runs["narrow"], runs["wide"]
    cus = auto["cus"]
    for case in CASES:
        assert auto["tile"][case["name"]] == 128
        for fam in families(case):
            assert torch.equal(auto["y"][case["name"], fam], narrow["y"][case["name"], fam])
    assert auto["tile"]["group"] == [128] * 3
    for (N, Cin, HW, Cout), got in auto["rule"].items():
        want = rule(cus, N, Cin, HW, Cout)
        assert got == want, ((N, Cin, HW, Cout), got, want, cus)
        assert narrow["rule"][N, Cin, HW, Cout] == min(want, 128)
        assert wide["rule"][N, Cin, HW, Cout] == (256 if Cout >= 256 else want)
    if cus == 256:      # MI355X: the measured winners of profiles/c1s_wide_ab.json (W = 2400, 150, 413, 207 wide; 300, 260, 75 not)
        assert [auto["rule"][s] for s in RULE_SHAPES] == [256, 128, 256, 128, 128, 64, 256, 128, 128, 128, 128, 256, 256, 256, 128]
    assert wide["tile"]["big"] == 256 and narrow["tile"]["big"] == 128
    assert auto["tile"]["big"] == rule(cus, BIG["N"], BIG["Cin"], BIG["H"] * BIG["W"], BIG["Cout"])
    assert auto["big_sha"] == narrow["big_sha"] == wide["big_sha"]
    d = make_data(BIG, "dense")
    x, res = d["inputs"][0]
    ref = exact_reference(x[:1], d["w"], d["scale"], d["shift"], res[:1], BIG["act"], d["Q"], d["qx"], d["qw"], 1, 0, dev=dev, fam="dense")
    assert torch.equal(auto["big_first"].to(dev), ref[:, :, :8])
