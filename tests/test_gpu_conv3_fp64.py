"""-m gpu: the 3x3 convolution forward and data gradient, and gemm_nt, per element against float64 (tests/conv3_reference.py: the reference,
the bound |got - ref'| <= CONV_TOL * scale + half a bf16 ulp, the two input regimes, the case list with the kernel each shape is there for;
tests/test_conv3_reference.py: the checker pinned on the CPU - truncation, a bf16 exchange of K-split partial sums and a bias added after the
rounding do not fit).

Every case of conv3_reference.CASES in both regimes, the kernel choice asserted before each call: forward with bias and ReLU, forward with
bias only, forward with nothing, data gradient with the fused mask, the accumulate form onto y_old with the mask where
conv3x3_accum_supported says so (a refusal where it does not), and the refusal of the data gradients that have no kernel (Cout % 32 != 0).
The cases with M >= 1024 again under OCR_GEMM_ENGINE 0, 2 and 3 (in-process), and the knob settings K2A, K2D, K2A+noK3, K2D+noK3, noK2 and
WS2 each as a child pytest over the cases its claims name (the knobs are read once per process), at most four at a time, each under its own
time limit, their worst ratios parsed into the parent's report.  gemm_nt: fp32 out, bias + ReLU bf16, mask bf16, splits = 3 onto a base,
accumulate, at one shape per ig_try_dispatch instance and the register-staged kernel.

Asserted: worst |device - reference| / bound <= 1 per call, no element excluded.  Measured on MI355X (worst ratio over all cases, both
regimes; -s prints them per family and form):
    family                 bias+relu  bias    plain   grad+mask  accumulate
    conv_halo              0.9980     0.9980  0.9983  0.9983     0.9983      (worst at (1100, 1, 1, 64, 64): few terms per element)
    conv_k2/A              0.9963     0.9963  0.9961  0.9969     0.9976
    conv_k2/D              0.9975     0.9975  0.9975  0.9980     0.9978
    conv_k3/A              0.9960     0.9963  0.9961  0.9964     0.9976
    conv_k3/D              0.9967     0.9973  0.9969  0.9980     0.9978
    conv_k3w/A             0.9966     0.9973  0.9971  0.9971     0.9983
    conv_k3w/D             0.9966     0.9973  0.9971  0.9971     0.9983
    conv_ws                0.9975     0.9977  0.9979  0.9969     -           (takes no accumulate flag)
    gemm (default build)   0.9967     0.9967  0.9974  0.9966     -           (refuses accumulate)
    gemm engines 0 / 2 / 3 0.9980                     0.9983                 (each engine alike)
    gemm_nt, bf16 outputs  0.9986 bias + ReLU, 0.9986 mask (every ig_try_dispatch instance 0.998 .. 0.9986, the register-staged kernel 0.9975)
    gemm_nt, fp32 outputs  0.072 fp32 out, 0.048 splits = 3 onto a base, 0.063 accumulate      (of CONV_TOL * scale alone)
Every bf16 output sits at the half ulp itself, as it should: the fp32 terms are three orders of magnitude below it (truncation would read 1.99,
a bf16 exchange of partial sums or a bias added after the rounding 30 and more).  The fp32 outputs use a fifteenth of what CONV_TOL allows.
Nothing the new cases reach is wrong on the device: the ragged channel tiles (Cout = 68, 96, 100, 132), H = 1, 3, 13, 30 and 32, the mask's
+0, -0, subnormal and smallest normal values and the single rounding of the accumulate form all hold the bound.  Found on the host side: the
data gradient of a layer with Cout % 32 != 0 has no kernel (conv3_reference.py's docstring); the call refuses, which is asserted here."""
import concurrent.futures
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv3_reference as c3  # noqa: E402

from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTING = os.environ.get("CONV3_FP64_SETTING", "default")        # a child of test_knob_settings_in_child_processes runs one setting's cases
GEMM_ENGINES = (0, 2, 3)
WORST = {}      # (family, form) -> (ratio, case)
RAN = set()     # what of the file this process has run: (shape, regime) of the default cases, knob settings


def _record(family, form, case, ratio, index):
    print("conv3 %s %s: ratio %.4f at %s of %s" % (family, form, ratio, index, case))
    if ratio >= WORST.get((family, form), (-1.0, None))[0]:
        WORST[(family, form)] = (ratio, case)
    return ratio


def _ids(cases):
    return ["x".join(map(str, s)) for s, _ in cases]


@pytest.fixture
def gemm_engine(dev):
    """ocr_set_gemm_engine for one test; afterwards the engine the environment names, else the default (1)."""
    try:
        yield lambda e: nat.call("ocr_set_gemm_engine", e)
    finally:
        nat.call("ocr_set_gemm_engine", int(os.environ.get("OCR_GEMM_ENGINE") or 1))


@functools.lru_cache(maxsize=1)
def _prepared(dev, shape, regime):
    """Inputs, float64 references and device operands of one case, computed once per shape and regime (the tests of one case follow each other)."""
    Nb, W, H, Ci, Co = shape
    i = c3.conv_inputs(shape, regime)
    x, w, bias, dy, mask = i["x"], i["w"], i["bias"], i["dy"], i["mask"]
    p = dict(bias=bias, mask=mask)
    p["ref"], p["scale"] = c3.fwd_ref(x, w)
    p["gref"], p["gscale"] = c3.dgrad_ref(dy, w) if Co % 32 == 0 else (None, None)
    p["y_old"] = c3.y_old_of(i["y_old_unit"], p["gref"]) if Co % 32 == 0 else None
    p["xd"], p["bd"], p["dyd"], p["maskd"] = x.to(dev).to(BF), bias.to(dev), dy.to(dev).to(BF), mask.to(dev).to(BF)
    assert torch.equal(p["maskd"].float().cpu(), mask)            # the special mask values reach the device as they are
    p["wpack"] = torch.empty((Co, 3, 3, Ci), dtype=BF, device=dev)
    ops.pack_transpose(w.reshape(9 * Ci, Co).to(dev), p["wpack"])  # [9 Ci][Co] -> [Co][9 Ci]
    p["wd"] = torch.empty((Ci, 3, 3, Co), dtype=BF, device=dev)
    ops.pack_conv_dgrad(w.to(dev), p["wd"])
    return p


def _run_conv(dev, shape, regime, claim, tag, forms=("relu", "bias", "plain", "grad", "accum"), name=None):
    """The forms of one case against its float64 reference; returns {(family, form): ratio} (family: `name` if given, else the kernel choice)."""
    Nb, W, H, Ci, Co = shape
    fwd, grad = claim
    choice = ops.conv3x3_kernel_choice
    p = _prepared(dev, shape, regime)
    bias, mask, ref, scale, gref, gscale = p["bias"], p["mask"], p["ref"], p["scale"], p["gref"], p["gscale"]
    xd, bd, dyd, maskd, wpack, wd = p["xd"], p["bd"], p["dyd"], p["maskd"], p["wpack"], p["wd"]
    refb, scaleb = ref + bias.double(), scale + bias.abs().double()
    case = "%s %s %s" % (tag, shape, regime)
    out = {}
    if "relu" in forms:
        assert choice(Nb, W, H, Ci, Co) == fwd, (case, choice(Nb, W, H, Ci, Co), fwd)
        y = ops.conv3x3(xd, wpack, bias=bd, relu=True)
        out[name or fwd, "bias+relu"] = _record(name or fwd, "bias+relu", case, *c3.check(y.float().cpu(), refb, scaleb, relu=True))
    if "bias" in forms:
        assert choice(Nb, W, H, Ci, Co, relu=False) == fwd, case
        y = ops.conv3x3(xd, wpack, bias=bd)
        out[name or fwd, "bias"] = _record(name or fwd, "bias", case, *c3.check(y.float().cpu(), refb, scaleb))
    if "plain" in forms:
        assert choice(Nb, W, H, Ci, Co, bias=False, relu=False) == fwd, case
        y = ops.conv3x3(xd, wpack)
        out[name or fwd, "plain"] = _record(name or fwd, "plain", case, *c3.check(y.float().cpu(), ref, scale))
    if grad is None:
        # no kernel computes this gradient (Cin of the gradient = Cout % 32 != 0): the call refuses, it does not fall back
        if "grad" in forms:
            with pytest.raises(nat.NativeError):
                ops.conv3x3(dyd, wd, mask=maskd)
            assert not ops.conv3x3_accum_supported(Nb, W, H, Co, Ci)
        return out
    if "grad" in forms:
        assert choice(Nb, W, H, Co, Ci, bias=False, relu=False, mask=True) == grad, case
        dx = ops.conv3x3(dyd, wd, mask=maskd)
        out[name or grad, "grad+mask"] = _record(name or grad, "grad+mask", case, *c3.check(dx.float().cpu(), gref, gscale, mask=mask))
    if "accum" in forms:
        y_old = p["y_old"]
        acc = y_old.to(dev).to(BF)
        if ops.conv3x3_accum_supported(Nb, W, H, Co, Ci):
            fam = choice(Nb, W, H, Co, Ci, bias=False, relu=False, mask=True, accumulate=True)
            assert fam != "gemm", case
            ops.conv3x3(dyd, wd, out=acc, mask=maskd, accumulate=True)
            out[fam, "accumulate"] = _record(fam, "accumulate", case, *c3.check(acc.float().cpu(), gref, gscale, mask=mask, y_old=y_old))
        else:
            with pytest.raises(nat.NativeError):
                ops.conv3x3(dyd, wd, out=acc, mask=maskd, accumulate=True)
            torch.cuda.synchronize()
            assert torch.equal(acc.float().cpu(), y_old)
    return out


@pytest.mark.parametrize("regime", c3.REGIMES)
@pytest.mark.parametrize("shape,claim", c3.cases_of(SETTING), ids=_ids(c3.cases_of(SETTING)))
def test_conv3x3_against_fp64(dev, shape, claim, regime):
    """Under the knob setting of this process (the default build's, unless a parent named another)."""
    assert all(os.environ.get(k) == v for k, v in c3.SETTINGS[SETTING].items()), (SETTING, "knobs not in the environment")
    ratios = _run_conv(dev, shape, regime, claim, SETTING)
    RAN.add((shape, regime))
    assert ratios and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("regime", c3.REGIMES)
@pytest.mark.parametrize("shape,claim", [c for c in c3.cases_of("default") if c[0][0] * c[0][1] * c[0][2] >= 1024],
                         ids=_ids([c for c in c3.cases_of("default") if c[0][0] * c[0][1] * c[0][2] >= 1024]))
def test_conv3x3_on_the_gemm_engines_against_fp64(dev, gemm_engine, shape, claim, regime):
    """OCR_GEMM_ENGINE 0 (register-staged tiles), 2 and 3 (igemm two- / three-stage where ig_try_dispatch takes the shape): forward with bias
    and ReLU and the masked data gradient of every case with M >= 1024, the same checker."""
    ratios = {}
    for e in GEMM_ENGINES:
        gemm_engine(e)
        ratios.update(_run_conv(dev, shape, regime, ("gemm", claim[1] and "gemm"), "engine%d" % e, forms=("relu", "grad"), name="gemm/engine%d" % e))
    assert max(ratios.values()) <= 1.0, ratios


# ------------------------------------------------------------------------------------------- the knob settings, one child pytest each
KNOB_SETTINGS = [s for s in c3.SETTINGS if s != "default"]


def _parse(stdout):
    worst = {}
    for fam, form, ratio in re.findall(r"conv3 (\S+) (\S+): ratio ([0-9.e+-]+|inf)", stdout):
        worst[fam, form] = max(worst.get((fam, form), 0.0), float(ratio))
    return worst


@pytest.fixture(scope="module")
def knob_runs(dev):
    def run(setting):
        env = dict(c3.child_env(setting), CONV3_FP64_SETTING=setting, OMP_NUM_THREADS="4", MKL_NUM_THREADS="4")
        try:
            out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k",
                                  "test_conv3x3_against_fp64"], env=env, capture_output=True, text=True, timeout=420, cwd=ROOT)
            return out.returncode, out.stdout
        except subprocess.TimeoutExpired as e:
            return -1, "timed out: %s" % e
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        return dict(zip(KNOB_SETTINGS, ex.map(run, KNOB_SETTINGS)))


@pytest.mark.parametrize("setting", KNOB_SETTINGS)
def test_knob_settings_in_child_processes(dev, knob_runs, setting):
    """conv_k2 / conv_k3 / conv_k3w with each tile forced, conv_k2 alone, conv_halo alone and conv_ws forced, over the cases whose claims name
    the setting, through test_conv3x3_against_fp64 in an interpreter of their own."""
    if SETTING != "default":
        return                                       # a child does not start children
    rc, stdout = knob_runs[setting]
    assert rc == 0, (setting, stdout[-3000:])
    assert " passed" in stdout and "skipped" not in stdout and "failed" not in stdout, stdout[-1000:]
    worst = _parse(stdout)
    print(setting, "worst ratios", {"%s %s" % k: round(v, 4) for k, v in sorted(worst.items())})
    claimed = {f for _, (fwd, grad) in c3.cases_of(setting) for f in (fwd, grad) if f}
    assert claimed <= {fam for fam, _ in worst}, (claimed, sorted(worst))
    assert max(worst.values()) <= 1.0, worst
    RAN.add(setting)
    for (fam, form), r in worst.items():
        if r >= WORST.get((fam, form), (-1.0, None))[0]:
            WORST[fam, form] = (r, setting)


# ------------------------------------------------------------------------------------------- gemm_nt
GEMM_INSTANCE = {(1100, 132): "ig4w/BN64", (7168, 1024): "ig4w/BN128", (25600, 512): "ig8w/BN128", (32768, 512): "ig8w/BN256",
                 (102400, 64): "ig8w/BN64", (300, 132): "gemm_nt_kernel", (70, 520): "gemm_nt_kernel"}


@pytest.mark.parametrize("regime", c3.REGIMES)
@pytest.mark.parametrize("M,N,K", c3.GEMM_CASES)
def test_gemm_nt_against_fp64(dev, M, N, K, regime):
    """out = P Q^T through the same checker: reference the float64 product, scale |P| |Q|^T + |bias| + |base|."""
    i = c3.gemm_inputs((M, N, K), regime)
    P, Q, bias, mask = i["P"], i["Q"], i["bias"], i["mask"]
    ref, scale = c3.gemm_ref(P, Q)
    refb, scaleb = ref + bias.double(), scale + bias.abs().double()
    base = c3.y_old_of(i["base_unit"], ref)
    Pd, Qd, bd, based = P.to(dev).to(BF), Q.to(dev).to(BF), bias.to(dev), base.to(dev)
    fam, case = "gemm_nt/" + GEMM_INSTANCE[M, N], "%s %s" % ((M, N, K), regime)
    r = {}
    r["f32"] = _record(fam, "f32", case, *c3.check(ops.gemm_nt(Pd, Qd, out_f32=True).cpu(), ref, scale, out="f32"))
    r["bias+relu"] = _record(fam, "bias+relu", case, *c3.check(ops.gemm_nt(Pd, Qd, bias=bd, relu=True).float().cpu(), refb, scaleb, relu=True))
    r["mask"] = _record(fam, "mask", case, *c3.check(ops.gemm_nt(Pd, Qd, mask=mask.to(dev).to(BF)).float().cpu(), ref, scale, mask=mask))
    # split-K with atomics accumulates onto the existing fp32 content; the register-staged kernel's fp32 accumulate epilogue
    out = ops.gemm_nt(Pd, Qd, out=based.clone(), splits=3, bias=bd)
    r["splits3"] = _record("gemm_nt/gemm_nt_kernel", "splits3+base", case, *c3.check(out.cpu(), refb, scaleb, out="f32", y_old=base))
    out = ops.gemm_nt(Pd, Qd, out=based.clone(), accumulate=True)
    r["accumulate"] = _record("gemm_nt/gemm_nt_kernel", "accumulate", case, *c3.check(out.cpu(), ref, scale, out="f32", y_old=base))
    assert max(r.values()) <= 1.0, r


def test_report_and_family_coverage(dev):
    """(last) the worst ratio per family and epilogue form over this process's run; with the whole file run under the default knobs, every
    family has gone through every form it has."""
    for (fam, form), (r, case) in sorted(WORST.items()):
        print("conv3 worst %-28s %-13s %.4f  (%s)" % (fam, form, r, case))
    assert all(r <= 1.0 for r, _ in WORST.values()), WORST
    if SETTING == "default" and RAN >= set(KNOB_SETTINGS) | {(s, r) for s, _ in c3.cases_of("default") for r in c3.REGIMES}:
        for fam in c3.FAMILIES:
            forms = {form for f, form in WORST if f == fam}
            want = {"bias+relu", "bias", "plain", "grad+mask"} | (set() if fam in ("gemm",) + c3.ACCUM_UNREACHABLE else {"accumulate"})
            assert want <= forms, (fam, want - forms)
