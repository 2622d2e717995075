"""-m gpu: the kernel generations a user can switch to, each against the same references and bars as the default build.

In-process (the setters take effect at the next call):
  OCR_GEMM_ENGINE = 0 / 2 / 3   gemm_nt and the 3x3 convolution (forward, data gradient) on the register-staged 128 x 128 tiles / on igemm.hip
                                two-stage / three-stage, none of the tap-reuse kernels
  OCR_WGRAD_ENGINE = 1 / 0      3x3 weight gradient and A^T B on gemm_tn2 (atomics) / on the register-staged gemm_tn_kernel
In child processes (read once per process): OCR_W9_PLANES=0, OCR_W9P_GENW=0 / 2 over the convolution parity test and the float64
weight-gradient test below; OCR_TN3_NST=5 over test_gemm_tn_jobs.
Kernel level: ops.conv3x3_wgrad_deferred + ONE ops.wgrad9_reduce_jobs against the per-layer calls (bit-identical) and float64.
Engine level: one forward + backward at (N, W) = (8, 88) under OCR_GEMM_ENGINE=0, =3 and OCR_WGRAD_ENGINE=0 against the ORACLE by the
bars of test_gpu_engine.py (two correct builds may differ from each other by percent: the comment above GRAD_L2_BAR).

The float64 weight-gradient reference and its bar.  dw[a][b] = shift_ab(x)^T dy in float64 (conv_shapes.wgrad_ref64: nine matmuls on
the zero-padded input), every element against ITS OWN scale: |got - ref|_ij <= WGRAD_TOL * (|x|-shifted^T |dy|)_ij, the sum of the
magnitudes of the terms that element adds up - the unit in which a summation-order error is a small multiple of 2^-24 whatever the
element's value.  (The single bar 1e-4 * max|ref| of test_gpu_kernels.py stays asserted beside it; in these units it is 1.7e-6 ..
2.1e-4 at the element it is loosest for.)  WGRAD_TOL comes from the reference side only, never from a device result: the same nine
matmuls in torch.float32 on the CPU against the float64 ones, same inputs (gen seeds 1 / 4, bf16-rounded), over the 39 shapes of the
list, measured 3.5e-9 (64, 128, 16, 64, 128) .. 1.11e-7 (2, 12, 4, 256, 512); product-size shapes 3.5e-9 .. 1.6e-8, the small ones
(few terms per element, where the one rounding of the result, 2^-24 = 6.0e-8, dominates) 2.5e-8 .. 1.11e-7.  torch's fp32 convolution
backward on the same inputs: 1.8e-8 .. 1.7e-7.
    WGRAD_TOL = 8 x 1.114e-7 = 8.9e-7
The factor 8 is for the kernels' other summation order: sequential MFMA chains of up to k_per_split pixels, then S slabs or S atomic
adds, where the CPU product sums blockwise.  The bias gradient (column sums of dy, from the same pass and the same splits) is checked the
same way against sum |dy| with the same tolerance (torch's pairwise fp32 sum is at 1.2e-9 .. 8.8e-9, below one fp32 rounding: no bar of
its own is taken from it).  The worst device ratio per engine / knob setting is printed (-s)."""
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_shapes as cs  # noqa: E402
import test_gpu_engine as te  # noqa: E402
import test_gpu_kernels as tk  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402
from lstm_ctc_ocr_amd.config import cfg  # noqa: E402
from lstm_ctc_ocr_amd.engine import Engine  # noqa: E402
from lstm_ctc_ocr_amd.models import get_network  # noqa: E402

BF = torch.bfloat16
bf, gen, relerr = tk.bf, tk.gen, tk.relerr
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WGRAD_TOL = 8 * 1.114e-7          # module docstring
GEMM_ENGINES = (0, 2, 3)
WGRAD_ENGINES = (2, 1, 0)         # 2 = the default: the float64 check of the slab kernels (and what the knob children run)


def _params(fn):
    return list(fn.pytestmark[0].args[1])


@pytest.fixture
def gemm_engine(dev):
    """ocr_set_gemm_engine for one test; afterwards the engine the environment names, else the default (1)."""
    try:
        yield lambda e: nat.call("ocr_set_gemm_engine", e)
    finally:
        nat.call("ocr_set_gemm_engine", int(os.environ.get("OCR_GEMM_ENGINE") or 1))


@pytest.fixture
def wgrad_engine(dev):
    """ocr_set_wgrad_engine for one test; afterwards the engine the environment names, else the default (2)."""
    try:
        yield lambda e: nat.call("ocr_set_wgrad_engine", e)
    finally:
        nat.call("ocr_set_wgrad_engine", int(os.environ.get("OCR_WGRAD_ENGINE") or 2))


# ------------------------------------------------------------------------------------------- convolution: OCR_GEMM_ENGINE 0 / 2 / 3
@pytest.mark.parametrize("Nb,W,H,Ci,Co", cs.CONV_SHAPES)
def test_conv3x3_fwd_dgrad_on_the_gemm_engines(dev, gemm_engine, Nb, W, H, Ci, Co):
    """Forward (bias + ReLU) and data gradient (fused mask) of test_conv3x3_fwd_dgrad_wgrad, same fp32 reference and bars, under each engine
    that runs the convolution as a generic GEMM: engine 0 = launch_gemm<1, 4, 4> (128 x 128 register-staged tiles; <1, 2, 2> below 128
    channels or 1024 pixels), engines 2 / 3 = igemm_kernel<BN, 1, stages> where ig_try_dispatch takes the shape (M >= 1024), else the same
    small tiles.  By ig_try_dispatch (mt = ceil(M / 256); the widest n-tile that still gives 256 workgroups, 128 also for tiny grids):
      BN = 256   forward of (64, 128, 8, 64, 256)  (mt = 256, one 256-wide tile) - two stages under both engines (3 x 64 KiB do not fit)
      BN = 128   forward of 20 shapes, e.g. the headline (64, 128, 16, 64, 128), (64, 64, 8, 128 / 256, 256), (64, 64, 4, 256 / 512, 512) and
                 the general widths (64, 79, 4, 256, 512), (64, 79, 8, 256, 256); data gradient of 17, e.g. (64, 64, 4, 512, 512), (17, 62, 4, 128, 128)
      BN = 64    every Cout = 64 forward and Cin = 64 data gradient, and grids below 256 tiles of 128: forward of (32, 64, 4, 512, 512),
                 (64, 20, 4, 512, 512), data gradient of (64, 64, 4, 256, 512), (64, 80, 4, 256, 512)
      none       (4, 16, 8, 64, 128), (2, 12, 4, 256, 512), (3, 20, 16, 64, 128), (3, 18, 2, 64, 128): fewer than 1024 pixels
    Under these engines nothing fused exists: the queries say so and the fused entry points refuse (the engine falls back on that)."""
    x = bf(gen((Nb, W, H, Ci), 1)); w = bf(gen((3, 3, Ci, Co), 2, 0.05)); b = gen((Co,), 3)
    dy = bf(gen((Nb, W, H, Co), 4)); below = gen((Nb, W, H, Ci), 5)
    xr = x.clone().requires_grad_(True)
    ref = tk._conv_ref(xr, w, b)
    ref.backward(dy)
    want_y = bf(torch.relu(ref.detach())); want_dx = bf(xr.grad * (bf(below) > 0))
    xd, dyd, bd, belowd = x.to(dev).to(BF), dy.to(dev).to(BF), b.to(dev), below.to(dev).to(BF)
    wpack = torch.empty((Co, 3, 3, Ci), dtype=BF, device=dev)
    ops.pack_transpose(w.reshape(9 * Ci, Co).to(dev), wpack)
    wd = torch.empty((Ci, 3, 3, Co), dtype=BF, device=dev)
    ops.pack_conv_dgrad(w.to(dev), wd)
    for e in GEMM_ENGINES:
        gemm_engine(e)
        assert ops.conv3x3_kernel_choice(Nb, W, H, Ci, Co) == "gemm"
        assert ops.conv3x3_kernel_choice(Nb, W, H, Co, Ci, bias=False, relu=False, mask=True) == "gemm"
        y = ops.conv3x3(xd, wpack, bias=bd, relu=True)
        ey = relerr(y.float().cpu(), want_y)
        dx = ops.conv3x3(dyd, wd, mask=belowd)
        edx = relerr(dx.float().cpu(), want_dx)
        print("gemm engine %d %s: forward %.2e, data gradient %.2e (bar 1e-2)" % (e, (Nb, W, H, Ci, Co), ey, edx))
        assert ey < 1e-2 and edx < 1e-2, (e, ey, edx)
        # no fused epilogue of any kind
        for kw, kh in ((1, 2), (2, 2)):
            assert not ops.conv3x3_pool_supported(Nb, W, H, Ci, Co, kw, kh)
            assert ops.conv3x3_kernel_choice(Nb, W, H, Ci, Co, pool=(kw, kh)) == "gemm"
        assert not ops.conv3x3_accum_supported(Nb, W, H, Ci, Co) and not ops.conv3x3_accum_supported(Nb, W, H, Co, Ci)
        assert ops.conv3x3_stats_rows(Nb, W, H, Ci, Co) == 0 and ops.conv3x3_bnbwd_rows(Nb, W, H, Co, Ci) == 0
        part = torch.zeros((max(Nb * W * H // 256, 1), 2, max(Ci, Co)), dtype=torch.float32, device=dev)
        vec = torch.zeros(max(Ci, Co), dtype=torch.float32, device=dev)
        with pytest.raises(nat.NativeError):
            ops.conv3x3_relu_pool(xd, wpack, torch.empty_like(y), torch.empty_like(y), bd, 1, 2)
        with pytest.raises(nat.NativeError):
            ops.conv3x3_stats(xd, wpack, torch.empty_like(y), part, bias=bd)
        with pytest.raises(nat.NativeError):
            ops.conv3x3_dgrad_bnbwd(dyd, wd, torch.empty_like(dx), belowd, belowd, vec, vec, part)
        with pytest.raises(nat.NativeError):
            ops.conv3x3(dyd, wd, out=dx, mask=belowd, accumulate=True)


# ------------------------------------------------------------------------------------------- gemm_nt: OCR_GEMM_ENGINE 0 / 2 / 3
@pytest.mark.parametrize("M,N,K", _params(tk.test_gemm_nt) + [(4032, 2048, 768)])       # + the BiLSTM input projection of the headline step
def test_gemm_nt_on_the_gemm_engines(dev, gemm_engine, M, N, K):
    """Every case and bar of test_gemm_nt (run as that test's own body) under each engine."""
    for e in GEMM_ENGINES:
        gemm_engine(e)
        tk.test_gemm_nt(dev, M, N, K)


def test_gemm_nt_rowswap_and_rowgroups_on_the_gemm_engines(dev, gemm_engine):
    """test_gemm_nt_rowswap_and_rowgroups under each engine, and conv5's overlapping row groups at the headline size (Nb = 64, W = 64, HC = 1024:
    M = 4032 rows of K = 2048 - the only size at which igemm's row-group addressing runs full tiles)."""
    Nb, W, HC, Co = 64, 64, 1024, 512
    x = bf(gen((Nb, W, HC), 3)); Wt = bf(gen((Co, 2 * HC), 4))
    rows = torch.cat([x[:, :-1], x[:, 1:]], dim=2).reshape(Nb * (W - 1), 2 * HC)        # row (n, w) = [x[n, w] | x[n, w + 1]]
    want = rows @ Wt.t()
    xd, Wd = x.to(dev).to(BF), Wt.to(dev).to(BF)
    for e in GEMM_ENGINES:
        gemm_engine(e)
        tk.test_gemm_nt_rowswap_and_rowgroups(dev)
        out = ops.gemm_nt(xd, Wd, M=Nb * (W - 1), N=Co, K=2 * HC, ldp=HC, row_group=W - 1, row_skip=1, out_f32=True)
        err = relerr(out.cpu(), want)
        print("gemm engine %d conv5 rows (4032, 512, 2048): %.2e (bar 2e-5)" % (e, err))
        assert err < 2e-5


# ------------------------------------------------------------------------------------------- weight gradient: float64, every engine
WORST = {}          # (setting, kernel) -> worst per-element ratio seen by this process


@functools.lru_cache(maxsize=2)
def _wgrad_case(shape):
    Nb, W, H, Ci, Co = shape
    x = bf(gen((Nb, W, H, Ci), 1)); dy = bf(gen((Nb, W, H, Co), 4))
    return (x, dy) + cs.wgrad_ref64(x, dy)


def _knob_setting():
    knobs = ["%s=%s" % (k, os.environ[k]) for k in ("OCR_W9_PLANES", "OCR_W9P_GENW") if os.environ.get(k)]
    return " ".join(knobs) or "default knobs"


def _check_wgrad(tag, kernel, dw, db, ref, scale, dbr, dbscale, times=1):
    """dw against times * ref: the per-element float64 bar and the old single bar; the same for the bias gradient."""
    got = dw.cpu().double()
    r = cs.element_ratio(got, times * ref, times * scale)
    rb = cs.element_ratio(db.cpu().double(), times * dbr, times * dbscale)
    WORST[(tag, kernel)] = max(WORST.get((tag, kernel), 0.0), r, rb)
    print("wgrad ratio %-34s %-22s dw %.2e dbias %.2e (bar %.2e)" % (tag, kernel, r, rb, WGRAD_TOL))
    assert r <= WGRAD_TOL and rb <= WGRAD_TOL, (tag, kernel, r, rb)
    assert relerr(got, times * ref) < 1e-4 and relerr(db.cpu().double(), times * dbr) < 1e-4


@pytest.mark.parametrize("engine", WGRAD_ENGINES, ids=["eng%d" % e for e in WGRAD_ENGINES])
@pytest.mark.parametrize("Nb,W,H,Ci,Co", cs.CONV_SHAPES)
def test_wgrad_fp64(dev, wgrad_engine, engine, Nb, W, H, Ci, Co):
    """The atomics, splits = 2 and workspace parts of test_conv3x3_fwd_dgrad_wgrad under each weight-gradient engine, against the float64
    reference per element (module docstring) and by that test's own bar; which kernel computed each part is asked of the library and printed.
    Under engines 1 / 0 a workspace changes nothing: the atomics path answers, and the query says so."""
    shape = (Nb, W, H, Ci, Co)
    x, dy, ref, scale, dbr, dbscale = _wgrad_case(shape)
    xd, dyd = x.to(dev).to(BF), dy.to(dev).to(BF)
    wgrad_engine(engine)
    tag = "engine %d %s" % (engine, _knob_setting())
    zeros = lambda: (torch.zeros((3, 3, Ci, Co), dtype=torch.float32, device=dev), torch.zeros(Co, dtype=torch.float32, device=dev))
    k_at, k_s2, k_ws = (ops.conv3x3_wgrad_kernel_choice(*shape, workspace=False), ops.conv3x3_wgrad_kernel_choice(*shape, workspace=False, splits=2),
                        ops.conv3x3_wgrad_kernel_choice(*shape))
    print("wgrad choice %s %s: atomics %s, splits=2 %s, workspace %s" % (tag, shape, k_at, k_s2, k_ws))
    slab = k_ws[0].startswith("wgrad9")
    assert not k_at[0].startswith("wgrad9") and not k_s2[0].startswith("wgrad9") and k_s2[1] == 2
    if engine != 2:
        assert k_ws == k_at and not slab
    if engine == 0:
        assert k_at[0] == ("gemm_tn<1,4,4>" if Ci >= 128 and Co >= 128 else "gemm_tn<1,2,2>")
    # atomics; then splits = 2 on top of it ("+=")
    dw, db = zeros()
    ops.conv3x3_wgrad(xd, dyd, dw, dbias=db)
    _check_wgrad(tag, k_at[0], dw, db, ref, scale, dbr, dbscale)
    ops.conv3x3_wgrad(xd, dyd, dw, splits=2, dbias=db)
    _check_wgrad(tag, k_at[0] + " + " + k_s2[0], dw, db, ref, scale, dbr, dbscale, times=2)
    dw, db = zeros()
    ops.conv3x3_wgrad(xd, dyd, dw, splits=2, dbias=db)
    _check_wgrad(tag, k_s2[0] + " splits=2", dw, db, ref, scale, dbr, dbscale)
    # workspace form: poisoned scratch, twice (the slab kernels give the same bits), and "+=" onto ones
    nbytes = ops.conv3x3_wgrad_workspace_bytes(*shape)
    if engine == 2:
        assert bool(nbytes) == slab
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    ws.fill_(0x7f)
    runs = []
    for _ in range(2):
        dw, db = zeros()
        ops.conv3x3_wgrad(xd, dyd, dw, dbias=db, workspace=ws)
        runs.append((dw.cpu(), db.cpu()))
        _check_wgrad(tag, k_ws[0] + " (workspace)", dw, db, ref, scale, dbr, dbscale)
    if slab:
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    dw = torch.ones((3, 3, Ci, Co), dtype=torch.float32, device=dev)
    ops.conv3x3_wgrad(xd, dyd, dw, workspace=ws)
    # one more fp32 rounding, of (1 + gradient): 2^-24 of it, in units of the element's scale
    got = dw.cpu().double() - 1.0
    assert bool(((got - ref).abs() <= WGRAD_TOL * scale + 2.0 ** -24 * (1.0 + ref.abs())).all())
    assert relerr(got, ref) < 1e-4


def test_wgrad_fp64_worst_ratios(dev):
    """Prints the worst per-element ratio this process has seen per (engine and knob setting, kernel) - after test_wgrad_fp64 in file order."""
    for (tag, kernel), r in sorted(WORST.items()):
        print("wgrad worst %-34s %-44s %.2e of the bar %.2e" % (tag, kernel, r, WGRAD_TOL))
    assert all(r <= WGRAD_TOL for r in WORST.values())


# ------------------------------------------------------------------------------------------- A^T B: OCR_WGRAD_ENGINE 1 / 0
@pytest.mark.parametrize("Mk,I,J", _params(tk.test_gemm_tn))
def test_gemm_tn_on_the_wgrad_engines(dev, wgrad_engine, Mk, I, J):
    """Every case and bar of test_gemm_tn under engines 1 (gemm_tn2 where I, J % 128 == 0 and Mk >= 256) and 0 (gemm_tn_kernel<0, ., .>)."""
    for e in (1, 0):
        wgrad_engine(e)
        tk.test_gemm_tn(dev, Mk, I, J)


def test_gemm_tn_batched_and_conv5_rows_on_the_wgrad_engines(dev, wgrad_engine):
    for e in (1, 0):
        wgrad_engine(e)
        tk.test_gemm_tn_batched_and_xh(dev)
        tk.test_gemm_tn_conv5_rows(dev)


# ------------------------------------------------------------------------------------------- deferred slab reduction, kernel level
DEFERRED_LAYERS = [   # the headline step's five 3x3 layers at Nb = 8 (S = 32, 8, 8, 4, 4: four rows per reduce block, then one), conv3_2 and conv2 at
    # Nb = 64 (S = 16: two rows, S = 64: eight) and a general width (zero-row instance, S = 8)
    (8, 128, 16, 64, 128), (8, 64, 8, 128, 256), (8, 64, 8, 256, 256), (8, 64, 4, 256, 512), (8, 64, 4, 512, 512),
    (64, 64, 8, 256, 256), (64, 128, 16, 64, 128), (32, 33, 4, 64, 64)]
DEFERRED_S = [32, 8, 8, 4, 4, 16, 64, 8]            # w9_plan: doubled while S * Cin/64 * Cout/64 <= 128 and every split keeps >= 512 pixels
DEFERRED_ROWS = [4, 1, 1, 1, 1, 2, 8, 1]            # S / 8 slab rows per reduce block, at least one


def test_deferred_reduction_of_several_layers_in_one_launch(dev):
    """ops.conv3x3_wgrad_deferred for eight layers of different split counts and reduce-block shapes, the job table built as the engine builds
    it (Engine.W9_JOB_DTYPE, running block_start), ONE ops.wgrad9_reduce_jobs: dw / dbias += the gradient, starting from non-zero content,
    scratch poisoned - bit-identical to the per-layer ops.conv3x3_wgrad(workspace=) calls and right against float64.  A shape the slab plan
    refuses returns (None, 0) and has computed the whole gradient at once."""
    plans = [ops.conv3x3_wgrad_kernel_choice(*s) for s in DEFERRED_LAYERS]
    print("deferred layers:", list(zip(DEFERRED_LAYERS, plans)))
    assert all(k.startswith("wgrad9") for k, _ in plans)
    assert [S for _, S in plans] == DEFERRED_S
    cases, pend = [], []
    for i, shape in enumerate(DEFERRED_LAYERS):
        Nb, W, H, Ci, Co = shape
        x = bf(gen((Nb, W, H, Ci), 11 + i)); dy = bf(gen((Nb, W, H, Co), 31 + i))
        dw0 = gen((3, 3, Ci, Co), 51 + i); db0 = gen((Co,), 71 + i)
        xd, dyd = x.to(dev).to(BF), dy.to(dev).to(BF)
        ws = torch.empty(ops.conv3x3_wgrad_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
        ws.fill_(0x7f)
        dw, db = dw0.to(dev), db0.to(dev)
        job, nblk = ops.conv3x3_wgrad_deferred(xd, dyd, dw, db, ws)
        assert job is not None and len(job) == 64 and nblk > 0
        torch.cuda.synchronize()
        assert torch.equal(dw.cpu(), dw0) and torch.equal(db.cpu(), db0)          # nothing added yet: the reduction is pending
        pend.append((job, nblk))
        cases.append((shape, x, dy, xd, dyd, dw0, db0, dw, db, ws))
    tab = np.frombuffer(b"".join(j for j, _ in pend), dtype=Engine.W9_JOB_DTYPE).copy()
    assert tab.itemsize == 64
    assert [int(v) for v in tab["S"]] == DEFERRED_S and [int(v) for v in tab["rows"]] == DEFERRED_ROWS
    start = 0
    for i, (_, nblk) in enumerate(pend):
        tab["block_start"][i] = start
        start += nblk
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    ops.wgrad9_reduce_jobs(table, len(pend), start)
    torch.cuda.synchronize()
    for shape, x, dy, xd, dyd, dw0, db0, dw, db, ws in cases:
        ws2 = torch.empty_like(ws)
        ws2.fill_(0x7f)
        dw2, db2 = dw0.to(dev), db0.to(dev)
        ops.conv3x3_wgrad(xd, dyd, dw2, dbias=db2, workspace=ws2)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), shape
        ref, scale, dbr, dbscale = cs.wgrad_ref64(x, dy)
        # float64 bar + the one fp32 rounding of (start value + gradient)
        ed = (dw.cpu().double() - dw0.double() - ref).abs() - 2.0 ** -24 * (dw0.double() + ref).abs()
        eb = (db.cpu().double() - db0.double() - dbr).abs() - 2.0 ** -24 * (db0.double() + dbr).abs()
        print("deferred %s: dw %.2e dbias %.2e of the scale (bar %.2e)" % (shape, float((ed / scale).max()), float((eb / dbscale).max()), WGRAD_TOL))
        assert bool((ed <= WGRAD_TOL * scale).all()) and bool((eb <= WGRAD_TOL * dbscale).all()), shape
    # refused by the slab plan (96 pixels): everything at once, nothing pending
    Nb, W, H, Ci, Co = 2, 12, 4, 256, 512
    assert ops.conv3x3_wgrad_workspace_bytes(Nb, W, H, Ci, Co) == 0
    x = bf(gen((Nb, W, H, Ci), 1)); dy = bf(gen((Nb, W, H, Co), 4))
    dw = torch.ones((3, 3, Ci, Co), dtype=torch.float32, device=dev); db = torch.ones(Co, dtype=torch.float32, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    assert ops.conv3x3_wgrad_deferred(x.to(dev).to(BF), dy.to(dev).to(BF), dw, db, ws) == (None, 0)
    ref, scale, dbr, dbscale = cs.wgrad_ref64(x, dy)
    assert relerr(dw.cpu().double() - 1.0, ref) < 1e-4 and relerr(db.cpu().double() - 1.0, dbr) < 1e-4


# ------------------------------------------------------------------------------------------- engine level, against the oracle
STEP_N, STEP_W = 8, 88


@pytest.fixture(scope="module")
def step_oracle():
    """Parameters (seed 3, as test_gpu_engine.py), batch and the oracle's answer for it - computed once for the three settings."""
    cfg.TRAIN.WEIGHT_DECAY = 1e-5
    cfg.TRAIN.LEARNING_RATE = 1e-4
    cfg.TRAIN.SOLVER = 'Adam'
    batch = te.make_batch(STEP_N, STEP_W, 2, 4, 2)
    state = Engine(get_network('LSTM_train'), device='cuda:0', seed=3).state_arrays()
    params = {k: torch.from_numpy(v) for k, v in state.items()}
    return batch, state, te.oracle_step(params, *batch)


@pytest.mark.parametrize("setter,value", [("ocr_set_gemm_engine", 0), ("ocr_set_gemm_engine", 3), ("ocr_set_wgrad_engine", 0)])
def test_train_step_on_an_older_generation_against_the_oracle(dev, gemm_engine, wgrad_engine, step_oracle, setter, value):
    """One forward + backward of the whole network with the engine generation set BEFORE the Engine is built (its plan asks the library what
    is fused): loss and every gradient against the oracle by test_train_step_parity's bars.  Under OCR_GEMM_ENGINE = 0 / 3 no fused epilogue
    may be active in the plan."""
    (x, labels, ll, sl), state, oracle = step_oracle
    (gemm_engine if setter == "ocr_set_gemm_engine" else wgrad_engine)(value)
    eng = Engine(get_network('LSTM_train'), device='cuda:0', seed=3)
    got = eng.state_arrays()
    assert all(np.array_equal(got[k], state[k]) for k in state)                   # same parameters as the oracle's
    sp = eng.plan(STEP_N, STEP_W)
    eng._bind(sp, x, sl, labels, ll)
    eng._run(sp, 'fb')
    torch.cuda.synchronize()
    if setter == "ocr_set_gemm_engine":
        assert not any(getattr(sp, 'bn_stat_rows', {}).values()) and not any(getattr(sp, 'bn_bwd_rows', {}).values())
        assert not getattr(sp, 'fused_pools', set())
    assert not sp.w9_pending
    te.check_step_against_oracle(eng, sp, oracle)


# ------------------------------------------------------------------------------------------- read-once knobs: child processes
_BOTH = [os.path.join(ROOT, 'tests', 'test_gpu_kernels.py'), os.path.join(ROOT, 'tests', 'test_gpu_kernel_generations.py')]
_W9_SEL = 'test_conv3x3_fwd_dgrad_wgrad or (test_wgrad_fp64 and (eng2 or worst))'
KNOB_RUNS = [(dict(OCR_W9_PLANES='0'), _BOTH, _W9_SEL), (dict(OCR_W9P_GENW='0'), _BOTH, _W9_SEL), (dict(OCR_W9P_GENW='2'), _BOTH, _W9_SEL),
             (dict(OCR_TN3_NST='5'), _BOTH[:1], 'test_gemm_tn_jobs')]
CHILD_TIMEOUT = 600
ENDED_BADLY = (124, 134, 137, 139)          # timeout, abort, kill, segmentation fault (or negative: ended by a signal)


@pytest.fixture(scope='module')
def knob_runs():
    """One pytest child per setting of KNOB_RUNS, at most four with the GPU open at a time, each with its own timeout, none ever started twice.
    A child that ends by a signal, an abort or its timeout stops the queue: settings not yet started are reported as not run."""
    import concurrent.futures
    stop = threading.Event()

    def run(job):
        env, files, sel = job
        if stop.is_set():
            return None, 'not run: an earlier child ended by a signal, an abort or its timeout'
        try:
            out = subprocess.run([sys.executable, '-m', 'pytest'] + files + ['-q', '-s', '-k', sel], capture_output=True, text=True, cwd=ROOT,
                                 env=dict(os.environ, OMP_NUM_THREADS='4', MKL_NUM_THREADS='4', **env), timeout=CHILD_TIMEOUT)
            rc, text = out.returncode, out.stdout
        except subprocess.TimeoutExpired as e:
            rc, text = 124, 'timed out: %s' % e
        if rc in ENDED_BADLY or rc < 0:
            stop.set()
        return rc, text
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        return list(ex.map(run, KNOB_RUNS))


@pytest.mark.parametrize("i", range(len(KNOB_RUNS)), ids=['%s=%s' % next(iter(e.items())) for e, _, _ in KNOB_RUNS])
def test_read_once_knobs_through_the_parity_tests(dev, knob_runs, i):
    """OCR_W9_PLANES=0 (wgrad9_kernel on the H = 4 / 8 layers), OCR_W9P_GENW=0 (general widths on wgrad9_kernel) and =2 (the zero-row wgrad9p
    instances on whole-image shapes too, the headline layers among them) through test_conv3x3_fwd_dgrad_wgrad and the float64 test above;
    OCR_TN3_NST=5 (gemm_tn3_kernel<5>) through test_gemm_tn_jobs.  tests/test_wgrad_dispatch_policy.py shows on the host that each setting
    moves shapes of the list, product sizes among them, onto the kernel it is there for."""
    rc, text = knob_runs[i]
    for line in (text or '').splitlines():
        if line.startswith('wgrad worst'):
            print(line)
    assert rc == 0, (KNOB_RUNS[i][0], rc, (text or '')[-3000:])
    assert ' passed' in text and ' skipped' not in text.splitlines()[-1], text[-500:]
