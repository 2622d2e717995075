"""-m gpu: the memory-bound kernels of every training step at product sizes and edge values.

Optimiser, pooling, element-wise ops, casts, softmax, dropout, inference batch norm, the strided pick, batch binding and the step
report, each against an independent CPU reference: fp64 arithmetic, torch's own `.to(bfloat16)` for rounding, the oracle's
`plan_exec.dropout_mask` for dropout.  Every case runs in three size regimes:
  sub_block  fewer work items than one workgroup has threads;
  ragged     a size that is not a multiple of the workgroup;
  past_cap   more work items than the kernel's capped grid has threads, so that its grid-stride loop goes round at least twice
             (the threshold is computed from the cap named beside each size table).
Selections, copies, integer outputs and bf16 values produced by an exact rule are compared bit for bit.  Every other bound is
derived in a comment from the operation's rounding and quotes the worst error measured on the MI355X.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pack_model import EDGE, EDGE_BITS, _plain_randoms  # noqa: E402,F401

from lstm_ctc_ocr_amd import ops  # noqa: E402
from oracle import plan_exec  # noqa: E402

BF = torch.bfloat16
WG = 256                # threads per workgroup of every kernel below but softmax (64: one wave per row)
RAG = 77                # work items beyond a whole number of workgroups / grids
EPS32 = 2.0 ** -24      # unit roundoff of fp32
REGIMES = ("sub_block", "ragged", "past_cap")


def _within(what, err, bound):
    assert err <= bound, "%s: error %.3e above the bound %.3e" % (what, err, bound)


def _within_each(what, err, bound):
    """err <= bound element by element (a NaN fails)."""
    bad = ~(err <= bound)
    assert not bool(bad.any()), "%s: %d of %d elements above their bound, worst %.3e against %.3e" % (
        what, int(bad.sum()), err.numel(), float(err[bad].max()) if bool((bad & (err == err)).any()) else float('nan'),
        float(bound[bad][0]))


def _rand(n, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) * (hi - lo) + lo


def _rand_bf16(shape, seed):
    return _rand(int(np.prod(shape)), seed).view(shape).to(BF)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _assert_bits_equal(what, got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (_bits(got) != _bits(want)).flatten().nonzero()
    assert bad.numel() == 0, "%s: %d of %d differ, first at flat index %d: got %r, want %r" % (
        what, bad.numel(), got.numel(), int(bad[0]), got.flatten()[bad[0]].item(), want.flatten()[bad[0]].item())


def _half_ulp_bf16(ref):
    """Half a bf16 ulp at each |ref| (fp64): a value in [2^(e-1), 2^e) has 8 significant bits, ulp 2^(e-8)."""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


# ================================================================================================ optimiser (csrc/optim.hip)
def _headline_flat_layout():
    """Length and regularised range of the flat parameter buffer of the headline network (BASELINE configs[1], LSTM_train),
    laid out as the engine lays it out."""
    from lstm_ctc_ocr_amd.engine import ALIGN
    from lstm_ctc_ocr_amd.layout import FlatLayout, execution_order
    from lstm_ctc_ocr_amd.models import get_network
    net = get_network('LSTM_train')
    lay = FlatLayout(net.param_specs.values(), ALIGN, order=[nd.name for nd in execution_order(net.get_output('logits'))])
    return lay.n_total, lay.reg_range


# ocr_optim_step_guarded2: update grid min(ceil(n / 1024), 2048) blocks of 256 threads x 4 floats (stride 2 Mi floats at the cap);
# norm pass (optim_prep_kernel) min(that, 1024) blocks (stride 1 Mi floats), unrolled four strides deep while i + 3 * stride < n.
PREP_STRIDE = 1024 * WG * 4
OPT_SIZES = {
    "sub_block": (200, (8, 180)),                       # 50 float4s: one workgroup, partly idle
    "5120": (5120, (516, 4612)),                        # test_optimizer's size: 5 blocks, fewer than the 32 partial-sum bins
    # n = 4 (mod 16) above 3 Mi floats: the four-deep main loop runs for the first 512 Ki + 4 floats of every lane, the tail loop for the
    # rest, 32 bins wrap 32 times; the update kernels go round their loop twice.  The range bounds fall inside a stride, not on one:
    # reg_begin in stride 0 behind the main loop's reach, reg_end in the main loop's fourth load of a lane.
    "ragged_past_unroll": (3 * PREP_STRIDE + PREP_STRIDE // 2 + 4, (4 * 250_003, 4 * 800_001)),
    "headline": None,                                   # the engine's flat buffer: ~7.2 M floats, every loop of both kernels
}
SOLVER_CONSTS = {"Adam": (0.9, 0.999, 1e-8), "Momentum": (0.9, 0.0, 0.0), "RMS": (0.9, 0.0, 1e-10)}
CLIP = 10.0             # train.py's clip_by_global_norm(g, 10.0), what the engine passes
WD = 1e-3               # the L2 term is then 1e-4 .. 0.3 of g: a missing or misplaced one moves the update far past its bound
LR0 = 0.1
# Parameter errors are measured against the step's largest update max|p_ref - p_prev|.  The reference starts every step from the
# state the device holds, so the error is this step's fp32 arithmetic: a handful of roundings of the update (<= ~8 * 2^-24 of it) plus
# the rounding of p itself when it is stored (half an ulp of max|p| <= 2^-25 * 2 / max|upd|; p stays below ~2 while the updates are
# >= 1e-4 here: <= 6e-7).  Moments: a handful of roundings of the moment itself.
TOL_P = 2e-6            # worst measured on MI355X: 8.1e-7 (Adam, ragged_past_unroll)
TOL_S = 6e-7            # ~10 roundings; worst measured on MI355X: 2.8e-7 (RMSProp mean square)


def _f32(x):
    return float(np.float32(x))


def _opt_size(name):
    return _headline_flat_layout() if name == "headline" else OPT_SIZES[name]


class _OptimRun(object):
    """Device optimiser state + the float64 reference of the TF update (train.py:73-85: L2 term folded into g, clip_by_global_norm,
    Adam / Momentum / RMSProp apply_gradients).  Scalars (step count, beta powers, lr, lr_t) are tracked on the host in double with the
    device's formulas; buffers are checked one step at a time, from the fp32 state the device holds."""

    def __init__(self, dev, solver, n, reg, seed):
        self.dev, self.solver, self.n, self.reg, self.seed = dev, solver, n, reg, seed
        self.b1, self.b2, self.eps = (_f32(c) for c in SOLVER_CONSTS[solver])
        self.p = (_rand(n, seed) * 1e-3).to(dev)
        self.s1 = torch.zeros(n, device=dev)
        self.s2 = torch.zeros(n, device=dev)
        self.sc = torch.zeros(ops.optim_scalar_count(), dtype=torch.float64, device=dev)
        ops.optim_init(self.sc, LR0)
        self.lr, self.t, self.b1t, self.b2t, self.lrt = LR0, 0, 1.0, 1.0, LR0
        self.skipped, self.timeouts, self.k = 0, 0, 0

    def set_lr(self, value, multiply):
        ops.optim_set_lr(self.sc, value, multiply=multiply)
        self.lr = self.lr * value if multiply else value

    def gradient(self, target_norm, wd, edge=False):
        """fp32 gradient whose combined norm ||g + wd * w (regularised range)|| is target_norm (solved in fp64).  On the regularised
        range g takes the sign of w: the kernel, like TF, forms g + wd * w in fp32, and where the two nearly cancel that rounding is
        amplified by Adam's and RMSProp's normalisation far beyond the step's own arithmetic — a property of the input, not of the kernel."""
        self.k += 1
        u = _rand(self.n, self.seed * 1000 + self.k).double()
        r0, r1 = self.reg
        w = torch.zeros(self.n, dtype=torch.float64)
        pr = self.p[r0:r1].double().cpu()
        u[r0:r1] = u[r0:r1].abs() * torch.where(pr < 0, -1.0, 1.0)
        if wd > 0:
            w[r0:r1] = _f32(wd) * pr
        a, b, c = float(u.dot(u)), float(u.dot(w)), float(w.dot(w))
        s = (-b + math.sqrt(b * b - a * (c - target_norm ** 2))) / a
        g = (s * u).float()
        if edge:                         # the premise of the clip-edge regime: the exact global norm is within 1 fp32 ulp of clip_norm
            norm = float((g.double() + w).norm())
            assert abs(norm - CLIP) <= 2.0 ** (math.floor(math.log2(CLIP)) - 23), norm
        return g

    def step(self, g, wd, guard=None, drop_flag=None, dropped=False, nbad=0):
        dev, n = self.dev, self.n
        r0, r1 = self.reg
        p0, m0, v0, sc0 = self.p.double().cpu(), self.s1.double().cpu(), self.s2.double().cpu(), self.sc.cpu()
        if dropped:
            keep = (self.p.clone(), self.s1.clone(), self.s2.clone())
        ops.optim_step(self.p, g.to(dev), self.s1, self.s2, self.reg, wd, CLIP, ops.SOLVERS[self.solver], self.b1, self.b2, self.eps,
                       self.sc, guard=guard, drop_flag=drop_flag)
        sc = self.sc.cpu()
        # the norm pass runs on dropped steps too: global norm and sum w^2 of THIS gradient, fp32 partial sums of <= 64 squares per lane
        # added in double (1e-5 relative is what the report promises; worst measured on MI355X: norm 2.0e-8, sum w^2 9.1e-8)
        gg = g.double()
        if wd > 0:
            gg[r0:r1] += _f32(wd) * p0[r0:r1]
        norm = float(gg.norm())
        reg2 = float(p0[r0:r1].square().sum()) if wd > 0 else 0.0
        _within("global norm, scalars[7]", abs(float(sc[7]) - norm) / norm, 1e-5)
        if wd > 0:
            _within("sum w^2, scalars[1]", abs(float(sc[1]) - reg2) / reg2, 1e-5)
        else:
            assert float(sc[1]) == 0.0                   # wd = 0: the regularised range is empty (r1 = r0)
        if dropped:
            self.skipped += 1
            self.timeouts += nbad
            assert torch.equal(self.p, keep[0]) and torch.equal(self.s1, keep[1]) and torch.equal(self.s2, keep[2])
            assert float(sc[72]) == 1.0 and float(sc[73]) == self.skipped and float(sc[74]) == self.timeouts
            for i in (2, 3, 4, 5, 6):                   # lr, lr_t, beta powers, step count: untouched
                assert float(sc[i]) == float(sc0[i]), i
            return
        assert float(sc[72]) == 0.0 and float(sc[73]) == self.skipped and float(sc[74]) == self.timeouts
        self.t += 1
        self.b1t *= self.b1
        self.b2t *= self.b2
        self.lrt = self.lr * math.sqrt(1.0 - self.b2t) / (1.0 - self.b1t)
        assert float(sc[6]) == self.t and float(sc[2]) == self.lr
        assert float(sc[4]) == self.b1t and float(sc[5]) == self.b2t           # the same double products as the device
        # lr_t = lr sqrt(1 - b2t) / (1 - b1t) in double, but the compiler contracts 1 - b^t into fma(-b^(t-1), b, 1): the unrounded
        # product, not the stored power.  The stored power's rounding (2^-53 b^t) becomes 2^-53 b^t / (1 - b^t) relative in 1 - b^t (halved
        # by the sqrt), plus a few roundings of the formula.  Measured on MI355X: 6.7e-15 at Adam's step 1 (b2t / (1 - b2t) = 999); lr_t
        # reaches the update kernels as a float, where this does not show.
        lrt_bound = 2.0 ** -53 * (0.5 * self.b2t / (1 - self.b2t) + self.b1t / (1 - self.b1t) + 4)
        _within("lr_t, scalars[3]", abs(float(sc[3]) - self.lrt) / self.lrt, lrt_bound)
        gg *= CLIP / max(norm, CLIP)
        b1, b2, eps = self.b1, self.b2, self.eps
        if self.solver == "Adam":
            m = b1 * m0 + (1 - b1) * gg
            v = b2 * v0 + (1 - b2) * gg * gg
            p = p0 - self.lrt * m / (v.sqrt() + eps)
        elif self.solver == "Momentum":
            m, v = b1 * m0 + gg, v0
            p = p0 - self.lr * m
        else:
            m, v = b1 * m0 + (1 - b1) * gg * gg, v0
            p = p0 - self.lr * gg / (m + eps).sqrt()
        upd = float((p - p0).abs().max())
        _within("%s p, step %d (relative to the update)" % (self.solver, self.t), float((self.p.double().cpu() - p).abs().max()) / upd, TOL_P)
        _within("%s state1, step %d" % (self.solver, self.t), float((self.s1.double().cpu() - m).abs().max()) / float(m.abs().max()), TOL_S)
        if self.solver == "Adam":
            _within("Adam state2, step %d" % self.t, float((self.s2.double().cpu() - v).abs().max()) / float(v.abs().max()), TOL_S)
        else:
            assert float(self.s2.abs().max()) == 0.0     # state2 is Adam's alone


# (clip regime, weight decay, lr change before the step): clip never active / active / the exact norm within 1 ulp of clip_norm
SCHEDULE = [("off", WD, None), ("on", WD, None), ("edge", WD, ("set", 0.05)), ("off", 0.0, None), ("on", WD, ("mul", 0.5)),
            ("edge", 0.0, None), ("off", WD, None)]
TARGET = {"off": 0.5 * CLIP, "on": 3.0 * CLIP, "edge": CLIP}


@pytest.mark.parametrize("size", list(OPT_SIZES))
@pytest.mark.parametrize("solver", ["Adam", "Momentum", "RMS"])
def test_optimizer_trajectory_against_float64_tf_update(dev, solver, size):
    n, reg = _opt_size(size)
    run = _OptimRun(dev, solver, n, reg, seed=7)
    for clip_regime, wd, lr_change in SCHEDULE:
        if lr_change is not None:
            run.set_lr(lr_change[1], multiply=lr_change[0] == "mul")
        run.step(run.gradient(TARGET[clip_regime], wd, edge=clip_regime == "edge"), wd)


@pytest.mark.parametrize("size", ["sub_block", "5120", "ragged_past_unroll"])
def test_optimizer_dropped_steps_guard_flag_and_step_report(dev, size):
    """Guard words (int words the persistent LSTM launches set to 1 on an expired wait; 0, or -1 in a block the caller prepared, is no
    error) and the data-parallel drop flag (> 0: that many ranks raised it).  A dropped step leaves parameters, moments, step count and
    beta powers bit-identical; the next step equals the reference that skipped it.  guard_flag and step_report read the same words."""
    n, reg = _opt_size(size)
    run = _OptimRun(dev, "Adam", n, reg, seed=11)
    words = torch.zeros((32, 65), dtype=torch.int32, device=dev)       # word i = last int of row i
    pattern = [1 if i % 5 == 2 else (-1 if i % 3 == 0 else 0) for i in range(32)]
    words[:, -1] = torch.tensor(pattern, dtype=torch.int32, device=dev)
    addrs = torch.tensor([words[i, -1:].data_ptr() for i in range(32)], dtype=torch.int64, device=dev)
    probe = 31                                                          # the word under test; words 3 and 4 read -1 and 0
    guard = torch.tensor([words[probe, -1:].data_ptr(), words[3, -1:].data_ptr(), words[4, -1:].data_ptr()], dtype=torch.int64, device=dev)
    assert pattern[3] == -1 and pattern[4] == 0
    flag_buf = torch.zeros(2, device=dev)
    costs = _rand(1000, 3, 0.0, 30.0)
    report = torch.zeros(4, dtype=torch.float64, device=dev)
    gf = torch.zeros(1, device=dev)
    for flag in (None, 0.0, 1.0, 2.0):
        for word in (1, 0, -1):
            words[probe, -1] = word
            if flag is not None:
                flag_buf[0] = flag
            nbad = int(word == 1) + (int(flag + 0.5) if flag else 0)
            run.step(run.gradient(0.5 * CLIP, WD), WD, guard=guard, drop_flag=None if flag is None else flag_buf[:1],
                     dropped=nbad > 0, nbad=nbad)
            gf.fill_(-3.0)
            ops.guard_flag(guard, gf)
            assert float(gf) == (1.0 if word == 1 else 0.0)
            ops.step_report(costs.to(dev), run.sc, addrs, report)
            o, sc = report.cpu().numpy(), run.sc.cpu().numpy()
            bits = sum(1 << i for i in range(32) if (word if i == probe else pattern[i]) == 1)
            assert o[3] == bits + (2.0 ** 40 if nbad else 0.0), (flag, word)
            assert o[1] == sc[1] and o[2] == sc[7]
            _within("step_report mean cost", abs(o[0] - float(costs.double().mean())) / float(costs.double().mean()), 1e-15)
    run.step(run.gradient(0.5 * CLIP, WD), WD)                           # no guard at all after the dropped steps
    gf.fill_(-3.0)
    ops.guard_flag(None, gf)
    assert float(gf) == 0.0
    words[probe, -1] = 1
    ops.step_report(costs.to(dev), None, addrs, report)
    o = report.cpu().numpy()
    assert o[1] == 0.0 and o[2] == 0.0 and o[3] == sum(1 << i for i in range(32) if (1 if i == probe else pattern[i]) == 1)


# ================================================================================================ pooling (pool.hip, dsl_ops.hip)
# ocr_maxpool_fwd / _bwd and ocr_avgpool_bf16: one thread per (output window, 8-channel group), grid capped at 8192 workgroups.
POOL_CAP = 8192
POOL_OUT = {"sub_block": (1, 3, 5, 64),         # 120 items
            "ragged": (3, 13, 7, 24),           # 819 items
            "past_cap": (2, 810, 810, 16)}      # 2,624,400 items > 8192 * 256 = 2,097,152: the first quarter of the grid goes round twice
WINDOWS = [(2, 2), (1, 2), (2, 1)]


def _pool_input_shape(regime, kw, kh):
    Nb, Wo, Ho, C = POOL_OUT[regime]
    return Nb, Wo * kw, Ho * kh, C


def _pool_items(regime):
    Nb, Wo, Ho, C = POOL_OUT[regime]
    return Nb * Wo * Ho * C // 8


def test_pool_regimes_are_what_they_claim():
    assert _pool_items("sub_block") < WG and _pool_items("ragged") % WG != 0 and _pool_items("past_cap") > POOL_CAP * WG


def _cells(t, kw, kh):
    """The window cells of an NWHC map in the kernels' (and torch's) scan order: axis W outer, axis H inner."""
    return [(a, b, t[:, a::kw, b::kh]) for a in range(kw) for b in range(kh)]


def _maxpool_ref(x, dy, kw, kh, relu_mask):
    cells = _cells(x, kw, kh)
    m = cells[0][2]
    for _, _, c in cells[1:]:
        m = torch.maximum(m, c)
    dx = torch.zeros_like(x)
    taken = torch.zeros(m.shape, dtype=torch.bool)
    zero = torch.zeros((), dtype=x.dtype)
    for a, b, c in cells:                # the gradient goes to the FIRST maximum of its window
        win = (c == m) & ~taken
        taken |= win
        v = torch.where(win, dy, zero)
        if relu_mask:
            v = torch.where(c > 0, v, zero)
        dx[:, a::kw, b::kh] = v
    return m, dx


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kw,kh", WINDOWS)
def test_maxpool_bit_exact_with_first_max_routing(dev, regime, kw, kh):
    Nb, W, H, C = _pool_input_shape(regime, kw, kh)
    g = torch.Generator().manual_seed(kw * 10 + kh)
    # eighths in [-6/8, 9/8]: ties inside windows everywhere, ReLU zeros, all-negative windows for relu_mask = False
    x = torch.randint(-6, 10, (Nb, W, H, C), dtype=torch.int8, generator=g).to(BF) / 8
    dy = _rand_bf16((Nb, W // kw, H // kh, C), 5)
    y_ref, dx_ref = _maxpool_ref(x, dy, kw, kh, False)
    _, dxr_ref = _maxpool_ref(x, dy, kw, kh, True)
    if regime != "past_cap":             # the reference routes exactly as torch's max_pool2d gradient does
        xr = x.float().requires_grad_(True)
        yr = F.max_pool2d(xr.permute(0, 3, 1, 2), (kw, kh), (kw, kh)).permute(0, 2, 3, 1)
        yr.backward(dy.float())
        assert torch.equal(yr.detach().to(BF), y_ref) and torch.equal(xr.grad.to(BF), dx_ref)
    xd, dyd = x.to(dev), dy.to(dev)
    _assert_bits_equal("maxpool_fwd", ops.maxpool_fwd(xd, kw, kh), y_ref)
    out = torch.full_like(xd, float('nan'))
    _assert_bits_equal("maxpool_bwd", ops.maxpool_bwd(xd, dyd, kw, kh, relu_mask=False, out=out), dx_ref)
    out.fill_(float('nan'))
    _assert_bits_equal("maxpool_bwd relu_mask", ops.maxpool_bwd(xd, dyd, kw, kh, relu_mask=True, out=out), dxr_ref)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kw,kh", WINDOWS + [(1, 1)])
def test_avgpool_forward_and_backward(dev, regime, kw, kh):
    Nb, W, H, C = _pool_input_shape(regime, kw, kh)
    x = _rand_bf16((Nb, W, H, C), 21)
    dy = _rand_bf16((Nb, W // kw, H // kh, C), 22)
    xd = x.to(dev)
    y = torch.full((Nb, W // kw, H // kh, C), float('nan'), dtype=BF, device=dev)
    ops.avgpool(xd, y, Nb, W, H, C, kw, kh)
    # forward: the window sum of <= 4 bf16 values in fp32 (one rounding of at most 2^-24 per addition of the absolute sum, nearly always
    # exact), times 1/(kw kh) (exact), rounded once to bf16: half a bf16 ulp of the fp64 mean plus the fp32 sum's rounding.
    # Measured on MI355X: the worst element sits exactly on its bound (a mean halfway between two bf16 values).
    cells = [c.double() for _, _, c in _cells(x, kw, kh)]
    ref = sum(cells) / (kw * kh)
    acc = (kw * kh - 1) * EPS32 * sum(c.abs() for c in cells) / (kw * kh)
    bound = _half_ulp_bf16(ref.abs() + acc) + acc
    _within_each("avgpool fwd", (y.cpu().double() - ref).abs(), bound)
    # backward: every window cell gets dy * (1 / (kw kh)) rounded once to bf16 — exactly
    dx = torch.full((Nb, W, H, C), float('nan'), dtype=BF, device=dev)
    ops.avgpool(dy.to(dev), dx, Nb, W, H, C, kw, kh, backward=True)
    want = torch.empty_like(x)
    scaled = (dy.float() * _f32(1.0 / (kw * kh))).to(BF)
    for a, b, _ in _cells(want, kw, kh):
        want[:, a::kw, b::kh] = scaled
    _assert_bits_equal("avgpool bwd", dx, want)


# ================================================================================================ element-wise (stream_ops.hip)
ELT_CAP = 4096          # ocr_eltwise_bf16: grid_for(n / 8, 4096), 8 elements per thread
ELT_N = {"sub_block": 8 * 37, "ragged": 8 * (WG * 9 + RAG), "past_cap": 8 * (2 * ELT_CAP * WG + RAG)}


@pytest.mark.parametrize("regime", REGIMES)
def test_eltwise_all_ops_bit_exact(dev, regime):
    n = ELT_N[regime]
    a, b, acc = _rand_bf16((n,), 31), _rand_bf16((n,), 32), _rand_bf16((n,), 33)
    b[::3] = 0                           # b > 0 is false at exact zeros
    a[1::5] = -b[1::5]                   # a + b == 0: relu of an exact zero; -0 where b is 0
    af, bf_, accf = a.float(), b.float(), acc.float()
    zero = torch.zeros((), dtype=BF)
    want = {0: (af + bf_).to(BF),
            1: torch.where(af > 0, a, zero),     # max(-0, 0) is +0 on the device; torch.relu would keep the -0 that a holds
            2: torch.where(bf_ > 0, a, zero),
            3: torch.relu((af + bf_).to(BF)),
            4: (accf + torch.where(bf_ > 0, af, torch.zeros(()))).to(BF)}
    ad, bd = a.to(dev), b.to(dev)
    for op in range(5):
        out = acc.to(dev) if op == 4 else torch.full((n,), float('nan'), dtype=BF, device=dev)
        ops.eltwise(op, ad, None if op == 1 else bd, out)
        _assert_bits_equal("eltwise op %d" % op, out, want[op])


# ================================================================================================ strided pick (dsl_ops.hip)
SUB_CAP = 8192          # ocr_subsample_bf16: one thread per 8-channel group of the output (forward) / input (backward), 8192 workgroups
SUB_IN = {"sub_block": (1, 5, 7, 16),           # backward 70 items
          "ragged": (3, 23, 17, 24),            # backward 3519 items
          "past_cap": (2, 1621, 1621, 16)}      # forward at stride (2, 2) >= 2 * 810 * 810 * 2 = 2,624,400 items > 8192 * 256


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("sw,sh", [(1, 2), (2, 1), (2, 2)])
def test_subsample_every_offset_and_its_adjoint(dev, regime, sw, sh):
    Nb, W, H, C = SUB_IN[regime]
    x = _rand_bf16((Nb, W, H, C), 41)
    xd = x.to(dev)
    for ow in range(sw):
        for oh in range(sh):
            for short in (0, 1) if regime == "ragged" else (0,):      # one output row / column fewer than fits: backward's upper guards
                Wo, Ho = (W - ow - 1) // sw + 1 - short, (H - oh - 1) // sh + 1 - short
                if regime == "past_cap":
                    assert Nb * Wo * Ho * C // 8 > SUB_CAP * WG
                what = "stride (%d, %d) offset (%d, %d) out %dx%d" % (sw, sh, ow, oh, Wo, Ho)
                y = torch.full((Nb, Wo, Ho, C), float('nan'), dtype=BF, device=dev)
                ops.subsample(xd, y, Nb, W, H, C, Wo, Ho, sw, sh, ow, oh)
                pick = x[:, ow::sw, oh::sh][:, :Wo, :Ho]
                _assert_bits_equal("subsample fwd " + what, y, pick)
                dy = _rand_bf16((Nb, Wo, Ho, C), 42 + ow + 2 * oh)
                dx = torch.full((Nb, W, H, C), float('nan'), dtype=BF, device=dev)      # poisoned: backward writes every element
                ops.subsample(dy.to(dev), dx, Nb, W, H, C, Wo, Ho, sw, sh, ow, oh, backward=True)
                want = torch.zeros_like(x)
                want[:, ow::sw, oh::sh][:, :Wo, :Ho] = dy
                _assert_bits_equal("subsample bwd " + what, dx, want)
                if x.numel() < (1 << 23):     # <S x, dy> = <x, S^T dy> in fp64 (implied by the bit checks above; kept where it is cheap)
                    lhs = float(y.cpu().double().flatten().dot(dy.double().flatten()))
                    rhs = float(x.double().flatten().dot(dx.cpu().double().flatten()))
                    _within("adjointness " + what, abs(lhs - rhs), 1e-12 * max(abs(lhs), 1.0))


# ================================================================================================ softmax (dsl_ops.hip)
SOFTMAX_CAP = 8192      # ocr_softmax_f32: one 64-thread workgroup per row, 8192 workgroups
SOFTMAX_ROWS = {"sub_block": 3, "ragged": 1000 + RAG, "past_cap": 2 * SOFTMAX_CAP + RAG}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("C", [1, 5, 63, 64, 65, 96, 200, 1000])
def test_softmax_against_float64(dev, regime, C):
    rows = SOFTMAX_ROWS[regime]
    x = _rand(rows * C, 50 + C, -4.0, 4.0).view(rows, C)
    x[0::3] *= 20.0                                      # logit spreads of +-80
    x[2::5] = _rand(len(range(2, rows, 5)), 51, -50.0, 50.0)[:, None]      # rows of equal values
    y = torch.full_like(x, float('nan'), device=dev)
    ops.softmax(x.to(dev), y)
    y = y.cpu().double()
    x64 = x.double()
    t = x64 - x64.max(-1, keepdim=True).values
    e = t.exp()
    ref = e / e.sum(-1, keepdim=True)
    # Device: d = x - max (fp32, 2^-24 |d|), __expf(d) = v_exp_f32(d * log2e) (the product's rounding and log2e's own are another
    # 1.5 * 2^-24 |d| in the exponent, v_exp_f32 ~1 ulp), the row sum of ceil(C / 64) terms per lane and a 6-level butterfly, 1 / s and
    # the product (correctly rounded).  Relative error of element i, with T = sum_j p_j |t_j| the sum's weighted share of the
    # exponent errors:  2^-24 * (3 (|t_i| + T) + ceil(C / 64) + 12).  Below 2^-100 (where v_exp_f32 may flush) absolute 2^-99.
    # Measured on MI355X: worst element 0.60 of its bound (2.4e-7 relative), worst row sum 2.2e-7 off 1.
    T = (ref * t.abs()).sum(-1, keepdim=True)
    rel = EPS32 * (3 * (t.abs() + T) + math.ceil(C / 64) + 12)
    err = (y - ref).abs()
    big = ref >= 2.0 ** -100
    _within_each("softmax C=%d relative" % C, err[big], (rel * ref)[big])
    _within_each("softmax C=%d absolute below 2^-100" % C, err[~big], torch.full_like(err[~big], 2.0 ** -99))
    _within_each("softmax C=%d row sums" % C, (y.sum(-1) - 1.0).abs(), (rel * ref).sum(-1) + C * 2.0 ** -99)


# ================================================================================================ inference batch norm (dsl_ops.hip)
# forward: dsl_grid(M * C / 8) (cap 4096 workgroups of 256 threads x 8 channels); backward: one workgroup per 256 rows x 64-channel slab,
# grid capped at 2048.  C = 72 leaves a partial second slab.
BN_M = {"sub_block": 24,                        # 216 forward items, one backward block per slab
        "ragged": 1000 + 13,                    # M % 256 != 0
        "past_cap": 256 * 1100 + RAG}           # backward 1101 x 2 = 2202 blocks > 2048; forward 2.5 M items > 4096 * 256
BN_C = 72
BN_EPS = 1e-3


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("relu", [True, False])
def test_bn_infer_forward_and_backward(dev, regime, relu):
    M, C = BN_M[regime], BN_C
    if regime == "past_cap":
        assert ((M + 255) // 256) * ((C + 63) // 64) > 2048 and M * C // 8 > 4096 * WG
    x, dy = _rand_bf16((M, C), 61), _rand_bf16((M, C), 62)
    gamma, beta, mean = 1 + 0.3 * _rand(C, 63), 0.2 * _rand(C, 64), 0.1 * _rand(C, 65)
    var = 1 + 0.5 * _rand(C, 66, 0.0, 1.0)
    dg0, db0 = _rand(C, 67, -5.0, 5.0), _rand(C, 68, -5.0, 5.0)           # backward accumulates onto these
    y = torch.full((M, C), float('nan'), dtype=BF, device=dev)
    ops.bn_infer_fwd(x.to(dev), gamma.to(dev), beta.to(dev), mean.to(dev), var.to(dev), BN_EPS, relu, y)
    x64, dy64 = x.double(), dy.double()
    rs = 1.0 / (var.double() + _f32(BN_EPS)).sqrt()
    sc = gamma.double() * rs
    xm = x64 - mean.double()
    pre = xm * sc + beta.double()
    ref = pre.clamp_min(0.0) if relu else pre
    # forward: the fp32 value (sub, rsqrt ~1 ulp, two products, add) is within delta = 2^-21 (|x - mean| |sc| + |beta|) of the fp64
    # pre-activation, then rounded to bf16 once: |y - ref| <= half a bf16 ulp at |ref| + 2 delta, plus 2 delta.
    # Measured on MI355X: the worst element reaches its bound (a pre-activation halfway between two bf16 values).
    delta = 2.0 ** -21 * (xm.abs() * sc.abs() + beta.double().abs())
    yc = y.cpu()
    _within_each("bn_infer_fwd", (yc.double() - ref).abs(), _half_ulp_bf16(ref.abs() + 2 * delta) + 2 * delta)
    if relu:                             # the mask can differ from the fp64 one only where the pre-activation is within 2 delta of zero
        flip = (yc > 0) != (pre > 0)
        _within_each("bn_infer_fwd ReLU sign flips", pre.abs()[flip], 2 * delta[flip])
    # backward takes y as an input and masks dy where y <= 0: the reference masks with the same y, so every element is compared
    dx = torch.full((M, C), float('nan'), dtype=BF, device=dev)
    dg, db = dg0.to(dev, copy=True), db0.to(dev, copy=True)
    ops.bn_infer_bwd(x.to(dev), y, dy.to(dev), gamma.to(dev), mean.to(dev), var.to(dev), dg, db, BN_EPS, relu, dx)
    dyp = dy64 * (yc > 0) if relu else dy64
    dx_ref = dyp * sc
    # dx = bf16(dy' * gamma * rsqrt(var + eps)): the fp32 value within 2^-21 relative, then one bf16 rounding (worst measured on
    # MI355X: at its bound, a half-ulp tie)
    fp32 = 2.0 ** -21 * dx_ref.abs()
    _within_each("bn_infer_bwd dx", (dx.cpu().double() - dx_ref).abs(), _half_ulp_bf16(dx_ref.abs() + fp32) + fp32)
    # dgamma / dbeta: fp32 chains of 8 rows per lane, 32 lanes in LDS, then one atomic per block onto the start value: at most
    # L = 8 + 32 + ceil(M / 256) + 1 additions, each rounding <= 2^-24 of the absolute sum, plus 4 roundings per term
    # (worst measured on MI355X: 0.027 of the bound)
    L = 8 + 32 + (M + 255) // 256 + 1
    terms_g = dyp * xm * rs
    for what, got, start, terms in (("dgamma", dg, dg0, terms_g), ("dbeta", db, db0, dyp)):
        want = start.double() + terms.sum(0)
        bound = (L + 4) * EPS32 * (start.double().abs() + terms.abs().sum(0))
        _within_each("bn_infer_bwd " + what, (got.cpu().double() - want).abs(), bound)


# ================================================================================================ dropout (dsl_ops.hip)
DROP_CAP = 4096         # ocr_dropout_bf16: dsl_grid(n / 8), 8 elements per thread
DROP_N = {"sub_block": 8 * 37, "ragged": 8 * (WG * 7 + RAG), "past_cap": 8 * (2 * DROP_CAP * WG + RAG)}
DROP_LAYER = 'fc_drop'


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("keep_prob", [1.0, 0.7, 0.1])
def test_dropout_mask_is_the_oracles(dev, regime, keep_prob):
    import zlib
    n = DROP_N[regime]
    seed = zlib.crc32(DROP_LAYER.encode()) ^ 0x5bd1e995                 # the engine's seed of a layer (plan_exec.dropout_mask)
    x, dy = _rand_bf16((n,), 71), _rand_bf16((n,), 72)
    xd, dyd = x.to(dev), dy.to(dev)
    inv = np.float32(1.0) / np.float32(keep_prob)                         # the kernel's fp32 1 / keep_prob
    zero = torch.zeros((), dtype=BF)
    for step in (None, 5):               # None: a NULL step counter, which means step 0
        counter = None if step is None else torch.tensor([float(step)], dtype=torch.float64, device=dev)
        out_f = torch.full((n,), float('nan'), dtype=BF, device=dev)
        out_b = torch.full((n,), float('nan'), dtype=BF, device=dev)
        ops.dropout(xd, out_f, seed, counter, keep_prob)                  # forward on activations ...
        ops.dropout(dyd, out_b, seed, counter, keep_prob)                 # ... and backward on gradients: the same mask
        if keep_prob == 1.0:
            _assert_bits_equal("dropout keep 1 fwd", out_f, x)
            _assert_bits_equal("dropout keep 1 bwd", out_b, dy)
            continue
        keep = plan_exec.dropout_mask((n,), DROP_LAYER, 0 if step is None else step, keep_prob) > 0
        for what, out, src in (("fwd", out_f, x), ("bwd", out_b, dy)):
            _assert_bits_equal("dropout %s keep %.1f step %s" % (what, keep_prob, step), out,
                               torch.where(keep, (src.float() * float(inv)).to(BF), zero))


# ================================================================================================ casts (stream_ops.hip)
# EDGE_BITS, EDGE and _plain_randoms: tests/pack_model.py (shared with the weight re-pack tests)


def _assert_bf16_rule(what, got, src):
    """Every finite value and +-Inf rounds as torch's .to(bfloat16) does, bit for bit; every NaN stays a NaN (of either sign)."""
    got, src = got.cpu(), src.cpu()
    nan = torch.isnan(src)
    assert bool(torch.isnan(got[nan].float()).all()), what + ": a NaN did not stay a NaN"
    _assert_bits_equal(what, got[~nan], src[~nan].to(BF))


CAST_CAP = 4096         # ocr_cast_f32_bf16: grid_for((n + 3) / 4), 4 floats per thread; n % 4 floats by the f2bf tail
CAST_N = {"sub_block": 4 * 37, "ragged": 4 * (WG * 5 + RAG), "past_cap": 4 * (2 * CAST_CAP * WG + RAG)}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rest", [0, 1, 2, 3])
def test_cast_bf16_edge_values_in_body_and_tail(dev, regime, rest):
    n = CAST_N[regime] + rest
    body = n - rest
    k = len(EDGE)
    x = _plain_randoms(n, 80 + rest)
    x[:k] = EDGE                         # the pack_bf2 (v_cvt_pk_bf16_f32) body, first and last float4s
    x[body - k:body] = EDGE
    xd = x.to(dev)
    out = torch.empty(n, dtype=BF, device=dev)
    ops.cast_bf16(xd, out)
    _assert_bf16_rule("cast_bf16 n=%d" % n, out, x)
    for j in range(0, k, rest) if rest else ():          # every edge value through the f2bf tail, `rest` at a time
        tail = EDGE[torch.arange(j, j + rest) % k]
        xd[body:] = tail.to(dev)
        ops.cast_bf16(xd, out)
        _assert_bf16_rule("cast_bf16 tail of n=%d" % n, out[body:], tail)
        _assert_bf16_rule("cast_bf16 body of n=%d" % n, out[body - k:body], EDGE)


# ocr_cast2d_f32_bf16 / ocr_tnc_to_ntc_bf16: grid_for (cap 4096 workgroups) over float4s / elements
CAST2D = {"sub_block": (3, 40, 44, 48), "ragged": (37, 200, 212, 204), "past_cap": (2 * 4096 * WG * 4 // 512 + 3, 512, 520, 528)}
TNC = {"sub_block": (3, 2, 36), "ragged": (13, 7, 37), "past_cap": (64, 65, 512)}     # T N C; 2,129,920 > 4096 * 256 * 2


@pytest.mark.parametrize("regime", REGIMES)
def test_cast2d_and_tnc_to_ntc_edge_values(dev, regime):
    rows, cols, ldin, ldout = CAST2D[regime]
    src = _plain_randoms(rows * ldin, 90).view(rows, ldin)
    k = len(EDGE)
    src[0, :k] = EDGE
    src[-1, cols - k:cols] = EDGE
    src[:, cols:] = float('nan')         # past the columns: never read into the output
    dst = torch.full((rows, ldout), -7.0, dtype=BF, device=dev)
    ops.cast2d_bf16(src.to(dev), ldin, dst, ldout, rows, cols)
    dst = dst.cpu()
    _assert_bf16_rule("cast2d_bf16", dst[:, :cols].contiguous(), src[:, :cols].contiguous())
    assert bool((dst[:, cols:] == -7.0).all())
    T, N, C = TNC[regime]
    g = _plain_randoms(T * N * C, 91).view(T, N, C)
    g.view(-1)[:k] = EDGE
    g.view(-1)[-k:] = EDGE
    o = torch.empty((N, T, C), dtype=BF, device=dev)
    ops.tnc_to_ntc_bf16(g.to(dev), o, 1.0)
    _assert_bf16_rule("tnc_to_ntc_bf16", o, g.permute(1, 0, 2).contiguous())


# ================================================================================================ input binding (stream_ops.hip)
U8_CAP = 4096           # ocr_u8_to_unit_f32 / ocr_bind_batch: grid_for(n / 4), 4 pixels per thread
U8_N = {"sub_block": 4 * 128, "ragged": 4 * (WG * 3 + RAG), "past_cap": 4 * (2 * U8_CAP * WG + RAG)}


def _u8_pixels(n, seed):
    g = torch.Generator().manual_seed(seed)
    pix = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    pix[:256] = torch.arange(256, dtype=torch.uint8)                      # every byte value, at the start and at the end
    pix[-256:] = torch.arange(256, dtype=torch.uint8).flip(0)
    return pix


@pytest.mark.parametrize("regime", REGIMES)
def test_u8_to_unit_and_bind_batch(dev, regime):
    n = U8_N[regime]
    pix = _u8_pixels(n, 100)
    want = torch.from_numpy(pix.numpy().astype(np.float32) / 255.)        # groupBatch's astype(float32) / 255.
    out = torch.full((n,), float('nan'), device=dev)
    ops.u8_to_unit_f32(pix.to(dev), out)
    _assert_bits_equal("u8_to_unit_f32", out, want)
    # bind_batch: the int32 vectors are copied by the LAST workgroup (grid 1 only for sub_block); labels longer than a workgroup
    g = torch.Generator().manual_seed(101)
    sl = torch.randint(1, 64, (64,), dtype=torch.int32, generator=g)
    lab = torch.randint(1, 63, (700,), dtype=torch.int32, generator=g)
    ll = torch.randint(1, 11, (64,), dtype=torch.int32, generator=g)
    for src, ref in ((pix, want), (_rand(n, 102), None)):
        ref = src if ref is None else ref                                  # fp32 pixels are copied as they are
        x = torch.full((n,), -1.0, device=dev)
        d_sl = torch.full((80,), -5, dtype=torch.int32, device=dev)
        d_lab = torch.full((800,), -5, dtype=torch.int32, device=dev)
        d_ll = torch.full((80,), -5, dtype=torch.int32, device=dev)
        ops.bind_batch(src.to(dev), x, sl.to(dev), d_sl, lab.to(dev), d_lab, ll.to(dev), d_ll)
        _assert_bits_equal("bind_batch %s pixels" % src.dtype, x, ref)
        for what, d, s in (("seq_len", d_sl, sl), ("labels", d_lab, lab), ("labels_len", d_ll, ll)):
            d = d.cpu()
            assert torch.equal(d[:s.numel()], s) and bool((d[s.numel():] == -5).all()), what


@pytest.mark.parametrize("M,C,lda", [(128 * 5 + 37, 2048, 2056), (77, 8, 16), (128 * 40 + 1, 520, 528)])
def test_colsum_strided_rows(dev, M, C, lda):
    a = _rand_bf16((M, lda), 110)
    out0 = _rand(C, 111, -10.0, 10.0)
    out = out0.to(dev, copy=True)
    ops.colsum(a.to(dev)[:, :C], out)
    # fp32: a lane adds up to 128 rows of its block in sequence, the block's row lanes are added, one atomic per block of 128 rows
    # onto the start value: at most L = 128 + 256 / (C / 8) + ceil(M / 128) + 1 additions of <= 2^-24 of the absolute sum each
    # (worst measured on MI355X: 0.001 of the bound)
    terms = a[:, :C].double()
    want = out0.double() + terms.sum(0)
    L = 128 + max(1, 256 // (C // 8)) + (M + 127) // 128 + 1
    bound = L * EPS32 * (out0.double().abs() + terms.abs().sum(0))
    _within_each("colsum", (out.cpu().double() - want).abs(), bound)
