"""The float64 reference of the 3x3 convolution forward and data gradient (and of gemm_nt), the per-element bound, the two input regimes
and the case list of test_conv3_reference.py (the checker and the claims pinned without a GPU) and test_gpu_conv3_fp64.py (the kernels).

Reference.  The definition, as conv_shapes.wgrad_products has it for the weight gradient: nine shifted matmuls on the zero-padded input, in
float64, from the bf16-rounded operands (x [Nb, W, H, Cin], tap a along W, tap b along H, weights HWIO):
    forward        y[n, w, h]  = sum_ab x[n, w + a - 1, h + b - 1] @ w[a][b]  (+ bias)
    data gradient  dx[n, w, h] = sum_ab dy[n, w + 1 - a, h + 1 - b] @ w[a][b]^T      (the same taps transposed: what the device computes from
                                                                                      ops.pack_conv_dgrad's pack of the same HWIO weights)
    scale          the same sums over |x| |w| (+ |bias|) (+ |y_old| for the accumulate form): each element's own sum of term magnitudes, the
                   unit of conv_shapes.wgrad_ref64 - a summation-order error is a small multiple of 2^-24 in it whatever the element's value.
No library convolution is called.

Bound, per element, none excluded, with e = CONV_TOL * scale:
    bf16 outputs   |got - ref'| <= e + ulp_bf16(|ref'| + e) / 2     ref' = the reference after the exact epilogue: max(ref, 0) for ReLU,
                                                                    y_old + ref for accumulate.  The ulp is taken at |ref'| + e, so that a
                                                                    result rounded across a power of two is covered.
    masked         an element whose mask is not positive (as a bf16 number: +0, -0 and negatives are not) is zero - with accumulate: is y_old,
                   bit for bit.
    fp32 outputs   |got - ref| <= e                                 (gemm_nt only)
    scale == 0     exact.
check() returns the worst ratio |got - ref'| / bound with its index.

CONV_TOL comes from the reference side only, as WGRAD_TOL does (test_gpu_kernel_generations.py), never from a device result: the same nine
matmuls in torch.float32 on the CPU against the float64 ones, in units of scale, over every case of CASES (forward with bias, data gradient)
and of GEMM_CASES, in both regimes.  Measured (test_conv3_reference.py::test_conv_tol_is_the_reference_side_error_times_eight asserts it):
    convolution forward   2.2e-8 (2, 12, 4, 256, 512) uniform .. 2.47e-7 (1100, 1, 1, 64, 64) activations
    data gradient         1.4e-8 (2, 12, 4, 256, 512) uniform .. 3.88e-7 (1100, 1, 1, 64, 64) activations
    gemm_nt               1.8e-8 (70, 520, 2048) uniform      .. 5.97e-7 (25600, 512, 320) activations
    uniform regime alone 1.4e-8 .. 1.7e-7; activations 7.5e-8 .. 5.97e-7 (few large terms per element: the one fp32 rounding of a term counts)
    CONV_TOL = 8 x 5.97e-7 = 4.78e-6
The factor 8 is WGRAD_TOL's, for the same reason: the kernels sum in sequential MFMA chains (9 Cin / 32 steps, K-split halves joined in
fp32), the CPU product sums blockwise.  A typical element then has e three orders of magnitude below its half ulp: the bf16 bound IS the half
ulp, and truncation, a bf16 exchange of K-split partial sums or a bias added after the rounding do not fit (test_conv3_reference.py).

Regimes, seeded and bf16-rounded, finite values only:
    uniform       test_conv3x3_fwd_dgrad_wgrad's gen inputs (seeds 1 .. 5, weights x 0.05), kept for continuity with the 1e-2 bars
    activations   what the layers see.  x = relu(normal) * s_c with the per-channel s_c log-uniform over 2^-6 .. 2^4 (stratified: the exponents
                  are a shuffled linspace, so the spread is 2^10 at every channel count); weights normal * sqrt(2 / (9 Cin)) times a
                  per-output-channel factor in 2^-2 .. 2^2; bias normal; dy half zeros, else log-uniform in magnitude over 2^-20 .. 2^-2 with
                  random sign; the mask holds +0, -0, the smallest positive normal bf16 (2^-126), a positive subnormal bf16 (2^-130) and
                  small negatives (-2^-130, -2^-126, -2^-10) among normal values; y_old normal at the result's own scale (its rms).
                  assert_regime() asserts from the generated data: at least 40 % zeros in x, channel-scale spread at least 2^8.

CASES: each shape with the kernel it is there for, as data: {knob setting: (forward choice, data-gradient choice)}, checked against
ops.conv3x3_kernel_choice by test_conv3_reference.py (the host-only query reports 256 CUs without a device, the MI355X's count).  The data
gradient of (Nb, W, H, Ci, Co) is the convolution (Nb, W, H, Co, Ci) with the mask.  A data-gradient choice of None: the call is REFUSED
(OCR_STATUS_INVALID) - found by this work: conv_halo takes any Cout % 4 == 0 forward, but the gradient of such a layer has Cin = Cout, and
the register-staged convolution mode needs Cin % 32 == 0 (a K tile stays inside one tap), so layers with Cout in {36, 40, 68, 100, 132}
have a forward and no data gradient; the query answers "gemm" for them although the call refuses.  The GPU test asserts the refusal."""
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CONV_TOL = 8 * 5.97e-7            # module docstring
BF = torch.bfloat16
FAMILIES = ("gemm", "conv_halo", "conv_k2/A", "conv_k2/D", "conv_k3/A", "conv_k3/D", "conv_k3w/A", "conv_k3w/D", "conv_ws")
REGIMES = ("uniform", "activations")

SETTINGS = {   # knob settings, read once per process: every one but "default" runs in a child interpreter
    "default": {},
    "K2A": dict(OCR_CONV_K2="1", OCR_K2_CFG="A"), "K2D": dict(OCR_CONV_K2="1", OCR_K2_CFG="D"),
    "K2A+noK3": dict(OCR_CONV_K2="1", OCR_K2_CFG="A", OCR_CONV_K3="0"), "K2D+noK3": dict(OCR_CONV_K2="1", OCR_K2_CFG="D", OCR_CONV_K3="0"),
    "noK2": dict(OCR_CONV_K2="0"), "WS2": dict(OCR_CONV_WS="2")}

_H, _K2A, _K2D, _K3A, _K3D, _WA, _WD, _WS, _G = ("conv_halo", "conv_k2/A", "conv_k2/D", "conv_k3/A", "conv_k3/D", "conv_k3w/A", "conv_k3w/D",
                                                  "conv_ws", "gemm")

CASES = [   # ((Nb, W, H, Ci, Co), {setting: (forward, data gradient)}, what the shape is there for)
    ((16, 64, 4, 64, 64), {"default": (_H, _H), "K2D": (_K3D, _K3D), "K2D+noK3": (_K2D, _K2D)}, "one input chunk, 9 K steps"),
    ((16, 64, 4, 192, 192), {"default": (_H, _H), "K2D": (_K3D, _K3D), "K2D+noK3": (_K2D, _K2D)}, "three chunks (odd count), three channel tiles"),
    ((16, 32, 8, 128, 128), {"default": (_H, _H), "K2A": (_K3A, _K3A), "K2D": (_K3D, _K3D), "K2A+noK3": (_K2A, _K2A), "WS2": (_WS, _WS)},
     "tile A at its smallest; conv_ws's H = 8, Cin = 128 K-split instance"),
    ((16, 16, 16, 64, 64), {"default": (_H, _H), "K2D": (_K3D, _K3D), "WS2": (_WS, _WS)}, "conv_k3 with a single halo buffer; conv_ws's Cin = 64 instance"),
    ((16, 16, 16, 128, 192), {"default": (_H, _H), "K2D": (_K3D, _K3D), "K2A": (_H, _K3A), "WS2": (_WS, _H)},
     "conv_k3 with two buffers at H = 16; conv_ws's H = 16, Cin = 128 instance"),
    ((64, 32, 2, 64, 128), {"default": (_H, _H), "K2A": (_WA, _H), "K2D": (_WD, _WD)}, "H = 2: general width only"),
    ((64, 17, 4, 128, 64), {"default": (_H, _H), "K2A": (_H, _WA), "K2D": (_WD, _WD)}, "general width: tiles cross up to four image boundaries"),
    ((32, 17, 8, 64, 128), {"default": (_H, _H), "K2A": (_WA, _H), "K2D": (_WD, _WD)}, "general width at H = 8"),
    ((17, 61, 4, 64, 64), {"default": (_H, _H), "K2D": (_K2D, _K2D)}, "M = 4148: ragged last 256-pixel tile"),
    ((5, 52, 16, 128, 128), {"default": (_H, _H), "K2A": (_K2A, _K2A), "K2D": (_K2D, _K2D)}, "M = 4160: ragged"),
    ((23, 60, 3, 64, 192), {"default": (_H, _H), "K2D": (_K2D, _K2D)}, "odd H = 3"),
    ((33, 62, 4, 128, 256), {"default": (_K2D, _H), "noK2": (_H, _H)}, "default conv_k2 forward"),
    ((16, 64, 4, 128, 512), {"default": (_K3D, _H), "noK2": (_H, _H)}, "default conv_k3 forward"),
    ((32, 64, 4, 128, 256), {"default": (_K3D, _H)}, "default conv_k3 forward"),
    ((4, 64, 4, 64, 100), {"default": (_H, None)}, "conv_halo with a ragged channel tile (64 + 36)"),
    ((9, 30, 4, 128, 68), {"default": (_H, None)}, "conv_halo with a 4-channel last tile, two chunks"),
    ((4, 64, 4, 64, 96), {"default": (_H, _G)}, "ragged channel tile whose data gradient exists (Cin = 96: the register-staged convolution mode)"),
    ((5, 17, 13, 192, 132), {"default": (_H, None)}, "conv_halo with odd H = 13, three chunks and a 4-channel last tile"),
    ((28, 64, 16, 64, 132), {"default": (_H, None)}, "conv_halo's 128-channel tile by plan_halo's rule (448 workgroups); the second tile holds 4 channels"),
    ((56, 64, 4, 64, 512), {"default": (_H, _H)}, "conv_halo's 128-channel tile, whole tiles"),
    ((3, 12, 30, 64, 64), {"default": (_H, _H)}, "conv_halo at H = 30: six-piece halo, M = 1080 ragged"),
    ((1100, 1, 1, 64, 64), {"default": (_H, _H)}, "W = H = 1: every tap but the centre is padding"),
    ((64, 16, 16, 64, 512), {"default": (_WS, _H)}, "default conv_ws: two tiles per persistent workgroup, XCD map on"),
    ((2, 12, 4, 256, 512), {"default": (_G, _G)}, "gemm, M < 1024"),
    ((3, 7, 5, 96, 36), {"default": (_G, None)}, "gemm, nothing aligned (Cin = 72 of the first draft is refused: Cin % 32)"),
    ((5, 24, 12, 96, 40), {"default": (_G, None)}, "gemm, Cin % 64 != 0 at M >= 1024"),
    ((2, 18, 32, 64, 128), {"default": (_G, _G)}, "H > 30: implicit-GEMM convolution mode, tiny-grid BN = 128"),
    ((2, 18, 32, 64, 64), {"default": (_G, _G)}, "H > 30: implicit-GEMM convolution mode, BN = 64"),
]
ACCUM_UNREACHABLE = ("conv_ws",)      # plan_ws takes no accumulate flag: the shape falls through to the next family
GRAD_UNREACHABLE = ()                 # every family takes a masked data gradient under some setting

GEMM_CASES = [   # (M, N, K): one ig_try_dispatch instance each at K = 64 (one step) and K = 320 (more steps than stages), and the register-staged kernel
    (1100, 132, 64), (1100, 132, 320),          # 4-wave BN 64
    (7168, 1024, 64), (7168, 1024, 320),        # 4-wave BN 128
    (25600, 512, 64), (25600, 512, 320),        # 8-wave BN 128
    (32768, 512, 64), (32768, 512, 320),        # BN 256
    (102400, 64, 64),                           # 8-wave BN 64
    (300, 132, 72), (70, 520, 2048)]            # gemm_nt_kernel (M < 1024)


def case_ids():
    return ["%dx%dx%d-%d-%d" % s for s, _, _ in CASES]


def cases_of(setting):
    return [(s, c[setting]) for s, c, _ in CASES if setting in c]


# ------------------------------------------------------------------------------------------- number formats
def bf(t):
    """Round to bf16 (nearest even), returned as float32."""
    return t.to(BF).to(torch.float32)


def bf_truncate(t32):
    """float32 -> bf16 by dropping the low 16 bits (the first mutation), returned as float32."""
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32)


def ulp_bf16(v):
    """The spacing of bf16 numbers at magnitude v (float64, v >= 0): 2^(floor(log2 v) - 7), 2^-133 in the subnormal range."""
    _, e = torch.frexp(v.clamp_min(2.0 ** -126))          # v = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 8)


# ------------------------------------------------------------------------------------------- reference
def conv_products(x, w, dtype=torch.float64):
    """sum_ab shift_ab(x) @ w[a][b]: x [Nb, W, H, Cin], w [3, 3, Cin, Cout] -> [Nb, W, H, Cout] in `dtype`."""
    Nb, W, H, Ci = x.shape
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))
    wd = w.to(dtype)
    y = torch.zeros((Nb * W * H, w.shape[-1]), dtype=dtype)
    for a in range(3):
        for b in range(3):
            y += xp[:, a:a + W, b:b + H, :].reshape(-1, Ci) @ wd[a, b]
    return y.reshape(Nb, W, H, -1)


def dgrad_weights(w):
    """The taps of the data gradient as a convolution of dy: w'[a][b] = w[2 - a][2 - b]^T  ([3, 3, Cout, Cin])."""
    return w.flip(0, 1).transpose(2, 3).contiguous()


def fwd_ref(x, w, bias=None, dtype=torch.float64):
    """(ref, scale) of the forward."""
    ref, scale = conv_products(x, w, dtype), conv_products(x.abs(), w.abs(), dtype)
    if bias is not None:
        ref, scale = ref + bias.to(dtype), scale + bias.abs().to(dtype)
    return ref, scale


def dgrad_ref(dy, w, dtype=torch.float64):
    """(ref, scale) of the data gradient, before the mask."""
    wt = dgrad_weights(w)
    return conv_products(dy, wt, dtype), conv_products(dy.abs(), wt.abs(), dtype)


def gemm_ref(P, Q, bias=None, dtype=torch.float64):
    ref, scale = P.to(dtype) @ Q.to(dtype).t(), P.abs().to(dtype) @ Q.abs().to(dtype).t()
    if bias is not None:
        ref, scale = ref + bias.to(dtype), scale + bias.abs().to(dtype)
    return ref, scale


# ------------------------------------------------------------------------------------------- checker
def check(got, ref, scale, *, out="bf16", relu=False, mask=None, y_old=None, tol=None):
    """(worst ratio, index) of |got - ref'| against the bound of the module docstring; no element excluded.  ref / scale: float64, before the
    epilogue; mask (values of a bf16 tensor): elements whose mask is not positive must be zero (y_old with accumulate) exactly; y_old: the
    accumulate form (its magnitude joins the scale); out = "f32": no storage rounding."""
    tol = CONV_TOL if tol is None else tol
    got, ref, scale = got.double(), ref.double(), scale.double()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    keep = None
    if mask is not None:
        keep = mask.double() > 0
        ref, scale = torch.where(keep, ref, torch.zeros_like(ref)), torch.where(keep, scale, torch.zeros_like(scale))
    if relu:
        ref = ref.clamp_min(0)
    if y_old is not None:
        ref = ref + y_old.double()
        scale = torch.where(scale > 0, scale + y_old.double().abs(), scale)      # a zero product added to y_old is y_old itself
    e = tol * scale
    bound = e if out == "f32" else e + 0.5 * ulp_bf16(ref.abs() + e)
    err = (got - ref).abs()
    exact = scale == 0
    ratio = torch.where(exact, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))), err / bound)
    idx = int(ratio.argmax())
    return float(ratio.reshape(-1)[idx]), tuple(int(i) for i in torch.unravel_index(torch.tensor(idx), ratio.shape))


# ------------------------------------------------------------------------------------------- inputs
def gen(shape, seed, scale=1.0):
    """test_gpu_kernels.gen: uniform in (-scale, scale)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


MASK_SPECIALS = (0.0, -0.0, 2.0 ** -126, 2.0 ** -130, -2.0 ** -130, -2.0 ** -126, -2.0 ** -10)


def _normal(shape, g):
    return torch.randn(*shape, generator=g)


def _log_uniform(n, lo, hi, g):
    """2^e with the exponents a shuffled linspace(lo, hi, n): log-uniform, with the full spread at every n."""
    e = torch.linspace(lo, hi, n)[torch.randperm(n, generator=g)] if n > 1 else torch.tensor([float(hi)])
    return torch.exp2(e)


def _mask_values(shape, g):
    m = _normal(shape, g).reshape(-1)
    sp = torch.tensor(MASK_SPECIALS, dtype=torch.float32)
    pos = torch.randperm(m.numel(), generator=g)[:max(m.numel() // 3, len(MASK_SPECIALS))]       # a third of the elements: the specials in turn
    m[pos] = sp[torch.arange(pos.numel()) % len(MASK_SPECIALS)]
    return m.reshape(shape)


def _sparse_log_uniform(shape, g):
    """Half zeros, else log-uniform in magnitude over 2^-20 .. 2^-2 with random sign."""
    mag = torch.exp2(torch.rand(*shape, generator=g) * 18 - 20)
    sign = torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(torch.rand(*shape, generator=g) < 0.5, torch.zeros(shape), mag * sign)


def conv_inputs(shape, regime):
    """x, w (HWIO), bias (fp32), dy, mask (the data gradient's: [Nb, W, H, Ci]), y_old_unit (unit-scale: accumulate's y_old is
    bf(y_old_unit * rms of the gradient reference)): float32 tensors holding bf16 values, but for the bias."""
    Nb, W, H, Ci, Co = shape
    if regime == "uniform":
        return dict(x=bf(gen((Nb, W, H, Ci), 1)), w=bf(gen((3, 3, Ci, Co), 2, 0.05)), bias=gen((Co,), 3), dy=bf(gen((Nb, W, H, Co), 4)),
                    mask=bf(gen((Nb, W, H, Ci), 5)), y_old_unit=gen((Nb, W, H, Ci), 6))
    assert regime == "activations", regime
    g = torch.Generator().manual_seed(1000 + Ci * 7 + Co)
    s_c = _log_uniform(Ci, -6.0, 4.0, g)
    x = bf(torch.relu(_normal((Nb, W, H, Ci), g)) * s_c)
    w = bf(_normal((3, 3, Ci, Co), g) * (2.0 / (9 * Ci)) ** 0.5 * _log_uniform(Co, -2.0, 2.0, g))
    return dict(x=x, w=w, bias=_normal((Co,), g), dy=bf(_sparse_log_uniform((Nb, W, H, Co), g)), mask=bf(_mask_values((Nb, W, H, Ci), g)),
                y_old_unit=_normal((Nb, W, H, Ci), g), s_c=s_c)


def gemm_inputs(shape, regime):
    """P [M, K], Q [N, K], bias [N] (fp32), mask [M, N], base_unit [M, N] (unit scale)."""
    M, N, K = shape
    if regime == "uniform":
        return dict(P=bf(gen((M, K), 1)), Q=bf(gen((N, K), 2)), bias=gen((N,), 3), base_unit=gen((M, N), 4), mask=bf(gen((M, N), 5)))
    g = torch.Generator().manual_seed(2000 + K * 7 + N)
    s_c = _log_uniform(K, -6.0, 4.0, g)
    P = bf(torch.relu(_normal((M, K), g)) * s_c)
    Q = bf(_normal((N, K), g) * (2.0 / K) ** 0.5 * _log_uniform(N, -2.0, 2.0, g).reshape(N, 1))
    return dict(P=P, Q=Q, bias=_normal((N,), g), base_unit=_normal((M, N), g), mask=bf(_mask_values((M, N), g)), s_c=s_c)


def y_old_of(unit, ref):
    """normal (or uniform) at the result's own scale: unit x rms(ref), bf16-rounded."""
    return bf(unit * float(ref.double().pow(2).mean().sqrt()))


def assert_regime(inp, regime, key="x"):
    """The properties that keep `activations` from drifting back to the easy regime, from the generated data; finite values in both."""
    for k, v in inp.items():
        assert bool(torch.isfinite(v).all()), k
    if regime != "activations":
        return
    x = inp[key]
    zeros = float((x == 0).float().mean())
    assert zeros >= 0.40, zeros
    per_channel = x.reshape(-1, x.shape[-1]).abs().amax(0)
    assert float(per_channel.min()) > 0 and float(per_channel.max() / per_channel.min()) >= 2.0 ** 8, per_channel
    m = inp["mask"]
    for v in MASK_SPECIALS:
        assert bool(((m == v) & (torch.signbit(m) == (str(v)[0] == "-"))).any()), v


# ------------------------------------------------------------------------------------------- the host-only query, per knob setting
def choices(setting):
    """[(forward, data gradient, gradient with accumulate, accumulate supported) per case claiming `setting`] from the loaded library."""
    from lstm_ctc_ocr_amd import ops
    out = []
    for (Nb, W, H, Ci, Co), _ in cases_of(setting):
        kw = dict(bias=False, relu=False, mask=True)
        out.append((ops.conv3x3_kernel_choice(Nb, W, H, Ci, Co), ops.conv3x3_kernel_choice(Nb, W, H, Co, Ci, **kw),
                    ops.conv3x3_kernel_choice(Nb, W, H, Co, Ci, accumulate=True, **kw), ops.conv3x3_accum_supported(Nb, W, H, Co, Ci)))
    return out


def child_env(setting):
    """The environment of a child interpreter under `setting`: no OCR_ knob inherited (they are read once per process)."""
    from lstm_ctc_ocr_amd import _native as nat
    e = {k: v for k, v in os.environ.items() if not k.startswith("OCR_")}
    e.update(SETTINGS[setting], OCR_NATIVE_LIB=nat.LIB_PATH)
    return e


def choices_in_child(setting):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), setting], env=child_env(setting), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return [tuple(v) for v in json.loads(out.stdout.splitlines()[-1])]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(choices(sys.argv[1])))
