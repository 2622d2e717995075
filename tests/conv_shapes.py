"""The shape list of the 3x3 convolution parity tests, shared by test_gpu_kernels.py (default build and the OCR_CONV_* generations),
test_gpu_kernel_generations.py (the engine generations and the weight-gradient knobs) and test_wgrad_dispatch_policy.py (which checks on the
host that the list reaches every weight-gradient kernel instance it claims to reach) — and the float64 weight-gradient reference.

WGRAD_CLAIMS: where a comment names the weight-gradient kernel a shape is there for, the claim as data: the host test compares it with
ops.conv3x3_wgrad_kernel_choice under the default knobs (workspace given)."""
import torch
import torch.nn.functional as F

CONV_SHAPES = [   # (Nb, W, H, Cin, Cout)
    (4, 16, 8, 64, 128), (2, 12, 4, 256, 512), (64, 64, 4, 256, 512), (3, 20, 16, 64, 128),
    (16, 32, 16, 64, 128), (64, 128, 8, 64, 256), (5, 52, 4, 128, 192), (32, 64, 4, 512, 512),
    (7, 22, 8, 128, 256), (32, 64, 2, 512, 512), (3, 18, 2, 64, 128), (9, 64, 2, 128, 64),
    (17, 62, 4, 128, 128), (9, 30, 16, 64, 256),       # ragged last tiles of the 256- / 128-pixel kernels
    (4, 128, 8, 128, 128), (6, 192, 4, 192, 64),       # plane-layout kernels (conv_k3; wgrad9p on whole-image steps): several tiles per image, 3 chunks
    (8, 48, 16, 128, 64), (16, 32, 16, 128, 128), (8, 64, 16, 64, 64),    # ... at H = 16 (one / two halo buffers)
    (32, 40, 4, 128, 128), (32, 24, 8, 64, 128), (16, 50, 8, 128, 64),    # ... tiles crossing image boundaries (general width)
    # weight-stationary persistent kernel (conv_ws, round 5): small grids (fewer tiles than workgroups, three channel
    # tiles = no XCD map, several images per workgroup run); taken by default only from two tiles per CU, forced with OCR_CONV_WS=2
    (2, 32, 16, 64, 128), (3, 24, 16, 128, 192), (5, 48, 8, 128, 64), (40, 64, 16, 64, 64),
    # the EXACT shapes of the benchmarked step (BASELINE configs[1], N = 64, W = 256): conv2, conv3_1, conv3_2, conv4_2
    # (conv4_1 is (64, 64, 4, 256, 512) above) — the dispatcher's full-chip tiles / 64-split slabs only exist at this size
    (64, 128, 16, 64, 128), (64, 64, 8, 128, 256), (64, 64, 8, 256, 256), (64, 64, 4, 512, 512),
    # ... and the extremes of configs[3] (W = 80 and W = 320 padded batches)
    (64, 40, 16, 64, 128), (64, 20, 4, 512, 512), (64, 80, 8, 256, 256), (64, 80, 4, 256, 512),
    # ... and widths that are no multiple of the weight-gradient kernel's step (round 6: wgrad9p's zero-row instances — every
    # step of (32, 33, 4) / (16, 17, 8) crosses an image boundary at another column; W = 79 = a 316-pixel configs[3] batch)
    (32, 33, 4, 64, 64), (16, 17, 8, 64, 64), (64, 79, 4, 256, 512), (64, 79, 8, 256, 256), (32, 47, 4, 128, 64)]

HEADLINE_WGRAD = [   # the five 3x3 layers of the headline step (N = 64, W = 256): (layer, shape)
    ("conv2", (64, 128, 16, 64, 128)), ("conv3_1", (64, 64, 8, 128, 256)), ("conv3_2", (64, 64, 8, 256, 256)),
    ("conv4_1", (64, 64, 4, 256, 512)), ("conv4_2", (64, 64, 4, 512, 512))]

WGRAD_CLAIMS = {   # shape -> (kernel, S) under the default knobs with a workspace (S = None: not claimed)
    (4, 128, 8, 128, 128): ("wgrad9p<8>", None), (6, 192, 4, 192, 64): ("wgrad9p<4>", None),                  # "plane-layout kernel"
    (32, 40, 4, 128, 128): ("wgrad9p<4>/zero-row", None), (32, 24, 8, 64, 128): ("wgrad9p<8>/zero-row", None),       # "general width"
    (16, 50, 8, 128, 64): ("wgrad9p<8>/zero-row", None),
    (64, 128, 16, 64, 128): ("wgrad9", 64),                                                                   # "64-split slabs only exist at this size"
    (32, 33, 4, 64, 64): ("wgrad9p<4>/zero-row", None), (16, 17, 8, 64, 64): ("wgrad9p<8>/zero-row", None),   # "wgrad9p's zero-row instances"
    (64, 79, 4, 256, 512): ("wgrad9p<4>/zero-row", None), (64, 79, 8, 256, 256): ("wgrad9p<8>/zero-row", None),
    (32, 47, 4, 128, 64): ("wgrad9p<4>/zero-row", None)}


def wgrad_products(x, dy, dtype=torch.float64):
    """The 3x3 weight gradient as its definition, dw[a][b] = shift_ab(x)^T dy: nine matmuls on the zero-padded input (x [Nb, W, H, Cin],
    dy [Nb, W, H, Cout], tap a along W, tap b along H: y[n, w, h] = sum_ab x[n, w + a - 1, h + b - 1] w[a][b]).  Returns [3, 3, Cin, Cout]."""
    Nb, W, H, Ci = x.shape
    Co = dy.shape[-1]
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))
    d2 = dy.to(dtype).reshape(-1, Co)
    dw = torch.empty((3, 3, Ci, Co), dtype=dtype)
    for a in range(3):
        for b in range(3):
            dw[a, b] = xp[:, a:a + W, b:b + H, :].reshape(-1, Ci).t() @ d2
    return dw


def wgrad_ref64(x, dy):
    """(dw, scale, dbias, bias_scale) in float64: the weight gradient, each element's own scale (|x|-shifted^T |dy|)_ij — the sum of the
    magnitudes of the terms that element adds up, the unit a summation-order error is measured in — the bias gradient and its scale."""
    d2 = dy.double().reshape(-1, dy.shape[-1])
    return wgrad_products(x, dy), wgrad_products(x.abs(), dy.abs()), d2.sum(0), d2.abs().sum(0)


def element_ratio(got, ref, scale):
    """max over elements of |got - ref| / scale (float64); elements whose scale is 0 must be exact."""
    err = (got.double() - ref).abs()
    assert bool((err[scale == 0] == 0).all())
    return float((err / scale.clamp_min(1e-300)).max())


def wgrad_choices():
    """{mode: [(kernel, S) per shape of CONV_SHAPES]} from the loaded library, for the three ways the parity tests call the weight gradient."""
    from lstm_ctc_ocr_amd import ops
    c = ops.conv3x3_wgrad_kernel_choice
    return {"workspace": [c(*s) for s in CONV_SHAPES], "atomics": [c(*s, workspace=False) for s in CONV_SHAPES],
            "splits2": [c(*s, workspace=False, splits=2) for s in CONV_SHAPES]}


def wgrad_choices_in_child(env):
    """wgrad_choices() of a fresh interpreter under the knobs `env` (no other OCR_ knob inherited: they are read once per process)."""
    import json
    import os
    import subprocess
    import sys
    from lstm_ctc_ocr_amd import _native as nat
    e = {k: v for k, v in os.environ.items() if not k.startswith("OCR_")}
    e.update(env, OCR_NATIVE_LIB=nat.LIB_PATH)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return {k: [tuple(v) for v in vs] for k, vs in json.loads(out.stdout.splitlines()[-1]).items()}


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(wgrad_choices()))
