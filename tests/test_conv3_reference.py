"""tests/conv3_reference.py pinned without a GPU: the checker (accepts the float32 nine-matmul result rounded to nearest even, rejects the
plausible epilogue bugs), CONV_TOL against its own measurement, the regimes' properties, and the case list's claims against the host-only
dispatch query under every knob setting."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv3_reference as c3  # noqa: E402

from lstm_ctc_ocr_amd import _native as nat  # noqa: E402

needs_lib = pytest.mark.skipif(not os.path.exists(nat.LIB_PATH), reason="libocrhip.so not built")
F32 = torch.float32

PIN_SHAPES = [(16, 64, 4, 64, 64), (16, 64, 4, 192, 192),      # one chunk; three 64-channel chunks
              (4, 64, 4, 64, 100), (3, 12, 30, 64, 64)]        # ragged channel tile; H = 30


def _ratio(got, ref, scale, **kw):
    return c3.check(got, ref, scale, **kw)[0]


@pytest.mark.parametrize("regime", c3.REGIMES)
@pytest.mark.parametrize("shape", PIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_accepts_fp32_round_to_nearest_and_rejects_the_mutations(shape, regime):
    """Forward with bias and ReLU.  Accepted: bf16_rne(relu(fp32 products + bias)).  Rejected: the output truncated to bf16; the second half of
    the K range (taps 5 .. 8, a K split by taps) handed over as bf16; the bias added after the bf16 rounding; the heaviest input channel of
    the centre tap dropped at the border column w = 0.  Measured ratios here (bound: 1): fp32 round-to-nearest 0.990 .. 0.996, truncation 1.98 ..
    1.99, the bf16 exchange 36 .. 136, the double rounding 31 .. 148, the dropped channel 806 .. 31726."""
    i = c3.conv_inputs(shape, regime)
    x, w, bias = i["x"], i["w"], i["bias"]
    ref, scale = c3.fwd_ref(x, w, bias)
    y32 = c3.conv_products(x, w, F32)
    kw = dict(relu=True)
    good = _ratio(c3.bf(torch.relu(y32 + bias)), ref, scale, **kw)
    trunc = _ratio(c3.bf_truncate(torch.relu(y32 + bias)), ref, scale, **kw)
    w_lo, w_hi = w.clone(), w.clone()
    w_lo.reshape(9, -1)[5:] = 0
    w_hi.reshape(9, -1)[:5] = 0
    ksplit = _ratio(c3.bf(torch.relu(c3.conv_products(x, w_lo, F32) + c3.bf(c3.conv_products(x, w_hi, F32)) + bias)), ref, scale, **kw)
    twice = _ratio(c3.bf(torch.relu(c3.bf(y32) + bias)), ref, scale, **kw)
    c0 = int(x.reshape(-1, x.shape[-1]).abs().sum(0).argmax())
    dropped = y32.clone()
    dropped[:, 0] -= x[:, 0, :, c0, None] * w[1, 1, c0]
    drop = _ratio(c3.bf(torch.relu(dropped + bias)), ref, scale, **kw)
    print("%s %s: fp32 rne %.3f | truncated %.2f, bf16 K-split exchange %.1f, bias after rounding %.1f, dropped channel %.1f" % (
        shape, regime, good, trunc, ksplit, twice, drop))
    assert good <= 1.0, good
    assert trunc > 1.0 and ksplit > 1.0 and twice > 1.0 and drop > 1.0, (trunc, ksplit, twice, drop)


@pytest.mark.parametrize("regime", c3.REGIMES)
@pytest.mark.parametrize("shape", PIN_SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_checker_on_the_masked_gradient_and_the_accumulate_form(shape, regime):
    """Data gradient with the mask, alone and accumulated onto y_old.  Accepted: the fp32 products, masked by `mask > 0` as a bf16 number,
    (+ y_old,) rounded once.  Rejected: truncation; the two-pass accumulate bf16(y_old + bf16(result)); a masked element that loses its y_old; and,
    where the mask holds such values (activations), `mask >= 0` and a positive subnormal mask value flushed to zero."""
    i = c3.conv_inputs(shape, regime)
    dy, w, mask = i["dy"], i["w"], i["mask"]
    ref, scale = c3.dgrad_ref(dy, w)
    g32 = c3.conv_products(dy, c3.dgrad_weights(w), F32)
    keep = mask > 0
    y_old = c3.y_old_of(i["y_old_unit"], ref)
    zero = torch.zeros(())
    assert _ratio(c3.bf(torch.where(keep, g32, zero)), ref, scale, mask=mask) <= 1.0
    assert _ratio(c3.bf_truncate(torch.where(keep, g32, zero)), ref, scale, mask=mask) > 1.0
    assert _ratio(c3.bf(y_old + torch.where(keep, g32, zero)), ref, scale, mask=mask, y_old=y_old) <= 1.0
    assert _ratio(c3.bf(y_old + c3.bf(torch.where(keep, g32, zero))), ref, scale, mask=mask, y_old=y_old) > 1.0
    assert _ratio(c3.bf(torch.where(keep, y_old + g32, zero)), ref, scale, mask=mask, y_old=y_old) == float("inf")      # masked: y_old must stay
    if regime == "activations":
        assert _ratio(c3.bf(torch.where(mask >= 0, g32, zero)), ref, scale, mask=mask) == float("inf")
        assert _ratio(c3.bf(torch.where(mask >= 2.0 ** -126, g32, zero)), ref, scale, mask=mask) > 1.0


def test_checker_requires_exact_zeros_and_reports_the_index():
    ref = torch.tensor([[1.0, 0.0], [3.0, -2.0]], dtype=torch.float64)
    scale = torch.tensor([[2.0, 0.0], [3.0, 2.0]], dtype=torch.float64)
    assert c3.check(ref.float(), ref, scale) == (0.0, (0, 0))
    got = ref.float().clone()
    got[0, 1] = 2.0 ** -133
    assert c3.check(got, ref, scale) == (float("inf"), (0, 1))
    got = ref.float().clone()
    got[1, 0] = 3.0 + 2.0 ** -6                     # one bf16 ulp at 3: twice the half ulp
    r, idx = c3.check(got, ref, scale)
    assert idx == (1, 0) and 1.9 < r <= 2.0
    r, idx = c3.check(got, ref, scale, out="f32")
    assert idx == (1, 0) and r > 1000
    # a result rounded across a power of two: ref just under 2, stored as 2 (ulp there twice the ulp below)
    ref2 = torch.tensor([2.0 - 2.0 ** -8 + 1e-9], dtype=torch.float64)
    assert c3.check(torch.tensor([2.0]), ref2, torch.tensor([4.0], dtype=torch.float64))[0] <= 1.0
    assert float(c3.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 2.0 ** -126, 2.0 ** -130, 0.0], dtype=torch.float64)).sub(
        torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133], dtype=torch.float64)).abs().max()) == 0.0


@pytest.fixture(scope="module")
def reference_side():
    """Every case and regime once: the regime properties asserted, and the float32 nine-matmul result against the float64 one in units of the
    scale.  {kind: [(error, shape, regime)]}"""
    res = {"forward": [], "gradient": [], "gemm_nt": []}
    for shape, _, _ in c3.CASES:
        for regime in c3.REGIMES:
            i = c3.conv_inputs(shape, regime)
            c3.assert_regime(i, regime)
            ref, scale = c3.fwd_ref(i["x"], i["w"], i["bias"])
            assert float(scale.min()) > 0
            y32 = c3.conv_products(i["x"], i["w"], F32) + i["bias"]
            res["forward"].append((float(((y32.double() - ref).abs() / scale).max()), shape, regime))
            ref, scale = c3.dgrad_ref(i["dy"], i["w"])
            g32 = c3.conv_products(i["dy"], c3.dgrad_weights(i["w"]), F32)
            assert bool((g32[scale == 0] == 0).all())
            res["gradient"].append((float(((g32.double() - ref).abs() / scale.clamp_min(1e-300)).max()), shape, regime))
    for shape in c3.GEMM_CASES:
        for regime in c3.REGIMES:
            i = c3.gemm_inputs(shape, regime)
            c3.assert_regime(i, regime, "P")
            ref, scale = c3.gemm_ref(i["P"], i["Q"], i["bias"])
            res["gemm_nt"].append((float((((i["P"] @ i["Q"].t() + i["bias"]).double() - ref).abs() / scale).max()), shape, regime))
    return res


def test_conv_tol_is_the_reference_side_error_times_eight(reference_side):
    """CONV_TOL = 8 x the worst float32-against-float64 error over every case and regime of conv3_reference.py (its docstring carries the
    ranges).  The constant was measured with one CPU's blocked fp32 products (the same at 1, 3 and 8 threads); another BLAS may block
    differently, so the assertion is that the constant is the measurement within a factor of two: never below it by more than that (a bar
    tighter than the reference's own error), never above it by more (a stale, loose bar)."""
    for kind, rows in reference_side.items():
        print("%-9s %.3g %s %s .. %.3g %s %s" % ((kind,) + min(rows) + max(rows)))
    worst = max(max(rows)[0] for rows in reference_side.values())
    print("8 x worst = %.4g, CONV_TOL = %.4g" % (8 * worst, c3.CONV_TOL))
    assert 0.5 * c3.CONV_TOL <= 8 * worst <= 2.0 * c3.CONV_TOL, (worst, c3.CONV_TOL)


def test_regimes_differ_as_described(reference_side):
    """(the properties themselves are asserted per case by the fixture) the activations regime is the harder one for the reference too."""
    for rows in reference_side.values():
        assert max(r for r in rows if r[2] == "activations")[0] > max(r for r in rows if r[2] == "uniform")[0]
    i = c3.conv_inputs((4, 64, 4, 64, 100), "activations")
    assert float(i["s_c"].max() / i["s_c"].min()) == 2.0 ** 10
    nz = i["dy"][i["dy"] != 0].abs()
    assert 0.45 < float((i["dy"] == 0).float().mean()) < 0.55 and float(nz.min()) >= 2.0 ** -20 and float(nz.max()) <= 2.0 ** -2
    assert float(nz.max() / nz.min()) > 2.0 ** 16


# ------------------------------------------------------------------------------------------- claims
@pytest.fixture(scope="module")
def answers():
    """{setting: the query's answers for the cases claiming it}, each setting in a child interpreter that inherits no OCR_ variable."""
    return {s: c3.choices_in_child(s) for s in c3.SETTINGS}


@needs_lib
@pytest.mark.parametrize("setting", list(c3.SETTINGS))
def test_every_claimed_choice_is_the_dispatchers(answers, setting):
    for ((shape, (fwd, grad)), (got_f, got_g, _, _)) in zip(c3.cases_of(setting), answers[setting]):
        assert got_f == fwd, (setting, shape, "forward", got_f, fwd)
        # a refused gradient (None: Cout % 32 != 0) is answered "gemm" by the query; the call refuses (test_gpu_conv3_fp64.py asserts that)
        assert got_g == (grad or "gemm"), (setting, shape, "data gradient", got_g, grad)
        assert (grad is None) == (shape[4] % 32 != 0), shape


@needs_lib
def test_the_claims_cover_every_family(answers):
    fwd = {f for s in c3.SETTINGS for _, (f, _) in c3.cases_of(s)}
    grad = {g for s in c3.SETTINGS for _, (_, g) in c3.cases_of(s) if g}
    assert fwd == set(c3.FAMILIES), set(c3.FAMILIES) - fwd
    assert grad == set(c3.FAMILIES) - set(c3.GRAD_UNREACHABLE), set(c3.FAMILIES) - grad
    # accumulate (onto the masked data gradient): every non-gemm family but conv_ws, which takes no accumulate flag
    accum = {a for s in c3.SETTINGS for (_, _, a, ok) in answers[s] if ok}
    assert accum == set(c3.FAMILIES) - {"gemm"} - set(c3.ACCUM_UNREACHABLE), accum
    assert all((a != "gemm") == ok for s in c3.SETTINGS for (_, _, a, ok) in answers[s])
