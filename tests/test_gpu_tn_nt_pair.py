"""The paired launch ocr_gemm_tn_jobs_nt_bf16 (gemm_tn3.hip: the plain weight-gradient tiles and an independent GEMM's workgroups in one
grid) against the two launches it replaces, ocr_gemm_tn_jobs_bf16 and ocr_gemm_nt_bf16: every buffer must hold the SAME bits — no
summation order changes, so the comparison is torch.equal, guard regions included.

Shapes: the smallest that still take every branch.  Contractions of 320 rows (five whole 64-row stages) and of 300 (the last stage's 44
tail rows come from the zero page); one job with two batched problems, one with conv5's overlapping row groups (row_group / row_skip,
lda = I / 2); I, J in {128, 256}; outputs and column sums that
start non-zero (the kernel adds).  The GEMM has M = 1040 rows — just above the large-tile engine's floor, a multiple of neither 128 nor
256, so the last 256-row tile is mostly tail — N = 256, K = 128, and writes into a wider, longer buffer whose other elements must stay.
The reference launch at that shape is the FOUR-wave 128 x 64-tile instance; the paired launch runs the eight-wave 256 x 128 one: equal bits
here also say that the tile shape does not change a GEMM's result.  One case has 8 weight-gradient tiles in front of the GEMM's (the
GEMM's XCD-aware remap keeps its meaning), one has 6 (the remap is rotated against the XCDs: results must not depend on it)."""
import pytest
import torch

from lstm_ctc_ocr_amd import _native as nat
from lstm_ctc_ocr_amd import ops

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 1024            # elements behind every output that no launch may touch
SENTINEL = 7.0


def _guarded(n, dev, dtype, gen):
    """A flat buffer of n random elements with GUARD sentinels behind them."""
    t = torch.empty(n + GUARD, dtype=dtype, device=dev)
    t[:n] = torch.randn(n, device=dev, generator=gen).to(dtype)
    t[n:] = SENTINEL
    return t


def _tn_case(dev, gen, Mk, I, J, nbatch=1, grouped=False):
    """-> (make_job(out, colsum), out0, colsum0): a job's fixed operands and the non-zero state its outputs start from."""
    if grouped:         # conv5's form: logical row m = physical rows m + m // grp and the next one, side by side
        grp, skip, lda = 20, 1, I // 2
        rows = Mk + (Mk + grp - 1) // grp * skip + 1
        A = torch.randn(rows, lda, device=dev, generator=gen).to(BF16)
        sA = 0
    else:
        grp, skip, lda = 0, 0, I
        A = torch.randn(nbatch, Mk, I, device=dev, generator=gen).to(BF16)
        sA = Mk * I
    B = torch.randn(Mk, nbatch * J, device=dev, generator=gen).to(BF16)
    out0 = _guarded(nbatch * I * J, dev, F32, gen)
    cs0 = _guarded(nbatch * J, dev, F32, gen)

    def make(out, cs):
        return ops.tn_job(A, lda, B, nbatch * J, out, J, Mk, I, J, nbatch=nbatch, strideA=sA, strideB=J, strideOut=I * J, colsum=cs,
                          strideColsum=J, row_group=grp, row_skip=skip, scale=0.5)
    return make, out0, cs0, (A, B)


CASES = {
    # name: ((Mk, I, J, nbatch, grouped) x 2) -> tiles in front of the GEMM
    'tiles6_rotated_remap': ((320, 256, 128, 2, False), (320, 128, 256, 1, True)),        # 4 + 2 tiles
    # 4 + 4 tiles; Mk = 300: 44 tail rows of zeros; the longer contraction comes second: the launch puts its tiles in front
    'tiles8_xcd_remap': ((300, 128, 256, 2, False), (320, 256, 256, 1, True)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_paired_launch_equals_the_two_launches(dev, name):
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    specs = CASES[name]
    made = [_tn_case(dev, gen, *s) for s in specs]
    ntiles = sum((s[1] // 128) * (s[2] // 128) * s[3] for s in specs)
    assert ntiles == (8 if 'tiles8' in name else 6)
    M, N, K, ldo, extra_rows = 1040, 256, 128, 256 + 64, 8
    P = torch.randn(M, K, device=dev, generator=gen).to(BF16)
    Q = torch.randn(N, K, device=dev, generator=gen).to(BF16)
    res = {}
    for form in ('two', 'one'):
        outs = [(o.clone(), c.clone()) for _, o, c, _ in made]
        jobs = [mk(o, c) for (mk, _, _, _), (o, c) in zip(made, outs)]
        y = torch.full((M + extra_rows, ldo), SENTINEL, dtype=BF16, device=dev)
        if form == 'two':
            assert ops.gemm_tn_jobs_supported(jobs)
            ops.gemm_tn_jobs(jobs)
            ops.gemm_nt(P, Q, out=y, M=M, N=N, K=K, ldo=ldo)
        else:
            assert ops.gemm_tn_jobs_nt_supported(jobs, M, N, K)
            ops.gemm_tn_jobs_nt(jobs, P, Q, y, M=M, N=N, K=K, ldo=ldo)
        torch.cuda.synchronize()
        res[form] = (outs, y)
    (outs2, y2), (outs1, y1) = res['two'], res['one']
    # the reference itself is sane: it moved every output, and matches a float64 product to bf16 / fp32 accuracy
    ref = P.double() @ Q.double().t()
    assert float((y2[:M, :N].double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max()) + 1e-6
    for (mk, o0, c0, (A, B)), (o2, c2), s in zip(made, outs2, specs):
        Mk, I, J, nb, grouped = s
        assert not torch.equal(o2[:-GUARD], o0[:-GUARD]) and not torch.equal(c2[:-GUARD], c0[:-GUARD])
        if not grouped:
            prod = torch.stack([A[b].double().t() @ B[:, b * J:(b + 1) * J].double() for b in range(nb)])
            mass = torch.stack([A[b].double().abs().t() @ B[:, b * J:(b + 1) * J].double().abs() for b in range(nb)])
            start = o0[:nb * I * J].double().view(nb, I, J)
            got = o2[:nb * I * J].double().view(nb, I, J)
            # fp32 accumulation of Mk exact products, one scaling and one add: (Mk + 2) roundings of 2^-24 on the mass of the terms
            assert float((got - (start + 0.5 * prod)).abs().max()) <= (Mk + 2) * 2.0 ** -24 * float((start.abs() + 0.5 * mass).max())
    # the paired launch: the same bits everywhere, guards included, and the guards still hold the sentinel
    assert torch.equal(y1, y2)
    assert bool((y1[M:] == SENTINEL).all()) and bool((y1[:, N:] == SENTINEL).all())
    for (o1, c1), (o2, c2) in zip(outs1, outs2):
        assert torch.equal(o1, o2) and torch.equal(c1, c2)
        assert bool((o1[-GUARD:] == SENTINEL).all()) and bool((c1[-GUARD:] == SENTINEL).all())


def test_paired_launch_with_f32_output_and_row_groups(dev):
    """The GEMM's other plain-mode forms the paired launch passes through: an fp32 output and P rows in groups with a skipped row behind each
    (conv5's forward form), at the same tail-heavy M."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    made = [_tn_case(dev, gen, 320, 128, 128, 1, False), _tn_case(dev, gen, 320, 128, 128, 1, True)]
    M, N, K, grp = 1040, 256, 128, 26
    P = torch.randn(M + M // grp + 1, K, device=dev, generator=gen).to(BF16)
    Q = torch.randn(N, K, device=dev, generator=gen).to(BF16)
    res = {}
    for form in ('two', 'one'):
        outs = [(o.clone(), c.clone()) for _, o, c, _ in made]
        jobs = [mk(o, c) for (mk, _, _, _), (o, c) in zip(made, outs)]
        y = torch.full((M + 8, N), SENTINEL, dtype=F32, device=dev)
        if form == 'two':
            ops.gemm_tn_jobs(jobs)
            ops.gemm_nt(P, Q, out=y, M=M, N=N, K=K, row_group=grp, row_skip=1)
        else:
            assert ops.gemm_tn_jobs_nt_supported(jobs, M, N, K, flags=nat.EPI_OUT_F32)
            ops.gemm_tn_jobs_nt(jobs, P, Q, y, M=M, N=N, K=K, row_group=grp, row_skip=1)
        torch.cuda.synchronize()
        res[form] = (outs, y)
    (outs2, y2), (outs1, y1) = res['two'], res['one']
    rows = torch.arange(M, device=dev)
    ref = P[rows + rows // grp].double() @ Q.double().t()
    mass = P[rows + rows // grp].double().abs() @ Q.double().abs().t()
    assert float((y2[:M].double() - ref).abs().max()) <= K * 2.0 ** -24 * float(mass.max())         # K roundings of the fp32 accumulator
    assert torch.equal(y1, y2) and bool((y1[M:] == SENTINEL).all())
    for (o1, c1), (o2, c2) in zip(outs1, outs2):
        assert torch.equal(o1, o2) and torch.equal(c1, c2)
