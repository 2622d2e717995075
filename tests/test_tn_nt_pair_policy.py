"""When may the plain weight-gradient launch take a GEMM's workgroups onto its idle CUs — the host-only query ocr_gemm_tn_jobs_nt_supported
(the policy the paired launch itself asks: gemm_tn3.hip tn3_nt_pair_ok), pinned without a GPU.  With no device visible the library counts
the MI355X's 256 CUs, so "a quarter of the CUs free" is at most 192 tiles here.  The descriptors hold made-up, 16-byte aligned addresses:
the query looks at shapes, strides and alignment and touches no memory."""
import ctypes
import os

import pytest

from lstm_ctc_ocr_amd import _native as nat
from lstm_ctc_ocr_amd import ops

pytestmark = pytest.mark.skipif(not os.path.exists(nat.LIB_PATH), reason="libocrhip.so not built")

INVALID = 2         # OCR_ERR_INVALID


def _job(Mk, I, J, nbatch=1, lda=None, row_group=0, row_skip=0, A=0x100000):
    lda = I if lda is None else lda
    return ops.TnJob(A, lda, Mk * lda, 0x200000, nbatch * J, J, 0x300000, J, I * J, 0x400000, J, Mk, I, J, nbatch, row_group, row_skip, 1.0, 0)


def _tiles(j):
    return (j.I // 128) * (j.J // 128) * j.nbatch


def _plan(N, W, U=256, D=512, HC=1024, co=512):
    """The two products and the GEMM of a plan's head at batch N, width W: the BiLSTM cells' [x | h]^T dz (both directions), conv5's x^T dz over
    overlapping rows, and conv5's data gradient dz W -> column matrix."""
    Wo = W // 4 - 1
    M = N * Wo
    lstm = _job(M, D + U, 4 * U, nbatch=2)
    conv5 = _job(M, 2 * HC, co, lda=HC, row_group=Wo, row_skip=1)
    return [lstm, conv5], (M, 2 * HC, co)


def test_headline_shape_is_accepted():
    jobs, (M, N, K) = _plan(64, 256)
    assert [_tiles(j) for j in jobs] == [96, 64] and (M, N, K) == (4032, 2048, 512)
    assert ops.gemm_tn_jobs_supported(jobs)
    assert ops.gemm_tn_jobs_nt_supported(jobs, M, N, K)
    assert ops.gemm_tn_jobs_nt_supported(jobs[::-1], M, N, K)
    # ... at every width of the variable-width workload whose GEMM has the engine's 1024 rows, and at the smallest batch the engine test uses
    for W in (80, 100, 128, 200, 320):
        jobs, (M, N, K) = _plan(64, W)
        assert ops.gemm_tn_jobs_nt_supported(jobs, M, N, K), W
    jobs, (M, N, K) = _plan(34, 128)
    assert M == 1054 and ops.gemm_tn_jobs_nt_supported(jobs, M, N, K)


def test_deep_plan_is_declined():
    """configs[4]: BiLSTM cells of 512 units per direction at batch 32 — the first layer's product alone has 8 x 16 x 2 = 256 tiles, one per
    CU: no CU stays free, whatever it is paired with."""
    Wo = 63
    M = 32 * Wo
    lstm1 = _job(M, 512 + 512, 4 * 512, nbatch=2)
    lstm2 = _job(M, 1024 + 512, 4 * 512, nbatch=2)
    conv5 = _job(M, 2048, 512, lda=1024, row_group=Wo, row_skip=1)
    assert _tiles(lstm1) == 256 and _tiles(lstm2) == 384
    for pair in ([lstm2, lstm1], [lstm1, conv5], [conv5, lstm1]):
        assert ops.gemm_tn_jobs_supported(pair)
        assert not ops.gemm_tn_jobs_nt_supported(pair, M, 2048, 512)


def test_the_bound_is_a_quarter_of_the_cus():
    M, N, K = 4032, 2048, 512
    a = _job(4032, 1024, 1024)                       # 64 tiles
    assert ops.gemm_tn_jobs_nt_supported([a, _job(4032, 1024, 2048)], M, N, K)            # 64 + 128 = 192: 64 CUs free
    assert not ops.gemm_tn_jobs_nt_supported([a, _job(4032, 1152, 1920)], M, N, K)        # 64 + 135 = 199: 57 free
    assert not ops.gemm_tn_jobs_nt_supported([a, _job(4032, 1024, 3072)], M, N, K)        # 64 + 192 = 256: none


def test_declined_for_a_job_or_a_gemm_that_is_not_covered():
    jobs, (M, N, K) = _plan(64, 256)
    assert not ops.gemm_tn_jobs_nt_supported(jobs[:1], M, N, K)                            # one job: nothing to pair it with
    assert not ops.gemm_tn_jobs_nt_supported([jobs[0], _job(4032, 2048, 448, lda=1024)], M, N, K)      # J % 128
    assert not ops.gemm_tn_jobs_nt_supported([jobs[0], _job(128, 2048, 512, lda=1024)], M, N, K)       # contraction below 256 rows
    assert not ops.gemm_tn_jobs_nt_supported([jobs[0], _job(4032, 2048, 512, lda=1024, A=0x100008)], M, N, K)      # A not 16-byte aligned
    assert not ops.gemm_tn_jobs_nt_supported(jobs, 1023, N, K)                             # the large-tile engine's floor: 1024 rows
    assert ops.gemm_tn_jobs_nt_supported(jobs, 1024, N, K)
    assert not ops.gemm_tn_jobs_nt_supported(jobs, M, N, K + 32)                           # K % 64
    assert not ops.gemm_tn_jobs_nt_supported(jobs, M, 64, K)                               # narrower than the 128-column tile
    assert not ops.gemm_tn_jobs_nt_supported(jobs, M, N + 2, K)                            # N % 4
    assert not ops.gemm_tn_jobs_nt_supported(jobs, M, N, K, flags=nat.EPI_ACCUM)           # accumulate: not the large-tile engine's
    assert ops.gemm_tn_jobs_nt_supported(jobs, M, N, K, flags=nat.EPI_OUT_F32)


def test_the_launch_refuses_what_the_query_refuses():
    """Status OCR_ERR_INVALID before anything touches the device: a refused pair launches nothing."""
    jobs, (M, N, K) = _plan(64, 256)
    arr = (ops.TnJob * 2)(*jobs)
    lib = nat.lib()
    args = (0x500000, K, 0x600000, K, 0x700000, N)
    assert lib.ocr_gemm_tn_jobs_nt_bf16(ctypes.cast(arr, ctypes.c_void_p), 1, *args, M, N, K, None, None, 0, 0, 0, 0, 0, 0, None) == INVALID
    assert lib.ocr_gemm_tn_jobs_nt_bf16(ctypes.cast(arr, ctypes.c_void_p), 2, *args, 1000, N, K, None, None, 0, 0, 0, 0, 0, 0, None) == INVALID
    assert lib.ocr_gemm_tn_jobs_nt_bf16(ctypes.cast(arr, ctypes.c_void_p), 2, None, K, 0x600000, K, 0x700000, N, M, N, K, None, None, 0, 0, 0, 0,
                                        0, 0, None) == INVALID
    assert lib.ocr_gemm_tn_jobs_nt_bf16(ctypes.cast(arr, ctypes.c_void_p), 2, *args, M, N, K, None, None, 0, nat.EPI_BIAS, 0, 0, 0, 0,
                                        None) == INVALID                                  # bias flag without a bias
    assert lib.ocr_gemm_tn_jobs_nt_supported(None, 2, M, N, K, 0) == 0
