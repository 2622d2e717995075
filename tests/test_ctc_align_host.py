"""The host-only side of CTC forced alignment (ctc_align.hip): ocr_ctc_align_supported, ocr_ctc_align_workspace_size, the refusals of ocr_ctc_align
before any launch, the header and the ctypes signatures, ops.ctc_align's argument checks, and the Engine methods' signatures.  No GPU."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_cases as ac  # noqa: E402


def test_header_declares_the_entry_points():
    from lstm_ctc_ocr_amd import _native as nat
    declared = nat.declared_symbols()
    for name in ('ocr_ctc_align_supported', 'ocr_ctc_align_workspace_size', 'ocr_ctc_align'):
        assert name in declared and name in nat._SIGS and hasattr(nat.lib(), name), name
    assert len(nat._SIGS['ocr_ctc_align'][0]) == 18 and len(nat._SIGS['ocr_ctc_align_workspace_size'][0]) == 6
    assert len(nat._SIGS['ocr_ctc_align_supported'][0]) == 4


def test_supported_ranges():
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    lib = nat.lib()
    grid = [(C, T, L, K) for C in (0, 1, 40, 16384, 16385) for T in (0, 1, 63, 1 << 20) for L in (-1, 0, 255, 256) for K in (0, 1, 65536, 65537)]
    for C, T, L, K in grid:
        assert bool(lib.ocr_ctc_align_supported(C, T, L, K)) == ac.supported(C, T, L, K), (C, T, L, K)
    for k in ac.cases():
        assert ops.ctc_align_supported(k.C, k.T, k.mll, k.K), k.name
    assert ops.ctc_align_supported(24, 520, 255, 3) and ops.ctc_align_supported(6625, 1024, 31, 1) and ops.ctc_align_supported(40, 63, 31, 5)
    assert not ops.ctc_align_supported(16385, 63, 31, 1) and not ops.ctc_align_supported(40, 63, 256, 1) and not ops.ctc_align_supported(40, 0, 31, 1)
    assert not ops.ctc_align_supported(40, 63, 31, 0) and not ops.ctc_align_supported(40, 63, 31, 65537)


def test_workspace_size():
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    lib = nat.lib()
    sz = ctypes.c_size_t(0)
    for k in ac.cases():
        assert lib.ocr_ctc_align_workspace_size(k.C, k.T, k.N, k.K, k.mll, ctypes.byref(sz)) == 0, k.name
        assert sz.value == ac.workspace_bytes(k.C, k.T, k.N, k.K, k.mll) and sz.value % 256 == 0 and sz.value >= 4 * k.T * k.N, k.name
        assert sz.value >= ops.ctc_score_workspace_bytes(k.C, k.T, k.N), k.name          # the lse table comes first, as ocr_ctc_score lays it out
    # the product shape keeps its back-pointers in LDS: the lse table is all there is
    assert ops.ctc_align_workspace_bytes(6625, 63, 64, 1, 31) == ops.ctc_score_workspace_bytes(6625, 63, 64) == 16128
    assert ops.ctc_align_workspace_bytes(40, 64, 64, 5, 31) == 64 * 64 * 4
    assert ops.ctc_align_workspace_bytes(40, 65, 2, 5, 31) == (2 * 65 * 4 + 255) // 256 * 256 + 2 * 5 * 65 * 128
    assert ops.ctc_align_workspace_bytes(6625, 1024, 64, 1, 31) == 64 * 1024 * 4 + 64 * 1024 * 128
    for C, T, N, K, L in [(16385, 63, 4, 1, 8), (0, 63, 4, 1, 8), (40, 0, 4, 1, 8), (40, 63, 0, 1, 8), (40, 63, -1, 1, 8), (40, 63, 65536, 1, 8),
                          (40, 63, 4, 0, 8), (40, 63, 4, 65537, 8), (40, 63, 4, 1, -1), (40, 63, 4, 1, 256), (40, 1 << 20, 2047, 65536, 8),
                          (40, 1 << 17, 65535, 65536, 8)]:
        assert ac.workspace_bytes(C, T, N, K, L) is None and lib.ocr_ctc_align_workspace_size(C, T, N, K, L, ctypes.byref(sz)) == 2, (C, T, N, K, L)
    assert lib.ocr_ctc_align_workspace_size(40, 63, 4, 1, 8, None) == 2
    with pytest.raises(nat.NativeError):
        ops.ctc_align_workspace_bytes(40, 63, 4, 1, 256)


def test_refusals_come_before_any_launch():
    """OCR_ERR_INVALID (2) for a NULL operand, a blank outside [0, C), a sample stride other than 0 or K, a short workspace and every shape the
    support function refuses: host memory stands in for the operands, nothing reads it."""
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    assert lib.ocr_ctc_align(None, None, None, None, 0, 40, 4, 63, 1, 8, 0, None, None, None, None, None, 0, None) == 2
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(acts=p, il=p, labels=p, lens=p, stride=16, C=40, N=4, T=63, K=16, L=8, blank=0, start=p, end=p, score=p, cost=p, ws=p, ws_bytes=1024)

    def status(**kw):
        v = dict(good, **kw)
        return lib.ocr_ctc_align(v['acts'], v['il'], v['labels'], v['lens'], v['stride'], v['C'], v['N'], v['T'], v['K'], v['L'], v['blank'],
                                 v['start'], v['end'], v['score'], v['cost'], v['ws'], v['ws_bytes'], None)
    assert ac.workspace_bytes(40, 63, 4, 16, 8) == 1024
    for operand in ('acts', 'il', 'labels', 'lens', 'start', 'end', 'score', 'cost', 'ws'):
        assert status(**{operand: None}) == 2, operand
    assert status(blank=-1) == 2 and status(blank=40) == 2
    assert status(stride=1) == 2 and status(stride=15) == 2 and status(stride=-16) == 2
    assert status(ws_bytes=1023) == 2
    assert status(T=65, ws_bytes=ac.workspace_bytes(40, 65, 4, 16, 8) - 1) == 2          # past 64 frames the back-pointer words count
    assert status(K=0) == 2 and status(K=65537) == 2 and status(L=-1) == 2 and status(L=256) == 2 and status(C=16385) == 2 and status(C=0) == 2
    assert status(T=0) == 2 and status(N=0) == 2 and status(N=65536, ws_bytes=1 << 30) == 2


def test_ops_checks_its_arguments():
    from lstm_ctc_ocr_amd import _native as nat
    from lstm_ctc_ocr_amd import ops
    acts = torch.zeros(5, 2, 6)
    il = torch.full((2,), 5, dtype=torch.int32)
    lab = torch.ones(2, 3, dtype=torch.int32)
    with pytest.raises(nat.NativeError):
        ops.ctc_align(acts, il, lab, torch.full((2,), 3, dtype=torch.int32))          # CPU tensors: no fallback
    cases = [
        (torch.ones(3, 3, dtype=torch.int32), torch.ones(3, dtype=torch.int32), False),            # [N', L] with N' != N
        (torch.ones(2, 3, dtype=torch.int32), torch.ones(2, 1, dtype=torch.int32), False),         # lengths of the wrong rank
        (torch.ones(2, 4, 3, dtype=torch.int32), torch.ones(2, 3, dtype=torch.int32), False),      # [N, K, L] against [N, K']
        (torch.ones(3, 4, 3, dtype=torch.int32), torch.ones(3, 4, dtype=torch.int32), False),      # N' != N
        (torch.ones(2, 4, 3, dtype=torch.int32), torch.ones(2, 4, dtype=torch.int32), True),       # a per-sample list passed as a shared one
        (torch.ones(4, 3, dtype=torch.int32), torch.ones(5, dtype=torch.int32), True),             # [K, L] against [K']
        (torch.ones(3, dtype=torch.int32), torch.ones(3, dtype=torch.int32), False),               # no label axis
    ]
    for labels, lens, shared in cases:          # (the layout is checked before anything else)
        with pytest.raises(ValueError):
            ops.ctc_align(acts, il, labels, lens, shared=shared)


def test_engine_methods():
    """The checks that need no engine state are made on an Engine that was never initialised (building one needs a GPU)."""
    from lstm_ctc_ocr_amd.engine import Engine
    assert list(inspect.signature(Engine.align).parameters) == ['self', 'data', 'seq_len', 'labels', 'blank']
    assert [(n, p.default) for n, p in inspect.signature(Engine.decode_spans).parameters.items()][3:] == [('method', 'greedy'), ('lexicon', None)]
    eng = object.__new__(Engine)
    for method in ('beam', 'viterbi', None):
        with pytest.raises(ValueError):
            eng.decode_spans(None, None, method=method)
    with pytest.raises(ValueError):
        eng.decode_spans(None, None, method='lexicon')
    # the signatures that must stay
    assert [(n, p.default) for n, p in inspect.signature(Engine.decode).parameters.items()][3:] == [('method', 'beam'), ('beam_width', 100), ('lexicon', None)]
    assert list(inspect.signature(Engine.score).parameters) == ['self', 'data', 'seq_len', 'lexicon', 'blank']
    assert list(inspect.signature(Engine.nbest).parameters) == ['self', 'data', 'seq_len', 'lexicon', 'k', 'blank']
