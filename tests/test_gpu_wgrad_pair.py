"""Two layers' 3x3 weight-gradient slab kernels in ONE launch (ocr_conv3x3_wgrad_pair_defer_bf16) against the same two layers as two
launches of ocr_conv3x3_wgrad_defer_bf16 on workspaces of their own.  The paired launch changes only where a layer's workgroups are
dispatched: every workgroup runs the code, the split and the tile it has in its own launch, so the comparison is for EQUALITY — the slab
workspaces word for word, then dw and db behind the merged reduction — on normal random operands (no exactly-summable grid is needed).

The cases are the smallest at which each piece can go wrong (shapes N x W x H, Cin -> Cout).  The split counts in the comments are what
w9_plan gives these shapes (asserted below through the kernel-choice query); the first job of a .. d is 1 x 32 x 16, 64 -> 128:
wgrad9_kernel, S = 1, grid 2, so the second job's workgroups start at block 2 — no multiple of 8.
  a   8 x 64 x 8, 128 -> 256    wgrad9p<8>, S = 8: the split = xcd map (1) behind a first grid that is no multiple of 8
  a2  4 x 64 x 8, 128 -> 256    wgrad9p<8>, S = 4: the 8/S-XCDs-per-split map (2) behind the same
  b   16 x 64 x 8, 128 -> 256   wgrad9p<8>, S = 16: map 1 with two rounds of splits
  c   16 x 24 x 8, 128 -> 128   the zero-row wgrad9p<8>: steps cross image boundaries (S = 4, map 2)
  d   16 x 32 x 4, 256 -> 512   wgrad9p<4> (S = 4, 128 workgroups)
  e   4 x 24 x 16, 128 -> 64    wgrad9_kernel behind wgrad9_kernel (S = 2 on 2 tiles: the plain map 0)
  f   64 x 128 x 16, 64 -> 128 in front of 64 x 64 x 8, 128 -> 256: the product pair (conv2 + conv3_1 of the 64 x 256 batch)
(a and b are the shapes the pairing was specified with, where they were expected to give S = 4 / map 2 and S = 8 / map 1; the planner
gives them S = 8 and S = 16, both map 1 — a2 is there so that map 2 behind an odd offset is still exercised on a whole-image wgrad9p<8>.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lstm_ctc_ocr_amd import ops
from lstm_ctc_ocr_amd.engine import Engine

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FIRST = (1, 32, 16, 64, 128)
CASES = {
    'a': (FIRST, (8, 64, 8, 128, 256), ('wgrad9', 1), ('wgrad9p<8>', 8)),
    'a2': (FIRST, (4, 64, 8, 128, 256), ('wgrad9', 1), ('wgrad9p<8>', 4)),
    'b': (FIRST, (16, 64, 8, 128, 256), ('wgrad9', 1), ('wgrad9p<8>', 16)),
    'c': (FIRST, (16, 24, 8, 128, 128), ('wgrad9', 1), ('wgrad9p<8>/zero-row', 4)),
    'd': (FIRST, (16, 32, 4, 256, 512), ('wgrad9', 1), ('wgrad9p<4>', 4)),
    'e': (FIRST, (4, 24, 16, 128, 64), ('wgrad9', 1), ('wgrad9', 2)),
    'f': ((64, 128, 16, 64, 128), (64, 64, 8, 128, 256), ('wgrad9', 64), ('wgrad9p<8>', 32)),
}


def _operands(shape, seed, dev):
    Nb, W, H, Ci, Co = shape
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((Nb, W, H, Ci), generator=g, device=dev).to(BF)
    dy = torch.randn((Nb, W, H, Co), generator=g, device=dev).to(BF)
    return x, dy


def _outputs(shape, dev, poison):
    Nb, W, H, Ci, Co = shape
    need = ops.conv3x3_wgrad_workspace_bytes(Nb, W, H, Ci, Co)
    assert need > 0
    ws = torch.full((need,), poison, dtype=torch.uint8, device=dev)      # scratch is neither zeroed nor kept: poison it
    return torch.zeros((3, 3, Ci, Co), dtype=torch.float32, device=dev), torch.zeros(Co, dtype=torch.float32, device=dev), ws


def _reduce(jobs, dev):
    """The merged reduction over the pending jobs, with the table Engine._flush_w9 builds."""
    tab = np.frombuffer(b''.join(j for j, _ in jobs), dtype=Engine.W9_JOB_DTYPE).copy()
    start = 0
    for i, (_, nblk) in enumerate(jobs):
        tab['block_start'][i] = start
        start += nblk
    ops.wgrad9_reduce_jobs(torch.from_numpy(tab.view(np.uint8).copy()).to(dev), len(jobs), start)


def _pair(first, second, ops0, ops1, dev, poison):
    o0, o1 = _outputs(first, dev, poison), _outputs(second, dev, poison)
    jobs = ops.conv3x3_wgrad_pair_deferred((ops0[0], ops0[1], o0[0], o0[1], o0[2]), (ops1[0], ops1[1], o1[0], o1[1], o1[2]))
    slabs = (o0[2].clone(), o1[2].clone())
    _reduce(list(jobs), dev)
    return slabs, (o0[0], o0[1], o1[0], o1[1]), jobs


@pytest.mark.parametrize("case", sorted(CASES))
def test_pair_equals_two_single_launches(dev, case):
    first, second, want0, want1 = CASES[case]
    assert ops.conv3x3_wgrad_kernel_choice(*first) == want0 and ops.conv3x3_wgrad_kernel_choice(*second) == want1
    assert ops.conv3x3_wgrad_pair_supported(first, second)
    ops0, ops1 = _operands(first, 11, dev), _operands(second, 12, dev)
    # the two layers as two launches
    single, sjobs = [], []
    for shape, (x, dy) in ((first, ops0), (second, ops1)):
        dw, db, ws = _outputs(shape, dev, 0x7f)
        job, nblk = ops.conv3x3_wgrad_deferred(x, dy, dw, db, ws)
        assert job is not None
        single.append((dw, db, ws))
        sjobs.append((job, nblk))
    slabs_single = (single[0][2].clone(), single[1][2].clone())
    _reduce(sjobs, dev)
    # ... and as one, twice
    slabs, grads, jobs = _pair(first, second, ops0, ops1, dev, 0x5a)
    slabs2, grads2, _ = _pair(first, second, ops0, ops1, dev, 0xa5)
    torch.cuda.synchronize()
    assert [n for _, n in jobs] == [n for _, n in sjobs]
    for k in range(2):
        assert torch.equal(slabs[k], slabs_single[k]), 'slab workspace of job %d' % k
        assert torch.equal(slabs2[k], slabs[k]), 'slab workspace of job %d, second run' % k
    want = (single[0][0], single[0][1], single[1][0], single[1][1])
    for name, got, again, ref in zip(('dw0', 'db0', 'dw1', 'db1'), grads, grads2, want):
        assert torch.equal(got, ref), name
        assert torch.equal(again, got), name + ', second run'
        assert bool(got.abs().max() > 0), name
    if case == 'a':
        # against torch's fp32 convolution weight gradient, at the tolerance of tests/test_gpu_kernels.py for this family
        for (x, dy), dw, db in ((ops0, grads[0], grads[1]), (ops1, grads[2], grads[3])):
            xr = x.float().cpu()
            wr = torch.zeros((3, 3, x.shape[-1], dy.shape[-1]), requires_grad=True)
            y = F.conv2d(xr.permute(0, 3, 1, 2), wr.permute(3, 2, 0, 1), None, padding=1).permute(0, 2, 3, 1)
            y.backward(dy.float().cpu())
            err = float((dw.cpu().double() - wr.grad.double()).abs().max()) / float(wr.grad.double().abs().max())
            print('relative error of dw against fp32 torch: %.3g' % err)
            assert err < 1e-4, err
            cs = dy.float().cpu().reshape(-1, dy.shape[-1]).sum(0)
            assert float((db.cpu().double() - cs.double()).abs().max()) / float(cs.double().abs().max()) < 1e-4


def test_pair_refuses_what_the_query_refuses(dev):
    """A pair the policy does not take is an error of the launch, nothing runs: here a plane-layout kernel in front."""
    from lstm_ctc_ocr_amd import _native as nat
    first, second = (16, 32, 4, 256, 512), FIRST
    assert not ops.conv3x3_wgrad_pair_supported(first, second)
    ops0, ops1 = _operands(first, 1, dev), _operands(second, 2, dev)
    o0, o1 = _outputs(first, dev, 0x33), _outputs(second, dev, 0x33)
    with pytest.raises(nat.NativeError):
        ops.conv3x3_wgrad_pair_deferred((ops0[0], ops0[1], o0[0], o0[1], o0[2]), (ops1[0], ops1[1], o1[0], o1[1], o1[2]))
    torch.cuda.synchronize()
    assert bool((o0[2] == 0x33).all()) and bool((o1[2] == 0x33).all())
