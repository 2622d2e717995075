"""Shapes and operands the tile generation of the fused conv1 + pool kernels (csrc/conv1.hip: conv1_pool_fwd_tile_kernel,
conv1_pool_bwd_tile_kernel) is tested at, the routine that runs its three training launches, and what they must give: exact_forward, and the
slab words of tests/golden/conv1_pool_first_generation.npz — shared by tests/test_gpu_conv1_tile.py (device; also as a child interpreter's
program: `python conv1_tile_cases.py OUT.npz Nb,W,H ...`) and tests/test_conv1_tile_shapes.py (the inputs' and the fixture's properties, no
GPU).  Plain module.

The fixture was recorded with this file's program from the first generation of the kernels at commit 29b4ab6 (`make EXPERIMENTS=1`,
OCR_NATIVE_LIB=<that library> and the knob that selected the first generation there; SHAPES at the default block size, PPB_SHAPE at OCR_CONV1_PPB=32 and 1024), in the same run in
which that commit's tile kernels passed their bit-equality tests against it and its pooled maps and codes equalled exact_forward.  That
generation is gone from the library, so the fixture cannot be recorded again: slab sums depend on the order of fp32 additions, and a kernel
that changes them needs a new argument, not a new recording.

A block owns a run of consecutive pooled pixels and stages the input rows they touch; the shapes are the smallest at which that can go wrong."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1_reference as cr  # noqa: E402

SHAPES = (
    (1, 2, 2),          # one pooled pixel, every halo element outside the image
    (2, 64, 2),         # H / 2 = 1: a run of 64 pixels is 64 pooled columns, and crosses into the second image
    (3, 30, 12),        # H / 2 = 6: 270 pixels = a full and a partial block of 256; runs cross two image boundaries, columns split between blocks
    (5, 24, 32),        # 960 pixels, partial last block
    (2, 250, 32),       # odd W / 2 = 125
)
PPB_SHAPE = (3, 30, 12)           # run again at OCR_CONV1_PPB = 32 and 1024
PPBS = {256: SHAPES, 32: (PPB_SHAPE,), 1024: (PPB_SHAPE,)}        # what the fixture holds: OCR_CONV1_PPB (256 = default) -> shapes
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv1_pool_first_generation.npz')
GRID_SEED = {(1, 2, 2): 8}        # one window x 64 channels: the first seed whose window holds a tied positive maximum (the others: seed 1)


def grid_operands(Nb, W, H, Co=64, seed=None):
    """Operands on the 1/64 grid (tests/test_gpu_kernels.py: test_conv1_pool_train_kernels_against_torch): every product is a multiple of
    2^-12 and every sum exact, so equal window values — ties — are frequent and a wrong first-maximum rule shows."""
    g = np.random.RandomState((GRID_SEED.get((Nb, W, H), 1) if seed is None else seed) + 31 * W + H)
    q = lambda t: (np.round(t * 64) / 64).astype(np.float32)
    return q(np.abs(g.standard_normal((Nb, W, H)))), q(0.3 * g.standard_normal((9, Co))), q(0.1 * g.standard_normal((Co,)))


def reference_operands(Nb, W, H):
    """The uniform random regime with full fp32 mantissas (few ambiguous windows): what the fp64 reference is asked about."""
    return cr.random_operands(Nb, W, H, seed=1 + W)


def tied_positive_share(x, w, b):
    """Share of the (window, channel) pairs whose positive maximum is held by two or more elements (on the reference's bf16 values)."""
    p = cr.Reference(x, w, b).pool()
    return float(((p['pooled'] > 0) & ((p['y'] == p['pooled'][:, :, :, None, :]).sum(3) >= 2)).mean())


def exact_forward(shape):
    """What the training forward must write on grid_operands(shape), from the fp64 reference alone: every product is a multiple of 2^-12 and
    max |x| sum |w| + max |b| <= 17.5 (17 bits), so the fp32 sums are exact in any order and z is the device's value (tests/
    test_conv1_tile_shapes.py asserts both).  -> (pooled bf16 bits, uint16 [Nb, W/2, H/2, 64]: the maximum over the window of bf16_rne(relu(z));
    codes, uint8 of the same shape: first arg-max in scan order | (max > 0) << 2, as cr.unpack_codes unpacks the device's words)."""
    z, _ = cr.conv(*grid_operands(*shape))
    y = cr.bf16_rne(cr.act(cr.windows(z), True) + 0.0)          # + 0.0: a -0.0 out of the maximum becomes the device's +0.0
    pooled = y.max(3)
    return cr.bf16_bits(pooled), y.argmax(3).astype(np.uint8) | ((pooled > 0).astype(np.uint8) << 2)


def fixture_key(ppb, shape, tag):
    """Key of tests/golden/conv1_pool_first_generation.npz: the slab words (int32 bit patterns) the first generation of the fused kernels
    wrote on grid_operands(shape) at OCR_CONV1_PPB = ppb, from saved codes (tag 'slab_codes') and from recomputed windows ('slab_recompute')."""
    return '%d/%dx%dx%d/%s' % ((ppb,) + tuple(shape) + (tag,))


def run_train_launches(dev, shape):
    """Forward-train and the slab backward with saved codes and with recomputed windows on grid_operands(shape), by the loaded library.
    -> dict of numpy arrays: pooled (bf16 bits), codes, slab_codes, slab_recompute (fp32 bits)."""
    import torch
    from lstm_ctc_ocr_amd import ops
    Nb, W, H = shape
    x, w, b = grid_operands(Nb, W, H)
    npix = Nb * (W // 2) * (H // 2)
    xd, wd, bd = (torch.from_numpy(a).to(dev) for a in (x, w, b))
    codes = torch.full((npix, 8), -1, dtype=torch.int32, device=dev)
    p = ops.conv1_pool_fwd(xd, wd, bd, codes=codes)
    dp = torch.from_numpy(cr.make_dp((Nb, W // 2, H // 2, 64), 4)).to(dev).to(torch.bfloat16)
    rows = ops.conv1_pool_bwd_slab_rows(Nb, W, H)
    out = dict(pooled=p.view(torch.int16).cpu().numpy(), codes=codes.cpu().numpy())
    for tag, cd in (('slab_codes', codes), ('slab_recompute', None)):
        slab = torch.full((rows, 640), float('nan'), device=dev)
        ops.conv1_pool_bwd_slab(xd, wd, bd, dp, slab, codes=cd)
        out[tag] = slab.view(torch.int32).cpu().numpy()
    return out


if __name__ == '__main__':
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    for s in sys.argv[2:]:
        shape = tuple(int(v) for v in s.split(','))
        for k, v in run_train_launches(torch.device('cuda', 0), shape).items():
            res['%dx%dx%d/%s' % (shape + (k,))] = v
    np.savez(sys.argv[1], **res)
    print('TILE_CASES_OK', len(res))
