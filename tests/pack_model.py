"""Host model of every layout the weight re-pack writes (csrc/stream_ops.hip: pack_jobs_kernel and the per-tensor pack kernels), and the case
list of test_pack_model.py (the model, the table rules, without a GPU) and test_gpu_pack_jobs.py (the kernels and the engine).

One function per layout: it takes the fp32 master array and returns the bit pattern the device must hold (uint16 for bf16 operands, uint32 for
the fp32 LSTM bias).  Rounding is round to nearest even, as torch.Tensor.to(torch.bfloat16) does; a NaN becomes 0x7fc0.  The comparison rule
(check) is that of the cast tests: every non-NaN value bit for bit, every NaN stays a NaN of whatever payload - f2bf and the hardware's packed
conversion may differ there and nowhere else.  Nothing in this file has a tolerance.

EDGE_BITS, EDGE and _plain_randoms live here and are imported by test_gpu_memory_bound_kernels.py, so the casts and the packs see the same values.
"""
import numpy as np
import torch

EDGE_BITS = [
    0x00000000, 0x80000000,                          # +-0
    0x00000001, 0x80000001,                          # smallest denormals: round to +-0
    0x00008000, 0x00018000,                          # denormal ties: to even (stays 0) and from odd (up to 0x0002)
    0x00400000, 0x00410000,                          # denormals bf16 holds exactly
    0x007f8000,                                      # denormal tie from odd: rounds up to the smallest bf16 normal 0x0080
    0x007fffff, 0x807fffff,                          # largest denormals: round to +-0x0080, a normal
    0x00800000,                                      # smallest normal
    0x3f808000, 0xbf808000,                          # ties with an even lower half: stay
    0x3f818000, 0xbf818000,                          # ties with an odd lower half: go up
    0x3f808001, 0x3f807fff,                          # just above / below a tie
    0x7f7f7fff, 0xff7f7fff,                          # largest floats that round to +-bf16 max 0x7f7f
    0x7f7f8000, 0xff7f8000,                          # smallest floats that round to +-Inf
    0x7f7fffff,                                      # FLT_MAX -> Inf
    0x7f800000, 0xff800000,                          # +-Inf
    0x7fc00000, 0xffc00000, 0x7fc12345,              # quiet NaNs, one with a payload
    0x7f800001, 0xff800001, 0x7fa00000, 0x7f80ffff,  # signalling NaNs, payloads in the low half only: truncation would give +-Inf
]
EDGE = torch.from_numpy(np.array(EDGE_BITS, dtype=np.uint32).view(np.float32).copy())


def _plain_randoms(n, seed):
    """Uniform values in [-1, 1] and, every other element, uniform fp32 bit patterns (every exponent, some NaNs)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=g) * 2 - 1
    x[1::2] = torch.randint(-2 ** 31, 2 ** 31, (len(range(1, n, 2)),), dtype=torch.int64, generator=g).to(torch.int32).view(torch.float32)
    return x


# ================================================================================================ the model
def bf16_bits(x):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even; NaN -> 0x7fc0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[(u & 0x7fffffff) > 0x7f800000] = 0x7fc0
    return r


def perm(c, U):
    """TF gate-major LSTM column c = g * U + u -> its column in the packed operands: 16 units of the four gates side by side."""
    c = np.asarray(c)
    g, u = c // U, c % U
    return (u // 16) * 64 + g * 16 + u % 16


def transpose_layout(w2d, lstm_units=0):
    """[R][Cc] -> [perm(c)][R], values untouched."""
    R, Cc = w2d.shape
    out = np.empty((Cc, R), w2d.dtype)
    out[perm(np.arange(Cc), lstm_units) if lstm_units > 0 else np.arange(Cc)] = w2d.T
    return out


def transpose(w2d, lstm_units=0):
    return bf16_bits(transpose_layout(np.asarray(w2d, np.float32), lstm_units))


def conv_dgrad_layout(w):
    """w[tap][ci][co] (HWIO with the taps flattened) -> out[ci][8 - tap][co], values untouched."""
    w = np.asarray(w)
    w = w.reshape(9, w.shape[-2], w.shape[-1])
    return np.ascontiguousarray(w[::-1].transpose(1, 0, 2))


def conv_dgrad(w):
    return bf16_bits(conv_dgrad_layout(np.asarray(w, np.float32)))


def cast2d(src2d, cols):
    """The first `cols` columns of a strided fp32 matrix, row by row."""
    return bf16_bits(np.asarray(src2d, np.float32)[:, :cols])


def cast(x):
    return bf16_bits(np.asarray(x, np.float32).reshape(-1))


def lstm_bias(b, U):
    """fp32 [4U] gate-major -> fp32 in packed column order, as bit patterns (uint32)."""
    b = np.ascontiguousarray(b, np.float32).reshape(-1)
    out = np.empty(4 * U, np.uint32)
    out[perm(np.arange(4 * U), U)] = b.view(np.uint32)
    return out


def _is_nan(bits):
    if bits.dtype == np.uint16:
        return (bits & 0x7fff) > 0x7f80
    assert bits.dtype == np.uint32, bits.dtype
    return (bits & 0x7fffffff) > 0x7f800000


def check(what, got, want):
    """got == want (bit patterns of one width) wherever want is no NaN; got is a NaN wherever want is one."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    nan = _is_nan(want)
    assert bool(_is_nan(got[nan]).all()), what + ": a NaN did not stay a NaN"
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, "%s: %d of %d differ, first at flat index %d: got 0x%x, want 0x%x" % (
        what, bad.size, got.size, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def check_same(what, a, b, want):
    """Two device results agree under the rule: bit for bit where the model has no NaN, both NaN where it has one."""
    a, b, want = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1), np.asarray(want).reshape(-1)
    nan = _is_nan(want)
    assert bool(_is_nan(a[nan]).all()) and bool(_is_nan(b[nan]).all()), what + ": a NaN did not stay a NaN"
    bad = np.flatnonzero((a != b) & ~nan)
    assert bad.size == 0, "%s: %d of %d differ, first at flat index %d: 0x%x against 0x%x" % (
        what, bad.size, a.size, int(bad[0]), int(a[bad[0]]), int(b[bad[0]]))


# ================================================================================================ cases
POISON = -7.0
POISON_BF16 = 0xc0e0        # -7.0 as bf16; a destination arena is bf16 words of it throughout
SLACK = 256                 # poisoned elements in front of, behind and between destinations


def _cyc(n, start=0):
    """n edge values, cyclically."""
    return EDGE[(torch.arange(n) + start) % len(EDGE)]


class Case(object):
    """One pack job: the geometry of its source and destination buffers, its source values, its model.

    Source buffer: `src_elems` floats, the job's src pointer `src_off` floats into it; everything the job must not read is NaN.
    Destination buffer: `dst_elems` elements of `dst_bits` bits, the job's dst pointer `dst_off` elements into it; written(buf) is the view of
    the elements the job must write, in the order model() lists them, and everything else must keep its poison."""

    def __init__(self, type, R=0, Cc=0, ldin=0, U=0, ldout=0, n=0, src_rows=None, row0=0, col0=0, why=''):
        self.type, self.R, self.Cc, self.ldin, self.U, self.ldout, self.n = type, R, Cc, ldin, U, ldout, n
        self.row0, self.col0, self.why = row0, col0, why
        if type in (0, 2):
            self.src_rows = (row0 + R) if src_rows is None else src_rows
            self.src_elems, self.src_off = self.src_rows * ldin, row0 * ldin
        else:
            if type == 1:
                self.n = 9 * R * Cc
            self.src_elems, self.src_off = self.n, 0
        self.dst_bits = 32 if type == 4 else 16
        if type == 0:
            self.dst_elems, self.dst_off = R * Cc, 0
        elif type == 2:
            self.dst_elems, self.dst_off = R * ldout, col0       # the whole [R][ldout] matrix the job writes one column block of
        else:
            self.dst_elems, self.dst_off = self.n, 0
        if type == 0:
            self.id = 't0-%dx%d-ld%d-U%d%s' % (R, Cc, ldin, U, '-row%d' % row0 if row0 else '')
        elif type == 1:
            self.id = 't1-%dx%d' % (R, Cc)
        elif type == 2:
            self.id = 't2-%dx%d-ld%d-ld%d%s' % (R, Cc, ldin, ldout, '-col%d' % col0 if col0 else '')
        else:
            self.id = 't%d-n%d' % (type, self.n)

    def job(self, src_addr, dst_addr):
        """The job dict an op's pack_jobs() would return (addresses of the BUFFERS; the offsets are added here)."""
        j = dict(type=self.type, src=src_addr + 4 * self.src_off, dst=dst_addr + (self.dst_bits // 8) * self.dst_off)
        if self.type == 0:
            j.update(R=self.R, Cc=self.Cc, ldin=self.ldin, lstm_units=self.U)
        elif self.type == 1:
            j.update(R=self.R, Cc=self.Cc, n=self.n)
        elif self.type == 2:
            j.update(R=self.R, Cc=self.Cc, ldin=self.ldin, ldout=self.ldout)
        elif self.type == 3:
            j.update(n=self.n)
        else:
            j.update(lstm_units=self.U, n=self.n)
        return j

    def region(self, buf):
        """View of the source elements the job reads: [R][Cc] (types 0, 2) or flat."""
        if self.type in (0, 2):
            return buf.view(self.src_rows, self.ldin)[self.row0:self.row0 + self.R, :self.Cc]
        return buf

    def source(self, seed):
        """torch fp32 [src_elems]: _plain_randoms, EDGE in the first and last row and the first and last column of the region (flat
        sources: at both ends), NaN everywhere outside the region.  An axis shorter than 4 * len(EDGE) gets edge values on a quarter of
        its length at either end and the window starts at the seed, so that the tiny jobs of a long table still differ from each other."""
        k = len(EDGE)
        if self.type not in (0, 2):
            x = _plain_randoms(self.n, seed)
            m = min(k, max(1, self.n // 4))
            x[:m] = _cyc(m, seed)
            x[self.n - m:] = _cyc(m, seed + 7)
            return x
        buf = torch.full((self.src_elems,), float('nan'))
        reg = _plain_randoms(self.R * self.Cc, seed).view(self.R, self.Cc)
        mr, mc = min(k, max(1, self.R // 4)), min(k, max(1, self.Cc // 4))
        reg[:mr, 0] = _cyc(mr, seed + 5)
        reg[self.R - mr:, -1] = _cyc(mr, seed + 11)
        reg[0, :mc] = _cyc(mc, seed)
        reg[-1, self.Cc - mc:] = _cyc(mc, seed + 7)
        self.region(buf).copy_(reg)
        return buf

    def model(self, buf):
        """Bit patterns of written(), from the source buffer (torch fp32 or numpy)."""
        buf = torch.as_tensor(buf)
        reg = self.region(buf).numpy()
        if self.type == 0:
            return transpose(reg, self.U).reshape(-1)
        if self.type == 1:
            return conv_dgrad(reg.reshape(9, self.R, self.Cc)).reshape(-1)
        if self.type == 2:
            return cast2d(reg, self.Cc).reshape(-1)
        if self.type == 3:
            return cast(reg)
        return lstm_bias(reg, self.U)

    def written(self, dst):
        """numpy view (or copy) of a destination buffer [dst_elems]: the elements the job writes, in model order."""
        if self.type == 2:
            return dst.reshape(self.R, self.ldout)[:, self.col0:self.col0 + self.Cc]
        return dst


# Type 0, pack_jobs_kernel's transpose: (R, Cc, ldin, lstm_units).  Loads: f32x4 where c + 3 < Cc and ldin % 4 == 0, else four guarded scalars.
# Stores: u32x2 of four rows where R % 4 == 0, else up to four f2bf scalars.  One block per 64 x 64 tile.
T0 = [
    Case(0, 512, 64, 64, why='the shipped FC: one column tile, vector loads and stores only'),
    Case(0, 512, 37, 37, why='ragged columns and an odd row stride: every load scalar (ldin % 4 != 0), vector stores'),
    Case(0, 70, 130, 132, why='R % 4 != 0: scalar stores; partial tiles on both axes; the last column group (c = 128) half scalar; '
                              'ldin > Cc with NaN past the columns'),
    Case(0, 1, 4, 4, why='one row: a single vector load, four one-element scalar stores'),
    Case(0, 63, 5, 8, why='ldin % 4 == 0 but Cc = 5: one vector load and one scalar group per row; R % 4 != 0 with a three-row last group'),
    Case(0, 576, 128, 128, why='a conv pack (9 * 64 rows): 2 x 9 whole tiles'),
    Case(0, 512, 1024, 1024, U=256, src_rows=768, why="the headline's wxT: the gate permutation over 16 column tiles, rows 512.. of the cell matrix NaN"),
    Case(0, 256, 1024, 1024, U=256, src_rows=768, row0=512, why="the headline's whT: src a row offset into the same matrix, as the engine passes w[D:]"),
    Case(0, 24, 128, 128, U=32, why='the gate permutation with U = 32 (two 16-unit groups per gate) and a partial row tile'),
    Case(0, 1024, 2048, 2048, U=512, why='512 blocks, U = 512'),
]
# Type 1, the data-gradient flip: (Cin, Cout).  Four output channels per thread; min(ceil(n / 256), 512) blocks stride over n / 4 float4s.
T1 = [
    Case(1, 3, 4, why='one float4 per (tap, ci): 27 work items, one block'),
    Case(1, 64, 100, why='Cout / 4 = 25: the div / mod by a non power of two'),
    Case(1, 128, 256, why='a shipped layer; 294912 elements over 512 blocks, less than one pass'),
    Case(1, 512, 512, why='2.36 M elements = 589824 float4s over 512 * 256 threads: the grid-stride loop runs 4.5 times'),
]
# Type 2, the strided cast: (rows, cols, ldin, ldout), the three CAST2D shapes of test_gpu_memory_bound_kernels.py (the third, 34 MB, is the
# list's largest buffer: at 512 blocks it is the one whose loop goes round, 16 times) and the engine's wcat half.
T2 = [
    Case(2, 3, 40, 44, ldout=48, why='sub_block: 30 work items'),
    Case(2, 37, 200, 212, ldout=204, why='ragged: 1850 work items over 8 blocks, ldout < ldin'),
    Case(2, 2 * 4096 * 256 * 4 // 512 + 3, 512, 520, ldout=528, why='past the 512-block cap'),
    Case(2, 512, 1024, 1024, ldout=2048, src_rows=768, col0=1024, why="the engine's (D, 4U, 4U, 8U) into column half d = 1; the other half is slack"),
]
# Type 3, the flat cast: n.  min(ceil(n / 4 / 256), 2048) blocks.
T3 = [
    Case(3, n=4, why='one float4'),
    Case(3, n=4 * (256 * 5 + 37), why='six blocks, the last ragged'),
    Case(3, n=4 * (2 * 2048 * 256 + 37), why='past the 2048-block cap: the loop runs twice and a bit'),
]
# Type 4, the LSTM bias permutation: U.
T4 = [
    Case(4, U=32, n=128, why='half a block'),
    Case(4, U=256, n=1024, why='the headline: four blocks'),
    Case(4, U=512, n=2048, why='eight blocks'),
]
CASES = T0 + T1 + T2 + T3 + T4
# the per-tensor kernels take what the job kernel's types 1 and 3 do not: one ragged case each ((5, 6): Cout % 4 != 0; n = 30: the f2bf tail)
EXTRA_TRANSPOSE = Case(0, 5, 6, 6, why='pack_transpose: both tile axes ragged')
EXTRA_DGRAD_SHAPE = (5, 6)
EXTRA_CAST_N = 30


def small_jobs(count, first_seed):
    """`count` one-block jobs of mixed types with a seed each: n = 4 casts, (1, 4, 4, 0) transposes, U = 32 biases."""
    kinds = [lambda: Case(3, n=4), lambda: Case(0, 1, 4, 4), lambda: Case(4, U=32, n=128)]
    return [(kinds[i % 3](), first_seed + i) for i in range(count)]
