"""fp64 reference of the first layer exactly as the device defines it (csrc/conv1.hip: conv1_fwd_kernel, conv1_wgrad_kernel,
conv1_pool_fwd_tile_kernel<CODES>, conv1_pool_bwd_tile_kernel<CODES> in its atomics and slab forms), the bounds the device has to meet with their
derivation, and the checker that tests/test_gpu_conv1.py (device) and tests/test_conv1_reference.py (a numpy model, no GPU) share.
Plain module, numpy only.

  x f32 [Nb, W, H] (one channel) -> conv 3 x 3 SAME with taps w [3][3][1][Co] (tap t = 3 i + j reads x[w + i - 1][h + j - 1], zero outside
  the image) + bias -> optional ReLU -> bf16 [Nb, W, H, Co]; the fused kernels keep only the 2 x 2 max-pool of that map.
  fp32 inputs are exact in fp64 and a product of two of them is exact too, so the fp64 sums below are the real values to 2^-53.

u = 2^-24 (unit roundoff of fp32), gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability, lemma 3.1).

FORWARD BOUND, per element.  The device computes s_1 = fl(x_1 w_1 + 0), s_t = fma(x_t, w_t, s_{t-1}) for the nine taps, then o = fl(s_9 +
b): ten correctly rounded operations in a row.  The product of tap t passes through the roundings t .. 9 and the one of the bias add, at
most ten factors (1 + d), |d| <= u; the bias through one.  Hence |o - z| <= gamma(10) a with a = sum |x_t w_t| + |b|, that is
    c = 10 / (1 - 10 u)         (C_FWD; 10.000006)
in `e = c 2^-24 a`.  max(., 0) is 1-Lipschitz, so |act(o) - act(z)| <= e, and the round-to-nearest-even to bf16 adds at most half a bf16
ulp: |y_dev - act(z)| <= ulp_bf16(act(z)) / 2 + e.  (The ulp is that of the reference value.  Where e < ulp / 2 a device value that has
crossed into the next binade rounds onto the power of two itself, which is within e of the reference, so the bound is strict; where e
exceeds the ulp — heavy cancellation next to zero — the rounding term is 2^-9 of e and immaterial.)  The pooled value is the maximum of
four such values and max is 1-Lipschitz in the sup norm: the same bound with the largest of the four e.

AMBIGUITY.  Rounding and ReLU are monotone, so the device's bf16 value lies in [bf16(act(z - e)), bf16(act(z + e))].  An element whose
interval is a single value is determined by the reference alone; the others (next to a rounding midpoint, or next to zero under the
ReLU) are ambiguous, and so is a window that holds one.
  unambiguous window   all four bf16 values are known: the pooled value bit for bit, and the 4-bit code exactly — bits 0-1 the FIRST maximum
                       of the rounded values in the scan order e = 2 (w offset) + (h offset), bit 2 = (max > 0), bit 3 = 0.
  ambiguous window     the device chose b with r_b >= r_j for the reference's arg-max j; r_b <= v_b + e_b + ulp / 2 and r_j >= v_j - e_j -
                       ulp / 2 (ulp of the window maximum, the larger of the two), hence v_j - v_b <= ulp + e_b + e_j.  Bit 2 set needs max hi
                       > 0, bit 2 clear needs max lo <= 0 for the interval ends lo, hi of the four elements.

BACKWARD.  gv = dp (bf16, exact) where bit 2 of the code is set, else 0; db[c] = sum gv, dW[t][c] = sum patch_best[t] gv, with the
reference's code in unambiguous windows and the device's own code in ambiguous ones (either choice is a valid gradient there).
Every term is one exact product rounded inside an fma; what the device adds to it is summation error: |dev - ref| <= gamma(k) sum |term|,
k = the longest chain of fp32 additions a partial sum passes through (chain_bwd):
    ppb / 32     the fmas of one thread: a block owns ppb consecutive pooled pixels, its 32 pixel lanes take every 32nd
  + 3            the shuffles over the lane bits 8, 16, 32 (the eight pixel lanes of a wave)
  + 3            red[0] + red[1] + red[2] + red[3] through LDS (four waves)
  + blocks       atomics form only: the atomicAdds of all blocks onto one word, ceil(npix / 256) of them (the first lands on a zero, so
                 this counts one too many)
  + 0            slab form: the test adds the rows in fp64
conv1_wgrad is the same reduction over the full-resolution pixels against a given bf16 dz, 1024 pixels per block, atomics: k = 32 + 6 +
ceil(npix / 1024).

Every check returns max |device - reference| / bound per tensor; the tests assert <= 1.
"""
import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64


def gamma(n):
    return n * U / (1.0 - n * U)


C_FWD = 10.0 / (1.0 - 10.0 * U)
WGRAD_PPB, ATOMICS_PPB = 1024, 256


def chain_bwd(ppb, atomic_blocks=0):
    """k of the backward bound: the longest chain of fp32 additions (module docstring)."""
    return ppb // 32 + 3 + 3 + atomic_blocks


def ceil_div(a, b):
    return -(-a // b)


# ================================================================================================ bf16 on fp64 values
def bf16_ulp(v):
    """Spacing of the bf16 grid at |v| (fp64 array): 2^(floor(log2 |v|) - 7), the subnormal spacing 2^-133 below 2^-126.  On the bits: the
    exponent field of the fp64 number, lowered by 7."""
    u = np.ascontiguousarray(v, F64).view(np.uint64)
    ex = np.maximum((u >> np.uint64(52)) & np.uint64(0x7ff), np.uint64(1023 - 126))
    return ((ex - np.uint64(7)) << np.uint64(52)).view(F64)


def bf16_rne(v):
    """fp64 -> the nearest bf16 value, ties to even, in ONE rounding (no detour through fp32); returned as fp64.  On the bits: bf16 keeps 7
    of the 52 fraction bits, so add half of the dropped 45 bits' range (less one, plus the lowest kept bit: ties to even) and clear them —
    the carry into the exponent is the rounding up to the next power of two.  Below 2^-126 the grid is the subnormal one."""
    v = np.ascontiguousarray(v, F64)
    u = v.view(np.uint64)
    r = ((u + np.uint64((1 << 44) - 1) + ((u >> np.uint64(45)) & np.uint64(1))) & np.uint64(~((1 << 45) - 1) & (2 ** 64 - 1))).view(F64)
    small = np.abs(v) < 2.0 ** -126
    if small.any():
        r = np.where(small, np.rint(v / 2.0 ** -133) * 2.0 ** -133, r)
    return r


def bf16_bits(v):
    """The 16 bits of values that ARE bf16 numbers (any float array) — what a bit-for-bit comparison compares."""
    return (np.ascontiguousarray(v, F32).view(np.uint32) >> 16).astype(np.uint16)


def f32_to_bf16(a, truncate=False):
    """fp32 array -> bf16 value as fp32, round to nearest even (the device's conversion) or truncation (a wrong one, for the model)."""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    if not truncate:
        u = u + 0x7fff + ((u >> 16) & 1)
    return ((u >> 16) << 16).astype(np.uint32).view(F32)


# ================================================================================================ forward
def pad(x):
    x = np.asarray(x, F32)
    xp = np.zeros((x.shape[0], x.shape[1] + 2, x.shape[2] + 2), F64)
    xp[:, 1:-1, 1:-1] = x
    return xp


def taps(xp, W, H, a=0, b=0, step=1):
    """[9, pixels]: what tap t = 3 i + j multiplies at the pixels (a + step w, b + step h) of the padded images xp."""
    return np.stack([xp[:, a + i:a + i + step * W:step, b + j:b + j + step * H:step].reshape(-1) for i in range(3) for j in range(3)])


def conv(x, w, b):
    """-> z (fp64 [Nb, W, H, Co], before the activation) and a = sum |x w| + |b|."""
    Nb, W, H = x.shape
    w9 = np.asarray(w, F32).reshape(9, -1).astype(F64)
    b = np.asarray(b, F32).astype(F64)
    P = np.ascontiguousarray(taps(pad(x), W, H).T)
    z = P @ w9
    z += b
    a = np.abs(P) @ np.abs(w9)
    a += np.abs(b)
    shape = (Nb, W, H, w9.shape[1])
    return z.reshape(shape), a.reshape(shape)


def act(z, relu):
    return np.maximum(z, 0.0) if relu else z


def windows(t):
    """[Nb, W, H, Co] -> [Nb, W/2, H/2, 4, Co], element e = 2 (w offset) + (h offset) of the 2 x 2 window."""
    Nb, W, H, Co = t.shape
    return t.reshape(Nb, W // 2, 2, H // 2, 2, Co).transpose(0, 1, 3, 2, 4, 5).reshape(Nb, W // 2, H // 2, 4, Co)


def unpack_codes(words, shape):
    """The device's code words, uint32 [pooled pixels][8]: nibble c of word g belongs to channel 8 g + c.  -> uint8, `shape` = [Nb, W/2,
    H/2, 64]."""
    wd = np.ascontiguousarray(words).view(np.uint32).reshape(-1, 8, 1)
    return ((wd >> (4 * np.arange(8, dtype=np.uint32))) & 15).astype(np.uint8).reshape(shape)


def _worst(diff, bound):
    """max diff / bound; an exact match counts 0 whatever the bound, a mismatch against a zero bound inf; NaN in diff gives inf."""
    diff = np.asarray(diff, F64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(diff == 0, 0.0, diff / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


class Reference:
    """The fp64 reference of one (x, w, b) and every check against it.  Device tensors come in as numpy arrays: bf16 ones converted to fp32
    (exact), code words as the int32 / uint32 array the kernel wrote."""

    def __init__(self, x, w, b):
        self.x = np.ascontiguousarray(x, F32)
        self.w = np.ascontiguousarray(w, F32).reshape(9, -1)
        self.b = np.ascontiguousarray(b, F32)
        self.Nb, self.W, self.H = self.x.shape
        self.Co = self.w.shape[1]
        self.z, a = conv(self.x, self.w, self.b)
        self.e = a
        self.e *= C_FWD * U
        self._pool = None

    # ---------------------------------------------------------------------------------------- full resolution
    def check_full(self, y_dev, relu):
        """conv1_fwd: max |y_dev - act(z)| / (ulp / 2 + e) over every element."""
        v = act(self.z, relu)
        return _worst(np.abs(np.asarray(y_dev, F64) - v), 0.5 * bf16_ulp(v) + self.e)

    def wgrad(self, dz):
        """conv1_wgrad against a given bf16 dz [Nb, W, H, Co] (as fp32): dW [9, Co], db [Co], and the sums of |term|."""
        xp = pad(self.x)
        g = np.asarray(dz, F64).reshape(-1, self.Co)
        P = taps(xp, self.W, self.H)
        return dict(dw=P @ g, db=g.sum(0), abs_dw=np.abs(P) @ np.abs(g), abs_db=np.abs(g).sum(0))

    def check_wgrad(self, dz, dw_dev, db_dev):
        r = self.wgrad(dz)
        k = chain_bwd(WGRAD_PPB, ceil_div(self.Nb * self.W * self.H, WGRAD_PPB))
        return _check_sums(r, dw_dev, db_dev, k)

    # ---------------------------------------------------------------------------------------- pooled map and codes
    def pool(self):
        """The window view of the ReLU reference (computed once): values, fp32 terms, the determined bf16 values and interval ends, the
        reference's pooled map and codes, which windows are ambiguous, and which unambiguous ones hold a positive tie."""
        if self._pool is None:
            z, e = windows(self.z), windows(self.e)
            p = dict(v=act(z, True), e=e)
            y = bf16_rne(p['v'])
            # lo and hi differ from y only where the interval reaches a quarter ulp from y (the nearer cell edge of a power of two) or,
            # at y = 0, above zero: the two roundings are done there alone
            near = np.where(y == 0, z + e > 0, np.abs(p['v'] - y) + e >= 0.25 * bf16_ulp(y))
            p['y'] = y.astype(F32)
            p['lo'], p['hi'] = p['y'].copy(), p['y'].copy()
            p['lo'][near] = bf16_rne(act(z[near] - e[near], True))
            p['hi'][near] = bf16_rne(act(z[near] + e[near], True))
            del z, y, near
            p['amb'] = (p['lo'] != p['hi']).any(3)
            p['pooled'] = p['y'].max(3)
            best = p['y'].argmax(3).astype(np.uint8)                                     # numpy's arg-max is the first maximum
            p['code'] = best | ((p['pooled'] > 0).astype(np.uint8) << 2)
            p['vmax'] = p['v'].max(3)
            p['tie'] = (p['pooled'] > 0) & ((p['y'] == p['pooled'][:, :, :, None, :]).sum(3) >= 2) & ~p['amb']
            self._pool = p
        return self._pool

    def shares(self):
        """(ambiguous share of the (window, channel) pairs, share of positive-maximum ties among the unambiguous ones)."""
        p = self.pool()
        clear = int((~p['amb']).sum())
        return float(p['amb'].mean()), (float(p['tie'].sum()) / clear if clear else 0.0)

    def check_pooled(self, p_dev, codes_dev=None):
        """conv1_pool_fwd.  -> dict of ratios (<= 1 passes): 'pooled' the forward bound on every window; 'exact' 0 if every unambiguous window
        is bit for bit the reference, else inf; with codes 'codes' (unambiguous: equal; bit 3 clear everywhere), 'choice' (ambiguous: the
        chosen element against the window maximum) and 'relu_bit' (ambiguous: consistent with the interval)."""
        p = self.pool()
        pd = np.asarray(p_dev, F32).reshape(p['pooled'].shape)
        clear = ~p['amb']
        out = dict(pooled=_worst(np.abs(pd.astype(F64) - p['vmax']), 0.5 * bf16_ulp(p['vmax']) + p['e'].max(3)),
                   exact=0.0 if np.array_equal(bf16_bits(pd[clear]), bf16_bits(p['pooled'][clear])) else np.inf)
        if codes_dev is None:
            return out
        cd = unpack_codes(codes_dev, p['code'].shape)
        out['codes'] = 0.0 if np.array_equal(cd[clear], p['code'][clear]) and not (cd & 8).any() else np.inf
        amb = p['amb']
        b = (cd & 3).astype(np.intp)[:, :, :, None, :]
        j = p['v'].argmax(3)[:, :, :, None, :]
        take = lambda t, i: np.take_along_axis(t, i, 3)[:, :, :, 0, :]
        gap = p['vmax'] - take(p['v'], b)
        room = bf16_ulp(p['vmax']) + take(p['e'], b) + take(p['e'], j)
        out['choice'] = _worst(gap[amb], room[amb])
        bit = (cd & 4) != 0
        ok = np.where(bit, p['hi'].max(3) > 0, p['lo'].max(3) <= 0)
        out['relu_bit'] = 0.0 if ok[amb].all() else np.inf
        return out

    # ---------------------------------------------------------------------------------------- backward
    def backward(self, dp, codes_dev):
        """The reference's code in unambiguous windows, the device's in ambiguous ones -> dw [9, Co], db [Co], sums of |term|."""
        p = self.pool()
        code = np.where(p['amb'], unpack_codes(codes_dev, p['code'].shape), p['code'])
        return self.backward_with(dp, code)

    def backward_with(self, dp, code):
        Wo, Ho, Co = self.W // 2, self.H // 2, self.Co
        xp = pad(self.x)
        gv = np.where((code & 4) != 0, np.asarray(dp, F64).reshape(code.shape), 0.0).reshape(-1, Co)
        best = (code & 3).reshape(-1, Co)
        dw, aw = np.zeros((9, Co)), np.zeros((9, Co))
        for el in range(4):
            a, b = el >> 1, el & 1
            g = np.where(best == el, gv, 0.0)
            P = taps(xp, Wo, Ho, a, b, 2)
            dw += P @ g
            aw += np.abs(P) @ np.abs(g)
        return dict(dw=dw, db=gv.sum(0), abs_dw=aw, abs_db=np.abs(gv).sum(0))

    def check_backward(self, bw, dw_dev, db_dev, ppb, atomics):
        """bw = self.backward(dp, codes_dev), computed once for all forms.  conv1_pool_bwd (atomics=True: dw_dev / db_dev are the accumulated
        fp32 tensors) or conv1_pool_bwd_slab (atomics=False: the slab rows added in fp64, split into dw and db).  -> dict(dw=, db=)."""
        npix = self.Nb * (self.W // 2) * (self.H // 2)
        k = chain_bwd(ppb, ceil_div(npix, ppb) if atomics else 0)
        return _check_sums(bw, dw_dev, db_dev, k)


def _check_sums(r, dw_dev, db_dev, k):
    dw = np.asarray(dw_dev, F64).reshape(r['dw'].shape)
    db = np.asarray(db_dev, F64).reshape(r['db'].shape)
    return dict(dw=_worst(np.abs(dw - r['dw']), gamma(k) * r['abs_dw']), db=_worst(np.abs(db - r['db']), gamma(k) * r['abs_db']))


def slab_sums(slab):
    """slab [rows, 640] fp32 = {dW [9][64] | db [64]} per block -> (dw [9, 64], db [64]), the rows added in fp64."""
    tot = np.asarray(slab, F64).sum(0)
    return tot[:576].reshape(9, 64), tot[576:]


# ================================================================================================ inputs
AMBIGUOUS_CAP, TIE_FLOOR = 0.05, 0.05

# name: (regime, source, Nb, W, H).  Regimes: 'captcha' committed images x = u8 / 255 with the committed trained conv1 taps and biases (bf16-
# representable); 'perturbed' the same with the taps and biases perturbed to full fp32 mantissas; 'random' the uniform regime; 'zeros' /
# 'ones' constant images under the perturbed taps (every interior window a four-way exact tie, only the borders differ; under the bf16-
# representable taps a sum of nine of them is a short binary number and sits exactly ON a bf16 rounding midpoint in 9 to 13 of the 64
# channels — the device computes those sums exactly, but by the definition above the whole channel is ambiguous, 13 to 20 % of the windows).
# The small shapes of the captcha regimes are crops of batch C1 inside the text (columns 10 .. 10 + W, rows 10 .. 10 + H).
SMALL = ((1, 2, 2), (2, 6, 2), (3, 30, 12))       # one pooled pixel / H/2 = 1 / odd W/2 and H/2 and a partial last block of 256 and of 1024
CASES = {}
for _s in SMALL:
    for _r in ('captcha', 'perturbed', 'random', 'zeros', 'ones'):
        CASES['%s-%dx%dx%d' % ((_r,) + _s)] = (_r, 'C1') + _s
CASES['captcha-C1'] = ('captcha', 'C1', 8, 88, 32)
CASES['perturbed-C1'] = ('perturbed', 'C1', 8, 88, 32)
CASES['captcha-V0'] = ('captcha', 'V0', 28, 320, 32)      # 71680 pooled pixels: a second sweep of the forward grid (65536 per sweep)
CASES['perturbed-V0'] = ('perturbed', 'V0', 28, 320, 32)
FULL_ONLY = {'captcha-V0x7': ('captcha', 'V0', 7, 320, 32)}      # 71680 full-resolution pixels: a second sweep of conv1_fwd
BATCH_CASES = ('captcha-C1', 'perturbed-C1', 'captcha-V0', 'perturbed-V0')        # whole rendered images: the tie-share floor holds here


_FIXTURE = {}


def _fixture():
    """The committed trained conv1 taps [9, 64] and biases [64], and the committed captcha batches (loaded once)."""
    if not _FIXTURE:
        import os
        import sys
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
        sys.path.insert(0, golden)
        try:
            import make_trained_fixture as fx
        finally:
            sys.path.remove(golden)
        wts = fx.load_weights()
        d = np.load(fx.BATCHES)
        _FIXTURE.update(w=wts['conv1/weights'].reshape(9, -1).astype(F32), b=wts['conv1/biases'].astype(F32),
                        C1=fx.load_batch(d, 'C1')[0], V0=fx.load_batch(d, 'V0')[0])
    return _FIXTURE


def case_operands(name):
    """-> x [Nb, W, H], w [9, 64], b [64] (fp32) of a case of CASES / FULL_ONLY."""
    regime, source, Nb, W, H = CASES.get(name) or FULL_ONLY[name]
    if regime == 'random':
        return random_operands(Nb, W, H, seed=1 + W)
    fx = _fixture()
    w, b = fx['w'], fx['b']
    if regime in ('perturbed', 'zeros', 'ones'):
        w, b = perturb(w, 11), perturb(b, 12)
    if regime in ('zeros', 'ones'):
        return np.full((Nb, W, H), 0.0 if regime == 'zeros' else 1.0, F32), w, b
    x = fx[source]
    o = 0 if H == x.shape[2] else 10
    return np.ascontiguousarray(x[:Nb, o:o + W, o:o + H], F32), w, b


def random_operands(Nb, W, H, Co=64, seed=1):
    """The uniform random regime of the existing conv1 tests: x in [0, 1), taps in (-0.3, 0.3), biases in (-0.1, 0.1), full fp32 mantissas."""
    g = np.random.RandomState(seed)
    x = g.uniform(0, 1, (Nb, W, H)).astype(F32)
    w = g.uniform(-0.3, 0.3, (9, Co)).astype(F32)
    b = g.uniform(-0.1, 0.1, (Co,)).astype(F32)
    return x, w, b


def perturb(w, seed):
    """w (1 + 2^-10 r), r uniform in (-1, 1): bf16-representable taps become full fp32 mantissas."""
    g = np.random.RandomState(seed)
    w = np.asarray(w, F32)
    return (w.astype(F64) * (1.0 + 2.0 ** -10 * g.uniform(-1, 1, w.shape))).astype(F32)


def make_dp(shape, seed):
    """bf16 values (as fp32) in (-1, 1) with exact zeros in about a quarter of the places."""
    g = np.random.RandomState(seed)
    dp = f32_to_bf16(g.uniform(-1, 1, shape).astype(F32))
    dp[g.uniform(0, 1, shape) < 0.25] = 0.0
    return dp
