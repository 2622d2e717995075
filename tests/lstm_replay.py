"""Step replay reference for the BiLSTM kernels (lstm.hip, lstm_seq.hip): every step is checked in isolation.

For step s the reference takes what the device itself stored for step s - 1 (the bf16 hout row, the fp32 cell row; backward: the bf16 dz
row of step s + 1), recomputes step s in float64 from the same bf16 operands and compares.  The device's error of ONE step is then not mixed
with the propagated error of the steps before it, and the bound per element is a derived one (below), not a measured one.

Tensor layouts are the device's own (numpy arrays, R = N * T rows, row(n, t) = n * T + t, ND directions):
  hout  [R, ND * U]      bf16 values as float32          gates [ND, R, 4U] fp32, PACKED columns p(g, u) = (u / 16) * 64 + g * 16 + u % 16
  cell  [ND, R, U] fp32                                   xproj [R, ND * 4U] fp32, packed columns, bias inside
  dz    [R, ND * 4U]     bf16 values, MASTER columns g * U + u        dhout [R, ND * U] bf16 values
  Wh[d] [U, 4U], Wx[d] [D, 4U], b[d] [4U]: master columns (i, j, f, o), bf16-representable values (the biases: fp32)

Error model (u = 2^-24, the fp32 unit round-off).

  Pre-activation.  z is a sum of K products (+ the projection / bias term, + forget_bias) accumulated in fp32 in whatever order:
      dz_pre = (K + 2) u mag,   mag = sum of the absolute values of everything that is added.

  Activations as built (common.h sigmoidf_ / tanhf_, lstm_seq.hip sigmoid_q / tanh_q): __expf(x) = v_exp_f32(x * log2(e)), then v_rcp_f32
  (or the correctly rounded reciprocal, which is better).  v_exp_f32 and v_rcp_f32 are 1 ulp = 2u relative each.  The product
  x * log2(e) is rounded (u relative) with a rounded constant (u/2 relative): 1.5 u |x log2 e| absolute in the exponent, i.e.
  ln 2 * 1.5 u |x| log2 e = 1.5 u |x| relative in the result.  So  e~ = exp(-x) (1 + eps),  |eps| <= u (2 + 2 |x|)  (rounded up).
    sigma = 1 / (1 + e): d sigma / d e * e = -sigma (1 - sigma), then the sum 1 + e (u relative) and the reciprocal (2u relative):
        a_sigma(x) = u [ sigma (1 - sigma) (2 + 2 |x|) + 3 sigma ]          (<= 4 u: |x| sigma (1 - sigma) <= 0.23)
    tanh t = (1 - e) / (1 + e), e = exp(-2 |x|), |eps| <= u (2 + 4 |x|): d t / d e * e = -(1 - t^2) / 2, then 1 - e, 1 + e, the product
    (u each) and the reciprocal (2u), all relative to t:
        a_tanh(x) = u [ (1 - t^2) / 2 * (2 + 4 |x|) + 5 |t| ]               (<= 7 u: |x| (1 - t^2) <= 0.45)
  The error grows with |x| while the function flattens: the product stays bounded, which is what the saturating regime exercises.
  exp(-x) = inf (x < -88) gives 1 / inf = 0 and a flushed exp(-x) gives 1: both within TINY = 2^-126 of the true value.

  Forward, per element:
      dg = slope * dz_pre + a       slope = 1/4 (sigma), 1 (tanh): the largest derivative
      dc = dg_f |c_prev| + dg_i + dg_j + 4 u (|g_f c_prev| + |g_i g_j|)      (|g_i|, |g_j| <= 1; two products and a sum)
      dh = 1/2 ulp_bf16(h_ref) + dg_o + dc + a_tanh(c_ref) + u |h_ref|       (|g_o|, |tanh c| <= 1, tanh' <= 1; the product)
  The half ulp is the storage rounding, round to nearest: truncation is a whole ulp and does not fit.

  Backward, per element (gates, cell, dz of the next step and dhout are the device's own values, exact operands of both sides):
      d(dh)  = (4U + 2) u (|dhout| + sum |Wh| |dz_next|)
      q = 1 - tc^2:  dq = 2 |tc| a_tanh(c) + 2 u
      l = dh g_o q:  dl = d(dh) g_o q + |dh| g_o dq + 3 u |l|
      dc = carry + l:  d(dc) = e + dl + u (|carry| + |l|),   e the running bound of the fp32 carry chain:  e <- d(dc) g_f + u |dc g_f|
      d(dz_o) = d(dh) |tc g_o (1 - g_o)| + |dh| a_tanh(c) g_o (1 - g_o) + 5 u |dz_o|
      d(dz_i) = d(dc) |g_j g_i (1 - g_i)| + 5 u |dz_i|
      d(dz_j) = d(dc) g_i (1 - g_j^2) + |dc| g_i 2 u + 4 u |dz_j|
      d(dz_f) = d(dc) |c_prev g_f (1 - g_f)| + 5 u |dz_f|
  each + 1/2 ulp_bf16(dz_ref) + TINY.

No element is excluded from any comparison.  Frames at or past a sample's length: hout and dz are bit-zero; gates and cell there are
unspecified and not read."""
import numpy as np

U32 = 2.0 ** -24
TINY = 2.0 ** -126


# ------------------------------------------------------------------------------------------------ number formats
def bf16_round(a):
    """float32 -> nearest-even bf16, returned as float32 (finite inputs)."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    return (b.astype(np.uint32) << 16).view(np.float32).reshape(np.shape(a))


def bf16_trunc(a):
    b = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return b.view(np.float32).reshape(np.shape(a))


def half_ulp_bf16(ref):
    """Half the spacing of bf16 (8 significant bits) at |ref|: 2^(floor(log2 |ref|) - 8)."""
    m = np.maximum(np.abs(np.asarray(ref, np.float64)), TINY)
    return np.exp2(np.floor(np.log2(m)) - 8.0)


def bit_zero(a):
    a = np.asarray(a)
    return (a == 0) & ~np.signbit(a)


# ------------------------------------------------------------------------------------------------ activations and their accuracy
def sigmoid64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def a_sigmoid(x, s):
    return U32 * (s * (1.0 - s) * (2.0 + 2.0 * np.abs(x)) + 3.0 * s) + TINY


def a_tanh(x, t):
    return U32 * ((1.0 - t * t) * 0.5 * (2.0 + 4.0 * np.abs(x)) + 5.0 * np.abs(t)) + TINY


# ------------------------------------------------------------------------------------------------ layouts
def packed_columns(U):
    """p[g, u] = packed column of (gate g, unit u)."""
    u = np.arange(U)
    return (u // 16)[None, :] * 64 + np.arange(4)[:, None] * 16 + (u % 16)[None, :]


def unpack_gate_columns(a, U):
    """[..., 4U] packed -> [..., 4, U] master."""
    return np.asarray(a)[..., packed_columns(U)]


def pack_gate_columns(a, U):
    """[..., 4, U] master -> [..., 4U] packed."""
    out = np.empty(a.shape[:-2] + (4 * U,), a.dtype)
    out[..., packed_columns(U)] = a
    return out


def clamped_lengths(seq_len, T):
    return np.clip(np.asarray(seq_len, np.int64), 0, T)


class Worst:
    """Worst |dev - ref| / bound of one tensor and where it occurred."""

    def __init__(self, name):
        self.name, self.ratio, self.where, self.err, self.bound, self.count = name, 0.0, None, 0.0, 0.0, 0

    def add(self, dev, ref, bound, locate):
        err = np.abs(np.asarray(dev, np.float64) - ref)
        r = np.where(np.isfinite(err), err / bound, np.inf)     # a NaN / Inf on the device is the worst possible answer, not a skipped element
        if r.size == 0:
            return
        self.count += r.size
        k = int(np.argmax(r))
        if r.flat[k] > self.ratio:
            self.ratio, self.err, self.bound = float(r.flat[k]), float(err.flat[k]), float(np.asarray(bound).flat[k])
            self.where = locate(np.unravel_index(k, r.shape))

    def flag(self, bad, locate):
        """Elements that must hold an exact value and do not: ratio inf."""
        self.count += bad.size
        if bad.any():
            self.ratio = float('inf')
            self.where = locate(np.unravel_index(int(np.argmax(bad)), bad.shape))

    def __repr__(self):
        return '%s: ratio %.4g (err %.3g, bound %.3g) at %s over %d elements' % (self.name, self.ratio, self.err, self.bound, self.where, self.count)


def report(res):
    return '; '.join(repr(res[k]) for k in sorted(res) if isinstance(res[k], Worst))


# ------------------------------------------------------------------------------------------------ forward
def forward_check(Wh, seq_len, N, T, U, hout, gates, cell, forget_bias, xproj=None, x=None, Wx=None, b=None, ndir=2):
    """-> dict(gates=Worst, cell=Worst, h=Worst, pad_h=Worst, sat_fraction=, max_abs_z=).  Either xproj (the device's projection tensor,
    K = U) or x, Wx, b (the fused-projection kernel: K = D + U)."""
    ND = ndir
    lens = clamped_lengths(seq_len, T)
    hout = np.asarray(hout, np.float32).reshape(N, T, ND, U)
    gates = unpack_gate_columns(np.asarray(gates, np.float32).reshape(ND, N, T, 4 * U), U)          # [ND, N, T, 4, U]
    cell = np.asarray(cell, np.float32).reshape(ND, N, T, U)
    if xproj is not None:
        xp = unpack_gate_columns(np.asarray(xproj, np.float32).reshape(N, T, ND, 4 * U), U)         # [N, T, ND, 4, U]
        K = U
    else:
        x = np.asarray(x, np.float64).reshape(N, T, -1)
        K = x.shape[-1] + U
    res = {k: Worst(k) for k in ('gates', 'cell', 'h', 'pad_h')}
    fb = np.zeros((4, 1)); fb[2] = forget_bias
    nsig = nsat = 0
    zmax = 0.0
    for d in range(ND):
        W = np.asarray(Wh[d], np.float64); Wa = np.abs(W)
        for s in range(T):
            idx = np.nonzero(lens > s)[0]
            if idx.size == 0:
                break
            t = s if d == 0 else lens[idx] - 1 - s
            tp = t - 1 if d == 0 else t + 1
            n = idx.size
            if s > 0:
                hp = hout[idx, tp, d].astype(np.float64)
                cp = cell[d, idx, tp].astype(np.float64)
            else:
                hp = np.zeros((n, U)); cp = np.zeros((n, U))
            if xproj is not None:
                z0 = xp[idx, t, d].astype(np.float64).reshape(n, 4 * U)
                m0 = np.abs(z0)
            else:
                xr = x[idx, t]
                z0 = xr @ np.asarray(Wx[d], np.float64) + np.asarray(b[d], np.float64)
                m0 = np.abs(xr) @ np.abs(np.asarray(Wx[d], np.float64)) + np.abs(np.asarray(b[d], np.float64))
            z = (z0 + hp @ W).reshape(n, 4, U) + fb
            mag = (m0 + np.abs(hp) @ Wa).reshape(n, 4, U) + np.abs(fb)
            dzp = (K + 2) * U32 * mag
            gi, gf, go = sigmoid64(z[:, 0]), sigmoid64(z[:, 2]), sigmoid64(z[:, 3])
            gj = np.tanh(z[:, 1])
            g_ref = np.stack([gi, gj, gf, go], 1)
            dg = np.stack([0.25 * dzp[:, 0] + a_sigmoid(z[:, 0], gi), dzp[:, 1] + a_tanh(z[:, 1], gj),
                           0.25 * dzp[:, 2] + a_sigmoid(z[:, 2], gf), 0.25 * dzp[:, 3] + a_sigmoid(z[:, 3], go)], 1)
            c_ref = gf * cp + gi * gj
            dc = dg[:, 2] * np.abs(cp) + dg[:, 0] + dg[:, 1] + 4 * U32 * (np.abs(gf * cp) + np.abs(gi * gj)) + TINY
            tc = np.tanh(c_ref)
            h_ref = go * tc
            dh = half_ulp_bf16(h_ref) + dg[:, 3] + dc + a_tanh(c_ref, tc) + U32 * np.abs(h_ref)
            res['gates'].add(gates[d, idx, t], g_ref, dg, lambda k: dict(n=int(idx[k[0]]), s=s, d=d, g='ijfo'[k[1]], u=int(k[2])))
            res['cell'].add(cell[d, idx, t], c_ref, dc, lambda k: dict(n=int(idx[k[0]]), s=s, d=d, u=int(k[1])))
            res['h'].add(hout[idx, t, d], h_ref, dh, lambda k: dict(n=int(idx[k[0]]), s=s, d=d, u=int(k[1])))
            sig = np.stack([gi, gf, go])
            nsig += sig.size
            nsat += int(((sig < 1e-3) | (sig > 1 - 1e-3)).sum())
            zmax = max(zmax, float(np.abs(z).max()))
    pad = np.arange(T)[None, :] >= lens[:, None]                                                    # [N, T]
    res['pad_h'].flag(~bit_zero(hout[pad]), lambda k: ('padding row', int(k[0])))
    res['sat_fraction'] = nsat / max(nsig, 1)
    res['max_abs_z'] = zmax
    return res


# ------------------------------------------------------------------------------------------------ backward
def backward_check(Wh, seq_len, N, T, U, dhout, gates, cell, dz, dc_state=None, ndir=2):
    """-> dict(dz=Worst, pad_dz=Worst[, dc_state=Worst]).  dc_state [ND, N, U]: the per-step kernels' carry after the call for step 0."""
    ND = ndir
    lens = clamped_lengths(seq_len, T)
    dhout = np.asarray(dhout, np.float32).reshape(N, T, ND, U)
    gates = unpack_gate_columns(np.asarray(gates, np.float32).reshape(ND, N, T, 4 * U), U)
    cell = np.asarray(cell, np.float32).reshape(ND, N, T, U)
    dz = np.asarray(dz, np.float32).reshape(N, T, ND, 4, U)
    res = {k: Worst(k) for k in ('dz', 'pad_dz')}
    if dc_state is not None:
        res['dc_state'] = Worst('dc_state')
        dc_state = np.asarray(dc_state, np.float32).reshape(ND, N, U)
    for d in range(ND):
        W = np.asarray(Wh[d], np.float64); Wa = np.abs(W)                                            # [U, 4U]
        carry = np.zeros((N, U)); e = np.zeros((N, U))
        for s in range(T - 1, -1, -1):
            idx = np.nonzero(lens > s)[0]
            if idx.size == 0:
                continue
            n = idx.size
            t = np.full(n, s) if d == 0 else lens[idx] - 1 - s
            has_next = lens[idx] > s + 1
            tn = np.where(has_next, t + 1 if d == 0 else t - 1, 0)
            zn = dz[idx, tn, d].astype(np.float64).reshape(n, 4 * U) * has_next[:, None]
            dho = dhout[idx, t, d].astype(np.float64)
            dh = dho + zn @ W.T
            ddh = (4 * U + 2) * U32 * (np.abs(dho) + np.abs(zn) @ Wa.T)
            g = gates[d, idx, t].astype(np.float64)
            gi, gj, gf, go = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
            c = cell[d, idx, t].astype(np.float64)
            cp = cell[d, idx, t - 1 if d == 0 else t + 1].astype(np.float64) if s > 0 else np.zeros((n, U))
            tc = np.tanh(c); at = a_tanh(c, tc)
            q = 1.0 - tc * tc; dq = 2 * np.abs(tc) * at + 2 * U32
            loc = dh * go * q
            dl = ddh * np.abs(go) * q + np.abs(dh * go) * dq + 3 * U32 * np.abs(loc)
            dc = carry[idx] + loc
            ddc = e[idx] + dl + U32 * (np.abs(carry[idx]) + np.abs(loc))
            ref = np.stack([dc * gj * gi * (1 - gi), dc * gi * (1 - gj * gj), dc * cp * gf * (1 - gf), dh * tc * go * (1 - go)], 1)
            bnd = np.stack([ddc * np.abs(gj * gi * (1 - gi)) + 5 * U32 * np.abs(ref[:, 0]),
                            ddc * np.abs(gi * (1 - gj * gj)) + np.abs(dc * gi) * 2 * U32 + 4 * U32 * np.abs(ref[:, 1]),
                            ddc * np.abs(cp * gf * (1 - gf)) + 5 * U32 * np.abs(ref[:, 2]),
                            ddh * np.abs(tc * go * (1 - go)) + np.abs(dh) * at * np.abs(go * (1 - go)) + 5 * U32 * np.abs(ref[:, 3])], 1)
            bnd = bnd + half_ulp_bf16(ref) + TINY
            res['dz'].add(dz[idx, t, d], ref, bnd, lambda k: dict(n=int(idx[k[0]]), s=s, d=d, g='ijfo'[k[1]], u=int(k[2])))
            carry[idx] = dc * gf
            e[idx] = ddc * np.abs(gf) + U32 * np.abs(carry[idx])
        if dc_state is not None:
            live = np.nonzero(lens > 0)[0]
            res['dc_state'].add(dc_state[d, live], carry[live], e[live] + TINY, lambda k: dict(n=int(live[k[0]]), d=d, u=int(k[1])))
            res['dc_state'].flag(~bit_zero(dc_state[d, lens == 0]), lambda k: ('dc_state of an empty sample', d, int(k[0])))
    pad = np.arange(T)[None, :] >= lens[:, None]
    res['pad_dz'].flag(~bit_zero(dz[pad]), lambda k: ('padding row', int(k[0])))
    return res


# ------------------------------------------------------------------------------------------------ lstm_hprev
def hprev_reference(hout, seq_len, N, T, U, ndir=2):
    """[ND, R, U]: the hout row of the step before (n, t) in direction d's own order; zero at a sample's first step and past its length."""
    lens = clamped_lengths(seq_len, T)
    h = np.asarray(hout).reshape(N, T, ndir, U)
    out = np.zeros((ndir, N, T, U), h.dtype)
    for n in range(N):
        L = int(lens[n])
        if L > 1:
            out[0, n, 1:L] = h[n, 0:L - 1, 0]
            if ndir > 1:
                out[1, n, 0:L - 1] = h[n, 1:L, 1]
    return out.reshape(ndir, N * T, U)


# ------------------------------------------------------------------------------------------------ inputs of the value regimes
REGIMES = ('small', 'trained', 'saturating')


def make_case(regime, N, T, D, U, seed=1):
    """-> x [N, T, D], Ws[d] [D + U, 4U], bs[d] [4U], dh [N, T, 2U]: float32, x / Ws / dh bf16-representable, all finite.
      small       what the kernel tests have always used: weights uniform +-0.08, inputs +-1: pre-activations of ~0.6, no gate saturates
      trained     the committed checkpoint's BiLSTM (logits/fw, logits/bw; D = 512, U = 256), non-negative inputs (conv5 ends in a ReLU)
      saturating  weights scaled so that the input part of z has a standard deviation of ~7.2 and the recurrent part up to ~7.5
                  (uniform +-21.6 / sqrt(D) and +-13 / sqrt(U)), biases +-1.2: |z| reaches 20 .. 60, a third of the gates sit on a rail"""
    rng = np.random.RandomState(seed)
    uni = lambda shape, a: rng.uniform(-a, a, shape).astype(np.float32)
    x = uni((N, T, D), 1.0)
    if regime == 'small':
        Ws = [uni((D + U, 4 * U), 0.08) for _ in range(2)]
        bs = [uni((4 * U,), 0.1) for _ in range(2)]
    elif regime == 'saturating':
        Ws = [np.concatenate([uni((D, 4 * U), 21.6 / np.sqrt(D)), uni((U, 4 * U), 13.0 / np.sqrt(U))]) for _ in range(2)]
        bs = [uni((4 * U,), 1.2) for _ in range(2)]
    elif regime == 'trained':
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
        import make_trained_fixture as fx
        w = fx.load_weights()
        assert (D, U) == (512, 256) and w['logits/fw/weights'].shape == (D + U, 4 * U)
        Ws = [w['logits/%s/weights' % k].astype(np.float32) for k in ('fw', 'bw')]
        bs = [w['logits/%s/biases' % k].astype(np.float32) for k in ('fw', 'bw')]
        x = np.abs(x)
    else:
        raise ValueError(regime)
    dh = uni((N, T, 2 * U), 1.0)
    return bf16_round(x), [bf16_round(w) for w in Ws], bs, bf16_round(dh)


def length_vector(kind, N, T, seed=1):
    """'full': all T;  'random': uniform in [1, T];  'edges': 0, 1, T and T + 5 in it (the kernels clamp a length to T)."""
    rng = np.random.RandomState(seed)
    if kind == 'full':
        return [T] * N
    lens = rng.randint(1, T + 1, N)
    if kind == 'edges':
        for k, v in enumerate((T + 5, 0, 1, T)):
            lens[(k * 5) % N if N >= 16 else k % N] = v
    return lens.tolist()
