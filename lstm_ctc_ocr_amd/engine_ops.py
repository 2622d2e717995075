"""The operators Engine._lower strings together: per layer kind one class that owns its packed weights, allocates its buffers in a
ShapePlan (alloc), and issues its forward / backward kernels (fwd / bwd).  Every plan-time decision (which fusion, which workspace) is
taken ONCE, in alloc, and recorded in the plan; fwd and bwd only read the record.  The convolution families are separate classes
(_Conv1Op, _Conv3x3Op, _Conv1x1Op, _ConvFullOp) over a base that owns the batch-norm stage."""
import os

import numpy as np
import torch

from . import ops

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
BN_EPS = 1e-3            # tf.contrib.layers.batch_norm default (reference network.py:176-178)


# ====================================================================================================== environment switches
def _env(name, default=None):
    """The one place the engine reads its environment (the table of the variables: engine.py)."""
    return os.environ.get(name, default)


def _switch(name, default=True):
    return _env(name, '1' if default else '0') != '0'


def _number(name, default, kind=int):
    return kind(_env(name, default))


# ====================================================================================================== ops
def _take_ring(sp, key):
    """True once per fill: the hand-off block `key` still holds the all-ones pattern the conv1 + pool launch of THIS forward pass wrote.
    The persistent LSTM launch that asks consumes it — a second launch on the same block (a repeated backward pass without a new
    training forward) gets False and fills the block itself."""
    if key not in sp.rings_ready:
        return False
    sp.rings_ready.discard(key)
    return True


class _Op(object):
    mask_in_consumer = False      # True: output has a fused ReLU whose backward the consumer must apply

    def __init__(self, eng, node, prev):
        self.eng, self.node, self.prev, self.name = eng, node, prev, node.name
        self.key = node.name          # buffer key; made unique by Engine._lower (the reference reuses layer names)
        self.inputs = [prev]
        self.consumers = 0            # how many ops read this op's output (residual graphs: > 1)

    def grad_owner(self):             # the op whose dy buffer really receives gradients for this output (views forward it)
        return self

    def out_shape(self, in_shape):
        raise NotImplementedError

    def alloc(self, sp, in_shape):
        pass

    def refresh(self):            # re-pack work that is not expressible as a pack job
        pass

    def pack_jobs(self):          # bf16 operand re-packs after a parameter update (executed by ONE launch)
        return []

    def shadow_params(self):      # variables whose plain bf16 copy (same layout, Engine.shadow) this op reads
        return []

    def fwd(self, sp):
        pass

    def bwd(self, sp):
        pass

    # gradient w.r.t. this op's output (written by the consumer)
    def y(self, sp):
        return sp.buf[self.key + '/y']

    def dy(self, sp):
        return sp.buf[self.key + '/dy']


class _InputOp(_Op):
    def __init__(self, eng):
        self.eng, self.name, self.prev, self.node = eng, 'data', None, None
        self.key = 'data'
        self.inputs, self.consumers = [], 0

    def dy_needed(self):
        return False

    def y(self, sp):
        return sp.x

    def dy(self, sp):
        return None


def _bnbwd_rows_allowed(p):
    """The ONE statement of the rule "partial rows XOR pooled-gradient routing": may the data-gradient kernel of producer p's only consumer
    take p's batch-norm BACKWARD sums (partial rows into p's workspace)?  Only for a batch-norm + ReLU convolution whose gradient is not
    spoken for otherwise — a producer with bn_pool routes a pooled gradient inside its own backward passes, and ocr_bn_train_bwd2 takes
    one form per launch, never both."""
    return (isinstance(p, _ConvOp) and p.bn and p.relu and p.consumers == 1 and p.tail_into is None and p.mask_from is None
            and p.bn_pool is None and p.kind != 'c1')


class _ConvOp(_Op):
    """What the four convolution families share: the attributes, the output / gradient / batch-norm buffers and the batch-norm stage with
    its cross-op links.  A family adds its kernels as _conv_fwd / _conv_bwd.  The op itself always runs at stride 1; Engine._lower appends
    a _SubsampleOp (a strided convolution is the stride-1 convolution evaluated at every s-th position)."""
    kind = None                # 'c1' | '3x3' | '1x1' | 'full': fixed per class (read by Engine._lower and by tools)

    def __init__(self, eng, node, prev):
        super(_ConvOp, self).__init__(eng, node, prev)
        a = node.attrs
        self.kh, self.kw, self.co, self.ci = a['k_h'], a['k_w'], a['c_o'], a['c_i']
        self.bn, self.relu, self.biased, self.padding = a['bn'], a['relu'], a['biased'], a['padding']
        self.mask_in_consumer = self.relu and not self.bn

    def dy_needed(self):
        return True

    def out_shape(self, s):
        return (s[0], s[1], s[2], self.co)

    fused_pool = None          # set by Engine._lower: conv1 + ReLU + 2x2 max-pool run as one kernel, no full-res activation
    tail_into = None           # set by Engine._lower: (add op, the add's other input) — this conv's batch-norm apply pass also does the
                               # residual add + relu and writes the add's output (the add's forward is then a no-op)
    mask_from = None           # set by Engine._lower: the fused add + relu that is this (BN, no ReLU) conv's only consumer: its batch-norm
                               # backward reads the add's gradient and applies the add's ReLU mask itself (no masked copy pass)
    bn_pool = None             # set by Engine._lower: the 1 x 2 max-pool that is this batch-norm layer's only consumer (written by the BN apply
                               # pass; its gradient is routed inside the BN backward passes)
    pool_after = None          # set by Engine._lower: the max-pool that follows this 3x3 conv + ReLU; where the shape allows, the conv's
                               # epilogue writes the pooled tensor too

    def _code_windows(self, sp, s, o):
        """Pooled outputs whose routing codes a training forward pass writes INSTEAD of the full-resolution y (0: keep y)."""
        return o[0] * o[1] * o[2] // 2 if self.bn_pool is not None else 0

    def _stats_rows(self, sp, s):
        """Partial statistics rows the convolution's own epilogue leaves in the batch-norm workspace (0: a statistics pass over z)."""
        return 0

    def alloc(self, sp, s):
        o = self.out_shape(s)
        dev = self.eng.device
        sp.shape[self.key] = (s, o)
        # A max-pool that is this layer's only consumer (bn_pool: behind the batch norm; pool_after: written by the convolution's epilogue): a
        # training forward pass writes the pool's routing codes (4 bits per pooled output: which element of the window won, and its ReLU
        # bit — conv1's format) instead of the full-resolution y, whose only readers were backward passes looking for exactly that
        # (OCR_POOL_CODES=0: keep y).  No y buffer then: an inference forward on this plan allocates it on first use (_ConvOp.y).
        windows = self._code_windows(sp, s, o) if _switch('OCR_POOL_CODES') else 0
        if windows:
            sp.buf[self.key + '/pool_codes'] = torch.empty((windows, self.co // 8), dtype=torch.int32, device=dev)
        else:
            sp.buf[self.key + '/y'] = torch.empty(o, dtype=BF16, device=dev)
        sp.buf[self.key + '/dy'] = torch.empty(o, dtype=BF16, device=dev)
        if self.bn:
            sp.buf[self.key + '/z'] = torch.empty(o, dtype=BF16, device=dev)
            sp.buf[self.key + '/dz'] = torch.empty(o, dtype=BF16, device=dev)
            sp.buf[self.key + '/mean'] = torch.empty(self.co, dtype=F32, device=dev)
            sp.buf[self.key + '/rstd'] = torch.empty(self.co, dtype=F32, device=dev)
            sp.buf[self.key + '/bnws'] = ops.bn_workspace(o[0] * o[1] * o[2], self.co, dev)
            sp.bn_stat_rows[self.key] = self._stats_rows(sp, s)

    def y(self, sp):
        t = sp.buf.get(self.key + '/y')
        if t is None:       # a plan whose training steps keep routing codes instead (alloc): an inference forward is the first to need it
            t = sp.buf[self.key + '/y'] = torch.empty(sp.shape[self.key][1], dtype=BF16, device=self.eng.device)
        return t

    def pack_jobs(self):
        w = self.eng.param(self.name + '/weights')
        return [dict(type=0, R=self.kh * self.kw * self.ci, Cc=self.co, ldin=self.co, src=w, dst=self.wpack)]

    def fwd(self, sp):
        codes = sp.buf.get(self.key + '/pool_codes') if self.eng.training else None
        y = None if codes is not None else self.y(sp)
        bias = self.eng.param(self.name + '/biases') if self.biased else None
        self._conv_fwd(sp, self.prev.y(sp), sp.buf[self.key + '/z'] if self.bn else y, bias, codes)
        if self.bn:
            self._bn_fwd(sp, y, codes)

    def bwd(self, sp):
        e = self.eng
        x = self.prev.y(sp)
        dz = self._bn_bwd(sp) if self.bn else self.dy(sp)       # (dy: already ReLU-masked by the consumer unless this layer has BN)
        self._conv_bwd(sp, x, dz, e.grad(self.name + '/weights'), e.grad(self.name + '/biases') if self.biased else None)

    def _bn_fwd(self, sp, y, codes):
        e, o = self.eng, sp.shape[self.key][1]
        M = o[0] * o[1] * o[2]
        res, relu = None, self.relu
        if self.tail_into is not None:          # y_add = relu(bf16(bn(z)) + other input): written straight into the add's buffer
            add, other = self.tail_into
            y, res, relu = add.y(sp), other.y(sp).view(M, self.co), True
        pooled = self.bn_pool.y(sp).view(M // 2, self.co) if self.bn_pool is not None else None
        ops.bn_train_fwd(sp.buf[self.key + '/z'].view(M, self.co), e.param('%s/%s/gamma' % (self.name, self.name)),
                         e.param('%s/%s/beta' % (self.name, self.name)), BN_EPS, relu,
                         sp.buf[self.key + '/bnws'], out=None if y is None else y.view(M, self.co),
                         save_mean=sp.buf[self.key + '/mean'], save_rstd=sp.buf[self.key + '/rstd'], residual=res,
                         partial_rows=sp.bn_stat_rows[self.key], pooled=pooled, codes=codes)

    def _bn_bwd(self, sp):
        """dz from dy (or from what stands in for it: the add's gradient, the pooled gradient); returns dz."""
        e, o = self.eng, sp.shape[self.key][1]
        M = o[0] * o[1] * o[2]
        dy, dz = self.dy(sp), sp.buf[self.key + '/dz']
        codes = sp.buf.get(self.key + '/pool_codes')
        ymask, relu = (self.y(sp) if codes is None else None), self.relu
        if self.mask_from is not None:          # gradient and ReLU mask straight from the residual add + relu behind this layer
            dy, ymask, relu = self.mask_from.dy(sp), self.mask_from.y(sp), True
        dy2 = dy.view(M, self.co)
        if self.bn_pool is not None:            # the pooled gradient, routed by the passes themselves
            dy2 = self.bn_pool.dy(sp).view(M // 2, self.co)
        colsrc = sp.col_bn.get(self.key)
        if colsrc is not None:                  # ... and formed by the statistics pass itself from the column matrix of the full-height
            col, Nb, W, HC = colsrc             # convolution behind the pool (_ConvFullOp._conv_bwd left its col2im out)
            ops.bn_train_bwd_codes_col(sp.buf[self.key + '/z'].view(M, self.co), codes, col, Nb, W, HC, dy2,
                                       e.param('%s/%s/gamma' % (self.name, self.name)), sp.buf[self.key + '/mean'],
                                       sp.buf[self.key + '/rstd'], e.grad('%s/%s/gamma' % (self.name, self.name)),
                                       e.grad('%s/%s/beta' % (self.name, self.name)), relu, sp.buf[self.key + '/bnws'], out=dz.view(M, self.co))
            return dz
        ops.bn_train_bwd(sp.buf[self.key + '/z'].view(M, self.co), None if ymask is None else ymask.view(M, self.co), dy2,
                         e.param('%s/%s/gamma' % (self.name, self.name)), sp.buf[self.key + '/mean'],
                         sp.buf[self.key + '/rstd'], e.grad('%s/%s/gamma' % (self.name, self.name)),
                         e.grad('%s/%s/beta' % (self.name, self.name)), relu, sp.buf[self.key + '/bnws'],
                         out=dz.view(M, self.co), pooled_dy=self.bn_pool is not None,
                         partial_rows=sp.bn_bwd_rows.get(self.key, 0), codes=codes)
        return dz


class _Conv1Op(_ConvOp):
    """The single-channel first layer, with or without its fused 2x2 max-pool (fused_pool)."""
    kind = 'c1'

    def __init__(self, eng, node, prev):
        super(_Conv1Op, self).__init__(eng, node, prev)
        if (self.kh, self.kw, self.padding) != (3, 3, 'SAME') or self.co != 64 or self.bn or not self.biased:
            raise NotImplementedError('%s: the single-channel input conv is lowered for 3x3 SAME, 64 filters' % self.name)

    def pack_jobs(self):
        return []

    def alloc(self, sp, s):
        if self.fused_pool is None:
            return super(_Conv1Op, self).alloc(sp, s)
        dev = self.eng.device
        sp.shape[self.key] = (s, self.out_shape(s))
        if self.eng.defer_w9 and _switch('OCR_CONV1_SLAB'):
            # the backward kernel's per-block partial sums (no atomics); two jobs of the merged slab reduction add them
            sp.buf[self.key + '/slab'] = torch.empty((ops.conv1_pool_bwd_slab_rows(s[0], s[1], s[2]), 640), dtype=F32, device=dev)
        if _switch('OCR_CONV1_CODES'):
            # pool routing + ReLU bits saved by the training forward pass (4 bits per pooled output) for the backward pass
            sp.buf[self.key + '/codes'] = torch.empty((s[0] * (s[1] // 2) * (s[2] // 2), 8), dtype=torch.int32, device=dev)

    def _conv_fwd(self, sp, x, out, bias, codes):
        ops.conv1_fwd(x, self.eng.param(self.name + '/weights'), bias, relu=self.relu, out=out)

    def _conv_bwd(self, sp, x, dz, dw, db):
        ops.conv1_wgrad(x, dz, dw, db)

    def fwd(self, sp):
        if self.fused_pool is None:
            return super(_Conv1Op, self).fwd(sp)
        e = self.eng
        zero, e._zero_pending = (e.grads if e._zero_pending else None), False     # the gradient buffer's clear rides on this launch
        codes = sp.buf.get(self.key + '/codes') if e.training else None
        ones, e._ones_pending = e._ones_pending, None                              # ... and so does the fill of the LSTM hand-off blocks
        ops.conv1_pool_fwd(self.prev.y(sp), e.param(self.name + '/weights'), e.param(self.name + '/biases'), out=self.fused_pool.y(sp),
                           zero=zero, codes=codes, ones=ones)
        # every hand-off block of the plan is armed now; each persistent launch consumes (and thereby dirties) its own block ONCE
        sp.rings_ready = set(sp.lstm_sync_keys) if ones is not None else set()
        sp.rings_armed = ones is not None         # (what the last forward pass did; rings_ready is consumed by the launches)

    def bwd(self, sp):
        if self.fused_pool is None:
            return super(_Conv1Op, self).bwd(sp)
        # pool routing + ReLU mask + weight gradient in one recomputing pass
        e = self.eng
        x, w, b, dp = self.prev.y(sp), e.param(self.name + '/weights'), e.param(self.name + '/biases'), self.fused_pool.dy(sp)
        codes = sp.buf.get(self.key + '/codes')
        slab = sp.buf.get(self.key + '/slab')
        if slab is None:
            ops.conv1_pool_bwd(x, w, b, dp, e.grad(self.name + '/weights'), e.grad(self.name + '/biases'), codes=codes)
            return
        ops.conv1_pool_bwd_slab(x, w, b, dp, slab, codes=codes)
        for dst, off, n4 in ((e.grad(self.name + '/weights'), 0, 144), (e.grad(self.name + '/biases'), 576, 16)):
            job = np.zeros(1, dtype=e.W9_JOB_DTYPE)
            job['dw'], job['part'], job['n4'], job['slab4'] = dst.data_ptr(), slab.data_ptr() + 4 * off, n4, 160
            job['S'], job['rows'], job['Cout'] = slab.shape[0], 8, 64
            sp.w9_pending.append((job.tobytes(), (n4 + 31) // 32))          # 256 / rows = 32 float4 columns per block


class _Conv3x3Op(_ConvOp):
    """The MFMA 3x3 SAME convolutions with their epilogue fusions (max-pool, pool codes, batch-norm statistics; the data gradient with the
    producer's batch-norm backward sums) and the slab weight gradient with its deferred reduction."""
    kind = '3x3'

    def __init__(self, eng, node, prev):
        super(_Conv3x3Op, self).__init__(eng, node, prev)
        if self.ci % 32 or self.co % 8:
            raise NotImplementedError('%s: 3x3 conv needs C_in %% 32 == 0 and C_out %% 8 == 0' % self.name)
        self.wpack = torch.empty((self.co, 9 * self.ci), dtype=BF16, device=eng.device)
        if prev.dy_needed():        # (absent, not None, where no data gradient is computed: hasattr(op, 'wdgrad') is the test)
            self.wdgrad = torch.empty((self.ci, 9 * self.co), dtype=BF16, device=eng.device)

    def pack_jobs(self):
        jobs = super(_Conv3x3Op, self).pack_jobs()
        if hasattr(self, 'wdgrad'):
            w = self.eng.param(self.name + '/weights')
            jobs.append(dict(type=1, R=self.ci, Cc=self.co, src=w, dst=self.wdgrad, n=w.numel()))
        return jobs

    def _code_windows(self, sp, s, o):
        p = self.pool_after
        if (p is not None and p.key in sp.fused_pools
                and ops.conv3x3_pool_codes_supported(s[0], s[1], s[2], self.ci, self.co, p.kw_t, p.kh_f)):
            return o[0] * (o[1] // p.kw_t) * (o[2] // p.kh_f)
        return super(_Conv3x3Op, self)._code_windows(sp, s, o)

    def _stats_rows(self, sp, s):
        # from the convolution's own epilogue where a plane-layout kernel takes the shape (partial rows into the BN workspace: it must hold them)
        if not self.eng.fuse_bn_stats:
            return 0
        rows = ops.conv3x3_stats_rows(s[0], s[1], s[2], self.ci, self.co, bias=self.biased)
        return rows if rows * 2 * self.co * 4 <= sp.buf[self.key + '/bnws'].numel() - 2 * self.co * 8 else 0

    def alloc(self, sp, s):
        e, dev, p = self.eng, self.eng.device, self.pool_after
        if p is not None and ops.conv3x3_pool_supported(s[0], s[1], s[2], self.ci, self.co, p.kw_t, p.kh_f):
            sp.fused_pools.add(p.key)           # this plan's launch of the layer writes the pooled tensor too
        super(_Conv3x3Op, self).alloc(sp, s)
        p = self.prev
        if hasattr(self, 'wdgrad') and e.fuse_bn_stats and _switch('OCR_FUSE_BN_BWD') and _bnbwd_rows_allowed(p):
            # the producer is a batch-norm + ReLU convolution feeding only this one: its batch-norm BACKWARD sums (and its ReLU mask) are
            # taken by this layer's data-gradient kernel (conv_k3's write-out), where a plane-layout kernel takes the shape
            rows = ops.conv3x3_bnbwd_rows(s[0], s[1], s[2], self.co, self.ci)
            sp.bn_bwd_rows[p.key] = rows if rows * 2 * self.ci * 4 <= sp.buf[p.key + '/bnws'].numel() - 2 * self.ci * 8 else 0
        if (hasattr(self, 'wdgrad') and _switch('OCR_FUSE_UNPOOL') and isinstance(p, _PoolOp) and p.consumers == 1
                and getattr(p.prev, 'pool_after', None) is p and p.key in sp.fused_pools and p.prev.key + '/pool_codes' in sp.buf
                and ops.conv3x3_unpool_supported(s[0], s[1], s[2], self.co, self.ci, p.kw_t, p.kh_f)
                and ops.conv3x3_kernel_choice(s[0], s[1], s[2], self.co, self.ci, bias=False, relu=False) in ('conv_k3/A', 'conv_k3/D')):
            # the producer is a max-pool whose own producer saved routing codes, and the plain data gradient runs an aligned-width conv_k3
            # kernel: that kernel's unpool write-out scatters the gradient straight into the gradient of the pool's INPUT (the same bits as the
            # pooled gradient + maxpool_bwd_codes) — the pool's backward is a no-op in this plan and its gradient buffer does not exist
            sp.unpool_pools.add(p.key)
            del sp.buf[p.key + '/dy']
        # scratch of the slab weight-gradient kernel
        need = ops.conv3x3_wgrad_workspace_bytes(s[0], s[1], s[2], self.ci, self.co)
        have = sp.buf.get('wgrad_ws')
        if need and e.defer_w9:
            # one buffer PER LAYER: the slabs stay until the end of the backward pass, where ONE launch reduces all layers'
            # (Engine._flush_w9) — ~20 MB per layer of 288 GB against four dependent launches less per step
            # ... shared by the plans of an engine (plans run one at a time on one stream and no slab outlives its backward body): a
            # variable-width run makes one plan per padded width — a narrower plan takes a view of the widest workspace allocated so
            # far instead of slabs of its own (9-61 plans x ~0.4 GB for the deep net otherwise)
            pool = e.w9_ws_pool
            have_ws = pool.get(self.key)
            if have_ws is None or have_ws.numel() < need:
                # sized ONCE for the widest batch this engine is expected to see (plans created in ascending width order — the usual
                # case for variable-width batches — each found the pool too small and allocated a block of their own): the slab bytes of a
                # layer grow with the split count, which is capped, so the need at OCR_MAX_WIDTH (default 320 = configs[3]'s widest) bounds them
                wmax = max(_number('OCR_MAX_WIDTH', 320), sp.W)
                scale = max(1, wmax // sp.W + (1 if wmax % sp.W else 0))
                big = need
                if scale > 1:
                    big = max(need, ops.conv3x3_wgrad_workspace_bytes(s[0], s[1] * scale, s[2], self.ci, self.co))
                have_ws = pool[self.key] = torch.empty(big, dtype=torch.uint8, device=dev)      # (older plans keep the block their graphs captured)
            sp.buf[self.key + '/w9ws'] = have_ws[:need]
            if e.w9_pair:
                self._plan_w9_pair(sp, s)
        elif need and (have is None or have.numel() < need):     # one buffer per plan, shared by all layers (one stream)
            sp.buf['wgrad_ws'] = torch.empty(need, dtype=torch.uint8, device=dev)

    def _plan_w9_pair(self, sp, s):
        """Should this layer's (A's) slab kernel wait for layer B's and run inside B's launch?  B = the next op in BACKWARD order that runs a slab
        kernel (= the nearest earlier 3x3 layer with slabs of its own: with deferred reductions every slab layer has them), in the same backward
        body (same side of Engine.split_op: nothing is held across the exchange between the bodies), not itself waiting for a third layer, and
        ocr_conv3x3_wgrad_pair_supported(B, A) — the library's policy: B alone leaves at least half the chip empty.
        Why A's operands survive the wait (A's backward .. B's backward): x is a forward activation (prev.y) and dz is A's own gradient
        buffer (key/dy, or key/dz behind a batch norm), complete before A's backward runs — every consumer of A comes earlier in backward
        order, in residual graphs too, where grad_dst / grad_dst_acc deliver into the PRODUCER's dy or a scratch tensor, never into a
        consumer's.  Backward ops write gradient buffers of ops in front of them, weight gradients and workspaces; none writes a y, and each
        key owns its tensors (no aliasing between keys), so no op between A and B touches either operand."""
        e = self.eng
        i = e.ops.index(self)
        for j in range(i - 1, -1, -1):
            b = e.ops[j]
            if isinstance(b, _Conv1Op) and b.key + '/slab' in sp.buf:
                return          # (reduce jobs of its own in between: the order of the pending list would change)
            if isinstance(b, _Conv3x3Op) and b.key + '/w9ws' in sp.buf:
                bs = sp.shape[b.key][0]
                if ((i >= e.split_op) == (j >= e.split_op) and b.key not in sp.w9_hold_for
                        and ops.conv3x3_wgrad_pair_supported((bs[0], bs[1], bs[2], b.ci, b.co), (s[0], s[1], s[2], self.ci, self.co))):
                    sp.w9_hold_for[self.key] = b.key
                return

    def _conv_fwd(self, sp, x, out, bias, codes):
        w, p = self.wpack.view(self.co, 3, 3, self.ci), self.pool_after
        if p is not None and p.key in sp.fused_pools:
            if codes is not None:
                ops.conv3x3_relu_pool_codes(x, w, None, p.y(sp), codes, bias, p.kw_t, p.kh_f)
            else:
                ops.conv3x3_relu_pool(x, w, out, p.y(sp), bias, p.kw_t, p.kh_f)
        elif self.bn and sp.bn_stat_rows[self.key]:
            ops.conv3x3_stats(x, w, out, sp.buf[self.key + '/bnws'], bias=bias)
        else:
            ops.conv3x3(x, w, out=out, bias=bias, relu=self.mask_in_consumer)

    def _conv_bwd(self, sp, x, dz, dw, db):
        e, o, p = self.eng, sp.shape[self.key][1], self.prev
        own_ws = sp.buf.get(self.key + '/w9ws')
        held = sp.w9_held
        if own_ws is not None and self.key in sp.w9_hold_for:
            e.w9_hold(sp, self.key, x, dz, dw, db, own_ws)      # inside the launch of the next slab layer (_plan_w9_pair)
        elif own_ws is not None and held is not None and sp.w9_hold_for.get(held[0]) == self.key:
            # this layer's few, long workgroups in front, the waiting layer's behind them in the same grid; the reductions join the pending
            # list in backward order, each with the flush test it would have had behind a launch of its own
            sp.w9_held = None
            mine, theirs = ops.conv3x3_wgrad_pair_deferred((x, dz, dw, db, own_ws), held[1:])
            e.w9_append(sp, theirs, held[5])
            e.w9_append(sp, mine, own_ws)
        elif own_ws is not None:    # slab kernel now, the reduction with the other layers' at the end of the pass
            e._release_w9(sp)
            job, nblk = ops.conv3x3_wgrad_deferred(x, dz, dw, db, own_ws)
            if job is not None:
                e.w9_append(sp, (job, nblk), own_ws)
        else:
            ops.conv3x3_wgrad(x, dz, dw, dbias=db, workspace=sp.buf.get('wgrad_ws'))   # bias gradient rides on the same pass
        if p.key in sp.unpool_pools:            # through the pool in front, by the codes of ITS producer (alloc)
            pdy, finish = e.grad_dst(sp, p.prev)
            if pdy is not None:
                ops.conv3x3_dgrad_unpool(dz, self.wdgrad.view(self.ci, 3, 3, self.co), sp.buf[p.prev.key + '/pool_codes'], p.kw_t, p.kh_f,
                                         p.prev.mask_in_consumer, out=pdy)
                finish()
            return
        # a producer with several consumers (residual graphs): where the halo kernel runs, its epilogue adds to what was already
        # delivered instead of writing a scratch tensor that a second pass adds
        pdy, finish, acc = e.grad_dst_acc(sp, p, ops.conv3x3_accum_supported(o[0], o[1], o[2], self.co, self.ci))
        if pdy is not None:
            wd = self.wdgrad.view(self.ci, 3, 3, self.co)
            if sp.bn_bwd_rows.get(p.key, 0) and not acc:
                ops.conv3x3_dgrad_bnbwd(dz, wd, pdy, p.y(sp), sp.buf[p.key + '/z'], sp.buf[p.key + '/mean'], sp.buf[p.key + '/rstd'],
                                        sp.buf[p.key + '/bnws'])
            else:
                ops.conv3x3(dz, wd, out=pdy, mask=x if p.mask_in_consumer else None, accumulate=acc)
            finish()


class _Conv1x1Op(_ConvOp):
    """A plain GEMM over pixels."""
    kind = '1x1'

    def __init__(self, eng, node, prev):
        super(_Conv1x1Op, self).__init__(eng, node, prev)
        if self.ci % 8 or self.co % 8:
            raise NotImplementedError('%s: 1x1 conv needs C_in %% 8 == 0 and C_out %% 8 == 0' % self.name)
        self.wpack = torch.empty((self.co, self.ci), dtype=BF16, device=eng.device)

    def shadow_params(self):
        return [self.name + '/weights']

    def _conv_fwd(self, sp, x, out, bias, codes):
        s = sp.shape[self.key][0]
        M = s[0] * s[1] * s[2]
        ops.gemm_nt(x.view(M, self.ci), self.wpack, out=out.view(M, self.co), bias=bias, relu=self.mask_in_consumer)

    def _conv_bwd(self, sp, x, dz, dw, db):
        e, o = self.eng, sp.shape[self.key][1]
        M = o[0] * o[1] * o[2]
        pdy, finish = e.grad_dst(sp, self.prev)
        ops.gemm_tn(x.view(M, self.ci), dz.view(M, self.co), dw.view(self.ci, self.co), colsum=db)
        if pdy is not None:
            wsh = e.shadow(self.name + '/weights').view(self.ci, self.co)      # Q[n = ci][k = co]
            ops.gemm_nt(dz.view(M, self.co), wsh, out=pdy.view(M, self.ci),
                        mask=x.view(M, self.ci) if self.prev.mask_in_consumer else None)
            finish()


class _ConvFullOp(_ConvOp):
    """The VALID convolution whose kernel spans the whole feature axis: a plain GEMM over overlapping rows, its data gradient GEMM + col2im."""
    kind = 'full'

    def __init__(self, eng, node, prev):
        super(_ConvFullOp, self).__init__(eng, node, prev)
        self.wpack = torch.empty((self.co, self.kh * self.kw * self.ci), dtype=BF16, device=eng.device)

    def shadow_params(self):
        return [self.name + '/weights']

    def out_shape(self, s):
        N, W, H = s[0], s[1], s[2]
        if self.kw != H:
            raise NotImplementedError('%s: VALID conv is lowered only when k_w equals the feature-axis size '
                                      '(got k_w=%d, H=%d)' % (self.name, self.kw, H))
        return (N, W - self.kh + 1, 1, self.co)

    def alloc(self, sp, s):
        super(_ConvFullOp, self).alloc(sp, s)
        N, W, H, C = s
        sp.buf[self.key + '/col'] = torch.empty((N * (W - self.kh + 1), self.kh * H * C), dtype=BF16, device=self.eng.device)
        p = self.prev
        bn = getattr(p, 'bn_fused_into', None)
        if (_switch('OCR_FUSE_COL2IM_BN', False) and isinstance(p, _PoolOp) and bn is not None and p.consumers == 1 and self.kh == 2
                and not p.mask_in_consumer and bn.key + '/pool_codes' in sp.buf and (H * C) % 8 == 0):
            # the producer is a pool inside a batch-norm layer that holds routing codes: this layer's data gradient stops at the column
            # matrix, and that layer's statistics pass forms the pooled gradient from it (no col2im launch; _ConvOp._bn_bwd).  Off by default:
            # bit-identical, but the statistics pass grows by what the col2im launch took (13.3 -> 19.4 us against 6.0)
            sp.col_bn[bn.key] = (sp.buf[self.key + '/col'], N, W, H * C)

    def _conv_fwd(self, sp, x, out, bias, codes):
        (N, W, H, C), o = sp.shape[self.key]
        Wo = o[1]
        ops.gemm_nt(x, self.wpack, out=out.view(N * Wo, self.co), M=N * Wo, N=self.co, K=self.kh * H * C,
                    ldp=H * C, ldq=self.kh * H * C, bias=bias, relu=self.mask_in_consumer, row_group=Wo, row_skip=self.kh - 1)

    def _conv_bwd(self, sp, x, dz, dw, db):
        e, ((N, W, H, C), o) = self.eng, sp.shape[self.key]
        Wo, M, K = o[1], o[0] * o[1] * o[2], self.kh * H * C
        pdy, finish = e.grad_dst(sp, self.prev)
        dz2, dw2 = dz.view(M, self.co), dw.view(K, self.co)
        # the data gradient's GEMM dz W -> column matrix reads dz and the weights' bf16 shadow only: where the library's policy accepts it runs
        # INSIDE the launch this product completes (Engine.tn_push), on the CUs the weight-gradient tiles leave idle
        nt = None
        if pdy is not None and not self.prev.mask_in_consumer and self.kh == 2:
            col = sp.buf[self.key + '/col']
            wsh = e.shadow(self.name + '/weights').view(K, self.co)      # [K][co] bf16, k = co contiguous
            nt = (dz2, wsh, col, M, K, self.co)
        paired = e.tn_push(sp, ops.tn_job(x, H * C, dz2, self.co, dw2, self.co, M, K, self.co, row_group=Wo, row_skip=self.kh - 1, colsum=db),
                           (x, dz2, dw2, db),
                           lambda: ops.gemm_tn(x, dz2, dw2, Mk=M, I=K, J=self.co, lda=H * C, ldb=self.co,
                                               ldo=self.co, row_group=Wo, row_skip=self.kh - 1, colsum=db), nt=nt)
        if pdy is not None:
            if nt is None:
                raise NotImplementedError('%s: data gradient of a full-height VALID conv is lowered for k_h = 2 '
                                          'behind a non-ReLU producer' % self.name)
            if not paired:
                ops.gemm_nt(dz2, wsh, out=col, M=M, N=K, K=self.co)
            bn = getattr(self.prev, 'bn_fused_into', None)
            if bn is None or bn.key not in sp.col_bn:       # else: inside that layer's batch-norm statistics pass (alloc recorded col there)
                ops.conv5_col2im(col, pdy, N, W, H * C)
            finish()


def _conv_op(eng, node, prev):
    """'conv' of Engine._lower's table: the family follows from the attributes (each class refuses what its kernels do not take)."""
    a = node.attrs
    if a['c_i'] == 1:
        cls = _Conv1Op
    elif (a['k_h'], a['k_w'], a['padding']) == (3, 3, 'SAME'):
        cls = _Conv3x3Op
    elif (a['k_h'], a['k_w']) == (1, 1):
        cls = _Conv1x1Op
    elif a['padding'] == 'VALID':
        cls = _ConvFullOp
    else:
        raise NotImplementedError('%s: %dx%d %s convolution is not lowered' % (node.name, a['k_h'], a['k_w'], a['padding']))
    return cls(eng, node, prev)


class _FcOp(_Conv1x1Op):
    """Network.fc (network.py:415-447) on a row tensor [N, T, d]: y = relu?(x W + b) over the last axis = the GEMMs of a 1 x 1 convolution
    (`weights [dim, num_out]` has the memory layout of a [1, 1, dim, num_out] filter), so forward, data gradient, weight gradient, bf16 shadow and
    re-pack are _Conv1x1Op's on the flattened rows."""

    def out_shape(self, s):
        return tuple(s[:-1]) + (self.co,)

    def alloc(self, sp, s):
        o = self.out_shape(s)
        rows = int(np.prod(s[:-1]))
        sp.shape[self.key] = ((rows, 1, 1, s[-1]), (rows, 1, 1, self.co))      # what the 1x1 paths multiply out
        sp.buf[self.key + '/y'] = torch.empty(o, dtype=BF16, device=self.eng.device)
        sp.buf[self.key + '/dy'] = torch.empty(o, dtype=BF16, device=self.eng.device)


class _PoolOp(_Op):
    def __init__(self, eng, node, prev):
        super(_PoolOp, self).__init__(eng, node, prev)
        a = node.attrs
        # reference argument order is (k_h, k_w, s_h, s_w) with TF "height" = our time axis W
        self.kw_t, self.kh_f = a['k_h'], a['k_w']
        if (a['s_h'], a['s_w']) != (a['k_h'], a['k_w']) or self.kw_t not in (1, 2) or self.kh_f not in (1, 2):
            raise NotImplementedError('%s: max-pool is lowered for window == stride in {1,2}' % self.name)

    def dy_needed(self):
        return True

    def out_shape(self, s):
        N, W, H, C = s
        if W % self.kw_t or H % self.kh_f:
            raise NotImplementedError('%s: pooled axes must divide evenly (W=%d, H=%d)' % (self.name, W, H))
        return (N, W // self.kw_t, H // self.kh_f, C)

    def alloc(self, sp, s):
        o = self.out_shape(s)
        sp.shape[self.key] = (s, o)
        sp.buf[self.key + '/y'] = torch.empty(o, dtype=BF16, device=self.eng.device)
        sp.buf[self.key + '/dy'] = torch.empty(o, dtype=BF16, device=self.eng.device)

    fused_into = None          # the conv1 op that computes this pool's output itself
    bn_fused_into = None       # the batch-norm conv whose apply pass writes this pool's output and whose backward passes route its gradient

    def fwd(self, sp):
        if self.bn_fused_into is not None:
            return
        if self.fused_into is None and self.key not in sp.fused_pools:      # else: written by the producing conv's epilogue
            ops.maxpool_fwd(self.prev.y(sp), self.kw_t, self.kh_f, out=self.y(sp))

    def bwd(self, sp):
        if self.fused_into is not None or self.bn_fused_into is not None or self.key in sp.unpool_pools:
            return                  # (unpool_pools: the consumer's data-gradient kernel routed the gradient through this pool)
        pdy, finish = self.eng.grad_dst(sp, self.prev)
        if pdy is not None:
            codes = sp.buf.get(self.prev.key + '/pool_codes') if getattr(self.prev, 'pool_after', None) is self else None
            if codes is not None:       # the producing convolution's training forward left routing codes and no full-resolution output
                ops.maxpool_bwd_codes(codes, self.dy(sp), self.kw_t, self.kh_f, self.prev.mask_in_consumer, out=pdy)
            else:
                ops.maxpool_bwd(self.prev.y(sp), self.dy(sp), self.kw_t, self.kh_f, self.prev.mask_in_consumer, out=pdy)
            finish()


class _ViewOp(_Op):
    """reshape_squeeze_layer / dropout(identity): no data movement, shares the producer's buffers."""

    def __init__(self, eng, node, prev):
        super(_ViewOp, self).__init__(eng, node, prev)
        self.mask_in_consumer = prev.mask_in_consumer

    def dy_needed(self):
        return True

    def out_shape(self, s):
        if self.node.op == 'reshape_squeeze':
            N, A, B, C = s
            return (N, A * B, C)
        return s

    def alloc(self, sp, s):
        sp.shape[self.key] = (s, self.out_shape(s))

    def y(self, sp):
        return self.prev.y(sp).view(sp.shape[self.key][1])

    def dy(self, sp):
        d = self.prev.dy(sp)
        return None if d is None else d.view(sp.shape[self.key][1])

    def grad_owner(self):
        return self.prev.grad_owner()


class _AddOp(_Op):
    """Network.add (network.py:461-463): element-wise sum of two feature maps (residual connections)."""

    def dy_needed(self):
        return True

    def out_shape(self, s):
        return s

    def alloc(self, sp, s):
        sp.shape[self.key] = (s, s)
        sp.buf[self.key + '/y'] = torch.empty(s, dtype=BF16, device=self.eng.device)
        sp.buf[self.key + '/dy'] = torch.empty(s, dtype=BF16, device=self.eng.device)

    relu = False               # True: the Network.relu that follows (its only consumer) is computed here, y = relu(a + b)

    fwd_by = None              # the producing conv whose batch-norm apply pass writes this op's output (Engine._lower)

    def fwd(self, sp):
        if self.fwd_by is None:
            ops.eltwise(3 if self.relu else 0, self.inputs[0].y(sp), self.inputs[1].y(sp), self.y(sp))

    def bwd(self, sp):
        for p in self.inputs:
            if getattr(p, 'mask_from', None) is self:
                continue                            # that producer's batch-norm backward reads dy / y of this op directly
            self.eng.deliver(sp, p, self.dy(sp), mask=self.y(sp) if self.relu else None)


class _ReluOp(_Op):
    """Network.relu (network.py:340-341) as a stand-alone layer (after a residual add)."""

    def dy_needed(self):
        return True

    def out_shape(self, s):
        return s

    fused_into = None          # the _AddOp that computes relu(a + b) itself: this op is then a view of it (no buffers, no launches)

    def alloc(self, sp, s):
        sp.shape[self.key] = (s, s)
        if self.fused_into is None:
            sp.buf[self.key + '/y'] = torch.empty(s, dtype=BF16, device=self.eng.device)
            sp.buf[self.key + '/dy'] = torch.empty(s, dtype=BF16, device=self.eng.device)

    def y(self, sp):
        return self.fused_into.y(sp) if self.fused_into is not None else sp.buf[self.key + '/y']

    def dy(self, sp):
        return self.fused_into.dy(sp) if self.fused_into is not None else sp.buf[self.key + '/dy']

    def grad_owner(self):
        return self.fused_into.grad_owner() if self.fused_into is not None else self

    def fwd(self, sp):
        if self.fused_into is None:
            ops.eltwise(1, self.prev.y(sp), None, self.y(sp))

    def bwd(self, sp):
        if self.fused_into is None:
            self.eng.deliver(sp, self.prev, self.dy(sp), mask=self.y(sp))


class _SubsampleOp(_Op):
    """Second half of a strided convolution (Network.conv / conv_single with s_h, s_w > 1, network.py:193-216): picks every
    s-th position of the stride-1 result.  TF SAME: out = ceil(in / s), pad_before = max((out-1) s + k - in, 0) // 2, so output
    o is the stride-1 output at o s + (k-1)//2 - pad_before."""

    def __init__(self, eng, node, prev):
        super(_SubsampleOp, self).__init__(eng, node, prev)
        a = node.attrs
        self.sw, self.sh, self.kw, self.kh = a['s_h'], a['s_w'], a['k_h'], a['k_w']      # reference "height" = our time axis W
        if a['padding'] != 'SAME':
            raise NotImplementedError('%s: strided convolution is lowered for SAME padding' % self.name)

    def dy_needed(self):
        return True

    @staticmethod
    def _geom(n, k, s):
        out = -(-n // s)
        before = max((out - 1) * s + k - n, 0) // 2
        return out, (k - 1) // 2 - before

    def out_shape(self, s):
        N, W, H, C = s
        Wo, self.ow = self._geom(W, self.kw, self.sw)
        Ho, self.oh = self._geom(H, self.kh, self.sh)
        return (N, Wo, Ho, C)

    def alloc(self, sp, s):
        o = self.out_shape(s)
        sp.shape[self.key] = (s, o)
        sp.buf[self.key + '/y'] = torch.empty(o, dtype=BF16, device=self.eng.device)
        sp.buf[self.key + '/dy'] = torch.empty(o, dtype=BF16, device=self.eng.device)

    def fwd(self, sp):
        (N, W, H, C), (_, Wo, Ho, _) = sp.shape[self.key]
        ops.subsample(self.prev.y(sp), self.y(sp), N, W, H, C, Wo, Ho, self.sw, self.sh, self.ow, self.oh)

    def bwd(self, sp):
        (N, W, H, C), (_, Wo, Ho, _) = sp.shape[self.key]
        pdy, finish = self.eng.grad_dst(sp, self.prev)
        if pdy is not None:
            ops.subsample(self.dy(sp), pdy, N, W, H, C, Wo, Ho, self.sw, self.sh, self.ow, self.oh, backward=True)
            if self.prev.mask_in_consumer:
                ops.eltwise(2, pdy, self.prev.y(sp), pdy)
            finish()


class _BatchNormOp(_Op):
    """Network.batch_normalization (network.py:466-473): batch statistics when is_training, else the stored moving ones."""

    def __init__(self, eng, node, prev):
        super(_BatchNormOp, self).__init__(eng, node, prev)
        self.relu, self.training = node.attrs['relu'], node.attrs['is_training']

    def dy_needed(self):
        return True

    def out_shape(self, s):
        return s

    def alloc(self, sp, s):
        dev, C = self.eng.device, s[-1]
        sp.shape[self.key] = (s, s)
        sp.buf[self.key + '/y'] = torch.empty(s, dtype=BF16, device=dev)
        sp.buf[self.key + '/dy'] = torch.empty(s, dtype=BF16, device=dev)
        sp.buf[self.key + '/dx'] = torch.empty(s, dtype=BF16, device=dev)
        if self.training:
            M = int(np.prod(s[:-1]))
            sp.buf[self.key + '/mean'] = torch.empty(C, dtype=F32, device=dev)
            sp.buf[self.key + '/rstd'] = torch.empty(C, dtype=F32, device=dev)
            sp.buf[self.key + '/bnws'] = ops.bn_workspace(M, C, dev)

    def _x(self, sp):
        if self.prev.mask_in_consumer:
            raise NotImplementedError('%s: batch_normalization behind a fused-ReLU convolution is not lowered' % self.name)
        return self.prev.y(sp)

    def fwd(self, sp):
        e, (s, _) = self.eng, sp.shape[self.key]
        C = s[-1]
        M = int(np.prod(s[:-1]))
        x, y = self._x(sp).view(M, C), self.y(sp).view(M, C)
        if self.training:
            ops.bn_train_fwd(x, e.param(self.name + '/gamma'), e.param(self.name + '/beta'), BN_EPS, self.relu, sp.buf[self.key + '/bnws'],
                             out=y, save_mean=sp.buf[self.key + '/mean'], save_rstd=sp.buf[self.key + '/rstd'])
        else:
            ops.bn_infer_fwd(x, e.param(self.name + '/gamma'), e.param(self.name + '/beta'), e.param(self.name + '/moving_mean'),
                             e.param(self.name + '/moving_variance'), BN_EPS, self.relu, y)

    def bwd(self, sp):
        e, (s, _) = self.eng, sp.shape[self.key]
        C = s[-1]
        M = int(np.prod(s[:-1]))
        x, y, dy, dx = self._x(sp).view(M, C), self.y(sp).view(M, C), self.dy(sp).view(M, C), sp.buf[self.key + '/dx'].view(M, C)
        if self.training:
            ops.bn_train_bwd(x, y, dy, e.param(self.name + '/gamma'), sp.buf[self.key + '/mean'], sp.buf[self.key + '/rstd'],
                             e.grad(self.name + '/gamma'), e.grad(self.name + '/beta'), self.relu, sp.buf[self.key + '/bnws'], out=dx)
        else:
            ops.bn_infer_bwd(x, y, dy, e.param(self.name + '/gamma'), e.param(self.name + '/moving_mean'),
                             e.param(self.name + '/moving_variance'), e.grad(self.name + '/gamma'), e.grad(self.name + '/beta'), BN_EPS,
                             self.relu, dx)
        e.deliver(sp, self.prev, sp.buf[self.key + '/dx'])


class _DropoutOp(_Op):
    """Network.dropout = tf.nn.dropout(x, keep_prob) (network.py:626-628).  keep_prob is the layer's own argument: the network's
    keep_prob input slot (what the shipped graphs pass) takes the value the driver feeds — 0.5 in training steps (train.py:126), 1.0
    otherwise (train.py:156, test.py:75): Engine.train_keep_prob / inference = 1 — and a NUMBER written in the graph is a constant of
    the graph, applied in training and inference alike, as tf.nn.dropout does with a Python float (it used to be ignored).
    The mask is a hash of (layer name, rank, completed optimiser steps, element index): data-parallel ranks draw different masks."""

    def __init__(self, eng, node, prev):
        super(_DropoutOp, self).__init__(eng, node, prev)
        self.mask_in_consumer = False
        import zlib
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank(eng.group)
        self.seed = (zlib.crc32(self.name.encode()) ^ 0x5bd1e995 ^ (rank * 0x9E3779B1)) & 0xffffffff
        kp = node.attrs.get('keep_prob')
        self.const_keep_prob = float(kp) if isinstance(kp, (int, float)) and not isinstance(kp, bool) else None

    def dy_needed(self):
        return True

    def out_shape(self, s):
        return s

    def alloc(self, sp, s):
        sp.shape[self.key] = (s, s)
        sp.buf[self.key + '/y'] = torch.empty(s, dtype=BF16, device=self.eng.device)
        sp.buf[self.key + '/dy'] = torch.empty(s, dtype=BF16, device=self.eng.device)
        sp.buf[self.key + '/dx'] = torch.empty(s, dtype=BF16, device=self.eng.device)

    def _kp(self):
        if self.const_keep_prob is not None:
            return self.const_keep_prob
        return float(self.eng.train_keep_prob) if self.eng.training else 1.0

    def fwd(self, sp):
        x = self.prev.y(sp)
        if self.prev.mask_in_consumer:
            raise NotImplementedError('%s: dropout directly behind a fused-ReLU convolution is not lowered' % self.name)
        ops.dropout(x, self.y(sp), self.seed, self.eng.step_counter(), self._kp())

    def bwd(self, sp):
        ops.dropout(self.dy(sp), sp.buf[self.key + '/dx'], self.seed, self.eng.step_counter(), self._kp())
        self.eng.deliver(sp, self.prev, sp.buf[self.key + '/dx'])


class _AvgPoolOp(_PoolOp):
    """Network.avg_pool (network.py:352-359), window == stride."""

    def fwd(self, sp):
        (N, W, H, C), _ = sp.shape[self.key]
        x = self.prev.y(sp)
        if self.prev.mask_in_consumer:
            pass            # the ReLU is already applied to the stored activation; only its BACKWARD is deferred to the consumer
        ops.avgpool(x, self.y(sp), N, W, H, C, self.kw_t, self.kh_f)

    def bwd(self, sp):
        (N, W, H, C), _ = sp.shape[self.key]
        pdy, finish = self.eng.grad_dst(sp, self.prev)
        if pdy is not None:
            ops.avgpool(self.dy(sp), pdy, N, W, H, C, self.kw_t, self.kh_f, backward=True)
            if self.prev.mask_in_consumer:
                ops.eltwise(2, pdy, self.prev.y(sp), pdy)
            finish()


class _ConcatOp(_Op):
    """Network.concat along the channel axis (network.py:154-158, axis = 3): copies, no arithmetic."""

    def __init__(self, eng, node, prev):
        super(_ConcatOp, self).__init__(eng, node, prev)
        if node.attrs.get('axis') not in (3, -1):
            raise NotImplementedError('%s: concat is lowered along the channel axis only' % self.name)

    def dy_needed(self):
        return True

    def out_shape(self, s):
        return tuple(s[:-1]) + (sum(self._cin),)

    def alloc(self, sp, s):
        self._cin = [sp.oshape[p.key][-1] for p in self.inputs]
        o = self.out_shape(s)
        sp.shape[self.key] = (s, o)
        sp.buf[self.key + '/y'] = torch.empty(o, dtype=BF16, device=self.eng.device)
        sp.buf[self.key + '/dy'] = torch.empty(o, dtype=BF16, device=self.eng.device)
        for i, c in enumerate(self._cin):
            sp.buf['%s/part%d' % (self.key, i)] = torch.empty(tuple(s[:-1]) + (c,), dtype=BF16, device=self.eng.device)

    def fwd(self, sp):
        y, off = self.y(sp), 0
        for p, c in zip(self.inputs, self._cin):
            if p.mask_in_consumer:
                raise NotImplementedError('%s: concat of a fused-ReLU convolution output is not lowered' % self.name)
            y[..., off:off + c].copy_(p.y(sp))
            off += c

    def bwd(self, sp):
        dy, off = self.dy(sp), 0
        for i, (p, c) in enumerate(zip(self.inputs, self._cin)):
            part = sp.buf['%s/part%d' % (self.key, i)]
            part.copy_(dy[..., off:off + c])
            self.eng.deliver(sp, p, part)
            off += c


class _SoftmaxOp(_Op):
    """Network.softmax (network.py:441-447) over the last axis of fp32 logits — an inference output (CTC takes unnormalised
    activations, so nothing differentiates through it in this engine)."""

    def out_shape(self, s):
        return s

    def alloc(self, sp, s):
        sp.shape[self.key] = (s, s)
        sp.buf[self.key + '/y'] = torch.empty(s, dtype=F32, device=self.eng.device)

    def dy(self, sp):
        return None

    def fwd(self, sp):
        ops.softmax(self.prev.y(sp), self.y(sp))

    def bwd(self, sp):
        raise NotImplementedError('%s: softmax is an inference output; the loss takes the unnormalised logits' % self.name)


class _BiLstmOp(_Op):
    """bi_lstm (network.py:97-129: ND = 2 directions of LSTMCell(num_hids // 2)) and one cell of the unidirectional stacked `lstm`
    (network.py:130-152: ND = 1, LSTMCell(num_hids)), optionally followed by the FC + [N,T] -> [T,N] transpose."""

    def __init__(self, eng, node, prev):
        super(_BiLstmOp, self).__init__(eng, node, prev)
        a = node.attrs
        self.ND = 2 if node.op == 'bi_lstm' else 1
        self.U, self.C, self.D = a['num_hids'] // self.ND, a['nclasses'], a['din']
        self.cells = a.get('cells') or [self.name + '/fw', self.name + '/bw']       # variable-name prefix of each direction's LSTMCell
        self.fc = a.get('fc', self.name)                                            # variable-name prefix of the FC
        self.with_fc = a.get('with_fc', True)       # False: a hidden layer of a stack, output = [N, T, ND * U]
        if self.U % 32 or self.D % 32 or self.C % 8:
            raise NotImplementedError('%s: needs hidden units per direction %% 32 == 0, input features %% 32 == 0, classes %% 8 == 0' % self.name)
        dev, U, D, C, ND = eng.device, self.U, self.D, self.C, self.ND
        self.wxT = torch.empty((ND * 4 * U, D), dtype=BF16, device=dev)
        self.whT = torch.empty((ND, 4 * U, U), dtype=BF16, device=dev)
        self.bias = torch.empty(ND * 4 * U, dtype=F32, device=dev)
        self.wfcT = torch.empty((C, ND * U), dtype=BF16, device=dev) if self.with_fc else None
        self.wcat = torch.empty((D, ND * 4 * U), dtype=BF16, device=dev)

    def dy_needed(self):
        return True

    def out_shape(self, s):
        N, T, D = s
        return (T, N, self.C) if self.with_fc else (N, T, self.ND * self.U)

    def y(self, sp):
        if self.with_fc:
            return sp.buf[self.key + '/y']
        (N, T, _), _ = sp.shape[self.key]
        return sp.buf[self.key + '/hout'].view(N, T, self.ND * self.U)

    def dy(self, sp):
        if self.with_fc:
            return sp.buf[self.key + '/dy']
        (N, T, _), _ = sp.shape[self.key]
        return sp.buf[self.key + '/dhout'].view(N, T, self.ND * self.U)

    def _persistent(self, N):
        return self.ND == 2 and self.eng.persistent_lstm and ops.lstm_seq_supported(N, self.U)

    def alloc(self, sp, s):
        N, T, D = s
        U, C, ND, dev = self.U, self.C, self.ND, self.eng.device
        R = N * T
        sp.shape[self.key] = (s, self.out_shape(s))
        b = sp.buf
        b[self.key + '/xproj'] = torch.empty((R, ND * 4 * U), dtype=F32, device=dev)
        b[self.key + '/hout'] = torch.zeros((R, ND * U), dtype=BF16, device=dev)
        b[self.key + '/gates'] = torch.zeros((ND, R, 4 * U), dtype=F32, device=dev)
        b[self.key + '/cell'] = torch.zeros((ND, R, U), dtype=F32, device=dev)
        if self.with_fc:
            b[self.key + '/y'] = torch.empty((T, N, C), dtype=F32, device=dev)      # logits, time-major
            b[self.key + '/dy'] = torch.empty((R, C), dtype=BF16, device=dev)       # d loss / d logits, [N,T,C]
            # split partials of the FC weight gradient (ops.gemm_tn_split: added in a fixed order, no float atomics)
            b[self.key + '/fc_ws'] = torch.empty(ops.gemm_tn_split_workspace(R, ND * U, C), dtype=F32, device=dev)
        b[self.key + '/dhout'] = torch.empty((R, ND * U), dtype=BF16, device=dev)
        b[self.key + '/dz'] = torch.zeros((R, ND * 4 * U), dtype=BF16, device=dev)
        b[self.key + '/dc'] = torch.zeros((ND, N, U), dtype=F32, device=dev)
        b[self.key + '/hprev'] = torch.empty((ND, R, U), dtype=BF16, device=dev)
        b[self.key + '/xh'] = torch.empty((ND, R, self.D + U), dtype=BF16, device=dev)
        if self.ND == 2:
            words = max(ops.lstm_seq_sync_words(N, U), 64) if self._persistent(N) else 64
            words = (words + 3) // 4 * 4                   # 16-byte granules: the blocks of a plan become views of ONE arena (ShapePlan)
            b[self.key + '/sync_f'] = torch.zeros(words, dtype=I32, device=dev)
            b[self.key + '/sync_b'] = torch.zeros(words, dtype=I32, device=dev)
            sp.lstm_sync_keys += (self.key + '/sync_f', self.key + '/sync_b')

    def shadow_params(self):
        return [c + '/weights' for c in self.cells] + ([self.fc + '/weights'] if self.with_fc else [])

    def pack_jobs(self):
        e, U, D, ND = self.eng, self.U, self.D, self.ND
        jobs = []
        for d, cell in enumerate(self.cells):
            w = e.param(cell + '/weights')                  # [D+U, 4U], gate-major columns
            jobs.append(dict(type=0, R=D, Cc=4 * U, ldin=4 * U, lstm_units=U, src=w[:D], dst=self.wxT[d * 4 * U:(d + 1) * 4 * U]))
            jobs.append(dict(type=0, R=U, Cc=4 * U, ldin=4 * U, lstm_units=U, src=w[D:], dst=self.whT[d]))
            jobs.append(dict(type=2, R=D, Cc=4 * U, ldin=4 * U, ldout=ND * 4 * U, src=w, dst=self.wcat[:, d * 4 * U:]))
        if self.with_fc:
            wf = e.param(self.fc + '/weights')
            jobs.append(dict(type=0, R=wf.shape[0], Cc=wf.shape[1], ldin=wf.shape[1], src=wf, dst=self.wfcT))
        for d, cell in enumerate(self.cells):      # the biases' gate-order permutation rides in the same launch
            jobs.append(dict(type=4, lstm_units=U, n=4 * U, src=e.param(cell + '/biases'), dst=self.bias[d * 4 * U:(d + 1) * 4 * U]))
        return jobs

    def fwd(self, sp):
        e, U, C, ND = self.eng, self.U, self.C, self.ND
        (N, T, D), _ = sp.shape[self.key]
        R = N * T
        b = sp.buf
        x = self.prev.y(sp).view(R, D)
        if (self._persistent(N) and ND == 2 and _switch('OCR_LSTM_FUSE_X') and x.is_contiguous()
                and ops.lstm_fwd_seq_x_supported(N, U, D)):
            # the input projection inside the recurrent kernel (its MFMAs run while a step's first poll is under way): no projection GEMM,
            # no fp32 projection tensor
            ops.lstm_fwd_seq_x(x, self.wxT, self.bias, self.whT, sp.seq_len, b[self.key + '/hout'], b[self.key + '/gates'],
                               b[self.key + '/cell'], N, T, U, b[self.key + '/sync_f'], 1.0, prepared=_take_ring(sp, self.key + '/sync_f'))
        elif self._persistent(N):
            ops.gemm_nt(x, self.wxT, out=b[self.key + '/xproj'], bias=self.bias)
            ops.lstm_fwd_seq(b[self.key + '/xproj'], self.whT, sp.seq_len, b[self.key + '/hout'], b[self.key + '/gates'],
                             b[self.key + '/cell'], N, T, U, b[self.key + '/sync_f'], 1.0, prepared=_take_ring(sp, self.key + '/sync_f'))
        else:
            ops.gemm_nt(x, self.wxT, out=b[self.key + '/xproj'], bias=self.bias)
            for s in range(T):
                ops.lstm_fwd_step(b[self.key + '/xproj'], self.whT, sp.seq_len, b[self.key + '/hout'],
                                  b[self.key + '/gates'], b[self.key + '/cell'], N, T, U, s, 1.0, ND)
        if self.with_fc:
            ops.gemm_nt(b[self.key + '/hout'], self.wfcT, out=b[self.key + '/y'].view(R, C),
                        bias=e.param(self.fc + '/biases'), rowswap=(T, N))

    def bwd(self, sp):
        e, U, C, D, ND = self.eng, self.U, self.C, self.D, self.ND
        (N, T, _), _ = sp.shape[self.key]
        R = N * T
        b = sp.buf
        hout = b[self.key + '/hout']
        x = self.prev.y(sp).view(R, D)
        batched = (D + U) % 128 == 0 and (4 * U) % 128 == 0
        if self.with_fc:
            dl = b[self.key + '/dy']
            # FC: dW += H^T dL, db += colsum dL, dH = dL Wfc^T  (the split contraction is added in a fixed order: the same bits every run)
            ops.gemm_tn_split(hout, dl, e.grad(self.fc + '/weights'), b[self.key + '/fc_ws'], colsum=e.grad(self.fc + '/biases'))
            ops.gemm_nt(dl, e.shadow(self.fc + '/weights'), out=b[self.key + '/dhout'])
        # BPTT, all directions per launch
        wsh = e.shadow(self.cells[0] + '/weights')
        stride = e.offset(self.cells[1] + '/weights') - e.offset(self.cells[0] + '/weights') if ND == 2 else 0
        if self._persistent(N):
            ops.lstm_bwd_seq(wsh[D:], 4 * U, stride, sp.seq_len, b[self.key + '/dhout'], b[self.key + '/gates'],
                             b[self.key + '/cell'], b[self.key + '/dz'], N, T, U, b[self.key + '/sync_b'], prepared=_take_ring(sp, self.key + '/sync_b'))
        else:
            b[self.key + '/dc'].zero_()
            for s in range(T - 1, -1, -1):
                ops.lstm_bwd_step(wsh[D:], 4 * U, stride, sp.seq_len, b[self.key + '/dhout'], b[self.key + '/gates'],
                                  b[self.key + '/cell'], b[self.key + '/dz'], b[self.key + '/dc'], N, T, U, s, ND)
        dz = b[self.key + '/dz']
        gw = [e.grad(cell + '/weights') for cell in self.cells]
        gb = [e.grad(cell + '/biases') for cell in self.cells]
        if batched:
            # dW_d[D+U, 4U] = [x | h_prev,d]^T dz_d for all directions in ONE launch (the TF LSTMCell matrix is applied to
            # concat([x_t, h_{t-1}]), network.py:104-107): 4 short-K weight-gradient launches become 1
            xh = b[self.key + '/xh']
            ops.lstm_xh(x, hout, sp.seq_len, xh, N, T, D, U, ND)
            scs = (e.offset(self.cells[1] + '/biases') - e.offset(self.cells[0] + '/biases')) if ND == 2 else 0
            e.tn_push(sp, ops.tn_job(xh, D + U, dz, ND * 4 * U, gw[0], 4 * U, R, D + U, 4 * U, nbatch=ND, strideA=R * (D + U), strideB=4 * U,
                                     strideOut=stride, colsum=gb[0], strideColsum=scs),
                      (xh, dz, gw[0], gb[0]),
                      lambda: ops.gemm_tn_batched(xh, D + U, R * (D + U), dz, ND * 4 * U, 4 * U, gw[0], 4 * U, stride, R, D + U, 4 * U, ND,
                                                  colsum=gb[0], strideColsum=scs))
        else:
            ops.lstm_hprev(hout, sp.seq_len, b[self.key + '/hprev'], N, T, U, ND)
            for d in range(ND):
                dzd = dz[:, d * 4 * U:(d + 1) * 4 * U]
                ops.gemm_tn(x, dzd, gw[d][:D], Mk=R, I=D, J=4 * U, lda=D, ldb=ND * 4 * U, ldo=4 * U, colsum=gb[d])
                ops.gemm_tn(b[self.key + '/hprev'][d], dzd, gw[d][D:], Mk=R, I=U, J=4 * U, lda=U, ldb=ND * 4 * U, ldo=4 * U)
        pdy, finish = e.grad_dst(sp, self.prev)
        if pdy is not None:
            pmask = self.prev.y(sp).view(R, D) if self.prev.mask_in_consumer else None
            ops.gemm_nt(dz, self.wcat, out=pdy.view(R, D), mask=pmask)
            finish()
