"""Plan executor: lowers a Network plan onto the gfx950 kernels of libocrhip.so.

What the reference does with a TF session (`sess.run([loss, train_op], feed_dict)` — lib/lstm/train.py:118-130)
is done here as:
  * ONE flat fp32 parameter buffer in HBM (TF variable names and layouts kept, so checkpoints stay portable),
    ordered [L2-regularised tensors | rest]; flat gradient / Adam-moment buffers of the same layout — the
    optimiser is two grid-stride kernels and the data-parallel exchange is one RCCL all-reduce of one buffer;
  * bf16 operand copies of the weights in the K-contiguous layouts the MFMA kernels want, refreshed by small
    pack kernels after every update;
  * per input shape (N, W) a statically allocated set of activation / gradient buffers and a captured hipGraph
    of the whole forward+backward (and of the optimiser), replayed each step — no allocator, no host scalars,
    no per-op launch cost on the hot loop;
  * layers run in plan order forward and in reverse order backward (the graph is a chain); ReLU backward is
    fused into the consumer's gradient kernel (dgrad epilogue / pool backward / BN backward).
Arithmetic contract: bf16 storage and MFMA operands, fp32 accumulation, fp32 gate / cell / CTC / BN-statistics /
optimiser math.  oracle/graph.py(sim_bf16=True) rounds at the same points.
"""
import time

import numpy as np
import torch

from . import dist as ocr_dist
from . import ops
from ._native import NativeError, call as nat_call
from .engine_ops import (BF16, F32, I32, _env, _number, _switch, _AddOp, _AvgPoolOp, _BatchNormOp, _BiLstmOp, _ConcatOp, _ConvOp,
                         _Conv3x3Op, _DropoutOp, _FcOp, _InputOp, _PoolOp, _ReluOp, _SoftmaxOp, _SubsampleOp, _ViewOp, _conv_op)
from .automaton import LabelAutomaton, SparseLabelAutomaton
from .lexicon import LexiconTrie
from .layout import FlatLayout, execution_order, init_host_parameters

ALIGN = 64               # parameter offsets are multiples of 64 elements (256 B)

# Every environment variable the engine reads (through engine_ops._env / _switch / _number, nowhere else), by the moment it is read.
# A switch is on unless it is '0' (default in brackets; a switch whose default is 0 is on when set to anything else); tests and tools set them between those moments.
#   read once, when the Engine is constructed
#     OCR_FUSE_BN_STATS [1]      0: batch-norm statistics (and backward sums) by passes of their own, not from the convolutions' write-outs
#     OCR_W9_FLUSH_MB [80]       slab megabytes after which the pending weight-gradient reductions run; 0: one reduction at the end of the body
#     OCR_W9_DEFER [1]           0: every 3x3 weight gradient reduces its slabs right behind its own kernel (shared workspace)
#     OCR_W9_DEFER_MAX_MB [192]  with OCR_W9_FLUSH_MB=0: total slab megabytes of a plan above which it falls back to the shared workspace
#     OCR_W9_PAIR [1]            0: every 3x3 weight-gradient slab kernel is a launch of its own, none waits to share a launch with the next layer's
#     OCR_TN_JOBS [1]            0: every plain weight-gradient product is a launch of its own, no paired gemm_tn3 launch
#     OCR_TN_SIDE [0]            1: the paired launch runs on a side stream beside the main chain
#     OCR_TN_NT_PAIR [1]         0: conv5's data-gradient GEMM stays a launch of its own behind the paired gemm_tn3 launch, not inside it
#     OCR_OVERLAP_ALLREDUCE [1]  0: data parallel without the split schedule: one all-reduce after the whole backward pass
#     OCR_DP_GRAPH [0]           '1': the whole data-parallel step as ONE graph with captured collectives (opt-in)
#     OCR_FORCE_ALLREDUCE [unset] any value: the RCCL call is exercised on a 1-rank group (tests)
#     OCR_FAKE_WORLD [unset]     n: single-GPU emulation of n identical ranks (tests)
#   read by every Engine._lower
#     OCR_FUSE_ADD_RELU [1]      0: residual add and the relu behind it stay two passes; no batch-norm tail / mask fusion
#     OCR_FUSE_CONV_POOL [1]     0: no max-pool in a 3x3 convolution's epilogue (pool_after)
#     OCR_FUSE_BN_POOL [1]       0: no 1 x 2 max-pool inside the batch-norm passes (bn_pool)
#   read by every op.alloc, i.e. per ShapePlan
#     OCR_POOL_CODES [1]         0: layers in front of a fused max-pool keep their full-resolution y instead of routing codes
#     OCR_CONV1_CODES [1]        0: conv1 + pool's backward recomputes the routing instead of reading saved codes
#     OCR_CONV1_SLAB [1]         0: conv1 + pool's weight gradient by atomics instead of slabs + the merged reduction
#     OCR_FUSE_BN_BWD [1]        0: no batch-norm backward sums from the consumer's data-gradient kernel
#     OCR_FUSE_UNPOOL [1]        0: a max-pool's backward stays a launch of its own behind the data gradient of the 3x3 convolution after it
#     OCR_FUSE_COL2IM_BN [0]     1: conv5's col2im inside the statistics pass of conv4_2's batch-norm backward (measured: no gain, off by default)
#     OCR_MAX_WIDTH [320]        widest input the shared slab workspaces are sized for ahead of time
#   read by every forward pass
#     OCR_FUSE_ZERO [1]          0: the gradient buffer is cleared by a fill, not by conv1 + pool's launch
#     OCR_FUSE_RINGFILL [1]      0: every persistent LSTM launch fills its own hand-off block
#     OCR_LSTM_FUSE_X [1]        0: the BiLSTM's input projection stays a GEMM of its own
#   read at every use (Engine._guard_on)
#     OCR_LSTM_TIMEOUT_GUARD [1] 0: a persistent-LSTM time-out does not drop the step's update




# ====================================================================================================== plan per shape
class ShapePlan(object):
    """All buffers for one (N, W) input shape plus the captured graphs."""

    def _init_fields(self, N, W):
        """Every host-side field engine code sets on a plan, declared here before any op allocates (no device needed)."""
        self.N, self.W = N, W
        self.buf, self.shape = {}, {}
        self.scratch = {}
        self.dy_done = set()
        self.w9_pending, self.w9_tables = [], {}    # deferred weight-gradient reductions of the running backward pass / their device tables
        self.w9_pending_bytes = 0                   # ... and the slab bytes they cover (Engine.w9_flush_bytes)
        self.tn_pending = []                        # plain weight-gradient products waiting for a partner (Engine.tn_push)
        self.w9_held = None                         # (key, x, dz, dw, db, workspace): a slab launch waiting for its partner layer (Engine.w9_hold)
        self.tn_side_open = False                   # a paired launch is running on the side stream (Engine._join_tn)
        # what the ops' alloc decided for this shape
        self.fused_pools = set()                    # keys of the max-pools a 3x3 convolution's epilogue writes
        self.bn_stat_rows = {}                      # conv key -> partial statistics rows its own epilogue writes (0: statistics pass)
        self.bn_bwd_rows = {}                       # conv key -> partial backward-sum rows its consumer's data gradient writes
        self.w9_hold_for = {}                       # conv key A -> conv key B: A's slab kernel waits and runs inside B's launch (_Conv3x3Op._plan_w9_pair)
        self.unpool_pools = set()                   # keys of the max-pools whose backward pass their consumer's data gradient does (no /dy)
        self.col_bn = {}                            # batch-norm conv key -> (col, Nb, W, HC): its statistics pass does conv5's col2im
        self.lstm_sync_keys = ()                    # buffer keys of the persistent LSTM launches' hand-off blocks
        self.lstm_arena, self.lstm_sync = None, ()
        # state of the last forward pass
        self.rings_ready, self.rings_armed = set(), False
        self.graph_fb = self.graph_fwd = self.graph_fb1 = self.graph_fb2 = self.graph_dp = self.graph_step = None
        self._guard_addrs = None                    # Engine._guard_addrs: None = not built yet, False = no persistent launch
        self._report = None                         # Engine.report_async's slots

    def __init__(self, eng, N, W):
        self._init_fields(N, W)
        dev = eng.device
        self.x = torch.zeros((N, W, eng.num_features), dtype=F32, device=dev)
        self.labels = torch.zeros(N * eng.max_label_len, dtype=I32, device=dev)
        self.labels_len = torch.zeros(N, dtype=I32, device=dev)
        self.seq_len = torch.ones(N, dtype=I32, device=dev)
        self.oshape = {'data': (N, W, eng.num_features)}       # output shape per op key (multi-input ops look their inputs up here)
        for op in eng.ops:
            s = self.oshape[op.prev.key]
            op.alloc(self, s)
            self.oshape[op.key] = op.out_shape(s)
        # the hand-off blocks of all persistent LSTM launches of a step as views of ONE arena: a training step sets the whole arena to the
        # pattern the kernels start from inside its first kernel (conv1 + pool forward) instead of one fill launch per LSTM launch
        keys = self.lstm_sync_keys
        if keys:
            self.lstm_arena = torch.zeros(sum(self.buf[k].numel() for k in keys), dtype=I32, device=dev)
            off = 0
            for k in keys:
                n = self.buf[k].numel()
                self.buf[k] = self.lstm_arena[off:off + n]
                off += n
        self.lstm_sync = tuple(self.buf[k] for k in keys)
        # deferred weight-gradient reductions keep every layer's slabs until the end of the backward body: that pays while the slabs
        # still sit in the Infinity Cache when the merged reduction reads them (162 MB for the CRNN at 64 x 256: 18 + 4 x 36 MB).  A deep graph (configs[4]:
        # 32 layers, ~0.4 GB of slabs) would read them back from HBM — measured 3 % slower than reducing behind each layer — so
        # such a plan falls back to ONE shared workspace and immediate reductions.
        # (round 4: with a flush threshold — OCR_W9_FLUSH_MB, default 80 — no more than that plus one layer of slabs is ever pending, so a deep
        #  plan keeps per-layer workspaces too and reduces ~80 MB at a time in merged launches instead of behind each of its 32 layers)
        own = [k for k in self.buf if k.endswith('/w9ws')]
        if own and sum(self.buf[k].numel() for k in own) > eng.w9_defer_max_bytes and not eng.w9_flush_bytes:
            need = max(self.buf[k].numel() for k in own)
            for k in own:
                del self.buf[k]
            self.w9_hold_for.clear()                # (no deferred reductions, no paired launches)
            self.buf['wgrad_ws'] = torch.empty(need, dtype=torch.uint8, device=dev)
        self.T, _, self.C = self.oshape[eng.ops[-1].key]
        self.costs = torch.zeros(N, dtype=F32, device=dev)
        _, ws_bytes, grad_shape = eng.ctc_form_of(self.C, self.T, N)
        self.ctc_grad = torch.empty(grad_shape, dtype=F32, device=dev)
        self.ctc_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        self.decoded = torch.zeros((N, self.T), dtype=I32, device=dev)
        self.decoded_len = torch.zeros(N, dtype=I32, device=dev)


# ====================================================================================================== engine
class Engine(object):
    """Owns parameters, optimiser state and per-shape plans for one Network on one GPU."""

    def __init__(self, net, device='cuda:0', seed=None, max_label_len=31, use_graphs=True, group=None,
                 persistent_lstm=True, fuse_conv1_pool=True, ctc_long=True, ctc_wide=True):
        from .config import cfg
        if max_label_len > self.CTC_MAX_LABEL_LEN:
            raise ValueError('max_label_len = %d: the CTC loss covers labels of at most %d characters' % (max_label_len, self.CTC_MAX_LABEL_LEN))
        if not torch.cuda.is_available():
            raise NativeError('Engine needs a ROCm GPU: the hot path has no CPU implementation')
        self.cfg = cfg
        self.net = net
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.num_features = cfg.NUM_FEATURES
        self.max_label_len = max_label_len
        self.ctc_long = ctc_long          # False: the one-launch long-label kernel is never chosen (A/B switch)
        self.ctc_wide = ctc_wide          # False: the two-launch wide-alphabet form is never chosen (A/B switch)
        self.use_graphs = use_graphs
        self.persistent_lstm = persistent_lstm
        self.fuse_conv1_pool = fuse_conv1_pool
        self.fuse_bn_stats = _switch('OCR_FUSE_BN_STATS')     # batch-norm statistics from the producing convolution's epilogue
        self.w9_flush_bytes = int(_number('OCR_W9_FLUSH_MB', 80, float) * (1 << 20))    # slab bytes after which the pending reductions run (0: one at the end of the body); 80 MB: profiles/r04e
        self.tn_defer = _switch('OCR_TN_JOBS')              # pairs of plain weight-gradient products as one gemm_tn3 launch
        self.tn_side = _switch('OCR_TN_SIDE', False)             # ... on a side stream beside the main chain's short kernels
        # OCR_TN_NT_PAIR=0: the GEMM issued right behind the paired launch (conv5's data gradient) stays a launch of its own (default: it runs
        # inside that launch on the CUs the tiles leave idle where ocr_gemm_tn_jobs_nt_supported accepts — same bits, one launch less)
        self.tn_nt_pair = _switch('OCR_TN_NT_PAIR')
        self.side_stream = torch.cuda.Stream(device=self.device) if (self.tn_side and torch.device(self.device).type == 'cuda') else None
        self.group = group
        self.world = 1
        self._check_xcd_placement()
        self.force_allreduce = bool(_env('OCR_FORCE_ALLREDUCE'))   # exercise the RCCL call on a 1-rank group (tests)
        if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(group)
        if _env('OCR_FAKE_WORLD'):                      # single-GPU emulation of identical ranks (tests): see dist.allreduce_sum_
            self.world = _number('OCR_FAKE_WORLD', None)
            self.force_allreduce = True
        self.overlap_allreduce = _switch('OCR_OVERLAP_ALLREDUCE')
        # OCR_DP_GRAPH=1 (round 6, opt-in): the WHOLE data-parallel step as ONE hipGraph — the two bucket all-reduces are captured on the communication
        # stream (fork behind the late backward, join in front of the optimiser) instead of being issued by Python between three graphs: no graph
        # boundaries, no host enqueue between them.  Opt-in because a captured RCCL collective cannot be validated on more than one rank here; the
        # engine checks at start-up that a captured collective replays correctly on THIS group and falls back to the three-graph schedule otherwise.
        self.dp_graph = _env('OCR_DP_GRAPH', '0') == '1'
        # OCR_W9_DEFER=0: every 3x3 weight gradient reduces its slabs right behind its own kernel (five reduce launches per step
        # for the CRNN); default: one merged reduction per backward body (bit-identical sums)
        self.defer_w9 = _switch('OCR_W9_DEFER')
        # OCR_W9_PAIR=0: no slab kernel waits for the next layer's (default: a layer whose grid fills at most half the chip takes the
        # previous layer's workgroups into its own launch — same slabs, one launch less; _Conv3x3Op._plan_w9_pair)
        self.w9_pair = _switch('OCR_W9_PAIR')
        self.w9_defer_max_bytes = _number('OCR_W9_DEFER_MAX_MB', self.W9_DEFER_MAX_BYTES >> 20) << 20     # only consulted with OCR_W9_FLUSH_MB=0
        self.w9_ws_pool = {}          # layer key -> the largest slab workspace any plan asked for so far (shared by the plans)
        self.comm_stream = torch.cuda.Stream(device=self.device)
        self.dp_host_s = [0.0, 0.0, 0.0, 0.0, 0.0, 0]      # host enqueue seconds of the data-parallel schedule's phases + step count (train_step)
        self._pack_table = None                          # built by the first refresh_weights
        self._pack_table_host = None                     # its host copy (numpy PACK_DTYPE records)
        self._fault_hook = None                          # fault injection (tests): called with the plan in front of the drop-flag launch
        self._watch_pending = None                       # the watchdog's outstanding report (_watchdog)
        self.dropped_reports = 0                         # steps whose update the device dropped, as seen by report_wait
        self._lower(net)                                 # operators first: the parameter layout follows their EXECUTION order
        self._layout(net)
        self._init_params(cfg.RNG_SEED if seed is None else seed)
        self.split_op = 0                                # first op of the late layers (backward part 1 = ops[split_op:])
        if self.split_layer is not None:
            for i, op in enumerate(self.ops):
                if op.name == self.split_layer:
                    self.split_op = i
                    break
            # the exchange of [late_begin, n_total) starts after backward part 1 = ops[split_op:]: no operator of part 2 may own
            # a variable in that range (it would be written while RCCL reads it), none of part 1 a variable below it
            for i, op in enumerate(self.ops):
                for name, owner in self._owner.items():
                    if owner == op.name:
                        assert (self.offsets[name] >= self.late_begin) == (i >= self.split_op), (op.name, name)
        self.plans = {}
        if self.dp_graph and (self.world > 1 or self.force_allreduce):
            self.dp_graph = self._check_graph_collectives()
        self.training = False                            # set by the run bodies: dropout keeps everything outside training steps
        self.train_keep_prob = 0.5                       # what the reference feeds in training steps (train.py:126)
        # optimiser scalars live from the start (all zero until setup_optimizer): graphs captured before the optimiser exists read the
        # step counter — the dropout masks' salt — through the same pointer afterwards (they kept a dummy zero for ever)
        self.scalars = torch.zeros(ops.optim_scalar_count(), dtype=torch.float64, device=self.device)
        self.opt_ready = False
        self.graph_opt = None
        self.iteration = 0
        self.refresh_weights()
        staged = getattr(net, '_staged_arrays', None)
        if staged:
            self.load_arrays(staged)

    # ------------------------------------------------------------------ parameters
    _xcd_checked = False

    def _check_xcd_placement(self):
        """The persistent LSTM's default hand-off keeps a workgroup group inside one XCD's L2 and relies on the dispatcher
        placing workgroups with equal (id & 7) on the same XCD.  Verified once per process on the device itself; if it does
        not hold (another partition mode, a future driver) the kernels are switched to the placement-independent protocol."""
        if Engine._xcd_checked:
            return
        Engine._xcd_checked = True
        n = 256
        out = torch.zeros(2 * n, dtype=torch.int32, device=self.device)
        nat_call('ocr_probe_xcc', out.data_ptr(), n, 64, torch.cuda.current_stream(self.device).cuda_stream)
        xcc = out[:n].cpu().numpy()
        colocated = all(len(set(xcc[r::8].tolist())) == 1 for r in range(8))
        if not colocated:
            nat_call('ocr_set_lstm_proto', 0)

    def _layout(self, net):
        """Flat parameter / gradient layout [early rest | early regularised | late regularised | late rest] — layout.py."""
        lay = FlatLayout(net.param_specs.values(), ALIGN, order=[op.name for op in self.ops])
        self._owner = lay.owner
        self.specs, self.offsets, self.n_total = lay.specs, lay.offsets, lay.n_total
        self.split_layer, self.reg_range, self.late_begin = lay.split_layer, lay.reg_range, lay.late_begin
        dev = self.device
        self.params = torch.zeros(self.n_total, dtype=F32, device=dev)
        # the gradient buffer has a hidden tail of GUARD_PAD floats behind the n_total gradients: word 0 of it is the data-parallel DROP FLAG (1.0 when
        # a persistent LSTM launch of this rank's step timed out, ocr_guard_flag); it rides at the end of the late bucket's all-reduce, so after
        # the exchange it is > 0 on EVERY rank iff any rank raised it, and every rank's optimiser launch drops the same step (_optim_body)
        self._grads_store = torch.zeros(self.n_total + self.GUARD_PAD, dtype=F32, device=dev)
        self.grads = self._grads_store[:self.n_total]
        self.drop_flag = self._grads_store[self.n_total:self.n_total + 1]
        self.params_bf16 = torch.zeros(self.n_total, dtype=BF16, device=dev)

    GUARD_PAD = 64         # floats behind the gradients (256 B: the exchanged range stays 256-B granular)

    def offset(self, name):
        return self.offsets[name]

    def _view(self, flat, name):
        s = self.specs[name]
        n = int(np.prod(s.shape))
        o = self.offsets[name]
        return flat[o:o + n].view(s.shape)

    def param(self, name):
        return self._view(self.params, name)

    def grad(self, name):
        return self._view(self.grads, name)

    def shadow(self, name):
        return self._view(self.params_bf16, name)

    def _init_params(self, seed):
        self.params.copy_(init_host_parameters(self.specs, self.offsets, self.n_total, seed))

    def load_arrays(self, arrays):
        """{TF variable name: numpy array} -> parameters (shapes must match the TF layouts)."""
        for name, arr in arrays.items():
            t = torch.as_tensor(np.asarray(arr, np.float32))
            if tuple(t.shape) != tuple(self.specs[name].shape):
                raise ValueError('%s: shape %s does not match %s' % (name, tuple(t.shape), self.specs[name].shape))
            self.param(name).copy_(t)
        self.refresh_weights()

    def state_arrays(self):
        return {name: self.param(name).detach().cpu().numpy().copy() for name in self.specs}

    PACK_DTYPE = np.dtype([('type', '<i4'), ('R', '<i4'), ('Cc', '<i4'), ('lstm_units', '<i4'), ('ldin', '<i8'),
                           ('ldout', '<i8'), ('src', '<u8'), ('dst', '<u8'), ('n', '<i8'), ('block_start', '<i4'),
                           ('nblocks', '<i4')])       # == struct PackJob in csrc/stream_ops.hip (64 bytes)

    def _build_pack_table(self):
        # plain bf16 copies only of the variables some op reads through Engine.shadow (the 3x3 convolution weights — most of the
        # parameters — have their own packed layouts): a flat shadow of everything was 28 MB read + 14 MB written per step
        jobs, labels = [], []
        for op in self.ops:
            for name in op.shadow_params():
                n = int(np.prod(self.specs[name].shape))
                jobs.append(dict(type=3, src=self._view(self.params, name).reshape(-1), dst=self._view(self.params_bf16, name).reshape(-1), n=n))
                labels.append('bf16 shadow of ' + name)
        for op in self.ops:
            mine = op.pack_jobs()
            jobs.extend(mine)
            labels.extend([op.name] * len(mine))
        tab, blocks = self.pack_table(jobs)
        self.validate_pack_table(tab, blocks, labels)
        self._pack_table_host = tab                      # (the host copy: what the tests compare the operands' byte ranges with)
        self._pack_table = torch.from_numpy(tab.view(np.uint8).copy()).to(self.device)
        self._pack_njobs, self._pack_blocks = len(jobs), blocks

    @staticmethod
    def pack_job_blocks(j):
        """Workgroups a pack job (a dict as op.pack_jobs() returns it) gets: one per 64 x 64 tile of a transpose, else one per 256 work
        items up to a cap (the kernel's loops stride by the job's block count)."""
        t = j['type']
        if t == 0:
            return ((j['Cc'] + 63) // 64) * ((j['R'] + 63) // 64)
        if t == 1:
            return min((j['n'] + 255) // 256, 512)
        if t == 2:
            return min((j['R'] * j['Cc'] // 4 + 255) // 256, 512)
        if t == 4:
            return min((j['n'] + 255) // 256, 512)
        return min((j['n'] // 4 + 255) // 256, 2048)

    @staticmethod
    def pack_table(jobs):
        """Job dicts (src / dst: tensors or device addresses) -> (PACK_DTYPE records in the given order, total workgroups).  Pure host."""
        addr = lambda a: a.data_ptr() if hasattr(a, 'data_ptr') else int(a)
        tab = np.zeros(len(jobs), Engine.PACK_DTYPE)
        start = 0
        for i, j in enumerate(jobs):
            nb = Engine.pack_job_blocks(j)
            tab[i] = (j['type'], j.get('R', 0), j.get('Cc', 0), j.get('lstm_units', 0), j.get('ldin', 0), j.get('ldout', 0),
                      addr(j['src']), addr(j['dst']), j.get('n', 0), start, nb)
            start += nb
        return tab, start

    @staticmethod
    def validate_pack_table(tab, total_blocks, labels=None):
        """What pack_jobs_kernel (csrc/stream_ops.hip) takes for granted about its table, checked on the host copy (ocr_pack_jobs sees only a
        device pointer).  Raises ValueError naming the job (and labels[job], where given) and the rule; every rule is a line of the kernel:
          the job search  takes the last job whose block_start <= blockIdx.x and b = blockIdx.x - block_start: block_start must be the running
                          sum of nblocks from 0, every nblocks >= 1 (a job without blocks is never found), and the launch has total_blocks blocks;
          type 0          one block per 64 x 64 tile, b -> (b % ctiles, b / ctiles): fewer blocks than tiles leave tiles stale; reads
                          src[r * ldin + c], 16 bytes at once where ldin % 4 == 0; writes dst[perm(c) * R + r], 8 bytes at once where R % 4 == 0;
                          perm(c) = (u / 16) * 64 + g * 16 + u % 16 stays inside [0, Cc) only for Cc == 4 U and U % 16 == 0;
          type 1          four output channels per thread: n / 4 float4s of w[tap][ci][co], tap = idx / (Cout / 4) / Cin must stay below 9;
          type 2, 3       float4 loads and 8-byte stores only, no scalar path: every count and stride is a multiple of 4;
          type 4          out[perm(i)] = src[i] for i < n, fp32 to fp32.
        The grid-stride types (1 - 4) are correct for any nblocks >= 1."""
        if tab.dtype != Engine.PACK_DTYPE:
            raise ValueError('pack table: dtype is not Engine.PACK_DTYPE')
        if len(tab) < 1:
            raise ValueError('pack table: no jobs')
        start = 0
        for i, j in enumerate(tab):
            t = int(j['type'])
            R, Cc, U, ldin, ldout, n = (int(j[k]) for k in ('R', 'Cc', 'lstm_units', 'ldin', 'ldout', 'n'))
            src, dst, nb = int(j['src']), int(j['dst']), int(j['nblocks'])

            def need(ok, rule):
                if not ok:
                    raise ValueError('pack job %d (type %d)%s: %s' % (i, t, ' of ' + labels[i] if labels else '', rule))
            need(0 <= t <= 4, 'type is one of 0 .. 4')
            need(nb >= 1, 'nblocks >= 1')
            need(int(j['block_start']) == start, 'block_start is the running sum of nblocks')
            need(src != 0 and dst != 0, 'src and dst are non-null')
            src_align, dst_align = 16, 8
            if t == 0:
                need(R >= 1 and Cc >= 1, 'R, Cc >= 1')
                need(ldin >= Cc, 'ldin >= Cc')
                need(nb == ((Cc + 63) // 64) * ((R + 63) // 64), 'nblocks is the number of 64 x 64 tiles')
                if U > 0:
                    need(Cc == 4 * U and U % 16 == 0, 'Cc == 4 * lstm_units and lstm_units % 16 == 0')
                src_align = 16 if (ldin % 4 == 0 and Cc >= 4) else 4
                dst_align = 8 if R % 4 == 0 else 2
            elif t == 1:
                need(R >= 1 and Cc >= 4 and Cc % 4 == 0, 'Cin >= 1, Cout >= 4 and Cout % 4 == 0')
                need(n == 9 * R * Cc, 'n == 9 * Cin * Cout')
            elif t == 2:
                need(R >= 1 and Cc >= 4 and Cc % 4 == 0 and ldin % 4 == 0 and ldout % 4 == 0, 'Cc, ldin and ldout are multiples of 4')
                need(ldin >= Cc and ldout >= Cc, 'ldin >= Cc and ldout >= Cc')
            elif t == 3:
                need(n >= 4 and n % 4 == 0, 'n % 4 == 0 and n >= 4')
            else:
                need(U >= 16 and U % 16 == 0 and n == 4 * U, 'n == 4 * lstm_units and lstm_units % 16 == 0')
                src_align = dst_align = 4
            need(src % src_align == 0, 'src is %d-byte aligned' % src_align)
            need(dst % dst_align == 0, 'dst is %d-byte aligned' % dst_align)
            start += nb
        if start != int(total_blocks):
            raise ValueError('pack table: total_blocks %d is not the sum of nblocks %d' % (int(total_blocks), start))

    def refresh_weights(self):
        if self._pack_table is None:
            self._build_pack_table()
        ops.pack_jobs(self._pack_table, self._pack_njobs, self._pack_blocks)
        for op in self.ops:
            op.refresh()

    # ------------------------------------------------------------------ lowering
    def _lower(self, net):
        """Topological lowering of the plan reachable from 'logits' (a chain for the shipped models, a DAG with residual
        adds for deeper extractors).  Only data edges count: the second input of bi_lstm is the time_step_len slot."""
        table = {'conv': _conv_op, 'fc': _FcOp, 'max_pool': _PoolOp, 'reshape_squeeze': _ViewOp, 'dropout': _DropoutOp, 'bi_lstm': _BiLstmOp, 'lstm': _BiLstmOp,
                 'add': _AddOp, 'relu': _ReluOp, 'batch_norm': _BatchNormOp, 'avg_pool': _AvgPoolOp, 'concat': _ConcatOp,
                 'softmax': _SoftmaxOp}
        data_op = _InputOp(self)
        built = {}
        self.ops = []
        for nd in execution_order(net.get_output('logits')):
            if nd.op not in table:
                raise NotImplementedError('layer %r (%s) has no gfx950 lowering yet' % (nd.op, nd.name))
            ins = [data_op if i.op == 'input' else built[id(i)] for i in (nd.inputs if nd.op in ('add', 'concat') else nd.inputs[:1])]
            op = table[nd.op](self, nd, ins[0])
            op.inputs = ins
            op.key = '%02d:%s' % (len(self.ops), nd.name)
            for i in ins:
                i.grad_owner().consumers += 1
            self.ops.append(op)
            if nd.op == 'conv' and (nd.attrs['s_h'], nd.attrs['s_w']) != (1, 1):       # strided: stride-1 convolution + strided pick
                if nd.attrs['bn']:
                    raise NotImplementedError('%s: a strided convolution with batch norm is not lowered' % nd.name)
                sub = _SubsampleOp(self, nd, op)
                sub.name = nd.name + '/stride'
                sub.inputs, sub.key = [op], '%02d:%s/stride' % (len(self.ops), nd.name)
                op.consumers += 1
                self.ops.append(sub)
                op = sub
            built[id(nd)] = op
        if _switch('OCR_FUSE_ADD_RELU'):
            # residual blocks: add -> relu (the add's only consumer) as ONE pass forward, and one masked delivery per input backward
            for r in self.ops:
                a = r.prev
                if isinstance(r, _ReluOp) and isinstance(a, _AddOp) and a.consumers == 1:
                    a.relu, r.fused_into = True, a
                    a.consumers = r.consumers
                    for p in a.inputs:                 # a (BN, no ReLU) conv feeding only this add: mask applied inside its BN backward
                        if (isinstance(p, _ConvOp) and p.bn and not p.relu and p.consumers == 1 and p.kind != 'c1'
                                and a.inputs.count(p) == 1):
                            p.mask_from = a
                    # ... and the LAST such conv to execute also does the add + relu in its batch-norm apply pass
                    cands = [p for p in a.inputs if getattr(p, 'mask_from', None) is a]
                    if cands and len(a.inputs) == 2:
                        p = max(cands, key=lambda q: self.ops.index(q))
                        other = a.inputs[1] if a.inputs[0] is p else a.inputs[0]
                        if isinstance(other, _InputOp) or self.ops.index(other) < self.ops.index(p):
                            p.tail_into, a.fwd_by = (a, other), p
        if _switch('OCR_FUSE_CONV_POOL'):
            for b in self.ops:
                a = b.prev
                if (isinstance(b, _PoolOp) and isinstance(a, _Conv3x3Op) and a.relu and not a.bn and a.biased
                        and a.consumers == 1 and (b.kw_t, b.kh_f) in ((1, 2), (2, 2))):
                    a.pool_after = b
        if _switch('OCR_FUSE_BN_POOL'):
            # conv + batch norm + ReLU followed by the 1 x 2 max-pool over the feature axis as its only consumer (LSTM_train.py:32-33: conv4_2
            # -> pool): the batch-norm apply pass writes the pooled tensor too, and the batch-norm backward passes route the pool's gradient
            # themselves — no max-pool forward / backward launches, no full-resolution gradient tensor written and re-read twice
            for b in self.ops:
                a = b.prev
                if (isinstance(b, _PoolOp) and isinstance(a, _ConvOp) and a.bn and a.kind != 'c1' and a.consumers == 1
                        and a.tail_into is None and a.mask_from is None and (b.kw_t, b.kh_f) == (1, 2)):
                    a.bn_pool, b.bn_fused_into = b, a
        if self.fuse_conv1_pool:
            for a, b in zip(self.ops[:-1], self.ops[1:]):
                if (isinstance(a, _ConvOp) and a.kind == 'c1' and a.relu and isinstance(b, _PoolOp) and b.prev is a
                        and a.consumers == 1 and (b.kw_t, b.kh_f) == (2, 2)):
                    a.fused_pool, b.fused_into = b, a

    # ------------------------------------------------------------------ gradient delivery (residual graphs)
    def _scratch(self, sp, like):
        key = (tuple(like.shape), like.dtype)
        if key not in sp.scratch:
            sp.scratch[key] = torch.empty_like(like)
        return sp.scratch[key]

    def grad_dst(self, sp, producer):
        """Where a consumer's backward kernel should write d(loss)/d(producer output), plus a `finish` callback.
        Single-consumer producers (every tensor of the shipped chain) get their dy buffer directly; for a tensor with
        several consumers the first delivery writes it and later ones go through a scratch buffer + one add kernel."""
        d = producer.dy(sp)
        if d is None:
            return None, (lambda: None)
        owner = producer.grad_owner()
        if owner.consumers <= 1 or owner.key not in sp.dy_done:
            sp.dy_done.add(owner.key)
            return d, (lambda: None)
        tmp = self._scratch(sp, d)
        return tmp, (lambda: ops.eltwise(0, d, tmp, d))

    def grad_dst_acc(self, sp, producer, can_accumulate):
        """grad_dst for a consumer whose kernel can add into the destination itself: (dst, finish, accumulate)."""
        d = producer.dy(sp)
        if d is None:
            return None, (lambda: None), False
        owner = producer.grad_owner()
        first = owner.consumers <= 1 or owner.key not in sp.dy_done
        if first or not can_accumulate:
            dst, finish = self.grad_dst(sp, producer)
            return dst, finish, False
        return d, (lambda: None), True

    def deliver(self, sp, producer, grad, mask=None):
        """Pass-through gradient (add / relu backward): dy(producer) (+)= mask > 0 ? grad : 0."""
        d = producer.dy(sp)
        if d is None:
            return
        g = grad.view(d.shape)
        if mask is None and producer.mask_in_consumer:
            mask = producer.y(sp)
        owner = producer.grad_owner()
        first = owner.consumers <= 1 or owner.key not in sp.dy_done
        sp.dy_done.add(owner.key)
        if first:
            if mask is None:
                d.copy_(g)
            else:
                ops.eltwise(2, g, mask.view(d.shape), d)
        elif mask is None:
            ops.eltwise(0, d, g, d)
        else:
            ops.eltwise(4, g, mask.view(d.shape), d)        # d += mask > 0 ? g : 0

    def plan(self, N, W):
        key = (N, W)
        if key not in self.plans:
            self.plans[key] = ShapePlan(self, N, W)
        return self.plans[key]

    # ------------------------------------------------------------------ input binding
    def _bind(self, sp, data, seq_len, labels=None, labels_len=None):
        def as_i32(v):
            return v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, np.int32))
        sl = as_i32(seq_len)
        lab = ll = None
        if labels is not None:
            lab, ll = as_i32(labels), as_i32(labels_len)
            if lab.numel() > sp.labels.numel():
                raise ValueError('flat label vector longer than batch * max_label_len (%d)' % sp.labels.numel())
        ints = [t for t in (sl, lab, ll) if t is not None]
        if (torch.is_tensor(data) and data.is_cuda and data.dtype in (torch.uint8, F32) and data.is_contiguous()
                and data.numel() == sp.x.numel() and all(t.is_cuda and t.dtype == I32 and t.is_contiguous() for t in ints)
                and sl.numel() == sp.seq_len.numel() and (ll is None or ll.numel() == sp.labels_len.numel())):
            # device-resident batch (prefetching pipeline, bench): ONE kernel binds pixels (uint8 -> / 255, a quarter of the H2D
            # bytes) and the three int vectors.  Per-tensor copies were four blit kernels (hipMemcpyAsync D2D, ~5 us each, each
            # preceded by a queue barrier that left the GPU idle at the start of every step).
            ops.bind_batch(data, sp.x, sl, sp.seq_len, lab, sp.labels, ll, sp.labels_len)
            return
        if torch.is_tensor(data) and data.dtype == torch.uint8:
            ops.u8_to_unit_f32(data if data.is_cuda else data.to(self.device, non_blocking=True), sp.x)
            dsts, srcs = [sp.seq_len], [sl]
        else:
            x = torch.as_tensor(np.asarray(data, np.float32)) if not torch.is_tensor(data) else data
            dsts, srcs = [sp.x, sp.seq_len], [x, sl]
        if lab is not None:
            dsts += [sp.labels[:lab.numel()], sp.labels_len]
            srcs += [lab, ll]
        for d, t in zip(dsts, srcs):
            d.copy_(t, non_blocking=True)

    # ------------------------------------------------------------------ forward / backward bodies (capturable)
    def step_counter(self):
        """Device double counting the completed optimiser steps (scalars[6]) — the per-step salt of the dropout masks."""
        return self.scalars[6:7]

    def _forward(self, sp, training=False):
        self.training = training
        # the flat gradient buffer is cleared by the forward pass's first kernel where that is conv1 + pool (one launch less); else by a fill
        self._zero_pending = bool(training) and self.grads.numel() % 4 == 0 and _switch('OCR_FUSE_ZERO')
        if training and not self._zero_pending:
            self.grads.zero_()
        # likewise the fill of the persistent LSTM launches' hand-off blocks (OCR_FUSE_RINGFILL=0: every launch fills its own); a graph whose
        # first kernel is not conv1 + pool never consumes it and its LSTM launches prepare their blocks themselves
        sp.rings_ready, sp.rings_armed = set(), False
        self._ones_pending = sp.lstm_arena if (training and sp.lstm_arena is not None and _switch('OCR_FUSE_RINGFILL')) else None
        for op in self.ops:
            op.fwd(sp)
        self._ones_pending = None
        if self._zero_pending:
            self.grads.zero_()
            self._zero_pending = False

    def _loss_and_backward(self, sp, flush=True):
        sp.dy_done = set()
        sp.w9_pending = []
        sp.tn_pending = []
        sp.w9_held = None
        logits = self.ops[-1].y(sp)
        # loss = mean over the GLOBAL batch -> d loss / d cost_n = 1 / (N * world)   (network.py:655)
        scale = ocr_dist.loss_scale(sp.N, self.world)
        path = self.ctc_form_of(sp.C, sp.T, sp.N)[0]
        if path == 'fast':
            ops.ctc_loss_train(logits, self.ops[-1].dy(sp), scale, sp.labels, sp.labels_len, sp.seq_len, self.max_label_len,
                               sp.costs, blank=0)
        elif path == 'long':
            ops.ctc_loss_long(logits, sp.labels, sp.labels_len, sp.seq_len, self.max_label_len, blank=0, want_grad=False,
                              grad_ntc_bf16=self.ops[-1].dy(sp), scale=scale, workspace=sp.ctc_ws, costs=sp.costs)
        elif path == 'wide':
            ops.ctc_loss_wide(logits, sp.labels, sp.labels_len, sp.seq_len, self.max_label_len, blank=0, want_grad=False,
                              grad_ntc_bf16=self.ops[-1].dy(sp), scale=scale, workspace=sp.ctc_ws, costs=sp.costs)
        else:
            ops.ctc_loss(logits, sp.labels, sp.labels_len, sp.seq_len, self.max_label_len, blank=0, want_grad=True,
                         workspace=sp.ctc_ws, costs=sp.costs, grads=sp.ctc_grad)
            ops.tnc_to_ntc_bf16(sp.ctc_grad, self.ops[-1].dy(sp), scale)
        for op in reversed(self.ops[self.split_op:]):
            op.bwd(sp)
        self._flush_tn(sp)                  # (always: the exchange of the late gradients may follow this body)
        self._join_tn(sp)
        self._release_w9(sp)                # (always, like the plain products: nothing is held across an exchange or a graph boundary)
        if flush:
            self._flush_w9(sp)

    CTC_MAX_LABEL_LEN = 255

    def ctc_path_of(self, C, T):
        """Which CTC form a plan with T frames of C classes takes: 'fast' (ctc_fast_kernel's training form, S <= 64 with its tables in
        LDS), 'long' (ctc_long_kernel, one launch, labels up to 255), 'wide' (rows kernel + samples kernel, up to 16384 classes: only the
        shapes neither of those two kernels covers) or 'general' (one-wave kernel + transpose)."""
        if ops.ctc_train_supported(C, T, self.max_label_len):
            return 'fast'
        long_covers = ops.ctc_long_supported(C, T, self.max_label_len)
        if self.ctc_long and long_covers:
            return 'long'
        if self.ctc_wide and not long_covers and ops.ctc_wide_supported(C, T, self.max_label_len):
            return 'wide'
        return 'general'

    def ctc_form_of(self, C, T, N):
        """-> (path, workspace bytes, shape of the f32 gradient hand-off) of a plan with N samples of T frames of C classes: everything a
        plan allocates for its CTC loss and the step dispatches on."""
        path = self.ctc_path_of(C, T)
        if path == 'wide':          # no f32 hand-off: both of its kernels write the bf16 gradient themselves
            return path, ops.ctc_wide_workspace_bytes(C, self.max_label_len, T, N), (0,)
        # every other plan keeps the general kernel's workspace where that kernel covers the labels (it stops at 127 characters)
        ws_bytes = ops.ctc_workspace_bytes(self.max_label_len, T, N) if self.max_label_len <= 127 else 1
        if path == 'long':
            ws_bytes = max(ws_bytes, ops.ctc_long_workspace_bytes(C, self.max_label_len, T, N))
        return path, ws_bytes, (T, N, C)

    def ctc_path(self, N, W):
        sp = self.plan(N, W)
        return self.ctc_path_of(sp.C, sp.T)

    def _backward_early(self, sp):
        for op in reversed(self.ops[:self.split_op]):
            op.bwd(sp)
        self._flush_tn(sp)
        self._join_tn(sp)
        self._release_w9(sp)
        self._flush_w9(sp)

    def tn_push(self, sp, job, keep, fallback, nt=None):
        """A plain weight-gradient product (X^T dY of conv5 / of the BiLSTM cells) joins the pending list; TWO of them go out as ONE launch of
        the ping-pong kernel (csrc/gemm_tn3.hip: no split over the contraction, no atomics).  `keep`: tensors the descriptor points into;
        `fallback`: the product as its own launch (gemm_tn2), used when it stays alone — with a split over the pixels that kernel fills the
        chip better than 64-96 unsplit tiles would.  `nt`: (P, Q, out, M, N, K) of a plain GEMM the caller would issue right behind this
        call, independent of every pending product; returns True when that GEMM went out INSIDE the paired launch (the caller skips it)."""
        if not self.tn_defer or not ops.gemm_tn_jobs_supported([job]):
            fallback()
            return False
        sp.tn_pending.append((job, keep, fallback))
        if len(sp.tn_pending) == 2:
            return self._flush_tn(sp, nt)
        return False

    def _flush_tn(self, sp, nt=None):
        pend, sp.tn_pending = sp.tn_pending, []
        if len(pend) == 2:
            jobs = [pend[0][0], pend[1][0]]
            if nt is not None and self.tn_nt_pair and not self.tn_side and ops.gemm_tn_jobs_nt_supported(jobs, nt[3], nt[4], nt[5]):
                # the tiles of the two products hold 160 of 256 CUs for the whole launch; the GEMM's workgroups take the other 96
                ops.gemm_tn_jobs_nt(jobs, nt[0], nt[1], nt[2], M=nt[3], N=nt[4], K=nt[5])
                return True
            if self.tn_side:
                # the two plain weight-gradient products (47 us, operand-fill-bound on 160 of 256 CUs) are needed by the optimiser / the
                # exchange only: they run on a side stream beside the short kernels that follow on the main chain (conv5's data gradient,
                # col2im, conv4_2's batch-norm backward passes); _join_tn() at the end of the backward body
                main = torch.cuda.current_stream(self.device)
                self.side_stream.wait_stream(main)
                with torch.cuda.stream(self.side_stream):
                    ops.gemm_tn_jobs([pend[0][0], pend[1][0]])
                sp.tn_side_open = True
            else:
                ops.gemm_tn_jobs([pend[0][0], pend[1][0]])
        else:
            for _, _, fallback in pend:
                fallback()
        return False

    def _join_tn(self, sp):
        if sp.tn_side_open:
            torch.cuda.current_stream(self.device).wait_stream(self.side_stream)
            sp.tn_side_open = False

    W9_DEFER_MAX_BYTES = 192 << 20       # total slab bytes of a plan up to which the reductions are deferred (Infinity Cache: 256 MB;
                                         # the headline plan has 162 MB); OCR_W9_DEFER_MAX_MB overrides
    W9_JOB_DTYPE = np.dtype([('dw', '<u8'), ('part', '<u8'), ('dbias', '<u8'), ('cs_part', '<u8'), ('n4', '<i8'), ('slab4', '<i8'),
                             ('S', '<i4'), ('rows', '<i4'), ('Cout', '<i4'), ('block_start', '<i4')])   # == struct W9ReduceJob (wgrad9.hip)

    def w9_append(self, sp, job, ws):
        """A slab kernel has been launched: its reduction (job, blocks) joins the pending list, its workspace the flush accounting."""
        sp.w9_pending.append(job)
        sp.w9_pending_bytes += ws.numel()
        if self.w9_flush_bytes and sp.w9_pending_bytes >= self.w9_flush_bytes:
            self._flush_w9(sp)          # (knob OCR_W9_FLUSH_MB: reduce while the slabs are still in the Infinity Cache)

    def w9_hold(self, sp, key, x, dz, dw, db, ws):
        """Layer `key`'s slab kernel is not launched now: the next slab layer of this backward body takes its workgroups into its own launch
        (sp.w9_hold_for; _Conv3x3Op._conv_bwd).  Its reduction is NOT pending yet.  The one hazard of holding is a gradient that reaches the
        exchange or the optimiser unreduced, so every path that ends a body or builds a reduction table releases first (_release_w9)."""
        self._release_w9(sp)
        sp.w9_held = (key, x, dz, dw, db, ws)

    def _release_w9(self, sp):
        """A held slab kernel whose partner did not come: a launch of its own, exactly the one it would have been without pairing."""
        held, sp.w9_held = sp.w9_held, None
        if held is not None:
            _, x, dz, dw, db, ws = held
            job, nblk = ops.conv3x3_wgrad_deferred(x, dz, dw, db, ws)
            if job is not None:
                self.w9_append(sp, (job, nblk), ws)

    def _flush_w9(self, sp):
        """ONE launch for the slab reductions the 3x3 weight-gradient kernels of this backward body left pending (dw += sum of the
        slabs, db += column sums).  The job table depends only on the plan's buffers, so it is uploaded once — on the eager run
        that precedes every capture — and the captured graphs replay the launch with the same device table."""
        self._release_w9(sp)            # (a held kernel's slabs must exist before a table that may follow it is built)
        pend, sp.w9_pending = sp.w9_pending, []
        sp.w9_pending_bytes = 0
        if not pend:
            return
        raw = b''.join(job for job, _ in pend)
        ent = sp.w9_tables.get(raw)
        if ent is None:
            tab = np.frombuffer(raw, dtype=self.W9_JOB_DTYPE).copy()
            assert tab.itemsize == 64 and len(tab) == len(pend)
            start = 0
            for i, (_, nblk) in enumerate(pend):
                tab['block_start'][i] = start
                start += nblk
            dev = torch.from_numpy(tab.view(np.uint8).copy()).to(self.device)
            ent = sp.w9_tables[raw] = (dev, len(pend), start)
        ops.wgrad9_reduce_jobs(*ent)

    def _capture(self, fn):
        """hipGraph capture of fn() with Python's cyclic garbage collector paused: a collection that frees device tensors of
        an unreferenced engine (engine <-> op cycles) in the middle of a capture aborts the process."""
        import gc
        gc.collect()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        was = gc.isenabled()
        gc.disable()
        try:
            # thread_local: other threads keep issuing work while this one captures — the input pipeline's feeder thread (H2D copies
            # on its own stream) and, with several ranks, RCCL's watchdog; in the default global mode any of their calls may
            # invalidate the capture
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                fn()
        finally:
            if was:
                gc.enable()
        return g

    def _run_split(self, sp):
        """forward + loss + backward of the late layers as one graph, backward of the early layers as a second one (data-
        parallel runs: the exchange of the late gradients is issued between the two)."""
        def body1():
            self._forward(sp, training=True)
            self._loss_and_backward(sp)
            self._publish_guard(sp)

        def body2():
            self._backward_early(sp)

        if not self.use_graphs:
            body1()
            return body2
        if sp.graph_fb1 is None:
            body1(); body2()                                    # warm-up outside capture (also uploads the drop flag's address table)
            sp.graph_fb1, sp.graph_fb2 = self._capture(body1), self._capture(body2)
        sp.graph_fb1.replay()
        return sp.graph_fb2.replay

    def _check_graph_collectives(self):
        """Can a collective of this group be captured in a hipGraph and replayed?  One eager all-reduce (communicator set-up), then a captured one on
        the communication stream replayed twice: the buffer must hold world^2 x its start value.  Every rank must agree (an eager MIN all-reduce of
        the verdict), else nobody uses the captured schedule.  gloo (tests: ranks sharing one GPU, staged through the host) is never capturable."""
        import torch.distributed as dist
        fake = bool(_env('OCR_FAKE_WORLD'))
        if not fake:
            if not (dist.is_available() and dist.is_initialized()) or dist.get_backend(self.group) != 'nccl':
                return False
        ok = True
        try:
            t = torch.ones(256, dtype=F32, device=self.device)
            main = torch.cuda.current_stream(self.device)
            self.comm_stream.wait_stream(main)
            with torch.cuda.stream(self.comm_stream):
                ocr_dist.allreduce_sum_(t, self.group, force=self.force_allreduce)
            main.wait_stream(self.comm_stream)
            torch.cuda.synchronize()

            def body():
                cur = torch.cuda.current_stream(self.device)
                self.comm_stream.wait_stream(cur)
                with torch.cuda.stream(self.comm_stream):
                    ocr_dist.allreduce_sum_(t, self.group, force=self.force_allreduce)
                cur.wait_stream(self.comm_stream)
            g = self._capture(body)
            t.fill_(1.0)
            g.replay(); g.replay()
            torch.cuda.synchronize()
            w = float(self.world if (fake or self.world > 1) else 1)
            ok = bool(float(t[0]) == w * w and float(t[-1]) == w * w)
        except Exception as e:       # noqa: BLE001
            import sys
            sys.stderr.write('[engine] OCR_DP_GRAPH=1: a captured collective failed on this group (%s: %s) — three-graph schedule instead\n' % (type(e).__name__, e))
            ok = False
        if not fake and dist.get_world_size(self.group) > 1:
            v = torch.tensor([1.0 if ok else 0.0], device=self.device)
            dist.all_reduce(v, op=dist.ReduceOp.MIN, group=self.group)
            ok = bool(float(v[0]) == 1.0)
        return ok

    def _run_dp_graph(self, sp):
        """The whole data-parallel step of this shape as ONE hipGraph (OCR_DP_GRAPH=1): forward, CTC, backward of the late layers, the drop flag ->
        [communication stream: all-reduce of the late bucket] || backward of the early layers -> [communication stream: all-reduce of the early
        bucket] -> join -> clip + optimiser + re-pack.  Same kernels, same order, same two buckets as the three-graph schedule of train_step."""
        if not self.opt_ready:
            self.setup_optimizer()

        def exchange(lo, hi):
            cur = torch.cuda.current_stream(self.device)
            self.comm_stream.wait_stream(cur)
            with torch.cuda.stream(self.comm_stream):
                self.allreduce_grads(lo, hi)

        def body():
            self._forward(sp, training=True)
            self._loss_and_backward(sp)
            self._publish_guard(sp)
            exchange(self.late_begin, self.n_total)
            self._backward_early(sp)
            exchange(0, self.late_begin)
            torch.cuda.current_stream(self.device).wait_stream(self.comm_stream)
            self._optim_body(None)

        if sp.graph_dp is None:
            # warm-up outside capture: forward + backward only (lazy module loads) — the optimiser mutates state, its first run is the first replay
            self._guard_addrs(sp)                            # (the address table of the drop flag's words is uploaded here, outside the capture)
            self._forward(sp, training=True)
            self._loss_and_backward(sp)
            self._backward_early(sp)
            sp.graph_dp = self._capture(body)
        sp.graph_dp.replay()

    def _run_step(self, sp):
        """Whole training step of this shape as one hipGraph (no exchange between backward and optimiser on a single GPU: the
        graph boundary cost ~8 us of idle GPU per step).  Only the forward/backward part is warmed up eagerly — the optimiser
        mutates state, so its first execution is the first replay."""
        if not self.opt_ready:
            self.setup_optimizer()

        def fb():
            self._forward(sp, training=True)
            self._loss_and_backward(sp, flush=False)      # one merged weight-gradient reduction at the end of the whole backward
            self._backward_early(sp)

        if sp.graph_step is None:
            self._guard(sp)                              # (its address table is uploaded here, outside the capture)
            fb()

            def body():
                fb()
                self._optim_body(sp)
            sp.graph_step = self._capture(body)
        sp.graph_step.replay()

    def _run(self, sp, which):
        """Run (or capture-then-replay) the forward(+backward) body for this shape."""
        attr = 'graph_fb' if which == 'fb' else 'graph_fwd'

        def body():
            self._forward(sp, training=(which == 'fb'))
            if which == 'fb':
                self._loss_and_backward(sp, flush=False)
                self._backward_early(sp)
                self._publish_guard(sp)

        if not self.use_graphs:
            body()
            return
        g = getattr(sp, attr)
        if g is None:
            body()                                   # warm-up outside capture (lazy module loads)
            g = self._capture(body)
            setattr(sp, attr, g)
        g.replay()

    # ------------------------------------------------------------------ public API
    def forward(self, data, seq_len):
        """Inference forward; returns the logits [T, N, C] (time-major, as network.py:127-128)."""
        data_shape = data.shape
        sp = self.plan(data_shape[0], data_shape[1])
        self._bind(sp, data, seq_len)
        self._run(sp, 'fwd')
        return self.ops[-1].y(sp)

    def decode(self, data, seq_len, method='beam', beam_width=100, lexicon=None):
        """Decoded label lists with zeros dropped (what accuracy_calculation / decodeRes see).
        method='beam'   : the reference's decoder — tf.nn.ctc_beam_search_decoder(beam 100, merge_repeated=True), whose
                          blank is class C-1; class 0 is an ordinary symbol that sparse_to_dense/ignore_value=0 strip later
                          (network.py:656-657, training.py:32).
        method='greedy' : best path with blank 0.
        method='prefix' : the textbook CTC prefix search: the same beam search with blank 0 and merge_repeated=False.  Its prefixes are label
                          strings (no zero occurs in them); not the reference's decoder.  decode_lm is this search fused with a language
                          model or a constraint.
        method='lexicon': the likeliest string of `lexicon` (label lists, blank 0, or a lexicon.LexiconTrie built with blank 0) under CTC; [] for a
                          sample none of them fits.  With a LexiconTrie only the arg-min leaves the device, not the N x K cost matrix."""
        return self._decode(data, seq_len, method, beam_width, lexicon, None)

    def decode_lm(self, data, seq_len, lm, beam_width=100):
        """decode(method='prefix') with the search fused with `lm`, an automaton.LabelAutomaton over the classes (blank 0): a language model
        (LabelAutomaton.from_ngram) or a constraint (from_lexicon, from_pattern) steers the beam itself (ops.ctc_beam_lm) where
        rescoring.rerank only re-orders what the acoustic beam kept.  An automaton.SparseLabelAutomaton (from_backoff_ngram, from_lexicon: any
        alphabet up to 16384 classes) runs the wide kernel's fused search (ops.ctc_beam_lm_sparse) instead.  -> the best string per sample under log p_beam + automaton.score; [] for
        a sample for which the automaton accepts nothing in the beam.  (A method of its own: decode's signature is pinned.)"""
        return self._decode(data, seq_len, 'prefix', beam_width, None, self._check_lm(lm))

    @staticmethod
    def _check_lm(lm):
        if not isinstance(lm, (LabelAutomaton, SparseLabelAutomaton)):
            raise ValueError('lm must be an automaton.LabelAutomaton (got %s)' % type(lm).__name__)
        if lm.blank != 0:
            raise ValueError('blank 0, but the %s was built with blank %d' % (type(lm).__name__, lm.blank))
        return lm

    def _decode(self, data, seq_len, method, beam_width, lexicon, lm):
        if method == 'lexicon':
            if lexicon is None:
                raise ValueError("decode(method='lexicon') needs a lexicon")
            if isinstance(lexicon, LexiconTrie):
                best = self._score_trie(data, seq_len, lexicon, 0)[1].cpu().numpy()
                return [[int(v) for v in lexicon[b] if v != 0] if b >= 0 else [] for b in best]
            _, best, _, _ = self.score(data, seq_len, lexicon, blank=0)
            return [[int(v) for v in lexicon[b] if v != 0] if b >= 0 else [] for b in best]
        sp = self.plan(data.shape[0], data.shape[1])
        self._bind(sp, data, seq_len)
        self._run(sp, 'fwd')
        logits = self.ops[-1].y(sp)
        if method == 'greedy':
            out, lens = ops.ctc_greedy_decode(logits, sp.seq_len, blank=0, pad_value=0)
        elif method == 'prefix':
            paths, plens = self._prefix_search(logits, sp.seq_len, 1, beam_width, lm)[:2]
            out, lens = paths[:, 0], plens[:, 0]
        else:
            out, lens, _ = ops.ctc_beam_decode(logits, sp.seq_len, beam_width=beam_width, merge_repeated=True, pad_value=0)
        out = out.cpu().numpy()
        lens = lens.cpu().numpy()
        if lm is not None:
            lens = np.maximum(lens, 0)                    # -1: the automaton accepts nothing in this sample's beam
        return [[int(v) for v in out[i, :lens[i]] if v != 0] for i in range(out.shape[0])]

    @staticmethod
    def _prefix_search(logits, seq_len, top_paths, beam_width, lm):
        """The CTC prefix search (blank 0, no merge) on device logits, fused with the automaton `lm` when one is given
        -> (paths, lengths, neg_log_prob, count, lm_score or None)."""
        if lm is None:
            return ops.ctc_beam_nbest(logits, seq_len, top_paths, beam_width=beam_width, blank=0, merge_repeated=False, pad_value=0) + (None,)
        search = ops.ctc_beam_lm_sparse if isinstance(lm, SparseLabelAutomaton) else ops.ctc_beam_lm      # (the sparse entry at its default cutoff)
        paths, lens, nlp, lm_score, count = search(logits, seq_len, lm, top_paths, beam_width=beam_width, blank=0, pad_value=0)
        return paths, lens, nlp, count, lm_score

    SCORE_MAX_LABEL_LEN = 255

    def _pack_lexicon(self, lexicon):
        """Device int32 [K, Lmax] labels and [K] lengths of a list of label lists; packed once per lexicon object (the last one is kept)."""
        held = getattr(self, '_lexicon', None)
        if held is not None and held[0] is lexicon:
            return held[1], held[2]
        if len(lexicon) == 0:
            raise ValueError('empty lexicon')
        lens = np.array([len(l) for l in lexicon], np.int32)
        if lens.max() > self.SCORE_MAX_LABEL_LEN:
            raise ValueError('lexicon entry of %d labels (at most %d)' % (lens.max(), self.SCORE_MAX_LABEL_LEN))
        dense = np.zeros((len(lexicon), max(int(lens.max()), 1)), np.int32)
        for k, l in enumerate(lexicon):
            dense[k, :len(l)] = l
        labels, lengths = torch.from_numpy(dense).to(self.device), torch.from_numpy(lens).to(self.device)
        self._lexicon = (lexicon, labels, lengths)
        return labels, lengths

    def _score_trie(self, data, seq_len, trie, blank):
        """Device costs, best, best_cost, log_norm of a LexiconTrie from one forward pass."""
        if blank != trie.blank:
            raise ValueError('blank %d, but the LexiconTrie was built with blank %d' % (blank, trie.blank))
        sp = self.plan(data.shape[0], data.shape[1])
        self._bind(sp, data, seq_len)
        self._run(sp, 'fwd')
        return ops.ctc_score_trie(self.ops[-1].y(sp), sp.seq_len, trie)

    def score(self, data, seq_len, lexicon, blank=0):
        """CTC costs of every string of `lexicon` (a list of label lists in the training convention: blank 0, classes from 1) for every sample,
        from one forward pass: -> (costs [N, K] float32, +inf for a string the sample cannot emit; best [N] int32, -1 where none can;
        best_cost [N]; log_norm [N] = log sum_k exp(-costs)) as numpy arrays.  exp(-costs - log_norm[:, None]) is the posterior within
        the lexicon.  A lexicon.LexiconTrie in place of the list takes the prefix-tree route (ops.ctc_score_trie: up to 1048576 words, shared prefixes
        computed once); its blank must be `blank`.  A list always takes the per-candidate route."""
        return tuple(v.cpu().numpy() for v in self._score_device(data, seq_len, lexicon, blank))

    def _score_device(self, data, seq_len, lexicon, blank):
        """score's four results as device tensors: the prefix-tree route for a LexiconTrie, the per-candidate route for a list."""
        if isinstance(lexicon, LexiconTrie):
            return self._score_trie(data, seq_len, lexicon, blank)
        labels, lengths = self._pack_lexicon(lexicon)
        sp = self.plan(data.shape[0], data.shape[1])
        self._bind(sp, data, seq_len)
        self._run(sp, 'fwd')
        return ops.ctc_score(self.ops[-1].y(sp), sp.seq_len, labels, lengths, blank=blank)

    def nbest(self, data, seq_len, lexicon, k=5, blank=0):
        """The k likeliest strings of `lexicon` (a list of label lists or a lexicon.LexiconTrie, as score takes them) for every sample, from one
        forward pass: -> (index [N, k] int32 into the lexicon, best first; costs [N, k] float32; log_post [N, k] float32 = -costs - log_norm, the
        log-posterior within the lexicon; count [N] int32 = how many of the k slots hold a string the sample can emit) as numpy arrays.  Slots at
        and beyond count[n] hold -1 / +inf / -inf.  Ties go to the lower index.  The selection runs on the device (ops.ctc_topk): only these
        O(N k) values leave it, not the N x K cost matrix."""
        costs, _, _, log_norm = self._score_device(data, seq_len, lexicon, blank)
        return tuple(v.cpu().numpy() for v in ops.ctc_topk(costs, k, log_norm=log_norm))

    def decode_nbest(self, data, seq_len, lexicon, k=5):
        """decode(method='lexicon') with alternatives: per sample a list of count[n] <= k pairs (labels with zeros dropped, log-posterior within the
        lexicon), best first; [] for a sample none of the lexicon's strings fits.  The lexicon's blank is 0, as decode's."""
        index, _, log_post, count = self.nbest(data, seq_len, lexicon, k=k, blank=0)
        return [[([int(v) for v in lexicon[int(index[n, j])] if v != 0], float(log_post[n, j])) for j in range(int(count[n]))]
                for n in range(index.shape[0])]

    NBEST_MAX_K = 64            # ops.ctc_topk's limit

    def decode_nbest_beam(self, data, seq_len, k=5, beam_width=100, candidates=None, rescore=True):
        """The k likeliest strings per sample without a lexicon: the `candidates` (default k) best prefixes of the CTC prefix search (blank 0,
        merge_repeated=False, as decode(method='prefix')), from one forward pass.  -> per sample a best-first list of at most k triples
        (labels, log_prob, log_post).  k <= 64 and k <= candidates <= beam_width.
        rescore=True : every candidate is scored exactly on the device (ops.ctc_score, per sample) and the k cheapest are selected there
                       (ops.ctc_topk); log_prob = minus the exact CTC cost, in the units of score; log_post is normalised within the candidate
                       list; the order is by exact cost.  A prefix beyond 255 labels has no exact cost and drops out.
        rescore=False: log_prob is the beam's own score (a lower bound: the beam sums a subset of the string's alignments), log_post its
                       normalisation over the returned paths; the order is the beam's."""
        return self._nbest_beam(data, seq_len, k, beam_width, candidates, rescore, None)

    def decode_nbest_beam_lm(self, data, seq_len, lm, k=5, beam_width=100, candidates=None, rescore=True):
        """decode_nbest_beam with the search fused with `lm`, an automaton.LabelAutomaton (blank 0): the candidates come from ops.ctc_beam_lm, so
        only strings the automaton accepts are returned (a sample may get an empty list).  With rescore=True their exact acoustic costs are
        computed as in decode_nbest_beam and the automaton's score (lm_score) is subtracted on the device (ops.ctc_score_fuse) before
        ops.ctc_topk selects: log_prob = the exact acoustic log-probability plus automaton.score(labels), log_post is normalised within the
        candidate list, the logits never leave the device.  With rescore=False log_prob is the fused search's own score."""
        return self._nbest_beam(data, seq_len, k, beam_width, candidates, rescore, self._check_lm(lm))

    def _nbest_beam(self, data, seq_len, k, beam_width, candidates, rescore, lm):
        k, beam_width = int(k), int(beam_width)
        candidates = k if candidates is None else int(candidates)
        if not (1 <= k <= self.NBEST_MAX_K and k <= candidates <= beam_width):
            raise ValueError('decode_nbest_beam takes 1 <= k <= %d and k <= candidates <= beam_width (got k = %d, candidates = %d, beam_width = %d)'
                             % (self.NBEST_MAX_K, k, candidates, beam_width))
        logits = self.forward(data, seq_len)
        sp_len = self.plan(data.shape[0], data.shape[1]).seq_len
        paths, lens, nlp, count, lm_score = self._prefix_search(logits, sp_len, candidates, beam_width, lm)
        if rescore:
            width = max(min(int(paths.shape[2]), self.SCORE_MAX_LABEL_LEN), 1)
            costs, _, _, log_norm = ops.ctc_score(logits, sp_len, paths[:, :, :width].contiguous(), lens, blank=0, per_sample=True)
            if lm is not None:
                # fused cost = exact acoustic cost - lm_score, and its normaliser over the candidate list (an empty slot stays +inf)
                costs, _, _, log_norm = ops.ctc_score_fuse(costs, lm_score)
            index, cost, log_post, count = (v.cpu().numpy() for v in ops.ctc_topk(costs, k, log_norm=log_norm))
            log_prob = -cost
        else:
            nlp, count = nlp[:, :k].cpu().numpy(), np.minimum(count.cpu().numpy(), k)
            log_prob = -nlp.astype(np.float64)
            log_post = np.full(log_prob.shape, -np.inf)
            for n in range(log_prob.shape[0]):
                v = log_prob[n, :count[n]]
                if v.size:
                    log_post[n, :count[n]] = v - (v.max() + np.log(np.exp(v - v.max()).sum()))
            index = np.tile(np.arange(k, dtype=np.int32), (log_prob.shape[0], 1))
        paths, lens = paths.cpu().numpy(), lens.cpu().numpy()
        return [[([int(v) for v in paths[n, index[n, j], :lens[n, index[n, j]]]], float(log_prob[n, j]), float(log_post[n, j]))
                 for j in range(int(count[n]))] for n in range(paths.shape[0])]

    def evaluate(self, data, seq_len, labels, method='beam', beam_width=100, per_sample=False):
        """Character error rate and sequence accuracy of a batch from one forward pass, counted on the device: the batch is decoded as
        decode(method=...) decodes it ('beam', 'greedy' or 'prefix'), the decoded ids stay on the device, ops.edit_distance compares each sample
        with its own label labels[n] (a list of N label lists; class 0 dropped from both sides, as accuracy_calculation's ignore_value) and
        ops.edit_stats sums: four integers leave the device.  -> dict: exact (samples at distance 0), edits (sum of the distances),
        ref_chars (sum of the labels' counted lengths), counted, skipped (samples with a string beyond 255 characters: they count as wrong),
        accuracy = exact / N (= accuracy_calculation(labels, decode(...)) when nothing is skipped), cer = edits / ref_chars (nan when
        ref_chars is 0); with per_sample=True also distances: int32 [N] numpy, -1 for a skipped sample."""
        if method not in ('beam', 'greedy', 'prefix'):
            raise ValueError("evaluate takes method 'beam', 'greedy' or 'prefix' (got %r)" % (method,))
        N = data.shape[0]
        if len(labels) != N:
            raise ValueError('%d label lists for %d samples' % (len(labels), N))
        lens = np.array([len(l) for l in labels], np.int32)
        dense = np.zeros((N, max(int(lens.max()), 1)), np.int32)
        for n, l in enumerate(labels):
            dense[n, :len(l)] = l
        sp = self.plan(N, data.shape[1])
        self._bind(sp, data, seq_len)
        self._run(sp, 'fwd')
        logits = self.ops[-1].y(sp)
        if method == 'greedy':
            out, olens = ops.ctc_greedy_decode(logits, sp.seq_len, blank=0, pad_value=0)
        elif method == 'prefix':
            paths, plens, _, _ = ops.ctc_beam_nbest(logits, sp.seq_len, 1, beam_width=beam_width, blank=0, merge_repeated=False, pad_value=0)
            out, olens = paths[:, 0], plens[:, 0].contiguous()
        else:
            out, olens, _ = ops.ctc_beam_decode(logits, sp.seq_len, beam_width=beam_width, merge_repeated=True, pad_value=0)
        ref, ref_len = torch.from_numpy(dense).to(self.device), torch.from_numpy(lens).to(self.device)
        dist, _, ref_count = ops.edit_distance(out, olens, ref, ref_len, ignore=0, want_counts=True)
        edits, ref_chars, exact, counted = (int(v) for v in ops.edit_stats(dist.view(-1), ref_count).cpu().numpy())
        res = dict(exact=exact, edits=edits, ref_chars=ref_chars, counted=counted, skipped=N - counted, accuracy=exact * 1.0 / N,
                   cer=edits * 1.0 / ref_chars if ref_chars else float('nan'))
        if per_sample:
            res['distances'] = dist.view(-1).cpu().numpy()
        return res

    def decode_mbr(self, data, seq_len, candidates=16, beam_width=100):
        """Minimum-Bayes-risk decoding under the edit distance, from one forward pass: the `candidates` best prefixes of the CTC prefix search
        (ops.ctc_beam_nbest, blank 0, merge_repeated=False) are scored exactly (ops.ctc_score per sample, as decode_nbest_beam(rescore=True)),
        ops.edit_distance compares them with each other and ops.mbr_select picks the one with the least expected distance to the others under
        their posterior within the list.  Only O(N * candidates) values leave the device.  -> per sample (labels, expected_edits, log_post) of
        the selected candidate, log_post = -cost - log_norm; ([], inf, -inf) where no candidate is valid.  1 <= candidates <= beam_width <= 128."""
        candidates, beam_width = int(candidates), int(beam_width)
        if not (1 <= candidates <= beam_width <= ops.MBR_MAX_K):
            raise ValueError('decode_mbr takes 1 <= candidates <= beam_width <= %d (got candidates = %d, beam_width = %d)'
                             % (ops.MBR_MAX_K, candidates, beam_width))
        logits = self.forward(data, seq_len)
        sp_len = self.plan(data.shape[0], data.shape[1]).seq_len
        paths, lens, _, _ = ops.ctc_beam_nbest(logits, sp_len, candidates, beam_width=beam_width, blank=0, merge_repeated=False, pad_value=0)
        width = max(min(int(paths.shape[2]), self.SCORE_MAX_LABEL_LEN), 1)
        costs, _, _, log_norm = ops.ctc_score(logits, sp_len, paths[:, :, :width].contiguous(), lens, blank=0, per_sample=True)
        dist = ops.edit_distance(paths, lens, paths, lens)
        _, best, best_risk = ops.mbr_select(dist, costs)
        pick = best.clamp(min=0).long()
        rows = torch.arange(paths.shape[0], device=paths.device)
        sel_paths, sel_len, sel_cost = paths[rows, pick], lens[rows, pick], costs[rows, pick]
        best, best_risk, sel_paths, sel_len, sel_cost, log_norm = (v.cpu().numpy() for v in (best, best_risk, sel_paths, sel_len, sel_cost, log_norm))
        return [([int(v) for v in sel_paths[n, :sel_len[n]]], float(best_risk[n]), float(np.float32(-sel_cost[n]) - log_norm[n]))
                if best[n] >= 0 else ([], float('inf'), float('-inf')) for n in range(paths.shape[0])]

    @staticmethod
    def _spans_of(strings, start, end, score, path_cost):
        """Per sample the list of (label, start_frame, end_frame, confidence) of its string from ops.ctc_align's results (host arrays);
        confidence = exp(score / frames), the geometric mean of the character's probability over its frames.  [] where path_cost is +inf."""
        out = []
        for n, s in enumerate(strings):
            if not np.isfinite(path_cost[n]):
                out.append([])
                continue
            out.append([(int(c), int(start[n, j]), int(end[n, j]), float(np.exp(np.float64(score[n, j]) / (int(end[n, j]) - int(start[n, j]) + 1))))
                        for j, c in enumerate(s)])
        return out

    def _align_strings(self, logits, seq_len, strings, blank):
        """ops.ctc_align of one string per sample (label lists; None = nothing to align: no spans, path_cost +inf) on logits that are on the
        device already -> (spans, path_cost as numpy)."""
        lens = np.array([-1 if s is None else len(s) for s in strings], np.int32)
        if lens.max() > self.SCORE_MAX_LABEL_LEN:
            raise ValueError('label of %d characters (at most %d)' % (lens.max(), self.SCORE_MAX_LABEL_LEN))
        dense = np.zeros((len(strings), max(int(lens.max()), 1)), np.int32)
        for n, s in enumerate(strings):
            if s:
                dense[n, :len(s)] = s
        labels, lengths = torch.from_numpy(dense).to(self.device), torch.from_numpy(lens).to(self.device)
        start, end, score, cost = (v.cpu().numpy() for v in ops.ctc_align(logits, seq_len, labels, lengths, blank=blank))
        return self._spans_of([s or [] for s in strings], start, end, score, cost), cost

    def align(self, data, seq_len, labels, blank=0):
        """Where each character sits: the best (Viterbi) alignment of sample n's transcript labels[n] (a list of N label lists, blank `blank`)
        against its logits, from one forward pass.  -> (spans, path_cost): spans[n] = [(label, start_frame, end_frame, confidence), ...] with
        frames inclusive and confidence = exp(score / frames) in (0, 1], [] for a sample that cannot emit its label; path_cost [N] float32 numpy,
        minus the log-probability of the best path, +inf for such a sample."""
        if len(labels) != data.shape[0]:
            raise ValueError('%d label lists for %d samples' % (len(labels), data.shape[0]))
        strings = [[int(v) for v in l] for l in labels]
        logits = self.forward(data, seq_len)
        return self._align_strings(logits, self.plan(data.shape[0], data.shape[1]).seq_len, strings, blank)

    def decode_spans(self, data, seq_len, method='greedy', lexicon=None):
        """decode and align from the same forward pass (the logits stay on the device between the two): -> (strings as decode(method=...) returns
        them, spans as align returns them for those strings).  method 'greedy', 'prefix' or 'lexicon', all with blank 0; the reference's beam
        decoder ('beam') has blank C - 1 and its results are not aligned here."""
        return self._decode_spans(data, seq_len, method, lexicon, None)

    def decode_spans_lm(self, data, seq_len, lm):
        """decode_spans(method='prefix') with the search fused with the automaton.LabelAutomaton `lm`, as decode_lm: -> (decode_lm's strings, their
        spans); a sample for which the automaton accepts nothing has the string [] and no spans."""
        return self._decode_spans(data, seq_len, 'prefix', None, self._check_lm(lm))

    def _decode_spans(self, data, seq_len, method, lexicon, lm):
        if method not in ('greedy', 'prefix', 'lexicon'):
            raise ValueError("decode_spans takes method 'greedy', 'prefix' or 'lexicon' (got %r)" % (method,))
        if method == 'lexicon' and lexicon is None:
            raise ValueError("decode_spans(method='lexicon') needs a lexicon")
        logits = self.forward(data, seq_len)
        sp_len = self.plan(data.shape[0], data.shape[1]).seq_len
        if method in ('greedy', 'prefix'):
            # the decoded labels [N, T] and their lengths go from the decoder to the aligner as they are; a string beyond 255 characters has no spans
            if method == 'greedy':
                out, lens = ops.ctc_greedy_decode(logits, sp_len, blank=0, pad_value=0)
            else:
                paths, plens = self._prefix_search(logits, sp_len, 1, 100, lm)[:2]
                out, lens = paths[:, 0], plens[:, 0].contiguous()
            width = max(min(int(out.shape[1]), self.SCORE_MAX_LABEL_LEN), 1)
            start, end, score, cost = (v.cpu().numpy() for v in ops.ctc_align(logits, sp_len, out[:, :width].contiguous(), lens, blank=0))
            out, lens = out.cpu().numpy(), lens.cpu().numpy()
            if lm is not None:
                lens = np.maximum(lens, 0)                # -1: the automaton accepts nothing in this sample's beam (no spans either)
            strings = [[int(v) for v in out[i, :lens[i]] if v != 0] for i in range(out.shape[0])]
            return strings, self._spans_of(strings, start, end, score, cost)
        if isinstance(lexicon, LexiconTrie):
            if lexicon.blank != 0:
                raise ValueError('blank 0, but the LexiconTrie was built with blank %d' % lexicon.blank)
            best = ops.ctc_score_trie(logits, sp_len, lexicon)[1].cpu().numpy()
        else:
            labels, lengths = self._pack_lexicon(lexicon)
            best = ops.ctc_score(logits, sp_len, labels, lengths, blank=0)[1].cpu().numpy()
        picked = [[int(v) for v in lexicon[b]] if b >= 0 else None for b in best]
        spans = self._align_strings(logits, sp_len, picked, 0)[0]
        return [[v for v in s if v != 0] if s is not None else [] for s in picked], spans

    def setup_optimizer(self, solver=None, lr=None):
        c = self.cfg.TRAIN
        self.solver = ops.SOLVERS.get(solver or c.SOLVER, 1)       # reference: anything else -> Momentum (train.py:76)
        self.lr = float(c.LEARNING_RATE if lr is None else lr)
        # slot initial values as TensorFlow creates them: Adam m = v = 0, Momentum accumulator 0, RMSProp "rms" slot = ONES
        # (tf.train.RMSPropOptimizer: the first steps are ~ lr * g / sqrt(0.9 + 0.1 g^2), not lr * sign(g) / sqrt(0.1))
        self.state1 = torch.ones_like(self.params) if self.solver == 2 else torch.zeros_like(self.params)
        self.state2 = torch.zeros_like(self.params) if self.solver == 0 else None
        self.scalars.zero_()                             # in place: captured graphs keep pointing at it
        ops.optim_init(self.scalars, self.lr)
        self.opt_ready = True
        self.graph_opt = None                            # captured optimiser graphs hold the old slot tensors
        for sp in self.plans.values():
            sp.graph_step = None
            sp.graph_dp = None

    def scale_lr(self, gamma):
        ops.optim_set_lr(self.scalars, gamma, multiply=True)
        self.lr *= gamma

    def _guard_on(self):
        return _switch('OCR_LSTM_TIMEOUT_GUARD')

    def _dp(self):
        return self.world > 1 or self.force_allreduce

    def _guard_addrs(self, sp):
        """Device addresses of the plan's persistent-LSTM error words (None: the plan has no persistent launch)."""
        if sp is None:
            return None
        g = sp._guard_addrs
        if g is None:
            words = sp.lstm_sync
            g = sp._guard_addrs = (torch.tensor([w[-1:].data_ptr() for w in words], dtype=torch.int64, device=self.device) if words else False)
        return g if g is not False else None

    def _guard(self, sp):
        """Single GPU: the error words themselves guard the update — a hand-off time-out inside the step drops the step's update on the device
        instead of applying a garbage gradient (ocr_optim_step_guarded2; the report, one step later, logs it: report_wait).  With several ranks
        every replica has to drop the SAME step: there the words are folded into the drop flag that rides on the late bucket (_publish_guard)."""
        if sp is None or self._dp() or not self._guard_on():
            return None
        return self._guard_addrs(sp)

    def _publish_guard(self, sp):
        """Data parallel: one tiny launch at the end of the backward graph that holds the LSTM (both error words are final there) writes this
        rank's 1.0 / 0.0 into the drop flag — the word right behind the late bucket, which the all-reduce that follows sums over the ranks."""
        if self._fault_hook is not None:                   # fault injection (tests): runs between the LSTM launches and the flag launch
            self._fault_hook(sp)
        if self._dp() and self._guard_on():
            ops.guard_flag(self._guard_addrs(sp), self.drop_flag)

    def _optim_body(self, sp=None):
        c = self.cfg.TRAIN
        if self.solver == 0:
            b1, b2, eps = 0.9, 0.999, 1e-8
        elif self.solver == 1:
            b1, b2, eps = float(c.MOMENTUM), 0.0, 0.0
        else:
            b1, b2, eps = 0.9, 0.0, 1e-10
        ops.optim_step(self.params, self.grads, self.state1, self.state2, self.reg_range, float(c.WEIGHT_DECAY), 10.0,
                       self.solver, b1, b2, eps, self.scalars, guard=self._guard(sp),
                       drop_flag=self.drop_flag if (self._dp() and self._guard_on()) else None)
        self.refresh_weights()

    def optimizer_step(self, sp=None):
        """sp: the plan whose backward pass produced the gradients — its LSTM error words guard the update when the step runs eagerly on one GPU
        (the shared optimiser graph of the multi-graph schedules is plan-independent: it is guarded by the exchanged drop flag)."""
        if not self.opt_ready:
            self.setup_optimizer()
        if not self.use_graphs:
            self._optim_body(sp)
            return
        if self.graph_opt is None:
            # capture WITHOUT a warm-up run: the optimiser mutates state, so the first real step is the capture's replay
            self.graph_opt = self._capture(self._optim_body)
        self.graph_opt.replay()

    def allreduce_grads(self, lo=0, hi=None):
        """Data-parallel exchange: all-reduce (sum) of a range of the flat fp32 gradient buffer over RCCL/xGMI.  The 1/world
        factor is already folded into the CTC gradient hand-off, so the sum IS the global-batch mean gradient; the
        clip then sees the same global norm a single GPU would see at the global batch size."""
        if self.world > 1 or self.force_allreduce:
            hi = self.n_total if hi is None else hi
            if hi == self.n_total and self._guard_on():
                hi += self.GUARD_PAD              # the range that ends the buffer carries the drop flag (_publish_guard)
            if hi > lo:
                ocr_dist.allreduce_sum_(self._grads_store[lo:hi], self.group, force=self.force_allreduce)

    def train_step(self, data, labels, labels_len, seq_len, fetch_loss=True):
        """One optimisation step on a batch laid out as gen.py:41-67 produces it.  Returns the total loss
        (mean CTC cost of the local batch + L2 term) as a Python float when fetch_loss, else None.
        Data-parallel schedule: graph 1 (forward, CTC, backward of the late layers) -> the late gradients (one contiguous
        range, ~87 % of the bytes for the CRNN) are all-reduced on the communication stream WHILE graph 2 (backward of the early layers)
        runs -> the early gradients are all-reduced on the same stream -> join -> graph 3 (clip + optimiser + re-pack)."""
        sp = self.plan(data.shape[0], data.shape[1])
        self._bind(sp, data, seq_len, labels, labels_len)
        if (self.world > 1 or self.force_allreduce) and self.overlap_allreduce and self.split_op > 0 and self.dp_graph and self.use_graphs:
            self._run_dp_graph(sp)
        elif (self.world > 1 or self.force_allreduce) and self.overlap_allreduce and self.split_op > 0:
            main = torch.cuda.current_stream(self.device)
            pc = time.perf_counter
            t0 = pc()
            rest = self._run_split(sp)
            t1 = pc()
            self.comm_stream.wait_stream(main)
            with torch.cuda.stream(self.comm_stream):
                self.allreduce_grads(self.late_begin, self.n_total)
            t2 = pc()
            rest()                                       # backward of the early layers, concurrent with the exchange above
            t3 = pc()
            # the early bucket goes out on the SAME stream as the late one: both collectives of a step are issued from one ordering
            # domain, in the same order on every rank (two streams relied on ProcessGroupNCCL's internal ordering)
            self.comm_stream.wait_stream(main)
            with torch.cuda.stream(self.comm_stream):
                self.allreduce_grads(0, self.late_begin)
            main.wait_stream(self.comm_stream)
            t4 = pc()
            self.optimizer_step()
            t5 = pc()
            # host-side enqueue time of the five phases (seconds, summed; bench.py prints the per-step averages so that a scaling record
            # explains itself: a host-bound schedule shows here, not in the kernel profile)
            h = self.dp_host_s
            h[0] += t1 - t0; h[1] += t2 - t1; h[2] += t3 - t2; h[3] += t4 - t3; h[4] += t5 - t4; h[5] += 1
        elif self.world == 1 and not self.force_allreduce and self.use_graphs:
            self._run_step(sp)                            # single GPU: forward, backward and optimiser as ONE graph
        else:
            self._run(sp, 'fb')
            self.allreduce_grads()
            self.optimizer_step(sp)
        self.iteration += 1
        self.last_plan = sp
        if fetch_loss:
            return self.last_loss()
        if self.iteration % 64 == 0:          # even when nobody reads the loss: look at the persistent LSTM's time-out words
            self._watchdog()                  # every 64 steps — WITHOUT a host sync (the report of 64 steps ago is read if it has landed)
        return None

    def _watchdog(self):
        """Queue a report of this step into the watchdog's OWN slot and evaluate the one queued 64 steps ago (an event query, no wait):
        a persistent-LSTM time-out raises at most 64 steps late instead of costing a pipeline drain every 64 steps."""
        pending = self._watch_pending
        if pending is not None:
            if not pending[1].query():
                return                            # the 'watch' slot's copy is still in flight: keep that handle, queue nothing over it
            self.report_wait(pending, update_mirrors=False)      # a 64-steps-old report must not overwrite last_ctc / last_reg / last_gnorm
        self._watch_pending = self.report_async(_slot='watch')

    def last_loss(self):
        """Loss of the last step: mean CTC cost of the local batch + L2 term.  ONE tiny kernel gathers the mean cost, the
        optimiser's scalars and the persistent-LSTM time-out words into 4 doubles, ONE 32-byte D2H copy into pinned memory and ONE
        stream wait follow (four blocking .cpu() / .item() round trips cost ~0.1 ms per iteration of the training loop, which
        fetches the loss every step like the reference: train.py:130,139; four async copies were four blit kernels)."""
        return self.report_wait(self.report_async(_slot='sync'))

    REPORT_SLOTS = 4       # handles that may be outstanding at once (the training loop keeps one, OCR_LOSS_LAG = 1)

    def report_async(self, _slot=None):
        """Queue the report of the step that was just issued (kernel + 32-byte copy + event) and return a handle for report_wait().
        The training loop waits for it one iteration LATER, so the host never drains the queue between two steps.
        Slot ownership (a two-slot ring shared with the engine's own every-64-steps check let that check take the slot
        a pending handle still pointed at — one logged loss in 64 was the NEXT step's): handles rotate over REPORT_SLOTS slots that
        only this function hands out, a slot is reused only after REPORT_SLOTS - 1 further handles were issued and its previous
        handle was waited for (checked), and the synchronous last_loss() and the watchdog each have a slot of their own."""
        sp = self.last_plan
        words = sp.lstm_sync
        ring = sp._report
        if ring is None:
            addrs = torch.tensor([w[-1:].data_ptr() for w in words], dtype=torch.int64, device=self.device) if words else None
            mk = lambda: [torch.zeros(4, dtype=torch.float64, device=self.device), torch.zeros(4, dtype=torch.float64).pin_memory(),
                          torch.cuda.Event(), False]                      # [device block, pinned host block, event, handle outstanding]
            ring = sp._report = dict(addrs=addrs, i=0, slots=[mk() for _ in range(self.REPORT_SLOTS)], sync=mk(), watch=mk())
        if _slot is None:
            ring['i'] = (ring['i'] + 1) % self.REPORT_SLOTS
            slot = ring['slots'][ring['i']]
            if slot[3]:
                raise RuntimeError('report_async: %d reports are outstanding — call report_wait() on the older handles first'
                                   % self.REPORT_SLOTS)
        else:
            slot = ring[_slot]
        slot[3] = True
        dev, host, ev = slot[0], slot[1], slot[2]
        ops.step_report(sp.costs, self.scalars if self.opt_ready else None, ring['addrs'], dev)
        host.copy_(dev, non_blocking=True)
        ev.record(torch.cuda.current_stream(self.device))
        return (host, ev, words, self.opt_ready, slot)

    def report_wait(self, handle, update_mirrors=True):
        host, ev, words, opt_ready, slot = handle
        ev.synchronize()
        slot[3] = False
        ctc, reg2, gnorm, bits = (float(v) for v in host.numpy())
        reg = 0.5 * float(self.cfg.TRAIN.WEIGHT_DECAY) * reg2 if (self.cfg.TRAIN.WEIGHT_DECAY > 0 and opt_ready) else 0.0
        if update_mirrors:
            self.last_ctc, self.last_reg, self.last_gnorm = ctc, reg, gnorm if opt_ready else 0.0
        bits = int(bits)
        dropped, bits = bool(bits >> 40 & 1), bits & 0xFFFFFFFF
        if dropped:
            # THIS step's update was dropped on the device (the step's own scalars[72], exported by the report kernel — not a comparison of the global
            # counter: a second report covering the same step, or two dropped steps in a row, used to raise — ADVICE r5): parameters and moments are
            # intact on every rank, training goes on; the reported loss of that step is meaningless.  bits == 0 here means ANOTHER rank timed out.
            self.dropped_reports += 1
            bad = [i for i in range(len(words)) if (bits >> i) & 1]
            import sys
            sys.stderr.write('[engine] WARNING: %s reported an expired inter-workgroup wait; that step\'s update was dropped on the device%s, parameters intact\n'
                             % (('the persistent LSTM %s kernel' % ('forward', 'backward')[bad[0] % 2]) if bad else 'another rank\'s persistent LSTM kernel',
                                ' on every rank' if self._dp() else ''))
            return float('nan')
        if bits != 0:
            bad = [i for i in range(len(words)) if (bits >> i) & 1]
            # the sync block = group counters (64-word stride, at most 2 * ceil(N / 16) of them) | hand-off ring | error word: print the
            # counters only (the ring is hundreds of thousands of 0xFFFFFFFF words)
            w = words[bad[0]]
            raise NativeError('persistent LSTM %s kernel: inter-workgroup wait timed out (results invalid); group counters %s, error word %d'
                              % (('forward', 'backward')[bad[0] % 2], w[:64 * 16:64].tolist(), int(w[-1])))
        return ctc + reg

    def guard_counters(self):
        """(steps dropped by the guarded optimiser step, expired hand-off waits it saw) since setup_optimizer — two device doubles, one blocking read."""
        if not self.opt_ready:
            return 0, 0
        v = self.scalars[73:75].cpu().numpy()
        return int(v[0]), int(v[1])
