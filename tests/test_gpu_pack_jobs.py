"""-m gpu: the one-launch weight re-pack (csrc/stream_ops.hip pack_jobs_kernel, what Engine.refresh_weights runs behind every optimiser update)
and the per-tensor pack kernels, bit for bit against the host model of every layout (tests/pack_model.py; pinned on the CPU by
tests/test_pack_model.py).  Every comparison is pack_model.check: non-NaN values bit for bit, NaNs stay NaNs.  No tolerance anywhere.

Kernel level.  All destinations of a launch are carved out of one bf16 arena filled with -7.0, 256 elements of it in front of, behind and
between them (a strided destination's other columns are poison too: the row gap is the case's own ldout - Cc); after the launch every word of
the arena is either a job's element and equals the model, or still poison.  Sources hold _plain_randoms with the edge values in the first and
last row and column, and NaN wherever the job has no business to read (past the columns of a strided matrix, the rows of a cell matrix that
belong to the other operand).

Branches reached, per job type (pack_model.py names the case for each):
  type 0  f32x4 loads (ldin % 4 == 0, c + 3 < Cc) and guarded scalar loads (odd ldin: every load; Cc % 4 != 0: the last column group);
          u32x2 stores (R % 4 == 0) and scalar stores (R % 4 != 0, with a last row group of 1, 2 and 3 rows); whole and partial tiles on
          both axes; one tile and 512 tiles; the gate permutation with U = 32, 256, 512; src as a row offset into a larger matrix.
  type 1  one block, less than one pass, 4.5 passes of the grid-stride loop; Cout / 4 a power of two and not.
  type 2  sub-block, ragged, 16 passes at the 512-block cap; ldout < ldin and > ldin; dst as a column offset into a wider matrix.
  type 3  one float4, a ragged last block, past the 2048-block cap.
  type 4  U = 32 (half a block), 256, 512.
  the job search  1 job; 24 jobs in both orders; 256, 257 and 300 jobs (thread t looks at jobs t and t + 256; the maximum over a wave and
          over the four waves), the first job with 512 blocks, the last with several.
Per-tensor kernels: pack_transpose (32 x 33 tile, f2bf stores) on every type-0 case and a (5, 6) matrix; pack_conv_dgrad on every type-1 case
and (5, 6) (Cout % 4 != 0); cast2d_bf16 on every type-2 case; cast_bf16 on every type-3 case and n = 30 (the f2bf tail); lstm_pack_bias on
every type-4 case.  Each equals the model and the job kernel's result.

Engine level.  For LSTM_train and the residual network with two stacked BiLSTMs, eagerly and under the captured step graph: every operand the
forward and backward kernels read (wpack, wdgrad, wxT, whT, wcat, wfcT, the packed bias, every bf16 shadow), named op class by op class
without looking at the ops' pack_jobs(), equals the model of the master parameter after construction, after three training steps (where it
must also have changed), after checkpoint save / restore into a second engine and after load_arrays of a state full of edge values; and the
byte ranges those operands cover are exactly the destination ranges of the engine's own pack table, so a pack added later cannot go unchecked.

Found on the MI355X: nothing wrong.  Every case, table and engine state matched the model bit for bit on the first run.  The tests were then run
against wrong builds: `tap` for `8 - tap` fails every type-1 case here (alone, per tensor, in the whole tables) and the engine tests; the
job search's max as a min fails the whole tables, the 256 / 257 / 300-job tables and the engine tests; _optim_body without its
refresh_weights fails the four engine tests after the training steps.  The type-0 store without its R % 4 guard was not run: it stores the
same four values with one 8-byte store at an address that is only 2- or 4-byte aligned, so it either gives the same bytes or faults; no
comparison of values can tell it from the kernel, and Engine.validate_pack_table holds the alignment the vector paths do need.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pack_model as pm  # noqa: E402

from lstm_ctc_ocr_amd import checkpoint, ops  # noqa: E402
from lstm_ctc_ocr_amd._native import NativeError  # noqa: E402
from lstm_ctc_ocr_amd.config import cfg  # noqa: E402
from lstm_ctc_ocr_amd.engine import Engine  # noqa: E402
from lstm_ctc_ocr_amd.engine_ops import _BiLstmOp, _Conv1Op, _Conv1x1Op, _Conv3x3Op, _ConvFullOp  # noqa: E402

BF = torch.bfloat16
_CACHE = {}


def _src_and_model(case, seed):
    """(source buffer, expected bits) of a case, computed once per session and never written to."""
    key = (case.id, seed)
    if key not in _CACHE:
        src = case.source(seed)
        _CACHE[key] = (src, case.model(src))
    return _CACHE[key]


class _Arena(object):
    """The sources of a list of (case, seed) in one device buffer, their destinations in one poisoned bf16 arena."""

    def __init__(self, dev, items):
        self.items = items
        self.soff, self.doff = [], []
        s, d = 0, pm.SLACK
        for case, _ in items:
            self.soff.append(s)
            s += (case.src_elems + 63) // 64 * 64                   # 256-byte granules: every source starts aligned
            d = (d + 7) // 8 * 8                                    # 16-byte granules
            self.doff.append(d)
            d += case.dst_elems * (case.dst_bits // 16) + pm.SLACK
        self.dst = torch.full((d,), pm.POISON, dtype=BF, device=dev)
        self.src = torch.empty(s, dtype=torch.float32, device=dev)
        self.load(0)

    def load(self, seed_shift):
        host = torch.full((self.src.numel(),), float('nan'))
        self.want = []
        for (case, seed), so in zip(self.items, self.soff):
            src, want = _src_and_model(case, seed + seed_shift)
            host[so:so + case.src_elems] = src
            self.want.append(want)
        self.src.copy_(host)

    def jobs(self, order=None):
        order = range(len(self.items)) if order is None else order
        return [self.items[i][0].job(self.src.data_ptr() + 4 * self.soff[i], self.dst.data_ptr() + 2 * self.doff[i]) for i in order]

    def launch(self, order=None):
        tab, blocks = Engine.pack_table(self.jobs(order))
        Engine.validate_pack_table(tab, blocks)
        table = torch.from_numpy(tab.view(np.uint8).copy()).to(self.dst.device)
        ops.pack_jobs(table, len(tab), blocks)
        torch.cuda.synchronize()
        return tab, blocks

    def per_tensor(self, i):
        """Item i by the per-tensor kernel of its layout."""
        case = self.items[i][0]
        sv = self.src[self.soff[i] + case.src_off:self.soff[i] + case.src_elems]
        words = case.dst_elems * (case.dst_bits // 16)
        dv = self.dst[self.doff[i]:self.doff[i] + words]
        if case.type == 0:
            ops.pack_transpose(sv, dv, lstm_units=case.U, R=case.R, Cc=case.Cc, ldin=case.ldin)
        elif case.type == 1:
            ops.pack_conv_dgrad(sv.view(3, 3, case.R, case.Cc), dv)
        elif case.type == 2:
            ops.cast2d_bf16(sv, case.ldin, dv[case.dst_off:], case.ldout, case.R, case.Cc)
        elif case.type == 3:
            ops.cast_bf16(sv, dv)
        else:
            ops.lstm_pack_bias(sv, None, dv.view(torch.float32), case.U, ndir=1)
        torch.cuda.synchronize()

    def read(self):
        return self.dst.view(torch.int16).cpu().numpy().view(np.uint16)

    def got(self, words, i):
        """Item i's written elements out of read()'s words, in model order."""
        case = self.items[i][0]
        w = words[self.doff[i]:self.doff[i] + case.dst_elems * (case.dst_bits // 16)]
        if case.dst_bits == 32:
            w = w.copy().view(np.uint32)
        return np.ascontiguousarray(case.written(w)).reshape(-1)

    def verify(self, what):
        """Every destination equals its model; every other word of the arena is poison.  Returns the per-item results."""
        words = self.read()
        free = np.ones(words.size, dtype=bool)
        out = []
        for i, (case, seed) in enumerate(self.items):
            g = self.got(words, i)
            pm.check("%s: job %d %s" % (what, i, case.id), g, self.want[i])
            n = case.dst_elems * (case.dst_bits // 16)
            f = free[self.doff[i]:self.doff[i] + n]
            if case.dst_bits == 32:
                f[:] = False
            else:
                case.written(f)[...] = False
            out.append(g)
        touched = np.flatnonzero(free & (words != pm.POISON_BF16))
        assert touched.size == 0, "%s: %d poisoned words written, first at arena word %d (destinations start at %s ...)" % (
            what, touched.size, int(touched[0]), self.doff[:4])
        assert int(free.sum()) >= pm.SLACK * (len(self.items) + 1)
        return out

    def untouched(self):
        return bool((self.read() == pm.POISON_BF16).all())


# ================================================================================================ a. each case alone
@pytest.mark.parametrize("case", pm.CASES, ids=lambda c: c.id)
def test_one_job_table(dev, case):
    a = _Arena(dev, [(case, 0)])
    assert a.untouched()
    a.launch()
    first = a.verify("first launch")[0]
    a.load(1)                          # another source into the same destination: the new values, not the old ones
    a.launch()
    second = a.verify("second launch")[0]
    assert (first != second).any()


# ================================================================================================ b. the per-tensor kernels
EXTRAS = [pm.EXTRA_TRANSPOSE, pm.Case(1, *pm.EXTRA_DGRAD_SHAPE, why='Cout % 4 != 0'), pm.Case(3, n=pm.EXTRA_CAST_N, why='n % 4 != 0')]


@pytest.mark.parametrize("case", pm.CASES + EXTRAS, ids=lambda c: c.id)
def test_per_tensor_kernel_equals_the_model_and_the_job_kernel(dev, case):
    a = _Arena(dev, [(case, 0)])
    a.per_tensor(0)
    one = a.verify("per-tensor kernel")[0]
    if case.type == 0 or case in pm.CASES:         # (the other two extras are what the job kernel does not take)
        b = _Arena(dev, [(case, 0)])
        b.launch()
        pm.check_same("per-tensor kernel against pack_jobs, " + case.id, one, b.verify("pack_jobs")[0], a.want[0])


# ================================================================================================ c. whole tables in one launch
@pytest.mark.parametrize("order", ["list", "reversed"])
def test_all_cases_in_one_launch(dev, order):
    """The destinations stay where they are; the TABLE lists the jobs in list order or reversed (other block ranges for every job)."""
    a = _Arena(dev, [(c, 0) for c in pm.CASES])
    idx = list(range(len(pm.CASES)))
    tab, blocks = a.launch(idx if order == "list" else idx[::-1])
    assert len(tab) == len(pm.CASES) and blocks > 4000
    a.verify("all cases, " + order)


def _long_table(njobs, first, last, seed0):
    return [(first, seed0)] + pm.small_jobs(njobs - 2, seed0 + 1) + [(last, seed0 + njobs)]


@pytest.mark.parametrize("njobs", [256, 257, 300])
def test_job_search_past_one_pass_of_256_threads(dev, njobs):
    """300: a 512-block transpose, 298 one-block jobs of mixed types, a six-block cast.  256 / 257: the same form around the boundary of
    what one pass of the search covers (job 256 is thread 0's second)."""
    first = pm.T0[-1] if njobs == 300 else pm.T0[2]
    items = _long_table(njobs, first, pm.T3[1], 1000 * njobs)
    a = _Arena(dev, items)
    tab, blocks = a.launch()
    assert len(tab) == njobs and int(tab['nblocks'][0]) == (512 if njobs == 300 else 6) and int(tab['nblocks'][-1]) == 6
    assert int((tab['nblocks'][1:-1] == 1).sum()) == njobs - 2
    got = a.verify("%d jobs" % njobs)
    # the small jobs do differ from their neighbours of the same kind: a block that took another job's record would show
    assert any((got[1] != got[4]).tolist()) and any((got[2] != got[5]).tolist()) and any((got[3] != got[6]).tolist())


# ================================================================================================ d. refusal
def test_empty_launches_are_refused_and_write_nothing(dev):
    a = _Arena(dev, [(pm.T3[1], 0)])
    tab, blocks = Engine.pack_table(a.jobs())
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    with pytest.raises(NativeError):
        ops.pack_jobs(table, 0, blocks)
    with pytest.raises(NativeError):
        ops.pack_jobs(table, len(tab), 0)
    torch.cuda.synchronize()
    assert a.untouched()


# ================================================================================================ engine level
def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == BF:
        return t.view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)
    assert t.dtype == torch.float32
    return t.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)


def _operands(eng):
    """[(label, device tensor or view, model bits)]: every packed operand and shadow of every op, from the op's class alone."""
    P = lambda name: eng.param(name).detach().cpu().numpy()
    out = []
    for op in eng.ops:
        if isinstance(op, _Conv1Op):
            assert not hasattr(op, 'wpack')                      # conv1's kernels read the fp32 master
        elif isinstance(op, _Conv3x3Op):
            w = P(op.name + '/weights')                          # [3][3][ci][co]
            out.append((op.name + ' wpack', op.wpack, pm.transpose(w.reshape(9 * op.ci, op.co))))
            if hasattr(op, 'wdgrad'):
                out.append((op.name + ' wdgrad', op.wdgrad, pm.conv_dgrad(w.reshape(9, op.ci, op.co))))
        elif isinstance(op, (_Conv1x1Op, _ConvFullOp)):          # (an FC is a 1x1 convolution)
            w = P(op.name + '/weights')
            out.append((op.name + ' wpack', op.wpack, pm.transpose(w.reshape(-1, op.co))))
            out.append((op.name + ' shadow', eng.shadow(op.name + '/weights'), pm.cast(w)))
        elif isinstance(op, _BiLstmOp):
            U, D = op.U, op.D
            for d, cell in enumerate(op.cells):
                w = P(cell + '/weights')                         # [D + U][4U], gate-major columns
                assert w.shape == (D + U, 4 * U)
                out.append(('%s wxT[%d]' % (op.name, d), op.wxT[d * 4 * U:(d + 1) * 4 * U], pm.transpose(w[:D], U)))
                out.append(('%s whT[%d]' % (op.name, d), op.whT[d], pm.transpose(w[D:], U)))
                out.append(('%s wcat[%d]' % (op.name, d), op.wcat[:, d * 4 * U:(d + 1) * 4 * U], pm.cast2d(w[:D], 4 * U)))
                out.append(('%s bias[%d]' % (op.name, d), op.bias[d * 4 * U:(d + 1) * 4 * U], pm.lstm_bias(P(cell + '/biases'), U)))
                out.append((cell + ' shadow', eng.shadow(cell + '/weights'), pm.cast(w)))
            if op.with_fc:
                w = P(op.fc + '/weights')
                out.append((op.name + ' wfcT', op.wfcT, pm.transpose(w)))
                out.append((op.fc + ' shadow', eng.shadow(op.fc + '/weights'), pm.cast(w)))
            else:
                assert op.wfcT is None
        else:
            assert op.pack_jobs() == [] and op.shadow_params() == [], op.name
    return out


def _merge(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def _view_ranges(t):
    e = t.element_size()
    if t.is_contiguous():
        return [(t.data_ptr(), t.data_ptr() + e * t.numel())]
    assert t.dim() == 2 and t.stride(1) == 1
    return [(t.data_ptr() + e * r * t.stride(0), t.data_ptr() + e * (r * t.stride(0) + t.shape[1])) for r in range(t.shape[0])]


def _table_ranges(tab):
    out = []
    for j in tab:
        t, dst, R, Cc, n = int(j['type']), int(j['dst']), int(j['R']), int(j['Cc']), int(j['n'])
        if t == 0:
            out.append((dst, dst + 2 * R * Cc))
        elif t == 2:
            out += [(dst + 2 * r * int(j['ldout']), dst + 2 * (r * int(j['ldout']) + Cc)) for r in range(R)]
        elif t == 4:
            out.append((dst, dst + 4 * n))
        else:
            out.append((dst, dst + 2 * n))
    return out


def _check_engine(eng, what):
    """Every operand equals the model of its master; the operands are exactly what the engine's pack table writes."""
    torch.cuda.synchronize()
    operands = _operands(eng)
    assert len(operands) >= 10
    for label, t, want in operands:
        pm.check("%s: %s" % (what, label), _bits(t), want)
    checked = _merge([r for _, t, _ in operands for r in _view_ranges(t)])
    Engine.validate_pack_table(eng._pack_table_host, eng._pack_blocks)
    assert len(eng._pack_table_host) == eng._pack_njobs
    assert (eng._pack_table.cpu().numpy().view(Engine.PACK_DTYPE) == eng._pack_table_host).all()
    assert checked == _merge(_table_ranges(eng._pack_table_host)), what + ": the pack table writes other bytes than the operands checked"
    return {label: _bits(t) for label, t, _ in operands}


def _batch(N, W, nclasses, seed):
    from test_gpu_engine import make_batch
    x, labels, ll, sl = make_batch(N, W, 2, 3, seed)
    return x, (labels % (nclasses - 2)) + 1, ll, sl


def _edge_state(eng):
    """The engine's state with the edge values in the first elements of every variable, and in the last (whT is made of a cell matrix's last
    rows, which the first elements do not reach)."""
    state = eng.state_arrays()
    for name, arr in state.items():
        flat = arr.reshape(-1)
        k = min(len(pm.EDGE), flat.size // 2)
        flat[:k] = pm.EDGE.numpy()[:k]
        flat[flat.size - k:] = pm.EDGE.numpy()[len(pm.EDGE) - k:]
    return state


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("which", ["LSTM_train", "residual_stacked"])
def test_engine_operands_are_the_model_of_the_master(dev, tmp_path, which, use_graphs):
    from lstm_ctc_ocr_amd import models
    old = (cfg.NCLASSES, cfg.TRAIN.NUM_LAYERS, cfg.TRAIN.WEIGHT_DECAY)
    try:
        cfg.TRAIN.WEIGHT_DECAY = 1e-5
        if which == "LSTM_train":
            make = lambda: models.get_network('LSTM_train')
            N, W, seed = 8, 88, 3
        else:
            cfg.NCLASSES, cfg.TRAIN.NUM_LAYERS = 96, 2

            class Tiny(models.RESNET_train):
                blocks, widths = (1, 1, 1, 1), (64, 128, 128, 256)
            make, N, W, seed = Tiny, 16, 96, 5
        eng = Engine(make(), device='cuda:0', seed=seed, use_graphs=use_graphs)
        before = _check_engine(eng, "after construction")
        # three training steps: the re-pack behind the optimiser (eager, or inside the captured step graph)
        x, labels, ll, sl = _batch(N, W, cfg.NCLASSES, 7)
        eng.setup_optimizer('Adam', 1e-3)
        for _ in range(3):
            eng.train_step(x, labels, ll, sl)
        after = _check_engine(eng, "after three training steps")
        same = [k for k in before if not (before[k] != after[k]).any()]
        assert not same, "operands the training steps did not change: %s" % same
        # checkpoint round trip into a second engine
        path = str(tmp_path / 'lstm_ctc_iter_3.ckpt')
        checkpoint.save(eng, path)
        eng2 = Engine(make(), device='cuda:0', seed=seed + 1, use_graphs=use_graphs)
        checkpoint.restore(eng2, path)
        restored = _check_engine(eng2, "after checkpoint.restore")
        assert sorted(restored) == sorted(after) and all((restored[k] == after[k]).all() for k in after)
        assert torch.equal(eng2.params.view(torch.int32), eng.params.view(torch.int32))
        # a state full of edge values (NaN, Inf, denormals, ties) through load_arrays
        eng2.load_arrays(_edge_state(eng2))
        edged = _check_engine(eng2, "after load_arrays of the edge values")
        assert bool(torch.isnan(eng2.params).any()) and all((edged[k] != restored[k]).any() for k in edged)
    finally:
        cfg.NCLASSES, cfg.TRAIN.NUM_LAYERS, cfg.TRAIN.WEIGHT_DECAY = old
