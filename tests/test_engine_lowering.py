"""Host-side lowering (Engine._lower) of the reference DSL's graphs, no GPU: which fusions the plan records for which layer chains.
The kernels behind the fusions are covered by tests/test_gpu_kernels.py / test_gpu_engine.py; this file pins the PREDICATES."""
import pytest
import torch

from lstm_ctc_ocr_amd import engine_ops
from lstm_ctc_ocr_amd.config import cfg
from lstm_ctc_ocr_amd.engine import Engine, ShapePlan
from lstm_ctc_ocr_amd.models import get_network
from lstm_ctc_ocr_amd.network import Network


def _lower(net, **env):
    e = Engine.__new__(Engine)          # lowering only: no device memory, no native calls
    e.fuse_conv1_pool = True
    e.device = torch.device('cpu')
    e._lower(net)
    return {op.key.split(':', 1)[1]: op for op in e.ops}, e


class _BnNoReluPool(Network):
    """conv + batch norm WITHOUT ReLU followed by a 1 x 2 max-pool as the only consumer, then the reference's tail."""
    def __init__(self, relu):
        self.inputs = []
        self.data = self.placeholder('data', 'float32', [None, None, cfg.NUM_FEATURES])
        self.labels = self.placeholder('labels', 'int32', [None])
        self.time_step_len = self.placeholder('time_step_len', 'int32', [None])
        self.labels_len = self.placeholder('labels_len', 'int32', [None])
        self.keep_prob = self.placeholder('keep_prob', 'float32', [])
        self.layers = {'data': self.data, 'labels': self.labels, 'time_step_len': self.time_step_len, 'labels_len': self.labels_len}
        self.trainable = True
        (self.feed('data').conv_single(3, 3, 64, 1, 1, name='c1', c_i=1).max_pool(2, 2, 2, 2, padding='VALID', name='p1')
             .conv_single(3, 3, 64, 1, 1, name='cb', bn=True, relu=relu).max_pool(1, 2, 1, 2, padding='VALID', name='pb')
             .conv_single(3, 3, 64, 1, 1, name='cc', bn=True)
             .max_pool(1, 2, 1, 2, padding='VALID', name='pc').max_pool(1, 2, 1, 2, padding='VALID', name='pd')
             .conv_single(2, 2, 128, 1, 1, padding='VALID', name='c5', relu=False).reshape_squeeze_layer(d=128, name='rs'))
        self.feed('rs', 'time_step_len').bi_lstm(64, 1, name='logits')


def test_shipped_graph_fusions():
    ops, _ = _lower(get_network('LSTM_train'))
    assert ops['conv1'].fused_pool is ops['pool1'] and ops['conv2'].pool_after is not None and ops['conv3_2'].pool_after is not None
    assert ops['conv4_2'].bn_pool is ops['pool3'] and ops['conv4_1'].bn_pool is None
    assert ops['conv3_1'].pool_after is None and ops['conv2'].bn_pool is None


def test_bn_pool_fusion_predicate_with_and_without_relu():
    """the BN + 1 x 2 pool fusion does not ask for a ReLU — the relu flag travels with the layer into ocr_bn_train_fwd2 /
    bwd2 (tests/test_gpu_kernels.py::test_batchnorm* cover relu on and off with the pooled form) — and it is the ONLY form in which
    such a layer's backward sums are taken: the following layer's data gradient must not also deliver partial rows for it."""
    for relu in (True, False):
        ops, _ = _lower(_BnNoReluPool(relu))
        cb, cc = ops['cb'], ops['cc']
        assert cb.bn and cb.relu is relu and cb.bn_pool is ops['pb'] and ops['pb'].bn_fused_into is cb
        assert cc.bn_pool is ops['pc']                      # the first pool behind cc; the second one (pd) stays a pool launch
        assert getattr(ops['pd'], 'bn_fused_into', None) is None
        # the alloc-time rule of _Conv3x3Op.alloc (engine_ops._bnbwd_rows_allowed): a producer with bn_pool never gets partial rows from
        # its consumer's data gradient
        for p in (cb, cc):
            fusable_rows = engine_ops._bnbwd_rows_allowed(p)
            assert not fusable_rows


class _Graph(Network):
    """The reference's placeholders; `build(self)` strings the layers."""
    def __init__(self, build):
        self.inputs = []
        self.data = self.placeholder('data', 'float32', [None, None, cfg.NUM_FEATURES])
        self.labels = self.placeholder('labels', 'int32', [None])
        self.time_step_len = self.placeholder('time_step_len', 'int32', [None])
        self.labels_len = self.placeholder('labels_len', 'int32', [None])
        self.keep_prob = self.placeholder('keep_prob', 'float32', [])
        self.layers = {'data': self.data, 'labels': self.labels, 'time_step_len': self.time_step_len, 'labels_len': self.labels_len}
        self.trainable = True
        build(self)
        self.feed('rs', 'time_step_len').bi_lstm(64, 1, name='logits')


def test_one_class_per_convolution_family():
    ops, _ = _lower(get_network('LSTM_train'))
    assert type(ops['conv1']) is engine_ops._Conv1Op
    for name in ('conv2', 'conv3_1', 'conv3_2', 'conv4_1', 'conv4_2'):
        assert type(ops[name]) is engine_ops._Conv3x3Op, name
    assert type(ops['conv5']) is engine_ops._ConvFullOp
    assert [ops[n].kind for n in ('conv1', 'conv2', 'conv5')] == ['c1', '3x3', 'full']
    # "this layer computes a data gradient" is hasattr(op, 'wdgrad'): absent (not None) elsewhere
    assert hasattr(ops['conv2'], 'wdgrad') and not hasattr(ops['conv1'], 'wdgrad') and not hasattr(ops['conv5'], 'wdgrad')


def test_deep_model_uses_the_four_families(monkeypatch):
    """The model `bench.py --workload deep` builds (configs[4]): residual blocks with 1 x 1 projections."""
    monkeypatch.setattr(cfg, 'NCLASSES', 96)
    monkeypatch.setattr(cfg.TRAIN, 'NUM_LAYERS', 2)
    monkeypatch.setattr(cfg.TRAIN, 'NUM_HID', 1024)
    _, e = _lower(get_network('RESNET_train'))
    convs = [op for op in e.ops if isinstance(op, engine_ops._ConvOp)]
    assert len(convs) > 30
    fams = {'c1': engine_ops._Conv1Op, '3x3': engine_ops._Conv3x3Op, '1x1': engine_ops._Conv1x1Op, 'full': engine_ops._ConvFullOp}
    for op in convs:
        assert op.kind in fams and type(op) is fams[op.kind], (op.name, op.kind, type(op))
    assert {op.kind for op in convs} == set(fams)


# the expected texts are those of the single _ConvOp.__init__ this file's parent commit had
@pytest.mark.parametrize('build, message', [
    (lambda n: n.feed('data').conv_single(3, 3, 32, 1, 1, name='bad', c_i=1).reshape_squeeze_layer(d=128, name='rs'),
     'bad: the single-channel input conv is lowered for 3x3 SAME, 64 filters'),
    (lambda n: n.feed('data').conv_single(3, 3, 64, 1, 1, name='c1', c_i=1).conv_single(3, 3, 64, 1, 1, name='bad', c_i=48)
     .reshape_squeeze_layer(d=128, name='rs'),
     'bad: 3x3 conv needs C_in % 32 == 0 and C_out % 8 == 0'),
    (lambda n: n.feed('data').conv_single(3, 3, 64, 1, 1, name='c1', c_i=1).conv_single(1, 1, 12, 1, 1, name='bad')
     .reshape_squeeze_layer(d=128, name='rs'),
     'bad: 1x1 conv needs C_in % 8 == 0 and C_out % 8 == 0'),
    (lambda n: n.feed('data').conv_single(3, 3, 64, 1, 1, name='c1', c_i=1).conv_single(5, 5, 64, 1, 1, name='bad')
     .reshape_squeeze_layer(d=128, name='rs'),
     'bad: 5x5 SAME convolution is not lowered'),
], ids=['c1-32-filters', '3x3-cin-48', '1x1-cout-12', '5x5-same'])
def test_unsupported_convolutions_are_refused_with_the_same_words(build, message):
    with pytest.raises(NotImplementedError) as err:
        _lower(_Graph(build))
    assert str(err.value) == message


def test_shape_plan_declares_its_fields():
    sp = ShapePlan.__new__(ShapePlan)
    sp._init_fields(4, 88)
    assert (sp.N, sp.W) == (4, 88)
    assert sp.bn_stat_rows == {} and sp.bn_bwd_rows == {} and sp.fused_pools == set() and sp.lstm_sync_keys == ()
    assert sp.rings_ready == set() and sp.rings_armed is False and sp.w9_pending_bytes == 0 and sp.tn_side_open is False
    for name in ('graph_fb', 'graph_fwd', 'graph_fb1', 'graph_fb2', 'graph_dp', 'graph_step', '_guard_addrs', '_report', 'lstm_arena'):
        assert getattr(sp, name) is None, name
    assert sp.buf == {} and sp.shape == {} and sp.scratch == {} and sp.dy_done == set()
    assert sp.w9_pending == [] and sp.w9_tables == {} and sp.tn_pending == [] and sp.lstm_sync == ()
