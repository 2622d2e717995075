"""Which kernel computes a 3x3 weight gradient — the host-only query ocr_conv3x3_wgrad_kernel_choice (the dispatchers' own decisions with
the launch cut off: wgrad9.hip w9_choose, gemm_tn2.hip tn2_plan, gemm_tn.hip tn_wgrad_plan), so that without a GPU
  - the policy of the headline step and of the configs[3] extremes is pinned (kernel and split count S),
  - the shape list of the GPU parity tests (tests/conv_shapes.py) is PROVEN to reach every kernel instance, under the default knobs and
    under every engine / knob setting tests/test_gpu_kernel_generations.py forces: a shape list that loses the last shape of an instance
    fails here, not silently on the GPU,
  - the refusals are seen to fall through to gemm_tn2 / gemm_tn."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_shapes as cs  # noqa: E402
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(nat.LIB_PATH), reason="libocrhip.so not built")

SLAB = {"wgrad9", "wgrad9p<4>", "wgrad9p<8>", "wgrad9p<4>/zero-row", "wgrad9p<8>/zero-row"}
ATOMICS = {"gemm_tn2/nine-tap", "gemm_tn2/paired-tap", "gemm_tn<1,4,4>", "gemm_tn<1,2,2>"}
PRODUCT = 64 * 20 * 4        # pixels of the smallest layer of a 64-image batch (configs[3], W = 80): "a product size" below


@pytest.fixture
def wgrad_engine():
    """Sets the weight-gradient engine for one test; afterwards the one the environment names, else the default (2)."""
    try:
        yield lambda e: nat.call("ocr_set_wgrad_engine", e)
    finally:
        nat.call("ocr_set_wgrad_engine", int(os.environ.get("OCR_WGRAD_ENGINE") or 2))


def test_names_cover_the_codes():
    assert set(ops.WGRAD_KERNEL_NAMES) == SLAB | ATOMICS and len(ops.WGRAD_KERNEL_NAMES) == 9
    assert nat.lib().ocr_conv3x3_wgrad_kernel_choice(0, 64, 4, 256, 512, 1, 0) < 0          # 0..8 | S << 8 are answers
    assert nat.lib().ocr_conv3x3_wgrad_kernel_choice(64, 64, 4, 252, 512, 1, 0) < 0         # channels % 8: the entry points refuse
    with pytest.raises(nat.NativeError):
        ops.conv3x3_wgrad_kernel_choice(64, 64, 4, 256, 0)


HEADLINE = [   # batch 64, 32 x 256 images: S halves as the channel tiles double (one workgroup per CU: S * Cin/64 * Cout/64 <= 256)
    ("conv2", 64, 128, 16, 64, 128, ("wgrad9", 64)),               # H = 16: no plane-layout instance
    ("conv3_1", 64, 64, 8, 128, 256, ("wgrad9p<8>", 32)),
    ("conv3_2", 64, 64, 8, 256, 256, ("wgrad9p<8>", 16)),
    ("conv4_1", 64, 64, 4, 256, 512, ("wgrad9p<4>", 8)),
    ("conv4_2", 64, 64, 4, 512, 512, ("wgrad9p<4>", 4)),
    # configs[3]: W = 80 and W = 320 padded batches
    ("conv2 W=80", 64, 40, 16, 64, 128, ("wgrad9", 64)),
    ("conv3_1 W=80", 64, 20, 8, 128, 256, ("wgrad9p<8>/zero-row", 16)),     # 20 columns, 16-column steps; M / 32 < 512: S = 16
    ("conv3_2 W=80", 64, 20, 8, 256, 256, ("wgrad9p<8>/zero-row", 16)),
    ("conv4_1 W=80", 64, 20, 4, 256, 512, ("wgrad9", 8)),                   # 20 columns < the 32-column step of H = 4
    ("conv4_2 W=80", 64, 20, 4, 512, 512, ("wgrad9", 4)),
    ("conv2 W=320", 64, 160, 16, 64, 128, ("wgrad9", 64)),
    ("conv3_1 W=320", 64, 80, 8, 128, 256, ("wgrad9p<8>", 32)),
    ("conv3_2 W=320", 64, 80, 8, 256, 256, ("wgrad9p<8>", 16)),
    ("conv4_1 W=320", 64, 80, 4, 256, 512, ("wgrad9p<4>/zero-row", 8)),     # 80 % 32 != 0
    ("conv4_2 W=320", 64, 80, 4, 512, 512, ("wgrad9p<4>/zero-row", 4)),
]


@pytest.mark.parametrize("layer,Nb,W,H,Ci,Co,want", HEADLINE)
def test_headline_layers_and_configs3_extremes(layer, Nb, W, H, Ci, Co, want):
    assert ops.conv3x3_wgrad_kernel_choice(Nb, W, H, Ci, Co) == want, layer
    S = want[1]
    assert ops.conv3x3_wgrad_workspace_bytes(Nb, W, H, Ci, Co) == S * (9 * Ci * Co + Co) * 4       # S slabs of dw + dbias


def _reached(choices, modes, product=False):
    """kernel -> shapes that take it in any of `modes` (product: only shapes of at least PRODUCT pixels)."""
    got = {}
    for m in modes:
        for s, (k, _) in zip(cs.CONV_SHAPES, choices[m]):
            if not product or s[0] * s[1] * s[2] >= PRODUCT:
                got.setdefault(k, []).append(s)
    return got


def test_parity_list_reaches_every_instance_by_default():
    ch = cs.wgrad_choices()
    ws, at = _reached(ch, ["workspace"]), _reached(ch, ["atomics", "splits2"])
    assert SLAB <= set(ws), "no shape of the parity list reaches %s" % (SLAB - set(ws))
    assert ATOMICS <= set(at), "no shape of the parity list reaches %s" % (ATOMICS - set(at))
    # ... and each at a product size (full-chip grids, the deepest split counts), not only at the small ragged ones
    assert SLAB <= set(_reached(ch, ["workspace"], True)) and ATOMICS <= set(_reached(ch, ["atomics", "splits2"], True))
    # an explicit split count never takes the slab kernels; no workspace neither
    assert not SLAB & set(at)
    assert all(S == 2 for _, S in ch["splits2"])
    # the comments of the list that name a weight-gradient kernel
    for s, (k, S) in cs.WGRAD_CLAIMS.items():
        got = ch["workspace"][cs.CONV_SHAPES.index(s)]
        assert got[0] == k and (S is None or got[1] == S), (s, got, (k, S))
    # the headline step's five layers are in the list
    for layer, s in cs.HEADLINE_WGRAD:
        assert s in cs.CONV_SHAPES, layer


def test_parity_list_reaches_the_older_engines_at_product_sizes(wgrad_engine):
    wgrad_engine(1)         # LDS-DMA per-tap tiles with atomics; register-staged where I, J % 128 != 0 or the split is refused
    ch = cs.wgrad_choices()
    assert ch["workspace"] == ch["atomics"]                                   # a workspace changes nothing: the atomics path
    assert set(_reached(ch, ["workspace", "splits2"], True)) == ATOMICS
    wgrad_engine(0)         # register-staged kernel only: both tile sizes
    ch = cs.wgrad_choices()
    assert ch["workspace"] == ch["atomics"]
    assert set(_reached(ch, ["workspace", "splits2"])) == {"gemm_tn<1,4,4>", "gemm_tn<1,2,2>"}
    assert set(_reached(ch, ["workspace"], True)) == {"gemm_tn<1,4,4>", "gemm_tn<1,2,2>"}
    for (k, _), s in zip(ch["workspace"], cs.CONV_SHAPES):
        assert k == ("gemm_tn<1,4,4>" if s[3] >= 128 and s[4] >= 128 else "gemm_tn<1,2,2>"), s


@pytest.mark.parametrize("env", ["OCR_W9_PLANES=0", "OCR_W9P_GENW=0", "OCR_W9P_GENW=2"])
def test_parity_list_under_the_read_once_knobs(env):
    """The knobs the GPU file forces in child processes, here in a child interpreter: what each setting moves, it moves at a product size and
    at a small ragged one, so the child's run of the parity tests does test the kernel it is there for."""
    base = cs.wgrad_choices()["workspace"]
    ch = cs.wgrad_choices_in_child(dict([env.split("=")]))
    got = ch["workspace"]
    assert ch["atomics"] == cs.wgrad_choices()["atomics"]                    # the atomics generations do not read these knobs
    assert [S for _, S in got] == [S for _, S in base]                       # nor does the slab plan
    moved = {}
    for s, (k0, _), (k1, _) in zip(cs.CONV_SHAPES, base, got):
        if k0 != k1:
            moved.setdefault((k0, k1), []).append(s)
    want = {"OCR_W9_PLANES=0": {(k, "wgrad9") for k in SLAB - {"wgrad9"}},
            "OCR_W9P_GENW=0": {("wgrad9p<4>/zero-row", "wgrad9"), ("wgrad9p<8>/zero-row", "wgrad9")},
            "OCR_W9P_GENW=2": {("wgrad9p<4>", "wgrad9p<4>/zero-row"), ("wgrad9p<8>", "wgrad9p<8>/zero-row")}}[env]
    assert set(moved) == want, moved
    for pair, shapes in moved.items():
        assert any(s[0] * s[1] * s[2] >= PRODUCT for s in shapes), (pair, shapes)
    if env == "OCR_W9_PLANES=0":
        assert not any(k.startswith("wgrad9p") for k, _ in got)
    if env == "OCR_W9P_GENW=2":                                              # the zero-row instances on whole-image shapes: the headline layers too
        for layer, s in cs.HEADLINE_WGRAD[1:]:
            assert got[cs.CONV_SHAPES.index(s)][0].endswith("/zero-row"), layer


def test_refusals_fall_through():
    c = ops.conv3x3_wgrad_kernel_choice
    assert c(64, 64, 4, 96, 128)[0] == "gemm_tn<1,2,2>"            # Cin % 64 != 0: no slab kernel; Cin % 128 != 0: no gemm_tn2 either
    assert c(64, 64, 4, 128, 192)[0] == "wgrad9p<4>"               # Cout % 64 == 0 is enough for the slab kernels ...
    assert c(64, 64, 4, 128, 192, workspace=False)[0] == "gemm_tn<1,4,4>"           # ... gemm_tn2 needs % 128
    assert c(64, 64, 4, 128, 200)[0] == "gemm_tn<1,4,4>"           # Cout % 64 != 0
    assert c(16, 64, 32, 128, 128)[0] == "gemm_tn2/nine-tap"       # H outside {2, 4, 8, 16}
    assert c(16, 64, 6, 128, 128)[0] == "gemm_tn2/nine-tap"
    assert c(128, 64, 1, 128, 128)[0] == "gemm_tn2/nine-tap"
    assert c(16, 64, 1, 128, 128)[0] == "gemm_tn<1,4,4>"           # ... and gemm_tn2 refuses what gives no XCD partition 12 K steps per workgroup
    assert c(1, 62, 8, 256, 512) == ("gemm_tn2/nine-tap", 1)       # M = 496 < 512 (gemm_tn2 from 256 rows)
    assert c(1, 30, 8, 256, 512)[0] == "gemm_tn<1,4,4>"            # M = 240: below gemm_tn2's 256 rows too
    assert c(512, 4, 4, 128, 128)[0] == "gemm_tn2/nine-tap"        # W * H = 16 < 32
    assert c(64, 64, 4, 256, 512, workspace=False) == ("gemm_tn2/nine-tap", 6)      # no workspace
    assert c(64, 64, 4, 256, 512, splits=2) == ("gemm_tn2/nine-tap", 2)             # explicit split count: honoured exactly, by the atomics kernels
    assert c(64, 64, 8, 128, 256, splits=3) == ("gemm_tn<1,4,4>", 3)                # ... by gemm_tn2 only where an XCD partition divides it (here 4 or 8 would)
    assert c(64, 128, 16, 64, 128, workspace=False) == ("gemm_tn2/paired-tap", 88)
    assert c(64, 128, 16, 64, 128, splits=2) == ("gemm_tn<1,2,2>", 2)
