"""The 3x3 convolution dispatch policy as a table: every host-only query of libocrhip.so that says which kernel a shape gets
(ocr_conv3x3_kernel_choice for each fused-pool window, _accum_supported, _pool_supported, _stats_rows, _bnbwd_rows) over a grid of
shapes and epilogue flags, under the default knobs and under each knob setting the parity tests force (the knobs are read once per
process: one child interpreter per setting).    python tests/golden/make_conv_plan_table.py   -> tests/golden/conv_plan_table.npz

tests/test_conv_dispatch_policy.py asks the library the same questions and wants the same answers, so a change to the selection code
that moves any shape onto another kernel (or refuses / accepts one more) shows without a GPU.  conv_ws sizes its grid by the device's
CU count and takes 256 (the MI355X's) without a device: the table holds on both."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_plan_table.npz")

EPI_BIAS, EPI_RELU, EPI_MASK, EPI_ACCUM = 1, 2, 16, 64
FLAG_SETS = (0, EPI_BIAS, EPI_BIAS | EPI_RELU, EPI_MASK, EPI_MASK | EPI_ACCUM, EPI_BIAS | EPI_RELU | EPI_MASK)
WINDOWS = ((0, 0), (1, 2), (2, 2), (2, 1))

# name -> knob environment: the default process, the seven convolution-generation settings of tests/test_gpu_kernels.py and the engines
SETTINGS = {
    "default": {},
    "k2A": dict(OCR_CONV_K2="1", OCR_K2_CFG="A"),
    "k2D": dict(OCR_CONV_K2="1", OCR_K2_CFG="D"),
    "k2A_nok3": dict(OCR_CONV_K2="1", OCR_K2_CFG="A", OCR_CONV_K3="0"),
    "k2D_nok3": dict(OCR_CONV_K2="1", OCR_K2_CFG="D", OCR_CONV_K3="0"),
    "nok2": dict(OCR_CONV_K2="0"),
    "ws2": dict(OCR_CONV_WS="2"),
    "ws0": dict(OCR_CONV_WS="0"),
    "engine0": dict(OCR_GEMM_ENGINE="0"),
    "engine2": dict(OCR_GEMM_ENGINE="2"),
    "engine3": dict(OCR_GEMM_ENGINE="3"),
}


def shapes():
    """(Nb, W, H, Cin, Cout) rows: the full grid, the workloads' layers, and shapes whose M * Cin * 2 crosses 2^31 (M still an int)."""
    import itertools
    grid = itertools.product((1, 4, 17, 32, 33, 64, 128), (16, 50, 62, 64, 80, 84, 128, 256), (1, 2, 3, 4, 8, 16, 30, 32),
                             (32, 64, 96, 128, 256, 512), (4, 64, 96, 128, 256, 512))
    layers = [(64, 128, 16, 64, 128), (64, 128, 16, 128, 64), (64, 64, 8, 128, 256), (64, 64, 8, 256, 128), (64, 64, 8, 256, 256),
              (64, 64, 4, 256, 512), (64, 64, 4, 512, 256), (64, 64, 4, 512, 512),                       # headline (batch 64, 32 x 256)
              (64, 80, 8, 256, 256), (64, 50, 4, 512, 512), (64, 80, 16, 64, 128), (64, 84, 16, 64, 128),   # variable width
              (32, 128, 16, 64, 64), (32, 64, 8, 128, 128), (32, 64, 4, 256, 256), (32, 64, 2, 512, 512),   # deep (configs[4])
              (32, 64, 8, 64, 128), (32, 64, 4, 128, 256), (32, 64, 2, 256, 512)]
    big = itertools.product((256, 512, 1024), (256,), (8, 16), (128, 256, 512), (64, 128, 512))
    rows = [r for r in list(grid) + layers + list(big) if r[0] * r[1] * r[2] < 2 ** 31]
    return np.array(rows, dtype=np.int32)


def query(S):
    """Answers of the loaded library (lstm_ctc_ocr_amd._native: OCR_NATIVE_LIB / OCR_GEMM_ENGINE apply) for the shapes S."""
    sys.path.insert(0, ROOT)
    from lstm_ctc_ocr_amd import _native as nat
    lib = nat.lib()
    kc, acc, ps, sr, br = (lib.ocr_conv3x3_kernel_choice, lib.ocr_conv3x3_accum_supported, lib.ocr_conv3x3_pool_supported,
                           lib.ocr_conv3x3_stats_rows, lib.ocr_conv3x3_bnbwd_rows)
    n = len(S)
    choice = np.zeros((n, len(FLAG_SETS), len(WINDOWS)), np.int8)
    stats = np.zeros((n, len(FLAG_SETS)), np.int32)
    accum = np.zeros(n, np.int8)
    pool = np.zeros((n, len(WINDOWS) - 1), np.int8)
    bnbwd = np.zeros(n, np.int32)
    for i, (Nb, W, H, Ci, Co) in enumerate(S.tolist()):
        for f, fl in enumerate(FLAG_SETS):
            for p, (kw, kh) in enumerate(WINDOWS):
                choice[i, f, p] = kc(Nb, W, H, Ci, Co, fl, kw, kh)
            stats[i, f] = sr(Nb, W, H, Ci, Co, fl)
        accum[i] = acc(Nb, W, H, Ci, Co)
        for p, (kw, kh) in enumerate(WINDOWS[1:]):
            pool[i, p] = ps(Nb, W, H, Ci, Co, kw, kh)
        bnbwd[i] = br(Nb, W, H, Ci, Co)
    return dict(choice=choice, accum=accum, pool=pool, stats=stats, bnbwd=bnbwd), nat.build_id()


def query_in_child(name, out_path, lib_path=None):
    """Runs query() in a fresh interpreter under SETTINGS[name] (no other OCR_ knob inherited) and saves its answers to out_path."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("OCR_")}
    env.update(SETTINGS[name])
    if lib_path:
        env["OCR_NATIVE_LIB"] = lib_path
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", out_path], env=env, cwd=ROOT)


def main():
    import tempfile
    S = shapes()
    with tempfile.TemporaryDirectory() as tmp:
        procs = {name: query_in_child(name, os.path.join(tmp, name + ".npz")) for name in SETTINGS}
        out = dict(shapes=S, flag_sets=np.array(FLAG_SETS, np.int32), windows=np.array(WINDOWS, np.int32))
        ids = set()
        for name, p in procs.items():
            if p.wait() != 0:
                raise SystemExit("child %s failed" % name)
            with np.load(os.path.join(tmp, name + ".npz")) as z:
                for k in z.files:
                    if k == "build_id":
                        ids.add(str(z[k]))
                    else:
                        out[name + "/" + k] = z[k]
    assert len(ids) == 1, ids
    out["build_id"] = np.array(ids.pop())
    out["settings"] = np.array(json.dumps(SETTINGS))
    np.savez_compressed(OUT, **out)
    print("%s: %d shapes x %d settings, %d bytes, library %s" % (OUT, len(S), len(SETTINGS), os.path.getsize(OUT), out["build_id"]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        res, bid = query(shapes())
        np.savez(sys.argv[2], build_id=np.array(bid), **res)
    else:
        main()
