"""Time ocr_ctc_beam_decode at the product shape (T, N, C, K) = (63, 64, 64, 100), table kernel and forced wide kernel, on peaky and on
flat logits: 30 launches after 5 warm-ups between HIP events, one JSON line.  OCR_NATIVE_LIB=<another build's libocrhip.so> times that
library with the same script (profiles/r19_beam_ab.log)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstm_ctc_ocr_amd import _native as nat  # noqa: E402
from lstm_ctc_ocr_amd import ops  # noqa: E402

T, N, C, K = 63, 64, 64, 100
dev = torch.device("cuda:0")


def inputs(kind):
    rng = np.random.RandomState(7)
    if kind == "peaky":
        a = (rng.randn(T, N, C) * 3).astype(np.float32)
        a[rng.rand(T, N) < 0.3, C - 1] += 5.0
        a[rng.rand(T, N) < 0.3, 0] += 5.0
    else:
        a = rng.randn(T, N, C).astype(np.float32)
    return a


res = {"lib": os.environ.get("OCR_NATIVE_LIB", "tree"), "build_id": nat.build_id()}
for kind in ("peaky", "flat"):
    a = torch.tensor(inputs(kind), device=dev)
    il = torch.full((N,), T, dtype=torch.int32, device=dev)
    out = torch.empty((N, T), dtype=torch.int32, device=dev)
    lens = torch.empty(N, dtype=torch.int32, device=dev)
    nlp = torch.empty(N, dtype=torch.float32, device=dev)
    sz = ctypes.c_size_t(0)
    nat.call("ocr_ctc_beam_workspace_size", C, N, T, K, ctypes.byref(sz))
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    for engine, name in ((0, "table"), (2, "wide")):
        ops.set_beam_engine(engine)
        assert ops.ctc_beam_kernel_choice(C, K) == name

        def run():
            nat.call("ocr_ctc_beam_decode", a.data_ptr(), il.data_ptr(), C, N, T, K, 1, 0, out.data_ptr(), lens.data_ptr(),
                     nlp.data_ptr(), ws.data_ptr(), ws.numel(), nat.stream())
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        res["%s_%s_ms" % (kind, name)] = {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}
        res["%s_%s_check" % (kind, name)] = [int(lens.sum().item()), round(float(nlp.sum().item()), 3)]
ops.set_beam_engine(0)
print(json.dumps(res))
