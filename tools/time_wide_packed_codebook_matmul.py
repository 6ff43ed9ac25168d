"""Times the split-plane ("wide packed") codebook matmul (ops.wide_packed_codebook_matmul: k_cbwp_stream / k_cbwp_tiled / k_cbwp_mfma)
against the byte-form codebook matmul on the same labels, one JSON line per (shape, K, dtype, m, implementation).

    python tools/time_wide_packed_codebook_matmul.py [--out FILE] [--baseline-lib PATH] [--dtypes f32,bf16,fp16] [--quick]

The yardstick is nnc_cbmm_f32 (float32 x) / nnc_cbmm_h16 (half x) on the labels held one per byte (K <= 256) or per two bytes.
``--baseline-lib`` names a libnnc_hip.so built from the commit before the wide packed form, loaded beside the current one; without it
the current library's entry points are used; the record's ``library`` says which ("baseline" or "current").  The yardstick is measured
five times per case; its run-to-run spread is the range of those five and is the margin the new call is held to: ``target`` is "met"
if the wide packed time is no more than the yardstick's median plus that spread, "missed" otherwise.

Measurement as tools/time_codebook_matmul.py: a sequence of calls captured in a HIP graph, HIP events around the replays, a window of
at least 0.2 s after a warm-up.  m = 1 and 16 are measured cold (a rotation over distinct matrices spanning >= 1 GiB, four times the
Infinity Cache; at most 1024 matrices, the span is reported), m = 256 and 4096 warm (the same matrix every call).  ``index_tb_s`` is
the index bytes of the form per second.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neural_network_compression_amd import _native as nat  # noqa: E402
from neural_network_compression_amd import ops  # noqa: E402
from tools.time_codebook_matmul import MAX_ROT, COLD_SPAN, _time_graph, _views  # noqa: E402

SHAPES = [("4096x4096", 4096, 4096), ("5000x5000", 5000, 5000), ("lenet300.dense1", 784, 300)]
KS = [17, 33, 257]
MS = [(1, "cold"), (16, "cold"), (256, "warm"), (4096, "warm")]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
REPEATS = 5


def _baseline(path):
    """The byte form's entry points and workspace queries from another build of the library (or from the current one)."""
    if path is None:
        return nat.load(), "current"
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ("nnc_cbmm_workspace_bytes", "nnc_cbmm_f32", "nnc_cbmm_h16_workspace_bytes", "nnc_cbmm_h16", "nnc_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L, "baseline"


def _byte_call(L, x, labels, lb, centers, kdim, ncols):
    m = x.shape[0]
    y = torch.empty(m, ncols, dtype=x.dtype, device=x.device)
    half = x.dtype != torch.float32
    ws_bytes = int((L.nnc_cbmm_h16_workspace_bytes if half else L.nnc_cbmm_workspace_bytes)(m, kdim, ncols, lb))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    wsp, s = None if ws is None else ws.data_ptr(), torch.cuda.current_stream().cuda_stream
    if half:
        dt = ops._H16_DT[x.dtype]
        rc = L.nnc_cbmm_h16(x.data_ptr(), dt, m, kdim, labels.data_ptr(), lb, ncols, centers.data_ptr(), centers.numel(), None, 0, y.data_ptr(), dt, wsp, ws_bytes, s)
    else:
        rc = L.nnc_cbmm_f32(x.data_ptr(), m, kdim, labels.data_ptr(), lb, ncols, centers.data_ptr(), centers.numel(), None, 0, y.data_ptr(), wsp, ws_bytes, s)
    if rc != 0:
        raise RuntimeError(L.nnc_last_error().decode())
    return y


def run(out, baseline_lib, dtypes, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base, base_name = _baseline(baseline_lib)
    _, cus = ops.device_info()
    for name, kdim, ncols in (SHAPES[:1] if quick else SHAPES):
        n = kdim * ncols
        for k in KS:
            bits, lb = ops.wide_packed_bits(k), 1 if k <= 256 else 2
            rot_u = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * lb))))
            lbuf, lviews = _views(n * lb, rot_u, torch.uint8 if lb == 1 else torch.int16, n, dev)
            lbuf.random_(0, k)
            centers = torch.randn(k, device=dev) * 0.05
            wbytes = ops.wide_packed_nbytes(kdim, ncols, bits)
            rot_w = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / wbytes)))
            codes = [ops.pack_codes_wide(lviews[i % rot_u], kdim, ncols, k) for i in range(rot_w)]
            for dname in dtypes:
                tdt = DTYPES[dname]
                chk = torch.rand(3, kdim, device=dev).to(tdt)       # both implementations multiply the same matrix
                assert torch.allclose(ops.wide_packed_codebook_matmul(chk, codes[0], centers).float(),
                                      _byte_call(base, chk, lviews[0], lb, centers, kdim, ncols).float(), rtol=2e-2, atol=2e-2)
                for m, state in MS:
                    if quick and m == 4096:
                        continue
                    x = torch.rand(m, kdim, device=dev).to(tdt)
                    cold = state == "cold"
                    nw, nu = (rot_w, rot_u) if cold else (1, 1)
                    fn_w = [(lambda i=i: ops.wide_packed_codebook_matmul(x, codes[i % nw], centers)) for i in range(nw if cold else 16)]
                    fn_u = [(lambda i=i: _byte_call(base, x, lviews[i % nu], lb, centers, kdim, ncols)) for i in range(nu if cold else 16)]
                    t_u = [_time_graph(fn_u) for _ in range(REPEATS)]
                    t_w = [_time_graph(fn_w) for _ in range(REPEATS)]
                    u_med, spread, w_med = statistics.median(t_u), max(t_u) - min(t_u), statistics.median(t_w)
                    plan = ops.cbwp_plan(tdt, m, kdim, ncols, bits, k, cus)
                    common = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "bits": bits, "dtype": dname, "m": m, "state": state}
                    recs = [dict(common, impl="wide_packed", us=round(w_med * 1e6, 3), repeats_us=[round(t * 1e6, 3) for t in t_w], index_bytes=wbytes,
                                 index_tb_s=round(wbytes / w_med / 1e12, 4), rotation_span_mib=round(nw * wbytes / 2 ** 20, 1),
                                 vs_byte=round(u_med / w_med, 3), target="met" if w_med <= u_med + spread else "missed",
                                 plan={f: plan[f] for f in ("path", "vb", "mt", "cols", "splits", "col_tiles", "row_tiles")}),
                            dict(common, impl="byte", library=base_name, label_bytes=lb, us=round(u_med * 1e6, 3),
                                 repeats_us=[round(t * 1e6, 3) for t in t_u], spread_us=round(spread * 1e6, 3), index_bytes=n * lb,
                                 index_tb_s=round(n * lb / u_med / 1e12, 4), rotation_span_mib=round(nu * n * lb / 2 ** 20, 1))]
                    for rec in recs:
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()
            del lbuf, lviews, codes
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--baseline-lib", default=None, help="a libnnc_hip.so built from the commit before the wide packed form: the byte yardstick")
    ap.add_argument("--dtypes", default="f32,bf16", help="comma-separated activation types: f32, bf16, fp16")
    ap.add_argument("--quick", action="store_true", help="4096 x 4096 at m = 1, 16, 256 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    with torch.no_grad():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                run(f, a.baseline_lib, a.dtypes.split(","), a.quick)
        else:
            run(None, a.baseline_lib, a.dtypes.split(","), a.quick)


if __name__ == "__main__":
    main()
