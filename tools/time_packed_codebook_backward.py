"""Times the packed codebook backward pass (ops.packed_codebook_matmul_dx: k_cbpkdx_stream / k_cbpkdx_tiled, k_cbgrad_reduce;
ops.packed_codebook_centroid_grad: k_cbgrad_absmax, k_cbpkdc_stream / k_cbpkdc_tiled, k_cbdc_finish) against the byte-form
backward on the same labels held one per byte (nnc_cbmm_dx_f32 / nnc_cbmm_dc_f32) and against torch's dense backward on the
decoded float32 W (g @ W.T and x.T @ g; the centroid sum of that dW is left out), one JSON line per (shape, width, m,
implementation).

    python tools/time_packed_codebook_backward.py [--out FILE] [--baseline-lib PATH] [--quick]
    rocprofv3 --kernel-trace --stats -- python tools/time_packed_codebook_backward.py --profile     (or --pmc ..., a run of its own)

The yardstick is the byte-form backward.  ``--baseline-lib`` names a libnnc_hip.so built from the commit before the packed
backward, loaded beside the current one; without it the current library's entry points are used; the record's ``library`` says
which ("baseline" or "current").  Runs of the yardstick and of the packed calls alternate; the yardstick is measured five times
per case and the range of the five is the margin: ``target`` (m = 1 and 16 only) is "met" if the packed median is no more than
the yardstick's median plus that range, "missed" otherwise, for dx, dc and dx + dc.

Measurement as tools/time_packed_codebook_matmul.py: a sequence of calls captured in a HIP graph, HIP events around the replays,
a window of at least 0.2 s after a warm-up, cold (a rotation over distinct matrices spanning >= 1 GiB, four times the Infinity
Cache; at most 1024 matrices, the span is reported).  ``--profile`` times nothing: it makes 20 plain (uncaptured, warm) calls of the
four entry points, interleaved, at 5000 x 5000 and 4096 x 4096, both widths, m = 1 and 16, for a profiler to look at.
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
from tools.time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views  # noqa: E402

SHAPES = [("5000x5000", 5000, 5000), ("4096x4096", 4096, 4096), ("lenet300.dense1", 784, 300), ("gpt2.qkv", 768, 2304), ("gpt2.proj", 3072, 768)]
WIDTHS = [(4, 16), (2, 4)]                       # (bits, K)
MS = [1, 16, 256, 4096]
REPEATS = 5
BASE_SYMBOLS = ("nnc_cbmm_dx_workspace_bytes", "nnc_cbmm_dx_f32", "nnc_cbmm_dc_workspace_bytes", "nnc_cbmm_dc_f32", "nnc_last_error")


def _baseline(path):
    """The byte-form backward and its workspace queries from another build of the library (or from the current one)."""
    if path is None:
        return nat.load(), "current"
    L = ctypes.CDLL(os.path.abspath(path))
    for name in BASE_SYMBOLS:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L, "baseline"


def _check(L, rc):
    if rc != 0:
        raise RuntimeError(L.nnc_last_error().decode())


def _byte_dx(L, g, labels, centers, kdim, ncols):
    m = g.shape[0]
    dx = torch.empty(m, kdim, dtype=torch.float32, device=g.device)
    ws_bytes = int(L.nnc_cbmm_dx_workspace_bytes(m, kdim, ncols, 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device) if ws_bytes else None
    _check(L, L.nnc_cbmm_dx_f32(g.data_ptr(), m, kdim, labels.data_ptr(), 1, ncols, centers.data_ptr(), centers.numel(), dx.data_ptr(),
                                None if ws is None else ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream))
    return dx


def _byte_dc(L, x, g, labels, k, kdim, ncols):
    m = g.shape[0]
    dc = torch.empty(k, dtype=torch.float64, device=g.device)
    ws_bytes = int(L.nnc_cbmm_dc_workspace_bytes(m, kdim, ncols, 1, k))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device)
    _check(L, L.nnc_cbmm_dc_f32(x.data_ptr(), g.data_ptr(), m, kdim, labels.data_ptr(), 1, ncols, k, dc.data_ptr(), 1, ws.data_ptr(), ws_bytes,
                                torch.cuda.current_stream().cuda_stream))
    return dc


def run(out, baseline_lib, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base, base_name = _baseline(baseline_lib)
    _, cus = ops.device_info()
    for name, kdim, ncols in (SHAPES[:3] if quick else SHAPES):
        n = kdim * ncols
        rot_f = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * 4))))
        fbuf, fviews = _views(n * 4, rot_f, torch.float32, n, dev)
        for bits, k in WIDTHS:
            rot_u = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
            lbuf, lviews = _views(n, rot_u, torch.uint8, n, dev)
            lbuf.random_(0, k)
            centers = torch.randn(k, device=dev) * 0.05
            pbytes = ops.packed_nbytes(kdim, ncols, bits)
            rot_p = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / pbytes)))
            codes = [ops.pack_codes(lviews[i % rot_u], kdim, ncols, k, bits) for i in range(rot_p)]
            for i in range(rot_f):
                fviews[i].copy_(ops.gather(centers, lviews[i % rot_u]))
            xc, gc = torch.rand(3, kdim, device=dev), torch.randn(3, ncols, device=dev) * 1e-2   # the implementations see the same matrix
            assert torch.equal(ops.packed_codebook_centroid_grad(xc, gc, codes[0]), _byte_dc(base, xc, gc, lviews[0], k, kdim, ncols))
            assert torch.allclose(ops.packed_codebook_matmul_dx(gc, codes[0], centers), _byte_dx(base, gc, lviews[0], centers, kdim, ncols),
                                  rtol=1e-4, atol=1e-6)
            for m in MS:
                if quick and m > 16:
                    continue
                x = torch.rand(m, kdim, device=dev)
                g = torch.randn(m, ncols, device=dev) * 1e-2
                fn = {"packed_dx": [(lambda i=i: ops.packed_codebook_matmul_dx(g, codes[i], centers)) for i in range(rot_p)],
                      "packed_dc": [(lambda i=i: ops.packed_codebook_centroid_grad(x, g, codes[i])) for i in range(rot_p)],
                      "byte_dx": [(lambda i=i: _byte_dx(base, g, lviews[i], centers, kdim, ncols)) for i in range(rot_u)],
                      "byte_dc": [(lambda i=i: _byte_dc(base, x, g, lviews[i], k, kdim, ncols)) for i in range(rot_u)]}
                t = {key: [] for key in fn}
                for r in range(REPEATS):                       # the two alternate
                    for key in ("byte_dx", "byte_dc"):
                        t[key].append(_time_graph(fn[key]))
                    if r < 3:
                        for key in ("packed_dx", "packed_dc"):
                            t[key].append(_time_graph(fn[key]))
                dxo, dwo = torch.empty(m, kdim, device=dev), torch.empty(kdim, ncols, device=dev)
                t_tdx = _time_graph([(lambda i=i: torch.matmul(g, fviews[i].view(kdim, ncols).t(), out=dxo)) for i in range(rot_f)])
                t_tdw = _time_graph([(lambda i=i: torch.matmul(x.t(), g, out=dwo)) for i in range(rot_f)])
                del dxo, dwo
                med = {key: statistics.median(v) for key, v in t.items()}
                spread = {key: max(t[key]) - min(t[key]) for key in ("byte_dx", "byte_dc")}
                dxp, dcp = ops.cbpk_dx_plan(m, kdim, ncols, bits, k, cus), ops.cbpk_dc_plan(m, kdim, ncols, bits, k, cus)
                common = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "bits": bits, "m": m, "state": "cold"}
                us = lambda s: round(s * 1e6, 3)   # noqa: E731
                pairs = [("dx", med["packed_dx"], med["byte_dx"], spread["byte_dx"]), ("dc", med["packed_dc"], med["byte_dc"], spread["byte_dc"]),
                         ("dx+dc", med["packed_dx"] + med["packed_dc"], med["byte_dx"] + med["byte_dc"], spread["byte_dx"] + spread["byte_dc"])]
                recs = []
                for what, tp, tb, sp in pairs:
                    rec = dict(common, impl="packed_" + what, us=us(tp), index_bytes=pbytes, rotation_span_mib=round(rot_p * pbytes / 2 ** 20, 1),
                               vs_byte=round(tb / tp, 3))
                    if what != "dx+dc":
                        rec["repeats_us"] = [us(v) for v in t["packed_" + what]]
                        plan = dxp if what == "dx" else dcp
                        rec["plan"] = {f: plan[f] for f in ("path", "vb", "mt", "cols", "copies", "splits", "col_tiles", "row_tiles")}
                    if m <= 16:
                        rec["target"] = "met" if tp <= tb + sp else "missed"
                    recs.append(rec)
                    brec = dict(common, impl="byte_" + what, library=base_name, us=us(tb), spread_us=us(sp), index_bytes=n,
                                rotation_span_mib=round(rot_u * n / 2 ** 20, 1))
                    if what != "dx+dc":
                        brec["repeats_us"] = [us(v) for v in t["byte_" + what]]
                    recs.append(brec)
                recs.append(dict(common, impl="torch_dx", us=us(t_tdx), index_bytes=4 * n, rotation_span_mib=round(rot_f * 4 * n / 2 ** 20, 1)))
                recs.append(dict(common, impl="torch_dw", us=us(t_tdw), index_bytes=4 * n))
                for rec in recs:
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
            del lbuf, lviews, codes
            torch.cuda.empty_cache()
        del fbuf, fviews
        torch.cuda.empty_cache()


def profile(baseline_lib):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base, _ = _baseline(baseline_lib)
    for _, kdim, ncols in SHAPES[:2]:
        for bits, k in WIDTHS:
            labels = torch.randint(0, k, (kdim * ncols,), device=dev).to(torch.uint8)
            codes = ops.pack_codes(labels, kdim, ncols, k, bits)
            centers = torch.randn(k, device=dev) * 0.05
            for m in (1, 16):
                x, g = torch.rand(m, kdim, device=dev), torch.randn(m, ncols, device=dev) * 1e-2
                for _ in range(20):
                    ops.packed_codebook_matmul_dx(g, codes, centers)
                    _byte_dx(base, g, labels, centers, kdim, ncols)
                    ops.packed_codebook_centroid_grad(x, g, codes)
                    _byte_dc(base, x, g, labels, k, kdim, ncols)
                torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--baseline-lib", default=None, help="a libnnc_hip.so built from the commit before the packed backward: the byte-form yardstick")
    ap.add_argument("--quick", action="store_true", help="the first three shapes at m = 1 and 16 only")
    ap.add_argument("--profile", action="store_true", help="no timing: 20 plain calls of each entry point per case, for a profiler")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    with torch.no_grad():
        if a.profile:
            profile(a.baseline_lib)
        elif a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                run(f, a.baseline_lib, a.quick)
        else:
            run(None, a.baseline_lib, a.quick)


if __name__ == "__main__":
    main()
