"""Times the packed codebook matmul (ops.packed_codebook_matmul: k_cbpk_stream / k_cbpk_tiled / k_cbmm_reduce) against the
uint8 codebook matmul on the same labels and against torch.matmul on the decoded float32 weights, one JSON line per (shape,
width, m, implementation).

    python tools/time_packed_codebook_matmul.py [--out FILE] [--baseline-lib PATH] [--quick]

The yardstick is nnc_cbmm_f32 on the labels held one per byte.  ``--baseline-lib`` names a libnnc_hip.so built from the commit
before the packed form (the same kernel source, but not the library under test), loaded beside the current one; without it the
current library's nnc_cbmm_f32 is used; the record's ``library`` says which ("baseline" or "current").  The yardstick is
measured five times per case; its run-to-run spread is the range of those five and is the margin the packed call is held to:
``target`` is "met" if the packed time is no more than the yardstick's median plus that spread, "missed" otherwise.

Measurement as tools/time_codebook_matmul.py: a sequence of calls captured in a HIP graph, HIP events around the replays, a
window of at least 0.2 s after a warm-up.  m = 1 and 16 are measured cold (a rotation over distinct matrices spanning >= 1 GiB,
four times the Infinity Cache; at most 1024 matrices, the span is reported), m = 256 and 4096 warm (the same matrix every call).
``index_tb_s`` is the index bytes of the form (packed rows, or one byte per label) per second.
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

SHAPES = [("5000x5000", 5000, 5000), ("4096x4096", 4096, 4096), ("gpt2.qkv", 768, 2304), ("gpt2.fc", 768, 3072), ("gpt2.proj", 3072, 768)]
WIDTHS = [(4, 16), (2, 4)]                       # (bits, K)
MS = [(1, "cold"), (16, "cold"), (256, "warm"), (4096, "warm")]
REPEATS = 5


def _baseline(path):
    """nnc_cbmm_f32 and its workspace query from another build of the library (or from the current one)."""
    if path is None:
        return nat.load(), "current"
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ("nnc_cbmm_workspace_bytes", "nnc_cbmm_f32", "nnc_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L, "baseline"


def _u8_call(L, x, labels, centers, kdim, ncols):
    m = x.shape[0]
    y = torch.empty(m, ncols, dtype=torch.float32, device=x.device)
    ws_bytes = int(L.nnc_cbmm_workspace_bytes(m, kdim, ncols, 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    rc = L.nnc_cbmm_f32(x.data_ptr(), m, kdim, labels.data_ptr(), 1, ncols, centers.data_ptr(), centers.numel(), None, 0, y.data_ptr(),
                        None if ws is None else ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(L.nnc_last_error().decode())
    return y


def run(out, baseline_lib, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base, base_name = _baseline(baseline_lib)
    _, cus = ops.device_info()
    for name, kdim, ncols in (SHAPES[1:3] if quick else SHAPES):
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
            chk = torch.rand(3, kdim, device=dev)       # the three implementations multiply the same matrix
            assert torch.allclose(ops.packed_codebook_matmul(chk, codes[0], centers), _u8_call(base, chk, lviews[0], centers, kdim, ncols),
                                  rtol=1e-4, atol=1e-4)
            for m, state in MS:
                if quick and m == 4096:
                    continue
                x = torch.rand(m, kdim, device=dev)
                cold = state == "cold"
                np_, nu, nf = (rot_p, rot_u, rot_f) if cold else (1, 1, 1)
                fn_p = [(lambda i=i: ops.packed_codebook_matmul(x, codes[i % np_], centers)) for i in range(max(np_, 16) if not cold else np_)]
                fn_u = [(lambda i=i: _u8_call(base, x, lviews[i % nu], centers, kdim, ncols)) for i in range(max(nu, 16) if not cold else nu)]
                yt = torch.empty(m, ncols, device=dev)
                fn_t = [(lambda i=i: torch.matmul(x, fviews[i % nf].view(kdim, ncols), out=yt)) for i in range(max(nf, 16) if not cold else nf)]
                t_u = [_time_graph(fn_u) for _ in range(REPEATS)]
                t_p = [_time_graph(fn_p) for _ in range(3)]
                t_t = _time_graph(fn_t)
                u_med, spread = statistics.median(t_u), max(t_u) - min(t_u)
                p_med = statistics.median(t_p)
                plan = ops.cbpk_plan(m, kdim, ncols, bits, k, cus)
                common = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "bits": bits, "m": m, "state": state}
                recs = [dict(common, impl="packed", us=round(p_med * 1e6, 3), repeats_us=[round(t * 1e6, 3) for t in t_p], index_bytes=pbytes,
                             index_tb_s=round(pbytes / p_med / 1e12, 4), rotation_span_mib=round(np_ * pbytes / 2 ** 20, 1),
                             vs_uint8=round(u_med / p_med, 3), vs_torch=round(t_t / p_med, 3),
                             target="met" if p_med <= u_med + spread else "missed",
                             plan={f: plan[f] for f in ("path", "vb", "mt", "cols", "splits", "col_tiles", "row_tiles")}),
                        dict(common, impl="uint8", library=base_name, us=round(u_med * 1e6, 3), repeats_us=[round(t * 1e6, 3) for t in t_u],
                             spread_us=round(spread * 1e6, 3), index_bytes=n, index_tb_s=round(n / u_med / 1e12, 4),
                             rotation_span_mib=round(nu * n / 2 ** 20, 1)),
                        dict(common, impl="torch_fp32", us=round(t_t * 1e6, 3), index_bytes=4 * n, index_tb_s=round(4 * n / t_t / 1e12, 4),
                             rotation_span_mib=round(nf * 4 * n / 2 ** 20, 1))]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--baseline-lib", default=None, help="a libnnc_hip.so built from the commit before the packed form: the uint8 yardstick")
    ap.add_argument("--quick", action="store_true", help="4096 x 4096 and 768 x 2304 at m = 1, 16, 256 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    with torch.no_grad():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                run(f, a.baseline_lib, a.quick)
        else:
            run(None, a.baseline_lib, a.quick)


if __name__ == "__main__":
    main()
