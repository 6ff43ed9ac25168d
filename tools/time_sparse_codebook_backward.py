"""Times the bitmap-sparse codebook backward pass (ops.sparse_codebook_matmul_dx: k_cbsp_rowsum, k_cbspdx_stream / k_cbspdx_tiled,
k_cbgrad_reduce, k_cbspdx_rank1; ops.sparse_codebook_centroid_grad: k_cbgrad_absmax, k_cbspdc_stream / k_cbspdc_tiled,
k_cbdc_finish) against the dense codebook backward on the same labels (ops.codebook_matmul_dx / codebook_centroid_grad) and
torch's dense backward on the decoded float32 W (g @ W.T, x.T @ g, then ops.centroid_gradient of that dW), one JSON line per
(shape, density, m, implementation).

    python tools/time_sparse_codebook_backward.py [--out FILE] [--quick]

The method of tools/time_codebook_backward.py: each sequence of calls is captured in a HIP graph and replayed between HIP events
for at least 0.2 s, cold (a rotation over distinct copies of the packed form / the index matrix / the float32 W spanning >= 1 GiB,
four times the Infinity Cache).  ops.centroid_gradient reads max |dW| back to the host, so the torch baseline's centroid sum is
timed uncaptured in a loop and added ("torch_dense" = the sum of the parts).  bytes: the packed form (or the indices) plus x, g and
dx; the bound is the larger of FLOPs / 157.3 TF and bytes / 8 TB/s, FLOPs counted for the stored weights only.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neural_network_compression_amd import ops  # noqa: E402
from tools.time_codebook_backward import _time_loop  # noqa: E402
from tools.time_codebook_matmul import COLD_SPAN, MAX_ROT, PEAK_TBS, PEAK_TF, _time_graph, _views  # noqa: E402

SHAPES = [("5000x5000", 5000, 5000, 256, 0.1), ("5000x5000", 5000, 5000, 256, 0.01), ("5000x5000", 5000, 5000, 257, 0.1),
          ("lenet300.dense1", 784, 300, 16, 0.1)]
MS = [1, 16, 256, 4096]


def _labels(kdim, ncols, k, density, lb, dev):
    keep = torch.rand(kdim * ncols, device=dev) < density
    lab = torch.where(keep, torch.randint(1, k, (kdim * ncols,), device=dev), torch.zeros((), dtype=torch.int64, device=dev))
    return lab.to(torch.uint8) if lb == 1 else lab.to(torch.int16)


def _rotation(codes, rot):
    """``rot`` distinct 256-byte aligned copies of the packed form."""
    out = []
    for _ in range(rot):
        buf = ops._aligned_bytes(codes.nbytes(), codes.device)
        buf.copy_(codes.buf)
        out.append(ops.SparseCodes(buf, codes.kdim, codes.ncols, codes.k, codes.zero_symbol, codes.label_bytes, codes.nnz))
    return out


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = SHAPES[:1] if quick else SHAPES
    for name, kdim, ncols, k, density in shapes:
        lb = 1 if k <= 256 else 2
        n = kdim * ncols
        labels = _labels(kdim, ncols, k, density, lb, dev)
        codes = ops.pack_sparse_codes(labels, kdim, ncols, k, zero_symbol=0)
        centers = torch.randn(k, device=dev) * 0.05
        rot_s = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / codes.nbytes())))
        rot_l = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * lb))))
        rot_f = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * 4))))
        srot = _rotation(codes, rot_s)
        lbuf, lviews = _views(n * lb, rot_l, labels.dtype, n, dev)
        for v in lviews:
            v.copy_(labels)
        fbuf, fviews = _views(n * 4, rot_f, torch.float32, n, dev)
        w = ops.gather(centers, labels)
        for v in fviews:
            v.copy_(w)
        del w
        for m in MS:
            if quick and m not in (1, 16):
                continue
            x = torch.rand(m, kdim, device=dev)
            g = torch.randn(m, ncols, device=dev) * 1e-2
            t_sdx = _time_graph([(lambda i=i: ops.sparse_codebook_matmul_dx(g, srot[i], centers)) for i in range(rot_s)])
            t_sdc = _time_graph([(lambda i=i: ops.sparse_codebook_centroid_grad(x, g, srot[i])) for i in range(rot_s)])
            t_ddx = _time_graph([(lambda i=i: ops.codebook_matmul_dx(g, lviews[i], centers, kdim, ncols)) for i in range(rot_l)])
            t_ddc = _time_graph([(lambda i=i: ops.codebook_centroid_grad(x, g, lviews[i], k, kdim, ncols)) for i in range(rot_l)])
            dxo = torch.empty(m, kdim, device=dev)
            dwo = torch.empty(kdim, ncols, device=dev)
            t_tdx = _time_graph([(lambda i=i: torch.matmul(g, fviews[i].view(kdim, ncols).t(), out=dxo)) for i in range(rot_f)])
            t_tdw = _time_graph([(lambda i=i: torch.matmul(x.t(), g, out=dwo)) for i in range(rot_f)])
            t_tcg = _time_loop(lambda i: ops.centroid_gradient(dwo, lviews[i % rot_l], k), rot_l)
            io = 4.0 * m * (2 * kdim + ncols)
            fl_s = 2.0 * m * codes.nnz + 2.0 * m * kdim
            fl_d = 2.0 * m * n
            sb = float(codes.nbytes())
            recs = [("sparse_dx", t_sdx, sb + io, fl_s), ("sparse_dc", t_sdc, sb + io, fl_d), ("sparse_dx+dc", t_sdx + t_sdc, 2 * sb + 2 * io, fl_s + fl_d),
                    ("codebook_dx", t_ddx, n * lb + io, fl_d), ("codebook_dc", t_ddc, n * lb + io, fl_d),
                    ("codebook_dx+dc", t_ddx + t_ddc, 2.0 * n * lb + 2 * io, 2 * fl_d),
                    ("torch_dx", t_tdx, n * 4.0 + io, fl_d), ("torch_dw", t_tdw, n * 4.0 + io, fl_d),
                    ("torch_centroid_gradient", t_tcg, n * (8.0 + lb), 0.0),
                    ("torch_dense", t_tdx + t_tdw + t_tcg, n * (16.0 + lb) + 2 * io, 2 * fl_d)]
            for impl, t, byts, fl in recs:
                t_min = max(fl / PEAK_TF, byts / PEAK_TBS)
                rec = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "label_bytes": lb, "density": round(codes.density(), 4), "m": m,
                       "state": "cold", "impl": impl, "us": round(t * 1e6, 3), "flops": fl, "bytes": byts, "tb_s": round(byts / t / 1e12, 3),
                       "tflops": round(fl / t / 1e12, 3), "bound": "compute" if fl / PEAK_TF >= byts / PEAK_TBS else "hbm",
                       "share": round(t_min / t, 4), "packed_bytes": codes.nbytes()}
                if impl == "sparse_dx+dc":
                    rec["speedup_vs_codebook"] = round((t_ddx + t_ddc) / (t_sdx + t_sdc), 3)
                    rec["speedup_vs_torch_dense"] = round((t_tdx + t_tdw + t_tcg) / (t_sdx + t_sdc), 3)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            del dwo, dxo
        del srot, lbuf, lviews, fbuf, fviews, labels, codes
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="the 5000 x 5000 uint8 10 %% case at m = 1, 16 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    with torch.no_grad():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                run(f, a.quick)
        else:
            run(None, a.quick)


if __name__ == "__main__":
    main()
