"""Times the bitmap-sparse group-wise codebook matmul on bf16 / fp16 activations (ops.grouped_sparse_codebook_matmul with
half_inputs=True: k_cbspg_rowterm, k_cbspg_stream and k_cbspg_combine for m <= 16, k_cbspg_mfma and k_cbmm_reduce above) against, in
the same run, the float32 product of the same form (ops.grouped_sparse_codebook_matmul), the ungrouped sparse product on half x
with one codebook (ops.sparse_codebook_matmul) and the byte form of the grouped layer on half x (ops.grouped_codebook_matmul), one
JSON line per (dtype, group_rows, m, cache state, implementation).

    python tools/time_grouped_sparse_codebook_matmul_h16.py [--out FILE] [--quick]

The method of tools/time_codebook_matmul.py, as tools/time_grouped_sparse_codebook_matmul.py applies it: a
sequence of calls captured in a HIP graph and replayed between HIP events for at least 0.2 s.  warm: the same weights every call;
cold: a rotation over distinct matrices spanning >= 1 GiB in each form (the span is reported).  The layer is 4096 x 4096, uint8
indices, K = 16, density 10 %, group_rows 128 and 32, m = 1, 16, 256 and 4096.  The skipped symbol is 0 in every group and its centre
is not 0, so the stream path carries its rank-1 term.

The two targets of DESIGN.md section 30 are written into the grouped_sparse_h16 rows at m = 4096: ``target_a`` (bf16 only): faster than
the float32 grouped sparse product of the same (group_rows, state); ``target_b``: at most 1.10 x the ungrouped half sparse product of
the same (dtype, state).  Each is "met" or "missed".  Every other row is reported, not required.  ``weight_bytes`` is the resident
form a call streams.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neural_network_compression_amd import ops  # noqa: E402
from time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views  # noqa: E402

KDIM = NCOLS = 4096
K = 16
DENSITY = 0.10
GROUP_ROWS = [128, 32]
MS = [1, 16, 256, 4096]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = KDIM * NCOLS
    rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
    lbuf, lviews = _views(n, rot, torch.uint8, n, dev)
    for v in lviews:
        v.random_(1, K)
        v.masked_fill_(torch.rand(n, device=dev) >= DENSITY, 0)
    centers = torch.randn(K, device=dev) * 0.05 + 0.02           # c_z = centers[0] != 0
    sp0 = ops.pack_sparse_codes(lviews[0], KDIM, NCOLS, K, zero_symbol=0)
    rot_s = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / sp0.nbytes())))
    scodes = [sp0] + [ops.pack_sparse_codes(lviews[i % rot], KDIM, NCOLS, K, zero_symbol=0) for i in range(1, rot_s)]
    for group_rows in GROUP_ROWS:
        groups = KDIM // group_rows
        centers_g = (centers[None, :] + torch.randn(groups, K, device=dev) * 0.01).contiguous()
        zs = torch.zeros(groups, dtype=torch.uint8, device=dev)
        gcodes = [ops.pack_grouped_sparse_codes(lviews[i % rot], KDIM, NCOLS, K, group_rows, zero_symbols=zs) for i in range(rot_s)]
        resident = {"grouped_sparse": gcodes[0].nbytes() + 4 * groups * K, "grouped_byte": n + 4 * groups * K, "sparse": sp0.nbytes() + 4 * K}
        for m in MS:
            if quick and m in (16, 256):
                continue
            x32 = torch.rand(m, KDIM, device=dev)
            for state in (("warm",) if quick else ("warm", "cold")):
                ns = 1 if state == "warm" else rot_s
                nl = 1 if state == "warm" else rot
                calls = lambda count: max(count, 16) if state == "warm" else count   # noqa: E731
                t_f32 = _time_graph([(lambda i=i: ops.grouped_sparse_codebook_matmul(x32, gcodes[i % ns], centers_g)) for i in range(calls(ns))])
                for name, dt in DTYPES.items():
                    if quick and name == "fp16":
                        continue
                    x = x32.to(dt)
                    t_new = _time_graph([(lambda i=i: ops.grouped_sparse_codebook_matmul(x, gcodes[i % ns], centers_g, half_inputs=True))
                                         for i in range(calls(ns))])
                    t_sp = _time_graph([(lambda i=i: ops.sparse_codebook_matmul(x, scodes[i % ns], centers)) for i in range(calls(ns))])
                    t_gb = _time_graph([(lambda i=i: ops.grouped_codebook_matmul(x, lviews[i % nl], centers_g, KDIM, NCOLS, group_rows))
                                        for i in range(calls(nl))])
                    rows = [("grouped_sparse_h16", name, t_new, "grouped_sparse", ns * gcodes[0].nbytes()), ("sparse_h16", name, t_sp, "sparse", ns * sp0.nbytes()),
                            ("grouped_byte_h16", name, t_gb, "grouped_byte", nl * float(n))]
                    if name == "bf16" or quick:
                        rows.append(("grouped_sparse_f32", "f32", t_f32, "grouped_sparse", ns * gcodes[0].nbytes()))
                    for impl, xdt, t, key, span in rows:
                        rec = {"case": f"{KDIM}x{NCOLS}", "kdim": KDIM, "ncols": NCOLS, "k": K, "density": DENSITY, "nnz": sp0.nnz, "group_rows": group_rows,
                               "groups": groups, "m": m, "state": state, "impl": impl, "x_dtype": xdt, "us": round(t * 1e6, 3),
                               "weight_bytes": resident[key], "rotation_span_mib": round(span / 2 ** 20, 1)}
                        if impl == "grouped_sparse_h16":
                            rec.update(vs_f32=round(t_new / t_f32, 3), vs_sparse_h16=round(t_new / t_sp, 3), vs_grouped_byte_h16=round(t_new / t_gb, 3))
                            if m == 4096:
                                if name == "bf16":
                                    rec.update(target_a="met" if t_new < t_f32 else "missed", bound_a_us=round(t_f32 * 1e6, 3))
                                rec.update(target_b="met" if t_new <= 1.10 * t_sp else "missed", bound_b_us=round(1.10 * t_sp * 1e6, 3))
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()
        del gcodes
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="warm only, bf16 only, m = 1 and 4096")
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
