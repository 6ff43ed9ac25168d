"""Times the bitmap-sparse group-wise codebook matmul (ops.grouped_sparse_codebook_matmul: k_cbspg_rowterm, k_cbspg_stream /
k_cbspg_tiled, k_cbspg_combine) against the ungrouped sparse product on the same indices with one codebook
(ops.sparse_codebook_matmul) and against the byte form of the grouped layer (ops.grouped_codebook_matmul), one JSON line per
(group_rows, m, cache state, implementation), all in the same run.

    python tools/time_grouped_sparse_codebook_matmul.py [--out FILE] [--quick]

The method of tools/time_codebook_matmul.py: a sequence of calls captured in a HIP graph and replayed between
HIP events for at least 0.2 s.  warm: the same weights every call; cold: a rotation over distinct matrices spanning >= 1 GiB in each
form (the span is reported).  The layer is 4096 x 4096, uint8 indices, K = 16, density 10 %, group_rows 128 and 32, m = 1, 16 and
4096.  The skipped symbol is 0 in every group and its centre is not 0, so both sparse products carry their rank-1 term.

The targets of DESIGN.md section 28 are written into every grouped sparse row: ``bound_us`` = 1.10 x the ungrouped sparse time of
the same (m, state), plus, for m <= 16, ``rowterm_us``, the time of k_cbspg_rowterm alone, which is the one launch the ungrouped
stream kernel fuses.  ``rowterm_us`` is measured in the same run by difference: a layer of the same kdim and groups with one
output column and no stored symbol leaves the main kernels next to nothing to do, and there the grouped call is the ungrouped call
(c_z = 0: no row sums) plus k_cbspg_rowterm.  ``target`` is "met" or "missed".  ``weight_bytes`` is the resident form a call streams.
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
MS = [1, 16, 4096]


def _rowterm_alone(x, groups, group_rows, centers_g, dev):
    """Seconds of k_cbspg_rowterm for this x and these codebooks, by difference on a one-column layer with nothing stored."""
    kdim = x.shape[1]
    lab = torch.zeros(kdim, dtype=torch.uint8, device=dev)
    zs = torch.zeros(groups, dtype=torch.uint8, device=dev)
    gcodes = ops.pack_grouped_sparse_codes(lab, kdim, 1, K, group_rows, zero_symbols=zs)
    scodes = ops.pack_sparse_codes(lab, kdim, 1, K, zero_symbol=0)
    flat = centers_g[0].clone()
    flat[0] = 0.0                      # the ungrouped call forms no row sums: what is left is the main kernel and its combine
    t_g = _time_graph([(lambda: ops.grouped_sparse_codebook_matmul(x, gcodes, centers_g)) for _ in range(16)])
    t_s = _time_graph([(lambda: ops.sparse_codebook_matmul(x, scodes, flat)) for _ in range(16)])
    return max(t_g - t_s, 0.0), t_g, t_s


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
        packed_bytes = ops.packed_nbytes(KDIM, NCOLS, 4)
        resident = {"grouped_sparse": gcodes[0].nbytes() + 4 * groups * K, "grouped_byte": n + 4 * groups * K,
                    "grouped_packed": packed_bytes + 4 * groups * K, "sparse": sp0.nbytes() + 4 * K}
        for m in MS:
            if quick and m == 16:
                continue
            x = torch.rand(m, KDIM, device=dev)
            rowterm, rt_g, rt_s = _rowterm_alone(x, groups, group_rows, centers_g, dev)
            for state in (("warm",) if quick else ("warm", "cold")):
                ns = 1 if state == "warm" else rot_s
                nl = 1 if state == "warm" else rot
                calls = lambda count: max(count, 16) if state == "warm" else count   # noqa: E731
                t_gs = _time_graph([(lambda i=i: ops.grouped_sparse_codebook_matmul(x, gcodes[i % ns], centers_g)) for i in range(calls(ns))])
                t_sp = _time_graph([(lambda i=i: ops.sparse_codebook_matmul(x, scodes[i % ns], centers)) for i in range(calls(ns))])
                t_gb = _time_graph([(lambda i=i: ops.grouped_codebook_matmul(x, lviews[i % nl], centers_g, KDIM, NCOLS, group_rows)) for i in range(calls(nl))])
                bound = 1.10 * t_sp + (rowterm if m <= 16 else 0.0)
                for impl, t, key, span in (("grouped_sparse", t_gs, "grouped_sparse", ns * gcodes[0].nbytes()), ("sparse", t_sp, "sparse", ns * sp0.nbytes()),
                                           ("grouped_byte", t_gb, "grouped_byte", nl * float(n))):
                    rec = {"case": f"{KDIM}x{NCOLS}", "kdim": KDIM, "ncols": NCOLS, "k": K, "density": DENSITY, "nnz": sp0.nnz, "group_rows": group_rows,
                           "groups": groups, "m": m, "state": state, "impl": impl, "us": round(t * 1e6, 3), "weight_bytes": resident[key],
                           "rotation_span_mib": round(span / 2 ** 20, 1)}
                    if impl == "grouped_sparse":
                        rec.update(vs_sparse=round(t_gs / t_sp, 3), vs_grouped_byte=round(t_gs / t_gb, 3), rowterm_us=round(rowterm * 1e6, 3),
                                   rowterm_from_us=[round(rt_g * 1e6, 3), round(rt_s * 1e6, 3)], bound_us=round(bound * 1e6, 3),
                                   target="met" if t_gs <= bound else "missed", resident_bytes=resident)
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
    ap.add_argument("--quick", action="store_true", help="warm only, m = 1 and 4096")
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
