"""Host time of one eager call of every codebook backward entry point: the time the host takes to enqueue
nnc_*_dx_f32 / nnc_*_dc_f32 of the five forms at m = 1, 256 x 256, K = 16 (group_rows 32; packed at 4 bits; the sparse form empty),
without waiting for the stream.  Two builds of the library are loaded in one process and alternate, 7 rounds of 500 calls each:

    python tools/backward_host_time.py --parent-lib OTHER/libnnc_hip.so > FILE

One JSON line per entry point: every round of both builds and their medians.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--parent-lib", required=True, help="a libnnc_hip.so built from the commit to compare with")
A = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib.util
import torch
spec = importlib.util.spec_from_file_location("rec", os.path.join(ROOT, "tools", "backward_host_record.py"))
rec = importlib.util.module_from_spec(spec); spec.loader.exec_module(rec)
libs = {"parent": rec.bind(A.parent_lib),
        "head": rec.bind(os.path.join(ROOT, "neural_network_compression_amd", "csrc", "libnnc_hip.so"))}
dev = torch.device("cuda", 0)
m, kdim, ncols, k, gr = 1, 256, 256, 16, 32
G = kdim // gr
g = torch.randn(m, ncols, device=dev); x = torch.randn(m, kdim, device=dev)
cen = torch.randn(G * k, device=dev)
lab = torch.zeros(kdim * ncols + 64, dtype=torch.uint8, device=dev)
dx = torch.zeros(m, kdim, device=dev); dc = torch.zeros(G * k, dtype=torch.float64, device=dev)
ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
L0 = libs["head"]
PKB = L0.nnc_cbpk_pack_bytes(kdim, ncols, 4)
SPB = L0.nnc_cbsp_pack_bytes(kdim, ncols, 1, 0)
pk = torch.zeros(PKB + 256, dtype=torch.uint8, device=dev)
sp = torch.zeros(SPB + 256, dtype=torch.uint8, device=dev)
P = lambda t: t.data_ptr()
WS = 1 << 20
def calls(L):
    return {
        "nnc_cbmm_dx_f32": lambda: L.nnc_cbmm_dx_f32(P(g), m, kdim, P(lab), 1, ncols, P(cen), k, P(dx), P(ws), WS, None),
        "nnc_cbmm_dc_f32": lambda: L.nnc_cbmm_dc_f32(P(x), P(g), m, kdim, P(lab), 1, ncols, k, P(dc), 1, P(ws), WS, None),
        "nnc_cbmm_grouped_dx_f32": lambda: L.nnc_cbmm_grouped_dx_f32(P(g), m, kdim, P(lab), ncols, P(cen), k, gr, P(dx), P(ws), WS, None),
        "nnc_cbmm_grouped_dc_f32": lambda: L.nnc_cbmm_grouped_dc_f32(P(x), P(g), m, kdim, P(lab), ncols, k, gr, P(dc), 1, P(ws), WS, None),
        "nnc_cbpk_dx_f32": lambda: L.nnc_cbpk_dx_f32(P(g), m, kdim, P(pk), PKB, 4, ncols, P(cen), k, P(dx), P(ws), WS, None),
        "nnc_cbpk_dc_f32": lambda: L.nnc_cbpk_dc_f32(P(x), P(g), m, kdim, P(pk), PKB, 4, ncols, k, P(dc), 1, P(ws), WS, None),
        "nnc_cbpk_grouped_dx_f32": lambda: L.nnc_cbpk_grouped_dx_f32(P(g), m, kdim, P(pk), PKB, 4, ncols, P(cen), k, gr, P(dx), P(ws), WS, None),
        "nnc_cbpk_grouped_dc_f32": lambda: L.nnc_cbpk_grouped_dc_f32(P(x), P(g), m, kdim, P(pk), PKB, 4, ncols, k, gr, P(dc), 1, P(ws), WS, None),
        "nnc_cbsp_dx_f32": lambda: L.nnc_cbsp_dx_f32(P(g), m, kdim, P(sp), SPB, 1, ncols, 0, 0, P(cen), k, P(dx), P(ws), WS, None),
        "nnc_cbsp_dc_f32": lambda: L.nnc_cbsp_dc_f32(P(x), P(g), m, kdim, P(sp), SPB, 1, ncols, 0, 0, k, P(dc), 1, P(ws), WS, None),
    }
C = {n: calls(L) for n, L in libs.items()}
N, ROUNDS = 500, 7
for name in C["head"]:
    for n in libs:
        rc = C[n][name]()
        assert rc == 0, (name, n, rc, libs[n].nnc_last_error())
    torch.cuda.synchronize()
    t = {"parent": [], "head": []}
    for r in range(ROUNDS):
        for n in ("parent", "head"):
            f = C[n][name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(N):
                f()
            t1 = time.perf_counter()       # the host's time to enqueue N calls (the stream is not waited for)
            torch.cuda.synchronize()
            t[n].append((t1 - t0) / N * 1e6)
    print(json.dumps({"entry": name, "m": m, "kdim": kdim, "ncols": ncols, "calls": N,
                      "parent_us": [round(v, 3) for v in t["parent"]], "head_us": [round(v, 3) for v in t["head"]],
                      "parent_median": round(statistics.median(t["parent"]), 3), "head_median": round(statistics.median(t["head"]), 3)}), flush=True)
