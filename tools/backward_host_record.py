"""The host behaviour of the five codebook backward units, recorded without a GPU.

    python tools/backward_host_record.py --lib PATH/libnnc_hip.so --out tests/golden/backward_host_record.json

sweep(lib) calls every plan entry point and every *_workspace_bytes query of the byte, group-wise, bitmap-sparse, packed and
group-wise packed forms over a grid of shapes, and every plan, workspace and *_f32 entry point with invalid arguments (which fail
before any HIP call).  The plan records are kept as one sha256 per (entry point, m) with the number of calls behind it, the
invalid calls as (return code, nnc_last_error() text).  The committed record was made from a library built at the commit BEFORE
the host glue of these units was written once (nnc_cbgrad.hpp: cbg_run_dx, cbg_run_dc, cbg_stream_case, cbg_plan_out):
tests/test_backward_host_record.py holds the library under test to it, so the record is never made from the code it checks.

    python tools/backward_host_record.py --half --lib PATH/libnnc_hip.so --out tests/golden/backward_h16_host_record.json

The same for the *_h16 twins of these entry points, the backward passes on bf16 / fp16 activations: the
sweep takes both dtypes, the invalid calls are made on a stream shape (m = 1) and an MFMA shape (m = 64) and add what only the
half entry points check (x_dtype, dx_dtype, the alignment of g, x and dx, 2-byte labels on an odd address).  That record was made
from a library built at the commit before the MFMA plan, the dx loop and the half glue were written once;
tests/test_backward_h16_host_record.py holds the library under test to it.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import itertools
import json
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_network_compression_amd import _native as nat  # noqa: E402

M = (0, 1, 2, 3, 8, 16, 17, 128, 256, 4096)
KDIM = (0, 1, 31, 32, 64, 100, 784, 4096)
NCOLS = (0, 1, 15, 16, 100, 256, 257, 1025, 4096)
BYTE_LK = ((1, 255), (1, 256), (2, 256), (2, 257))      # (label_bytes, K): both widths, a K on each side of 256
GROUPED_K = (255, 256)
PACKED_BK = ((2, 1), (2, 4), (2, 16), (4, 1), (4, 4), (4, 16))   # (bits, K); (2, 16) is refused, and recorded as such
GROUP_ROWS = (32, 64, 96, 128, 160)
CUS = (1, 64, 256, 304)
ADDR = (0, 1, 4, 16)
P = 0x1000          # a fake, never dereferenced, 256-byte aligned address
PLAN_LEN = 32       # more than any plan record
DTYPES = (nat.DT_BF16, nat.DT_F16)
HALF_M_INVALID = (1, 64)   # the invalid half calls: a stream shape and an MFMA shape, each with a workspace in both directions


def bind(path):
    L = ctypes.CDLL(path)
    for name, (res, args) in list(nat.SIGNATURES.items()) + list(nat.GROUPED_GRAD_SIGNATURES.items()) + list(nat.GROUPED_PACKED_GRAD_SIGNATURES.items()) + \
            list(nat.H16_GRAD_SIGNATURES.items()) + list(nat.SPARSE_H16_GRAD_SIGNATURES.items()) + list(nat.PACKED_H16_SIGNATURES.items()) + \
            list(nat.GROUPED_H16_GRAD_SIGNATURES.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    L.nnc_last_error.restype = ctypes.c_char_p
    return L


def _err(lib):
    return lib.nnc_last_error().decode("utf-8", "replace")


class _Hashes:
    def __init__(self):
        self.h, self.n = {}, {}

    def add(self, name, m, blob):
        key = f"{name}|m={m}"
        self.h.setdefault(key, hashlib.sha256()).update(blob)
        self.n[key] = self.n.get(key, 0) + 1

    def result(self):
        return {k: [self.n[k], self.h[k].hexdigest()] for k in sorted(self.h)}


def _plan(lib, H, name, m, args):
    out = (ctypes.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    rc = getattr(lib, name)(*args, out)
    blob = struct.pack(f"<i{PLAN_LEN}q", rc, *out)
    if rc != 0:
        blob += _err(lib).encode()
    H.add(name, m, blob)


def _ws(lib, H, name, m, args):
    H.add(name, m, struct.pack("<q", getattr(lib, name)(*args)))


def sweep_plans(lib, half=False):
    """{"<entry point>|m=<m>": [calls, sha256 of their records]}; half: the *_h16 entry points, every plan at both dtypes"""
    H = _Hashes()
    h = "_h16" if half else ""
    dts = [(dt,) for dt in DTYPES] if half else [()]
    for m, kdim, ncols in itertools.product(M, KDIM, NCOLS):
        s = (m, kdim, ncols)
        for lb, k in BYTE_LK:
            _ws(lib, H, f"nnc_cbmm_dx{h}_workspace_bytes", m, (*s, lb))
            _ws(lib, H, f"nnc_cbmm_dc{h}_workspace_bytes", m, (*s, lb, k))
            _ws(lib, H, f"nnc_cbsp_dx{h}_workspace_bytes", m, (*s, lb))
            _ws(lib, H, f"nnc_cbsp_dc{h}_workspace_bytes", m, (*s, lb, k))
            for dt, cus in itertools.product(dts, CUS):
                _plan(lib, H, f"nnc_cbsp_dx{h}_plan", m, (*dt, *s, lb, k, cus))
                _plan(lib, H, f"nnc_cbsp_dc{h}_plan", m, (*dt, *s, lb, k, cus))
                for addr in ADDR:
                    _plan(lib, H, f"nnc_cbmm_dx{h}_plan", m, (*dt, *s, lb, k, cus, addr))
                    _plan(lib, H, f"nnc_cbmm_dc{h}_plan", m, (*dt, *s, lb, k, cus, addr))
        _ws(lib, H, f"nnc_cbmm_grouped_dx{h}_workspace_bytes", m, s)
        for k, gr in itertools.product(GROUPED_K, GROUP_ROWS):
            _ws(lib, H, f"nnc_cbmm_grouped_dc{h}_workspace_bytes", m, (*s, k, gr))
            for dt, cus, addr in itertools.product(dts, CUS, ADDR):
                _plan(lib, H, f"nnc_cbmm_grouped_dx{h}_plan", m, (*dt, *s, k, gr, cus, addr))
                _plan(lib, H, f"nnc_cbmm_grouped_dc{h}_plan", m, (*dt, *s, k, gr, cus, addr))
        for bits, k in PACKED_BK:
            _ws(lib, H, f"nnc_cbpk_dx{h}_workspace_bytes", m, (*s, bits))
            _ws(lib, H, f"nnc_cbpk_dc{h}_workspace_bytes", m, (*s, bits, k))
            _ws(lib, H, f"nnc_cbpk_grouped_dx{h}_workspace_bytes", m, (*s, bits))
            for dt, cus in itertools.product(dts, CUS):
                _plan(lib, H, f"nnc_cbpk_dx{h}_plan", m, (*dt, *s, bits, k, cus))
                _plan(lib, H, f"nnc_cbpk_dc{h}_plan", m, (*dt, *s, bits, k, cus))
            for gr in GROUP_ROWS:
                _ws(lib, H, f"nnc_cbpk_grouped_dc{h}_workspace_bytes", m, (*s, bits, k, gr))
                for dt, cus in itertools.product(dts, CUS):
                    _plan(lib, H, f"nnc_cbpk_grouped_dx{h}_plan", m, (*dt, *s, bits, k, gr, cus))
                    _plan(lib, H, f"nnc_cbpk_grouped_dc{h}_plan", m, (*dt, *s, bits, k, gr, cus))
    return H.result()


# ------------------------------------------------------------------ invalid calls
# every entry point: its parameters in order, on top of BASE (a valid call of a shape that needs both workspaces)
BASE = dict(x=P, g=P, m=1, kdim=5000, ncols=5000, labels=P, packed=P, centers=P, dx=P, dc=P, f64=1, stream=None, cus=256, addr=0, out="out",
            lb=1, bits=4, k=16, gr=32, z=0, nnz=0, dt=nat.DT_BF16, dxdt=nat.DT_BF16)
FORMS = {
    "nnc_cbmm": dict(width="lb", grouped=False,
                     dx_ws="m kdim ncols lb", dc_ws="m kdim ncols lb k", plan="m kdim ncols lb k cus addr out",
                     dx="g m kdim labels lb ncols centers k dx ws ws_bytes stream", dc="x g m kdim labels lb ncols k dc f64 ws ws_bytes stream"),
    "nnc_cbmm_grouped": dict(width=None, grouped=True,
                             dx_ws="m kdim ncols", dc_ws="m kdim ncols k gr", plan="m kdim ncols k gr cus addr out",
                             dx="g m kdim labels ncols centers k gr dx ws ws_bytes stream", dc="x g m kdim labels ncols k gr dc f64 ws ws_bytes stream"),
    "nnc_cbsp": dict(width="lb", grouped=False,
                     dx_ws="m kdim ncols lb", dc_ws="m kdim ncols lb k", plan="m kdim ncols lb k cus out",
                     dx="g m kdim packed packed_bytes lb ncols z nnz centers k dx ws ws_bytes stream",
                     dc="x g m kdim packed packed_bytes lb ncols z nnz k dc f64 ws ws_bytes stream"),
    "nnc_cbpk": dict(width="bits", grouped=False,
                     dx_ws="m kdim ncols bits", dc_ws="m kdim ncols bits k", plan="m kdim ncols bits k cus out",
                     dx="g m kdim packed packed_bytes bits ncols centers k dx ws ws_bytes stream",
                     dc="x g m kdim packed packed_bytes bits ncols k dc f64 ws ws_bytes stream"),
    "nnc_cbpk_grouped": dict(width="bits", grouped=True,
                             dx_ws="m kdim ncols bits", dc_ws="m kdim ncols bits k gr", plan="m kdim ncols bits k gr cus out",
                             dx="g m kdim packed packed_bytes bits ncols centers k gr dx ws ws_bytes stream",
                             dc="x g m kdim packed packed_bytes bits ncols k gr dc f64 ws ws_bytes stream"),
}
BAD_SIZES = [dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(m=1 << 41), dict(kdim=1 << 41), dict(ncols=1 << 41)]
BAD_WIDTH = {"lb": [dict(lb=0), dict(lb=3), dict(lb=1, k=257)], "bits": [dict(bits=3), dict(bits=8), dict(bits=2, k=5)], None: [dict(k=257)]}
BAD_K = [dict(k=0), dict(k=-3), dict(k=1 << 20)]
BAD_GROUP_ROWS = [dict(gr=0), dict(gr=-32), dict(gr=16), dict(gr=48), dict(gr=1 << 41), dict(kdim=1 << 40, ncols=4, gr=32)]
# misaligned: the entry points that ask for an alignment (the byte form's dx takes any)
# what only the half entry points check: the dtypes, the alignment of g, x and dx, 2-byte labels on an odd address
BAD_DTYPE = [dict(dt=nat.DT_F32), dict(dt=7)]
HALF_OPERANDS = {"dx": [dict(dxdt=7), dict(dxdt=nat.DT_F16), dict(g=P + 1), dict(dx=P + 1), dict(dxdt=nat.DT_F32, dx=P + 2)], "dc": [dict(x=P + 1), dict(g=P + 1)]}
WS_ALIGNED = {"nnc_cbmm": ("dc",), "nnc_cbmm_grouped": ("dc",), "nnc_cbsp": ("dx", "dc"), "nnc_cbpk": ("dx", "dc"), "nnc_cbpk_grouped": ("dx", "dc")}


def _packed_bytes(lib, form, a):
    if min(a["kdim"], a["ncols"]) < 0:
        return 0
    if form == "nnc_cbsp":
        return lib.nnc_cbsp_pack_bytes(a["kdim"], a["ncols"], a["lb"], a["nnz"]) if a["lb"] in (1, 2) else 0
    return lib.nnc_cbpk_pack_bytes(a["kdim"], a["ncols"], a["bits"]) if a["bits"] in (2, 4) else 0


def _call(lib, name, params, a):
    lib.nnc_cbmm_dx_plan(-1, 0, 0, 1, 1, 1, 0, None)      # a fixed text in nnc_last_error(): what a call that sets none leaves behind
    out = (ctypes.c_int64 * PLAN_LEN)()
    rc = getattr(lib, name)(*[out if (p == "out" and a[p] == "out") else a[p] for p in params.split()])
    return [int(rc), _err(lib)]


def _half(params):
    """the parameters of the *_h16 twin of an entry point: x_dtype first in a plan, behind g in a call, dx_dtype behind dx"""
    t = params.split()
    if "g" not in t:
        return " ".join(["dt"] + t)
    t.insert(t.index("g") + 1, "dt")
    if "dx" in t:
        t.insert(t.index("dx") + 1, "dxdt")
    return " ".join(t)


def sweep_invalid(lib, half=False):
    """[[entry point, the arguments changed from BASE, return code, nnc_last_error()], ...]; half: the *_h16 entry points"""
    rows = []
    h = "_h16" if half else ""
    for form, F in FORMS.items():
        plan, call = (_half(F["plan"]), {d: _half(F[d]) for d in ("dx", "dc")}) if half else (F["plan"], F)
        shape_bad = BAD_SIZES + BAD_WIDTH[F["width"]] + BAD_K + (BAD_GROUP_ROWS if F["grouped"] else []) + (BAD_DTYPE if half else [])
        for d in ("dx", "dc"):
            for kw in shape_bad:
                if not set(kw) <= set(F[f"{d}_ws"].split()):      # (the query does not take what this case changes)
                    continue
                a = {**BASE, **kw}
                rows.append([f"{form}_{d}{h}_workspace_bytes", kw, *_call(lib, f"{form}_{d}{h}_workspace_bytes", F[f"{d}_ws"], a)])
            for kw in shape_bad + [dict(cus=0), dict(cus=-1), dict(out=None), dict(cus=0, out=None)]:
                a = {**BASE, **kw}
                rows.append([f"{form}_{d}{h}_plan", kw, *_call(lib, f"{form}_{d}{h}_plan", plan, a)])
            operands = ([dict(g=None), dict(centers=None), dict(dx=None)] if d == "dx" else [dict(x=None), dict(g=None), dict(dc=None)])
            operands += [dict(labels=None)] if "labels" in F[d] else [dict(packed=None), dict(packed=P + 8), dict(packed_bytes=7)]
            if form == "nnc_cbsp":
                operands += [dict(z=-2), dict(z=1 << 20), dict(nnz=-1)]
            if half:
                operands += HALF_OPERANDS[d] + ([dict(lb=2, labels=P + 1)] if form == "nnc_cbmm" else [])
            space = [dict(ws_bytes=-1), dict(ws_delta=-1), dict(ws=None)] + ([dict(ws=P + 2)] if half or d in WS_ALIGNED[form] else [])
            for kw, m in itertools.product(shape_bad + operands + space, HALF_M_INVALID if half else (BASE["m"],)):
                a = {**BASE, "m": m, **{k: v for k, v in kw.items() if k != "ws_delta"}}
                a.setdefault("packed_bytes", _packed_bytes(lib, form, a))
                a.setdefault("ws", P)
                if "ws_bytes" not in a:
                    lib.nnc_cbmm_dx_plan(-1, 0, 0, 1, 1, 1, 0, None)
                    a["ws_bytes"] = max(0, getattr(lib, f"{form}_{d}{h}_workspace_bytes")(*[a[p] for p in F[f"{d}_ws"].split()])) + kw.get("ws_delta", 0)
                name = f"{form}_{d}_h16" if half else f"{form}_{d}_f32"
                rc, msg = _call(lib, name, call[d], a)
                assert rc != 0, (name, kw, m, "an invalid call must fail before any HIP call")
                rows.append([name, {"m": m, **kw} if half else kw, rc, msg])
    return rows


def sweep(lib, half=False):
    return {"plans": sweep_plans(lib, half), "invalid": sweep_invalid(lib, half)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the libnnc_hip.so to record (built from the commit before the one under test)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--half", action="store_true", help="record the *_h16 entry points (the bf16 / fp16 backward passes)")
    a = ap.parse_args()
    rec = sweep(bind(a.lib), a.half)
    with open(a.out, "w") as f:
        plans = ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(rec["plans"].items()))      # one entry per line
        invalid = ",\n".join(json.dumps(r, sort_keys=True) for r in rec["invalid"])
        f.write('{"invalid": [\n' + invalid + '\n],\n"plans": {\n' + plans + "\n}}\n")
    print(f"{a.out}: {len(rec['plans'])} hashes over {sum(n for n, _ in rec['plans'].values())} calls, {len(rec['invalid'])} invalid calls")


if __name__ == "__main__":
    main()
