"""Every stream instantiation of the backward units of the byte, bitmap-sparse and grouped index forms, float32 and bf16 / fp16, run
through the raw C ABI on the case list of tests/helpers/stream_cells_ref.py (run with -m gpu).  These are the
kernels every step of fine-tuning a compressed network runs at small batch sizes.

Per case, on exact data: dx equals the float64 formula bit for bit as float32 and, from a half unit, also rounded once to the half
type (the direct half store on the one-block width, k_cbgrad_reduce's on the two-block width); dc equals it as float64 and rounded
once as float32; a second call gives the same bits.  dx, dc and the workspace are slices of larger buffers filled with a sentinel no
result can equal (a NaN payload; 0x7BCD units for a half dx; 0xA5 bytes for the workspace, which is exactly the queried size): after
the call the frame is intact and no element inside is still the sentinel.  NaNs lie directly behind x and g and 0xFF bytes directly
behind the labels, so a value read past a row's end that reaches a result shows."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import h16_ref  # noqa: E402
from tests.helpers import stream_cells_ref as cells  # noqa: E402

SENT16 = 0x7BCD
SENT32 = 0x7FA5A5A5                 # a float32 NaN
SENT64 = 0x7FF8A5A5A5A5A5A5         # a float64 NaN
WS_BYTE, WS_PAD = 0xA5, 256
PAD = 64                            # frame units on each side of dx and dc
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DT_CODE = dict(h16_ref.DT_CODE, f32=0)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    return _native.load(), ops


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared arrays are read-only)


def _values(a, dtype):
    """``a`` on the device as ``dtype``, directly in front of 64 NaNs"""
    a = np.array(a, dtype=np.float32)
    buf = torch.full((a.size + 64,), float("nan"), dtype=TDT[dtype], device="cuda")
    buf[: a.size] = torch.from_numpy(a.ravel()).cuda().to(TDT[dtype])
    return buf[: a.size]


def _labels(lab, lb, off):
    """The indices as uint8 / int16, ``off`` elements into a 0xFF-filled buffer with 16 spare bytes behind them."""
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.full((off + host.size + 16 // lb,), 255 if lb == 1 else -1, dtype=torch.uint8 if lb == 1 else torch.int16, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host).ravel()).cuda()
    return buf[off: off + host.size]


@functools.lru_cache(maxsize=None)
def _index_form(form, case_id):
    """The case's indices on the device, made once and shared by the three dtypes: the labels, or for the sparse form the packed
    buffer (256-byte aligned, 0xFF bytes behind it) with its skipped symbol and nnz."""
    from neural_network_compression_amd import ops

    case = cells.BY_ID[form][case_id]
    lab = cells.data(case, "f32")["labels"]
    if form != "sparse":
        t = _labels(lab, case["lb"], case["off"])
        assert (t.data_ptr() % case["vb"] == 0 and (case["ncols"] * case["lb"]) % case["vb"] == 0) == bool(case["aligned"])
        return t
    codes = ops.pack_sparse_codes(_labels(lab, case["lb"], 0), case["kdim"], case["ncols"], case["k"], zero_symbol=case["z"])
    assert codes.zero_symbol == case["z"] and codes.nnz == int((lab != case["z"]).sum()) > 0
    buf = torch.full((codes.nbytes() + 64,), 255, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[: codes.nbytes()] = codes.buf
    return buf[: codes.nbytes()], codes.nnz


def _framed(units, tdtype, sent, pad=PAD):
    buf = torch.full((units + 2 * pad,), sent, dtype=tdtype, device="cuda")
    return buf, buf[pad: pad + units]


def _frame_intact(buf, units, sent, pad=PAD):
    return bool((buf[:pad] == sent).all()) and bool((buf[pad + units:] == sent).all())


def _workspace(nbytes):
    buf = torch.full((nbytes + 2 * WS_PAD,), WS_BYTE, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + WS_PAD


class Unit:
    """The raw entry points of one form for one dtype: dx(out_ptr, out_code, ws_ptr, ws_bytes) / dc(out_ptr, f64, ws_ptr, ws_bytes) and
    the two workspace sizes, over the case's device buffers."""

    def __init__(self, env, case, dtype):
        L, ops = env
        self.case, self.dtype = case, dtype
        d = cells.data(case, dtype)
        form, m, kdim, ncols, k = case["form"], case["m"], case["kdim"], case["ncols"], case["k"]
        h = dtype != "f32"
        dt = (DT_CODE[dtype],) if h else ()
        sfx = "_h16" if h else ""
        self.x, self.g, self.centers = _values(d["x"], dtype), _values(d["g"], dtype), _cuda(d["centers"])
        self.keep = _index_form(form, case["id"])
        x, g, c = self.x.data_ptr(), self.g.data_ptr(), self.centers.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        if form == "byte":
            lab, lb = self.keep.data_ptr(), case["lb"]
            fdx, fdc = getattr(L, "nnc_cbmm_dx" + ("_h16" if h else "_f32")), getattr(L, "nnc_cbmm_dc" + ("_h16" if h else "_f32"))
            self.dx_ws = int(getattr(L, f"nnc_cbmm_dx{sfx}_workspace_bytes")(m, kdim, ncols, lb))
            self.dc_ws = int(getattr(L, f"nnc_cbmm_dc{sfx}_workspace_bytes")(m, kdim, ncols, lb, k))
            self.dx = lambda out, code, ws, n: fdx(g, *dt, m, kdim, lab, lb, ncols, c, k, out, *((code,) if h else ()), ws, n, stream)
            self.dc = lambda out, f64, ws, n: fdc(x, g, *dt, m, kdim, lab, lb, ncols, k, out, f64, ws, n, stream)
        elif form == "sparse":
            (packed, nnz), lb, z = self.keep, case["lb"], case["z"]
            pk, pkn = packed.data_ptr(), packed.numel()
            fdx, fdc = getattr(L, "nnc_cbsp_dx" + ("_h16" if h else "_f32")), getattr(L, "nnc_cbsp_dc" + ("_h16" if h else "_f32"))
            self.dx_ws = int(getattr(L, f"nnc_cbsp_dx{sfx}_workspace_bytes")(m, kdim, ncols, lb))
            self.dc_ws = int(getattr(L, f"nnc_cbsp_dc{sfx}_workspace_bytes")(m, kdim, ncols, lb, k))
            self.dx = lambda out, code, ws, n: fdx(g, *dt, m, kdim, pk, pkn, lb, ncols, z, nnz, c, k, out, *((code,) if h else ()), ws, n, stream)
            self.dc = lambda out, f64, ws, n: fdc(x, g, *dt, m, kdim, pk, pkn, lb, ncols, z, nnz, k, out, f64, ws, n, stream)
        else:
            lab, gr = self.keep.data_ptr(), case["group_rows"]
            fdx = getattr(L, "nnc_cbmm_grouped_dx" + ("_h16" if h else "_f32"))
            fdc = getattr(L, "nnc_cbmm_grouped_dc" + ("_h16" if h else "_f32"))
            self.dx_ws = int(getattr(L, f"nnc_cbmm_grouped_dx{sfx}_workspace_bytes")(m, kdim, ncols))
            self.dc_ws = int(getattr(L, f"nnc_cbmm_grouped_dc{sfx}_workspace_bytes")(m, kdim, ncols, k, gr))
            self.dx = lambda out, code, ws, n: fdx(g, *dt, m, kdim, lab, ncols, c, k, gr, out, *((code,) if h else ()), ws, n, stream)
            self.dc = lambda out, f64, ws, n: fdc(x, g, *dt, m, kdim, lab, ncols, k, gr, out, f64, ws, n, stream)

    def run_dx(self, half_out):
        """dx into a framed buffer with a framed workspace; the frames checked; -> the bits inside (int32, or int16 for a half dx)"""
        from neural_network_compression_amd import _native as nat

        n = self.case["m"] * self.case["kdim"]
        obuf, out = _framed(n, torch.int16, SENT16) if half_out else _framed(n, torch.int32, SENT32)
        wbuf, ws = _workspace(self.dx_ws)
        nat.check(self.dx(out.data_ptr(), DT_CODE[self.dtype] if half_out else 0, ws, self.dx_ws))
        torch.cuda.synchronize()
        sent = SENT16 if half_out else SENT32
        assert _frame_intact(obuf, n, sent), "a store outside dx"
        assert _frame_intact(wbuf, self.dx_ws, WS_BYTE, WS_PAD), "a store outside the dx workspace"
        assert not bool((out == sent).any()), "a dx element left unwritten"
        return out.clone()

    def run_dc(self, f64):
        from neural_network_compression_amd import _native as nat

        n = cells.data(self.case, self.dtype)["dc"].size
        obuf, out = _framed(n, torch.int64, SENT64) if f64 else _framed(n, torch.int32, SENT32)
        wbuf, ws = _workspace(self.dc_ws)
        nat.check(self.dc(out.data_ptr(), 1 if f64 else 0, ws, self.dc_ws))
        torch.cuda.synchronize()
        sent = SENT64 if f64 else SENT32
        assert _frame_intact(obuf, n, sent), "a store outside dc"
        assert _frame_intact(wbuf, self.dc_ws, WS_BYTE, WS_PAD), "a store outside the dc workspace"
        assert not bool((out == sent).any()), "a dc element left unwritten"
        return out.clone()


def _check(env, case, dtype):
    d = cells.data(case, dtype)
    u = Unit(env, case, dtype)
    m, kdim = case["m"], case["kdim"]
    want = d["dx"].astype(np.float32)
    assert np.array_equal(want.astype(np.float64), d["dx"])                    # the formula's value is a float32
    dx = u.run_dx(False)
    assert np.array_equal(dx.view(torch.float32).cpu().numpy().reshape(m, kdim), want), "dx"
    assert torch.equal(dx, u.run_dx(False)), "dx: a second call gives other bits"
    if dtype != "f32":
        want_h = h16_ref.round_to(d["dx"], dtype)
        assert not (want_h == torch.tensor([SENT16], dtype=torch.int16).view(TDT[dtype]).float().item()).any()   # no result is the sentinel
        dxh = u.run_dx(True)
        assert np.array_equal(dxh.view(TDT[dtype]).float().cpu().numpy().reshape(m, kdim), want_h), "half dx"
        assert torch.equal(dxh, u.run_dx(True)), "half dx: a second call gives other bits"
    for f64 in (1, 0):
        dc = u.run_dc(f64)
        got = dc.view(torch.float64 if f64 else torch.float32).cpu().numpy().reshape(d["dc"].shape)
        assert np.array_equal(got, d["dc"] if f64 else d["dc"].astype(np.float32)), ("dc", f64)
        assert torch.equal(dc, u.run_dc(f64)), "dc: a second call gives other bits"


UNIT_DTYPES = [(unit, dtype) for unit in sorted(cells.UNITS) for dtype in cells.UNITS[unit][1]]


@pytest.mark.parametrize("unit,dtype", UNIT_DTYPES, ids=[f"{u}-{d}" for u, d in UNIT_DTYPES])
def test_every_cell_of_the_unit(env, unit, dtype):
    """One test per unit and element type, so that the suite grows by nine ids and not by one per case: first the plans at the device's
    own CU count and the labels' real addresses (every table entry, with the claimed blocks and splits), then every case of the form;
    the ids of all the cases that fail are reported together, each with the first line of what it failed on."""
    _, ops = env
    _, cus = ops.device_info()
    form = cells.UNITS[unit][0]
    hit = set()
    for case in cells.CASES[form]:
        addr = _index_form(form, case["id"]).data_ptr() if form != "sparse" else 0     # the address the kernel is given
        dx, dc, _, _ = cells.plans(case, dtype, cus, addr)
        for which, p in (("dx", dx), ("dc", dc)):
            assert p["path"] == cells.PATH_STREAM and cells.cell_of_plan(case, p) == cells.cell_of(case), (case["id"], which, p)
            assert (p["col_tiles"], p["splits"]) == (case["expect"][which]["col_tiles"], case["expect"][which]["splits"])
            assert p["row_tiles"] >= 3
            hit.add(cells.cell_of_plan(case, p))
    assert hit == cells.CELLS[form]
    failed = []
    for case in cells.CASES[form]:
        try:
            _check(env, case, dtype)
        except AssertionError as e:
            failed.append(f"{case['id']}-{dtype}: {(str(e).splitlines() or [''])[0][:80]}")
    print(f"{unit} {dtype}: {len(cells.CASES[form])} cases, {len(failed)} failed")
    assert not failed, f"{len(failed)} of {len(cells.CASES[form])} cases failed:\n" + "\n".join(failed)
