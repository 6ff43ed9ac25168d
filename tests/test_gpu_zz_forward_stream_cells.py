"""Every stream instantiation of the forward codebook units (byte and bitmap-sparse form in bf16 / fp16, grouped byte form, packed
form, grouped packed form with nnc_cbpk_h16 as its one-group call) and of the half packed backward units, grouped and not, run through the raw C ABI on the
case lists of tests/helpers/forward_stream_cells_ref.py (run with -m gpu).  These are the kernels every
compressed layer runs at batch sizes up to 16.  The file sorts behind every other GPU file, so no earlier id moves.

Per case, on exact data: y equals the float64 formula bit for bit as float32 and, from a half unit, also rounded once to the half
type (the kernel's own half store where the call has one split, k_cbmm_reduce's where it has more); a second call gives the same
bits.  y and the workspace are slices of larger buffers filled with a sentinel no result can equal (a NaN payload; 0x7BCD units for a
half y; 0xA5 bytes for the workspace, which is exactly the queried size): after the call the frame is intact and no element inside
is still the sentinel.  NaNs lie directly behind x and the bias and 0xFF bytes directly behind the labels or the packed buffer, so a
value read past an end that reaches a result shows.  Results are compared element by element as section 29 compares them: every
value equal, a NaN equal to nothing.  The backward cases check dx and dc as section 29 does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import forward_stream_cells_ref as cells  # noqa: E402
from tests.helpers import h16_ref  # noqa: E402

SENT16 = 0x7BCD
SENT32 = 0x7FA5A5A5                 # a float32 NaN
SENT64 = 0x7FF8A5A5A5A5A5A5         # a float64 NaN
WS_BYTE, WS_PAD = 0xA5, 256
WS_WORD = -1515870811               # four 0xA5 bytes as an int32: -2.9e-16 as a float32, no multiple of 1/4
PAD = 64                            # frame units on each side of y, dx and dc
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DT_CODE = {"f32": 0, "bf16": 1, "fp16": 2}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    return _native.load(), ops, ops.device_info()[1]


def _values(a, dtype):
    """``a`` on the device as ``dtype``, directly in front of 64 NaNs"""
    a = np.array(a, dtype=np.float32)
    buf = torch.full((a.size + 64,), float("nan"), dtype=TDT[dtype], device="cuda")
    buf[: a.size] = torch.from_numpy(a.ravel()).cuda().to(TDT[dtype])
    return buf[: a.size]


def _bytes(host, spare=64, off=0):
    """uint8 ``host`` on the device, ``off`` bytes into a 256-byte aligned buffer of 0xFF bytes with ``spare`` of them behind it"""
    buf = torch.full((off + host.size + spare,), 255, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[off: off + host.size] = torch.from_numpy(np.array(host, dtype=np.uint8).ravel()).cuda()
    return buf[off: off + host.size]


def _labels(lab, lb, off):
    """The indices as uint8 / uint16, ``off`` elements into their buffer, 16 bytes of 0xFF behind them"""
    host = lab.astype(np.uint8) if lb == 1 else np.ascontiguousarray(lab.astype(np.uint16)).view(np.uint8)
    return _bytes(host, 16, off * lb)


_INDEX = {}


def _index_form(ops, case, d):
    """The case's indices on the device, made once and shared by the element types (and by the cases of one wide packed shape): the
    labels, the bitmap-sparse buffer with its nnz, or the packed bytes."""
    key = (case["form"], case["id"]) if "packed" not in d else ("packed", d["packed"].ctypes.data)
    if key not in _INDEX:
        if "packed" in d:
            _INDEX[key] = _bytes(d["packed"])
        elif case["form"] == "sparse":
            lab = _labels(d["labels"], case["lb"], 0)
            lab = lab if case["lb"] == 1 else lab.view(torch.int16)
            codes = ops.pack_sparse_codes(lab, case["kdim"], case["ncols"], case["k"], zero_symbol=case["z"])
            assert codes.zero_symbol == case["z"] and codes.nnz == int((d["labels"] != case["z"]).sum()) > 0
            _INDEX[key] = (_bytes(codes.buf.cpu().numpy()), codes.nnz)
        else:
            t = _labels(d["labels"], case["lb"], case["off"])
            assert (t.data_ptr() % case["vb"] == 0 and (case["ncols"] * case["lb"]) % case["vb"] == 0) == bool(case["aligned"])
            _INDEX[key] = t
    return _INDEX[key]


def _framed(units, tdtype, sent):
    buf = torch.full((units + 2 * PAD,), sent, dtype=tdtype, device="cuda")
    return buf, buf[PAD: PAD + units]


def _launch(call, units, kind, ws_bytes, ws_words, what):
    """One raw call into a framed output of ``units`` elements (kind: torch.int16 / int32 / int64 with its sentinel) and a framed
    workspace of exactly ``ws_bytes``; the frames intact, nothing inside the output or the first ``ws_words`` float32 words of the
    workspace left as the sentinel (one host read for all of it); -> the bits inside the output."""
    from neural_network_compression_amd import _native as nat

    sent = {torch.int16: SENT16, torch.int32: SENT32, torch.int64: SENT64}[kind]
    obuf, out = _framed(units, kind, sent)
    wbuf = torch.full((ws_bytes + 2 * WS_PAD,), WS_BYTE, dtype=torch.uint8, device="cuda")
    assert wbuf.data_ptr() % 256 == 0 and ws_bytes % 4 == 0
    nat.check(call(out.data_ptr(), wbuf.data_ptr() + WS_PAD, ws_bytes))
    inside = wbuf[WS_PAD: WS_PAD + 4 * ws_words].view(torch.int32)
    flags = torch.stack([(obuf[:PAD] == sent).all() & (obuf[PAD + units:] == sent).all(),
                         (wbuf[:WS_PAD] == WS_BYTE).all() & (wbuf[WS_PAD + ws_bytes:] == WS_BYTE).all(),
                         ~(out == sent).any(), ~(inside == WS_WORD).any()]).tolist()
    assert flags[0], f"a store outside {what}"
    assert flags[1], f"a store outside the {what} workspace"
    assert flags[2], f"a {what} element left unwritten"
    assert flags[3], f"a word of the {what} partials left unwritten"
    return out


def _same_bits(got, want_f32, tdtype):
    """the output, read as ``tdtype``, against float32 values that ``tdtype`` holds exactly: every value equal (a NaN equals nothing)"""
    want = torch.from_numpy(np.ascontiguousarray(want_f32, dtype=np.float32).ravel()).cuda().to(tdtype)
    return torch.equal(got.view(tdtype), want)


class Forward:
    """The raw forward entry point of one case for one element type over the case's device buffers."""

    def __init__(self, env, case, dtype):
        L, ops, cus = env
        self.case, self.dtype = case, dtype
        self.d = d = cells.data(case, dtype)
        form, m, kdim, ncols, k = case["form"], case["m"], case["kdim"], case["ncols"], case["k"]
        self.x = _values(d["x"], dtype)
        self.bias = None if d["bias"] is None else _values(d["bias"], "f32")
        cen = np.asarray(d["centers"], dtype=np.float32)
        self.centers = torch.from_numpy(np.array(cen)).cuda()
        self.first = torch.from_numpy(np.array(cen[0] if cen.ndim == 2 else cen)).cuda()       # the first group's centres
        self.index = _index_form(ops, case, d)
        x, b, c, c0 = self.x.data_ptr(), None if self.bias is None else self.bias.data_ptr(), self.centers.data_ptr(), self.first.data_ptr()
        relu, dt, stream = int(case["relu"]), DT_CODE[dtype], torch.cuda.current_stream().cuda_stream
        self.one_group = None
        if form == "byte":
            lab, lb = self.index.data_ptr(), case["lb"]
            self.addr = lab
            self.call = lambda y, code, ws, n: L.nnc_cbmm_h16(x, dt, m, kdim, lab, lb, ncols, c, k, b, relu, y, code, ws, n, stream)
        elif form == "sparse":
            (buf, nnz), lb, z = self.index, case["lb"], case["z"]
            pk, pkn = buf.data_ptr(), buf.numel()
            self.addr = None
            self.call = lambda y, code, ws, n: L.nnc_cbsp_h16(x, dt, m, kdim, pk, pkn, lb, ncols, z, nnz, c, k, b, relu, y, code, ws, n, stream)
        elif form == "grouped":
            lab, gr = self.index.data_ptr(), case["group_rows"]
            self.addr = lab
            self.call = lambda y, code, ws, n: L.nnc_cbmm_grouped(x, dt, m, kdim, lab, ncols, c, k, gr, b, relu, y, code, ws, n, stream)
        else:
            pk, pkn, bits = self.index.data_ptr(), self.index.numel(), case["bits"]
            self.addr = None
            if form == "packed":
                self.call = lambda y, code, ws, n: L.nnc_cbpk_f32(x, m, kdim, pk, pkn, bits, ncols, c0, k, b, relu, y, ws, n, stream)
            else:
                gr = case["group_rows"]
                self.call = lambda y, code, ws, n: L.nnc_cbpk_grouped(x, dt, m, kdim, pk, pkn, bits, ncols, c, k, gr, b, relu, y, code, ws, n, stream)
                if dtype != "f32":
                    self.one_group = lambda y, code, ws, n: L.nnc_cbpk_h16(x, dt, m, kdim, pk, pkn, bits, ncols, c0, k, b, relu, y, code, ws, n, stream)
        self.plan, self.ws_bytes = cells.plan(case, dtype, cus, self.addr)
        self.cell = cells.check_plan(case, self.plan, cus)
        if self.one_group:
            p1, ws1 = cells.plan(case, dtype, cus, one_group=True)
            assert cells.check_plan(case, p1, cus, one_group=True) == self.cell and ws1 == self.ws_bytes
        assert self.plan["workspace"] <= self.ws_bytes
        self.ws_words = self.plan["splits"] * m * ncols if self.plan["splits"] > 1 else 0     # the float32 partials, at the start of the workspace

    def run(self, half_out, one_group=False):
        call = self.one_group if one_group else self.call
        code = DT_CODE[self.dtype] if half_out else 0
        return _launch(lambda y, ws, n: call(y, code, ws, n), self.case["m"] * self.case["ncols"], torch.int16 if half_out else torch.int32,
                       self.ws_bytes, self.ws_words, "y")


def _check_forward(u):
    dtype = u.dtype
    for one_group in (False, True) if u.one_group else (False,):
        want = u.d["y1" if one_group else "y"]
        tag = "one group: " if one_group else ""
        y = u.run(False, one_group)
        assert _same_bits(y, want, torch.float32), tag + "y"
        assert torch.equal(y, u.run(False, one_group)), tag + "y: a second call gives other bits"
        if dtype != "f32":
            want_h = h16_ref.round_to(want, dtype)
            assert not (want_h == torch.tensor([SENT16], dtype=torch.int16).view(TDT[dtype]).float().item()).any()   # no result is the sentinel
            yh = u.run(True, one_group)
            assert _same_bits(yh, want_h, TDT[dtype]), tag + "half y"
            assert torch.equal(yh, u.run(True, one_group)), tag + "half y: a second call gives other bits"


class Backward:
    """nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16 of one packed backward case, or nnc_cbpk_grouped_dx_h16 / nnc_cbpk_grouped_dc_h16 of a grouped one"""

    def __init__(self, env, case, dtype):
        L, ops, cus = env
        self.case, self.dtype = case, dtype
        self.d = d = cells.bwd_data(case["form"], case["id"])
        m, kdim, ncols, k, bits = case["m"], case["kdim"], case["ncols"], case["k"], case["bits"]
        self.x, self.g = _values(d["x"], dtype), _values(d["g"], dtype)
        self.centers = torch.from_numpy(np.array(d["centers"])).cuda()
        self.index = _index_form(ops, case, d)
        x, g, c, pk, pkn = self.x.data_ptr(), self.g.data_ptr(), self.centers.data_ptr(), self.index.data_ptr(), self.index.numel()
        dt, stream = DT_CODE[dtype], torch.cuda.current_stream().cuda_stream
        self.dxp, self.dcp, self.dx_ws, self.dc_ws = cells.bwd_plans(case, dtype, cus)
        for p in (self.dxp, self.dcp):
            assert p["path"] == cells.PATH_STREAM and cells.cell_of_plan(case, p) == case["cell"], (case["id"], p)
        assert self.dxp["splits"] == self.dxp["col_tiles"] == case["expect"]["splits"] and self.dcp["row_tiles"] >= 3
        self.cell = case["cell"]
        if case["form"] == "gpacked_bwd":
            gr = case["group_rows"]
            for p in (self.dxp, self.dcp):
                assert (p["group_rows"], p["groups"]) == (gr, case["expect"]["groups"]), (case["id"], p)
            self.dx = lambda out, code, ws, n: L.nnc_cbpk_grouped_dx_h16(g, dt, m, kdim, pk, pkn, bits, ncols, c, k, gr, out, code, ws, n, stream)
            self.dc = lambda out, f64, ws, n: L.nnc_cbpk_grouped_dc_h16(x, g, dt, m, kdim, pk, pkn, bits, ncols, k, gr, out, f64, ws, n, stream)
        else:
            self.dx = lambda out, code, ws, n: L.nnc_cbpk_dx_h16(g, dt, m, kdim, pk, pkn, bits, ncols, c, k, out, code, ws, n, stream)
            self.dc = lambda out, f64, ws, n: L.nnc_cbpk_dc_h16(x, g, dt, m, kdim, pk, pkn, bits, ncols, k, out, f64, ws, n, stream)

    def run_dx(self, half_out):
        n = self.case["m"] * self.case["kdim"]
        code = DT_CODE[self.dtype] if half_out else 0
        words = self.dxp["splits"] * n if self.dxp["splits"] > 1 else 0
        return _launch(lambda out, ws, nb: self.dx(out, code, ws, nb), n, torch.int16 if half_out else torch.int32, self.dx_ws, words, "dx")

    def run_dc(self, f64):
        return _launch(lambda out, ws, nb: self.dc(out, f64, ws, nb), self.d["dc"].size, torch.int64 if f64 else torch.int32, self.dc_ws, 0, "dc")


def _check_backward(u):
    d, dtype = u.d, u.dtype
    assert np.array_equal(d["dx"].astype(np.float32).astype(np.float64), d["dx"])                    # the formula's value is a float32
    dx = u.run_dx(False)
    assert _same_bits(dx, d["dx"], torch.float32), "dx"
    assert torch.equal(dx, u.run_dx(False)), "dx: a second call gives other bits"
    want_h = h16_ref.round_to(d["dx"], dtype)
    assert not (want_h == torch.tensor([SENT16], dtype=torch.int16).view(TDT[dtype]).float().item()).any()
    dxh = u.run_dx(True)
    assert _same_bits(dxh, want_h, TDT[dtype]), "half dx"
    assert torch.equal(dxh, u.run_dx(True)), "half dx: a second call gives other bits"
    for f64 in (1, 0):
        dc = u.run_dc(f64)
        got = dc.view(torch.float64 if f64 else torch.float32).cpu().numpy().reshape(d["dc"].shape)
        assert np.array_equal(got, d["dc"] if f64 else d["dc"].astype(np.float32)), ("dc", f64)
        assert torch.equal(dc, u.run_dc(f64)), "dc: a second call gives other bits"


UNIT_DTYPES = [(unit, dtype) for unit in sorted(cells.UNITS) for dtype in cells.UNITS[unit][1]]


@pytest.mark.parametrize("unit,dtype", UNIT_DTYPES, ids=[f"{u}-{d}" for u, d in UNIT_DTYPES])
def test_every_cell_of_the_unit(env, unit, dtype):
    """One test per unit and element type, not one per case: first the plans of all the cases at the device's own CU count and the
    labels' real addresses (each in its cell on the stream path, with the column blocks, splits and groups it claims; the cells hit
    are the whole table, each in both modes), then every case runs; the ids of all the cases that fail are reported together, each
    with the first line of what it failed on."""
    form = cells.UNITS[unit][0]
    make, check = (Backward, _check_backward) if form.endswith("_bwd") else (Forward, _check_forward)
    units = [make(env, case, dtype) for case in cells.CASES[form]]
    hit = {(u.cell, u.case["mode"]) for u in units}
    assert {cell for cell, _ in hit} == cells.CELLS[form]
    assert form.endswith("_bwd") or hit == {(cell, mode) for cell in cells.CELLS[form] for mode in ("direct", "split")}
    failed = []
    for u in units:
        try:
            check(u)
        except AssertionError as e:
            failed.append(f"{u.case['id']}-{dtype}: {(str(e).splitlines() or [''])[0][:80]}")
    print(f"{unit} {dtype}: {len(units)} cases, {len(failed)} failed")
    assert not failed, f"{len(failed)} of {len(units)} cases failed:\n" + "\n".join(failed)
