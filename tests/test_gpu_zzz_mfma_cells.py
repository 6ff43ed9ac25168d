"""Every MFMA tile instantiation of the fifteen half-precision codebook units (five forward, five dx and five dc kernels; m > 16), run
through the raw C ABI on the case lists of tests/helpers/mfma_cells_ref.py (run with -m gpu).  These are the
kernels every compressed layer runs at batch sizes above 16.  The file sorts behind every other GPU file, so no earlier id moves.

Per case, on exact data: y / dx / dc equal the float64 formula bit for bit as float32 (dc also as float64) and, where the call has a
half output, rounded once to the half type (the kernel's own half store where the call has one split, the reduce's where it has
more); a second call gives the same bits.  The output and a workspace of exactly the queried size are slices of sentinel-filled
buffers (test_gpu_zz_forward_stream_cells' ``_launch``): afterwards the frames are intact and no sentinel is left inside the output or
the float32 partials.  NaNs lie directly in front of and behind x, g and the bias, 0xFF bytes directly behind the labels, the packed
buffer and the bitmap-sparse buffer; the first case of every uint8 cell has a NaN centre 255 that no label uses.  Before anything
runs, each test checks the plans at the device's own CU count against the whole table of its unit, and the real device addresses of x
and g against the arm each case claims."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import test_gpu_zz_forward_stream_cells as zz  # noqa: E402
from tests.helpers import h16_ref  # noqa: E402
from tests.helpers import mfma_cells_ref as cells  # noqa: E402

TDT = zz.TDT
DT_CODE = zz.DT_CODE


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    return _native.load(), ops, ops.device_info()[1]


def _values(a, dtype, off=0):
    """``a`` on the device as ``dtype`` inside a 256-byte aligned buffer of NaNs: 8 of them (16 bytes of a half type, so the alignment
    the arms ask about stays) and ``off`` more in front, 64 behind"""
    a = np.array(a, dtype=np.float32)
    lo = 8 + off
    buf = torch.full((lo + a.size + 64,), float("nan"), dtype=TDT[dtype], device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[lo: lo + a.size] = torch.from_numpy(a.ravel()).cuda().to(TDT[dtype])
    return buf[lo: lo + a.size]


_INDEX = {}


def _index_form(ops, case, d):
    """The case's indices on the device, made once and shared by the element types: the labels, the packed bytes, or the bitmap-sparse
    buffer with its nnz (and the skipped symbols of a grouped one); 0xFF bytes directly behind each"""
    key = (cells.unit_of(case), case["id"])
    if key in _INDEX:
        return _INDEX[key]
    form, kdim, ncols, k = case["form"], case["kdim"], case["ncols"], case["k"]
    if "packed" in d:
        out = zz._bytes(d["packed"])
    elif form in ("byte", "gbyte"):
        out = zz._labels(d["labels"], case["arg"] or 1, 0)
    elif form == "sparse":
        lab = zz._labels(d["labels"], case["arg"], 0)
        codes = ops.pack_sparse_codes(lab if case["arg"] == 1 else lab.view(torch.int16), kdim, ncols, k, zero_symbol=cells.SPARSE_Z)
        assert codes.zero_symbol == cells.SPARSE_Z and codes.nnz == int((d["labels"] != cells.SPARSE_Z).sum()) > 0
        out = (zz._bytes(codes.buf.cpu().numpy()), codes.nnz, None)
    else:
        zs = torch.from_numpy(np.array(d["zs"])).cuda()
        codes = ops.pack_grouped_sparse_codes(zz._labels(d["labels"], 1, 0), kdim, ncols, k, case["group_rows"], zero_symbols=zs)
        assert codes.nnz == int((d["labels"] != d["zs"][np.arange(kdim) // case["group_rows"]][:, None]).sum()) > 0
        out = (zz._bytes(codes.buf.cpu().numpy()), codes.nnz, zs)
    _INDEX[key] = out
    return out


class Unit:
    """The raw entry point of one case for one element type over the case's device buffers: ``run(half_or_f64)`` -> the output's bits"""

    def __init__(self, env, case, dtype):
        L, ops, cus = env
        self.case, self.dtype = case, dtype
        self.d = d = cells.data(case)
        form, way, a, m, kdim, ncols, k = case["form"], case["direction"], case["arg"], case["m"], case["kdim"], case["ncols"], case["k"]
        self.x, self.g = _values(d["x"], dtype, case["xoff"]), _values(d["g"], dtype, case["goff"])
        self.bias = None if d["bias"] is None else _values(d["bias"], "f32")
        cen = np.asarray(d["centers"], dtype=np.float32)
        self.centers = torch.from_numpy(np.array(cen)).cuda()
        self.first = torch.from_numpy(np.array(cen[0] if cen.ndim == 2 else cen)).cuda()
        self.index = _index_form(ops, case, d)
        x, g, c, c0 = self.x.data_ptr(), self.g.data_ptr(), self.centers.data_ptr(), self.first.data_ptr()
        self.arm = cells.arm_of(way, x, g, kdim, ncols)
        b = None if self.bias is None else self.bias.data_ptr()
        dt, st, gr = DT_CODE[dtype], torch.cuda.current_stream().cuda_stream, case.get("group_rows")
        relu = int(case["relu"])
        if form in ("byte", "gbyte"):
            ix = (self.index.data_ptr(),) + ((a,) if form == "byte" else ())
            tail = (ncols,)
        elif form in ("packed", "gpacked"):
            ix, tail = (self.index.data_ptr(), self.index.numel(), a), (ncols,)
        else:
            buf, nnz, zs = self.index
            ix = (buf.data_ptr(), buf.numel()) + ((a,) if form == "sparse" else ())
            tail = (ncols, cells.SPARSE_Z if form == "sparse" else zs.data_ptr(), nnz)
        grp = (gr,) if gr else ()
        name = {"byte": "cbmm", "sparse": "cbsp", "packed": "cbpk", "gbyte": "cbmm_grouped", "gpacked": "cbpk_grouped", "gsparse": "cbsp_grouped"}[form]
        self.one_group = None
        if way == "fwd":
            fn = getattr(L, f"nnc_{name}" + ("" if form in ("gbyte", "gpacked") else "_h16"))
            self.call = lambda out, code, ws, n: fn(x, dt, m, kdim, *ix, *tail, c, k, *grp, b, relu, out, code, ws, n, st)
            if form == "gpacked":
                self.one_group = lambda out, code, ws, n: L.nnc_cbpk_h16(x, dt, m, kdim, *ix, *tail, c0, k, b, relu, out, code, ws, n, st)
            self.units, self.want = m * ncols, "y"
        elif way == "dx":
            fn = getattr(L, f"nnc_{name}_dx_h16")
            self.call = lambda out, code, ws, n: fn(g, dt, m, kdim, *ix, *tail, c, k, *grp, out, code, ws, n, st)
            self.units, self.want = m * kdim, "dx"
        else:
            fn = getattr(L, f"nnc_{name}_dc_h16")
            self.call = lambda out, f64, ws, n: fn(x, g, dt, m, kdim, *ix, *tail, k, *grp, out, f64, ws, n, st)
            self.units, self.want = d["dc"].size, "dc"
        self.plan, self.ws_bytes = cells.plan(case, dtype, cus)
        self.splits, _ = cells.check_plan(case, self.plan, cus)
        if self.one_group:
            p1, ws1 = cells.plan(case, dtype, cus, one_group=True)
            assert cells.check_plan(case, p1, cus, one_group=True)[0] == self.splits and ws1 == self.ws_bytes
        assert self.plan["workspace"] <= self.ws_bytes
        self.ws_words = self.splits * self.units if self.splits > 1 and way != "dc" else 0      # the float32 partials, at the start of the workspace

    def run(self, wide, one_group=False):
        """``wide``: forward / dx: the output as the half type; dc: as float64"""
        call = self.one_group if one_group else self.call
        if self.case["direction"] == "dc":
            return zz._launch(lambda out, ws, n: call(out, int(wide), ws, n), self.units, torch.int64 if wide else torch.int32, self.ws_bytes, 0, "dc")
        code = DT_CODE[self.dtype] if wide else 0
        return zz._launch(lambda out, ws, n: call(out, code, ws, n), self.units, torch.int16 if wide else torch.int32, self.ws_bytes, self.ws_words,
                          self.want)


def _check(u):
    dtype, way = u.dtype, u.case["direction"]
    if way == "dc":
        for f64 in (1, 0):
            dc = u.run(f64)
            got = dc.view(torch.float64 if f64 else torch.float32).cpu().numpy().reshape(u.d["dc"].shape)
            assert np.array_equal(got, u.d["dc"] if f64 else u.d["dc"].astype(np.float32)), f"dc (f64 {f64})"
            assert torch.equal(dc, u.run(f64)), "dc: a second call gives other bits"
        return
    for one_group in (False, True) if u.one_group else (False,):
        want = u.d["y1" if one_group else u.want]
        tag = ("one group: " if one_group else "") + u.want
        out = u.run(False, one_group)
        assert zz._same_bits(out, want, torch.float32), tag
        assert torch.equal(out, u.run(False, one_group)), tag + ": a second call gives other bits"
        want_h = h16_ref.round_to(want, dtype)
        assert not (want_h == torch.tensor([zz.SENT16], dtype=torch.int16).view(TDT[dtype]).float().item()).any()   # no result is the sentinel
        half = u.run(True, one_group)
        assert zz._same_bits(half, want_h, TDT[dtype]), "half " + tag
        assert torch.equal(half, u.run(True, one_group)), "half " + tag + ": a second call gives other bits"


GROUPS = [(form, group, dtype) for form, group in (("byte", "fwd"), ("sparse", "fwd"), ("gbyte", "fwd"), ("gpacked", "fwd"), ("gsparse", "fwd"),
                                                    ("byte", "bwd"), ("sparse", "bwd"), ("packed", "bwd"), ("gbyte", "bwd"), ("gpacked", "bwd"))
          for dtype in cells.DTYPES]


@pytest.mark.parametrize("form,group,dtype", GROUPS, ids=[f"{f}-{g}-{d}" for f, g, d in GROUPS])
def test_every_mfma_cell_of_the_unit(env, form, group, dtype):
    """One test per (unit, direction group, element type): first the plans of all the cases at the device's own CU count (each on the
    MFMA path with the tiles, splits and groups it claims) and the arm the real addresses of x and g select (the cells hit are the
    whole table, each in both modes), then every case runs; the ids of all the cases that fail are reported together, each with the
    first line of what it failed on."""
    failed, n = [], 0
    for way in ("fwd",) if group == "fwd" else ("dx", "dc"):
        units = [Unit(env, case, dtype) for case in cells.CASES[(form, way)]]
        for u in units:
            assert u.arm == u.case["arm"], (u.case["id"], u.x.data_ptr() % 16, u.g.data_ptr() % 16)
        assert {(dtype, u.case["arg"], u.arm, "split" if u.splits > 1 else "direct") for u in units} == {c for c in cells.CELLS[(form, way)] if c[0] == dtype}
        for u in units:
            n += 1
            try:
                _check(u)
            except AssertionError as e:
                failed.append(f"{u.case['id']}-{dtype}: {(str(e).splitlines() or [''])[0][:80]}")
    print(f"{form} {group} {dtype}: {n} cases, {len(failed)} failed")
    assert not failed, f"{len(failed)} of {n} cases failed:\n" + "\n".join(failed)
