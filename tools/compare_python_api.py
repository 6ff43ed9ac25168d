"""The Python wrappers of the codebook products (ops.py, compressed.py) of this tree against those of another checkout.

    python tools/compare_python_api.py OTHER_CHECKOUT [--out FILE] [--phase results|host-time|all] [--repeats N]

Both checkouts must hold a built csrc/libnnc_hip.so (the same one: copy it, then both packages load the same kernels and
what is compared is the Python in front of them).  This launcher never initialises the GPU: it starts one fresh child per
checkout and phase (subprocess, each under its own ``timeout -k 10``), every child imports its own checkout's package and
writes its records to a file; the launcher compares the two files, prints one JSON line per case (``--out`` keeps them) and
exits with 1 on any difference.  A child that ends with 124, 134, 137, 139 or a negative status ends the run at once (exit
status 2, as for a child that fails otherwise: no GPU, a package from elsewhere, a device fault in one of its calls, which
the child re-raises so that it ends with a non-zero status and nothing more is started on the card).  A product for which no
shape with splits > 1 is found counts as a difference.

Phase "results": seeded inputs at the smallest shapes where the wrappers can differ -- 96 x 40 (ncols no multiple of 64, three
groups of 32 rows), x of shape (kdim,), (5, kdim), (2, 3, kdim), (0, kdim), K = 4 / 16 / 200 / 300, bias and ReLU on and off,
half x for the byte and the grouped form, one shape per product whose ``*_plan`` reports splits > 1 (found by calling the plan)
-- compared as raw bytes: every forward, dx, dc, the three gradients of each ``*_linear``, the layers' forward, state and
bytes, the plan dicts; and about twenty invalid calls per form, compared by (type, message).  No invalid call reaches a kernel.

Phase "host-time": each form's forward at m = 1 on a 256 x 256 matrix with K = 16, called eagerly 2000 times between two
synchronises after a warm-up, by the host clock, in microseconds per call.  At this size the call is bounded by the Python in
front of the launch, not by the kernel: that is the quantity a change of the wrappers can worsen, so the toy size is
deliberate and says nothing about kernel time.  The two checkouts alternate, ``--repeats`` (at least five) times each; this
tree passes if its median is within the other's median plus the range of the other's repeats.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = (124, 134, 137, 139)
NOTE = ("m = 1, 256 x 256, K = 16: bounded by the Python in front of the launch, not by the kernel (the toy size is deliberate); "
        "2000 eager calls between two synchronises, host clock")
KDIM, NCOLS, GROUP_ROWS = 96, 40, 32


# ------------------------------------------------------------------ the children
def _device_fault(e: Exception) -> bool:
    return any(w in str(e) for w in ("HIP error", "hipError", "illegal memory access"))


class _Recorder:
    def __init__(self, torch):
        self.torch, self.records = torch, {}

    def put(self, case, value):
        assert case not in self.records, case
        self.records[case] = value

    def tensor(self, case, t):
        raw = t.detach().contiguous().cpu().reshape(-1).view(self.torch.uint8).numpy().tobytes()
        self.put(case, {"dtype": str(t.dtype), "shape": list(t.shape), "nbytes": len(raw), "sha256": hashlib.sha256(raw).hexdigest(),
                        "head": raw[:32].hex()})

    def call(self, case, fn):
        """A valid call: its tensor result (or tuple of them) as raw bytes.  An exception is a record too, and a difference."""
        try:
            out = fn()
        except Exception as e:   # noqa: BLE001 - the record is the point
            if _device_fault(e):
                raise
            self.put(case, {"error": [type(e).__name__, str(e)]})
            return
        for i, t in enumerate(out if isinstance(out, tuple) else (out,)):
            if t is None:
                self.put(f"{case}[{i}]", None)
            else:
                self.tensor(f"{case}[{i}]" if isinstance(out, tuple) else case, t)

    def value(self, case, fn):
        """A host result that JSON holds as it is (a plan dict, a shape)."""
        try:
            self.put(case, fn())
        except Exception as e:   # noqa: BLE001
            self.put(case, {"error": [type(e).__name__, str(e)]})

    def invalid(self, case, fn):
        try:
            fn()
        except Exception as e:   # noqa: BLE001
            if _device_fault(e):
                raise
            self.put("invalid " + case, {"error": [type(e).__name__, str(e)]})
        else:
            self.put("invalid " + case, {"error": None})


def _child_results(torch, np, ops, C, rec):
    from neural_network_compression_amd import _native as nat
    from neural_network_compression_amd.neural_networks import layers

    dev = "cuda"
    rng = np.random.RandomState(20261018)
    _, cus = ops.device_info()

    def f32(*shape):
        return torch.from_numpy(np.asarray(rng.standard_normal(shape), dtype=np.float32)).to(dev)

    def labels_of(n, k, wide=False):
        lab = rng.randint(0, k, size=n)
        lab[rng.rand(n) < 0.5] = 0   # a most frequent symbol for the sparse form to skip
        host = lab.astype(np.uint16).view(np.int16) if wide else lab.astype(np.uint8)
        return torch.from_numpy(host).to(dev)

    leads = ((), (5,), (2, 3), (0,))
    options = ((False, False), (True, False), (True, True), (False, True))   # bias, relu

    forms = {}

    # ---- the four forms at 96 x 40
    def section_0():
        for k in (4, 16, 200, 300):
            lab = labels_of(KDIM * NCOLS, k, wide=k > 256)
            cen, bias = f32(k), f32(NCOLS)
            forms["byte", k] = (lab, cen, bias)
            if k <= 256:
                forms["grouped", k] = (lab, f32(3, k), bias)
                forms["sparse", k] = (ops.pack_sparse_codes(lab, KDIM, NCOLS, k), cen, bias)
            if k <= 16:
                forms["packed", k] = (ops.pack_codes(lab, KDIM, NCOLS, k), cen, bias)
        forward = {"byte": lambda x, i, c, **kw: ops.codebook_matmul(x, i, c, KDIM, NCOLS, **kw),
                   "grouped": lambda x, i, c, **kw: ops.grouped_codebook_matmul(x, i, c, KDIM, NCOLS, GROUP_ROWS, **kw),
                   "sparse": ops.sparse_codebook_matmul, "packed": ops.packed_codebook_matmul}
        dx = {"byte": lambda g, i, c: ops.codebook_matmul_dx(g, i, c, KDIM, NCOLS), "sparse": ops.sparse_codebook_matmul_dx,
              "packed": ops.packed_codebook_matmul_dx}
        dc = {"byte": lambda x, g, i, c, **kw: ops.codebook_centroid_grad(x, g, i, c.numel(), KDIM, NCOLS, **kw),
              "sparse": lambda x, g, i, c, **kw: ops.sparse_codebook_centroid_grad(x, g, i, **kw),
              "packed": lambda x, g, i, c, **kw: ops.packed_codebook_centroid_grad(x, g, i, **kw)}
        linear = {"byte": lambda x, i, c, b, r: ops.codebook_linear(x, i, c, KDIM, NCOLS, bias=b, relu=r),
                  "sparse": lambda x, i, c, b, r: ops.sparse_codebook_linear(x, i, c, bias=b, relu=r),
                  "packed": lambda x, i, c, b, r: ops.packed_codebook_linear(x, i, c, bias=b, relu=r)}

        def linear_grads(fn, x, index, cen, bias, relu, gy):
            x, cen = x.clone().requires_grad_(True), cen.clone().requires_grad_(True)
            bias = None if bias is None else bias.clone().requires_grad_(True)
            y = fn(x, index, cen, bias, relu)
            y.backward(gy)
            return y, x.grad, cen.grad, None if bias is None else bias.grad

        for (form, k), (index, cen, bias) in forms.items():
            for lead in leads:
                x, g = f32(*lead, KDIM), f32(*lead, NCOLS)
                tag = f"{form} K={k} x={lead + (KDIM,)}"
                with torch.no_grad():
                    for has_bias, relu in options:
                        rec.call(f"forward {tag} bias={has_bias} relu={relu}",
                                 lambda: forward[form](x, index, cen, bias=bias if has_bias else None, relu=relu))
                    if form in ("byte", "grouped"):
                        for dt in (torch.bfloat16, torch.float16):
                            for out_dtype in (None, torch.float32):
                                rec.call(f"forward {tag} {dt} out={out_dtype}",
                                         lambda: forward[form](x.to(dt), index, cen, bias=bias, relu=True, out_dtype=out_dtype))
                    if form == "grouped":
                        continue
                    rec.call(f"dx {tag}", lambda: dx[form](g, index, cen))
                    for dt in (torch.float64, torch.float32):
                        rec.call(f"dc {tag} {dt}", lambda: dc[form](x, g, index, cen, dtype=dt))
                for has_bias, relu in options:
                    rec.call(f"linear {tag} bias={has_bias} relu={relu}",
                             lambda: linear_grads(linear[form], x, index, cen, bias if has_bias else None, relu, g))

    # ---- one shape per product whose plan splits the reduction: the workspace path
    def section_1():
        def first_split(plan):
            shapes = ((1024, 40), (4096, 40), (16384, 40), (4096, 64), (16384, 64), (40, 4096), (64, 16384), (65536, 40), (40, 65536))
            for m, kd, nc in [(1,) + s for s in shapes] + [(256, KDIM, NCOLS), (4096, KDIM, NCOLS), (4096, 1024, 40)]:   # dc splits the rows
                if plan(m, kd, nc)["splits"] > 1:
                    return m, kd, nc
            return None

        def split_case(name, plan, run):
            shape = first_split(plan)
            rec.put(f"split shape {name}", shape)
            if shape is None:   # a workspace path that was never run must not pass as "same"
                rec.put(f"tool error in: no shape with splits > 1 found for {name}", "extend the candidates of first_split")
                return
            m, kd, nc = shape
            lab = labels_of(kd * nc, 16)
            with torch.no_grad():
                rec.call(f"split {name} m={m} {kd} x {nc}", lambda: run(kd, nc, lab, f32(16), f32(m, kd), f32(m, nc), f32(nc)))

        split_case("byte forward", lambda m, kd, nc: ops.cbmm_plan(m, kd, nc, 1, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.codebook_matmul(x, lab, c, kd, nc, bias=b, relu=True))
        for dt in (torch.bfloat16, torch.float16):
            split_case(f"byte forward {dt}", lambda m, kd, nc: ops.cbmm_h16_plan(dt, m, kd, nc, 1, 16, cus),
                       lambda kd, nc, lab, c, x, g, b: ops.codebook_matmul(x.to(dt), lab, c, kd, nc, bias=b, relu=True))
        split_case("byte dx", lambda m, kd, nc: ops.cbmm_dx_plan(m, kd, nc, 1, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.codebook_matmul_dx(g, lab, c, kd, nc))
        split_case("byte dc", lambda m, kd, nc: ops.cbmm_dc_plan(m, kd, nc, 1, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.codebook_centroid_grad(x, g, lab, 16, kd, nc))
        split_case("grouped forward", lambda m, kd, nc: ops.cbmm_grouped_plan(torch.float32, m, kd, nc, 16, GROUP_ROWS, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.grouped_codebook_matmul(x, lab, f32(-(-kd // GROUP_ROWS), 16), kd, nc, GROUP_ROWS, bias=b))
        split_case("sparse forward", lambda m, kd, nc: ops.cbsp_plan(m, kd, nc, 1, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.sparse_codebook_matmul(x, ops.pack_sparse_codes(lab, kd, nc, 16), c, bias=b, relu=True))
        split_case("sparse dx", lambda m, kd, nc: ops.cbsp_dx_plan(m, kd, nc, 1, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.sparse_codebook_matmul_dx(g, ops.pack_sparse_codes(lab, kd, nc, 16), c))
        split_case("sparse dc", lambda m, kd, nc: ops.cbsp_dc_plan(m, kd, nc, 1, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.sparse_codebook_centroid_grad(x, g, ops.pack_sparse_codes(lab, kd, nc, 16)))
        split_case("packed forward", lambda m, kd, nc: ops.cbpk_plan(m, kd, nc, 4, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.packed_codebook_matmul(x, ops.pack_codes(lab, kd, nc, 16), c, bias=b, relu=True))
        split_case("packed dx", lambda m, kd, nc: ops.cbpk_dx_plan(m, kd, nc, 4, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.packed_codebook_matmul_dx(g, ops.pack_codes(lab, kd, nc, 16), c))
        split_case("packed dc", lambda m, kd, nc: ops.cbpk_dc_plan(m, kd, nc, 4, 16, cus),
                   lambda kd, nc, lab, c, x, g, b: ops.packed_codebook_centroid_grad(x, g, ops.pack_codes(lab, kd, nc, 16)))

    # ---- the plan dicts
    def section_2():
        for m, kd, nc in ((1, 96, 40), (5, 96, 40), (16, 784, 300), (256, 4096, 4096), (1, 5000, 5000), (4096, 3072, 768)):
            for k, width in ((4, 1), (16, 1), (200, 1), (300, 2)):
                tag = f"m={m} {kd} x {nc} K={k}"
                rec.value(f"plan cbmm {tag}", lambda: ops.cbmm_plan(m, kd, nc, width, k, cus, labels_addr=64))
                rec.value(f"plan cbmm_dx {tag}", lambda: ops.cbmm_dx_plan(m, kd, nc, width, k, cus))
                rec.value(f"plan cbmm_dc {tag}", lambda: ops.cbmm_dc_plan(m, kd, nc, width, k, cus))
                rec.value(f"plan cbmm_h16 {tag}", lambda: ops.cbmm_h16_plan(torch.bfloat16, m, kd, nc, width, k, cus))
                rec.value(f"plan cbsp {tag}", lambda: ops.cbsp_plan(m, kd, nc, width, k, cus))
                rec.value(f"plan cbsp_dx {tag}", lambda: ops.cbsp_dx_plan(m, kd, nc, width, k, cus))
                rec.value(f"plan cbsp_dc {tag}", lambda: ops.cbsp_dc_plan(m, kd, nc, width, k, cus))
                if k <= 256:
                    rec.value(f"plan cbmm_grouped {tag}", lambda: ops.cbmm_grouped_plan(torch.float16, m, kd, nc, k, GROUP_ROWS, cus))
                if k <= 16:
                    bits = ops.packed_bits(k)
                    rec.value(f"plan cbpk {tag}", lambda: ops.cbpk_plan(m, kd, nc, bits, k, cus))
                    rec.value(f"plan cbpk_dx {tag}", lambda: ops.cbpk_dx_plan(m, kd, nc, bits, k, cus))
                    rec.value(f"plan cbpk_dc {tag}", lambda: ops.cbpk_dc_plan(m, kd, nc, bits, k, cus))
        rec.invalid("plan cbmm_h16 float32", lambda: ops.cbmm_h16_plan(torch.float32, 1, 96, 40, 1, 4, cus))
        rec.invalid("plan cbmm_grouped int8", lambda: ops.cbmm_grouped_plan(torch.int8, 1, 96, 40, 4, 32, cus))
        rec.invalid("plan cbmm m='a'", lambda: ops.cbmm_plan("a", 96, 40, 1, 4, cus))

    # ---- the layers
    def section_3():
        ks, cin, cout, pad = 3, 2, 4, 1
        k = 4
        dlab, clab = labels_of(KDIM * NCOLS, k), labels_of(ks * ks * cin * cout, k)
        cen, dbias, cbias = f32(k), f32(NCOLS), f32(cout)
        bcodes_d, bcodes_c = (f32(k), labels_of(NCOLS, k)), (f32(k), labels_of(cout, k))
        xd, xc = f32(5, KDIM), f32(2, 6, 6, cin)
        made = {"CompressedDense": lambda: C.CompressedDense(KDIM, NCOLS, dlab, cen, dbias, torch.relu),
                "GroupedCompressedDense": lambda: C.GroupedCompressedDense(KDIM, NCOLS, GROUP_ROWS, dlab, f32(3, k), dbias, torch.tanh)}
        for name in ("SparseCompressedDense", "PackedCompressedDense"):
            made[name] = lambda name=name: getattr(C, name).from_codes(KDIM, NCOLS, dlab, cen, dbias, torch.relu)
        for name in ("CompressedConv2D", "SparseCompressedConv2D", "PackedCompressedConv2D"):
            made[name] = lambda name=name: getattr(C, name).from_codes(ks, cin, cout, pad, clab, cen, cbias, torch.tanh)
        for quantized in (False, True):
            q = " bias_codes" if quantized else ""
            db, dcodes, cb, ccodes = (None, bcodes_d, None, bcodes_c) if quantized else (dbias, None, cbias, None)
            made["TrainableCompressedDense" + q] = lambda db=db, dcodes=dcodes: C.TrainableCompressedDense(KDIM, NCOLS, dlab, cen, db, dcodes, torch.relu)
            made["TrainableCompressedConv2D" + q] = lambda cb=cb, ccodes=ccodes: C.TrainableCompressedConv2D(
                ks, cin, cout, pad, C._unfold_labels(ks, cin, cout, clab), cen, cb, ccodes, torch.tanh)
            for name in ("TrainableSparseCompressedDense", "TrainablePackedCompressedDense"):
                made[name + q] = lambda name=name, db=db, dcodes=dcodes: getattr(C, name).from_codes(KDIM, NCOLS, dlab, cen, db, dcodes, torch.relu)
            for name in ("TrainableSparseCompressedConv2D", "TrainablePackedCompressedConv2D"):
                made[name + q] = lambda name=name, cb=cb, ccodes=ccodes: getattr(C, name).from_codes(ks, cin, cout, pad, clab, cen, cb, ccodes, torch.tanh)
        bases = ("_CodebookLayer", "_SparseCodebookLayer", "_PackedCodebookLayer", "_TrainableCentres", "_TrainableCodebookLayer",
                 "_TrainableSparseCodebookLayer", "_TrainablePackedCodebookLayer", "GroupedCompressedDense")
        for name, make in made.items():
            layer = make()
            x = xc if "Conv2D" in name else xd
            rec.put(f"layer {name} state", {"state_dict": [[n, str(t.dtype), list(t.shape)] for n, t in layer.state_dict().items()],
                                            "parameters": [n for n, _ in layer.named_parameters()],
                                            "buffers": [[n, str(b.dtype), list(b.shape)] for n, b in layer.named_buffers()],
                                            "isinstance": [b for b in bases if isinstance(layer, getattr(C, b))],
                                            "nbytes": layer.nbytes(), "compressed_nbytes": C.compressed_nbytes(layer), "get_weights": layer.get_weights()})
            for n, t in layer.state_dict().items():
                rec.tensor(f"layer {name} state {n}", t)
            with torch.no_grad():
                rec.call(f"layer {name} forward", lambda: layer(x))
                rec.call(f"layer {name} forward empty batch", lambda: layer(x[:0]))
            if name.startswith("Trainable"):
                rec.call(f"layer {name} kernel_sq_sum", layer.kernel_sq_sum)

                def grads():
                    layer.zero_grad()
                    xg = x.clone().requires_grad_(True)
                    (layer(xg).square().sum() + layer.kernel_sq_sum()).backward()
                    return (xg.grad,) + tuple(p.grad for p in layer.parameters())
                rec.call(f"layer {name} backward", grads)
            else:
                rec.invalid(f"layer {name} forward under autograd", lambda: layer(x.clone().requires_grad_(True)))
            rec.invalid(f"layer {name} float64 x", lambda: layer(x.double()))
            if "Sparse" in name or "Packed" in name or name.startswith("Trainable"):
                rec.invalid(f"layer {name} half x", lambda: layer(x.half()))

        dense, conv = layers.Dense(KDIM, NCOLS, activation=torch.relu).to(dev), layers.Conv2D(cin, cout, ks, padding="same").to(dev)
        for name in ("CompressedDense", "GroupedCompressedDense", "SparseCompressedDense", "PackedCompressedDense",
                     "TrainableSparseCompressedDense", "TrainablePackedCompressedDense"):
            rec.invalid(f"{name}.from_dense no model", lambda: getattr(C, name).from_dense(dense, None))
        for name in ("CompressedConv2D", "SparseCompressedConv2D", "PackedCompressedConv2D", "TrainableSparseCompressedConv2D",
                     "TrainablePackedCompressedConv2D"):
            rec.invalid(f"{name}.from_conv no model", lambda: getattr(C, name).from_conv(conv, None))
        rec.invalid("_trainable no model", lambda: C._trainable(dense, None, None))
        rec.invalid("_trainable no model, no layer", lambda: C._trainable(layers.Weightless(torch.relu), None, None))
        rec.invalid("CompressedDense labels short", lambda: C.CompressedDense(KDIM, NCOLS, dlab[:-1], cen, dbias))
        rec.invalid("GroupedCompressedDense int16 labels", lambda: C.GroupedCompressedDense(KDIM, NCOLS, GROUP_ROWS, dlab.to(torch.int16), f32(3, k), dbias))
        rec.invalid("GroupedCompressedDense two groups", lambda: C.GroupedCompressedDense(KDIM, NCOLS, GROUP_ROWS, dlab, f32(2, k), dbias))
        rec.invalid("SparseCompressedDense centres short", lambda: C.SparseCompressedDense(forms["sparse", 4][0], f32(3), dbias))
        rec.invalid("PackedCompressedDense centres short", lambda: C.PackedCompressedDense(forms["packed", 4][0], f32(3), dbias))
        rec.invalid("SparseCompressedConv2D wrong rows", lambda: C.SparseCompressedConv2D(ks, cin, pad, forms["sparse", 4][0], cen, None))
        rec.invalid("PackedCompressedConv2D wrong rows", lambda: C.PackedCompressedConv2D(ks, cin, pad, forms["packed", 4][0], cen, None))
        rec.invalid("TrainablePackedCompressedConv2D wrong rows, centres short",
                    lambda: C.TrainablePackedCompressedConv2D(ks, cin, pad, forms["packed", 4][0], dlab, f32(3)))
        rec.invalid("TrainableSparseCompressedDense labels short, centres short",
                    lambda: C.TrainableSparseCompressedDense(forms["sparse", 4][0], dlab[:-1], f32(3)))
        rec.invalid("TrainableCompressedDense bias codes short", lambda: C.TrainableCompressedDense(KDIM, NCOLS, dlab, cen, None, (f32(k), dlab[:7])))
        rec.invalid("PackedCompressedConv2D.from_codes K=17", lambda: C.PackedCompressedConv2D.from_codes(ks, cin, cout, pad, clab[:-1], f32(17), None, None))
        rec.invalid("compress_network_trainable packed='yes'", lambda: C.compress_network_trainable(None, {}, packed="yes"))

    # ---- invalid calls of the ops: none reaches a kernel
    def section_4():
        x, g = f32(5, KDIM), f32(5, NCOLS)
        lab, cen, bias = forms["byte", 4]
        cpu = lambda t: t.cpu()   # noqa: E731
        needs = lambda t: t.clone().requires_grad_(True)   # noqa: E731
        xt = f32(KDIM, 5).t()   # (5, KDIM), not contiguous
        b = rec.invalid
        mm = lambda x=x, lab=lab, cen=cen, bias=bias, **kw: ops.codebook_matmul(x, lab, cen, KDIM, NCOLS, bias=bias, **kw)   # noqa: E731
        b("byte x on the CPU", lambda: mm(x=cpu(x)))
        b("byte x a list", lambda: mm(x=[1.0]))
        b("byte labels on the CPU", lambda: mm(lab=cpu(lab)))
        b("byte centers on the CPU", lambda: mm(cen=cpu(cen)))
        b("byte bias on the CPU", lambda: mm(bias=cpu(bias)))
        b("byte x float64", lambda: mm(x=x.double()))
        b("byte centers float64", lambda: mm(cen=cen.double()))
        b("byte bias float16", lambda: mm(bias=bias.half()))
        b("byte labels int32", lambda: mm(lab=lab.to(torch.int32)))
        b("byte x not contiguous", lambda: mm(x=xt))
        b("byte x last dimension", lambda: mm(x=f32(5, KDIM + 1)))
        b("byte x 0-d", lambda: mm(x=f32()))
        b("byte bias length", lambda: mm(bias=f32(NCOLS + 1)))
        b("byte labels count", lambda: mm(lab=lab[:-1]))
        b("byte x requires grad", lambda: mm(x=needs(x)))
        b("byte centers requires grad", lambda: mm(cen=needs(cen)))
        b("byte bias requires grad", lambda: mm(bias=needs(bias)))
        b("byte out_dtype float16 for float32 x", lambda: mm(out_dtype=torch.float16))
        b("byte out_dtype bfloat16 for float16 x", lambda: mm(x=x.half(), out_dtype=torch.bfloat16))
        b("byte two: x on the CPU, bias length", lambda: mm(x=cpu(x), bias=f32(3)))
        b("byte two: x last dimension, bias length", lambda: mm(x=f32(5, 7), bias=f32(3)))
        b("byte two: requires grad, labels count", lambda: mm(x=needs(x), lab=lab[:-1]))
        b("byte two: centers float64, labels on the CPU", lambda: mm(cen=cen.double(), lab=cpu(lab)))
        b("byte two: x not contiguous, out_dtype", lambda: mm(x=xt, out_dtype=torch.float16))
        b("byte two: half x on the CPU, out_dtype", lambda: mm(x=cpu(x).half(), out_dtype=torch.float16))
        b("byte two: labels int32, bias length", lambda: mm(lab=lab.to(torch.int32), bias=f32(3)))
        bdx = lambda g=g, lab=lab, cen=cen: ops.codebook_matmul_dx(g, lab, cen, KDIM, NCOLS)   # noqa: E731
        b("byte dx g on the CPU", lambda: bdx(g=cpu(g)))
        b("byte dx g float64", lambda: bdx(g=g.double()))
        b("byte dx g last dimension", lambda: bdx(g=f32(5, NCOLS - 1)))
        b("byte dx labels count", lambda: bdx(lab=lab[:-1]))
        b("byte dx centers on the CPU", lambda: bdx(cen=cpu(cen)))
        b("byte dx no centres", lambda: bdx(cen=f32(0)))
        b("byte dx labels int32", lambda: bdx(lab=lab.to(torch.int32)))
        b("byte dx two: g last dimension, labels count", lambda: bdx(g=f32(5, 3), lab=lab[:-1]))
        b("byte dx two: centers on the CPU, g on the CPU", lambda: bdx(cen=cpu(cen), g=cpu(g)))
        b("byte dx two: g not contiguous, no centres", lambda: bdx(g=f32(NCOLS, 5).t(), cen=f32(0)))
        bdc = lambda x=x, g=g, lab=lab, k=4, **kw: ops.codebook_centroid_grad(x, g, lab, k, KDIM, NCOLS, **kw)   # noqa: E731
        b("byte dc x on the CPU", lambda: bdc(x=cpu(x)))
        b("byte dc g on the CPU", lambda: bdc(g=cpu(g)))
        b("byte dc leading shapes", lambda: bdc(x=f32(4, KDIM)))
        b("byte dc x last dimension", lambda: bdc(x=f32(5, KDIM - 1)))
        b("byte dc dtype int32", lambda: bdc(dtype=torch.int32))
        b("byte dc k = 0", lambda: bdc(k=0))
        b("byte dc k = 300 on uint8 labels", lambda: bdc(k=300))
        b("byte dc k above the limit", lambda: bdc(k=nat.NNC_KMAX + 1))
        b("byte dc two: dtype int32, leading shapes", lambda: bdc(dtype=torch.int32, x=f32(4, KDIM)))
        b("byte dc two: x last dimension, g last dimension", lambda: bdc(x=f32(5, 3), g=f32(5, 3)))
        b("byte dc two: k = 300, dtype int32", lambda: bdc(k=300, dtype=torch.int32))
        b("byte linear half x", lambda: ops.codebook_linear(x.half(), lab, cen, KDIM, NCOLS))
        b("byte linear x last dimension", lambda: ops.codebook_linear(needs(f32(5, 7)), lab, cen, KDIM, NCOLS))
        b("byte linear bias length", lambda: ops.codebook_linear(x, lab, needs(cen), KDIM, NCOLS, bias=f32(3)))

        glab, gcen, gbias = forms["grouped", 4]
        gm = lambda x=x, lab=glab, cen=gcen, bias=gbias, rows=GROUP_ROWS, **kw: ops.grouped_codebook_matmul(   # noqa: E731
            x, lab, cen, KDIM, NCOLS, rows, bias=bias, **kw)
        b("grouped x on the CPU", lambda: gm(x=cpu(x)))
        b("grouped x int32", lambda: gm(x=x.to(torch.int32)))
        b("grouped x a list", lambda: gm(x=[1.0]))
        b("grouped labels on the CPU", lambda: gm(lab=cpu(glab)))
        b("grouped labels int16", lambda: gm(lab=glab.to(torch.int16)))
        b("grouped centers on the CPU", lambda: gm(cen=cpu(gcen)))
        b("grouped centers float64", lambda: gm(cen=gcen.double()))
        b("grouped bias on the CPU", lambda: gm(bias=cpu(gbias)))
        b("grouped x not contiguous", lambda: gm(x=xt))
        b("grouped x last dimension", lambda: gm(x=f32(5, KDIM + 1)))
        b("grouped bias length", lambda: gm(bias=f32(NCOLS - 1)))
        b("grouped labels count", lambda: gm(lab=glab[:-1]))
        b("grouped centers one row", lambda: gm(cen=f32(4)))
        b("grouped centers two groups", lambda: gm(cen=f32(2, 4)))
        b("grouped centers K = 257", lambda: gm(cen=f32(3, 257)))
        b("grouped group_rows 33", lambda: gm(rows=33))
        b("grouped group_rows 0", lambda: gm(rows=0))
        b("grouped x requires grad", lambda: gm(x=needs(x)))
        b("grouped centers requires grad", lambda: gm(cen=needs(gcen)))
        b("grouped out_dtype float16", lambda: gm(out_dtype=torch.float16))
        b("grouped two: group_rows 33, x last dimension", lambda: gm(rows=33, x=f32(5, 7)))
        b("grouped two: requires grad, group_rows 0", lambda: gm(x=needs(x), rows=0))
        b("grouped two: labels int16, centers on the CPU", lambda: gm(lab=glab.to(torch.int16), cen=cpu(gcen)))
        b("grouped two: centers two groups, bias length", lambda: gm(cen=f32(2, 4), bias=f32(3)))
        b("grouped two: out_dtype, labels on the CPU", lambda: gm(out_dtype=torch.float16, lab=cpu(glab)))

        for form, other in (("sparse", "packed"), ("packed", "sparse")):
            codes, cen, bias = forms[form, 4]
            wrong = forms[other, 4][0]
            fw, fdx, fdc, flin = (getattr(ops, f"{form}_codebook_{what}") for what in ("matmul", "matmul_dx", "centroid_grad", "linear"))
            fm = lambda x=x, codes=codes, cen=cen, bias=bias, fw=fw, **kw: fw(x, codes, cen, bias=bias, **kw)   # noqa: E731
            b(f"{form} x on the CPU", lambda: fm(x=cpu(x)))
            b(f"{form} centers on the CPU", lambda: fm(cen=cpu(cen)))
            b(f"{form} bias on the CPU", lambda: fm(bias=cpu(bias)))
            b(f"{form} x float64", lambda: fm(x=x.double()))
            b(f"{form} x bfloat16", lambda: fm(x=x.bfloat16()))
            b(f"{form} x float16", lambda: fm(x=x.half()))
            b(f"{form} centers float16", lambda: fm(cen=cen.half()))
            b(f"{form} x not contiguous", lambda: fm(x=xt))
            b(f"{form} x last dimension", lambda: fm(x=f32(5, KDIM + 1)))
            b(f"{form} x 0-d", lambda: fm(x=f32()))
            b(f"{form} bias length", lambda: fm(bias=f32(NCOLS + 1)))
            b(f"{form} centers count", lambda: fm(cen=f32(5)))
            b(f"{form} x requires grad", lambda: fm(x=needs(x)))
            b(f"{form} bias requires grad", lambda: fm(bias=needs(bias)))
            b(f"{form} codes of the other form", lambda: fm(codes=wrong))
            b(f"{form} codes a tensor", lambda: fm(codes=lab))
            b(f"{form} two: codes of the other form, x on the CPU", lambda: fm(codes=wrong, x=cpu(x)))
            b(f"{form} two: codes a tensor, x requires grad", lambda: fm(codes=lab, x=needs(x)))
            b(f"{form} two: half x on the CPU", lambda: fm(x=cpu(x).half()))
            b(f"{form} two: centers count, bias length", lambda: fm(cen=f32(5), bias=f32(3)))
            b(f"{form} two: x last dimension, centers count", lambda: fm(x=f32(5, 7), cen=f32(5)))
            b(f"{form} two: requires grad, x last dimension", lambda: fm(x=needs(f32(5, 7))))
            b(f"{form} dx g on the CPU", lambda: fdx(cpu(g), codes, cen))
            b(f"{form} dx centers on the CPU", lambda: fdx(g, codes, cpu(cen)))
            b(f"{form} dx g last dimension", lambda: fdx(f32(5, NCOLS + 1), codes, cen))
            b(f"{form} dx centers count", lambda: fdx(g, codes, f32(5)))
            b(f"{form} dx codes of the other form", lambda: fdx(g, wrong, cen))
            b(f"{form} dx two: codes of the other form, g float64", lambda: fdx(g.double(), wrong, cen))
            b(f"{form} dx two: g last dimension, centers count", lambda: fdx(f32(5, 3), codes, f32(5)))
            b(f"{form} dc x on the CPU", lambda: fdc(cpu(x), g, codes))
            b(f"{form} dc g float64", lambda: fdc(x, g.double(), codes))
            b(f"{form} dc leading shapes", lambda: fdc(f32(4, KDIM), g, codes))
            b(f"{form} dc dtype int32", lambda: fdc(x, g, codes, dtype=torch.int32))
            b(f"{form} dc codes of the other form", lambda: fdc(x, g, wrong))
            b(f"{form} dc two: dtype int32, leading shapes", lambda: fdc(f32(2, 3, KDIM), g, codes, dtype=torch.int32))
            b(f"{form} dc two: codes a tensor, x on the CPU", lambda: fdc(cpu(x), g, lab))
            b(f"{form} linear half x", lambda: flin(x.half(), codes, cen))
            b(f"{form} linear codes of the other form", lambda: flin(x, wrong, cen))
            b(f"{form} linear two: codes a tensor, half x", lambda: flin(x.half(), lab, cen))
            b(f"{form} linear centers count", lambda: flin(needs(x), codes, f32(5)))

    for section, title in ((section_0, "the four forms at 96 x 40"), (section_1, "one shape per product whose plan splits"), (section_2, "the plan dicts"),
                           (section_3, "the layers"), (section_4, "invalid calls of the ops")):
        try:
            section()
        except Exception as e:   # noqa: BLE001 - a fault of this tool, not of a wrapper: reported as one, the other sections still run
            rec.put("tool error in: " + title, traceback.format_exc())
            if _device_fault(e):
                raise   # the device faulted: the child ends with a non-zero status, and the launcher starts nothing more
    torch.cuda.synchronize()


def _child_host_time(torch, np, ops, rec, calls=2000, warm=200):
    import time

    dev = "cuda"
    rng = np.random.RandomState(7)
    n, k = 256, 16
    lab = torch.from_numpy(rng.randint(0, k, size=n * n).astype(np.uint8)).to(dev)
    cen = torch.from_numpy(rng.standard_normal(k).astype(np.float32)).to(dev)
    gcen = torch.from_numpy(rng.standard_normal((n // 64, k)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((1, n)).astype(np.float32)).to(dev)
    sparse, packed = ops.pack_sparse_codes(lab, n, n, k), ops.pack_codes(lab, n, n, k)
    forms = {"byte": lambda: ops.codebook_matmul(x, lab, cen, n, n), "grouped": lambda: ops.grouped_codebook_matmul(x, lab, gcen, n, n, 64),
             "sparse": lambda: ops.sparse_codebook_matmul(x, sparse, cen), "packed": lambda: ops.packed_codebook_matmul(x, packed, cen)}
    with torch.no_grad():
        for form, call in forms.items():
            for _ in range(warm):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            rec.put(form, (time.perf_counter() - t0) / calls * 1e6)


def _child(phase: str, root: str, result: str) -> int:
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    import numpy as np
    import torch

    import neural_network_compression_amd as pkg
    from neural_network_compression_amd import compressed, ops

    if not os.path.abspath(pkg.__file__).startswith(root + os.sep):
        print(f"child: the package came from {pkg.__file__}, not from {root}", file=sys.stderr)
        return 3
    if not torch.cuda.is_available():
        print("child: no GPU: this comparison runs the HIP kernels, there is nothing to fall back to", file=sys.stderr)
        return 3
    rec = _Recorder(torch)
    try:   # an exception that gets here (a device fault among them) ends the child with a non-zero status
        if phase == "results":
            _child_results(torch, np, ops, compressed, rec)
        else:
            _child_host_time(torch, np, ops, rec)
    finally:
        with open(result, "w") as f:
            json.dump(rec.records, f)
    return 0


# ------------------------------------------------------------------ the launcher
class _Stop(Exception):
    pass


def _run_child(phase: str, root: str, result: str, limit: int):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", phase, "--root", root, "--result", result]
    status = subprocess.run(cmd, cwd=root).returncode
    if status in FATAL or status < 0:
        raise _Stop(f"the {phase} child of {root} ended with status {status}: nothing more is started")
    if status != 0:
        raise _Stop(f"the {phase} child of {root} failed with status {status}")
    with open(result) as f:
        return json.load(f)


def _results(other: str, tmp: str, emit) -> int:
    mine = _run_child("results", ROOT, os.path.join(tmp, "results_this.json"), 420)
    theirs = _run_child("results", other, os.path.join(tmp, "results_other.json"), 420)
    different = 0
    for case in list(mine) + [c for c in theirs if c not in mine]:
        same = case in mine and case in theirs and mine[case] == theirs[case] and not case.startswith("tool error")
        line = {"phase": "results", "case": case, "same": same}
        if not same:
            different += 1
            line.update(this=mine.get(case, "missing"), other=theirs.get(case, "missing"))
        emit(line)
    emit({"phase": "results", "cases": len(set(mine) | set(theirs)), "different": different})
    return different


def _host_time(other: str, tmp: str, repeats: int, emit) -> int:
    runs = {"this": [], "other": []}
    for i in range(repeats):   # the two alternate, the yardstick first
        for who, root in (("other", other), ("this", ROOT)):
            runs[who].append(_run_child("host-time", root, os.path.join(tmp, f"host_{who}_{i}.json"), 180))
            emit({"phase": "host-time", "checkout": who, "repeat": i, "us_per_call": {f: round(v, 3) for f, v in runs[who][-1].items()}})
    missed = 0
    for form in runs["other"][0]:
        this, base = [r[form] for r in runs["this"]], [r[form] for r in runs["other"]]
        spread = max(base) - min(base)
        ok = statistics.median(this) <= statistics.median(base) + spread
        missed += not ok
        emit({"phase": "host-time", "form": form, "this_median_us": round(statistics.median(this), 3),
              "other_median_us": round(statistics.median(base), 3), "other_spread_us": round(spread, 3),
              "this_spread_us": round(max(this) - min(this), 3), "repeats": repeats, "target": "met" if ok else "missed", "note": NOTE})
    return missed


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("other", nargs="?", metavar="OTHER_CHECKOUT", help="the checkout to compare with (its library built)")
    ap.add_argument("--out", help="also write the JSON lines here")
    ap.add_argument("--phase", choices=("results", "host-time", "all"), default="all")
    ap.add_argument("--repeats", type=int, default=5, help="host-time runs per checkout (at least five)")
    ap.add_argument("--child", choices=("results", "host-time"), help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    ap.add_argument("--result", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return _child(args.child, args.root, args.result)
    if not args.other:
        ap.error("OTHER_CHECKOUT is required")
    other = os.path.abspath(args.other)
    if not os.path.isfile(os.path.join(other, "neural_network_compression_amd", "ops.py")):
        ap.error(f"{other} holds no neural_network_compression_amd/ops.py")
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    lines = []

    def emit(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    bad, stopped = 0, False
    try:
        with tempfile.TemporaryDirectory() as tmp:
            if args.phase in ("results", "all"):
                bad += _results(other, tmp, emit)
            if args.phase in ("host-time", "all"):
                bad += _host_time(other, tmp, args.repeats, emit)
    except _Stop as e:
        emit({"stopped": str(e)})
        stopped = True
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 2 if stopped else 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
