"""Device-level operators: thin torch-tensor wrappers over the C ABI (include/nnc.h).

Every function takes CUDA (ROCm) tensors that are already resident in HBM, enqueues HIP
kernels from csrc/nnc_hip.hip on torch's current stream and returns device tensors; none
of them synchronises unless its docstring says so.  PyTorch is plumbing here (memory,
streams); the arithmetic is in the HIP kernels.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import threading
import math

import numpy as np
import torch

from . import _native as nat


def _require_cuda(t: torch.Tensor, name: str, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (ROCm) torch tensor resident in HBM")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _require_f32_x(x, who: str):
    """The entry points that have no half-precision kernels: a bfloat16 / float16 x names the one form that has."""
    if isinstance(x, torch.Tensor) and x.dtype in (torch.bfloat16, torch.float16):
        raise TypeError(f"{who} takes float32 activations, got {x.dtype}: bfloat16 and float16 inputs run on the byte form "
                        "(ops.codebook_matmul and ops.codebook_linear; CompressedDense / CompressedConv2D, and their trainable "
                        "layers built with half_inputs=True) and on the bitmap-sparse form (ops.sparse_codebook_matmul and "
                        "ops.sparse_codebook_linear; the sparse layers built with half_inputs=True) and on the 2- / 4-bit packed form "
                        "(ops.packed_codebook_matmul and ops.packed_codebook_linear; the packed layers built with half_inputs=True)")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


_STAGE = threading.local()
_STAGE_SLOTS, _STAGE_BYTES = 16, 8192


def small_to_device(arr: np.ndarray, dev) -> torch.Tensor:
    """A few kilobytes of host data (initial centres, histogram steps) to the device without the blocking staging copy a pageable
    source costs: through a ring of pinned slots of this host thread, asynchronously on the current stream.  A slot is reused
    only after the copy that last read it has completed (an event per slot)."""
    arr = np.ascontiguousarray(arr)
    nb = arr.nbytes
    if nb == 0 or nb > _STAGE_BYTES:
        return torch.from_numpy(arr).to(dev)
    ring = getattr(_STAGE, "ring", None)
    if ring is None:
        ring = _STAGE.ring = {"buf": torch.empty(_STAGE_SLOTS * _STAGE_BYTES, dtype=torch.uint8, pin_memory=True),
                              "ev": [None] * _STAGE_SLOTS, "next": 0}
    i = ring["next"]
    ring["next"] = (i + 1) % _STAGE_SLOTS
    if ring["ev"][i] is not None:
        ring["ev"][i].synchronize()
    slot = ring["buf"][i * _STAGE_BYTES: i * _STAGE_BYTES + nb]
    slot.numpy()[:] = arr.view(np.uint8).reshape(-1)
    out = torch.empty(nb, dtype=torch.uint8, device=dev)
    out.copy_(slot, non_blocking=True)
    ev = ring["ev"][i] = ring["ev"][i] or torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return out.view(torch.from_numpy(arr).dtype).reshape(arr.shape)


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def device_info():
    L = nat.load()
    buf = ctypes.create_string_buffer(64)
    cu = ctypes.c_int(0)
    nat.check(L.nnc_device_info(buf, 64, ctypes.byref(cu)))
    return buf.value.decode(), cu.value


# ------------------------------------------------------------------ NumPy-exact reductions
def chunk_sums(x: torch.Tensor, mean_dev: torch.Tensor | None = None) -> torch.Tensor:
    """Per-8192-chunk NumPy pairwise sums of x (or of (x-mean)^2 when mean_dev is given)."""
    _require_cuda(x, "x", torch.float32)
    L = nat.load()
    n = x.numel()
    out = torch.empty((n + nat.NNC_CHUNK - 1) // nat.NNC_CHUNK, dtype=torch.float32, device=x.device)
    nat.check(L.nnc_chunk_sums_f32(_ptr(x), n, 1 if mean_dev is not None else 0, _ptr(mean_dev), _ptr(out), _stream(x)))
    return out


def fold(chunks: torch.Tensor, count: int, op: int, scale_dev: torch.Tensor | None = None) -> torch.Tensor:
    """Left-to-right float32 fold; returns a device float32[2] = {result, result*scale}."""
    _require_cuda(chunks, "chunks", torch.float32)
    L = nat.load()
    out = torch.empty(2, dtype=torch.float32, device=chunks.device)   # [1] is written only with a scale; nobody reads it otherwise
    nat.check(L.nnc_fold_f32(_ptr(chunks), chunks.numel(), int(count), op, _ptr(scale_dev), _ptr(out), _stream(chunks)))
    return out


def _gather_chunks(chunks: torch.Tensor, group) -> torch.Tensor:
    from . import sharding

    return sharding.gather_chunks(chunks, group)


def moments(x: torch.Tensor, n_total: int | None = None, group=None):
    """NumPy-exact float32 (mean, var, std) of the whole vector, as device tensors.

    Sharded (``group`` given): every rank passes its shard, shards start on multiples of
    8192 elements; the chunk sums are all-gathered and folded identically on every rank."""
    n_total = x.numel() if n_total is None else int(n_total)
    c1 = chunk_sums(x)
    if group is not None:
        c1 = _gather_chunks(c1, group)
    mean = fold(c1, n_total, nat.FOLD_MEAN)
    c2 = chunk_sums(x, mean)
    if group is not None:
        c2 = _gather_chunks(c2, group)
    var = fold(c2, n_total, nat.FOLD_MEAN)
    std = fold(c2, n_total, nat.FOLD_STD)
    return mean[0:1], var[0:1], std[0:1]


# ------------------------------------------------------------------ prune
def prune_(x: torch.Tensor, q: float, std_smooth: bool = True):
    """In place: mask = |x| < (std(x)*q | q); x[mask] = 0.  Returns (mask uint8, stats float32[2]
    = {sigma, thr}, nzeroed int64[1]) as device tensors.  q is taken as float32."""
    _require_cuda(x, "x", torch.float32)
    L = nat.load()
    n = x.numel()
    mask = torch.empty(n, dtype=torch.uint8, device=x.device)
    # (the library writes both: stats = {sigma, threshold} with std_smooth, {-, threshold} without; the count is zeroed there)
    stats = torch.empty(2, dtype=torch.float32, device=x.device) if std_smooth else torch.zeros(2, dtype=torch.float32, device=x.device)
    nz = torch.empty(1, dtype=torch.int64, device=x.device)
    ws_bytes = L.nnc_prune_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    nat.check(L.nnc_prune_f32(_ptr(x), n, float(np.float32(q)), 1 if std_smooth else 0, _ptr(mask), _ptr(stats),
                              _ptr(nz), _ptr(ws), ws_bytes, _stream(x)))
    return mask.view(x.shape), stats, nz


def prune_stats_(x: torch.Tensor, q: float, std_smooth: bool = True):
    """prune_ and, from the same pass, minmax_signs of the pruned tensor: (mask, stats, nzeroed, float32[4] = {min, max, min
    over the non-zeros, max over the non-zeros}, int64[2] = {#negative, #zero})."""
    _require_cuda(x, "x", torch.float32)
    if x.numel() == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    L = nat.load()
    n = x.numel()
    mask = torch.empty(n, dtype=torch.uint8, device=x.device)
    stats = torch.empty(2, dtype=torch.float32, device=x.device) if std_smooth else torch.zeros(2, dtype=torch.float32, device=x.device)
    nz = torch.empty(1, dtype=torch.int64, device=x.device)
    mm = torch.empty(4, dtype=torch.float32, device=x.device)
    signs = torch.empty(2, dtype=torch.int64, device=x.device)
    ws_bytes = L.nnc_prune_stats_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    nat.check(L.nnc_prune_stats_f32(_ptr(x), n, float(np.float32(q)), 1 if std_smooth else 0, _ptr(mask), _ptr(stats), _ptr(nz), _ptr(mm), _ptr(signs),
                                    _ptr(ws), ws_bytes, _stream(x)))
    return mask.view(x.shape), stats, nz, mm, signs


def threshold_mask_(x: torch.Tensor, thr_dev: torch.Tensor):
    """In place threshold pass with the float32 threshold already on the device."""
    _require_cuda(x, "x", torch.float32)
    _require_cuda(thr_dev, "thr_dev", torch.float32)
    L = nat.load()
    n = x.numel()
    mask = torch.empty(n, dtype=torch.uint8, device=x.device)
    nz = torch.empty(1, dtype=torch.int64, device=x.device)   # zeroed by the library
    nat.check(L.nnc_threshold_mask_f32(_ptr(x), n, _ptr(thr_dev), _ptr(mask), _ptr(nz), _stream(x)))
    return mask.view(x.shape), nz


def apply_mask_(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """x[mask] = 0 in place (Trainer._reset_pruned_parameters)."""
    _require_cuda(x, "x", torch.float32)
    _require_cuda(mask, "mask")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8 or mask.numel() != x.numel():
        raise ValueError("mask must be uint8/bool with as many elements as x")
    L = nat.load()
    nat.check(L.nnc_apply_mask_f32(_ptr(x), _ptr(mask), x.numel(), _stream(x)))
    return x


# ------------------------------------------------------------------ distribution passes
def minmax(x: torch.Tensor, skip_zeros: bool = False):
    """(float32[2] = {min, max}, int64[1] count) on the device."""
    _require_cuda(x, "x", torch.float32)
    if x.numel() == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    L = nat.load()
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    cnt = torch.empty(1, dtype=torch.int64, device=x.device)   # written by the final reduction
    ws_bytes = L.nnc_minmax_workspace_bytes(x.numel())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    nat.check(L.nnc_minmax_f32(_ptr(x), x.numel(), 1 if skip_zeros else 0, _ptr(out), _ptr(cnt), _ptr(ws), ws_bytes, _stream(x)))
    return out, cnt


def minmax_signs(x: torch.Tensor):
    """(float32[4] = {min, max, min over the non-zeros, max over the non-zeros}, int64[2] = {#negative, #zero})
    on the device, one pass."""
    _require_cuda(x, "x", torch.float32)
    if x.numel() == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    L = nat.load()
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    signs = torch.empty(2, dtype=torch.int64, device=x.device)
    ws_bytes = L.nnc_minmax_workspace_bytes(x.numel())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    nat.check(L.nnc_minmax_signs_f32(_ptr(x), x.numel(), _ptr(out), _ptr(signs), _ptr(ws), ws_bytes, _stream(x)))
    return out, signs


def hist31(x: torch.Tensor, steps: torch.Tensor, skip_zeros: bool = False) -> torch.Tensor:
    """int64[31] counts of steps[b] <= x < steps[b+1] (steps: device float32[32])."""
    _require_cuda(x, "x", torch.float32)
    _require_cuda(steps, "steps", torch.float32)
    if steps.numel() != 32:
        raise ValueError("steps must hold 32 values")
    L = nat.load()
    counts = torch.zeros(31, dtype=torch.int64, device=x.device)
    nat.check(L.nnc_hist31_f32(_ptr(x), x.numel(), 1 if skip_zeros else 0, _ptr(steps), _ptr(counts), _stream(x)))
    return counts


def bincount(labels: torch.Tensor, k: int) -> torch.Tensor:
    """int64[k] histogram of uint8 / uint16(int16 storage) centroid indices."""
    _require_cuda(labels, "labels")
    if labels.dtype == torch.uint8:
        lb = 1
    elif labels.dtype in (torch.int16, torch.uint16):
        lb = 2
    else:
        raise TypeError("labels must be uint8 or 16-bit")
    L = nat.load()
    counts = torch.zeros(int(k), dtype=torch.int64, device=labels.device)
    nat.check(L.nnc_bincount(_ptr(labels), lb, labels.numel(), int(k), _ptr(counts), _stream(labels)))
    return counts


def _label_bytes(labels: torch.Tensor) -> int:
    if labels.dtype == torch.uint8:
        return 1
    if labels.dtype in (torch.int16, torch.uint16):
        return 2
    raise TypeError("labels must be uint8 or 16-bit (QuantizedModel.labels_compact_)")


def centroid_gradient(grad: torch.Tensor, labels: torch.Tensor, k: int, group=None) -> torch.Tensor:
    """dL/dC_j = sum of dL/dW over the weights whose centroid index is j (Deep Compression's centroid fine-tuning,
    described but left out by the reference, papers/lat/report.tex:149-158) -> float64[k] on the device.
    Exact fixed-point sums (include/nnc.h, nnc_centroid_grad_f32): independent of order and, with ``group`` (every rank
    holds a shard of the layer), of the number of GPUs.  One host read (max |grad|) sizes the fixed point.  A NaN or Inf
    anywhere in ``grad`` (on any rank) makes every entry NaN, as codebook_centroid_grad does."""
    _require_cuda(grad, "grad", torch.float32)
    _require_cuda(labels, "labels")
    g = grad.reshape(-1)
    if labels.numel() != g.numel():
        raise ValueError("labels and grad must have the same number of elements")
    L = nat.load()
    n = g.numel()
    if n == 0:
        return torch.zeros(int(k), dtype=torch.float64, device=g.device)
    mm, _ = minmax(g)
    n_total = n
    if group is not None:
        from . import sharding

        mm = sharding.allreduce_minmax(mm, group)
        n_total = sharding.total_count(n, g.device, group)
    host = mm.cpu().numpy()
    S = fix_shift(float(max(abs(host[0]), abs(host[1]))), n_total)
    buf = torch.empty(int(k) + 1, dtype=torch.int64, device=g.device)   # the k sums, then the non-finite flag
    sums, nonfinite = buf[: int(k)], buf[int(k):]
    nat.check(L.nnc_centroid_grad_f32(_ptr(g), _ptr(labels), _label_bytes(labels), n, int(k), S, _ptr(sums), 0, _ptr(nonfinite), _stream(g)))
    if group is not None:
        from . import sharding

        sharding.allreduce_sum_(buf, group)   # the flags of every rank with the sums
    out = torch.ldexp(sums.to(torch.float64), torch.tensor(-S, device=g.device))
    return out.masked_fill_(nonfinite != 0, float("nan"))


def gather(centers: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """cluster_centers_[labels_] on the device (utility.py:239): float32 vector of labels.numel() values."""
    _require_cuda(centers, "centers", torch.float32)
    _require_cuda(labels, "labels")
    L = nat.load()
    out = torch.empty(labels.numel(), dtype=torch.float32, device=labels.device)
    nat.check(L.nnc_gather_f32(_ptr(centers), centers.numel(), _ptr(labels), _label_bytes(labels), labels.numel(), _ptr(out), _stream(labels)))
    return out


# ------------------------------------------------------------------ codebook products: the steps every index form shares
# The byte, grouped, bitmap-sparse, packed and grouped packed wrappers below run these in the same order; what differs per form (the dtype
# rule of x, the checks of the indices, the native call) stays in the form's own function, between them.
def _workspace(nbytes: int, dev) -> torch.Tensor | None:
    """The uint8 scratch of ``nbytes`` a native call asked for, or None when it needs none."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None


def _rows(t: torch.Tensor, name: str, last: int):
    """(lead, m) of ``t`` read as m rows of ``last`` values: its leading shape and their product, the last dimension checked."""
    if t.dim() < 1 or t.shape[-1] != last:
        raise ValueError(f"{name} must have shape (..., {last}), got {tuple(t.shape)}")
    lead = tuple(t.shape[:-1])
    return lead, (int(np.prod(lead)) if lead else 1)


def _require_centers_bias(centers, bias):
    _require_cuda(centers, "centers", torch.float32)
    if bias is not None:
        _require_cuda(bias, "bias", torch.float32)


def _one_device(names: str, *tensors):
    if len({t.device for t in tensors if t is not None}) != 1:
        raise ValueError(f"{names} must be on one device")


def _inference_only(who: str, names: str, x, index, centers, bias):
    """The forward products compute no gradient: refuse to record one, then hold the operands to one device."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, centers, bias)):
        raise RuntimeError(f"{who} is inference only: it computes no gradient (run it under torch.no_grad())")
    _one_device(names, x, index, centers, bias)


def _empty_y(x: torch.Tensor, lead: tuple, ncols: int, bias, dtype) -> torch.Tensor:
    """The (..., ncols) result on x's device, once the bias is known to hold a value per column."""
    if bias is not None and bias.numel() != ncols:
        raise ValueError(f"bias must hold ncols = {ncols} values, got {bias.numel()}")
    return torch.empty(lead + (ncols,), dtype=dtype, device=x.device)


def _dc_args(x: torch.Tensor, lead: tuple, kdim: int, names: str, index, g: torch.Tensor, dtype):
    """The centroid gradients' checks behind those of g: x row for row with g, one device, a float result type."""
    if x.dim() < 1 or x.shape[-1] != kdim or tuple(x.shape[:-1]) != lead:
        raise ValueError(f"x must have shape {lead + (kdim,)}, got {tuple(x.shape)}")
    _one_device(names, x, g, index)
    if dtype not in (torch.float64, torch.float32):
        raise TypeError("dtype must be torch.float64 or torch.float32")


def _plan(entry, fields: tuple, *args) -> dict:
    """Host: one nnc_*_plan entry point called with the integer ``args`` -> its int64 record as a dict keyed by ``fields``."""
    out = (ctypes.c_int64 * len(fields))()
    nat.check(entry(*(int(a) for a in args), out))
    return dict(zip(fields, (int(v) for v in out)))


_H16_DT = {torch.bfloat16: nat.DT_BF16, torch.float16: nat.DT_F16}   # the half activation types of nnc_cbmm_h16


def codebook_matmul(x: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, kdim: int, ncols: int,
                    bias: torch.Tensor | None = None, relu: bool = False, out_dtype=None) -> torch.Tensor:
    """y = x @ W + bias (then ReLU) with W[i, o] = centers[labels[i * ncols + o]] read from the indices, never decoded to float32
    (include/nnc.h, nnc_cbmm_f32).  x: float32 (..., kdim); labels: the kdim * ncols uint8 / 16-bit indices (QuantizedModel.
    labels_compact_, any storage offset); centers: float32[K]; bias: float32[ncols] or None.  Returns float32 (..., ncols).
    A bfloat16 or float16 x takes nnc_cbmm_h16: centers and bias stay float32, every centre is rounded to
    x's dtype as ``centers.to(x.dtype)`` does, the products are exact and the sums float32; the result has ``out_dtype``: None
    (x's dtype, the float32 value rounded once) or torch.float32.  A float32 x takes no ``out_dtype`` but None or torch.float32.
    Inference only: with autograd recording a tensor that needs a gradient it raises instead of returning a result without one."""
    if isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_cuda(x, "x")
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None ({x.dtype}) or torch.float32 for x of {x.dtype}, got {out_dtype}")
        y_dtype = x.dtype if out_dtype is None else out_dtype
    else:
        _require_cuda(x, "x", torch.float32)
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None or torch.float32 for a float32 x, got {out_dtype}")
        y_dtype = torch.float32
    _require_cuda(labels, "labels")
    _require_centers_bias(centers, bias)
    kdim, ncols = int(kdim), int(ncols)
    _inference_only("codebook_matmul", "x, labels, centers and bias", x, labels, centers, bias)
    lead, m = _rows(x, "x", kdim)
    if labels.numel() != kdim * ncols:
        raise ValueError(f"labels must hold kdim * ncols = {kdim * ncols} indices, got {labels.numel()}")
    y = _empty_y(x, lead, ncols, bias, y_dtype)
    L = nat.load()
    lb = _label_bytes(labels)
    if x.dtype in _H16_DT:
        ws_bytes = int(L.nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, lb))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbmm_h16(_ptr(x), _H16_DT[x.dtype], m, kdim, _ptr(labels), lb, ncols, _ptr(centers), centers.numel(), _ptr(bias),
                                 1 if relu else 0, _ptr(y), _H16_DT.get(y_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(x)))
        return y
    ws_bytes = int(L.nnc_cbmm_workspace_bytes(m, kdim, ncols, lb))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbmm_f32(_ptr(x), m, kdim, _ptr(labels), lb, ncols, _ptr(centers), centers.numel(), _ptr(bias), 1 if relu else 0,
                             _ptr(y), _ptr(ws), ws_bytes, _stream(x)))
    return y


def cbmm_plan(m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_f32 follows for this call on a device with ``cus`` compute units (include/nnc.h, nnc_cbmm_plan),
    as a dict keyed by _native.CBMM_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_plan, nat.CBMM_PLAN_FIELDS, m, kdim, ncols, label_bytes, k, cus, labels_addr)


def cbmm_h16_plan(dtype, m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_h16 follows for x of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus`` compute
    units (include/nnc.h, nnc_cbmm_h16_plan), as a dict keyed by _native.CBMM_H16_PLAN_FIELDS.  No device needed."""
    if dtype not in _H16_DT:
        raise TypeError(f"dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    return _plan(nat.load().nnc_cbmm_h16_plan, nat.CBMM_H16_PLAN_FIELDS, _H16_DT[dtype], m, kdim, ncols, label_bytes, k, cus, labels_addr)


_X_DT = {torch.float32: nat.DT_F32, **_H16_DT}   # the activation types of nnc_cbmm_grouped


def grouped_codebook_matmul(x: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, kdim: int, ncols: int, group_rows: int,
                            bias: torch.Tensor | None = None, relu: bool = False, out_dtype=None) -> torch.Tensor:
    """y = x @ W + bias (then ReLU) with one codebook per block of ``group_rows`` input rows: W[i, o] = centers[i // group_rows]
    [labels[i * ncols + o]] (include/nnc.h, nnc_cbmm_grouped).  x: float32, bfloat16 or float16 (..., kdim);
    labels: the kdim * ncols uint8 indices (any storage offset); centers: float32 (G, K), G = ceil(kdim / group_rows), K <= 256;
    group_rows: a positive multiple of 32; bias: float32[ncols] or None.  ``out_dtype`` and half x are as for codebook_matmul,
    and with one group (group_rows >= kdim) so is every bit of the result.  Inference only: it raises under autograd."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _X_DT:
        raise TypeError(f"x must be a float32, bfloat16 or float16 tensor, got {getattr(x, 'dtype', type(x))}")
    _require_cuda(x, "x")
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"out_dtype must be None ({x.dtype}) or torch.float32, got {out_dtype}")
    y_dtype = x.dtype if out_dtype is None else out_dtype
    _require_cuda(labels, "labels")
    if labels.dtype != torch.uint8:
        raise TypeError(f"grouped_codebook_matmul takes uint8 labels (K <= 256 per group), got {labels.dtype}")
    _require_centers_bias(centers, bias)
    kdim, ncols, group_rows = int(kdim), int(ncols), int(group_rows)
    _inference_only("grouped_codebook_matmul", "x, labels, centers and bias", x, labels, centers, bias)
    if group_rows < 32 or group_rows % 32:
        raise ValueError(f"group_rows must be a positive multiple of 32, got {group_rows}")
    groups = -(-kdim // group_rows)
    if centers.dim() != 2 or centers.shape[0] != max(groups, 1) or not 1 <= centers.shape[1] <= 256:
        raise ValueError(f"centers must have shape ({max(groups, 1)}, K <= 256) for kdim {kdim} and group_rows {group_rows}, got {tuple(centers.shape)}")
    lead, m = _rows(x, "x", kdim)
    if labels.numel() != kdim * ncols:
        raise ValueError(f"labels must hold kdim * ncols = {kdim * ncols} indices, got {labels.numel()}")
    y = _empty_y(x, lead, ncols, bias, y_dtype)
    L = nat.load()
    ws_bytes = int(L.nnc_cbmm_grouped_workspace_bytes(_X_DT[x.dtype], m, kdim, ncols))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbmm_grouped(_ptr(x), _X_DT[x.dtype], m, kdim, _ptr(labels), ncols, _ptr(centers), int(centers.shape[1]), group_rows, _ptr(bias),
                                 1 if relu else 0, _ptr(y), _X_DT[y_dtype], _ptr(ws), ws_bytes, _stream(x)))
    return y


def cbmm_grouped_plan(dtype, m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_grouped follows for x of ``dtype`` (torch.float32 / bfloat16 / float16) on a device with ``cus``
    compute units (include/nnc.h, nnc_cbmm_grouped_plan), as a dict keyed by _native.CBMM_GROUPED_PLAN_FIELDS.  No device needed."""
    if dtype not in _X_DT:
        raise TypeError(f"dtype must be torch.float32, torch.bfloat16 or torch.float16, got {dtype}")
    return _plan(nat.load().nnc_cbmm_grouped_plan, nat.CBMM_GROUPED_PLAN_FIELDS, _X_DT[dtype], m, kdim, ncols, k, group_rows, cus, labels_addr)


def _grad_args(g: torch.Tensor, labels: torch.Tensor, kdim: int, ncols: int, k: int):
    """The byte form's checks of g and the indices -> (lead, m) of g.  g: float32, or bfloat16 / float16."""
    _require_cuda(g, "g", g.dtype if isinstance(g, torch.Tensor) and g.dtype in _H16_DT else torch.float32)
    _require_cuda(labels, "labels")
    if labels.numel() != kdim * ncols:
        raise ValueError(f"labels must hold kdim * ncols = {kdim * ncols} indices, got {labels.numel()}")
    lead_m = _rows(g, "g", ncols)
    if not 1 <= k <= nat.NNC_KMAX:
        raise ValueError(f"k = {k} outside 1..{nat.NNC_KMAX}")
    return lead_m


def codebook_matmul_dx(g: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, kdim: int, ncols: int, out_dtype=None) -> torch.Tensor:
    """dx = g @ W^T with W[i, o] = centers[labels[i * ncols + o]] read from the indices (include/nnc.h, nnc_cbmm_dx_f32): the input
    gradient of codebook_matmul.  g: float32 (..., ncols); labels, centers as codebook_matmul.  Returns float32 (..., kdim).  Split
    partials are summed in a fixed order: the same call gives the same bits.  No host read.
    A bfloat16 or float16 g takes nnc_cbmm_dx_h16: centers stay float32 and are rounded to g's dtype as the
    forward rounds them, the products are exact, the sums float32; the result has ``out_dtype``: None (g's dtype, the float32 value
    rounded once) or torch.float32.  A float32 g takes no ``out_dtype`` but None or torch.float32."""
    kdim, ncols = int(kdim), int(ncols)
    _require_cuda(centers, "centers", torch.float32)
    lead, m = _grad_args(g, labels, kdim, ncols, centers.numel())
    _one_device("g, labels and centers", g, labels, centers)
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"out_dtype must be None or torch.float32, got {out_dtype}")
    L = nat.load()
    if g.dtype in _H16_DT:
        dx_dtype = g.dtype if out_dtype is None else out_dtype
        dx = torch.empty(lead + (kdim,), dtype=dx_dtype, device=g.device)
        lb = _label_bytes(labels)
        ws_bytes = int(L.nnc_cbmm_dx_h16_workspace_bytes(m, kdim, ncols, lb))
        ws = _workspace(ws_bytes, g.device)
        nat.check(L.nnc_cbmm_dx_h16(_ptr(g), _H16_DT[g.dtype], m, kdim, _ptr(labels), lb, ncols, _ptr(centers), centers.numel(), _ptr(dx),
                                    _H16_DT.get(dx_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(g)))
        return dx
    dx = torch.empty(lead + (kdim,), dtype=torch.float32, device=g.device)
    lb = _label_bytes(labels)
    ws_bytes = int(L.nnc_cbmm_dx_workspace_bytes(m, kdim, ncols, lb))
    ws = _workspace(ws_bytes, g.device)
    nat.check(L.nnc_cbmm_dx_f32(_ptr(g), m, kdim, _ptr(labels), lb, ncols, _ptr(centers), centers.numel(), _ptr(dx), _ptr(ws), ws_bytes, _stream(g)))
    return dx


def codebook_centroid_grad(x: torch.Tensor, g: torch.Tensor, labels: torch.Tensor, k: int, kdim: int, ncols: int,
                           dtype=torch.float64) -> torch.Tensor:
    """dc[j] = sum over the (i, o) with labels[i * ncols + o] = j of (x^T g)[i, o] (include/nnc.h, nnc_cbmm_dc_f32): the centroid
    gradient of codebook_matmul, the kdim x ncols dW never written.  x: float32 (..., kdim), g: float32 (..., ncols) with the same
    leading shape.  Exact fixed-point sums (S from max|x| and max|g| on the device, cbgrad_shift): the result depends on the shape
    and the data only.  Returns ``dtype`` (float64 or float32) [k].  No host read.
    x and g both bfloat16 or both float16 take nnc_cbmm_dc_h16: the products are exact, dW is formed in float32
    and binned by the same rule; the result is the gradient with respect to the float32 centres."""
    kdim, ncols, k = int(kdim), int(ncols), int(k)
    if isinstance(x, torch.Tensor) and isinstance(g, torch.Tensor) and x.dtype != g.dtype and (x.dtype in _H16_DT or g.dtype in _H16_DT):
        raise TypeError(f"x and g must have one dtype, got {x.dtype} and {g.dtype}")
    _require_cuda(x, "x", x.dtype if isinstance(x, torch.Tensor) and x.dtype in _H16_DT else torch.float32)
    lead, m = _grad_args(g, labels, kdim, ncols, k)
    _dc_args(x, lead, kdim, "x, g and labels", labels, g, dtype)
    L = nat.load()
    lb = _label_bytes(labels)
    if lb == 1 and k > 256:
        raise ValueError("k > 256 needs 16-bit labels")
    dc = torch.empty(k, dtype=dtype, device=x.device)
    if x.dtype in _H16_DT:
        ws_bytes = int(L.nnc_cbmm_dc_h16_workspace_bytes(m, kdim, ncols, lb, k))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbmm_dc_h16(_ptr(x), _ptr(g), _H16_DT[x.dtype], m, kdim, _ptr(labels), lb, ncols, k, _ptr(dc), 1 if dtype == torch.float64 else 0,
                                    _ptr(ws), ws_bytes, _stream(x)))
        return dc
    ws_bytes = int(L.nnc_cbmm_dc_workspace_bytes(m, kdim, ncols, lb, k))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbmm_dc_f32(_ptr(x), _ptr(g), m, kdim, _ptr(labels), lb, ncols, k, _ptr(dc), 1 if dtype == torch.float64 else 0,
                                _ptr(ws), ws_bytes, _stream(x)))
    return dc


def cbmm_dx_plan(m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_dx_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbmm_dx_plan), as a dict
    keyed by _native.CBDX_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_dx_plan, nat.CBDX_PLAN_FIELDS, m, kdim, ncols, label_bytes, k, cus, labels_addr)


def cbmm_dc_plan(m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_dc_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbmm_dc_plan), as a dict
    keyed by _native.CBDC_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_dc_plan, nat.CBDC_PLAN_FIELDS, m, kdim, ncols, label_bytes, k, cus, labels_addr)


def _h16_dt(dtype) -> int:
    if dtype not in _H16_DT:
        raise TypeError(f"dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    return _H16_DT[dtype]


def cbmm_dx_h16_plan(dtype, m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_dx_h16 follows for g of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus`` compute
    units (include/nnc_cbgrad_h16.h), as a dict keyed by _native.CBDX_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_dx_h16_plan, nat.CBDX_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, label_bytes, k, cus, labels_addr)


def cbmm_dc_h16_plan(dtype, m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_dc_h16 follows for x and g of ``dtype`` (include/nnc_cbgrad_h16.h), as a dict keyed by
    _native.CBDC_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_dc_h16_plan, nat.CBDC_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, label_bytes, k, cus, labels_addr)


CBGRAD_OK, CBGRAD_NONFINITE, CBGRAD_ZERO = 0, 1, 2


def cbgrad_shift(m: int, absmax_x: float, absmax_g: float, terms_log2: int):
    """Host mirror of the shift rule of nnc_cbmm_dc_f32 (include/nnc.h): (S, flag) with S = 62 - T - P, 2^P > m * max|x| * max|g|
    (float64, in that order), T = terms_log2.  flag CBGRAD_NONFINITE (dc is NaN) for a non-finite maximum or P > 127,
    CBGRAD_ZERO (dc = 0) for a zero one; S is 0 then."""
    ax, ag = float(np.float32(absmax_x)), float(np.float32(absmax_g))
    if not (math.isfinite(ax) and math.isfinite(ag)):
        return 0, CBGRAD_NONFINITE
    bound = float(m) * ax * ag
    if not bound > 0:
        return 0, CBGRAD_ZERO
    _, P = math.frexp(bound)
    if P > 127:
        return 0, CBGRAD_NONFINITE
    return 62 - int(terms_log2) - P, CBGRAD_OK


class _CodebookLinear(torch.autograd.Function):
    """The one autograd Function of the three trainable forms.  ``index`` is what the form keeps of the indices (the labels
    tensor, a SparseCodes, a PackedCodes); ``fwd(x, index, centers, bias, relu)``, ``dx(g, index, centers)`` and
    ``dc(x, g, index, centers)`` are the form's products on (m, kdim) / (m, ncols) rows."""

    @staticmethod
    def forward(ctx, x, index, centers, bias, relu, kdim, ncols, fwd, dx, dc):
        with torch.no_grad():
            y = fwd(x.contiguous(), index, centers, bias, relu)
        ctx.kdim, ctx.ncols, ctx.relu, ctx.dx, ctx.dc = kdim, ncols, relu, dx, dc
        held = isinstance(index, torch.Tensor)   # a labels tensor is saved with the others, a codes object kept as it is
        ctx.index = None if held else index
        ctx.save_for_backward(x, centers, y if relu else None, index if held else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, centers, y, labels = ctx.saved_tensors
        index = labels if ctx.index is None else ctx.index
        g = gy.contiguous()
        if ctx.relu:   # as torch.relu's backward: the gradient passes where y > 0 only (a NaN or negative output gets 0)
            g = torch.where(y > 0, g, torch.zeros((), dtype=g.dtype, device=g.device))
        g2 = g.reshape(-1, ctx.ncols)
        dx = dc = db = None
        if ctx.needs_input_grad[0]:
            dx = ctx.dx(g2, index, centers).view(x.shape)
        if ctx.needs_input_grad[2]:
            dc = ctx.dc(x.contiguous().reshape(-1, ctx.kdim), g2, index, centers)
        if ctx.needs_input_grad[3]:
            db = g2.sum(0, dtype=torch.float32)   # (a float32 g: the same bits; a half g: the float32 bias's gradient)
        return dx, None, dc, db, None, None, None, None, None, None


def codebook_linear(x: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, kdim: int, ncols: int, bias: torch.Tensor | None = None,
                    relu: bool = False) -> torch.Tensor:
    """codebook_matmul with gradients for x, centers and bias (an autograd Function).  The forward is the same nnc_cbmm_f32 call
    (under no_grad the bits of codebook_matmul); the backward runs codebook_matmul_dx only if x needs a gradient and
    codebook_centroid_grad (float32) only if centers does, masks a fused ReLU as torch does and sums the bias gradient over the
    rows.  The indices get no gradient.  No host read.
    A bfloat16 or float16 x: the forward is nnc_cbmm_h16 with x's dtype out, dx has x's dtype, the gradients
    of the float32 centers and bias are float32.  A half ``centers`` or ``bias`` raises ``TypeError``."""
    kdim, ncols = int(kdim), int(ncols)
    if isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_centers_bias(centers, bias)
    return _CodebookLinear.apply(
        x, labels, centers, bias, bool(relu), kdim, ncols,
        lambda x2, lab, c, b, r: codebook_matmul(x2, lab, c, kdim, ncols, bias=b, relu=r),
        lambda g2, lab, c: codebook_matmul_dx(g2, lab, c, kdim, ncols),
        lambda x2, g2, lab, c: codebook_centroid_grad(x2, g2, lab, c.numel(), kdim, ncols, dtype=torch.float32))


def _grouped_grad_args(who: str, g: torch.Tensor, labels: torch.Tensor, kdim: int, ncols: int, k: int, group_rows: int):
    """The grouped form's checks of g, the indices and the groups -> (lead, m, G) of g, G as the layers count it (>= 1).  g: float32,
    or bfloat16 / float16."""
    _require_cuda(g, "g", g.dtype if isinstance(g, torch.Tensor) and g.dtype in _H16_DT else torch.float32)
    _require_cuda(labels, "labels")
    if labels.dtype != torch.uint8:
        raise TypeError(f"{who} takes uint8 labels (K <= 256 per group), got {labels.dtype}")
    if group_rows < 32 or group_rows % 32:
        raise ValueError(f"group_rows must be a positive multiple of 32, got {group_rows}")
    if not 1 <= k <= 256:
        raise ValueError(f"k = {k} outside 1..256")
    if labels.numel() != kdim * ncols:
        raise ValueError(f"labels must hold kdim * ncols = {kdim * ncols} indices, got {labels.numel()}")
    lead, m = _rows(g, "g", ncols)
    return lead, m, max(-(-kdim // group_rows), 1)


def grouped_codebook_matmul_dx(g: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, kdim: int, ncols: int, group_rows: int,
                               out_dtype=None) -> torch.Tensor:
    """dx = g @ W^T with W[i, o] = centers[i // group_rows][labels[i * ncols + o]] (include/nnc.h, nnc_cbmm_grouped_dx_f32; DESIGN.md
    section 19): the input gradient of grouped_codebook_matmul.  g: float32 (..., ncols); labels, centers (G, K) and group_rows as
    grouped_codebook_matmul.  Returns float32 (..., kdim); the columns of a group are, bit for bit, those codebook_matmul_dx gives
    with that group's table.  No host read.
    A bfloat16 or float16 g takes nnc_cbmm_grouped_dx_h16: centers stay float32 and are rounded to g's dtype as
    the grouped forward rounds them; the result has ``out_dtype``: None (g's dtype, the float32 value rounded once) or torch.float32,
    and the same identity holds against the half codebook_matmul_dx.  As in codebook_matmul_dx, g's own dtype is asked for with None,
    not by naming it: any other ``out_dtype`` than None or torch.float32 is a ``TypeError``, for a float32 g too."""
    kdim, ncols, group_rows = int(kdim), int(ncols), int(group_rows)
    _require_cuda(centers, "centers", torch.float32)
    k = int(centers.shape[1]) if centers.dim() == 2 and 1 <= centers.shape[1] <= 256 else 0
    lead, m, groups = _grouped_grad_args("grouped_codebook_matmul_dx", g, labels, kdim, ncols, k or 1, group_rows)
    if not k or centers.shape[0] != groups:
        raise ValueError(f"centers must have shape ({groups}, K <= 256) for kdim {kdim} and group_rows {group_rows}, got {tuple(centers.shape)}")
    _one_device("g, labels and centers", g, labels, centers)
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"out_dtype must be None or torch.float32, got {out_dtype}")
    L = nat.load()
    if g.dtype in _H16_DT:
        dx_dtype = g.dtype if out_dtype is None else out_dtype
        dx = torch.empty(lead + (kdim,), dtype=dx_dtype, device=g.device)
        ws_bytes = int(L.nnc_cbmm_grouped_dx_h16_workspace_bytes(m, kdim, ncols))
        ws = _workspace(ws_bytes, g.device)
        nat.check(L.nnc_cbmm_grouped_dx_h16(_ptr(g), _H16_DT[g.dtype], m, kdim, _ptr(labels), ncols, _ptr(centers), k, group_rows, _ptr(dx),
                                            _H16_DT.get(dx_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(g)))
        return dx
    dx = torch.empty(lead + (kdim,), dtype=torch.float32, device=g.device)
    ws_bytes = int(L.nnc_cbmm_grouped_dx_workspace_bytes(m, kdim, ncols))
    ws = _workspace(ws_bytes, g.device)
    nat.check(L.nnc_cbmm_grouped_dx_f32(_ptr(g), m, kdim, _ptr(labels), ncols, _ptr(centers), k, group_rows, _ptr(dx), _ptr(ws), ws_bytes, _stream(g)))
    return dx


def grouped_codebook_centroid_grad(x: torch.Tensor, g: torch.Tensor, labels: torch.Tensor, k: int, kdim: int, ncols: int, group_rows: int,
                                   dtype=torch.float64) -> torch.Tensor:
    """dc[q, j] = sum over the (i, o) with i // group_rows = q and labels[i * ncols + o] = j of (x^T g)[i, o] (include/nnc.h,
    nnc_cbmm_grouped_dc_f32): the centroid gradient of grouped_codebook_matmul, the kdim x ncols dW never written.  x: float32
    (..., kdim), g: float32 (..., ncols) with the same leading shape.  Exact fixed-point sums with the shift of the ungrouped call
    (cbgrad_shift on the plan's terms_log2).  Returns ``dtype`` (float64 or float32) (G, k).  No host read.
    x and g both bfloat16 or both float16 take nnc_cbmm_grouped_dc_h16: dW is formed as the half
    codebook_centroid_grad forms it, and the result equals that call on the 16-bit labels q * k + label, bit for bit."""
    kdim, ncols, k, group_rows = int(kdim), int(ncols), int(k), int(group_rows)
    if isinstance(x, torch.Tensor) and isinstance(g, torch.Tensor) and x.dtype != g.dtype and (x.dtype in _H16_DT or g.dtype in _H16_DT):
        raise TypeError(f"x and g must have one dtype, got {x.dtype} and {g.dtype}")
    _require_cuda(x, "x", x.dtype if isinstance(x, torch.Tensor) and x.dtype in _H16_DT else torch.float32)
    lead, m, groups = _grouped_grad_args("grouped_codebook_centroid_grad", g, labels, kdim, ncols, k, group_rows)
    _dc_args(x, lead, kdim, "x, g and labels", labels, g, dtype)
    L = nat.load()
    dc = torch.empty((groups, k), dtype=dtype, device=x.device)
    if x.dtype in _H16_DT:
        ws_bytes = int(L.nnc_cbmm_grouped_dc_h16_workspace_bytes(m, kdim, ncols, k, group_rows))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbmm_grouped_dc_h16(_ptr(x), _ptr(g), _H16_DT[x.dtype], m, kdim, _ptr(labels), ncols, k, group_rows, _ptr(dc),
                                            1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
        return dc
    ws_bytes = int(L.nnc_cbmm_grouped_dc_workspace_bytes(m, kdim, ncols, k, group_rows))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbmm_grouped_dc_f32(_ptr(x), _ptr(g), m, kdim, _ptr(labels), ncols, k, group_rows, _ptr(dc), 1 if dtype == torch.float64 else 0,
                                        _ptr(ws), ws_bytes, _stream(x)))
    return dc


def cbmm_grouped_dx_plan(m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_grouped_dx_f32 follows on a device with ``cus`` compute units (include/nnc.h,
    nnc_cbmm_grouped_dx_plan), as a dict keyed by _native.CBDX_GROUPED_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_grouped_dx_plan, nat.CBDX_GROUPED_PLAN_FIELDS, m, kdim, ncols, k, group_rows, cus, labels_addr)


def cbmm_grouped_dc_plan(m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_grouped_dc_f32 follows on a device with ``cus`` compute units (include/nnc.h,
    nnc_cbmm_grouped_dc_plan), as a dict keyed by _native.CBDC_GROUPED_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_grouped_dc_plan, nat.CBDC_GROUPED_PLAN_FIELDS, m, kdim, ncols, k, group_rows, cus, labels_addr)


def cbmm_grouped_dx_h16_plan(dtype, m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_grouped_dx_h16 follows for g of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus``
    compute units (include/nnc_cbgrad_grouped_h16.h), as a dict keyed by _native.CBDX_GROUPED_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_grouped_dx_h16_plan, nat.CBDX_GROUPED_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, k, group_rows, cus, labels_addr)


def cbmm_grouped_dc_h16_plan(dtype, m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int, labels_addr: int = 0) -> dict:
    """Host: the plan nnc_cbmm_grouped_dc_h16 follows for x and g of ``dtype`` (include/nnc_cbgrad_grouped_h16.h), as a dict keyed by
    _native.CBDC_GROUPED_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbmm_grouped_dc_h16_plan, nat.CBDC_GROUPED_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, k, group_rows, cus, labels_addr)


def grouped_codebook_linear(x: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, kdim: int, ncols: int, group_rows: int,
                            bias: torch.Tensor | None = None, relu: bool = False, half_inputs: bool = False) -> torch.Tensor:
    """grouped_codebook_matmul with gradients for x, centers (G, K) and bias, through the autograd Function of codebook_linear.
    The forward is the same float32 nnc_cbmm_grouped call (under no_grad the bits of grouped_codebook_matmul); the backward runs
    grouped_codebook_matmul_dx only if x needs a gradient and grouped_codebook_centroid_grad (float32) only if centers does.  The
    ReLU mask and the bias gradient are codebook_linear's.  No host read.
    ``half_inputs=True`` lets a bfloat16 or float16 x through: the forward is the grouped half forward with
    x's dtype out, dx has x's dtype, the gradients of the float32 centers and bias are float32.  Without it a half x raises
    ``TypeError`` as before; a half ``centers`` or ``bias`` always does."""
    if not half_inputs:
        _require_f32_x(x, "grouped_codebook_linear")
    elif isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_centers_bias(centers, bias)
    if isinstance(labels, torch.Tensor) and labels.dtype != torch.uint8:
        raise TypeError(f"grouped_codebook_linear takes uint8 labels (K <= 256 per group), got {labels.dtype}")
    kdim, ncols, group_rows = int(kdim), int(ncols), int(group_rows)
    return _CodebookLinear.apply(
        x, labels, centers, bias, bool(relu), kdim, ncols,
        lambda x2, lab, c, b, r: grouped_codebook_matmul(x2, lab, c, kdim, ncols, group_rows, bias=b, relu=r),
        lambda g2, lab, c: grouped_codebook_matmul_dx(g2, lab, c, kdim, ncols, group_rows),
        lambda x2, g2, lab, c: grouped_codebook_centroid_grad(x2, g2, lab, c.shape[1], kdim, ncols, group_rows, dtype=torch.float32))


class SparseCodes:
    """The bitmap-sparse form of one (kdim, ncols) index matrix (include/nnc.h, nnc_cbsp_*): one 256-byte aligned uint8 device
    buffer holding the bitmap, the symbol counts and the ``nnz`` stored symbols, plus the metadata a product needs.  ``k`` is the
    codebook size the labels index; ``zero_symbol`` the skipped index."""

    def __init__(self, buf: torch.Tensor, kdim: int, ncols: int, k: int, zero_symbol: int, label_bytes: int, nnz: int):
        self.buf, self.kdim, self.ncols, self.k = buf, int(kdim), int(ncols), int(k)
        self.zero_symbol, self.label_bytes, self.nnz = int(zero_symbol), int(label_bytes), int(nnz)

    @property
    def device(self):
        return self.buf.device

    def density(self) -> float:
        n = self.kdim * self.ncols
        return self.nnz / n if n else 0.0

    def nbytes(self) -> int:
        """Resident bytes of the form (the buffer)."""
        return self.buf.numel() * self.buf.element_size()

    def to_dense(self) -> torch.Tensor:
        """The kdim * ncols labels again (uint8, or int16 storage for 2-byte labels), by nnc_cbsp_unpack."""
        L = nat.load()
        dt = torch.uint8 if self.label_bytes == 1 else torch.int16
        out = torch.empty(self.kdim * self.ncols, dtype=dt, device=self.buf.device)
        nat.check(L.nnc_cbsp_unpack(_ptr(self.buf), self.nbytes(), self.label_bytes, self.kdim, self.ncols, self.zero_symbol, self.nnz,
                                    _ptr(out), _stream(self.buf)))
        return out

    def __repr__(self):
        return (f"SparseCodes(kdim={self.kdim}, ncols={self.ncols}, k={self.k}, zero_symbol={self.zero_symbol}, "
                f"label_bytes={self.label_bytes}, nnz={self.nnz}, nbytes={self.nbytes()})")


def _aligned_bytes(nbytes: int, dev) -> torch.Tensor:
    """A uint8 device buffer of ``nbytes`` starting on a 256-byte boundary (the caching allocator gives at least 512)."""
    buf = torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    return buf[: int(nbytes)]


def pack_sparse_codes(labels: torch.Tensor, kdim: int, ncols: int, k: int, zero_symbol: int | None = None) -> SparseCodes:
    """The (kdim, ncols) labels (uint8 / 16-bit, any storage offset) -> SparseCodes on their device (nnc_cbsp_pack: bitmap,
    counts, symbols; no per-weight temporary).  ``zero_symbol``: the skipped index, by default the most frequent one (ties:
    the lowest), as storage.pack_indices chooses it.  Two passes: the first returns the count of stored symbols (one host read)."""
    _require_cuda(labels, "labels")
    kdim, ncols, k = int(kdim), int(ncols), int(k)
    lb = _label_bytes(labels)
    if labels.numel() != kdim * ncols:
        raise ValueError(f"labels must hold kdim * ncols = {kdim * ncols} indices, got {labels.numel()}")
    if not 1 <= k <= nat.NNC_KMAX or (lb == 1 and k > 256):
        raise ValueError(f"k = {k} outside 1..{256 if lb == 1 else nat.NNC_KMAX}")
    labels = labels.reshape(-1)
    if zero_symbol is None:
        zero_symbol = int(torch.argmax(bincount(labels, k)).item()) if labels.numel() else 0
    L = nat.load()
    st = _stream(labels)
    struct_bytes = int(L.nnc_cbsp_pack_bytes(kdim, ncols, lb, 0))
    if struct_bytes == 0 and kdim * ncols > 0:
        raise ValueError(f"no sparse form for a {kdim} x {ncols} matrix (ncols < 2^32, kdim * ceil(ncols / 64) <= 2^40)")
    nnz_dev = torch.zeros(1, dtype=torch.int64, device=labels.device)
    probe = _aligned_bytes(struct_bytes, labels.device)
    nat.check(L.nnc_cbsp_pack(_ptr(labels), lb, kdim, ncols, int(zero_symbol), _ptr(probe), struct_bytes, _ptr(nnz_dev), st))
    nnz = int(nnz_dev.item())
    del probe
    total = int(L.nnc_cbsp_pack_bytes(kdim, ncols, lb, nnz))
    buf = _aligned_bytes(total, labels.device)
    nat.check(L.nnc_cbsp_pack(_ptr(labels), lb, kdim, ncols, int(zero_symbol), _ptr(buf), total, None, st))
    return SparseCodes(buf, kdim, ncols, k, int(zero_symbol), lb, nnz)


def sparse_codebook_matmul(x: torch.Tensor, codes: SparseCodes, centers: torch.Tensor, bias: torch.Tensor | None = None,
                           relu: bool = False, out_dtype=None) -> torch.Tensor:
    """y = c_z * sum_i x[., i] + the stored weights' x[., i] * (centers[label] - c_z) (+ bias, then ReLU): x @ W for W[i, o] =
    centers[labels[i, o]] read from the bitmap-sparse form (include/nnc.h, nnc_cbsp_f32).  With centers[zero_symbol] == 0 the
    skipped weights are absent (an Inf in x meets no 0).  x: float32 (..., kdim); centers: float32[codes.k]; bias: float32[ncols]
    or None.  Returns float32 (..., ncols).
    A bfloat16 or float16 x takes nnc_cbsp_h16: centers and bias stay float32, every centre is rounded to x's
    dtype as ``centers.to(x.dtype)`` does, the products are exact and the sums float32; the result has ``out_dtype``: None (x's dtype,
    the float32 value rounded once) or torch.float32.  Up to 16 rows of x it is the float32 product of the widened x and the rounded
    centres bit for bit; above, it is ops.codebook_matmul on ``codes.to_dense()`` bit for bit, in which a skipped weight is an entry
    of W (an Inf in x at a skipped position gives NaN).  A float32 x takes no ``out_dtype`` but None or torch.float32.
    Inference only, as codebook_matmul."""
    if isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_cuda(x, "x")
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None ({x.dtype}) or torch.float32 for x of {x.dtype}, got {out_dtype}")
        y_dtype = x.dtype if out_dtype is None else out_dtype
    else:
        _require_cuda(x, "x", torch.float32)
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None or torch.float32 for a float32 x, got {out_dtype}")
        y_dtype = torch.float32
    _require_centers_bias(centers, bias)
    if not isinstance(codes, SparseCodes):
        raise TypeError("codes must be a SparseCodes (ops.pack_sparse_codes)")
    _inference_only("sparse_codebook_matmul", "x, codes, centers and bias", x, codes.buf, centers, bias)
    kdim, ncols = codes.kdim, codes.ncols
    lead, m = _rows(x, "x", kdim)
    if centers.numel() != codes.k:
        raise ValueError(f"centers must hold k = {codes.k} values, got {centers.numel()}")
    y = _empty_y(x, lead, ncols, bias, y_dtype)
    L = nat.load()
    if x.dtype in _H16_DT:
        ws_bytes = int(L.nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, codes.label_bytes))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbsp_h16(_ptr(x), _H16_DT[x.dtype], m, kdim, _ptr(codes.buf), codes.nbytes(), codes.label_bytes, ncols, codes.zero_symbol,
                                 codes.nnz, _ptr(centers), centers.numel(), _ptr(bias), 1 if relu else 0, _ptr(y), _H16_DT.get(y_dtype, nat.DT_F32),
                                 _ptr(ws), ws_bytes, _stream(x)))
        return y
    ws_bytes = int(L.nnc_cbsp_workspace_bytes(m, kdim, ncols, codes.label_bytes))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbsp_f32(_ptr(x), m, kdim, _ptr(codes.buf), codes.nbytes(), codes.label_bytes, ncols, codes.zero_symbol, codes.nnz,
                             _ptr(centers), centers.numel(), _ptr(bias), 1 if relu else 0, _ptr(y), _ptr(ws), ws_bytes, _stream(x)))
    return y


def cbsp_plan(m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbsp_plan), as a dict keyed
    by _native.CBSP_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_plan, nat.CBSP_PLAN_FIELDS, m, kdim, ncols, label_bytes, k, cus)


def cbsp_h16_plan(dtype, m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_h16 follows for x of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus`` compute units
    (include/nnc_cbsp_h16.h, nnc_cbsp_h16_plan), as a dict keyed by _native.CBSP_H16_PLAN_FIELDS.  No device needed."""
    if dtype not in _H16_DT:
        raise TypeError(f"dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    return _plan(nat.load().nnc_cbsp_h16_plan, nat.CBSP_H16_PLAN_FIELDS, _H16_DT[dtype], m, kdim, ncols, label_bytes, k, cus)


def sparse_codebook_matmul_dx(g: torch.Tensor, codes: SparseCodes, centers: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """dx = g @ W^T from the bitmap-sparse form (include/nnc.h, nnc_cbsp_dx_f32): c_z * sum_o g[., o] + the stored weights'
    g[., o] * (centers[label] - c_z), the input gradient of sparse_codebook_matmul with its conventions (with centers[zero_symbol]
    == 0 a skipped weight forms no product).  g: float32 (..., ncols); centers: float32[codes.k].  Returns float32 (..., kdim).
    Split partials are summed in a fixed order: the same call gives the same bits.  No host read.
    A bfloat16 or float16 g takes nnc_cbsp_dx_h16: centers stay float32 and are rounded to g's dtype as the
    forward rounds them, the products are exact, the sums float32; the result has ``out_dtype``: None (g's dtype, the float32 value
    rounded once) or torch.float32.  Up to 16 rows of g it is the float32 call on the widened g and the rounded centres bit for bit;
    above, it is ops.codebook_matmul_dx on ``codes.to_dense()`` bit for bit, in which a skipped weight is an entry of W (an Inf in g at
    a skipped position gives NaN).  A float32 g takes no ``out_dtype`` but None or torch.float32."""
    _require_cuda(centers, "centers", torch.float32)
    half = isinstance(g, torch.Tensor) and g.dtype in _H16_DT
    _require_cuda(g, "g", g.dtype if half else torch.float32)
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"out_dtype must be None or torch.float32, got {out_dtype}")
    if not isinstance(codes, SparseCodes):
        raise TypeError("codes must be a SparseCodes (ops.pack_sparse_codes)")
    lead, m = _rows(g, "g", codes.ncols)
    if centers.numel() != codes.k:
        raise ValueError(f"centers must hold k = {codes.k} values, got {centers.numel()}")
    _one_device("g, codes and centers", g, codes.buf, centers)
    L = nat.load()
    kdim, ncols, lb = codes.kdim, codes.ncols, codes.label_bytes
    if half:
        dx_dtype = g.dtype if out_dtype is None else out_dtype
        dx = torch.empty(lead + (kdim,), dtype=dx_dtype, device=g.device)
        ws_bytes = int(L.nnc_cbsp_dx_h16_workspace_bytes(m, kdim, ncols, lb))
        ws = _workspace(ws_bytes, g.device)
        nat.check(L.nnc_cbsp_dx_h16(_ptr(g), _H16_DT[g.dtype], m, kdim, _ptr(codes.buf), codes.nbytes(), lb, ncols, codes.zero_symbol, codes.nnz,
                                    _ptr(centers), centers.numel(), _ptr(dx), _H16_DT.get(dx_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(g)))
        return dx
    dx = torch.empty(lead + (kdim,), dtype=torch.float32, device=g.device)
    ws_bytes = int(L.nnc_cbsp_dx_workspace_bytes(m, kdim, ncols, lb))
    ws = _workspace(ws_bytes, g.device)
    nat.check(L.nnc_cbsp_dx_f32(_ptr(g), m, kdim, _ptr(codes.buf), codes.nbytes(), lb, ncols, codes.zero_symbol, codes.nnz, _ptr(centers),
                                centers.numel(), _ptr(dx), _ptr(ws), ws_bytes, _stream(g)))
    return dx


def sparse_codebook_centroid_grad(x: torch.Tensor, g: torch.Tensor, codes: SparseCodes, dtype=torch.float64) -> torch.Tensor:
    """dc[j] = sum over the (i, o) whose label is j of (x^T g)[i, o], the skipped positions counted under zero_symbol
    (include/nnc.h, nnc_cbsp_dc_f32): bit for bit codebook_centroid_grad(x, g, codes.to_dense(), codes.k, ...), the indices
    never unpacked and dW never written.  x: float32 (..., kdim), g: float32 (..., ncols) with the same leading shape.  Returns
    ``dtype`` (float64 or float32) [codes.k].  No host read.
    x and g both bfloat16 or both float16 take nnc_cbsp_dc_h16: again codebook_centroid_grad on
    ``codes.to_dense()`` and the same half inputs bit for bit; the result is the gradient with respect to the float32 centres."""
    if isinstance(x, torch.Tensor) and isinstance(g, torch.Tensor) and x.dtype != g.dtype and (x.dtype in _H16_DT or g.dtype in _H16_DT):
        raise TypeError(f"x and g must have one dtype, got {x.dtype} and {g.dtype}")
    half = isinstance(x, torch.Tensor) and x.dtype in _H16_DT
    _require_cuda(x, "x", x.dtype if half else torch.float32)
    _require_cuda(g, "g", x.dtype if half else torch.float32)
    if not isinstance(codes, SparseCodes):
        raise TypeError("codes must be a SparseCodes (ops.pack_sparse_codes)")
    kdim, ncols, k, lb = codes.kdim, codes.ncols, codes.k, codes.label_bytes
    lead, m = _rows(g, "g", ncols)
    _dc_args(x, lead, kdim, "x, g and codes", codes.buf, g, dtype)
    L = nat.load()
    dc = torch.empty(k, dtype=dtype, device=x.device)
    if half:
        ws_bytes = int(L.nnc_cbsp_dc_h16_workspace_bytes(m, kdim, ncols, lb, k))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbsp_dc_h16(_ptr(x), _ptr(g), _H16_DT[x.dtype], m, kdim, _ptr(codes.buf), codes.nbytes(), lb, ncols, codes.zero_symbol,
                                    codes.nnz, k, _ptr(dc), 1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
        return dc
    ws_bytes = int(L.nnc_cbsp_dc_workspace_bytes(m, kdim, ncols, lb, k))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbsp_dc_f32(_ptr(x), _ptr(g), m, kdim, _ptr(codes.buf), codes.nbytes(), lb, ncols, codes.zero_symbol, codes.nnz, k, _ptr(dc),
                                1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
    return dc


def cbsp_dx_plan(m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_dx_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbsp_dx_plan), as a dict
    keyed by _native.CBSPDX_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_dx_plan, nat.CBSPDX_PLAN_FIELDS, m, kdim, ncols, label_bytes, k, cus)


def cbsp_dc_plan(m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_dc_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbsp_dc_plan), as a dict
    keyed by _native.CBSPDC_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_dc_plan, nat.CBSPDC_PLAN_FIELDS, m, kdim, ncols, label_bytes, k, cus)


def cbsp_dx_h16_plan(dtype, m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_dx_h16 follows for g of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus`` compute
    units (include/nnc_cbspgrad_h16.h), as a dict keyed by _native.CBSPDX_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_dx_h16_plan, nat.CBSPDX_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, label_bytes, k, cus)


def cbsp_dc_h16_plan(dtype, m: int, kdim: int, ncols: int, label_bytes: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_dc_h16 follows for x and g of ``dtype`` (include/nnc_cbspgrad_h16.h), as a dict keyed by
    _native.CBSPDC_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_dc_h16_plan, nat.CBSPDC_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, label_bytes, k, cus)


def sparse_codebook_linear(x: torch.Tensor, codes: SparseCodes, centers: torch.Tensor, bias: torch.Tensor | None = None,
                           relu: bool = False) -> torch.Tensor:
    """sparse_codebook_matmul with gradients for x, centers and bias (an autograd Function shaped like codebook_linear).  The
    forward is the same nnc_cbsp_f32 call (under no_grad the bits of sparse_codebook_matmul); the backward runs
    sparse_codebook_matmul_dx only if x needs a gradient and sparse_codebook_centroid_grad (float32) only if centers does, masks a
    fused ReLU as torch does and sums the bias gradient over the rows.  The indices get no gradient.  No host read.
    A bfloat16 or float16 x: the forward is nnc_cbsp_h16 with x's dtype out, dx has x's dtype, the gradients
    of the float32 centers and bias are float32.  A half ``centers`` or ``bias`` raises ``TypeError``."""
    if not isinstance(codes, SparseCodes):
        raise TypeError("codes must be a SparseCodes (ops.pack_sparse_codes)")
    if isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_centers_bias(centers, bias)
    return _CodebookLinear.apply(x, codes, centers, bias, bool(relu), codes.kdim, codes.ncols, sparse_codebook_matmul, sparse_codebook_matmul_dx,
                                 lambda x2, g2, cd, c: sparse_codebook_centroid_grad(x2, g2, cd, dtype=torch.float32))


class GroupedSparseCodes:
    """The bitmap-sparse form of one (kdim, ncols) uint8 index matrix of a group-wise layer (include/nnc_cbsp_grouped.h; DESIGN.md
    section 28): the buffer of SparseCodes at one byte per stored symbol, with one skipped symbol per block of ``group_rows`` rows,
    ``zero_symbols`` (uint8[G] on the device).  ``k`` is the size of every group's codebook."""

    def __init__(self, buf: torch.Tensor, kdim: int, ncols: int, k: int, group_rows: int, zero_symbols: torch.Tensor, nnz: int):
        self.buf, self.kdim, self.ncols, self.k = buf, int(kdim), int(ncols), int(k)
        self.group_rows, self.zero_symbols, self.nnz = int(group_rows), zero_symbols, int(nnz)

    @property
    def device(self):
        return self.buf.device

    @property
    def groups(self) -> int:
        return -(-self.kdim // self.group_rows)

    def density(self) -> float:
        n = self.kdim * self.ncols
        return self.nnz / n if n else 0.0

    def nbytes(self) -> int:
        """Resident bytes of the form: the buffer and the G skipped symbols."""
        return self.buf.numel() + self.zero_symbols.numel()

    def to_dense(self) -> torch.Tensor:
        """The kdim * ncols uint8 labels again, by nnc_cbsp_grouped_unpack."""
        L = nat.load()
        out = torch.empty(self.kdim * self.ncols, dtype=torch.uint8, device=self.buf.device)
        nat.check(L.nnc_cbsp_grouped_unpack(_ptr(self.buf), self.buf.numel(), self.kdim, self.ncols, self.group_rows, _ptr(self.zero_symbols), self.nnz,
                                            _ptr(out), _stream(self.buf)))
        return out

    def __repr__(self):
        return (f"GroupedSparseCodes(kdim={self.kdim}, ncols={self.ncols}, k={self.k}, group_rows={self.group_rows}, groups={self.groups}, "
                f"nnz={self.nnz}, nbytes={self.nbytes()})")


def _check_group_rows(kdim: int, group_rows: int) -> int:
    if group_rows < 32 or group_rows % 32:
        raise ValueError(f"group_rows must be a positive multiple of 32, got {group_rows}")
    return -(-kdim // group_rows)


def pack_grouped_sparse_codes(labels: torch.Tensor, kdim: int, ncols: int, k: int, group_rows: int,
                              zero_symbols: torch.Tensor | None = None) -> GroupedSparseCodes:
    """The (kdim, ncols) uint8 labels of a group-wise layer (any storage offset) -> GroupedSparseCodes on their device
    (nnc_cbsp_grouped_pack: bitmap, counts, symbols; no per-weight temporary).  ``zero_symbols``: the skipped index of every group
    (uint8[G] on the device, any byte), by default the most frequent index of the group's rows (ties: the lowest), from nnc_bincount
    on each group's slice, chosen on the device.  Two passes as pack_sparse_codes: the first returns the count of stored symbols
    (the one host read)."""
    _require_cuda(labels, "labels")
    if labels.dtype != torch.uint8:
        raise TypeError(f"pack_grouped_sparse_codes takes uint8 labels (K <= 256 per group), got {labels.dtype}")
    kdim, ncols, k, group_rows = int(kdim), int(ncols), int(k), int(group_rows)
    if labels.numel() != kdim * ncols:
        raise ValueError(f"labels must hold kdim * ncols = {kdim * ncols} indices, got {labels.numel()}")
    if not 1 <= k <= 256:
        raise ValueError(f"k = {k} outside 1..256")
    groups = _check_group_rows(kdim, group_rows)
    labels = labels.reshape(-1)
    if zero_symbols is None:
        if groups and ncols:
            counts = torch.stack([bincount(labels[g * group_rows * ncols: min(kdim, (g + 1) * group_rows) * ncols], k) for g in range(groups)])
            zero_symbols = torch.argmax(counts, dim=1).to(torch.uint8)
        else:
            zero_symbols = torch.zeros(groups, dtype=torch.uint8, device=labels.device)
    else:
        _require_cuda(zero_symbols, "zero_symbols", torch.uint8)
        _one_device("labels and zero_symbols", labels, zero_symbols)
        if zero_symbols.numel() != groups:
            raise ValueError(f"zero_symbols must hold one byte per group ({groups}), got {zero_symbols.numel()}")
        zero_symbols = zero_symbols.reshape(-1)
    L = nat.load()
    st = _stream(labels)
    struct_bytes = int(L.nnc_cbsp_pack_bytes(kdim, ncols, 1, 0))
    if struct_bytes == 0 and kdim * ncols > 0:
        raise ValueError(f"no sparse form for a {kdim} x {ncols} matrix (ncols < 2^32, kdim * ceil(ncols / 64) <= 2^40)")
    nnz_dev = torch.zeros(1, dtype=torch.int64, device=labels.device)
    probe = _aligned_bytes(struct_bytes, labels.device)
    nat.check(L.nnc_cbsp_grouped_pack(_ptr(labels), kdim, ncols, group_rows, _ptr(zero_symbols), _ptr(probe), struct_bytes, _ptr(nnz_dev), st))
    nnz = int(nnz_dev.item())
    del probe
    total = int(L.nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz))
    buf = _aligned_bytes(total, labels.device)
    nat.check(L.nnc_cbsp_grouped_pack(_ptr(labels), kdim, ncols, group_rows, _ptr(zero_symbols), _ptr(buf), total, None, st))
    return GroupedSparseCodes(buf, kdim, ncols, k, group_rows, zero_symbols, nnz)


def grouped_sparse_codebook_matmul(x: torch.Tensor, codes: GroupedSparseCodes, centers: torch.Tensor, bias: torch.Tensor | None = None,
                                   relu: bool = False, out_dtype=None, half_inputs: bool = False) -> torch.Tensor:
    """y = t + the stored weights' x[., i] * (centers[g][label] - c_{z_g}) (+ bias, then ReLU), g = i // group_rows and t =
    sum_g c_{z_g} * (the sum of x over group g's rows): x @ W for W[i, o] = centers[i // group_rows][labels[i, o]] read from the
    bitmap-sparse form (include/nnc_cbsp_grouped.h, nnc_cbsp_grouped_f32).  A group with c_{z_g} == 0 adds
    nothing to t and its skipped weights are absent (an Inf in x there meets no 0).  x: float32 (..., kdim); centers: float32
    (G, codes.k); bias: float32[ncols] or None.  Returns float32 (..., ncols).
    With ``half_inputs=True`` a bfloat16 or float16 x takes nnc_cbsp_grouped_h16 (include/nnc_cbsp_grouped_h16.h; DESIGN.md section
    30): centers and bias stay float32, every centre is rounded to x's dtype as ``centers.to(x.dtype)`` does, the products are exact
    and the sums float32; the result has ``out_dtype``: None (x's dtype, the float32 value rounded once) or torch.float32.  Up to 16
    rows of x it is the float32 product of the widened x and the rounded centres bit for bit; above, it is
    ops.grouped_codebook_matmul on ``codes.to_dense()`` bit for bit, in which a skipped weight is an entry of W (an Inf in x at a
    skipped position gives NaN).  Without the keyword a bfloat16 or float16 x raises ``TypeError``, as it always did; a float32 x
    takes the same call with or without it, and no ``out_dtype`` but None or torch.float32.
    Inference only, as sparse_codebook_matmul: it raises under autograd."""
    half = isinstance(x, torch.Tensor) and x.dtype in _H16_DT
    if half and not half_inputs:
        raise TypeError(f"grouped_sparse_codebook_matmul takes float32 activations, got {x.dtype}: pass half_inputs=True to run bfloat16 and "
                        "float16 inputs from the bitmap-sparse form (or use the byte and packed forms, ops.grouped_codebook_matmul, "
                        "ops.grouped_packed_codebook_matmul)")
    if half:
        _require_cuda(x, "x")
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None ({x.dtype}) or torch.float32 for x of {x.dtype}, got {out_dtype}")
        y_dtype = x.dtype if out_dtype is None else out_dtype
    else:
        _require_cuda(x, "x", torch.float32)
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None or torch.float32 for a float32 x, got {out_dtype}")
        y_dtype = torch.float32
    _require_centers_bias(centers, bias)
    if not isinstance(codes, GroupedSparseCodes):
        raise TypeError("codes must be a GroupedSparseCodes (ops.pack_grouped_sparse_codes)")
    _inference_only("grouped_sparse_codebook_matmul", "x, codes, centers and bias", x, codes.buf, centers, bias)
    kdim, ncols = codes.kdim, codes.ncols
    lead, m = _rows(x, "x", kdim)
    if centers.dim() != 2 or tuple(centers.shape) != (max(codes.groups, 1), codes.k):
        raise ValueError(f"centers must have shape ({max(codes.groups, 1)}, {codes.k}), got {tuple(centers.shape)}")
    y = _empty_y(x, lead, ncols, bias, y_dtype)
    L = nat.load()
    if half:
        ws_bytes = int(L.nnc_cbsp_grouped_h16_workspace_bytes(_H16_DT[x.dtype], m, kdim, ncols))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbsp_grouped_h16(_ptr(x), _H16_DT[x.dtype], m, kdim, _ptr(codes.buf), codes.buf.numel(), ncols, _ptr(codes.zero_symbols),
                                         codes.nnz, _ptr(centers), codes.k, codes.group_rows, _ptr(bias), 1 if relu else 0, _ptr(y),
                                         _H16_DT.get(y_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(x)))
        return y
    ws_bytes = int(L.nnc_cbsp_grouped_workspace_bytes(m, kdim, ncols))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbsp_grouped_f32(_ptr(x), m, kdim, _ptr(codes.buf), codes.buf.numel(), ncols, _ptr(codes.zero_symbols), codes.nnz, _ptr(centers),
                                     codes.k, codes.group_rows, _ptr(bias), 1 if relu else 0, _ptr(y), _ptr(ws), ws_bytes, _stream(x)))
    return y


def cbsp_grouped_plan(m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_grouped_f32 follows on a device with ``cus`` compute units (include/nnc_cbsp_grouped.h,
    nnc_cbsp_grouped_plan), as a dict keyed by _native.CBSP_GROUPED_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_grouped_plan, nat.CBSP_GROUPED_PLAN_FIELDS, m, kdim, ncols, k, group_rows, cus)


def cbsp_grouped_h16_plan(dtype, m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_grouped_h16 follows for x of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus`` compute
    units (include/nnc_cbsp_grouped_h16.h, nnc_cbsp_grouped_h16_plan), as a dict keyed by _native.CBSP_GROUPED_H16_PLAN_FIELDS.  No
    device needed."""
    return _plan(nat.load().nnc_cbsp_grouped_h16_plan, nat.CBSP_GROUPED_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, k, group_rows, cus)


def _grouped_sparse_grad_args(who: str, g, codes, centers=None):
    """The checks of the grouped sparse backward ops: float32 g of (..., ncols) rows, a GroupedSparseCodes, and (dx) float32 centers
    (G, codes.k) -> (lead, m) of g."""
    if isinstance(g, torch.Tensor) and g.dtype in _H16_DT:
        raise TypeError(f"{who} takes float32 activations, got {g.dtype}: the backward pass from the grouped bitmap-sparse form has no bfloat16 / "
                        "float16 path (use the byte or packed forms, ops.grouped_codebook_linear(half_inputs=True))")
    _require_cuda(g, "g", torch.float32)
    if not isinstance(codes, GroupedSparseCodes):
        raise TypeError("codes must be a GroupedSparseCodes (ops.pack_grouped_sparse_codes)")
    _check_group_rows(codes.kdim, codes.group_rows)
    if centers is not None:
        _require_cuda(centers, "centers", torch.float32)
        if centers.dim() != 2 or tuple(centers.shape) != (max(codes.groups, 1), codes.k):
            raise ValueError(f"centers must have shape ({max(codes.groups, 1)}, {codes.k}), got {tuple(centers.shape)}")
    return _rows(g, "g", codes.ncols)


def grouped_sparse_codebook_matmul_dx(g: torch.Tensor, codes: GroupedSparseCodes, centers: torch.Tensor) -> torch.Tensor:
    """dx = g @ W^T from the bitmap-sparse form of a group-wise layer (include/nnc_cbspgrad_grouped.h, nnc_cbsp_grouped_dx_f32;
    DESIGN.md section 32): with q = i // group_rows, dx[., i] = c_{z_q} * sum_o g[., o] + the stored weights' g[., o] *
    (centers[q][label] - c_{z_q}), the input gradient of grouped_sparse_codebook_matmul with its conventions (a group with c_{z_q} == 0
    drops the rank-1 term, and its skipped weights form no product).  g: float32 (..., ncols); centers: float32 (G, codes.k).
    Returns float32 (..., kdim).  The columns of group q are, bit for bit, those sparse_codebook_matmul_dx gives on the same buffer
    read as ``SparseCodes(codes.buf, kdim, ncols, k, z_q, 1, codes.nnz)`` with the one table ``centers[q]``.  No host read."""
    lead, m = _grouped_sparse_grad_args("grouped_sparse_codebook_matmul_dx", g, codes, centers)
    _one_device("g, codes and centers", g, codes.buf, codes.zero_symbols, centers)
    L = nat.load()
    kdim, ncols = codes.kdim, codes.ncols
    dx = torch.empty(lead + (kdim,), dtype=torch.float32, device=g.device)
    ws_bytes = int(L.nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols))
    ws = _workspace(ws_bytes, g.device)
    nat.check(L.nnc_cbsp_grouped_dx_f32(_ptr(g), m, kdim, _ptr(codes.buf), codes.buf.numel(), ncols, _ptr(codes.zero_symbols), codes.nnz, _ptr(centers),
                                        codes.k, codes.group_rows, _ptr(dx), _ptr(ws), ws_bytes, _stream(g)))
    return dx


def grouped_sparse_codebook_centroid_grad(x: torch.Tensor, g: torch.Tensor, codes: GroupedSparseCodes, dtype=torch.float64) -> torch.Tensor:
    """dc[q, j] = sum over the (i, o) of group q whose label is j of (x^T g)[i, o], the skipped positions counted under the group's
    zero symbol (include/nnc_cbspgrad_grouped.h, nnc_cbsp_grouped_dc_f32): bit for bit grouped_codebook_centroid_grad(x, g,
    codes.to_dense(), ...), the indices never unpacked and dW never written.  x: float32 (..., kdim), g: float32 (..., ncols) with the
    same leading shape.  Returns ``dtype`` (float64 or float32) (G, codes.k).  No host read."""
    if isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        raise TypeError(f"grouped_sparse_codebook_centroid_grad takes float32 activations, got {x.dtype}: the backward pass from the grouped "
                        "bitmap-sparse form has no bfloat16 / float16 path")
    lead, m = _grouped_sparse_grad_args("grouped_sparse_codebook_centroid_grad", g, codes)
    _require_cuda(x, "x", torch.float32)
    kdim, ncols, k = codes.kdim, codes.ncols, codes.k
    _dc_args(x, lead, kdim, "x, g and codes", codes.buf, g, dtype)
    L = nat.load()
    dc = torch.empty((max(codes.groups, 1), k), dtype=dtype, device=x.device)
    ws_bytes = int(L.nnc_cbsp_grouped_dc_workspace_bytes(m, kdim, ncols, k, codes.group_rows))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbsp_grouped_dc_f32(_ptr(x), _ptr(g), m, kdim, _ptr(codes.buf), codes.buf.numel(), ncols, _ptr(codes.zero_symbols), codes.nnz, k,
                                        codes.group_rows, _ptr(dc), 1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
    return dc


def cbsp_grouped_dx_plan(m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_grouped_dx_f32 follows on a device with ``cus`` compute units (include/nnc_cbspgrad_grouped.h,
    nnc_cbsp_grouped_dx_plan), as a dict keyed by _native.CBSPDX_GROUPED_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_grouped_dx_plan, nat.CBSPDX_GROUPED_PLAN_FIELDS, m, kdim, ncols, k, group_rows, cus)


def cbsp_grouped_dc_plan(m: int, kdim: int, ncols: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbsp_grouped_dc_f32 follows on a device with ``cus`` compute units (include/nnc_cbspgrad_grouped.h,
    nnc_cbsp_grouped_dc_plan), as a dict keyed by _native.CBSPDC_GROUPED_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbsp_grouped_dc_plan, nat.CBSPDC_GROUPED_PLAN_FIELDS, m, kdim, ncols, k, group_rows, cus)


def grouped_sparse_codebook_linear(x: torch.Tensor, codes: GroupedSparseCodes, centers: torch.Tensor, bias: torch.Tensor | None = None,
                                   relu: bool = False) -> torch.Tensor:
    """grouped_sparse_codebook_matmul with gradients for x, centers (G, K) and bias, through the autograd Function of codebook_linear
    (DESIGN.md section 32).  The forward is the same float32 nnc_cbsp_grouped_f32 call (under no_grad the bits of
    grouped_sparse_codebook_matmul); the backward runs grouped_sparse_codebook_matmul_dx only if x needs a gradient and
    grouped_sparse_codebook_centroid_grad (float32) only if centers does, masks a fused ReLU as torch does and sums the bias gradient
    over the rows.  The indices get no gradient.  No host read.  float32 activations only: a bfloat16 or float16 x raises
    ``TypeError``."""
    if not isinstance(codes, GroupedSparseCodes):
        raise TypeError("codes must be a GroupedSparseCodes (ops.pack_grouped_sparse_codes)")
    _require_f32_x(x, "grouped_sparse_codebook_linear")
    return _CodebookLinear.apply(x, codes, centers, bias, bool(relu), codes.kdim, codes.ncols, grouped_sparse_codebook_matmul,
                                 grouped_sparse_codebook_matmul_dx,
                                 lambda x2, g2, cd, c: grouped_sparse_codebook_centroid_grad(x2, g2, cd, dtype=torch.float32))


class PackedCodes:
    """The 2- or 4-bit packed form of one (kdim, ncols) index matrix of a codebook of ``k`` <= 2^bits centres (include/nnc.h,
    nnc_cbpk_*): ``packed``, one 256-byte aligned uint8 device buffer of kdim rows of nnc_cbpk_row_bytes(ncols, bits) bytes, and
    the metadata a product needs."""

    def __init__(self, packed: torch.Tensor, kdim: int, ncols: int, bits: int, k: int):
        self.packed, self.kdim, self.ncols, self.bits, self.k = packed, int(kdim), int(ncols), int(bits), int(k)

    @property
    def device(self):
        return self.packed.device

    @property
    def nbytes(self) -> int:
        """Resident bytes of the form (the buffer)."""
        return self.packed.numel()

    def to_dense(self) -> torch.Tensor:
        """The kdim * ncols labels again (uint8), by nnc_cbpk_unpack."""
        L = nat.load()
        out = torch.empty(self.kdim * self.ncols, dtype=torch.uint8, device=self.packed.device)
        nat.check(L.nnc_cbpk_unpack(_ptr(self.packed), self.nbytes, self.bits, self.kdim, self.ncols, _ptr(out), 1, _stream(self.packed)))
        return out

    def __repr__(self):
        return f"PackedCodes(kdim={self.kdim}, ncols={self.ncols}, bits={self.bits}, k={self.k}, nbytes={self.nbytes})"


def packed_bits(k: int, bits: int | None = None) -> int:
    """The width the packed form takes for a codebook of ``k`` centres: the smaller of 2 and 4 that holds k, or ``bits`` once
    checked.  ValueError for k > 16, a width other than 2 or 4, or k > 2^bits."""
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k} is not a codebook size")
    if k > 16:
        raise ValueError(f"k = {k} centres do not fit 4-bit indices (the packed form holds at most 16; use the byte form)")
    if bits is None:
        return 2 if k <= 4 else 4
    bits = int(bits)
    if bits not in (2, 4):
        raise ValueError(f"bits must be 2 or 4, got {bits}")
    if k > 1 << bits:
        raise ValueError(f"k = {k} centres do not fit {bits}-bit indices")
    return bits


def packed_nbytes(kdim: int, ncols: int, bits: int) -> int:
    """Host: the bytes of the packed form of a (kdim, ncols) index matrix (nnc_cbpk_pack_bytes)."""
    return int(nat.load().nnc_cbpk_pack_bytes(int(kdim), int(ncols), int(bits)))


def pack_codes(labels: torch.Tensor, kdim: int, ncols: int, k: int, bits: int | None = None) -> PackedCodes:
    """The (kdim, ncols) labels (uint8 / 16-bit, any storage offset) of a codebook of ``k`` <= 16 centres -> PackedCodes on their
    device (nnc_cbpk_pack: one pass, no per-weight temporary).  ``bits``: 2 or 4, by default the smaller that holds k.
    ValueError (before any launch) for k > 16 or k > 2^bits, and for a label >= 2^bits (one host read of the pack's count)."""
    kdim, ncols, k = int(kdim), int(ncols), int(k)
    bits = packed_bits(k, bits)
    _require_cuda(labels, "labels")
    lb = _label_bytes(labels)
    if labels.numel() != kdim * ncols:
        raise ValueError(f"labels must hold kdim * ncols = {kdim * ncols} indices, got {labels.numel()}")
    labels = labels.reshape(-1)
    L = nat.load()
    total = int(L.nnc_cbpk_pack_bytes(kdim, ncols, bits))
    if total == 0 and kdim * ncols > 0:
        raise ValueError(f"no packed form for a {kdim} x {ncols} matrix")
    buf = _aligned_bytes(total, labels.device)
    bad = torch.empty(1, dtype=torch.int32, device=labels.device)
    nat.check(L.nnc_cbpk_pack(_ptr(labels), lb, kdim, ncols, bits, _ptr(buf), total, _ptr(bad), _stream(labels)))
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"{nbad} labels are >= 2^{bits}: they do not fit the packed form")
    return PackedCodes(buf, kdim, ncols, bits, k)


def packed_codebook_matmul(x: torch.Tensor, codes: PackedCodes, centers: torch.Tensor, bias: torch.Tensor | None = None,
                           relu: bool = False, out_dtype=None) -> torch.Tensor:
    """y = x @ W + bias (then ReLU) with W[i, o] = centers[label (i, o)] read from the 2- or 4-bit packed indices (include/nnc.h,
    nnc_cbpk_f32): codebook_matmul on the unpacked labels, from a half or a quarter of the index bytes.  x: float32 (..., kdim);
    centers: float32[codes.k]; bias: float32[ncols] or None.  Returns float32 (..., ncols).
    A bfloat16 or float16 x takes nnc_cbpk_h16: centers and bias stay float32, every centre is rounded to x's
    dtype as ``centers.to(x.dtype)`` does, the products are exact and the sums float32; the result has ``out_dtype``: None (x's dtype,
    the float32 value rounded once) or torch.float32.  It is grouped_packed_codebook_matmul with one group bit for bit; above 16 rows
    of x also ops.codebook_matmul on ``codes.to_dense()``, up to 16 rows with float32 output the float32 product of the widened x and
    the rounded centres.  A float32 x takes no ``out_dtype`` but None or torch.float32.
    Inference only, as codebook_matmul."""
    if isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_cuda(x, "x")
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None ({x.dtype}) or torch.float32 for x of {x.dtype}, got {out_dtype}")
        y_dtype = x.dtype if out_dtype is None else out_dtype
    else:
        _require_cuda(x, "x", torch.float32)
        if out_dtype not in (None, torch.float32):
            raise TypeError(f"out_dtype must be None or torch.float32 for a float32 x, got {out_dtype}")
        y_dtype = torch.float32
    _require_centers_bias(centers, bias)
    if not isinstance(codes, PackedCodes):
        raise TypeError("codes must be a PackedCodes (ops.pack_codes)")
    _inference_only("packed_codebook_matmul", "x, codes, centers and bias", x, codes.packed, centers, bias)
    kdim, ncols = codes.kdim, codes.ncols
    lead, m = _rows(x, "x", kdim)
    if centers.numel() != codes.k:
        raise ValueError(f"centers must hold k = {codes.k} values, got {centers.numel()}")
    y = _empty_y(x, lead, ncols, bias, y_dtype)
    L = nat.load()
    if x.dtype in _H16_DT:
        ws_bytes = int(L.nnc_cbpk_h16_workspace_bytes(m, kdim, ncols, codes.bits))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbpk_h16(_ptr(x), _H16_DT[x.dtype], m, kdim, _ptr(codes.packed), codes.nbytes, codes.bits, ncols, _ptr(centers), centers.numel(),
                                 _ptr(bias), 1 if relu else 0, _ptr(y), _H16_DT.get(y_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(x)))
        return y
    ws_bytes = int(L.nnc_cbpk_workspace_bytes(m, kdim, ncols, codes.bits))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbpk_f32(_ptr(x), m, kdim, _ptr(codes.packed), codes.nbytes, codes.bits, ncols, _ptr(centers), centers.numel(), _ptr(bias),
                             1 if relu else 0, _ptr(y), _ptr(ws), ws_bytes, _stream(x)))
    return y


def cbpk_plan(m: int, kdim: int, ncols: int, bits: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbpk_plan), as a dict keyed
    by _native.CBPK_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_plan, nat.CBPK_PLAN_FIELDS, m, kdim, ncols, bits, k, cus)


def cbpk_h16_plan(dtype, m: int, kdim: int, ncols: int, bits: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_h16 follows for x of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus`` compute units
    (include/nnc_cbpk_h16.h, nnc_cbpk_h16_plan), as a dict keyed by _native.CBPK_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_h16_plan, nat.CBPK_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, bits, k, cus)


def grouped_packed_codebook_matmul(x: torch.Tensor, codes: PackedCodes, centers: torch.Tensor, group_rows: int, bias: torch.Tensor | None = None,
                                   relu: bool = False, out_dtype=None) -> torch.Tensor:
    """y = x @ W + bias (then ReLU) with one codebook per block of ``group_rows`` input rows, W[i, o] = centers[i // group_rows]
    [label (i, o)] read from the 2- or 4-bit packed indices (include/nnc.h, nnc_cbpk_grouped):
    grouped_codebook_matmul on the unpacked labels, bit for bit, from a half or a quarter of the index bytes.  x: float32, bfloat16
    or float16 (..., kdim); codes: the PackedCodes of the whole (kdim, ncols) index matrix (ops.pack_codes); centers: float32
    (G, K), G = ceil(kdim / group_rows), K = codes.k <= 2^bits; group_rows: a positive multiple of 32; bias: float32[ncols] or None.
    ``out_dtype`` and half x are as for grouped_codebook_matmul.  Inference only: it raises under autograd."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _X_DT:
        raise TypeError(f"x must be a float32, bfloat16 or float16 tensor, got {getattr(x, 'dtype', type(x))}")
    _require_cuda(x, "x")
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"out_dtype must be None ({x.dtype}) or torch.float32, got {out_dtype}")
    y_dtype = x.dtype if out_dtype is None else out_dtype
    if not isinstance(codes, PackedCodes):
        raise TypeError("codes must be a PackedCodes (ops.pack_codes)")
    _require_centers_bias(centers, bias)
    group_rows = int(group_rows)
    _inference_only("grouped_packed_codebook_matmul", "x, codes, centers and bias", x, codes.packed, centers, bias)
    if group_rows < 32 or group_rows % 32:
        raise ValueError(f"group_rows must be a positive multiple of 32, got {group_rows}")
    kdim, ncols = codes.kdim, codes.ncols
    groups = max(-(-kdim // group_rows), 1)
    if centers.dim() != 2 or tuple(centers.shape) != (groups, codes.k):
        raise ValueError(f"centers must have shape ({groups}, {codes.k}) for kdim {kdim}, group_rows {group_rows} and codes of k = {codes.k}, "
                         f"got {tuple(centers.shape)}")
    lead, m = _rows(x, "x", kdim)
    y = _empty_y(x, lead, ncols, bias, y_dtype)
    L = nat.load()
    ws_bytes = int(L.nnc_cbpk_grouped_workspace_bytes(_X_DT[x.dtype], m, kdim, ncols, codes.bits))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbpk_grouped(_ptr(x), _X_DT[x.dtype], m, kdim, _ptr(codes.packed), codes.nbytes, codes.bits, ncols, _ptr(centers), codes.k, group_rows,
                                 _ptr(bias), 1 if relu else 0, _ptr(y), _X_DT[y_dtype], _ptr(ws), ws_bytes, _stream(x)))
    return y


def cbpk_grouped_plan(dtype, m: int, kdim: int, ncols: int, bits: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_grouped follows for x of ``dtype`` (torch.float32 / bfloat16 / float16) on a device with ``cus``
    compute units (include/nnc.h, nnc_cbpk_grouped_plan), as a dict keyed by _native.CBPK_GROUPED_PLAN_FIELDS.  No device needed."""
    if dtype not in _X_DT:
        raise TypeError(f"dtype must be torch.float32, torch.bfloat16 or torch.float16, got {dtype}")
    return _plan(nat.load().nnc_cbpk_grouped_plan, nat.CBPK_GROUPED_PLAN_FIELDS, _X_DT[dtype], m, kdim, ncols, bits, k, group_rows, cus)


def packed_codebook_matmul_dx(g: torch.Tensor, codes: PackedCodes, centers: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """dx = g @ W^T with W[i, o] = centers[label (i, o)] read from the 2- or 4-bit packed indices (include/nnc.h,
    nnc_cbpk_dx_f32): the input gradient of packed_codebook_matmul with the conventions of codebook_matmul_dx (a label >= k reads 0;
    the padding of a row forms no product).  g: float32 (..., ncols); centers: float32[codes.k].  Returns float32 (..., kdim).
    Split partials are summed in a fixed order: the same call gives the same bits.  No host read.
    A bfloat16 or float16 g takes nnc_cbpk_dx_h16: centers stay float32 and are rounded to g's dtype as the
    forward rounds them, the products are exact, the sums float32; the result has ``out_dtype``: None (g's dtype, the float32 value
    rounded once) or torch.float32.  Up to 16 rows of g it is the float32 call on the widened g and the rounded centres bit for bit;
    above, it is ops.codebook_matmul_dx on ``codes.to_dense()`` bit for bit.  A float32 g takes no ``out_dtype`` but None or
    torch.float32."""
    _require_cuda(centers, "centers", torch.float32)
    half = isinstance(g, torch.Tensor) and g.dtype in _H16_DT
    _require_cuda(g, "g", g.dtype if half else torch.float32)
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"out_dtype must be None or torch.float32, got {out_dtype}")
    if not isinstance(codes, PackedCodes):
        raise TypeError("codes must be a PackedCodes (ops.pack_codes)")
    lead, m = _rows(g, "g", codes.ncols)
    if centers.numel() != codes.k:
        raise ValueError(f"centers must hold k = {codes.k} values, got {centers.numel()}")
    _one_device("g, codes and centers", g, codes.packed, centers)
    L = nat.load()
    kdim, ncols, bits = codes.kdim, codes.ncols, codes.bits
    if half:
        dx_dtype = g.dtype if out_dtype is None else out_dtype
        dx = torch.empty(lead + (kdim,), dtype=dx_dtype, device=g.device)
        ws_bytes = int(L.nnc_cbpk_dx_h16_workspace_bytes(m, kdim, ncols, bits))
        ws = _workspace(ws_bytes, g.device)
        nat.check(L.nnc_cbpk_dx_h16(_ptr(g), _H16_DT[g.dtype], m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, _ptr(centers), centers.numel(),
                                    _ptr(dx), _H16_DT.get(dx_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(g)))
        return dx
    dx = torch.empty(lead + (kdim,), dtype=torch.float32, device=g.device)
    ws_bytes = int(L.nnc_cbpk_dx_workspace_bytes(m, kdim, ncols, bits))
    ws = _workspace(ws_bytes, g.device)
    nat.check(L.nnc_cbpk_dx_f32(_ptr(g), m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, _ptr(centers), centers.numel(), _ptr(dx),
                                _ptr(ws), ws_bytes, _stream(g)))
    return dx


def packed_codebook_centroid_grad(x: torch.Tensor, g: torch.Tensor, codes: PackedCodes, dtype=torch.float64) -> torch.Tensor:
    """dc[j] = sum over the (i, o) whose label is j of (x^T g)[i, o] (include/nnc.h, nnc_cbpk_dc_f32): bit for bit
    codebook_centroid_grad(x, g, codes.to_dense(), codes.k, ...), the indices never unpacked and dW never written.  x: float32
    (..., kdim), g: float32 (..., ncols) with the same leading shape.  Returns ``dtype`` (float64 or float32) [codes.k].  No host
    read.
    x and g both bfloat16 or both float16 take nnc_cbpk_dc_h16: again codebook_centroid_grad on
    ``codes.to_dense()`` and the same half inputs bit for bit; the result is the gradient with respect to the float32 centres."""
    if isinstance(x, torch.Tensor) and isinstance(g, torch.Tensor) and x.dtype != g.dtype and (x.dtype in _H16_DT or g.dtype in _H16_DT):
        raise TypeError(f"x and g must have one dtype, got {x.dtype} and {g.dtype}")
    half = isinstance(x, torch.Tensor) and x.dtype in _H16_DT
    _require_cuda(x, "x", x.dtype if half else torch.float32)
    _require_cuda(g, "g", x.dtype if half else torch.float32)
    if not isinstance(codes, PackedCodes):
        raise TypeError("codes must be a PackedCodes (ops.pack_codes)")
    kdim, ncols, k, bits = codes.kdim, codes.ncols, codes.k, codes.bits
    lead, m = _rows(g, "g", ncols)
    _dc_args(x, lead, kdim, "x, g and codes", codes.packed, g, dtype)
    L = nat.load()
    dc = torch.empty(k, dtype=dtype, device=x.device)
    if half:
        ws_bytes = int(L.nnc_cbpk_dc_h16_workspace_bytes(m, kdim, ncols, bits, k))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbpk_dc_h16(_ptr(x), _ptr(g), _H16_DT[x.dtype], m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, k, _ptr(dc),
                                    1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
        return dc
    ws_bytes = int(L.nnc_cbpk_dc_workspace_bytes(m, kdim, ncols, bits, k))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbpk_dc_f32(_ptr(x), _ptr(g), m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, k, _ptr(dc),
                                1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
    return dc


def cbpk_dx_plan(m: int, kdim: int, ncols: int, bits: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_dx_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbpk_dx_plan), as a dict
    keyed by _native.CBPKDX_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_dx_plan, nat.CBPKDX_PLAN_FIELDS, m, kdim, ncols, bits, k, cus)


def cbpk_dc_plan(m: int, kdim: int, ncols: int, bits: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_dc_f32 follows on a device with ``cus`` compute units (include/nnc.h, nnc_cbpk_dc_plan), as a dict
    keyed by _native.CBPKDC_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_dc_plan, nat.CBPKDC_PLAN_FIELDS, m, kdim, ncols, bits, k, cus)


def cbpk_dx_h16_plan(dtype, m: int, kdim: int, ncols: int, bits: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_dx_h16 follows for g of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus`` compute
    units (include/nnc_cbpk_h16.h), as a dict keyed by _native.CBPKDX_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_dx_h16_plan, nat.CBPKDX_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, bits, k, cus)


def cbpk_dc_h16_plan(dtype, m: int, kdim: int, ncols: int, bits: int, k: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_dc_h16 follows for x and g of ``dtype`` (include/nnc_cbpk_h16.h), as a dict keyed by
    _native.CBPKDC_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_dc_h16_plan, nat.CBPKDC_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, bits, k, cus)


def packed_codebook_linear(x: torch.Tensor, codes: PackedCodes, centers: torch.Tensor, bias: torch.Tensor | None = None,
                           relu: bool = False) -> torch.Tensor:
    """packed_codebook_matmul with gradients for x, centers and bias (an autograd Function shaped like codebook_linear).  The
    forward is the same nnc_cbpk_f32 call (under no_grad the bits of packed_codebook_matmul); the backward runs
    packed_codebook_matmul_dx only if x needs a gradient and packed_codebook_centroid_grad (float32) only if centers does, masks a
    fused ReLU as torch does and sums the bias gradient over the rows.  The indices get no gradient.  No host read.
    A bfloat16 or float16 x: the forward is nnc_cbpk_h16 with x's dtype out, dx has x's dtype, the gradients
    of the float32 centers and bias are float32.  A half ``centers`` or ``bias`` raises ``TypeError``."""
    if not isinstance(codes, PackedCodes):
        raise TypeError("codes must be a PackedCodes (ops.pack_codes)")
    if isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_centers_bias(centers, bias)
    return _CodebookLinear.apply(x, codes, centers, bias, bool(relu), codes.kdim, codes.ncols, packed_codebook_matmul, packed_codebook_matmul_dx,
                                 lambda x2, g2, cd, c: packed_codebook_centroid_grad(x2, g2, cd, dtype=torch.float32))


def _grouped_packed_args(codes, centers: torch.Tensor, group_rows: int) -> int:
    """The grouped packed form's checks of the codes, the (G, K) centres and group_rows -> G, as the layers count it (>= 1)."""
    if not isinstance(codes, PackedCodes):
        raise TypeError("codes must be a PackedCodes (ops.pack_codes)")
    if group_rows < 32 or group_rows % 32:
        raise ValueError(f"group_rows must be a positive multiple of 32, got {group_rows}")
    groups = max(-(-codes.kdim // group_rows), 1)
    if centers is not None and (centers.dim() != 2 or tuple(centers.shape) != (groups, codes.k)):
        raise ValueError(f"centers must have shape ({groups}, {codes.k}) for kdim {codes.kdim}, group_rows {group_rows} and codes of k = {codes.k}, "
                         f"got {tuple(centers.shape)}")
    return groups


def grouped_packed_codebook_matmul_dx(g: torch.Tensor, codes: PackedCodes, centers: torch.Tensor, group_rows: int, out_dtype=None) -> torch.Tensor:
    """dx = g @ W^T with W[i, o] = centers[i // group_rows][label (i, o)] read from the 2- or 4-bit packed indices
    (include/nnc_cbpkgrad_grouped.h, nnc_cbpk_grouped_dx_f32): the input gradient of
    grouped_packed_codebook_matmul.  g: float32 (..., ncols); codes, centers (G, K) and group_rows as grouped_packed_codebook_matmul.
    Returns float32 (..., kdim); the columns of a group are, bit for bit, those packed_codebook_matmul_dx gives with that group's
    table.  No host read.
    A bfloat16 or float16 g takes nnc_cbpk_grouped_dx_h16: bit for bit the half grouped_codebook_matmul_dx on
    codes.to_dense(); ``out_dtype`` as there: None (g's dtype) or torch.float32, anything else a ``TypeError``, for a float32 g too."""
    group_rows = int(group_rows)
    _require_cuda(centers, "centers", torch.float32)
    _require_cuda(g, "g", g.dtype if isinstance(g, torch.Tensor) and g.dtype in _H16_DT else torch.float32)
    _grouped_packed_args(codes, centers, group_rows)
    lead, m = _rows(g, "g", codes.ncols)
    _one_device("g, codes and centers", g, codes.packed, centers)
    if out_dtype not in (None, torch.float32):
        raise TypeError(f"out_dtype must be None or torch.float32, got {out_dtype}")
    L = nat.load()
    kdim, ncols, bits = codes.kdim, codes.ncols, codes.bits
    if g.dtype in _H16_DT:
        dx_dtype = g.dtype if out_dtype is None else out_dtype
        dx = torch.empty(lead + (kdim,), dtype=dx_dtype, device=g.device)
        ws_bytes = int(L.nnc_cbpk_grouped_dx_h16_workspace_bytes(m, kdim, ncols, bits))
        ws = _workspace(ws_bytes, g.device)
        nat.check(L.nnc_cbpk_grouped_dx_h16(_ptr(g), _H16_DT[g.dtype], m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, _ptr(centers), codes.k,
                                            group_rows, _ptr(dx), _H16_DT.get(dx_dtype, nat.DT_F32), _ptr(ws), ws_bytes, _stream(g)))
        return dx
    dx = torch.empty(lead + (kdim,), dtype=torch.float32, device=g.device)
    ws_bytes = int(L.nnc_cbpk_grouped_dx_workspace_bytes(m, kdim, ncols, bits))
    ws = _workspace(ws_bytes, g.device)
    nat.check(L.nnc_cbpk_grouped_dx_f32(_ptr(g), m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, _ptr(centers), codes.k, group_rows, _ptr(dx),
                                        _ptr(ws), ws_bytes, _stream(g)))
    return dx


def grouped_packed_codebook_centroid_grad(x: torch.Tensor, g: torch.Tensor, codes: PackedCodes, group_rows: int, dtype=torch.float64) -> torch.Tensor:
    """dc[q, j] = sum over the (i, o) with i // group_rows = q whose label is j of (x^T g)[i, o] (include/nnc_cbpkgrad_grouped.h,
    nnc_cbpk_grouped_dc_f32): bit for bit grouped_codebook_centroid_grad(x, g, codes.to_dense(), codes.k, ...), the indices never
    unpacked and dW never written.  x: float32 (..., kdim), g: float32 (..., ncols) with the same leading shape.  Returns ``dtype``
    (float64 or float32) (G, codes.k).  No host read.
    x and g both bfloat16 or both float16 take nnc_cbpk_grouped_dc_h16: bit for bit the half
    grouped_codebook_centroid_grad on codes.to_dense()."""
    group_rows = int(group_rows)
    if isinstance(x, torch.Tensor) and isinstance(g, torch.Tensor) and x.dtype != g.dtype and (x.dtype in _H16_DT or g.dtype in _H16_DT):
        raise TypeError(f"x and g must have one dtype, got {x.dtype} and {g.dtype}")
    _require_cuda(x, "x", x.dtype if isinstance(x, torch.Tensor) and x.dtype in _H16_DT else torch.float32)
    _require_cuda(g, "g", g.dtype if isinstance(g, torch.Tensor) and g.dtype in _H16_DT else torch.float32)
    groups = _grouped_packed_args(codes, None, group_rows)
    kdim, ncols, k, bits = codes.kdim, codes.ncols, codes.k, codes.bits
    lead, m = _rows(g, "g", ncols)
    _dc_args(x, lead, kdim, "x, g and codes", codes.packed, g, dtype)
    L = nat.load()
    dc = torch.empty((groups, k), dtype=dtype, device=x.device)
    if x.dtype in _H16_DT:
        ws_bytes = int(L.nnc_cbpk_grouped_dc_h16_workspace_bytes(m, kdim, ncols, bits, k, group_rows))
        ws = _workspace(ws_bytes, x.device)
        nat.check(L.nnc_cbpk_grouped_dc_h16(_ptr(x), _ptr(g), _H16_DT[x.dtype], m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, k, group_rows,
                                            _ptr(dc), 1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
        return dc
    ws_bytes = int(L.nnc_cbpk_grouped_dc_workspace_bytes(m, kdim, ncols, bits, k, group_rows))
    ws = _workspace(ws_bytes, x.device)
    nat.check(L.nnc_cbpk_grouped_dc_f32(_ptr(x), _ptr(g), m, kdim, _ptr(codes.packed), codes.nbytes, bits, ncols, k, group_rows, _ptr(dc),
                                        1 if dtype == torch.float64 else 0, _ptr(ws), ws_bytes, _stream(x)))
    return dc


def cbpk_grouped_dx_plan(m: int, kdim: int, ncols: int, bits: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_grouped_dx_f32 follows on a device with ``cus`` compute units (include/nnc_cbpkgrad_grouped.h,
    nnc_cbpk_grouped_dx_plan), as a dict keyed by _native.CBPKDX_GROUPED_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_grouped_dx_plan, nat.CBPKDX_GROUPED_PLAN_FIELDS, m, kdim, ncols, bits, k, group_rows, cus)


def cbpk_grouped_dc_plan(m: int, kdim: int, ncols: int, bits: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_grouped_dc_f32 follows on a device with ``cus`` compute units (include/nnc_cbpkgrad_grouped.h,
    nnc_cbpk_grouped_dc_plan), as a dict keyed by _native.CBPKDC_GROUPED_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_grouped_dc_plan, nat.CBPKDC_GROUPED_PLAN_FIELDS, m, kdim, ncols, bits, k, group_rows, cus)


def cbpk_grouped_dx_h16_plan(dtype, m: int, kdim: int, ncols: int, bits: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_grouped_dx_h16 follows for g of ``dtype`` (torch.bfloat16 / torch.float16) on a device with ``cus``
    compute units (include/nnc_cbgrad_grouped_h16.h), as a dict keyed by _native.CBPKDX_GROUPED_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_grouped_dx_h16_plan, nat.CBPKDX_GROUPED_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, bits, k, group_rows, cus)


def cbpk_grouped_dc_h16_plan(dtype, m: int, kdim: int, ncols: int, bits: int, k: int, group_rows: int, cus: int) -> dict:
    """Host: the plan nnc_cbpk_grouped_dc_h16 follows for x and g of ``dtype`` (include/nnc_cbgrad_grouped_h16.h), as a dict keyed by
    _native.CBPKDC_GROUPED_H16_PLAN_FIELDS.  No device needed."""
    return _plan(nat.load().nnc_cbpk_grouped_dc_h16_plan, nat.CBPKDC_GROUPED_H16_PLAN_FIELDS, _h16_dt(dtype), m, kdim, ncols, bits, k, group_rows, cus)


def grouped_packed_codebook_linear(x: torch.Tensor, codes: PackedCodes, centers: torch.Tensor, group_rows: int, bias: torch.Tensor | None = None,
                                   relu: bool = False, half_inputs: bool = False) -> torch.Tensor:
    """grouped_packed_codebook_matmul with gradients for x, centers (G, K) and bias, through the autograd Function of codebook_linear.
    The forward is the same float32 nnc_cbpk_grouped call (under no_grad the bits of grouped_packed_codebook_matmul, which stays
    inference only); the backward runs grouped_packed_codebook_matmul_dx only if x needs a gradient and
    grouped_packed_codebook_centroid_grad (float32) only if centers does.  The ReLU mask and the bias gradient are codebook_linear's.
    The indices get no gradient.  No host read.
    ``half_inputs=True`` lets a bfloat16 or float16 x through, as in grouped_codebook_linear; without it a half
    x raises ``TypeError`` as before."""
    if not isinstance(codes, PackedCodes):
        raise TypeError("codes must be a PackedCodes (ops.pack_codes)")
    if not half_inputs:
        _require_f32_x(x, "grouped_packed_codebook_linear")
    elif isinstance(x, torch.Tensor) and x.dtype in _H16_DT:
        _require_centers_bias(centers, bias)
    group_rows = int(group_rows)
    return _CodebookLinear.apply(
        x, codes, centers, bias, bool(relu), codes.kdim, codes.ncols,
        lambda x2, cd, c, b, r: grouped_packed_codebook_matmul(x2, cd, c, group_rows, bias=b, relu=r),
        lambda g2, cd, c: grouped_packed_codebook_matmul_dx(g2, cd, c, group_rows),
        lambda x2, g2, cd, c: grouped_packed_codebook_centroid_grad(x2, g2, cd, group_rows, dtype=torch.float32))


def huffman_lengths(counts) -> tuple:
    """Host: (lengths uint8[k], hist int64[max_len+1], total_bits) from an index histogram."""
    L = nat.load()
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.int64))
    k = c.size
    lengths = np.zeros(k, dtype=np.uint8)
    hist = np.zeros(65, dtype=np.int64)
    total = ctypes.c_int64(0)
    nat.check(L.nnc_huffman_lengths(c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), k,
                                    lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                    hist.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(total)))
    top = int(lengths.max()) if k else 0
    return lengths, hist[: top + 1].copy(), int(total.value)


# ------------------------------------------------------------------ fixed-point rule (host mirror)
def fix_shift(absmax: float, n_total: int) -> int:
    """S of the fixed-point sums (same rule as nnc_fix_shift; pure host arithmetic)."""
    L = max(1, (int(n_total) - 1).bit_length())
    if not (absmax > 0) or not math.isfinite(absmax):
        return 0
    _, P = math.frexp(float(absmax))
    return min(28, 62 - L) - P


def fix_f32(v, S: int) -> int:
    """Fixed-point image of one float32, (int) rint(v * 2^S) with ties to even (bit-for-bit the
    device function fix_f32)."""
    from fractions import Fraction

    fr = Fraction(float(np.float32(v))) * (Fraction(2) ** int(S))
    fl = fr.numerator // fr.denominator
    rem = fr - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (fl & 1)):
        fl += 1
    return int(fl)
