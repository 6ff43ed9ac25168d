"""Quantized layers run from their stored form: a K-entry codebook and one 1- or 2-byte centroid index per weight.

``Trainer.quantize`` writes ``cluster_centers_[labels_]`` back into the float32 parameters, so the network it leaves reads
4 bytes per weight in every forward pass.  The layers here keep what the fit produced -- ``cluster_centers_`` and
``labels_compact_`` -- and multiply with the indices directly (ops.codebook_matmul, csrc/nnc_cbmm.hip): the float32 weight
tensor is never rebuilt.  Biases (one value per output column) are decoded once at construction and added by the kernel.

    CompressedDense.from_dense(dense, weight_model, bias_model)
    CompressedConv2D.from_conv(conv, weight_model, bias_model)     stride 1, padding "valid" | "same", NHWC in and out
    compress_network(network, models_by_layer, sparse=False, trainable=False, packed=False)   a deep copy with the quantized layers replaced
    load_network(path, network, sparse=False, packed=False)        the same from a ``weights.nnc`` (Trainer.store_report)
    pack_grouped_layers(network, packed=True)                      a deep copy with the grouped layers' indices packed to 2 or 4 bits
    sparsify_grouped_layers(network, sparse=True)                  a deep copy with the grouped layers' indices in the bitmap-sparse form
    smallest_grouped_layers(network)                               a deep copy with every grouped layer in the smallest of its three forms
    compressed_nbytes(network)                                     resident bytes of the layers' tensors

A pruned layer can instead keep its indices in the bitmap-sparse form (ops.pack_sparse_codes, csrc/nnc_cbsp.hip, DESIGN.md
section 11): one bit per weight, a count per 64 columns, and only the indices that are not the skipped (pruned) cluster's.
``SparseCompressedDense`` / ``SparseCompressedConv2D``; ``sparse=True`` in compress_network / load_network /
Trainer.compressed_network takes it for every quantized layer, ``sparse="auto"`` for each layer whose sparse form is smaller.

A layer of at most 16 centres can keep its indices at 2 or 4 bits each (ops.pack_codes, csrc/nnc_cbpk.hip, DESIGN.md section
14): rows of whole 16-byte groups, a half or a quarter of the byte form.  ``PackedCompressedDense`` / ``PackedCompressedConv2D``;
``packed=True`` in compress_network / load_network / Trainer.compressed_network takes it for every layer it can hold (K <= 16:
it is the number of centres that decides, not the ``bits`` of the fit), ``packed="auto"`` where it is the smallest.  Per layer
the candidates are the byte form (unless ``sparse is True``, or ``packed is True`` and K <= 16), the bitmap-sparse form (if
``sparse`` is not False) and the packed form (if ``packed`` is not False and K <= 16); the one with the fewest resident bytes is
kept, on equal bytes the earlier in this list.  The selection is by bytes, not by speed.

``CompressedDense`` / ``CompressedConv2D`` also run on bfloat16 and float16 inputs (ops.codebook_matmul -> nnc_cbmm_h16,
csrc/nnc_cbmm_h16.hip): the path is chosen by the input's dtype and the output has that dtype, so a chain
of compressed layers stays in half.  ``centers`` and ``bias`` stay float32 buffers (each centre is rounded to the input's dtype
inside the kernel, the bias is added in float32): feed half inputs, leave the module float32.  A module cast with ``.half()`` /
``.bfloat16()`` turns those buffers into half tensors, and the layer then raises the dtype ``TypeError`` of ops.codebook_matmul.
Half inputs are for the byte form unless a layer is built for them: the bitmap-sparse, the packed and every trainable layer raise
``TypeError`` on them (the trainable byte layers train on them when built with ``half_inputs=True``; so do
``TrainableSparseCompressedDense`` / ``TrainableSparseCompressedConv2D``, from their bitmap-sparse form, ops.sparse_codebook_linear ->
csrc/nnc_cbspgrad_h16.hip, DESIGN.md section 24: ``compress_network_trainable(..., sparse=..., sparse_half_inputs=True)``), and
``torch.autocast`` is not registered.  ``SparseCompressedDense`` / ``SparseCompressedConv2D`` built with ``half_inputs=True``
(``sparse_half_inputs=True`` in compress_network / load_network / Trainer.compressed_network) run on them too
(ops.sparse_codebook_matmul -> nnc_cbsp_h16, csrc/nnc_cbsp_h16.hip), path and output dtype by the input's dtype.
The four packed layers built with ``half_inputs=True`` (``packed_half_inputs=True`` in compress_network / load_network /
Trainer.compressed_network / compress_network_trainable) run and train on them as well (ops.packed_codebook_matmul /
ops.packed_codebook_linear -> csrc/nnc_cbpk_h16.hip).  The two grouped trainable layers built with
``half_inputs=True`` (compress_network_trainable_grouped(..., half_inputs=True), Trainer.fine_tune_grouped(..., activation_dtype=))
train on them too (csrc/nnc_cbgrad_grouped_h16.hip, csrc/nnc_cbpkgrad_grouped_h16.hip).

``GroupedCompressedDense`` runs a Dense layer whose kernel has one codebook per block of ``group_rows`` input rows
(utility.get_quantized_weight_grouped, Trainer.quantize(..., group_rows=); ops.grouped_codebook_matmul, csrc/nnc_cbmm_grouped.hip,
DESIGN.md section 17), on float32, bfloat16 and float16 inputs as ``CompressedDense`` does.  compress_network and load_network
build it for a layer fitted that way; there ``sparse``, ``packed`` and ``trainable`` raise ``NotImplementedError`` naming the
layer.  ``pack_grouped_layers(network, packed=True | "auto")`` is the way to the 2- and 4-bit packed form of grouped layers of at
most 16 centres per group: ``GroupedPackedCompressedDense`` (ops.grouped_packed_codebook_matmul, csrc/nnc_cbpk_grouped.hip,
DESIGN.md section 18), the same function from a half or a quarter of the index bytes, on the same three input dtypes.
``sparsify_grouped_layers(network, sparse=True | "auto")`` is the way to the bitmap-sparse form of a pruned grouped layer, with one
skipped index per group: ``GroupedSparseCompressedDense`` (ops.grouped_sparse_codebook_matmul, csrc/nnc_cbsp_grouped.hip, DESIGN.md
section 28), on float32 inputs, and built with ``half_inputs=True`` (a keyword of the layer and of both functions here) on bfloat16 and
float16 inputs too (csrc/nnc_cbsp_grouped_h16.hip); ``smallest_grouped_layers(network)`` picks per layer, by
resident bytes, among the byte, the packed and the sparse form.

These layers are inference only: under autograd, with an input that needs a gradient, they raise instead of returning a result
that silently has none.  ``trainable=True`` in compress_network / Trainer.compressed_network gives the trainable variants instead
(``TrainableCompressedDense`` / ``TrainableCompressedConv2D``): their ``centers`` is an nn.Parameter and the
forward goes through ops.codebook_linear, whose backward forms dx and the centroid gradient from the codebook and the indices
(csrc/nnc_cbgrad.hip) -- W and dW are never built.  A quantized bias keeps its indices and a ``bias_centers`` parameter; a raw bias
stays frozen.  ``kernel_sq_sum()`` gives the trainers' L2 term without W.  Trainer.fine_tune_compressed trains them.

    compress_network_trainable(network, models_by_layer, sparse=False, packed=False)   the trainable layers, byte, bitmap-sparse, packed or per layer

The bitmap-sparse layers train too (``TrainableSparseCompressedDense`` / ``TrainableSparseCompressedConv2D``, DESIGN.md section
13): ops.sparse_codebook_linear's backward forms dx and the centroid gradient from the packed form (csrc/nnc_cbspgrad.hip), and
the centroid gradient is the dense trainable layer's bit for bit -- the same function, stored differently.
compress_network_trainable(..., sparse=True | "auto") and Trainer.fine_tune_compressed(..., sparse=...) give them;
compress_network(..., trainable=True) stays the dense form.

So do the packed layers (``TrainablePackedCompressedDense`` / ``TrainablePackedCompressedConv2D``):
ops.packed_codebook_linear's backward forms dx and the centroid gradient from the 2- or 4-bit packed rows (csrc/nnc_cbpkgrad.hip),
the centroid gradient again the byte layer's bit for bit, and no byte-per-weight tensor stays resident while training.
compress_network_trainable(..., packed=True | "auto") and Trainer.fine_tune_compressed(..., packed=...) give them, chosen per
layer by the rule above applied to the trainable forms.

A grouped Dense layer trains too (``TrainableGroupedCompressedDense``): ops.grouped_codebook_linear's
backward forms dx and the (G, K) centroid gradient from the codebooks and the byte indices (csrc/nnc_cbgrad_grouped.hip).  The
options above keep refusing grouped layers; the way in is

    compress_network_trainable_grouped(network, models_by_layer, packed=False)   the byte trainable layers, grouped Dense layers included

and Trainer.fine_tune_grouped trains it.  With ``packed=True | "auto"`` there a grouped layer of at most 16 centres per group
trains from its 2- or 4-bit packed indices (``TrainableGroupedPackedCompressedDense``):
ops.grouped_packed_codebook_linear's backward forms dx and the (G, K) centroid gradient from the packed rows
(csrc/nnc_cbpkgrad_grouped.hip), the centroid gradient the byte grouped layer's bit for bit, and no byte-per-weight tensor stays
resident while training.  With ``sparse=True | "auto"`` there a pruned grouped layer trains from the bitmap-sparse form of its
indices (``TrainableGroupedSparseCompressedDense``): ops.grouped_sparse_codebook_linear's backward forms dx and
the (G, K) centroid gradient from the buffer of ``GroupedSparseCompressedDense`` (csrc/nnc_cbspgrad_grouped.hip), the centroid
gradient again the byte grouped layer's bit for bit, on float32 activations only.  Grouped Conv2D does not train.

How the classes are laid out: ``_Activated`` (the activation behind the product, ``get_weights``) is the root of
``_InferenceLayer`` (the float32 ``centers`` / ``bias`` buffers behind the family's index buffer, ``nbytes``) and of
``_TrainableCentres`` (the ``centers`` parameter, ``counts``, the three kinds of bias).  A family -- ``_CodebookLayer``,
``GroupedCompressedDense``, ``GroupedPackedCompressedDense``, ``GroupedSparseCompressedDense``, ``_SparseCodebookLayer``, ``_PackedCodebookLayer`` and the trainable ones -- adds its index
buffer and the one ops call of ``_matmul``; ``_SparseForm`` / ``_PackedForm`` hold what the inference and the trainable layer of
a form share (the ``packed`` buffer, the metadata, ``codes``).  ``_DenseHalf`` and ``_Conv2DHalf`` are the two forwards over
``_matmul``; a public class is one of them on a family, with the constructors of its own signature.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ops

_PATCH_BYTES = 256 << 20   # a Conv2D forward unfolds at most this many bytes of patches at a time


def _codes(model, device):
    centers = torch.from_numpy(np.ascontiguousarray(model.cluster_centers_.ravel(), dtype=np.float32)).to(device)
    return centers, model.labels_compact_


def _decoded_bias(raw: torch.Tensor, bias_model) -> torch.Tensor:
    if bias_model is None:
        return raw.detach().reshape(-1).clone()
    centers, labels = _codes(bias_model, raw.device)
    return ops.gather(centers, labels)


def _require_model(weight_model):
    if weight_model is None:
        raise ValueError("the kernel was not quantized (no fitted model): keep the float32 layer")


def _conv_shape(conv):
    """(h, in, out) of a Keras (h, w, in, out) kernel, which has to be square."""
    h, w, cin, cout = conv.kernel.shape
    if h != w:
        raise ValueError("square kernels only (as layers.Conv2D)")
    return h, cin, cout


def _inference_codes(layer, weight_model, bias_model):
    """What from_dense / from_conv of the inference layers start from: (labels, centers, decoded bias), in the order the
    from_codes take them."""
    _require_model(weight_model)
    centers, labels = _codes(weight_model, layer.kernel.device)
    return labels, centers, _decoded_bias(layer.bias, bias_model)


def _trainable_codes(layer, weight_model, bias_model):
    """(labels, centers, raw bias, bias codes) of a trainable layer: a quantized bias keeps its codes, a raw one stays frozen."""
    _require_model(weight_model)
    centers, labels = _codes(weight_model, layer.kernel.device)
    bias, bias_codes = (None, _codes(bias_model, layer.kernel.device)) if bias_model is not None else (layer.bias, None)
    return labels, centers, bias, bias_codes


def _tensor_bytes(*tensors) -> int:
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


class _Activated(nn.Module):
    """What every layer here does behind its product: the activation (a ReLU is fused into the kernel, any other applied to
    its result) and the empty Keras weight list."""

    def _set_activation(self, activation):
        self.activation = activation
        self._fused_relu = activation is torch.relu

    def _activate(self, y: torch.Tensor) -> torch.Tensor:
        if self.activation is not None and not self._fused_relu:
            y = self.activation(y)
        return y

    def get_weights(self):
        return []


class _InferenceLayer(_Activated):
    """The base of the four inference families: behind the index buffer ``_INDEX`` names (registered first by the family), the
    float32 buffers centers and bias (or None)."""

    _INDEX = "labels"

    def _init_codebook(self, centers: torch.Tensor, bias: torch.Tensor | None, activation):
        self.register_buffer("centers", centers.to(torch.float32).contiguous())
        self.register_buffer("bias", None if bias is None else bias.reshape(-1).to(torch.float32).contiguous())
        self._set_activation(activation)

    def nbytes(self) -> int:
        return _tensor_bytes(getattr(self, self._INDEX), self.centers, self.bias)


class _DenseHalf:
    """A Dense layer's forward over a family's ``_matmul``."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._matmul(x.contiguous())


class _Conv2DHalf:
    """A Conv2D layer's geometry and forward over a family's ``_matmul``."""

    def _set_conv(self, kernel_size: int, cin: int, pad: int):
        self.kernel_size, self.cin, self.pad = int(kernel_size), int(cin), int(pad)

    def forward(self, x: torch.Tensor) -> torch.Tensor:   # x: (N, H, W, C)
        return _conv_forward(self, x)


class _CodebookLayer(_InferenceLayer):
    """labels (kdim * ncols indices, row-major (kdim, ncols)), centers float32[K], bias float32[ncols] or None.  A bfloat16 or
    float16 input gives an output of that dtype (ops.codebook_matmul); centers and bias stay float32: feed half inputs, leave the
    module float32 (after ``.half()`` / ``.bfloat16()`` on the module the forward raises ops.codebook_matmul's dtype TypeError)."""

    def __init__(self, kdim: int, ncols: int, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None, activation=None):
        super().__init__()
        if labels.numel() != kdim * ncols:
            raise ValueError(f"{labels.numel()} indices for a {kdim} x {ncols} weight matrix")
        self.kdim, self.ncols = int(kdim), int(ncols)
        self.register_buffer("labels", labels.reshape(-1))
        self._init_codebook(centers.reshape(-1), bias, activation)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(ops.codebook_matmul(x, self.labels, self.centers, self.kdim, self.ncols, bias=self.bias, relu=self._fused_relu))


class CompressedDense(_DenseHalf, _CodebookLayer):
    """Dense run from its codebook: y = act(x @ kernel + bias), kernel (in, out) as Keras stores it (kdim = in, ncols = out)."""

    @classmethod
    def from_dense(cls, dense, weight_model, bias_model=None) -> "CompressedDense":
        codes = _inference_codes(dense, weight_model, bias_model)
        kin, kout = dense.kernel.shape
        return cls(kin, kout, *codes, dense.activation)


class GroupedCompressedDense(_DenseHalf, _InferenceLayer):
    """Dense run from one codebook per block of ``group_rows`` input rows: labels (kdim * ncols uint8 indices, row-major),
    centers float32 (G, K), G = ceil(kdim / group_rows), bias float32[ncols] or None.  The path follows the input's dtype as in
    CompressedDense (float32, bfloat16, float16; the output has the input's dtype); centers and bias stay float32."""

    def __init__(self, kdim: int, ncols: int, group_rows: int, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None,
                 activation=None):
        super().__init__()
        if labels.numel() != kdim * ncols:
            raise ValueError(f"{labels.numel()} indices for a {kdim} x {ncols} weight matrix")
        if labels.dtype != torch.uint8:
            raise TypeError(f"group-wise codebooks take uint8 indices, got {labels.dtype}")
        groups = max(1, -(-int(kdim) // int(group_rows)))
        if centers.dim() != 2 or centers.shape[0] != groups:
            raise ValueError(f"centers must have shape ({groups}, K) for {kdim} rows in groups of {group_rows}, got {tuple(centers.shape)}")
        self.kdim, self.ncols, self.group_rows = int(kdim), int(ncols), int(group_rows)
        self.register_buffer("labels", labels.reshape(-1))
        self._init_codebook(centers, bias, activation)

    @classmethod
    def from_dense(cls, dense, weight_model, bias_model=None) -> "GroupedCompressedDense":
        """From a Dense layer and the GroupedModel of its kernel (utility.get_quantized_weight_grouped)."""
        _require_model(weight_model)
        kin, kout = dense.kernel.shape
        centers = torch.from_numpy(np.ascontiguousarray(weight_model.cluster_centers_, dtype=np.float32)).to(dense.kernel.device)
        return cls(kin, kout, weight_model.group_rows, weight_model.labels_compact_, centers, _decoded_bias(dense.bias, bias_model), dense.activation)

    @classmethod
    def from_codes(cls, kdim, ncols, group_rows, labels, centers, bias, activation) -> "GroupedCompressedDense":
        return cls(kdim, ncols, group_rows, labels, centers, bias, activation)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(ops.grouped_codebook_matmul(x, self.labels, self.centers, self.kdim, self.ncols, self.group_rows, bias=self.bias,
                                                          relu=self._fused_relu))


def _is_grouped(model) -> bool:
    return hasattr(model, "group_rows")


def _grouped_only_byte_form(name, what):
    raise NotImplementedError(f"layer {name!r} has group-wise codebooks (group_rows): {what} is not implemented for it; "
                              "build it in the byte form (GroupedCompressedDense); pack_grouped_layers packs its indices afterwards")


def keras_rows_for_unfold(h: int, w: int, cin: int) -> np.ndarray:
    """Row r of ``F.unfold``'s patch matrix is (c, dy, dx) = r // (h*w), (r // w) % h, r % w; the same tap is row
    (dy * w + dx) * cin + c of a Keras (h, w, in, out) kernel flattened to (h*w*in, out).  Returns those Keras rows, int64[h*w*in]:
    kernel.reshape(h*w*in, out)[keras_rows_for_unfold(h, w, cin)] is the kernel in unfold order."""
    r = np.arange(h * w * cin, dtype=np.int64)
    c, dy, dx = r // (h * w), (r // w) % h, r % w
    return (dy * w + dx) * cin + c


def conv_patches(x: torch.Tensor, kernel_size: int, pad: int) -> torch.Tensor:
    """NHWC input -> (N, Ho * Wo, kernel_size^2 * C) patches in unfold order (c, dy, dx), stride 1, ``pad`` zeros on every side."""
    p = F.unfold(x.permute(0, 3, 1, 2), kernel_size=kernel_size, padding=pad)
    return p.transpose(1, 2)


class CompressedConv2D(_Conv2DHalf, _CodebookLayer):
    """Conv2D (stride 1, NHWC) run from its codebook: the patches of x times the kernel read from its indices, whose rows are
    put in unfold order once at construction (keras_rows_for_unfold)."""

    def __init__(self, kernel_size: int, cin: int, cout: int, pad: int, labels_unfold: torch.Tensor, centers: torch.Tensor,
                 bias: torch.Tensor | None, activation=None):
        super().__init__(kernel_size * kernel_size * cin, cout, labels_unfold, centers, bias, activation)
        self._set_conv(kernel_size, cin, pad)

    @classmethod
    def from_conv(cls, conv, weight_model, bias_model=None) -> "CompressedConv2D":
        codes = _inference_codes(conv, weight_model, bias_model)
        h, cin, cout = _conv_shape(conv)
        return cls.from_codes(h, cin, cout, conv.pad, *codes, conv.activation)

    @classmethod
    def from_codes(cls, kernel_size, cin, cout, pad, labels, centers, bias, activation) -> "CompressedConv2D":
        """labels in the Keras order of the (h, w, in, out) kernel."""
        return cls(kernel_size, cin, cout, pad, _unfold_labels(kernel_size, cin, cout, labels), centers, bias, activation)


def _conv_forward(layer, x: torch.Tensor) -> torch.Tensor:
    """The patches of NHWC x, at most _PATCH_BYTES of them at a time, through layer._matmul -> (N, Ho, Wo, ncols)."""
    n, hh, ww, _ = x.shape
    ho, wo = hh + 2 * layer.pad - layer.kernel_size + 1, ww + 2 * layer.pad - layer.kernel_size + 1
    per = max(1, _PATCH_BYTES // max(1, ho * wo * layer.kdim * x.element_size()))
    outs = [layer._matmul(conv_patches(x[i: i + per], layer.kernel_size, layer.pad).contiguous()) for i in range(0, n, per)]
    if not outs:   # an empty batch: the (0, kdim) product, as F.conv2d gives an empty result
        outs = [layer._matmul(x.new_empty((0, layer.kdim)))]
    y = outs[0] if len(outs) == 1 else torch.cat(outs)
    return y.reshape(n, ho, wo, layer.ncols)


def _unfold_labels(kernel_size: int, cin: int, cout: int, labels: torch.Tensor) -> torch.Tensor:
    """Labels of a Keras (h, w, in, out) kernel -> the same labels with their rows in unfold order (keras_rows_for_unfold)."""
    rows = torch.from_numpy(keras_rows_for_unfold(kernel_size, kernel_size, cin)).to(labels.device)
    return labels.reshape(-1, cout)[rows].contiguous()


def _unfold_then_pack(pack, kernel_size: int, cin: int, cout: int, labels: torch.Tensor, k: int, option):
    """The codes of a Conv2D layer: ``pack`` (ops.pack_sparse_codes with its zero_symbol, ops.pack_codes with its bits) over the
    labels in unfold order, which are dropped once packed."""
    return pack(_unfold_labels(kernel_size, cin, cout, labels), kernel_size * kernel_size * cin, cout, k, option)


def _check_conv_rows(codes, kernel_size: int, cin: int):
    if codes.kdim != kernel_size * kernel_size * cin:
        raise ValueError(f"{codes.kdim} index rows for a {kernel_size} x {kernel_size} x {cin} kernel")


class _GatherCenters(torch.autograd.Function):
    """centers[labels] (ops.gather) with the centroid gradient of the result (ops.centroid_gradient) as the backward."""

    @staticmethod
    def forward(ctx, centers, labels):
        ctx.save_for_backward(labels)
        ctx.k = centers.numel()
        return ops.gather(centers.detach().contiguous(), labels)

    @staticmethod
    def backward(ctx, grad):
        (labels,) = ctx.saved_tensors
        return ops.centroid_gradient(grad.contiguous(), labels, ctx.k).to(torch.float32), None


class _TrainableCentres(_Activated):
    """What the trainable layers share: centers a float32[K] nn.Parameter, counts (the histogram of the kdim * ncols indices, for
    kernel_sq_sum) a buffer, and the bias: a quantized one (bias_labels buffer + bias_centers parameter), a frozen raw one (bias
    buffer) or None."""

    def _init_centres(self, labels: torch.Tensor, centers: torch.Tensor, ncols: int, bias, bias_codes, activation, counts=None):
        """``counts`` given (the grouped layer: a histogram per group): the centres keep their shape, which is that of counts."""
        flat = centers.detach().to(torch.float32)
        self.centers = nn.Parameter((flat.reshape(-1) if counts is None else flat).clone())
        self.register_buffer("counts", ops.bincount(labels, self.centers.numel()) if counts is None else counts)
        if bias_codes is not None:
            bcenters, blabels = bias_codes
            if blabels.numel() != ncols:
                raise ValueError(f"{blabels.numel()} bias indices for {ncols} columns")
            self.register_buffer("bias_labels", blabels.reshape(-1))
            self.bias_centers = nn.Parameter(bcenters.detach().reshape(-1).to(torch.float32).clone())
            self.register_buffer("bias", None)
        else:
            self.register_buffer("bias_labels", None)
            self.bias_centers = None
            self.register_buffer("bias", None if bias is None else bias.detach().reshape(-1).to(torch.float32).clone())
        self._set_activation(activation)

    def current_bias(self) -> torch.Tensor | None:
        if self.bias_centers is not None:
            return _GatherCenters.apply(self.bias_centers, self.bias_labels)
        return self.bias

    def kernel_sq_sum(self) -> torch.Tensor:
        """sum of kernel^2 = sum_k count_k * c_k^2, differentiable in the centres, without W."""
        return (self.counts.to(torch.float32) * self.centers ** 2).sum()

    def _nbytes(self, indices: torch.Tensor) -> int:
        return _tensor_bytes(indices, self.centers, self.bias, self.bias_labels, self.bias_centers)


class _TrainableCodebookLayer(_TrainableCentres):
    """labels (kdim * ncols indices, row-major (kdim, ncols)) a buffer; the centres, counts and bias of _TrainableCentres.
    ``half_inputs=True`` lets the layer train on bfloat16 / float16 inputs (ops.codebook_linear): the output and
    the input gradient have the input's dtype, centres and bias stay float32 parameters with float32 gradients.  Without it a half
    input raises ``TypeError``: training in half is a numerics decision the caller makes knowingly."""

    def __init__(self, kdim: int, ncols: int, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None = None,
                 bias_codes=None, activation=None, half_inputs: bool = False):
        super().__init__()
        if labels.numel() != kdim * ncols:
            raise ValueError(f"{labels.numel()} indices for a {kdim} x {ncols} weight matrix")
        self.kdim, self.ncols = int(kdim), int(ncols)
        self.half_inputs = bool(half_inputs)
        self.register_buffer("labels", labels.reshape(-1))
        self._init_centres(self.labels, centers, ncols, bias, bias_codes, activation)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        if not self.half_inputs and x.dtype in (torch.bfloat16, torch.float16):
            raise TypeError(f"{type(self).__name__} takes float32 activations, got {x.dtype}: a trainable layer of the byte form trains on "
                            "bfloat16 and float16 inputs only when built with half_inputs=True")
        return self._activate(ops.codebook_linear(x, self.labels, self.centers, self.kdim, self.ncols, bias=self.current_bias(),
                                                  relu=self._fused_relu))

    def nbytes(self) -> int:
        return self._nbytes(self.labels)


class TrainableCompressedDense(_DenseHalf, _TrainableCodebookLayer):
    """CompressedDense with trainable centres (ops.codebook_linear)."""


class TrainableCompressedConv2D(_Conv2DHalf, _TrainableCodebookLayer):
    """CompressedConv2D with trainable centres: the patches (F.unfold, chunked as CompressedConv2D) through ops.codebook_linear;
    autograd carries the patch gradients back through the unfold."""

    def __init__(self, kernel_size: int, cin: int, cout: int, pad: int, labels_unfold: torch.Tensor, centers: torch.Tensor, bias=None,
                 bias_codes=None, activation=None, half_inputs: bool = False):
        super().__init__(kernel_size * kernel_size * cin, cout, labels_unfold, centers, bias, bias_codes, activation, half_inputs)
        self._set_conv(kernel_size, cin, pad)


def _group_counts(labels: torch.Tensor, per: int, groups: int, k: int) -> torch.Tensor:
    """The (G, K) histogram of every group's indices: a group's ``per`` = group_rows * ncols indices lie one after the other."""
    return torch.stack([ops.bincount(labels[q * per: (q + 1) * per], k) for q in range(groups)])


class TrainableGroupedCompressedDense(_DenseHalf, _TrainableCentres):
    """GroupedCompressedDense with trainable centres (ops.grouped_codebook_linear): labels (kdim * ncols uint8
    indices, row-major) a buffer, centers a float32 (G, K) nn.Parameter, counts the (G, K) histogram of every group's indices, so
    kernel_sq_sum() = sum counts * centers^2; the bias of _TrainableCentres.  The backward forms dx and the (G, K) centroid
    gradient from the codebooks and the indices (csrc/nnc_cbgrad_grouped.hip): W and dW are never built.  ``half_inputs=True`` lets
    the layer train on bfloat16 / float16 inputs (csrc/nnc_cbgrad_grouped_h16.hip): the output and the input
    gradient have the input's dtype, centres and bias stay float32 with float32 gradients.  Without it a half input raises
    ``TypeError``."""

    def __init__(self, kdim: int, ncols: int, group_rows: int, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None = None,
                 bias_codes=None, activation=None, half_inputs: bool = False):
        super().__init__()
        if labels.numel() != kdim * ncols:
            raise ValueError(f"{labels.numel()} indices for a {kdim} x {ncols} weight matrix")
        if labels.dtype != torch.uint8:
            raise TypeError(f"group-wise codebooks take uint8 indices, got {labels.dtype}")
        groups = max(1, -(-int(kdim) // int(group_rows)))
        if centers.dim() != 2 or centers.shape[0] != groups:
            raise ValueError(f"centers must have shape ({groups}, K) for {kdim} rows in groups of {group_rows}, got {tuple(centers.shape)}")
        self.kdim, self.ncols, self.group_rows = int(kdim), int(ncols), int(group_rows)
        self.half_inputs = bool(half_inputs)
        self.register_buffer("labels", labels.reshape(-1))
        counts = _group_counts(self.labels, self.group_rows * self.ncols, groups, centers.shape[1])
        self._init_centres(self.labels, centers, ncols, bias, bias_codes, activation, counts=counts)

    @classmethod
    def from_dense(cls, dense, grouped_model, bias_model=None, half_inputs: bool = False) -> "TrainableGroupedCompressedDense":
        """From a Dense layer and the GroupedModel of its kernel; a quantized bias keeps its codes, a raw one stays frozen."""
        _require_model(grouped_model)
        kin, kout = dense.kernel.shape
        dev = dense.kernel.device
        centers = torch.from_numpy(np.ascontiguousarray(grouped_model.cluster_centers_, dtype=np.float32)).to(dev)
        bias, bias_codes = (None, _codes(bias_model, dev)) if bias_model is not None else (dense.bias, None)
        return cls(kin, kout, grouped_model.group_rows, grouped_model.labels_compact_, centers, bias, bias_codes, dense.activation, half_inputs)

    @classmethod
    def from_codes(cls, kdim, ncols, group_rows, labels, centers, bias=None, bias_codes=None, activation=None,
                   half_inputs: bool = False) -> "TrainableGroupedCompressedDense":
        return cls(kdim, ncols, group_rows, labels, centers, bias, bias_codes, activation, half_inputs)

    @classmethod
    def from_grouped(cls, layer: GroupedCompressedDense, half_inputs: bool = False) -> "TrainableGroupedCompressedDense":
        """The trainable layer of a GroupedCompressedDense: the same indices and centres, its decoded bias frozen."""
        return cls(layer.kdim, layer.ncols, layer.group_rows, layer.labels, layer.centers, layer.bias, None, layer.activation, half_inputs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(ops.grouped_codebook_linear(x, self.labels, self.centers, self.kdim, self.ncols, self.group_rows,
                                                          bias=self.current_bias(), relu=self._fused_relu, half_inputs=self.half_inputs))

    def nbytes(self) -> int:
        return self._nbytes(self.labels)


def _trainable(layer, weight_model, bias_model, dense_cls=None, conv_cls=None, half_inputs=False):
    """The trainable layer of ``layer``, the one Dense / Conv2D dispatch of the trainable forms: through from_dense / from_conv
    of ``dense_cls`` / ``conv_cls`` (the bitmap-sparse or the packed pair), or, without them, the byte classes built here
    (``half_inputs``: the byte classes', and the bitmap-sparse and the packed pair's from_dense / from_conv)."""
    from .neural_networks.layers import Conv2D, Dense

    if dense_cls is None:   # the byte form takes its codes before it looks at the layer's type, as it always did
        labels, centers, bias, bias_codes = _trainable_codes(layer, weight_model, bias_model)
    if isinstance(layer, Dense):
        if dense_cls is not None:
            return dense_cls.from_dense(layer, weight_model, bias_model, **(dict(half_inputs=True) if half_inputs else {}))
        kin, kout = layer.kernel.shape
        return TrainableCompressedDense(kin, kout, labels, centers, bias, bias_codes, layer.activation, half_inputs)
    if isinstance(layer, Conv2D):
        if conv_cls is not None:
            return conv_cls.from_conv(layer, weight_model, bias_model, **(dict(half_inputs=True) if half_inputs else {}))
        h, cin, cout = _conv_shape(layer)
        return TrainableCompressedConv2D(h, cin, cout, layer.pad, _unfold_labels(h, cin, cout, labels), centers, bias, bias_codes,
                                         layer.activation, half_inputs)
    raise TypeError(f"no compressed form of {type(layer).__name__}")


class _SparseForm:
    """What the inference and the trainable bitmap-sparse layers keep of an ops.SparseCodes: its buffer as the module's ``packed``
    buffer and its metadata as attributes, from which ``codes`` is the same SparseCodes again."""

    _INDEX = "packed"
    _product, _linear = staticmethod(ops.sparse_codebook_matmul), staticmethod(ops.sparse_codebook_linear)

    def _take_codes(self, codes: ops.SparseCodes):
        self.kdim, self.ncols = codes.kdim, codes.ncols
        self.k, self.zero_symbol, self.label_bytes, self.nnz = codes.k, codes.zero_symbol, codes.label_bytes, codes.nnz
        self.register_buffer("packed", codes.buf)

    @property
    def codes(self) -> ops.SparseCodes:
        return ops.SparseCodes(self.packed, self.kdim, self.ncols, self.k, self.zero_symbol, self.label_bytes, self.nnz)


class _PackedForm:
    """What the inference and the trainable packed layers keep of an ops.PackedCodes: its buffer as the module's ``packed``
    buffer and its metadata as attributes, from which ``codes`` is the same PackedCodes again."""

    _INDEX = "packed"
    _product, _linear = staticmethod(ops.packed_codebook_matmul), staticmethod(ops.packed_codebook_linear)

    def _take_codes(self, codes: ops.PackedCodes):
        self.kdim, self.ncols, self.bits, self.k = codes.kdim, codes.ncols, codes.bits, codes.k
        self.register_buffer("packed", codes.packed)

    @property
    def codes(self) -> ops.PackedCodes:
        return ops.PackedCodes(self.packed, self.kdim, self.ncols, self.bits, self.k)


class _CodesLayer(_InferenceLayer):
    """An inference layer over a form's codes (_SparseForm, _PackedForm): centers float32[K], bias float32[ncols] or None.  No
    kdim * ncols tensor stays resident."""

    def __init__(self, codes, centers: torch.Tensor, bias: torch.Tensor | None, activation=None):
        super().__init__()
        self._take_codes(codes)
        if centers.numel() != codes.k:
            raise ValueError(f"{centers.numel()} centres for indices into a codebook of {codes.k}")
        self._init_codebook(centers.reshape(-1), bias, activation)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(self._product(x, self.codes, self.centers, bias=self.bias, relu=self._fused_relu))


class _TrainableCodesLayer(_TrainableCentres):
    """A trainable layer over a form's codes: the ``packed`` buffer with the centres, counts and bias of _TrainableCentres; the
    forward goes through the form's ops.*_codebook_linear, whose backward forms dx and the centroid gradient from the stored form.
    ``counts`` is taken from the labels before packing, so kernel_sq_sum() is the byte trainable layer's bit for bit.  No
    kdim * ncols tensor stays resident."""

    def __init__(self, codes, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None = None, bias_codes=None, activation=None):
        super().__init__()
        if centers.numel() != codes.k:
            raise ValueError(f"{centers.numel()} centres for indices into a codebook of {codes.k}")
        if labels.numel() != codes.kdim * codes.ncols:
            raise ValueError(f"{labels.numel()} indices for a {codes.kdim} x {codes.ncols} weight matrix")
        self._take_codes(codes)
        self._init_centres(labels.reshape(-1), centers, codes.ncols, bias, bias_codes, activation)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(self._linear(x, self.codes, self.centers, bias=self.current_bias(), relu=self._fused_relu))

    def nbytes(self) -> int:
        return self._nbytes(self.packed)


class _SparseCodebookLayer(_SparseForm, _CodesLayer):
    """The indices in the bitmap-sparse form (ops.SparseCodes: its buffer is the module's ``packed`` buffer), centers float32[K],
    bias float32[ncols] or None.  No kdim * ncols tensor stays resident.  ``half_inputs=True`` lets the layer run on bfloat16 /
    float16 inputs (ops.sparse_codebook_matmul -> nnc_cbsp_h16): the path is chosen by the input's dtype and the
    output has that dtype; centers and bias stay float32.  Without it a half input raises TypeError, as it always did."""

    def __init__(self, codes, centers: torch.Tensor, bias: torch.Tensor | None, activation=None, half_inputs: bool = False):
        super().__init__(codes, centers, bias, activation)
        self.half_inputs = bool(half_inputs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        if not self.half_inputs and x.dtype in (torch.bfloat16, torch.float16):
            raise TypeError(f"{type(self).__name__} takes float32 activations, got {x.dtype}: bfloat16 and float16 inputs run on the byte form "
                            "(CompressedDense / CompressedConv2D), and on a bitmap-sparse inference layer only when it is built with "
                            "half_inputs=True")
        return super()._matmul(x)


class SparseCompressedDense(_DenseHalf, _SparseCodebookLayer):
    """Dense run from its codebook and the bitmap-sparse form of its (in, out) indices."""

    @classmethod
    def from_dense(cls, dense, weight_model, bias_model=None, zero_symbol=None, half_inputs: bool = False) -> "SparseCompressedDense":
        codes = _inference_codes(dense, weight_model, bias_model)
        kin, kout = dense.kernel.shape
        return cls.from_codes(kin, kout, *codes, dense.activation, zero_symbol, half_inputs)

    @classmethod
    def from_codes(cls, kdim, ncols, labels, centers, bias, activation, zero_symbol=None, half_inputs: bool = False) -> "SparseCompressedDense":
        return cls(ops.pack_sparse_codes(labels, kdim, ncols, centers.numel(), zero_symbol), centers, bias, activation, half_inputs)


class SparseCompressedConv2D(_Conv2DHalf, _SparseCodebookLayer):
    """Conv2D (stride 1, NHWC) run from its codebook and the bitmap-sparse form of its indices, packed after the rows were put
    in unfold order (keras_rows_for_unfold); patch chunking and the empty batch as CompressedConv2D."""

    def __init__(self, kernel_size: int, cin: int, pad: int, codes: ops.SparseCodes, centers: torch.Tensor, bias: torch.Tensor | None,
                 activation=None, half_inputs: bool = False):
        _check_conv_rows(codes, kernel_size, cin)
        super().__init__(codes, centers, bias, activation, half_inputs)
        self._set_conv(kernel_size, cin, pad)

    @classmethod
    def from_conv(cls, conv, weight_model, bias_model=None, zero_symbol=None, half_inputs: bool = False) -> "SparseCompressedConv2D":
        codes = _inference_codes(conv, weight_model, bias_model)
        h, cin, cout = _conv_shape(conv)
        return cls.from_codes(h, cin, cout, conv.pad, *codes, conv.activation, zero_symbol, half_inputs)

    @classmethod
    def from_codes(cls, kernel_size, cin, cout, pad, labels, centers, bias, activation, zero_symbol=None,
                   half_inputs: bool = False) -> "SparseCompressedConv2D":
        """labels in the Keras order of the (h, w, in, out) kernel."""
        codes = _unfold_then_pack(ops.pack_sparse_codes, kernel_size, cin, cout, labels, centers.numel(), zero_symbol)
        return cls(kernel_size, cin, pad, codes, centers, bias, activation, half_inputs)


class _TrainableSparseCodebookLayer(_SparseForm, _TrainableCodesLayer):
    """The indices in the bitmap-sparse form (the ``packed`` buffer, as _SparseCodebookLayer) with the centres, counts and bias of
    _TrainableCentres; the forward goes through ops.sparse_codebook_linear, whose backward forms dx and the centroid gradient
    from the packed form (csrc/nnc_cbspgrad.hip).  ``counts`` is taken from the labels before packing, so kernel_sq_sum() is the
    dense trainable layer's bit for bit.  No kdim * ncols tensor stays resident.  ``half_inputs=True`` lets the layer train on
    bfloat16 / float16 inputs (ops.sparse_codebook_linear -> nnc_cbsp_h16 and csrc/nnc_cbspgrad_h16.hip): the
    output and the input gradient have the input's dtype, centres and bias stay float32 parameters with float32 gradients.  Without
    it a half input raises ``TypeError``, as it always did."""

    def __init__(self, codes, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None = None, bias_codes=None, activation=None,
                 half_inputs: bool = False):
        super().__init__(codes, labels, centers, bias, bias_codes, activation)
        self.half_inputs = bool(half_inputs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        if not self.half_inputs and x.dtype in (torch.bfloat16, torch.float16):
            raise TypeError(f"{type(self).__name__} takes float32 activations, got {x.dtype}: bfloat16 and float16 inputs train on the byte form "
                            "(TrainableCompressedDense / TrainableCompressedConv2D built with half_inputs=True), and on a bitmap-sparse "
                            "trainable layer only when it is built with half_inputs=True")
        return super()._matmul(x)


class TrainableSparseCompressedDense(_DenseHalf, _TrainableSparseCodebookLayer):
    """SparseCompressedDense with trainable centres (ops.sparse_codebook_linear)."""

    @classmethod
    def from_dense(cls, dense, weight_model, bias_model=None, zero_symbol=None, half_inputs: bool = False) -> "TrainableSparseCompressedDense":
        labels, centers, bias, bias_codes = _trainable_codes(dense, weight_model, bias_model)
        kin, kout = dense.kernel.shape
        return cls(ops.pack_sparse_codes(labels, kin, kout, centers.numel(), zero_symbol), labels, centers, bias, bias_codes, dense.activation,
                   half_inputs)

    @classmethod
    def from_codes(cls, kdim, ncols, labels, centers, bias=None, bias_codes=None, activation=None,
                   zero_symbol=None) -> "TrainableSparseCompressedDense":
        return cls(ops.pack_sparse_codes(labels, kdim, ncols, centers.numel(), zero_symbol), labels, centers, bias, bias_codes, activation)


class TrainableSparseCompressedConv2D(_Conv2DHalf, _TrainableSparseCodebookLayer):
    """SparseCompressedConv2D with trainable centres: the patches (chunked as CompressedConv2D) through
    ops.sparse_codebook_linear; autograd carries the patch gradients back through the unfold."""

    def __init__(self, kernel_size: int, cin: int, pad: int, codes: ops.SparseCodes, labels: torch.Tensor, centers: torch.Tensor, bias=None,
                 bias_codes=None, activation=None, half_inputs: bool = False):
        _check_conv_rows(codes, kernel_size, cin)
        super().__init__(codes, labels, centers, bias, bias_codes, activation, half_inputs)
        self._set_conv(kernel_size, cin, pad)

    @classmethod
    def from_conv(cls, conv, weight_model, bias_model=None, zero_symbol=None, half_inputs: bool = False) -> "TrainableSparseCompressedConv2D":
        h, cin, cout = _conv_shape(conv)
        labels, centers, bias, bias_codes = _trainable_codes(conv, weight_model, bias_model)
        codes = _unfold_then_pack(ops.pack_sparse_codes, h, cin, cout, labels, centers.numel(), zero_symbol)
        return cls(h, cin, conv.pad, codes, labels, centers, bias, bias_codes, conv.activation, half_inputs)

    @classmethod
    def from_codes(cls, kernel_size, cin, cout, pad, labels, centers, bias=None, bias_codes=None, activation=None,
                   zero_symbol=None) -> "TrainableSparseCompressedConv2D":
        """labels in the Keras order of the (h, w, in, out) kernel (the counts are the same in either order)."""
        codes = _unfold_then_pack(ops.pack_sparse_codes, kernel_size, cin, cout, labels, centers.numel(), zero_symbol)
        return cls(kernel_size, cin, pad, codes, labels, centers, bias, bias_codes, activation)


class _PackedCodebookLayer(_PackedForm, _CodesLayer):
    """The indices in the 2- or 4-bit packed form (ops.PackedCodes: its buffer is the module's ``packed`` buffer), centers
    float32[K <= 2^bits], bias float32[ncols] or None.  No kdim * ncols tensor stays resident.  ``half_inputs=True`` lets the layer run
    on bfloat16 / float16 inputs (ops.packed_codebook_matmul -> nnc_cbpk_h16): the path is chosen by the input's
    dtype and the output has that dtype; centers and bias stay float32.  Without it a half input raises TypeError, as it always did."""

    def __init__(self, codes, centers: torch.Tensor, bias: torch.Tensor | None, activation=None, half_inputs: bool = False):
        super().__init__(codes, centers, bias, activation)
        self.half_inputs = bool(half_inputs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        if not self.half_inputs:
            ops._require_f32_x(x, type(self).__name__)
        return super()._matmul(x)


class PackedCompressedDense(_DenseHalf, _PackedCodebookLayer):
    """Dense run from its codebook and the 2- or 4-bit packed form of its (in, out) indices."""

    @classmethod
    def from_dense(cls, dense, weight_model, bias_model=None, bits=None, half_inputs: bool = False) -> "PackedCompressedDense":
        codes = _inference_codes(dense, weight_model, bias_model)
        kin, kout = dense.kernel.shape
        return cls.from_codes(kin, kout, *codes, dense.activation, bits, half_inputs)

    @classmethod
    def from_codes(cls, kdim, ncols, labels, centers, bias, activation, bits=None, half_inputs: bool = False) -> "PackedCompressedDense":
        return cls(ops.pack_codes(labels, kdim, ncols, centers.numel(), bits), centers, bias, activation, half_inputs)


class PackedCompressedConv2D(_Conv2DHalf, _PackedCodebookLayer):
    """Conv2D (stride 1, NHWC) run from its codebook and the packed form of its indices, packed after the rows were put in
    unfold order (keras_rows_for_unfold); patch chunking and the empty batch as CompressedConv2D."""

    def __init__(self, kernel_size: int, cin: int, pad: int, codes: ops.PackedCodes, centers: torch.Tensor, bias: torch.Tensor | None,
                 activation=None, half_inputs: bool = False):
        _check_conv_rows(codes, kernel_size, cin)
        super().__init__(codes, centers, bias, activation, half_inputs)
        self._set_conv(kernel_size, cin, pad)

    @classmethod
    def from_conv(cls, conv, weight_model, bias_model=None, bits=None, half_inputs: bool = False) -> "PackedCompressedConv2D":
        codes = _inference_codes(conv, weight_model, bias_model)
        h, cin, cout = _conv_shape(conv)
        return cls.from_codes(h, cin, cout, conv.pad, *codes, conv.activation, bits, half_inputs)

    @classmethod
    def from_codes(cls, kernel_size, cin, cout, pad, labels, centers, bias, activation, bits=None,
                   half_inputs: bool = False) -> "PackedCompressedConv2D":
        """labels in the Keras order of the (h, w, in, out) kernel."""
        ops.packed_bits(centers.numel(), bits)   # a codebook that does not fit raises before the unfold
        codes = _unfold_then_pack(ops.pack_codes, kernel_size, cin, cout, labels, centers.numel(), bits)
        return cls(kernel_size, cin, pad, codes, centers, bias, activation, half_inputs)


class _TrainablePackedCodebookLayer(_PackedForm, _TrainableCodesLayer):
    """The indices in the 2- or 4-bit packed form (the ``packed`` buffer, as _PackedCodebookLayer) with the centres, counts and bias
    of _TrainableCentres; the forward goes through ops.packed_codebook_linear, whose backward forms dx and the centroid gradient
    from the packed rows (csrc/nnc_cbpkgrad.hip).  ``counts`` is taken from the labels before packing, so kernel_sq_sum() is the
    byte trainable layer's bit for bit.  No kdim * ncols tensor stays resident.  ``half_inputs=True`` lets the layer train on bfloat16 /
    float16 inputs (csrc/nnc_cbpk_h16.hip): the output and the input gradient have the input's dtype; the centres,
    the bias and their gradients stay float32.  Without it a half input raises TypeError, as it always did."""

    def __init__(self, codes, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None = None, bias_codes=None, activation=None,
                 half_inputs: bool = False):
        super().__init__(codes, labels, centers, bias, bias_codes, activation)
        self.half_inputs = bool(half_inputs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        if not self.half_inputs:
            ops._require_f32_x(x, type(self).__name__)
        return super()._matmul(x)


class TrainablePackedCompressedDense(_DenseHalf, _TrainablePackedCodebookLayer):
    """PackedCompressedDense with trainable centres (ops.packed_codebook_linear)."""

    @classmethod
    def from_dense(cls, dense, weight_model, bias_model=None, bits=None, half_inputs: bool = False) -> "TrainablePackedCompressedDense":
        codes = _trainable_codes(dense, weight_model, bias_model)
        kin, kout = dense.kernel.shape
        return cls.from_codes(kin, kout, *codes, dense.activation, bits, half_inputs)

    @classmethod
    def from_codes(cls, kdim, ncols, labels, centers, bias=None, bias_codes=None, activation=None, bits=None,
                   half_inputs: bool = False) -> "TrainablePackedCompressedDense":
        return cls(ops.pack_codes(labels, kdim, ncols, centers.numel(), bits), labels, centers, bias, bias_codes, activation, half_inputs)


class TrainablePackedCompressedConv2D(_Conv2DHalf, _TrainablePackedCodebookLayer):
    """PackedCompressedConv2D with trainable centres: the patches (chunked as CompressedConv2D) through
    ops.packed_codebook_linear; autograd carries the patch gradients back through the unfold."""

    def __init__(self, kernel_size: int, cin: int, pad: int, codes: ops.PackedCodes, labels: torch.Tensor, centers: torch.Tensor, bias=None,
                 bias_codes=None, activation=None, half_inputs: bool = False):
        _check_conv_rows(codes, kernel_size, cin)
        super().__init__(codes, labels, centers, bias, bias_codes, activation, half_inputs)
        self._set_conv(kernel_size, cin, pad)

    @classmethod
    def from_conv(cls, conv, weight_model, bias_model=None, bits=None, half_inputs: bool = False) -> "TrainablePackedCompressedConv2D":
        h, cin, cout = _conv_shape(conv)
        return cls.from_codes(h, cin, cout, conv.pad, *_trainable_codes(conv, weight_model, bias_model), conv.activation, bits, half_inputs)

    @classmethod
    def from_codes(cls, kernel_size, cin, cout, pad, labels, centers, bias=None, bias_codes=None, activation=None,
                   bits=None, half_inputs: bool = False) -> "TrainablePackedCompressedConv2D":
        """labels in the Keras order of the (h, w, in, out) kernel (the counts are the same in either order)."""
        ops.packed_bits(centers.numel(), bits)   # a codebook that does not fit raises before the unfold
        codes = _unfold_then_pack(ops.pack_codes, kernel_size, cin, cout, labels, centers.numel(), bits)
        return cls(kernel_size, cin, pad, codes, labels, centers, bias, bias_codes, activation, half_inputs)


class GroupedPackedCompressedDense(_DenseHalf, _PackedForm, _InferenceLayer):
    """Dense run from one codebook per block of ``group_rows`` input rows and the 2- or 4-bit packed form of its (in, out) indices
    (ops.grouped_packed_codebook_matmul): packed (the ordinary packed buffer of the whole index matrix),
    centers float32 (G, K <= 2^bits), G = ceil(kdim / group_rows), bias float32[ncols] or None.  The path follows the input's
    dtype as in GroupedCompressedDense (float32, bfloat16, float16; the output has the input's dtype); centers and bias stay
    float32.  No kdim * ncols tensor stays resident."""

    def __init__(self, codes: ops.PackedCodes, group_rows: int, centers: torch.Tensor, bias: torch.Tensor | None, activation=None):
        super().__init__()
        groups = max(1, -(-codes.kdim // int(group_rows)))
        if centers.dim() != 2 or tuple(centers.shape) != (groups, codes.k):
            raise ValueError(f"centers must have shape ({groups}, {codes.k}) for {codes.kdim} rows in groups of {group_rows} and indices into "
                             f"codebooks of {codes.k}, got {tuple(centers.shape)}")
        self._take_codes(codes)
        self.group_rows = int(group_rows)
        self._init_codebook(centers, bias, activation)

    @classmethod
    def from_dense(cls, dense, grouped_model, bias_model=None, bits=None) -> "GroupedPackedCompressedDense":
        """From a Dense layer and the GroupedModel of its kernel (utility.get_quantized_weight_grouped), K <= 16."""
        _require_model(grouped_model)
        kin, kout = dense.kernel.shape
        centers = torch.from_numpy(np.ascontiguousarray(grouped_model.cluster_centers_, dtype=np.float32)).to(dense.kernel.device)
        return cls.from_codes(kin, kout, grouped_model.group_rows, grouped_model.labels_compact_, centers, _decoded_bias(dense.bias, bias_model),
                              dense.activation, bits)

    @classmethod
    def from_codes(cls, kdim, ncols, group_rows, labels, centers, bias, activation, bits=None) -> "GroupedPackedCompressedDense":
        if centers.dim() != 2:
            raise ValueError(f"centers must have shape (G, K), got {tuple(centers.shape)}")
        return cls(ops.pack_codes(labels, kdim, ncols, centers.shape[1], bits), group_rows, centers, bias, activation)

    @classmethod
    def from_grouped(cls, layer: GroupedCompressedDense, bits=None) -> "GroupedPackedCompressedDense":
        """The same layer from the packed form of a GroupedCompressedDense's indices: the same function, bit for bit."""
        return cls.from_codes(layer.kdim, layer.ncols, layer.group_rows, layer.labels, layer.centers, layer.bias, layer.activation, bits)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(ops.grouped_packed_codebook_matmul(x, self.codes, self.centers, self.group_rows, bias=self.bias, relu=self._fused_relu))


class GroupedSparseCompressedDense(_DenseHalf, _InferenceLayer):
    """Dense run from one codebook per block of ``group_rows`` input rows and the bitmap-sparse form of its (in, out) indices
    (ops.grouped_sparse_codebook_matmul): packed (the bitmap-sparse buffer of the whole index matrix, one
    byte per stored symbol), zero_symbols (the skipped index of every group, uint8[G]), centers float32 (G, K), G = ceil(kdim /
    group_rows), bias float32[ncols] or None.  ``half_inputs=True`` lets the layer run on bfloat16 / float16 inputs
    (ops.grouped_sparse_codebook_matmul -> nnc_cbsp_grouped_h16): the path is chosen by the input's dtype and
    the output has that dtype; centers and bias stay float32.  Without it a half input raises TypeError, as it always did.  Inference
    only.  No kdim * ncols tensor stays resident."""

    _INDEX = "packed"

    def __init__(self, codes: ops.GroupedSparseCodes, centers: torch.Tensor, bias: torch.Tensor | None, activation=None, half_inputs: bool = False):
        super().__init__()
        self.half_inputs = bool(half_inputs)
        groups = max(1, codes.groups)
        if centers.dim() != 2 or tuple(centers.shape) != (groups, codes.k):
            raise ValueError(f"centers must have shape ({groups}, {codes.k}) for {codes.kdim} rows in groups of {codes.group_rows} and indices into "
                             f"codebooks of {codes.k}, got {tuple(centers.shape)}")
        self.kdim, self.ncols, self.k, self.group_rows, self.nnz = codes.kdim, codes.ncols, codes.k, codes.group_rows, codes.nnz
        self.register_buffer("packed", codes.buf)
        self.register_buffer("zero_symbols", codes.zero_symbols)
        self._init_codebook(centers, bias, activation)

    @property
    def codes(self) -> ops.GroupedSparseCodes:
        return ops.GroupedSparseCodes(self.packed, self.kdim, self.ncols, self.k, self.group_rows, self.zero_symbols, self.nnz)

    @classmethod
    def from_dense(cls, dense, grouped_model, bias_model=None, zero_symbols=None, half_inputs: bool = False) -> "GroupedSparseCompressedDense":
        """From a Dense layer and the GroupedModel of its kernel (utility.get_quantized_weight_grouped)."""
        _require_model(grouped_model)
        kin, kout = dense.kernel.shape
        centers = torch.from_numpy(np.ascontiguousarray(grouped_model.cluster_centers_, dtype=np.float32)).to(dense.kernel.device)
        return cls.from_codes(kin, kout, grouped_model.group_rows, grouped_model.labels_compact_, centers, _decoded_bias(dense.bias, bias_model),
                              dense.activation, zero_symbols, half_inputs)

    @classmethod
    def from_codes(cls, kdim, ncols, group_rows, labels, centers, bias, activation, zero_symbols=None,
                   half_inputs: bool = False) -> "GroupedSparseCompressedDense":
        if centers.dim() != 2:
            raise ValueError(f"centers must have shape (G, K), got {tuple(centers.shape)}")
        return cls(ops.pack_grouped_sparse_codes(labels, kdim, ncols, centers.shape[1], group_rows, zero_symbols), centers, bias, activation,
                   half_inputs)

    @classmethod
    def from_grouped(cls, layer: GroupedCompressedDense, zero_symbols=None, half_inputs: bool = False) -> "GroupedSparseCompressedDense":
        """The same layer from the bitmap-sparse form of a GroupedCompressedDense's indices: the same weights, the sums in the
        order of DESIGN.md section 28."""
        return cls.from_codes(layer.kdim, layer.ncols, layer.group_rows, layer.labels, layer.centers, layer.bias, layer.activation, zero_symbols,
                              half_inputs)

    def nbytes(self) -> int:
        """The buffer, the G skipped symbols, the G * K centres and the bias."""
        return super().nbytes() + _tensor_bytes(self.zero_symbols)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(ops.grouped_sparse_codebook_matmul(x, self.codes, self.centers, bias=self.bias, relu=self._fused_relu,
                                                                 half_inputs=self.half_inputs))


class TrainableGroupedPackedCompressedDense(_DenseHalf, _PackedForm, _TrainableCentres):
    """GroupedPackedCompressedDense with trainable centres (ops.grouped_packed_codebook_linear): packed (the
    ordinary 2- or 4-bit packed buffer of the whole index matrix) the only index buffer, centers a float32 (G, K <= 2^bits)
    nn.Parameter, counts the (G, K) histogram of every group's indices taken from the labels before packing, so kernel_sq_sum() is
    TrainableGroupedCompressedDense's bit for bit; the bias of _TrainableCentres.  The backward forms dx and the (G, K) centroid
    gradient from the codebooks and the packed rows (csrc/nnc_cbpkgrad_grouped.hip): the indices are never unpacked, W and dW never
    built, and no byte-per-weight tensor stays resident while training.  ``half_inputs=True`` lets the layer train on bfloat16 /
    float16 inputs (csrc/nnc_cbpkgrad_grouped_h16.hip), as TrainableGroupedCompressedDense; without it a half
    input raises ``TypeError``."""

    def __init__(self, codes: ops.PackedCodes, group_rows: int, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None = None,
                 bias_codes=None, activation=None, half_inputs: bool = False):
        super().__init__()
        self.half_inputs = bool(half_inputs)
        groups = max(1, -(-codes.kdim // int(group_rows)))
        if centers.dim() != 2 or tuple(centers.shape) != (groups, codes.k):
            raise ValueError(f"centers must have shape ({groups}, {codes.k}) for {codes.kdim} rows in groups of {group_rows} and indices into "
                             f"codebooks of {codes.k}, got {tuple(centers.shape)}")
        if labels.numel() != codes.kdim * codes.ncols:
            raise ValueError(f"{labels.numel()} indices for a {codes.kdim} x {codes.ncols} weight matrix")
        self._take_codes(codes)
        self.group_rows = int(group_rows)
        counts = _group_counts(labels.reshape(-1), self.group_rows * self.ncols, groups, codes.k)
        self._init_centres(None, centers, codes.ncols, bias, bias_codes, activation, counts=counts)

    @classmethod
    def from_dense(cls, dense, grouped_model, bias_model=None, bits=None, half_inputs: bool = False) -> "TrainableGroupedPackedCompressedDense":
        """From a Dense layer and the GroupedModel of its kernel, K <= 16; a quantized bias keeps its codes, a raw one stays frozen."""
        _require_model(grouped_model)
        kin, kout = dense.kernel.shape
        dev = dense.kernel.device
        centers = torch.from_numpy(np.ascontiguousarray(grouped_model.cluster_centers_, dtype=np.float32)).to(dev)
        bias, bias_codes = (None, _codes(bias_model, dev)) if bias_model is not None else (dense.bias, None)
        return cls.from_codes(kin, kout, grouped_model.group_rows, grouped_model.labels_compact_, centers, bias, bias_codes, dense.activation, bits,
                              half_inputs)

    @classmethod
    def from_codes(cls, kdim, ncols, group_rows, labels, centers, bias=None, bias_codes=None, activation=None,
                   bits=None, half_inputs: bool = False) -> "TrainableGroupedPackedCompressedDense":
        if centers.dim() != 2:
            raise ValueError(f"centers must have shape (G, K), got {tuple(centers.shape)}")
        return cls(ops.pack_codes(labels, kdim, ncols, centers.shape[1], bits), group_rows, labels, centers, bias, bias_codes, activation, half_inputs)

    @classmethod
    def from_grouped(cls, layer: GroupedCompressedDense, bits=None, half_inputs: bool = False) -> "TrainableGroupedPackedCompressedDense":
        """The trainable packed layer of a GroupedCompressedDense: its indices packed, the same centres, its decoded bias frozen."""
        return cls.from_codes(layer.kdim, layer.ncols, layer.group_rows, layer.labels, layer.centers, layer.bias, None, layer.activation, bits,
                              half_inputs)

    @classmethod
    def from_grouped_packed(cls, layer: GroupedPackedCompressedDense, half_inputs: bool = False) -> "TrainableGroupedPackedCompressedDense":
        """The trainable layer of a GroupedPackedCompressedDense on the same packed buffer; the counts come from a temporary unpack
        (nnc_cbpk_unpack), which is dropped afterwards."""
        return cls(layer.codes, layer.group_rows, layer.codes.to_dense(), layer.centers, layer.bias, None, layer.activation, half_inputs)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(ops.grouped_packed_codebook_linear(x, self.codes, self.centers, self.group_rows, bias=self.current_bias(),
                                                                 relu=self._fused_relu, half_inputs=self.half_inputs))

    def nbytes(self) -> int:
        return self._nbytes(self.packed)


class TrainableGroupedSparseCompressedDense(_DenseHalf, _TrainableCentres):
    """GroupedSparseCompressedDense with trainable centres (ops.grouped_sparse_codebook_linear): packed (the
    bitmap-sparse buffer of the whole index matrix) and zero_symbols (uint8[G]) the only index buffers, centers a float32 (G, K)
    nn.Parameter, counts the (G, K) histogram of every group's indices taken from the labels before packing, so kernel_sq_sum() is
    TrainableGroupedCompressedDense's bit for bit; the bias of _TrainableCentres.  The backward forms dx and the (G, K) centroid
    gradient from the codebooks and the bitmap-sparse form (csrc/nnc_cbspgrad_grouped.hip): the indices are never unpacked, W and dW
    never built, and no byte-per-weight tensor stays resident while training.  float32 activations only: a bfloat16 or float16 input
    raises ``TypeError``."""

    def __init__(self, codes: ops.GroupedSparseCodes, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None = None,
                 bias_codes=None, activation=None):
        super().__init__()
        groups = max(1, codes.groups)
        if centers.dim() != 2 or tuple(centers.shape) != (groups, codes.k):
            raise ValueError(f"centers must have shape ({groups}, {codes.k}) for {codes.kdim} rows in groups of {codes.group_rows} and indices into "
                             f"codebooks of {codes.k}, got {tuple(centers.shape)}")
        if labels.numel() != codes.kdim * codes.ncols:
            raise ValueError(f"{labels.numel()} indices for a {codes.kdim} x {codes.ncols} weight matrix")
        self.kdim, self.ncols, self.k, self.group_rows, self.nnz = codes.kdim, codes.ncols, codes.k, codes.group_rows, codes.nnz
        self.register_buffer("packed", codes.buf)
        self.register_buffer("zero_symbols", codes.zero_symbols)
        counts = _group_counts(labels.reshape(-1), self.group_rows * self.ncols, groups, codes.k)
        self._init_centres(None, centers, codes.ncols, bias, bias_codes, activation, counts=counts)

    @property
    def codes(self) -> ops.GroupedSparseCodes:
        return ops.GroupedSparseCodes(self.packed, self.kdim, self.ncols, self.k, self.group_rows, self.zero_symbols, self.nnz)

    @classmethod
    def from_dense(cls, dense, grouped_model, bias_model=None, zero_symbols=None) -> "TrainableGroupedSparseCompressedDense":
        """From a Dense layer and the GroupedModel of its kernel; a quantized bias keeps its codes, a raw one stays frozen."""
        _require_model(grouped_model)
        kin, kout = dense.kernel.shape
        dev = dense.kernel.device
        centers = torch.from_numpy(np.ascontiguousarray(grouped_model.cluster_centers_, dtype=np.float32)).to(dev)
        bias, bias_codes = (None, _codes(bias_model, dev)) if bias_model is not None else (dense.bias, None)
        return cls.from_codes(kin, kout, grouped_model.group_rows, grouped_model.labels_compact_, centers, bias, bias_codes, dense.activation,
                              zero_symbols)

    @classmethod
    def from_codes(cls, kdim, ncols, group_rows, labels, centers, bias=None, bias_codes=None, activation=None,
                   zero_symbols=None) -> "TrainableGroupedSparseCompressedDense":
        if centers.dim() != 2:
            raise ValueError(f"centers must have shape (G, K), got {tuple(centers.shape)}")
        return cls(ops.pack_grouped_sparse_codes(labels, kdim, ncols, centers.shape[1], group_rows, zero_symbols), labels, centers, bias, bias_codes,
                   activation)

    @classmethod
    def from_grouped(cls, layer: GroupedCompressedDense, zero_symbols=None) -> "TrainableGroupedSparseCompressedDense":
        """The trainable sparse layer of a GroupedCompressedDense: its indices packed, the same centres, its decoded bias frozen."""
        return cls.from_codes(layer.kdim, layer.ncols, layer.group_rows, layer.labels, layer.centers, layer.bias, None, layer.activation, zero_symbols)

    @classmethod
    def from_grouped_sparse(cls, layer: GroupedSparseCompressedDense) -> "TrainableGroupedSparseCompressedDense":
        """The trainable layer of a GroupedSparseCompressedDense on the same buffer; the counts come from a temporary unpack
        (nnc_cbsp_grouped_unpack), which is dropped afterwards."""
        return cls(layer.codes, layer.codes.to_dense(), layer.centers, layer.bias, None, layer.activation)

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        return self._activate(ops.grouped_sparse_codebook_linear(x, self.codes, self.centers, bias=self.current_bias(), relu=self._fused_relu))

    def nbytes(self) -> int:
        """The buffer, the G skipped symbols, the G * K centres and the bias."""
        return self._nbytes(self.packed) + _tensor_bytes(self.zero_symbols)


PACKED_MAX_K = 16   # the packed form holds at most 4-bit indices


def _check_packed(packed, sparse=False, trainable=False):
    if packed not in (False, True, "auto"):
        raise ValueError(f"packed must be False, True or 'auto', got {packed!r}")
    if packed is True and sparse is True:
        raise ValueError("sparse=True and packed=True both ask for every layer: take one, or 'auto' for either")
    if trainable and packed is not False:
        raise ValueError("trainable=True needs packed=False here: the packed layers of compress_network are inference only; use "
                         "compress_network_trainable(..., packed=...) for trainable 2- and 4-bit packed layers")


def _check_sparse(sparse):
    if sparse not in (False, True, "auto"):
        raise ValueError(f"sparse must be False, True or 'auto', got {sparse!r}")


def _pick(dense_layer, make_sparse, sparse):
    """The dense form, the sparse one, or (``"auto"``) whichever holds fewer resident bytes."""
    if sparse is False:
        return dense_layer()
    sp = make_sparse()
    if sparse is True:
        return sp
    de = dense_layer()
    return sp if sp.nbytes() < de.nbytes() else de


def _pick3(k, make_byte, make_sparse, make_packed, sparse, packed):
    """The candidates in the order byte form (unless ``sparse is True``, or ``packed is True`` and K <= 16), bitmap-sparse form (if
    ``sparse`` is not False), packed form (if ``packed`` is not False and K <= 16); the one with the fewest resident bytes, on
    equal bytes the earliest."""
    fits = k <= PACKED_MAX_K
    makers = []
    if sparse is not True and not (packed is True and fits):
        makers.append(make_byte)
    if sparse is not False:
        makers.append(make_sparse)
    if packed is not False and fits:
        makers.append(make_packed)
    best = None
    for make in makers:
        cand = make()
        if best is None or cand.nbytes() < best.nbytes():
            best = cand
    return best


def _from_codes(layer, shape, labels, centers, bias, sparse, packed=False, sparse_half_inputs=False, packed_half_inputs=False):
    from .neural_networks.layers import Conv2D, Dense

    half = dict(half_inputs=True) if sparse_half_inputs else {}
    pk_half = dict(half_inputs=True) if packed_half_inputs else {}
    if isinstance(layer, Dense):
        args = (shape[0], shape[1], labels, centers, bias, layer.activation)
        make_byte, make_sparse, make_packed = (lambda: CompressedDense(*args), lambda: SparseCompressedDense.from_codes(*args, **half),
                                               lambda: PackedCompressedDense.from_codes(*args, **pk_half))
    elif isinstance(layer, Conv2D):
        args = (shape[0], shape[2], shape[3], layer.pad, labels, centers, bias, layer.activation)
        make_byte, make_sparse, make_packed = (lambda: CompressedConv2D.from_codes(*args), lambda: SparseCompressedConv2D.from_codes(*args, **half),
                                               lambda: PackedCompressedConv2D.from_codes(*args, **pk_half))
    else:
        raise TypeError(f"no compressed form of {type(layer).__name__}")
    if packed is False:
        return _pick(make_byte, make_sparse, sparse)
    return _pick3(centers.numel(), make_byte, make_sparse, make_packed, sparse, packed)


def _replace(layer, weight_model, bias_model, sparse=False, packed=False, sparse_half_inputs=False, packed_half_inputs=False):
    from .neural_networks.layers import Conv2D, Dense

    if sparse is False and packed is False:
        if isinstance(layer, Dense):
            return CompressedDense.from_dense(layer, weight_model, bias_model)
        if isinstance(layer, Conv2D):
            return CompressedConv2D.from_conv(layer, weight_model, bias_model)
        raise TypeError(f"no compressed form of {type(layer).__name__}")
    if not isinstance(layer, (Dense, Conv2D)):
        raise TypeError(f"no compressed form of {type(layer).__name__}")
    centers, labels = _codes(weight_model, layer.kernel.device)
    return _from_codes(layer, tuple(layer.kernel.shape), labels, centers, _decoded_bias(layer.bias, bias_model), sparse, packed, sparse_half_inputs,
                       packed_half_inputs)


def _check_half_inputs(half_inputs, sparse, packed, trainable=True):
    if not half_inputs:
        return
    if not trainable:
        raise ValueError("half_inputs=True is an option of the trainable layers (trainable=True): the inference layers of the byte form "
                         "take bfloat16 and float16 inputs as they are")
    if sparse is not False or packed is not False:
        raise ValueError("half_inputs=True needs sparse=False and packed=False: only the byte form trains on bfloat16 / float16 inputs")


def _check_sparse_half_inputs(sparse_half_inputs, sparse, trainable=False):
    if not sparse_half_inputs:
        return
    if trainable:
        raise ValueError("sparse_half_inputs=True builds the bitmap-sparse inference layers here: it needs trainable=False "
                         "(compress_network_trainable(..., sparse=..., sparse_half_inputs=True) builds the trainable sparse layers "
                         "that train on bfloat16 / float16 inputs)")
    if sparse is False:
        raise ValueError("sparse_half_inputs=True needs sparse=True or sparse='auto': it builds the bitmap-sparse layers with "
                         "half_inputs=True (the byte form takes bfloat16 and float16 inputs as it is)")


def _check_packed_half_inputs(packed_half_inputs, sparse, packed, sparse_half_inputs, trainable=False):
    if not packed_half_inputs:
        return
    if trainable:
        raise ValueError("packed_half_inputs=True builds the packed inference layers here: it needs trainable=False "
                         "(compress_network_trainable(..., packed=..., packed_half_inputs=True) builds the trainable packed layers "
                         "that train on bfloat16 / float16 inputs)")
    if packed is False:
        raise ValueError("packed_half_inputs=True needs packed=True or packed='auto': it builds the 2- / 4-bit packed layers with "
                         "half_inputs=True")
    if sparse is not False and not sparse_half_inputs:
        raise ValueError("packed_half_inputs=True with sparse=True or sparse='auto' needs sparse_half_inputs=True too: a layer that "
                         "'auto' gives to the bitmap-sparse form would refuse the bfloat16 / float16 input")


def compress_network(network: nn.Module, models_by_layer, sparse=False, trainable=False, packed=False, half_inputs=False,
                     sparse_half_inputs=False, packed_half_inputs=False) -> nn.Module:
    """A deep copy of ``network`` whose quantized layers (``models_by_layer``: layer -> [kernel model, bias model], as
    Trainer.quantized_models_by_layer) run from their codebooks.  Layers are replaced by the attribute names of
    ``get_config()``; a layer whose kernel passed through unquantized (model None) stays float32.  ``sparse``: False (the
    indices as they are), True (the bitmap-sparse form, skipping the most frequent index), "auto" (per layer, the smaller).
    ``packed``: False, True (2- or 4-bit packed indices for every layer of at most 16 centres, the others in the byte form) or
    "auto"; with ``sparse`` it decides per layer by resident bytes as the module's docstring tells.
    ``trainable=True`` (dense indices only): TrainableCompressedDense / TrainableCompressedConv2D, centres as parameters;
    compress_network_trainable gives the bitmap-sparse and the packed trainable layers too.  ``half_inputs=True`` (with
    trainable=True, sparse=False and packed=False only, else ValueError): those layers train on bfloat16 / float16 inputs too.
    ``sparse_half_inputs=True`` (with ``sparse`` True or "auto" and trainable=False only, else ValueError): the bitmap-sparse layers are
    built with half_inputs=True and run on bfloat16 / float16 inputs; layers that "auto" leaves in the byte form
    take them anyway, and what "auto" picks does not change.
    ``packed_half_inputs=True`` (with ``packed`` True or "auto" and trainable=False only, and with ``sparse`` other than False only
    together with sparse_half_inputs=True, else ValueError): the packed layers are built with half_inputs=True and run on bfloat16 /
    float16 inputs; what "auto" picks does not change.
    A layer whose kernel model is a utility.GroupedModel (one codebook per block of input rows) becomes a GroupedCompressedDense;
    with ``sparse``, ``packed`` or ``trainable`` set it raises NotImplementedError and names the layer (pack_grouped_layers packs
    the grouped layers of the result, sparsify_grouped_layers gives them the bitmap-sparse form, smallest_grouped_layers the
    smallest of the three)."""
    _check_sparse(sparse)
    _check_packed(packed, sparse, trainable)
    _check_half_inputs(half_inputs, sparse, packed, trainable)
    _check_sparse_half_inputs(sparse_half_inputs, sparse, trainable)
    _check_packed_half_inputs(packed_half_inputs, sparse, packed, sparse_half_inputs, trainable)
    if trainable and sparse is not False:
        raise ValueError("trainable=True needs sparse=False here: use compress_network_trainable(..., sparse=...) for trainable "
                         "bitmap-sparse layers")
    if trainable:
        return compress_network_trainable(network, models_by_layer, half_inputs=half_inputs)
    what = "sparse=" + repr(sparse) if sparse is not False else ("packed=" + repr(packed) if packed is not False else None)
    return _compress_each(network, models_by_layer, lambda layer, wm, bm: _replace(layer, wm, bm, sparse, packed, sparse_half_inputs, packed_half_inputs),
                          grouped=what)


def compress_network_trainable(network: nn.Module, models_by_layer, sparse=False, packed=False, half_inputs=False,
                               sparse_half_inputs=False, packed_half_inputs=False) -> nn.Module:
    """compress_network with the centres (and quantized biases' centres) as nn.Parameters.  ``sparse``: False
    (TrainableCompressedDense / TrainableCompressedConv2D, the layers of compress_network(..., trainable=True)), True
    (TrainableSparseCompressedDense / TrainableSparseCompressedConv2D: the indices in the bitmap-sparse form, skipping the most
    frequent one) or "auto" (per layer, the form with fewer resident bytes).  ``packed``: False, True
    (TrainablePackedCompressedDense / TrainablePackedCompressedConv2D for every layer of at most 16 centres, the others in the
    byte form) or "auto"; with ``sparse`` it decides per layer by resident bytes as the module's docstring tells.  All train the
    same function: the sparse and the packed layer's centroid gradient is the byte one's bit for bit (DESIGN.md sections 13, 15).
    ``half_inputs=True`` (sparse=False and packed=False only, else ValueError): the byte layers built with half_inputs=True, which
    train on bfloat16 / float16 inputs.
    ``sparse_half_inputs=True`` (``sparse`` True or "auto" and packed=False only, else ValueError): the bitmap-sparse layers are built
    with half_inputs=True and train on bfloat16 / float16 inputs; the layers "auto" leaves in the byte form are
    built with it too, so the whole network trains on half inputs, and what "auto" picks does not change.
    ``packed_half_inputs=True`` (``packed`` True or "auto" only, and with ``sparse`` other than False only together with
    sparse_half_inputs=True, else ValueError): the packed layers are built with half_inputs=True and train on bfloat16 / float16 inputs
    (DESIGN.md section 25); the layers left in the byte form are built with it too, and what "auto" picks does not change."""
    _check_packed_half_inputs(packed_half_inputs, sparse, packed, sparse_half_inputs)
    if sparse_half_inputs and (sparse is False or (packed is not False and not packed_half_inputs)):
        raise ValueError("sparse_half_inputs=True needs sparse=True or sparse='auto', and packed=False: it builds the trainable "
                         "bitmap-sparse layers with half_inputs=True (half_inputs=True builds the byte form's; the packed layers "
                         "take float32 activations)")
    _check_sparse(sparse)
    _check_packed(packed, sparse)
    _check_half_inputs(half_inputs, sparse, packed)
    half = bool(half_inputs or sparse_half_inputs or packed_half_inputs)

    def make(layer, wm, bm):
        byte, sp, pk = (lambda: _trainable(layer, wm, bm, half_inputs=half),
                        lambda: _trainable(layer, wm, bm, TrainableSparseCompressedDense, TrainableSparseCompressedConv2D,
                                           half_inputs=bool(sparse_half_inputs)),
                        lambda: _trainable(layer, wm, bm, TrainablePackedCompressedDense, TrainablePackedCompressedConv2D,
                                           half_inputs=bool(packed_half_inputs)))
        return _pick(byte, sp, sparse) if packed is False else _pick3(wm.cluster_centers_.size, byte, sp, pk, sparse, packed)

    return _compress_each(network, models_by_layer, make, grouped="trainable=True")


def _grouped_trainable_pick(layer, wm, bm, sparse, packed):
    """The trainable grouped layer of compress_network_trainable_grouped(sparse=, packed=) with ``sparse`` not False: the candidates in
    the order byte form (unless ``sparse is True``, or ``packed is True`` and K <= 16), packed form (``packed`` not False and K <= 16),
    bitmap-sparse form; the one with the fewest resident bytes, on equal bytes the earliest (smallest_grouped_layers' order).
    The forms differ in their index bytes only (the sparse one also keeps its G skipped symbols), which are known from the labels'
    histograms: only the winner is built."""
    k = wm.cluster_centers_.shape[1]
    fits = k <= PACKED_MAX_K
    kin, kout = layer.kernel.shape
    rows = int(wm.group_rows)
    groups = max(1, -(-kin // rows))
    cands = []   # (index bytes, maker), in the order of the ties
    if sparse is not True and not (packed is True and fits):
        cands.append((kin * kout, TrainableGroupedCompressedDense.from_dense))
    if packed is not False and fits:
        cands.append((ops.packed_nbytes(kin, kout, ops.packed_bits(k)), TrainableGroupedPackedCompressedDense.from_dense))
    counts = _group_counts(wm.labels_compact_.reshape(-1), rows * kout, groups, k)
    nnz = kin * kout - int(counts.max(dim=1).values.sum().item())   # every group skips its most frequent index
    cands.append((int(ops.nat.load().nnc_cbsp_pack_bytes(kin, kout, 1, nnz)) + -(-kin // rows), TrainableGroupedSparseCompressedDense.from_dense))
    return min(cands, key=lambda c: c[0])[1](layer, wm, bm)   # (min keeps the first of equals)


def compress_network_trainable_grouped(network: nn.Module, models_by_layer, packed=False, sparse=False, half_inputs=False) -> nn.Module:
    """compress_network_trainable(network, models_by_layer) -- the byte forms -- in which every layer whose kernel model is a
    utility.GroupedModel becomes a TrainableGroupedCompressedDense instead of raising.  On a network
    without grouped layers it returns what compress_network_trainable returns.  ``packed``: False (the byte grouped layers), True
    (a TrainableGroupedPackedCompressedDense, DESIGN.md section 20, for every grouped layer of at most 16 centres per group) or
    "auto" (that class only where the packed form holds fewer resident bytes; on equal bytes the byte form stays); anything else
    is a ValueError.  Ungrouped layers stay in the byte trainable forms either way.  Trainer.fine_tune_grouped trains it.
    ``half_inputs=True``: the grouped layers of either form and the ungrouped byte-form layers are built with half_inputs=True and
    train on bfloat16 / float16 inputs (DESIGN.md sections 22 and 26).
    ``sparse``: False (as above), True (a TrainableGroupedSparseCompressedDense, DESIGN.md section 32, for every grouped layer) or
    "auto" (that class only where the bitmap-sparse form holds fewer resident bytes than the byte form); anything else is a
    ValueError.  Together with ``packed`` not False a grouped layer takes the smallest of its candidates, on equal bytes in the order
    byte, packed, sparse; ``sparse=True`` with ``packed=True`` is a ValueError (both ask for every layer).  The sparse trainable layer
    takes float32 activations only: ``sparse`` not False with ``half_inputs=True`` is a ValueError."""
    _check_sparse(sparse)
    if packed not in (False, True, "auto"):
        raise ValueError(f"packed must be False, True or 'auto', got {packed!r}")
    if sparse is not False and half_inputs:
        raise ValueError("sparse needs half_inputs=False here: the trainable grouped bitmap-sparse layer takes float32 activations only "
                         "(half_inputs trains the byte and packed grouped forms)")
    if sparse is True and packed is True:
        raise ValueError("sparse=True and packed=True both ask for every layer: take one, or 'auto' for either")
    half = dict(half_inputs=True) if half_inputs else {}
    if sparse is not False:
        def make_grouped(layer, wm, bm):
            return _grouped_trainable_pick(layer, wm, bm, sparse, packed)
    elif packed is False:
        def make_grouped(layer, wm, bm):
            return TrainableGroupedCompressedDense.from_dense(layer, wm, bm, **half)
    elif packed is True or packed == "auto":
        def make_grouped(layer, wm, bm):
            k = wm.cluster_centers_.shape[1]
            kin, kout = layer.kernel.shape
            if k > PACKED_MAX_K or (packed == "auto" and ops.packed_nbytes(kin, kout, ops.packed_bits(k)) >= kin * kout):
                return TrainableGroupedCompressedDense.from_dense(layer, wm, bm, **half)
            return TrainableGroupedPackedCompressedDense.from_dense(layer, wm, bm, **half)
    else:
        raise ValueError(f"packed must be False, True or 'auto', got {packed!r}")
    return _compress_each(network, models_by_layer, lambda layer, wm, bm: _trainable(layer, wm, bm, half_inputs=bool(half_inputs)),
                          make_grouped=make_grouped)


def _compress_each(network: nn.Module, models_by_layer, make, grouped=None, make_grouped=GroupedCompressedDense.from_dense) -> nn.Module:
    """A deep copy of ``network`` with every quantized layer replaced by make(layer, kernel model, bias model).  A layer fitted
    with group-wise codebooks becomes make_grouped(...), a GroupedCompressedDense; ``grouped`` names the option that has no grouped
    form (None: there is one) and then raises NotImplementedError with the layer's name, before anything is built."""
    todo = []
    for name, layer in network.get_config().items():
        models = models_by_layer.get(layer)
        if not models or models[0] is None:
            continue
        if _is_grouped(models[0]) and grouped is not None:
            _grouped_only_byte_form(name, grouped)
        todo.append((name, layer, models[0], models[1] if len(models) > 1 else None))
    out = copy.deepcopy(network)
    for name, layer, wm, bm in todo:
        setattr(out, name, make_grouped(layer, wm, bm) if _is_grouped(wm) else make(layer, wm, bm))
    return out


def load_network(path: str, network: nn.Module, device=None, sparse=False, packed=False, sparse_half_inputs=False,
                 packed_half_inputs=False) -> nn.Module:
    """``compress_network`` from a stored network (storage.save_compressed, as Trainer.store_report writes it: records
    "{layer}.weights" / "{layer}.biases", or "{layer}.weights#g{g}" per group of a kernel with group-wise codebooks, whose
    ``group_rows`` is the row count of the first).  ``network`` gives the architecture; layers stored raw get the stored float32 values.
    ``sparse``, ``packed``, ``sparse_half_inputs`` and ``packed_half_inputs`` as in compress_network: the stored format is the same, the indices are packed after loading.  A
    kernel with group-wise codebooks raises NotImplementedError for either; pack_grouped_layers packs it after loading, and
    sparsify_grouped_layers gives it the bitmap-sparse form."""
    from . import storage

    _check_sparse(sparse)
    _check_packed(packed, sparse)
    _check_sparse_half_inputs(sparse_half_inputs, sparse)
    _check_packed_half_inputs(packed_half_inputs, sparse, packed, sparse_half_inputs)
    device = next(network.parameters()).device if device is None else device
    codes = storage.load_compressed_codes(path, device)
    out = copy.deepcopy(network)

    def tensor_of(entry):
        if isinstance(entry, tuple):
            _, centers, labels = entry
            return ops.gather(centers, labels)
        return entry.reshape(-1)

    for name, layer in network.get_config().items():
        wkey, bkey = f"{name}.weights", f"{name}.biases"
        if f"{wkey}#g0" in codes:   # a kernel with group-wise codebooks: one record per group (Trainer.store_compressed)
            if sparse is not False or packed is not False:
                _grouped_only_byte_form(name, "sparse=" + repr(sparse) if sparse is not False else "packed=" + repr(packed))
            parts = []
            while f"{wkey}#g{len(parts)}" in codes:
                parts.append(codes[f"{wkey}#g{len(parts)}"])
            (rows0, ncols), kdim = parts[0][0], sum(shape[0] for shape, _, _ in parts)
            bias = tensor_of(codes[bkey]) if bkey in codes else None
            group_rows = rows0 if len(parts) > 1 else -(-rows0 // 32) * 32   # one group: any multiple of 32 that holds every row
            setattr(out, name, GroupedCompressedDense(kdim, ncols, group_rows, torch.cat([lab.reshape(-1) for _, _, lab in parts]),
                                                      torch.stack([cen for _, cen, _ in parts]), bias, layer.activation))
            continue
        if wkey not in codes:
            continue
        went = codes[wkey]
        bias = tensor_of(codes[bkey]) if bkey in codes else None
        if not isinstance(went, tuple):
            target = getattr(out, name)
            target.set_weights([went.reshape(target.kernel.shape)] + ([bias.reshape(target.bias.shape)] if bias is not None else []))
            continue
        shape, centers, labels = went
        setattr(out, name, _from_codes(layer, tuple(shape), labels, centers, bias, sparse, packed, sparse_half_inputs, packed_half_inputs))
    return out


def pack_grouped_layers(network: nn.Module, packed=True) -> nn.Module:
    """A deep copy of a compressed ``network`` (compress_network, Trainer.compressed_network() or load_network) whose
    GroupedCompressedDense layers keep their indices in the 2- or 4-bit packed form (GroupedPackedCompressedDense, DESIGN.md section
    18).  ``packed``: True (every grouped layer of at most 16 centres per group) or "auto" (a layer only where the packed form
    holds fewer resident bytes; on equal bytes the byte form stays); anything else is a ValueError.  Grouped layers of more than
    16 centres and all other layers are left as they are.  Every replaced layer computes what it computed before, bit for bit."""
    if packed is not True and packed != "auto":
        raise ValueError(f"packed must be True or 'auto', got {packed!r}")
    out = copy.deepcopy(network)
    for name, layer in out.get_config().items():
        if not isinstance(layer, GroupedCompressedDense) or layer.centers.shape[1] > PACKED_MAX_K:
            continue
        bits = ops.packed_bits(layer.centers.shape[1])
        if packed == "auto" and ops.packed_nbytes(layer.kdim, layer.ncols, bits) >= layer.labels.numel():
            continue
        setattr(out, name, GroupedPackedCompressedDense.from_grouped(layer))
    return out


def sparsify_grouped_layers(network: nn.Module, sparse=True, half_inputs: bool = False) -> nn.Module:
    """A deep copy of a compressed ``network`` (compress_network, Trainer.compressed_network() or load_network) whose
    GroupedCompressedDense layers keep their indices in the bitmap-sparse form with one skipped index per group
    (GroupedSparseCompressedDense).  ``sparse``: True (every GroupedCompressedDense) or "auto" (a layer only
    where the sparse form holds fewer resident bytes; on equal bytes the byte form stays); anything else is a ValueError.
    GroupedPackedCompressedDense layers and all other layers are left as they are.  A replaced layer has the same weights; its sums run
    in another order (within the float bound of section 28, the same bits on exact data).  It takes float32 activations, and with
    ``half_inputs=True`` bfloat16 and float16 ones too (GroupedSparseCompressedDense(half_inputs=True));
    ``half_inputs`` does not change which layers are replaced."""
    if sparse is not True and sparse != "auto":
        raise ValueError(f"sparse must be True or 'auto', got {sparse!r}")
    out = copy.deepcopy(network)
    for name, layer in out.get_config().items():
        if not isinstance(layer, GroupedCompressedDense):
            continue
        made = GroupedSparseCompressedDense.from_grouped(layer, half_inputs=half_inputs)
        if sparse == "auto" and made.nbytes() >= layer.nbytes():
            continue
        setattr(out, name, made)
    return out


def smallest_grouped_layers(network: nn.Module, half_inputs: bool = False) -> nn.Module:
    """A deep copy of a compressed ``network`` in which every GroupedCompressedDense takes the form with the fewest resident bytes
    (nbytes()) of the three it has: the byte form it is in, the 2- or 4-bit packed form (GroupedPackedCompressedDense, a candidate
    only with at most 16 centres per group) and the bitmap-sparse form (GroupedSparseCompressedDense).  On equal bytes the order is
    byte, then packed, then sparse.  All other layers are left as they are.  A layer that ends in the sparse form takes float32
    activations, and with ``half_inputs=True`` bfloat16 and float16 ones too, as the other two forms do;
    ``half_inputs`` does not change which form is picked."""
    out = copy.deepcopy(network)
    for name, layer in out.get_config().items():
        if not isinstance(layer, GroupedCompressedDense):
            continue
        best = layer
        if layer.centers.shape[1] <= PACKED_MAX_K:
            made = GroupedPackedCompressedDense.from_grouped(layer)
            best = made if made.nbytes() < best.nbytes() else best
        made = GroupedSparseCompressedDense.from_grouped(layer, half_inputs=half_inputs)
        best = made if made.nbytes() < best.nbytes() else best
        if best is not layer:
            setattr(out, name, best)
    return out


def compressed_nbytes(network: nn.Module) -> int:
    """Resident bytes of the tensors of ``network``'s layers (or of one layer): indices (or their bitmap-sparse or packed form) + codebook +
    decoded bias for the compressed ones, the float32 parameters for the others."""
    layers = network.get_config().values() if hasattr(network, "get_config") else [network]
    total = 0
    for layer in layers:
        if isinstance(layer, (_InferenceLayer, _TrainableCentres)):
            total += layer.nbytes()
        else:
            total += sum(p.numel() * p.element_size() for p in layer.parameters())
    return total
