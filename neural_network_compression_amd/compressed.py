"""Quantized layers run from their stored form: a K-entry codebook and one 1- or 2-byte centroid index per weight.

``Trainer.quantize`` writes ``cluster_centers_[labels_]`` back into the float32 parameters, so the network it leaves reads
4 bytes per weight in every forward pass.  The layers here keep what the fit produced -- ``cluster_centers_`` and
``labels_compact_`` -- and multiply with the indices directly (ops.codebook_matmul, csrc/nnc_cbmm.hip): the float32 weight
tensor is never rebuilt.  Biases (one value per output column) are decoded once at construction and added by the kernel.

    CompressedDense.from_dense(dense, weight_model, bias_model)
    CompressedConv2D.from_conv(conv, weight_model, bias_model)     stride 1, padding "valid" | "same", NHWC in and out
    compress_network(network, models_by_layer)                     a deep copy with the quantized layers replaced
    load_network(path, network)                                    the same from a ``weights.nnc`` (Trainer.store_report)
    compressed_nbytes(network)                                     resident bytes of the layers' tensors

Inference only: under autograd, with an input that needs a gradient, the layers raise instead of returning a result that
silently has none (fine-tuning stays ``Trainer.fine_tune_centroids``).
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


class _CodebookLayer(nn.Module):
    """labels (kdim * ncols indices, row-major (kdim, ncols)), centers float32[K], bias float32[ncols] or None."""

    def __init__(self, kdim: int, ncols: int, labels: torch.Tensor, centers: torch.Tensor, bias: torch.Tensor | None, activation=None):
        super().__init__()
        if labels.numel() != kdim * ncols:
            raise ValueError(f"{labels.numel()} indices for a {kdim} x {ncols} weight matrix")
        self.kdim, self.ncols = int(kdim), int(ncols)
        self.register_buffer("labels", labels.reshape(-1))
        self.register_buffer("centers", centers.reshape(-1).to(torch.float32).contiguous())
        self.register_buffer("bias", None if bias is None else bias.reshape(-1).to(torch.float32).contiguous())
        self.activation = activation
        self._fused_relu = activation is torch.relu

    def _matmul(self, x: torch.Tensor) -> torch.Tensor:
        y = ops.codebook_matmul(x, self.labels, self.centers, self.kdim, self.ncols, bias=self.bias, relu=self._fused_relu)
        if self.activation is not None and not self._fused_relu:
            y = self.activation(y)
        return y

    def get_weights(self):
        return []

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.labels, self.centers, self.bias) if t is not None)


class CompressedDense(_CodebookLayer):
    """Dense run from its codebook: y = act(x @ kernel + bias), kernel (in, out) as Keras stores it (kdim = in, ncols = out)."""

    @classmethod
    def from_dense(cls, dense, weight_model, bias_model=None) -> "CompressedDense":
        if weight_model is None:
            raise ValueError("the kernel was not quantized (no fitted model): keep the float32 layer")
        kin, kout = dense.kernel.shape
        centers, labels = _codes(weight_model, dense.kernel.device)
        return cls(kin, kout, labels, centers, _decoded_bias(dense.bias, bias_model), dense.activation)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._matmul(x.contiguous())


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


class CompressedConv2D(_CodebookLayer):
    """Conv2D (stride 1, NHWC) run from its codebook: the patches of x times the kernel read from its indices, whose rows are
    put in unfold order once at construction (keras_rows_for_unfold)."""

    def __init__(self, kernel_size: int, cin: int, cout: int, pad: int, labels_unfold: torch.Tensor, centers: torch.Tensor,
                 bias: torch.Tensor | None, activation=None):
        super().__init__(kernel_size * kernel_size * cin, cout, labels_unfold, centers, bias, activation)
        self.kernel_size, self.cin, self.pad = int(kernel_size), int(cin), int(pad)

    @classmethod
    def from_conv(cls, conv, weight_model, bias_model=None) -> "CompressedConv2D":
        if weight_model is None:
            raise ValueError("the kernel was not quantized (no fitted model): keep the float32 layer")
        h, w, cin, cout = conv.kernel.shape
        if h != w:
            raise ValueError("square kernels only (as layers.Conv2D)")
        centers, labels = _codes(weight_model, conv.kernel.device)
        return cls.from_codes(h, cin, cout, conv.pad, labels, centers, _decoded_bias(conv.bias, bias_model), conv.activation)

    @classmethod
    def from_codes(cls, kernel_size, cin, cout, pad, labels, centers, bias, activation) -> "CompressedConv2D":
        """labels in the Keras order of the (h, w, in, out) kernel."""
        rows = torch.from_numpy(keras_rows_for_unfold(kernel_size, kernel_size, cin)).to(labels.device)
        return cls(kernel_size, cin, cout, pad, labels.reshape(-1, cout)[rows].contiguous(), centers, bias, activation)

    def forward(self, x: torch.Tensor) -> torch.Tensor:   # x: (N, H, W, C)
        n, hh, ww, _ = x.shape
        ho, wo = hh + 2 * self.pad - self.kernel_size + 1, ww + 2 * self.pad - self.kernel_size + 1
        per = max(1, _PATCH_BYTES // max(1, ho * wo * self.kdim * 4))
        outs = [self._matmul(conv_patches(x[i: i + per], self.kernel_size, self.pad).contiguous()) for i in range(0, n, per)]
        if not outs:   # an empty batch: the (0, kdim) product, as F.conv2d gives an empty result
            outs = [self._matmul(x.new_empty((0, self.kdim)))]
        y = outs[0] if len(outs) == 1 else torch.cat(outs)
        return y.reshape(n, ho, wo, self.ncols)


def _replace(layer, weight_model, bias_model):
    from .neural_networks.layers import Conv2D, Dense

    if isinstance(layer, Dense):
        return CompressedDense.from_dense(layer, weight_model, bias_model)
    if isinstance(layer, Conv2D):
        return CompressedConv2D.from_conv(layer, weight_model, bias_model)
    raise TypeError(f"no compressed form of {type(layer).__name__}")


def compress_network(network: nn.Module, models_by_layer) -> nn.Module:
    """A deep copy of ``network`` whose quantized layers (``models_by_layer``: layer -> [kernel model, bias model], as
    Trainer.quantized_models_by_layer) run from their codebooks.  Layers are replaced by the attribute names of
    ``get_config()``; a layer whose kernel passed through unquantized (model None) stays float32."""
    out = copy.deepcopy(network)
    for name, layer in network.get_config().items():
        models = models_by_layer.get(layer)
        if not models or models[0] is None:
            continue
        bias_model = models[1] if len(models) > 1 else None
        setattr(out, name, _replace(layer, models[0], bias_model))
    return out


def load_network(path: str, network: nn.Module, device=None) -> nn.Module:
    """``compress_network`` from a stored network (storage.save_compressed, as Trainer.store_report writes it: records
    "{layer}.weights" / "{layer}.biases").  ``network`` gives the architecture; layers stored raw get the stored float32 values."""
    from . import storage
    from .neural_networks.layers import Conv2D, Dense

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
        if wkey not in codes:
            continue
        went = codes[wkey]
        bias = tensor_of(codes[bkey]) if bkey in codes else None
        if not isinstance(went, tuple):
            target = getattr(out, name)
            target.set_weights([went.reshape(target.kernel.shape)] + ([bias.reshape(target.bias.shape)] if bias is not None else []))
            continue
        shape, centers, labels = went
        if isinstance(layer, Dense):
            new = CompressedDense(shape[0], shape[1], labels, centers, bias, layer.activation)
        elif isinstance(layer, Conv2D):
            new = CompressedConv2D.from_codes(shape[0], shape[2], shape[3], layer.pad, labels, centers, bias, layer.activation)
        else:
            raise TypeError(f"no compressed form of {type(layer).__name__}")
        setattr(out, name, new)
    return out


def compressed_nbytes(network: nn.Module) -> int:
    """Resident bytes of the tensors of ``network``'s layers (or of one layer): indices + codebook + decoded bias for the
    compressed ones, the float32 parameters for the others."""
    layers = network.get_config().values() if hasattr(network, "get_config") else [network]
    total = 0
    for layer in layers:
        if isinstance(layer, _CodebookLayer):
            total += layer.nbytes()
        else:
            total += sum(p.numel() * p.element_size() for p in layer.parameters())
    return total
