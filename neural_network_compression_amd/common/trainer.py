"""Trainer with the reference's call surface, weights and masks resident on the GPU.

Counterpart of neural_network_compression/common/trainer.py.  The compression steps are the
hot path and run in the HIP kernels:

    Trainer._prune_parameters        (trainer.py:177-193)  -> utility.prune_weigth per tensor, in place in HBM
    Trainer._reset_pruned_parameters (trainer.py:195-206)  -> ops.apply_mask_ with the stored device masks
    Trainer.quantize                 (trainer.py:42-72)    -> utility.get_weight_distribution (zeros skipped on
                                                              the device) + utility.get_quantized_weight

The reference round-trips every tensor through host NumPy on every batch
(layer.get_weights()/set_weights()); here nothing leaves the device.  The gradient / Adam / accuracy
parts (trainer.py:208-232, TensorFlow upstream) are a minimal torch loop: they are callers of the path,
not the path.
"""
from __future__ import annotations

import pathlib
from abc import ABC, abstractmethod
from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch

from .. import ops
from . import utility


class LeNetDataset(NamedTuple):
    input_data: np.ndarray
    output_data: np.ndarray


def _batches(x: torch.Tensor, y: torch.Tensor, batch: int = 512, shuffle_buffer: int = 1000):
    """tf.data .shuffle(1000).batch(512, drop_remainder=True) in spirit: a windowed shuffle."""
    n = x.shape[0]
    order = torch.arange(n, device=x.device)
    for lo in range(0, n, shuffle_buffer):
        hi = min(n, lo + shuffle_buffer)
        order[lo:hi] = order[lo:hi][torch.randperm(hi - lo, device=x.device)]
    for lo in range(0, n - batch + 1, batch):
        idx = order[lo: lo + batch]
        yield x[idx], y[idx]


def kernel_l2(layer) -> torch.Tensor:
    """tf.nn.l2_loss of a layer's kernel, sum(kernel^2) / 2: from the float32 kernel, or for a trainable codebook layer from its
    codebook and index counts (kernel_sq_sum, compressed.py) without the kernel."""
    if hasattr(layer, "kernel_sq_sum"):
        return layer.kernel_sq_sum() / 2
    return (layer.kernel ** 2).sum() / 2


class _HalfActivations(torch.nn.Module):
    """A trainable codebook network run on half activations: the input cast to ``dtype``, the output back to float32 (before the
    loss).  Everything else -- get_config, the layers by name, the parameters -- is the wrapped network's."""

    def __init__(self, network: torch.nn.Module, dtype):
        super().__init__()
        self.network, self.dtype = network, dtype

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(super().__getattr__("network"), name)

    def forward(self, x, *args, **kwargs):
        return self.network(x.to(self.dtype), *args, **kwargs).to(torch.float32)


class Trainer(ABC):
    neural_network: torch.nn.Module
    optimizer: torch.optim.Optimizer

    # zero-weight masks per layer; class level, as in the reference (trainer.py:25)
    pruned_indexes_by_layer: Dict[torch.nn.Module, Tuple[torch.Tensor, torch.Tensor]] = {}

    @property
    @abstractmethod
    def model_name(self) -> str:
        """The model name."""

    @property
    @abstractmethod
    def _layers_to_prune_with_threshold(self) -> Dict[torch.nn.Module, Tuple[float, float]]:
        """layer -> (weight threshold, bias threshold)."""

    @abstractmethod
    def _get_error(self, input_data: torch.Tensor, expected_output: torch.Tensor, network: torch.nn.Module | None = None) -> torch.Tensor:
        """The loss of ``network`` (by default the float network; fine_tune_compressed passes its trainable codebook copy)."""

    # ------------------------------------------------------------------ device plumbing
    @property
    def device(self) -> torch.device:
        return next(self.neural_network.parameters()).device

    def _to_device(self, a) -> torch.Tensor:
        return torch.as_tensor(np.asarray(a)).to(self.device)

    # ------------------------------------------------------------------ the hot path
    def quantize(self, test_dataset: LeNetDataset, with_cumulative_weight_distribution: bool,
                 maximum_centroid_bits: int, k_means_initialization_mode: str, *, arith: str = "auto", reloc: str = "auto",
                 group_rows: int | None = None) -> float:
        """The reference's signature (common/trainer.py:42-48) plus two keywords that select its own arithmetic where identity
        with it is wanted (utility.get_quantized_weight): ``arith="reference"`` = scikit-learn's float32 running sums in sample
        order on tensors of any length (centres, indices and n_iter_ then equal the reference's on one thread bit for bit; slower:
        a host round trip per Lloyd iteration beyond 4096 weights), ``reloc="reference"`` = numpy.argpartition's own choice of the
        far samples at an empty-cluster event.  The defaults are the order-independent exact sums and the on-device selection.
        ``group_rows`` (None: one codebook per tensor, as ever): every 2-D Dense kernel gets one codebook per block of that many
        input rows (a positive multiple of 32; utility.get_quantized_weight_grouped): its model is a
        utility.GroupedModel and compressed_network() runs it as a GroupedCompressedDense.  Conv2D kernels (their rows in unfold
        order are not contiguous in the Keras kernel) and biases are fitted as without it.  A group too small for the number of
        centroids, or more than 256 of them, is a ValueError before any fit."""
        from ..neural_networks.layers import Dense

        self.quantized_models_by_layer = {}   # layer -> [fitted model or None per tensor]: what fine_tune_centroids needs
        layers = [layer for _layer_name, layer in self.neural_network.get_config().items()]
        # The tensors of the network are independent: where the init draws nothing from NumPy's global generator (linear,
        # density) they go through the library's one-call layer, several side by side on streams of their own
        # (pipeline.compress_layers) -- the same results as the calls below one after the other
        # (tests/test_gpu_config5.py::test_layer_as_one_library_call_equals_the_step_by_step_path, test_layers_side_by_side_...).
        # Everything else -- forgy / kmeans++ (global generator, in layer order), tensors too short for the number of centroids
        # (the reference's "not enough bits" pass-through), the error cases -- takes the reference's own sequence of calls.
        mode, bits = k_means_initialization_mode, maximum_centroid_bits
        # (layer index, tensor index) -> the row ranges of the groups of a Dense kernel; checked for every kernel before the first fit
        grouped = {}
        if group_rows is not None:
            for li, layer in enumerate(layers):
                if isinstance(layer, Dense):
                    grouped[(li, 0)] = utility.grouped_slices(tuple(layer.kernel.shape), group_rows, bits, mode)
        batched = {}
        if (arith, reloc) == ("auto", "auto") and mode in ("linear", "density") and (mode != "density" or with_cumulative_weight_distribution) and isinstance(bits, int) and 1 <= bits <= 10:
            from .. import pipeline

            todo = [(li, ti, params) for li, layer in enumerate(layers) for ti, params in enumerate(layer.get_weights())
                    if isinstance(params, torch.Tensor) and params.is_cuda and params.dtype == torch.float32 and params.is_contiguous()
                    and params.numel() >= 2 ** bits + 1]
            # a grouped kernel goes in as its groups' slices (contiguous: the kernel is row-major), each a tensor of the batch
            parts = []
            for li, ti, p in todo:
                parts += [p[lo:hi] for lo, hi in grouped[(li, ti)]] if (li, ti) in grouped else [p]
            if parts:
                res = iter(pipeline.compress_layers([p.reshape(-1) for p in parts], workers=8, q=None, bits=bits, mode=mode,
                                                    with_cdf=(mode == "density"), huffman=True, want_values=True))
                for li, ti, p in todo:
                    if (li, ti) in grouped:
                        rs = [next(res) for _ in grouped[(li, ti)]]
                        batched[(li, ti)] = (torch.cat([r.values for r in rs]).view(p.shape), utility.GroupedModel(group_rows, [r.model for r in rs]))
                    else:
                        r = next(res)
                        batched[(li, ti)] = (r.values.view(p.shape), r.model)
        for li, layer in enumerate(layers):
            quantized_weights_and_bias = []
            models = []
            for ti, params in enumerate(layer.get_weights()):
                if (li, ti) in batched:
                    quantized, model = batched[(li, ti)]
                elif (li, ti) in grouped:
                    cdfs = None
                    if with_cumulative_weight_distribution:
                        cdfs = [utility.get_weight_distribution(params[lo:hi], skip_zeros=True) for lo, hi in grouped[(li, ti)]]
                    quantized, model = utility.get_quantized_weight_grouped(params, group_rows, bits=bits, mode=mode, cdfs_by_group=cdfs,
                                                                            arith=arith, reloc=reloc)
                else:
                    cdfs = None
                    if with_cumulative_weight_distribution:
                        # the reference strips exact zeros with numpy.delete first (trainer.py:55-59);
                        # the device kernels skip them instead -- same histogram, no compaction
                        cdfs = utility.get_weight_distribution(params, skip_zeros=True)
                    quantized, model = utility.get_quantized_weight(params, bits=maximum_centroid_bits,
                                                                    mode=k_means_initialization_mode, cdfs=cdfs, arith=arith, reloc=reloc)
                quantized_weights_and_bias.append(quantized)
                models.append(model)
            layer.set_weights(quantized_weights_and_bias)
            if models:
                self.quantized_models_by_layer[layer] = models
        return self._get_accuracy(test_dataset)

    def fine_tune_centroids(self, train_dataset: LeNetDataset, test_dataset: LeNetDataset, epochs: int,
                            learning_rate: float = 1e-3) -> List[float]:
        """Deep Compression's trained quantization, which the reference describes and leaves out as too slow on the host
        (papers/lat/report.tex:149-158): after ``quantize`` the centroid indices stay fixed; per batch the gradient of
        every quantized tensor is summed per centroid (ops.centroid_gradient: dL/dC_k = sum of dL/dW over cluster k, on
        the device), the centroids take a plain gradient step and the tensor is re-decoded from its indices
        (ops.gather).  Tensors that passed through unquantized are left alone.  Returns the accuracy per epoch."""
        models = getattr(self, "quantized_models_by_layer", None)
        if not models:
            raise RuntimeError("fine_tune_centroids needs a quantized network: call quantize first")
        for name, layer in self.neural_network.get_config().items():
            if any(hasattr(m, "group_rows") for m in models.get(layer, [])):
                raise NotImplementedError(f"layer {name!r} has group-wise codebooks (group_rows): fine_tune_centroids is not implemented for it")
        x = self._to_device(train_dataset.input_data).float()
        y = self._to_device(train_dataset.output_data).float()
        centers = {}
        for layer, ms in models.items():
            for ti, m in enumerate(ms):
                if m is not None:
                    centers[(layer, ti)] = torch.from_numpy(np.ascontiguousarray(m.cluster_centers_.ravel())).to(self.device)
        accuracies = []
        for _ in range(epochs):
            for xb, yb in _batches(x, y):
                self.optimizer.zero_grad(set_to_none=True)
                self._get_error(xb, yb).backward()
                with torch.no_grad():
                    for layer, ms in models.items():
                        tensors = layer.get_weights()
                        params = layer.trainable_tensors() if hasattr(layer, "trainable_tensors") else list(layer.parameters())
                        for ti, m in enumerate(ms):
                            if m is None or params[ti].grad is None:
                                continue
                            c = centers[(layer, ti)]
                            g = ops.centroid_gradient(params[ti].grad.contiguous(), m.labels_compact_, c.numel())
                            c.sub_((learning_rate * g).to(torch.float32))
                            tensors[ti] = ops.gather(c, m.labels_compact_).view(tensors[ti].shape)
                        layer.set_weights(tensors)
            accuracies.append(self._get_accuracy(test_dataset))
        for (layer, ti), c in centers.items():
            models[layer][ti].cluster_centers_ = c.cpu().numpy().reshape(-1, 1)
        return accuracies

    def fine_tune_compressed(self, train_dataset: LeNetDataset, test_dataset: LeNetDataset, epochs: int,
                             learning_rate: float = 1e-3, sparse=False, packed=False, activation_dtype=None,
                             sparse_half_inputs=False, packed_half_inputs=False) -> List[float]:
        """fine_tune_centroids' algorithm run on ``compressed.compress_network_trainable(..., sparse=sparse, packed=packed)``
        (both False: the network of ``compressed_network(trainable=True)``; sparse True or "auto": the bitmap-sparse trainable
        layers, for every quantized layer or where that form is smaller; packed True or "auto": the 2- or 4-bit packed trainable
        layers for the layers of at most 16 centres, or where that form is the smallest): the indices stay fixed and per batch
        every quantized tensor's centres take the plain step c -= learning_rate * dc, dc formed from the codebook and the indices
        (byte, bitmap-sparse or packed) by the backward of ops.codebook_linear / ops.sparse_codebook_linear /
        ops.packed_codebook_linear (DESIGN.md sections 12, 13, 15; neither W nor dW is built).
        Tensors that passed through unquantized stay frozen.  At the end the tuned centres go into ``quantized_models_by_layer``
        and the float layers are re-decoded from them (ops.gather), as after fine_tune_centroids.  Returns the accuracy per epoch
        (of the trainable network).
        ``activation_dtype``: None (float32), torch.bfloat16 or torch.float16 (sparse=False and packed=False
        only, else ValueError): the trainable network is built with half_inputs=True, its input is cast to the dtype and its output
        back to float32 before the loss, so the centres are tuned in the arithmetic the compressed network runs inference in.  The
        centres, their steps and the L2 term stay float32.  Every weighted layer then has to be a byte-form trainable layer: one that
        passed through unquantized raises a ValueError that names it.
        ``sparse_half_inputs=True`` (with ``activation_dtype`` and ``sparse`` True or "auto", packed=False; else ValueError): the
        pruned layers train on the half activations from their bitmap-sparse form -- the network is
        ``compress_network_trainable(..., sparse=sparse, sparse_half_inputs=True)``, in which the layers "auto" leaves in the byte
        form take half inputs too; a weighted layer that is neither raises the ValueError above.  Without the keyword
        ``activation_dtype`` with ``sparse`` stays a ValueError.
        ``packed_half_inputs=True`` (with ``activation_dtype`` and ``packed`` True or "auto"; with ``sparse`` other than False also
        sparse_half_inputs=True; else ValueError): the layers of at most 16 centres train on the half activations from their 2- or 4-bit
        packed form -- the network is ``compress_network_trainable(..., packed=packed, packed_half_inputs=True)``,
        in which the layers left in the byte form take half inputs too.  Without the keyword ``activation_dtype`` with ``packed``
        stays a ValueError."""
        models = getattr(self, "quantized_models_by_layer", None)
        if not models:
            raise RuntimeError("fine_tune_compressed needs a quantized network: call quantize first")
        from .. import compressed

        if packed_half_inputs and (activation_dtype is None or packed is False):
            raise ValueError("packed_half_inputs=True needs activation_dtype=torch.bfloat16 or torch.float16 and packed=True or 'auto': "
                             "it trains the 2- / 4-bit packed layers on half activations")
        if sparse_half_inputs and (activation_dtype is None or sparse is False or (packed is not False and not packed_half_inputs)):
            raise ValueError("sparse_half_inputs=True needs activation_dtype=torch.bfloat16 or torch.float16, sparse=True or 'auto' and "
                             "packed=False: it trains the bitmap-sparse layers on half activations")
        if activation_dtype is None:
            net = compressed.compress_network_trainable(self.neural_network, models, sparse=sparse, packed=packed)
            return self._tune_centres(net, models, train_dataset, test_dataset, epochs, learning_rate)
        if activation_dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"activation_dtype must be None, torch.bfloat16 or torch.float16, got {activation_dtype}")
        if not sparse_half_inputs and not packed_half_inputs and (sparse is not False or packed is not False):
            raise ValueError("activation_dtype needs sparse=False and packed=False (the byte form), or sparse=True / 'auto' with "
                             "sparse_half_inputs=True (the bitmap-sparse form): the packed forms do not train on bfloat16 / float16 inputs "
                             "unless packed=True / 'auto' comes with packed_half_inputs=True")
        if packed_half_inputs:   # (sparse without sparse_half_inputs: compress_network_trainable's ValueError, which names it)
            net = compressed.compress_network_trainable(self.neural_network, models, sparse=sparse, packed=packed,
                                                        sparse_half_inputs=sparse_half_inputs, packed_half_inputs=True)
        elif sparse_half_inputs:
            net = compressed.compress_network_trainable(self.neural_network, models, sparse=sparse, sparse_half_inputs=True)
        else:
            net = compressed.compress_network_trainable(self.neural_network, models, half_inputs=True)
        half_layers = (compressed._TrainableCodebookLayer, compressed._TrainableSparseCodebookLayer, compressed._TrainablePackedCodebookLayer)
        for name, layer in net.get_config().items():
            takes_half = isinstance(layer, half_layers) and layer.half_inputs
            if not takes_half and (hasattr(layer, "kernel") or next(layer.parameters(), None) is not None):
                raise ValueError(f"activation_dtype={activation_dtype}: layer {name!r} ({type(layer).__name__}) is not a byte-form, "
                                 "bitmap-sparse or packed trainable layer built with half_inputs (its kernel passed through unquantized, or it has "
                                 "no half-precision backward pass)")
        return self._tune_centres(_HalfActivations(net, activation_dtype), models, train_dataset, test_dataset, epochs, learning_rate)

    def fine_tune_grouped(self, train_dataset: LeNetDataset, test_dataset: LeNetDataset, epochs: int, learning_rate: float = 1e-3,
                          packed=False, sparse=False, activation_dtype=None) -> List[float]:
        """fine_tune_compressed's loop on ``compressed.compress_network_trainable_grouped(..., packed=packed, sparse=sparse)``: the Dense layers
        quantized with ``group_rows`` train their (G, K) centres through ops.grouped_codebook_linear (neither W
        nor dW is built), every other quantized tensor trains as in fine_tune_compressed(sparse=False, packed=False).  ``packed``
        True or "auto": the grouped layers of at most 16 centres per group train from their 2- or 4-bit packed indices instead
        (ops.grouped_packed_codebook_linear), every one or where that form is smaller.  At the end a
        GroupedModel's ``cluster_centers_`` gets the tuned (G, K), each of its ``models[q].cluster_centers_`` the first entries that
        are that group's own (not the zero padding of a shorter codebook), and the float kernel is re-decoded group by group, so
        compressed_network(), store_report and load_network see the tuned centres.  Returns the accuracy per epoch.
        ``activation_dtype``: None (float32), torch.bfloat16 or torch.float16 (with any ``packed``): the network is built with half_inputs=True, its input is cast to the dtype and its output back to float32 before
        the loss, as in fine_tune_compressed; centres, bias and their gradients stay float32, and the write-back and the re-decode
        are the same.  A layer with weights that takes no half input is a ValueError.
        ``sparse`` True or "auto": the grouped layers train from the bitmap-sparse form of their indices instead
        (ops.grouped_sparse_codebook_linear), every one or where that form is smaller; with ``packed`` not False
        a layer takes the smallest of its forms.  float32 activations only: ``sparse`` not False with ``activation_dtype`` is a
        ValueError.  The write-back of the tuned (G, K) is unchanged."""
        if sparse is not False and activation_dtype is not None:
            raise ValueError("sparse needs activation_dtype=None: the trainable grouped bitmap-sparse layer takes float32 activations only "
                             "(activation_dtype trains the byte and packed grouped forms)")
        models = getattr(self, "quantized_models_by_layer", None)
        if not models:
            raise RuntimeError("fine_tune_grouped needs a quantized network: call quantize first")
        from .. import compressed

        # ``sparse`` is passed only where it is asked for: older tests replace compress_network_trainable_grouped by a recorder and
        # pin the keywords of this call, so without ``sparse`` it stays the call it was
        if activation_dtype is None:
            net = compressed.compress_network_trainable_grouped(self.neural_network, models, packed=packed,
                                                                **({} if sparse is False else dict(sparse=sparse)))
            return self._tune_centres(net, models, train_dataset, test_dataset, epochs, learning_rate)
        if activation_dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"activation_dtype must be None, torch.bfloat16 or torch.float16, got {activation_dtype}")
        net = compressed.compress_network_trainable_grouped(self.neural_network, models, packed=packed, half_inputs=True)
        half_layers = (compressed._TrainableCodebookLayer, compressed.TrainableGroupedCompressedDense, compressed.TrainableGroupedPackedCompressedDense)
        for name, layer in net.get_config().items():
            takes_half = isinstance(layer, half_layers) and layer.half_inputs
            if not takes_half and (hasattr(layer, "kernel") or next(layer.parameters(), None) is not None):
                raise ValueError(f"activation_dtype={activation_dtype}: layer {name!r} ({type(layer).__name__}) is not a byte-form or group-wise "
                                 "trainable layer built with half_inputs (its kernel passed through unquantized, or it has no half-precision "
                                 "backward pass)")
        return self._tune_centres(_HalfActivations(net, activation_dtype), models, train_dataset, test_dataset, epochs, learning_rate)

    def _tune_centres(self, net, models, train_dataset, test_dataset, epochs, learning_rate) -> List[float]:
        """The loop of fine_tune_compressed / fine_tune_grouped on the trainable network ``net`` of this trainer's quantized
        network: plain steps on the centres, then the tuned centres into ``models`` and the float layers re-decoded from them."""
        from .. import compressed

        for p in net.parameters():
            p.requires_grad_(False)
        tuned = {}   # layer name -> trainable layer
        params = []
        for name, layer in net.get_config().items():
            if isinstance(layer, compressed._TrainableCentres):
                tuned[name] = layer
                for p in (layer.centers, layer.bias_centers):
                    if p is not None:
                        p.requires_grad_(True)
                        params.append(p)
        x = self._to_device(train_dataset.input_data).float()
        y = self._to_device(train_dataset.output_data).float()
        accuracies = []
        for _ in range(epochs):
            for xb, yb in _batches(x, y):
                for p in params:
                    p.grad = None
                self._get_error(xb, yb, net).backward()
                with torch.no_grad():
                    for p in params:
                        if p.grad is not None:
                            p.sub_(learning_rate * p.grad)
            accuracies.append(self._get_accuracy(test_dataset, net))
        with torch.no_grad():
            for name, layer in self.neural_network.get_config().items():
                t = tuned.get(name)
                if t is None:
                    continue
                ms = models[layer]
                tensors = layer.get_weights()
                for ti, c in ((0, t.centers), (1, t.bias_centers)):
                    if c is None or ti >= len(ms) or ms[ti] is None:
                        continue
                    c = c.detach().contiguous()
                    if hasattr(ms[ti], "group_rows"):   # group-wise codebooks: (G, K) back, each group's own entries into its model
                        ms[ti].cluster_centers_ = c.cpu().numpy()
                        parts = []
                        for q, gm in enumerate(ms[ti].models):
                            size = int(gm.cluster_centers_.size)
                            gm.cluster_centers_ = ms[ti].cluster_centers_[q, :size].reshape(-1, 1).copy()
                            parts.append(ops.gather(c[q].contiguous(), gm.labels_compact_))
                        tensors[ti] = torch.cat(parts).view(tensors[ti].shape)
                        continue
                    ms[ti].cluster_centers_ = c.cpu().numpy().reshape(-1, 1)
                    tensors[ti] = ops.gather(c, ms[ti].labels_compact_).view(tensors[ti].shape)
                layer.set_weights(tensors)
        return accuracies

    def compressed_network(self, sparse=False, trainable=False, packed=False, half_inputs=False, sparse_half_inputs=False,
                           packed_half_inputs=False) -> torch.nn.Module:
        """A copy of the network whose quantized layers run from their codebooks and centroid indices (compressed.py; the
        float32 weights are never rebuilt), with the centres as they stand (after fine_tune_centroids, the tuned ones).
        ``sparse``: False, True (the indices in the bitmap-sparse form) or "auto" (per layer, the smaller form).
        ``packed``: False, True (2- or 4-bit packed indices for every layer of at most 16 centres) or "auto" (per layer, the smallest
        form).
        ``trainable=True`` (with sparse=False and packed=False only): the layers' centres are parameters with a backward pass (DESIGN.md
        section 12); fine_tune_compressed(..., sparse=..., packed=...) trains the other two forms.  ``half_inputs=True`` with it:
        those layers train on bfloat16 / float16 inputs too.  ``sparse_half_inputs=True`` (with ``sparse`` True or
        "auto", not trainable): the bitmap-sparse layers run on bfloat16 / float16 inputs.
        ``packed_half_inputs=True`` (with ``packed`` True or "auto", not trainable): the packed layers run on them.
        A layer quantized with ``group_rows`` becomes a GroupedCompressedDense; with it any of the three options raises
        NotImplementedError with the layer's name (compressed.pack_grouped_layers packs the grouped layers of the result, DESIGN.md
        section 18)."""
        models = getattr(self, "quantized_models_by_layer", None)
        if not models:
            raise RuntimeError("compressed_network needs a quantized network: call quantize first")
        from .. import compressed

        return compressed.compress_network(self.neural_network, models, sparse=sparse, trainable=trainable, packed=packed, half_inputs=half_inputs,
                                            sparse_half_inputs=sparse_half_inputs, packed_half_inputs=packed_half_inputs)

    def _discard_quantization(self) -> None:
        """The weights are about to change: the centroid indices of ``quantize`` no longer describe them, so nothing may store, run
        or fine-tune from them any more."""
        self.quantized_models_by_layer = {}

    def _prune_parameters(self, with_standard_deviation_smoothing: bool) -> None:
        self._discard_quantization()
        for layer, (weight_threshold, bias_threshold) in self._layers_to_prune_with_threshold.items():
            weights, biases = layer.get_weights()
            zero_weight = utility.prune_weigth(weights, threshold=weight_threshold,
                                               std_smooth=with_standard_deviation_smoothing)
            zero_bias = utility.prune_weigth(biases, threshold=bias_threshold,
                                             std_smooth=with_standard_deviation_smoothing)
            self.pruned_indexes_by_layer[layer] = (zero_weight, zero_bias)
            layer.set_weights([weights, biases])

    def _reset_pruned_parameters(self) -> None:
        for layer, (zero_weight, zero_bias) in self.pruned_indexes_by_layer.items():
            weights, biases = layer.get_weights()
            ops.apply_mask_(weights, zero_weight)
            ops.apply_mask_(biases, zero_bias)
            layer.set_weights([weights, biases])

    # ------------------------------------------------------------------ callers of the path
    def train(self, train_dataset: LeNetDataset, test_dataset: LeNetDataset, epochs: int) -> List[float]:
        return self._epochs(train_dataset, test_dataset, epochs, prune=False, reset=False)

    def semi_pruned_train(self, train_dataset: LeNetDataset, test_dataset: LeNetDataset, epochs: int) -> List[float]:
        return self._epochs(train_dataset, test_dataset, epochs, prune=False, reset=True)

    def pruned_train(self, train_dataset: LeNetDataset, test_dataset: LeNetDataset, epochs: int,
                     with_standard_deviation_smoothing: bool) -> List[float]:
        return self._epochs(train_dataset, test_dataset, epochs, prune=True, reset=True,
                            smoothing=with_standard_deviation_smoothing)

    def _epochs(self, train_dataset, test_dataset, epochs, prune, reset, smoothing=True) -> List[float]:
        self._discard_quantization()
        x = self._to_device(train_dataset.input_data).float()
        y = self._to_device(train_dataset.output_data).float()
        accuracies = []
        for _ in range(epochs):
            for xb, yb in _batches(x, y):
                if prune:
                    self._prune_parameters(smoothing)
                self._apply_gradient(self._get_gradient(xb, yb))
                if reset:
                    self._reset_pruned_parameters()
            accuracies.append(self._get_accuracy(test_dataset))
        return accuracies

    def store_report(self, directory: str) -> None:
        """Zero counts per layer, as the reference's report.txt (common/trainer.py:154-175; its plots are out of scope).  After
        ``quantize`` (and no retraining since) also ``store_compressed``: the stored network and its ratio."""
        pathlib.Path(directory).mkdir(parents=True, exist_ok=True)
        report = ""
        for layer_name, layer in self.neural_network.get_config().items():
            tensors = layer.get_weights()
            if not tensors:
                continue
            weight_layer, bias_layer = tensors
            report += f"layer: {layer_name}\n"
            report += f"zeroed weights: {int((weight_layer == 0).sum())}\ntotal weights: {weight_layer.numel()}\n"
            report += f"zeroed biases: {int((bias_layer == 0).sum())}\ntotal weights: {bias_layer.numel()}\n\n"
        with open(f"{directory}/report.txt", "w") as f:
            f.write(report)
        if getattr(self, "quantized_models_by_layer", None):
            self.store_compressed(directory)

    def store_compressed(self, directory: str) -> dict:
        """The quantized network in its stored form (storage.save_compressed: codebook + Huffman-coded centroid indices, dense or
        relative-index sparse, whichever is smaller per tensor -> ``weights.nnc``); appends to ``report.txt`` what Deep Compression
        reports: bits per weight of every tensor and the compression ratio against 32-bit weights.  Needs ``quantize`` with no
        retraining since (the indices must describe the weights).  A kernel with group-wise codebooks (quantize(..., group_rows=))
        is stored as one ordinary record per group, "{layer}.weights#g{g}" of shape (rows of the group, out); compressed.load_network
        puts them together again.  Returns storage.save_compressed's report."""
        models = getattr(self, "quantized_models_by_layer", None)
        if not models:
            raise RuntimeError("store_compressed needs a quantized network: call quantize first (retraining discards it)")
        from .. import storage

        pathlib.Path(directory).mkdir(parents=True, exist_ok=True)
        stored = {}
        for layer_name, layer in self.neural_network.get_config().items():
            if layer not in models:
                continue
            for kind, t, m in zip(("weights", "biases"), layer.get_weights(), models[layer]):
                if hasattr(m, "group_rows"):   # group-wise codebooks: one ordinary record per group, "{layer}.weights#g{g}"
                    for g, gm in enumerate(m.models):
                        rows = min(m.group_rows, t.shape[0] - g * m.group_rows)
                        stored[f"{layer_name}.{kind}#g{g}"] = ((rows, t.shape[1]), gm, None)
                    continue
                stored[f"{layer_name}.{kind}"] = (tuple(t.shape), m, t if m is None else None)
        rep = {}
        storage.save_compressed(f"{directory}/weights.nnc", stored, report=rep)
        self.compression_report = rep
        report = ""
        for name, r in rep.items():
            if name != "total":
                report += f"stored {name}: {r['bytes']} bytes, {r['bits_per_weight']:.3f} bits per weight ({r['form']}, {r['k']} centroids)\n"
        t = rep["total"]
        report += (f"stored network: {t['bytes']} bytes for {t['n']} weights = {t['bits_per_weight']:.3f} bits per weight; "
                   f"compression ratio {t['compression_ratio']:.1f}x against float32\n")
        with open(f"{directory}/report.txt", "a") as f:
            f.write(report)
        return rep

    def _get_gradient(self, input_data: torch.Tensor, expected_output: torch.Tensor):
        self.optimizer.zero_grad(set_to_none=True)
        loss = self._get_error(input_data, expected_output)
        loss.backward()
        return [p.grad for p in self.neural_network.parameters()]

    def _apply_gradient(self, gradient) -> None:
        for p, g in zip(self.neural_network.parameters(), gradient):
            p.grad = g
        self.optimizer.step()

    @torch.no_grad()
    def _get_accuracy(self, dataset: LeNetDataset, network: torch.nn.Module | None = None) -> float:
        x = self._to_device(dataset.input_data).float()
        y = self._to_device(dataset.output_data)
        net = self.neural_network if network is None else network
        pred = torch.argmax(torch.softmax(net(x), dim=1), dim=1)
        return float((pred == y.to(pred.dtype)).float().mean().item())
