"""Compressed on-disk form of quantized layers: codebook + Huffman-coded centroid indices, dense or relative-index sparse.

The reference keeps nothing on disk and only names the third stage of Deep Compression (Huffman coding,
README.md:9); what ``get_quantized_weight`` returns -- ``cluster_centers_`` and ``labels_``
(neural_network_compression/common/utility.py:239) -- is exactly a codebook and an index stream, so the stored layer is
those two, with the indices entropy coded on the GPU (include/nnc.h, nnc_huffman_*; csrc/nnc_codec.hip).  Decoding gives
back ``cluster_centers_[labels_]`` bit for bit.

Two forms of the index stream, the smaller one is kept per tensor (``form="auto"``):
  * dense  : every index Huffman coded (the pruned zeros share one centroid, whose index then costs one bit);
  * sparse : Deep Compression's relative-index format (section 3 of the paper the reference's report follows,
             papers/lat/report.tex:327): only the indices that are not the zero cluster's, each with the distance to the
             previous stored position in 4 or 8 bits, filler entries for longer gaps; both entry streams Huffman coded.

File layout (little endian), one record per tensor:

    "NNC2" | u32 n_tensors
    per tensor: u16 name length, name (utf-8) | u8 ndim, u64 shape[ndim] | u32 K | u8 label_bytes | u64 N | u64 total_bits
                f32 codebook[K] | u8 form (0 dense, 1 sparse)
      dense :   STREAM(K, N)
      sparse:   u8 delta_bits | u32 zero_symbol | u64 entries | u16 entries_in_chunk[ceil(N / 1024)]
                STREAM(2^delta_bits, entries) of the distances - 1 | STREAM(K, entries) of the indices
      STREAM(k, n) = u64 bits | u8 code_length[k] | u32 chunk_bits[ceil(n / 1024)] | u32 words[ceil(bits / 32)]  (MSB-first)
    total_bits = all stream bits of the record (what the compression ratio counts besides the tables).
    a tensor that passed through unquantized ("not enough bits") is stored raw: K = 0, then f32 data[N].

A file is checked field by field on the host before anything reaches the device (_parse_records): a malformed
or truncated one raises ValueError naming the field.  Files of the older NNC1 layout are not read.
"""
from __future__ import annotations

import ctypes
import math
import struct
from typing import Dict, Tuple

import numpy as np
import torch

from . import _native as nat
from . import ops

MAGIC = b"NNC2"
CHUNK = 1024
NNC_KMAX = nat.NNC_KMAX


def _flatten_lengths(lengths: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """Code lengths beyond 32 bits (possible only for hugely skewed histograms with hundreds of symbols) are replaced by a
    fixed-width code over the used symbols: still a prefix code, decodable by the same tables."""
    if int(lengths.max(initial=0)) <= 32:
        return lengths
    used = counts > 0
    width = max(1, int(np.ceil(np.log2(max(2, int(used.sum()))))))
    out = np.zeros_like(lengths)
    out[used] = width
    return out


def _check_histogram(counts: np.ndarray, k: int, n: int) -> None:
    """The encoders give an index >= k no bits and the histogram does not count it, so the stream would silently lose it: a
    histogram of k bins that does not add up to n means such an index is there."""
    if counts.size != k or int(counts.sum()) != n:
        raise ValueError(f"an index is >= k = {k} (the histogram of {n} indices over {k} symbols adds up to {int(counts.sum())})")


def encode_indices(labels: torch.Tensor, k: int, counts: np.ndarray | None = None):
    """labels: device uint8 / int16-storage centroid indices.  Returns (words uint32 device tensor, chunk_bits np.uint32[nchunks],
    lengths np.uint8[k], total_bits)."""
    L = nat.load()
    n = labels.numel()
    lb = ops._label_bytes(labels)
    if counts is None:
        counts = ops.bincount(labels, k).cpu().numpy()
    counts = np.asarray(counts, dtype=np.int64)
    _check_histogram(counts, k, n)
    lengths, _, _ = ops.huffman_lengths(counts)
    lengths = _flatten_lengths(np.ascontiguousarray(lengths, dtype=np.uint8), counts)
    codes = np.zeros(k, dtype=np.uint32)
    nat.check(L.nnc_huffman_codes(lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), k, codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
    dev = labels.device
    stream = ops._stream(labels)
    len_d = torch.from_numpy(lengths).to(dev)
    codes_d = torch.from_numpy(codes.view(np.int32)).to(dev)
    nchunks = int(L.nnc_codec_chunks(n))
    off = torch.empty(nchunks + 1, dtype=torch.int64, device=dev)
    nat.check(L.nnc_huffman_chunk_offsets(ops._ptr(labels), lb, n, len_d.data_ptr(), k, off.data_ptr(), stream))
    total_bits = int((counts * lengths.astype(np.int64)).sum())     # known on the host: no read of the device total needed
    nwords = total_bits // 32 + 2
    words = torch.empty(nwords, dtype=torch.int32, device=dev)
    nat.check(L.nnc_huffman_encode(ops._ptr(labels), lb, n, codes_d.data_ptr(), len_d.data_ptr(), k, off.data_ptr(), words.data_ptr(), nwords, stream))
    off_h = off.cpu().numpy()
    assert int(off_h[-1]) == total_bits, (int(off_h[-1]), total_bits)
    chunk_bits = np.diff(off_h).astype(np.uint32)
    return words[: (total_bits + 31) // 32], chunk_bits, lengths, total_bits


def decode_indices(words: torch.Tensor, chunk_bits: np.ndarray, n: int, lengths: np.ndarray, k: int, label_bytes: int) -> torch.Tensor:
    """The inverse of encode_indices on the device; raises if the stream does not parse."""
    L = nat.load()
    dev = words.device
    stream = ops._stream(words)
    tb = int(L.nnc_huffman_decode_tables_bytes())
    tables = np.zeros(tb, dtype=np.uint8)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint8)
    nat.check(L.nnc_huffman_decode_tables(lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), k, tables.ctypes.data, tb))
    tables_d = torch.from_numpy(tables).to(dev)
    off = np.zeros(chunk_bits.size + 1, dtype=np.int64)
    np.cumsum(chunk_bits.astype(np.int64), out=off[1:])
    off_d = torch.from_numpy(off).to(dev)
    padded = torch.zeros(words.numel() + 2, dtype=torch.int32, device=dev)   # the decoder may look one word past the end
    padded[: words.numel()] = words
    out = torch.empty(n, dtype=torch.uint8 if label_bytes == 1 else torch.int16, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    nat.check(L.nnc_huffman_decode(padded.data_ptr(), off_d.data_ptr(), n, tables_d.data_ptr(), k, ops._ptr(out), label_bytes, bad.data_ptr(), stream))
    if int(bad.item()):
        raise ValueError("corrupt index stream")
    return out


def encode_sparse(labels: torch.Tensor, zero_symbol: int, delta_bits: int, k: int | None = None, counts: np.ndarray | None = None):
    """The relative-index entries of ``labels`` (device, indices < k; ``counts`` their histogram over k if known) -> (delta uint8
    device tensor [distance - 1], sym device tensor [indices, the labels' width], entries_in_chunk np.uint16[nchunks]).  Without
    ``k`` the bound is the codec's own, NNC_KMAX; pack_indices passes the tensor's K.  ValueError for an index or zero_symbol
    >= k."""
    L = nat.load()
    n = labels.numel()
    if k is None:
        k, counts = NNC_KMAX, None
    if not 0 <= int(zero_symbol) < k:
        raise ValueError(f"zero_symbol {zero_symbol} is not an index below k = {k}")
    if counts is None:
        counts = ops.bincount(labels, k).cpu().numpy()
    _check_histogram(np.asarray(counts, dtype=np.int64), k, n)
    lb = ops._label_bytes(labels)
    dev = labels.device
    stream = ops._stream(labels)
    nchunks = int(L.nnc_codec_chunks(n))
    off = torch.empty(nchunks + 1, dtype=torch.int64, device=dev)
    nat.check(L.nnc_sparse_entry_offsets(ops._ptr(labels), lb, n, int(zero_symbol), int(delta_bits), off.data_ptr(), stream))
    off_h = off.cpu().numpy()
    entries = int(off_h[-1])
    delta = torch.empty(max(entries, 1), dtype=torch.uint8, device=dev)
    sym = torch.empty(max(entries, 1), dtype=labels.dtype, device=dev)
    nat.check(L.nnc_sparse_emit(ops._ptr(labels), lb, n, int(zero_symbol), int(delta_bits), off.data_ptr(), delta.data_ptr(), sym.data_ptr(), stream))
    return delta[:entries], sym[:entries], np.diff(off_h).astype(np.uint16)


def decode_sparse(delta: torch.Tensor, sym: torch.Tensor, entries_in_chunk: np.ndarray, n: int, zero_symbol: int) -> torch.Tensor:
    """The inverse of encode_sparse on the device; raises if an entry points outside its chunk."""
    L = nat.load()
    dev = sym.device
    off = np.zeros(entries_in_chunk.size + 1, dtype=np.int64)
    np.cumsum(entries_in_chunk.astype(np.int64), out=off[1:])
    if int(off[-1]) != delta.numel() or delta.numel() != sym.numel():
        raise ValueError("corrupt entry table")
    off_d = torch.from_numpy(off).to(dev)
    out = torch.empty(n, dtype=sym.dtype, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    nat.check(L.nnc_sparse_expand(ops._ptr(delta), ops._ptr(sym), ops._label_bytes(sym), off_d.data_ptr(), n, int(zero_symbol), out.data_ptr(), bad.data_ptr(),
                                  ops._stream(sym)))
    if int(bad.item()):
        raise ValueError("corrupt sparse entries")
    return out


def _stream_bytes(words, chunk_bits, lengths, total_bits) -> bytes:
    return struct.pack("<Q", int(total_bits)) + lengths.tobytes() + chunk_bits.tobytes() + words.cpu().numpy().tobytes()


class _Reader:
    """Bounds-checked reads from a stored blob: running past its end is a ValueError, not a struct.error or a short array."""

    def __init__(self, blob, pos=0):
        self.blob, self.pos = blob, pos

    def take(self, fmt):
        size = struct.calcsize(fmt)
        if self.pos + size > len(self.blob):
            raise ValueError(f"truncated file: {size} bytes needed at offset {self.pos}, {len(self.blob)} in all")
        out = struct.unpack_from(fmt, self.blob, self.pos)
        self.pos += size
        return out

    def array(self, dtype, count):
        size = np.dtype(dtype).itemsize * count
        if self.pos + size > len(self.blob):
            raise ValueError(f"truncated file: {size} bytes needed at offset {self.pos}, {len(self.blob)} in all")
        out = np.frombuffer(self.blob, dtype=dtype, count=count, offset=self.pos)
        self.pos += size
        return out


def _parse_stream(r: _Reader, k: int, n: int, what: str):
    """STREAM(k, n) checked on the host -> (words int32, chunk_bits uint32, lengths uint8, total_bits).  The device decoder trusts
    its tables and chunk table, so everything it indexes by is checked here."""
    (total_bits,) = r.take("<Q")
    lengths = r.array(np.uint8, k)
    if int(lengths.max(initial=0)) > 32:
        raise ValueError(f"{what}: code_length {int(lengths.max())} > 32")
    used = lengths[lengths > 0].astype(np.int64)
    if int(np.sum(np.left_shift(1, 32 - used, dtype=np.int64))) > 1 << 32:
        raise ValueError(f"{what}: code_length violates Kraft's inequality")
    nchunks = (n + CHUNK - 1) // CHUNK
    chunk_bits = r.array(np.uint32, nchunks)
    if nchunks and int(chunk_bits.max()) > 32 * CHUNK:
        raise ValueError(f"{what}: chunk_bits {int(chunk_bits.max())} > {32 * CHUNK}")
    if int(chunk_bits.astype(np.int64).sum()) != total_bits:
        raise ValueError(f"{what}: chunk_bits do not add up to the stream's bits")
    words = r.array(np.int32, (total_bits + 31) // 32)
    return words, chunk_bits, lengths, total_bits


def _decode_stream(parsed, n, device, label_bytes):
    words, chunk_bits, lengths, total_bits = parsed
    if n == 0:
        return torch.empty(0, dtype=torch.uint8 if label_bytes == 1 else torch.int16, device=device)
    k = lengths.size
    return decode_indices(torch.from_numpy(words.copy()).to(device), chunk_bits, n, lengths.copy(), k, label_bytes)


SPARSE_MIN_ZERO_SHARE = 0.5     # below this share of zero-cluster indices the sparse form cannot win: it is not even tried


def pack_indices(labels: torch.Tensor, k: int, counts: np.ndarray | None = None, form: str = "auto"):
    """The index stream of one tensor -> (bytes from the `form` byte on, total stream bits, form name).  form: "dense", "sparse4",
    "sparse8", or "auto" (the smallest of the three in bytes)."""
    n = labels.numel()
    if counts is None:
        counts = ops.bincount(labels, k).cpu().numpy()
    counts = np.asarray(counts, dtype=np.int64)
    cands = {}
    if form in ("dense", "auto"):
        words, chunk_bits, lengths, total_bits = encode_indices(labels, k, counts)
        cands["dense"] = (struct.pack("<B", 0) + _stream_bytes(words, chunk_bits, lengths, total_bits), total_bits)
    zero = int(np.argmax(counts))
    for name, db in (("sparse4", 4), ("sparse8", 8)):
        if form != name and not (form == "auto" and n > 0 and counts[zero] >= SPARSE_MIN_ZERO_SHARE * n):
            continue
        delta, sym, per_chunk = encode_sparse(labels, zero, db, k, counts)
        e = delta.numel()
        body = struct.pack("<BBIQ", 1, db, zero, e) + per_chunk.tobytes()
        bits = 0
        for arr, kk in ((delta, 1 << db), (sym, k)):
            if e:
                w, cb, ln, tb = encode_indices(arr, kk)
            else:
                w, cb, ln, tb = torch.empty(0, dtype=torch.int32, device=labels.device), np.zeros(0, np.uint32), np.zeros(kk, np.uint8), 0
            body += _stream_bytes(w, cb, ln, tb)
            bits += tb
        cands[name] = (body, bits)
    if not cands:
        raise ValueError(f"unknown index form {form!r}")
    best = min(cands, key=lambda nm: (len(cands[nm][0]), nm))
    return cands[best][0], cands[best][1], best


def _parse_indices(r: _Reader, k: int, n: int, lb: int):
    """The index part of a record (from the form byte on), checked on the host."""
    (form,) = r.take("<B")
    if form == 0:
        return ("dense", _parse_stream(r, k, n, "dense stream"))
    if form != 1:
        raise ValueError(f"form {form} is neither 0 (dense) nor 1 (sparse)")
    db, zero, e = r.take("<BIQ")
    if db not in (4, 8):
        raise ValueError(f"delta_bits {db} is neither 4 nor 8")
    if zero >= k:
        raise ValueError(f"zero_symbol {zero} >= K = {k}")
    if e > n:
        raise ValueError(f"entries {e} > N = {n}")
    nchunks = (n + CHUNK - 1) // CHUNK
    per_chunk = r.array(np.uint16, nchunks)
    if nchunks and int(per_chunk.max()) > CHUNK:
        raise ValueError(f"entries_in_chunk {int(per_chunk.max())} > {CHUNK}")
    if int(per_chunk.astype(np.int64).sum()) != e:
        raise ValueError("entries_in_chunk do not add up to the entries")
    delta = _parse_stream(r, 1 << db, e, "distance stream")
    sym = _parse_stream(r, k, e, "index stream")
    return ("sparse", zero, e, per_chunk, delta, sym)


def _decode_parsed_indices(parsed, n, lb, device):
    if parsed[0] == "dense":
        return _decode_stream(parsed[1], n, device, lb)
    _, zero, e, per_chunk, delta, sym = parsed
    return decode_sparse(_decode_stream(delta, e, device, 1), _decode_stream(sym, e, device, lb), per_chunk, n, zero)


def unpack_indices(blob, pos, k, n, lb, device):
    """The inverse of pack_indices: (indices device tensor, position behind them).  The header fields are checked before any
    device call (ValueError)."""
    r = _Reader(blob, pos)
    parsed = _parse_indices(r, k, n, lb)
    return _decode_parsed_indices(parsed, n, lb, device), r.pos


def pack_tensor(name: str, shape, model, raw: torch.Tensor | None = None, form: str = "auto", info: dict | None = None) -> bytes:
    """One record.  model: kmeans.QuantizedModel (or None with ``raw`` = the unquantized float32 tensor).  ``info`` (optional dict)
    receives what a report needs: n, bytes, stream bits, form."""
    nm = name.encode("utf-8")
    head = struct.pack("<H", len(nm)) + nm + struct.pack("<B", len(shape)) + b"".join(struct.pack("<Q", int(d)) for d in shape)
    n = int(np.prod(shape)) if len(shape) else 1
    if model is None:
        data = np.ascontiguousarray(raw.detach().cpu().numpy(), dtype=np.float32).reshape(-1)
        rec = head + struct.pack("<IBQQ", 0, 0, n, 0) + data.tobytes()
        if info is not None:
            info.update({"n": n, "bytes": len(rec), "stream_bits": 32 * n, "form": "raw", "k": 0})
        return rec
    k = int(model.cluster_centers_.size)
    labels = model.labels_compact_
    counts = model.counts_device_.cpu().numpy() if getattr(model, "counts_device_", None) is not None else None
    body_idx, total_bits, chosen = pack_indices(labels, k, counts, form)
    lb = ops._label_bytes(labels)
    body = struct.pack("<IBQQ", k, lb, n, total_bits)
    body += np.ascontiguousarray(model.cluster_centers_.ravel(), dtype=np.float32).tobytes()
    rec = head + body + body_idx
    if info is not None:
        info.update({"n": n, "bytes": len(rec), "stream_bits": int(total_bits), "form": chosen, "k": k})
    return rec


def save_compressed(path: str, tensors: Dict[str, Tuple[tuple, object, torch.Tensor | None]], form: str = "auto", report: dict | None = None) -> int:
    """tensors: name -> (shape, QuantizedModel | None, raw tensor if unquantized).  Returns the file size in bytes; ``report`` (optional
    dict) receives name -> {n, bytes, stream_bits, form, k} and, under "total", the whole file against 32 bits per weight."""
    blob = MAGIC + struct.pack("<I", len(tensors))
    total_n = 0
    for name, (shape, model, raw) in tensors.items():
        info = {}
        blob += pack_tensor(name, tuple(shape), model, raw, form, info)
        total_n += info["n"]
        if report is not None:
            info["bits_per_weight"] = 8.0 * info["bytes"] / max(info["n"], 1)
            report[name] = info
    with open(path, "wb") as f:
        f.write(blob)
    if report is not None:
        report["total"] = {"n": total_n, "bytes": len(blob), "bits_per_weight": 8.0 * len(blob) / max(total_n, 1),
                           "compression_ratio": 4.0 * total_n / max(len(blob), 1)}
    return len(blob)


def _parse_records(blob):
    """Every record of a stored blob, checked on the host before anything reaches the device: (name, shape, k, lb, n, payload)
    with payload the raw float32 array (K = 0) or (centers float32[K], parsed indices).  ValueError names the field at fault."""
    if blob[:4] != MAGIC:
        raise ValueError(f"magic {bytes(blob[:4])!r} is not {MAGIC!r} (files of the older NNC1 layout are not read)")
    r = _Reader(blob, 4)
    (nt,) = r.take("<I")
    out = []
    for _ in range(nt):
        (ln,) = r.take("<H")
        name = bytes(r.array(np.uint8, ln)).decode("utf-8")
        (nd,) = r.take("<B")
        shape = r.take("<" + "Q" * nd)
        k, lb, n, total_bits = r.take("<IBQQ")
        if n != math.prod(shape):
            raise ValueError(f"{name}: N = {n} is not the product of the shape {shape}")
        if k == 0:
            if lb != 0 or total_bits != 0:
                raise ValueError(f"{name}: a raw record (K = 0) has label_bytes {lb} and total_bits {total_bits}, not 0 and 0")
            out.append((name, shape, k, lb, n, r.array(np.float32, n)))
            continue
        if k > NNC_KMAX:
            raise ValueError(f"{name}: K = {k} is not in 1 .. {NNC_KMAX}")
        if lb not in (1, 2):
            raise ValueError(f"{name}: label_bytes {lb} is neither 1 nor 2")
        if lb == 1 and k > 256:
            raise ValueError(f"{name}: label_bytes 1 cannot hold the indices of K = {k} > 256")
        centers = r.array(np.float32, k)
        parsed = _parse_indices(r, k, n, lb)
        bits = parsed[1][3] if parsed[0] == "dense" else parsed[4][3] + parsed[5][3]
        if bits != total_bits:
            raise ValueError(f"{name}: total_bits {total_bits} is not the {bits} bits of its streams")
        out.append((name, shape, k, lb, n, (centers, parsed)))
    if r.pos != len(blob):
        raise ValueError(f"{len(blob) - r.pos} trailing bytes after the last record")
    return out


def _records(path: str, device):
    """(name, shape, value) per stored tensor: value = the raw float32 device tensor (K = 0) or (centers float32[K] host array,
    indices device tensor) decoded by the device decoders.  The whole file is checked before the first device call."""
    with open(path, "rb") as f:
        blob = f.read()
    for name, shape, k, lb, n, payload in _parse_records(blob):
        if k == 0:
            yield name, shape, torch.from_numpy(payload.copy()).to(device).reshape(shape)
            continue
        centers, parsed = payload
        yield name, shape, (centers, _decode_parsed_indices(parsed, n, lb, device))


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else device


def load_compressed(path: str, device=None) -> Dict[str, torch.Tensor]:
    """name -> decoded float32 tensor on the device: cluster_centers_[labels_] in the stored shape."""
    device = _device(device)
    out = {}
    for name, shape, value in _records(path, device):
        if isinstance(value, tuple):
            centers, labels = value
            value = ops.gather(torch.from_numpy(centers.copy()).to(device), labels).reshape(shape)
        out[name] = value
    return out


def load_compressed_codes(path: str, device=None) -> Dict[str, object]:
    """name -> (shape, centers float32[K] on the device, centroid indices uint8 / 16-bit on the device) without decoding the
    weights (what compressed.load_network runs from), or the raw float32 tensor of a record stored unquantized (K = 0)."""
    device = _device(device)
    out = {}
    for name, shape, value in _records(path, device):
        if isinstance(value, tuple):
            centers, labels = value
            value = (tuple(int(d) for d in shape), torch.from_numpy(centers.copy()).to(device), labels)
        out[name] = value
    return out
