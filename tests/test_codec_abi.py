"""CPU checks of the index codecs' host halves (include/nnc.h: nnc_huffman_codes, nnc_huffman_decode_tables, nnc_huffman_lengths)
against the plain references in tests/helpers/codec_ref.py, and of storage.py's header checks on hand-built files: every field a
record carries is checked on the host, so a malformed file raises ValueError before anything reaches a device."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from tests.helpers import codec_ref

NNC_EINVAL = -1
KMAX = 1040
TABLE_BYTES = 3 * 33 * 4 + KMAX * 2


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


@pytest.fixture(scope="module")
def mods(lib):
    from neural_network_compression_amd import ops, storage

    return ops, storage


def _u8p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def lib_codes(lib, lengths):
    lengths = np.ascontiguousarray(lengths, dtype=np.uint8)
    codes = np.full(max(lengths.size, 1), 0xDEADBEEF, dtype=np.uint32)
    rc = lib.nnc_huffman_codes(_u8p(lengths), lengths.size, codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return rc, codes[: lengths.size]


def lib_tables(lib, lengths, k=None, nbytes=TABLE_BYTES, pad=64):
    """nnc_huffman_decode_tables into a buffer framed by 0xA5 bytes; returns (rc, the table bytes, the frame intact?)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint8)
    buf = np.full(nbytes + 2 * pad, 0xA5, dtype=np.uint8)
    rc = lib.nnc_huffman_decode_tables(_u8p(lengths), lengths.size if k is None else k, buf[pad:].ctypes.data, nbytes)
    frame = bool((buf[:pad] == 0xA5).all() and (buf[pad + nbytes:] == 0xA5).all())
    return rc, buf[pad: pad + nbytes].tobytes(), frame


def complete_lengths(rng, k, maxlen=32):
    """A random Kraft-complete length set of k symbols: split random leaves of a full binary tree, no leaf deeper than maxlen."""
    leaves = [1, 1]
    while len(leaves) < k:
        cand = [i for i, l in enumerate(leaves) if l < maxlen]
        i = cand[rng.randint(len(cand))]
        leaves[i] += 1
        leaves.insert(i + 1, leaves[i])
    out = np.array(leaves[:k], dtype=np.uint8)
    rng.shuffle(out)
    return out


def _length_sets():
    rng = np.random.RandomState(7)
    sets = {
        "k1_len1": np.array([1]), "k1_len32": np.array([32]),
        "chain_1_to_32": np.array(list(range(1, 33)) + [32]),
        "chain_reversed": np.array([32] + list(range(32, 0, -1))),
        "all32_k1040": np.full(KMAX, 32),
        "one_and_32s": np.array([1] + [32] * 300),
        "zeros_between": np.array([0, 3, 0, 0, 1, 3, 0, 2, 0, 0, 0, 0]),
        "k1040_two_lengths": np.array([10] * 1008 + [11] * 32),   # 1008 / 1024 + 32 / 2048 = 1: complete
    }
    for i, k in enumerate((2, 3, 17, 256, 257, 1040)):
        sets[f"complete_k{k}"] = complete_lengths(rng, k)
        inc = complete_lengths(rng, k)
        inc[rng.randint(k)] = 0                                           # one symbol unused
        if k > 2:
            j = int(np.argmin(np.where(inc > 0, inc, 99)))
            inc[j] += 1                                                   # and one code a bit longer than it needs
        sets[f"incomplete_k{k}"] = inc
    return sets


LENGTH_SETS = _length_sets()


@pytest.mark.parametrize("name", sorted(LENGTH_SETS))
def test_canonical_codes_match_the_reference(lib, name):
    lengths = LENGTH_SETS[name].astype(np.uint8)
    rc, codes = lib_codes(lib, lengths)
    assert rc == nat.NNC_OK
    want = codec_ref.canonical_codes(lengths)
    assert np.array_equal(codes, want)
    assert codec_ref.kraft_ok(lengths)
    if name == "chain_1_to_32":
        assert int(codes[-1]) == 0xFFFFFFFF and int(codes[-2]) == 0xFFFFFFFE and int(codes[0]) == 0


@pytest.mark.parametrize("name", sorted(LENGTH_SETS))
def test_decode_tables_match_the_reference_byte_for_byte(lib, name):
    lengths = LENGTH_SETS[name].astype(np.uint8)
    assert lib.nnc_huffman_decode_tables_bytes() == TABLE_BYTES
    rc, got, frame = lib_tables(lib, lengths, nbytes=TABLE_BYTES)
    assert rc == nat.NNC_OK and frame
    assert got == codec_ref.decode_tables(lengths)
    # a larger buffer: the tables take the same bytes, nothing behind them is written
    rc, got2, _ = lib_tables(lib, lengths, nbytes=TABLE_BYTES + 40)
    assert rc == nat.NNC_OK and got2[:TABLE_BYTES] == got and got2[TABLE_BYTES:] == b"\xa5" * 40


@pytest.mark.parametrize("lengths", [[33], [1, 33], [2, 2, 2, 40], [1, 1, 1], [2, 2, 2, 2, 3], [32] * 3 + [1, 1], [1, 2, 2, 32]])
def test_bad_lengths_are_einval(lib, lengths):
    """A length over 32 bits, or lengths that violate Kraft's inequality: EINVAL from both host functions, tables untouched."""
    lengths = np.array(lengths, dtype=np.uint8)
    assert not codec_ref.kraft_ok(lengths)
    rc, _ = lib_codes(lib, lengths)
    assert rc == NNC_EINVAL
    rc, got, frame = lib_tables(lib, lengths)
    assert rc == NNC_EINVAL and frame
    if int(lengths.max()) <= 32:
        with pytest.raises(ValueError):
            codec_ref.canonical_codes(lengths)


def test_bad_arguments_are_einval(lib):
    ok = np.full(KMAX + 1, 11, dtype=np.uint8)
    codes = np.zeros(KMAX + 1, dtype=np.uint32)
    cp = codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert lib.nnc_huffman_codes(_u8p(ok), 0, cp) == NNC_EINVAL
    assert lib.nnc_huffman_codes(_u8p(ok), KMAX + 1, cp) == NNC_EINVAL
    assert lib.nnc_huffman_codes(_u8p(ok), KMAX, cp) == nat.NNC_OK
    for k, nbytes in ((KMAX + 1, TABLE_BYTES), (0, TABLE_BYTES), (4, TABLE_BYTES - 1), (4, 0)):
        rc, got, frame = lib_tables(lib, ok, k=k, nbytes=max(nbytes, 0))
        assert rc == NNC_EINVAL and frame and got == b"\xa5" * nbytes, (k, nbytes)


def fib_counts(m):
    c = [1, 1]
    while len(c) < m:
        c.append(c[-1] + c[-2])
    return np.array(c[:m], dtype=np.int64)


@pytest.mark.parametrize("m", [33, 34, 36])
def test_fibonacci_histograms_reach_and_pass_32_bits(mods, m):
    """Fibonacci counts make the Huffman tree a chain: 33 symbols give codes of exactly 32 bits, kept as they are; 34 and 36 give
    33 and 35 bits, which storage._flatten_lengths replaces by a fixed width over the used symbols (still a prefix code)."""
    ops, storage = mods
    counts = fib_counts(m)
    lengths, hist, total = ops.huffman_lengths(counts)
    assert int(lengths.max()) == m - 1 and total == int((counts * lengths.astype(np.int64)).sum())
    flat = storage._flatten_lengths(np.ascontiguousarray(lengths, dtype=np.uint8), counts)
    if m == 33:
        assert flat is lengths or np.array_equal(flat, lengths)
        assert int(flat.max()) == 32 and codec_ref.kraft_ok(flat)
        assert sorted(flat.tolist()) == list(range(1, 32)) + [32, 32]
        return
    width = math.ceil(math.log2(m))
    assert set(flat.tolist()) == {width} and codec_ref.kraft_ok(flat)
    assert int((counts * flat.astype(np.int64)).sum()) == width * int(counts.sum())
    codes = codec_ref.canonical_codes(flat)
    assert np.array_equal(codes, np.arange(m))                               # a fixed-width code: symbol s is s
    rc, lc = lib_codes(nat.load(), flat)
    assert rc == nat.NNC_OK and np.array_equal(lc, codes)
    # an unused symbol among them keeps length 0; the width follows the used symbols only
    c2 = np.insert(counts, 5, 0)
    l2 = storage._flatten_lengths(np.ascontiguousarray(ops.huffman_lengths(c2)[0], dtype=np.uint8), c2)
    assert l2[5] == 0 and set(np.delete(l2, 5).tolist()) == {width}


# ------------------------------------------------------------------ the references themselves, against the bit-by-bit loops
def _loop_stream(labels, lengths):
    codes = codec_ref.canonical_codes(lengths)
    bits = []
    for s in labels:
        c, l = int(codes[int(s)]), int(lengths[int(s)])
        bits.extend((c >> (l - 1 - i)) & 1 for i in range(l))
    return np.array(bits, dtype=np.uint8)


@pytest.mark.parametrize("name", ["chain_1_to_32", "all32_k1040", "zeros_between", "complete_k257", "incomplete_k17", "k1_len32"])
def test_reference_stream_equals_a_bit_by_bit_loop(name):
    lengths = LENGTH_SETS[name].astype(np.int64)
    rng = np.random.RandomState(len(name))
    used = np.flatnonzero(lengths)
    labels = used[rng.randint(used.size, size=3001)]
    bits = codec_ref.stream_bits(labels, lengths, block=257)
    assert np.array_equal(bits, _loop_stream(labels, lengths))
    words, nb = codec_ref.stream_words(labels, lengths)
    assert nb == bits.size and np.array_equal(codec_ref.words_to_bits(words)[:nb], bits)
    off = codec_ref.chunk_offsets(labels, lengths)
    assert off[-1] == nb and off.size == (labels.size + 1023) // 1024 + 1
    assert off[1] == int(lengths[labels[:1024]].sum())
    lead = 13
    w2 = codec_ref.bits_to_words(bits, lead)
    assert np.array_equal(codec_ref.words_to_bits(w2)[lead: lead + nb], bits) and int(w2[0]) >> (32 - lead) == 0


@pytest.mark.parametrize("dbits", range(1, 9))
def test_reference_sparse_entries_equal_the_loop(dbits):
    rng = np.random.RandomState(dbits)
    n = 5 * 1024 + 77
    lab = np.where(rng.rand(n) < 0.05, rng.randint(0, 9, size=n), 4)
    lab[1023] = 1; lab[1024] = 2; lab[2047] = 3                           # chunk ends and starts
    lab[3 * 1024: 4 * 1024] = 4                                           # an empty chunk
    for got, want in zip(codec_ref.sparse_entries(lab, 4, dbits), codec_ref.sparse_entries_loop(lab, 4, dbits)):
        assert np.array_equal(got, want)


# ------------------------------------------------------------------ storage.py: every header field is checked on the host
def _lengths_of(ops, storage):
    def f(counts):
        counts = np.asarray(counts, dtype=np.int64)
        return storage._flatten_lengths(np.ascontiguousarray(ops.huffman_lengths(counts)[0], dtype=np.uint8), counts)
    return f


NAME = "layer.w"


def _dense_file(ops, storage):
    rng = np.random.RandomState(3)
    shape, k = (40, 70), 16
    lab = rng.randint(0, k, size=math.prod(shape))
    lab[:500] = 3
    centers = np.linspace(-1, 1, k).astype(np.float32)
    return codec_ref.file_bytes([codec_ref.record(NAME, shape, centers, lab, _lengths_of(ops, storage))]), lab, k, shape


def _sparse_file(ops, storage):
    rng = np.random.RandomState(4)
    shape, k, zero = (5000,), 300, 7
    lab = np.where(rng.rand(shape[0]) < 0.1, rng.randint(0, k, size=shape[0]), zero)
    centers = np.linspace(-1, 1, k).astype(np.float32)
    rec = codec_ref.record(NAME, shape, centers, lab, _lengths_of(ops, storage), form="sparse", zero=zero, dbits=4)
    return codec_ref.file_bytes([rec]), lab, k, shape


def _offsets(blob, shape, k):
    """Byte offsets of the fields of the first record (storage.py's layout)."""
    o = {"magic": 0, "n_tensors": 4}
    p = 8 + 2 + len(NAME)
    o["ndim"] = p
    o["shape"] = p + 1
    p += 1 + 8 * len(shape)
    o.update(K=p, label_bytes=p + 4, N=p + 5, total_bits=p + 13, centers=p + 21)
    p += 21 + 4 * k
    o["form"] = p
    nchunks = -(-math.prod(shape) // 1024)
    if blob[p] == 0:
        o.update(stream=p + 1, lengths=p + 9, chunk_bits=p + 9 + k)
    else:
        o.update(delta_bits=p + 1, zero_symbol=p + 2, entries=p + 6, entries_in_chunk=p + 14)
        q = p + 14 + 2 * nchunks
        o.update(delta_stream=q, delta_lengths=q + 8, delta_chunk_bits=q + 8 + 16)
    return o


@pytest.fixture
def no_device(mods, monkeypatch):
    """storage's device decoders replaced by recorders: the header checks must run before either is reached."""
    _, storage = mods
    calls = []

    def fake_indices(words, chunk_bits, n, lengths, k, label_bytes):
        calls.append(("indices", words.cpu().numpy().copy(), np.asarray(chunk_bits).copy(), n, np.asarray(lengths).copy(), k, label_bytes))
        return torch.zeros(n, dtype=torch.uint8 if label_bytes == 1 else torch.int16)

    def fake_sparse(delta, sym, entries_in_chunk, n, zero_symbol):
        calls.append(("sparse", n, zero_symbol))
        return torch.zeros(n, dtype=sym.dtype)

    monkeypatch.setattr(storage, "decode_indices", fake_indices)
    monkeypatch.setattr(storage, "decode_sparse", fake_sparse)
    return calls


def _load(storage, tmp_path, blob):
    p = tmp_path / "one.nnc"
    p.write_bytes(bytes(blob))
    return storage.load_compressed_codes(str(p), device=torch.device("cpu"))


def test_well_formed_hand_built_files_reach_the_decoders(mods, no_device, tmp_path):
    """The positive control of the checks below: both hand-built files pass them, and the dense stream handed to the decoder is
    the reference's."""
    ops, storage = mods
    blob, lab, k, shape = _dense_file(ops, storage)
    got = _load(storage, tmp_path, blob)
    assert list(got) == [NAME] and got[NAME][0] == shape
    (call,) = no_device
    lengths = _lengths_of(ops, storage)(np.bincount(lab, minlength=k))
    words, nb = codec_ref.stream_words(lab, lengths)
    assert call[0] == "indices" and np.array_equal(call[1].view(np.uint32), words) and call[3] == lab.size and call[5:] == (k, 1)
    assert np.array_equal(call[2], np.diff(codec_ref.chunk_offsets(lab, lengths)))
    no_device.clear()
    blob, lab, k, shape = _sparse_file(ops, storage)
    _load(storage, tmp_path, blob)
    assert [c[0] for c in no_device] == ["indices", "indices", "sparse"] and no_device[-1][1:] == (lab.size, 7)


def _put(blob, off, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, value)
    return b


def _dense_mutations(blob, o, k):
    cb0 = struct.unpack_from("<I", blob, o["chunk_bits"])[0]
    return {
        "magic": (bytearray(b"NNC1" + blob[4:]), "magic"),
        "K over KMAX": (_put(blob, o["K"], "<I", KMAX + 1), "K ="),
        "K over 256 in one byte": (_put(blob, o["K"], "<I", 257), "label_bytes 1"),
        "label_bytes 0": (_put(blob, o["label_bytes"], "<B", 0), "label_bytes"),
        "label_bytes 3": (_put(blob, o["label_bytes"], "<B", 3), "label_bytes"),
        "N": (_put(blob, o["N"], "<Q", 2801), "N ="),
        "ndim": (_put(blob, o["ndim"], "<B", 1), "N ="),
        "shape": (_put(blob, o["shape"], "<Q", 41), "N ="),
        "record total_bits": (_put(blob, o["total_bits"], "<Q", struct.unpack_from("<Q", blob, o["total_bits"])[0] + 1), "total_bits"),
        "form": (_put(blob, o["form"], "<B", 2), "form"),
        "code length 33": (_put(blob, o["lengths"] + 5, "<B", 33), "code_length"),
        "Kraft": (_put(_put(_put(blob, o["lengths"], "<B", 1), o["lengths"] + 1, "<B", 1), o["lengths"] + 2, "<B", 1), "Kraft"),
        "chunk over 32 * 1024 bits": (_put(blob, o["chunk_bits"], "<I", 32 * 1024 + 1), "chunk_bits"),
        "chunk sum": (_put(blob, o["chunk_bits"], "<I", cb0 + 1), "chunk_bits"),
        "stream bits": (_put(blob, o["stream"], "<Q", struct.unpack_from("<Q", blob, o["stream"])[0] - 32), "chunk_bits"),
        "n_tensors": (_put(blob, o["n_tensors"], "<I", 2), "truncated"),
        "truncated": (bytearray(blob[:-1]), "truncated"),
        "truncated header": (bytearray(blob[: o["N"] + 3]), "truncated"),
        "trailing bytes": (bytearray(blob + b"\0"), "trailing"),
    }


def _sparse_mutations(blob, o, k):
    e = struct.unpack_from("<Q", blob, o["entries"])[0]
    pc0 = struct.unpack_from("<H", blob, o["entries_in_chunk"])[0]
    out = {f"delta_bits {db}": (_put(blob, o["delta_bits"], "<B", db), "delta_bits") for db in (0, 1, 2, 3, 5, 7, 9, 255)}
    out.update({
        "zero_symbol K": (_put(blob, o["zero_symbol"], "<I", k), "zero_symbol"),
        "zero_symbol huge": (_put(blob, o["zero_symbol"], "<I", 0xFFFFFFFF), "zero_symbol"),
        "entries over N": (_put(blob, o["entries"], "<Q", 5001), "entries"),
        "entries sum": (_put(blob, o["entries"], "<Q", e - 1), "entries_in_chunk"),
        "entries_in_chunk over 1024": (_put(blob, o["entries_in_chunk"], "<H", 1025), "entries_in_chunk"),
        "entries_in_chunk sum": (_put(blob, o["entries_in_chunk"], "<H", pc0 + 1), "entries_in_chunk"),
        "delta code length 33": (_put(blob, o["delta_lengths"], "<B", 33), "code_length"),
        "delta chunk over 32 * 1024 bits": (_put(blob, o["delta_chunk_bits"], "<I", 32 * 1024 + 1), "chunk_bits"),
        "record total_bits": (_put(blob, o["total_bits"], "<Q", 0), "total_bits"),
        "label_bytes 1 with K 300": (_put(blob, o["label_bytes"], "<B", 1), "label_bytes 1"),
        "truncated": (bytearray(blob[:-3]), "truncated"),
        "trailing bytes": (bytearray(blob + b"\0" * 8), "trailing"),
    })
    return out


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_every_malformed_header_field_raises_before_the_device(mods, no_device, tmp_path, form):
    ops, storage = mods
    blob, lab, k, shape = (_dense_file if form == "dense" else _sparse_file)(ops, storage)
    o = _offsets(blob, shape, k)
    muts = (_dense_mutations if form == "dense" else _sparse_mutations)(blob, o, k)
    for what, (bad, match) in muts.items():
        assert bytes(bad) != blob, what
        with pytest.raises(ValueError, match=match):
            _load(storage, tmp_path, bad)
        assert no_device == [], what
    _load(storage, tmp_path, blob)                 # unchanged, the file still passes
    assert no_device


def test_raw_record_fields_are_checked(mods, no_device, tmp_path):
    _, storage = mods
    data = np.arange(12, dtype=np.float32).reshape(3, 4)
    blob = codec_ref.file_bytes([codec_ref.raw_record("b", data)])
    got = _load(storage, tmp_path, blob)
    assert np.array_equal(got["b"].numpy(), data)
    p = 8 + 2 + 1 + 1 + 16                                    # K of the raw record
    for off, fmt, v, match in ((p + 4, "<B", 1, "raw record"), (p + 13, "<Q", 5, "raw record"), (p + 5, "<Q", 13, "N ="),
                               (p + 5, "<Q", 1 << 40, "N =")):
        with pytest.raises(ValueError, match=match):
            _load(storage, tmp_path, _put(blob, off, fmt, v))
    with pytest.raises(ValueError, match="truncated"):
        _load(storage, tmp_path, blob[:-4])
    assert no_device == []
