"""Plain NumPy references of the index codecs (csrc/nnc_codec.hip, storage.py), built from their definitions and independent of
the library's tables: canonical Huffman codes, the MSB-first word stream, chunk bit counts, the decode-table layout of
nnc_huffman_decode_tables, the relative-index entries, and whole stored records (storage.py's file layout) for hand-built files."""
import math
import struct

import numpy as np

CHUNK = 1024
KMAX = 1040
MAXLEN = 32


def canonical_codes(lengths):
    """uint32[k] canonical codes: symbols with a length > 0 ordered by (length, symbol), each code the previous one + 1, shifted
    left when the length grows.  Raises ValueError if a code does not fit in its length (Kraft's inequality violated)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    codes = np.zeros(lengths.size, dtype=np.uint32)
    used = np.flatnonzero(lengths > 0)
    code, prev = 0, 0
    for s in used[np.lexsort((used, lengths[used]))]:
        l = int(lengths[s])
        code <<= l - prev
        if code >= 1 << l:
            raise ValueError("the lengths violate Kraft's inequality")
        codes[s] = code
        code += 1
        prev = l
    return codes


def kraft_ok(lengths) -> bool:
    """All lengths <= 32 and sum of 2^-l over the used symbols <= 1 (in integers: 2^(32 - l) summed <= 2^32)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.size and int(lengths.max()) > MAXLEN:
        return False
    used = lengths[lengths > 0]
    return int(sum(1 << (MAXLEN - int(l)) for l in used)) <= 1 << MAXLEN


def chunk_offsets(labels, lengths):
    """int64[nchunks + 1]: the first bit of every chunk of 1024 indices, then the total."""
    labels = np.asarray(labels)
    per = np.asarray(lengths, dtype=np.uint8)[labels]
    nchunks = (labels.size + CHUNK - 1) // CHUNK
    padded = np.zeros(nchunks * CHUNK, dtype=np.uint8)
    padded[: per.size] = per
    off = np.zeros(nchunks + 1, dtype=np.int64)
    np.cumsum(padded.reshape(nchunks, CHUNK).sum(axis=1, dtype=np.int64), out=off[1:])
    return off


def stream_bits(labels, lengths, codes=None, block=1 << 18):
    """The code bits of ``labels`` one after the other (uint8 0/1 per bit), MSB of every code first.  Vectorised: every symbol's
    code is repeated over its length and each bit picked by its position inside the code (a cumsum of the lengths)."""
    labels = np.asarray(labels).astype(np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    if codes is None:
        codes = canonical_codes(lengths)
    codes = np.asarray(codes, dtype=np.uint64)
    per = lengths[labels]
    out = np.zeros(int(per.sum()), dtype=np.uint8)
    pos = 0
    for lo in range(0, labels.size, block):
        l = per[lo: lo + block]
        c = codes[labels[lo: lo + block]]
        m = int(l.sum())
        start = np.cumsum(l) - l
        j = np.arange(m, dtype=np.int64) - np.repeat(start, l)           # bit index inside its code, 0 = MSB
        shift = (np.repeat(l, l) - 1 - j).astype(np.uint64)
        out[pos: pos + m] = (np.repeat(c, l) >> shift) & np.uint64(1)
        pos += m
    return out


def bits_to_words(bits, lead=0):
    """uint32 words of an MSB-first bit string that starts ``lead`` bits into its first word (zero padded on both ends)."""
    nb = lead + bits.size
    buf = np.zeros(((nb + 31) // 32) * 32, dtype=np.uint8)
    buf[lead: nb] = bits
    return np.packbits(buf).view(">u4").astype(np.uint32)


def words_to_bits(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).astype(">u4").view(np.uint8))


def stream_words(labels, lengths, codes=None):
    """(uint32 words ceil(bits / 32), total bits) of the whole stream."""
    bits = stream_bits(labels, lengths, codes)
    return bits_to_words(bits), int(bits.size)


def decode_tables(lengths, kmax=KMAX):
    """The bytes nnc_huffman_decode_tables writes: uint32 first_code[33], count[33], first_index[33] (index 0 unused, zero), then
    uint16 symbols[kmax] ordered by (length, symbol), zero behind the used ones.  first_code[l] is the canonical first code of
    length l truncated to 32 bits, also for lengths nobody has."""
    lengths = np.asarray(lengths, dtype=np.int64)
    cn = np.zeros(MAXLEN + 1, dtype=np.int64)
    for l in lengths[lengths > 0]:
        cn[int(l)] += 1
    fc = np.zeros(MAXLEN + 1, dtype=np.uint32)
    fi = np.zeros(MAXLEN + 1, dtype=np.uint32)
    code, idx = 0, 0
    for l in range(1, MAXLEN + 1):
        code = (code + int(cn[l - 1])) << 1
        fc[l] = code & 0xFFFFFFFF
        fi[l] = idx
        idx += int(cn[l])
    codes = canonical_codes(lengths)
    for l in range(1, MAXLEN + 1):       # the recurrence agrees with the codes themselves where a length is used
        if cn[l]:
            assert int(fc[l]) == int(codes[lengths == l].min())
    used = np.flatnonzero(lengths > 0)
    syms = np.zeros(kmax, dtype=np.uint16)
    syms[: used.size] = used[np.lexsort((used, lengths[used]))]
    return fc.tobytes() + cn.astype(np.uint32).tobytes() + fi.tobytes() + syms.tobytes()


def sparse_entries_loop(lab, zero, dbits):
    """The entries position by position in plain Python: (distance - 1, index) per stored position, filler entries
    (distance 2^dbits, index = zero) for longer gaps, distances restarting at every chunk of 1024 positions."""
    D = 1 << dbits
    deltas, syms, per_chunk = [], [], []
    for base in range(0, len(lab), CHUNK):
        prev, cnt = base - 1, 0
        for i in range(base, min(base + CHUNK, len(lab))):
            if lab[i] == zero:
                continue
            gap = i - prev
            while gap > D:
                deltas.append(D - 1); syms.append(zero); gap -= D; cnt += 1
            deltas.append(gap - 1); syms.append(int(lab[i])); cnt += 1
            prev = i
        per_chunk.append(cnt)
    return np.array(deltas, dtype=np.int64), np.array(syms, dtype=np.int64), np.array(per_chunk, dtype=np.int64)


def sparse_entries(lab, zero, dbits):
    """sparse_entries_loop vectorised: int64 (distance - 1 per entry, index per entry, entries per chunk)."""
    lab = np.asarray(lab).astype(np.int64)
    D = 1 << dbits
    nchunks = (lab.size + CHUNK - 1) // CHUNK
    nz = np.flatnonzero(lab != zero)
    chunk = nz // CHUNK
    prev = np.empty_like(nz)
    prev[1:] = nz[:-1]
    first = np.ones(nz.size, dtype=bool)
    first[1:] = chunk[1:] != chunk[:-1]
    prev[first] = chunk[first] * CHUNK - 1                 # the position in front of a chunk counts as stored
    gap = nz - prev
    fill = (gap - 1) >> dbits
    ent = fill + 1
    ends = np.cumsum(ent) - 1                               # a stored position's own entry closes its group
    delta = np.full(int(ent.sum()), D - 1, dtype=np.int64)
    sym = np.full(int(ent.sum()), zero, dtype=np.int64)
    delta[ends] = gap - fill * D - 1
    sym[ends] = lab[nz]
    per_chunk = np.bincount(chunk, weights=ent, minlength=nchunks).astype(np.int64)
    return delta, sym, per_chunk


# ------------------------------------------------------------------ whole records of storage.py's file layout, built on the host
def _stream_record(labels, lengths):
    """STREAM(k, n) = u64 bits | u8 code_length[k] | u32 chunk_bits[ceil(n / 1024)] | u32 words[ceil(bits / 32)]."""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint8)
    off = chunk_offsets(labels, lengths)
    words, bits = stream_words(labels, lengths)
    return struct.pack("<Q", bits) + lengths.tobytes() + np.diff(off).astype(np.uint32).tobytes() + words.tobytes(), bits


def index_bytes(labels, k, lengths_of, form="dense", zero=None, dbits=4):
    """The index part of a record, from its form byte on (what storage.pack_indices returns), and its stream bits.
    ``lengths_of(counts)`` gives the code lengths for a histogram (the library's rule: ops.huffman_lengths +
    storage._flatten_lengths); form "dense" or "sparse" (delta_bits ``dbits``, zero cluster ``zero``)."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    if form == "dense":
        body, bits = _stream_record(labels, lengths_of(np.bincount(labels, minlength=k)))
        return struct.pack("<B", 0) + body, bits
    delta, sym, per_chunk = sparse_entries(labels, zero, dbits)
    e = delta.size
    idx = struct.pack("<BBIQ", 1, dbits, zero, e) + per_chunk.astype(np.uint16).tobytes()
    bits = 0
    for arr, kk in ((delta, 1 << dbits), (sym, k)):
        if e:
            body, b = _stream_record(arr, lengths_of(np.bincount(arr, minlength=kk)))
        else:
            body, b = struct.pack("<Q", 0) + np.zeros(kk, np.uint8).tobytes(), 0
        idx += body
        bits += b
    return idx, bits


def record(name, shape, centers, labels, lengths_of, form="dense", zero=None, dbits=4):
    """One record of a quantized tensor (index part: index_bytes)."""
    centers = np.ascontiguousarray(centers, dtype=np.float32).ravel()
    labels = np.asarray(labels).astype(np.int64).ravel()
    k, n = centers.size, labels.size
    lb = 1 if k <= 256 else 2
    nm = name.encode("utf-8")
    head = struct.pack("<H", len(nm)) + nm + struct.pack("<B", len(shape)) + b"".join(struct.pack("<Q", int(d)) for d in shape)
    assert n == math.prod(shape)
    idx, bits = index_bytes(labels, k, lengths_of, form, zero, dbits)
    return head + struct.pack("<IBQQ", k, lb, n, bits) + centers.tobytes() + idx


def raw_record(name, data):
    data = np.ascontiguousarray(data, dtype=np.float32)
    nm = name.encode("utf-8")
    head = struct.pack("<H", len(nm)) + nm + struct.pack("<B", data.ndim) + b"".join(struct.pack("<Q", int(d)) for d in data.shape)
    return head + struct.pack("<IBQQ", 0, 0, data.size, 0) + data.tobytes()


def file_bytes(records):
    return b"NNC2" + struct.pack("<I", len(records)) + b"".join(records)
