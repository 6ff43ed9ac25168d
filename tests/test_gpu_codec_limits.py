"""The index codecs (csrc/nnc_codec.hip) at their limits, against the plain references of tests/helpers/codec_ref.py, through the
raw C ABI with buffers the test owns (run with -m gpu).

Every output -- the chunk-offset array, the word stream, the decoded labels, the sparse entries -- is a slice of a larger buffer
filled with a sentinel: nothing outside a slice may change, the words between the stream's end and the nwords the encoder was given
must be zero, and a second encode must give the same words.  Covered: codes of 31 and 32 bits at every bit offset and across the
1024-index chunk boundaries, the decoder's look-ahead word, K up to NNC_KMAX, label views off alignment, n = 0, a stream beyond 2^32
bits, the flattened fixed-width branch of storage._flatten_lengths, every delta_bits of the relative-index form with the chunk
shapes where it goes wrong, and storage.pack_indices / unpack_indices in all three forms."""
import ctypes
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import codec_ref  # noqa: E402

CHUNK = 1024
KMAX = 1040
W_SENT = 0x7FA5A5A5                    # int32 sentinel around the word stream
O_SENT = 0x5A5A5A5A5A5A5A5A            # int64 sentinel around the chunk / entry offsets
L_SENT = {1: 0xA5, 2: 0x5A5A}          # label sentinels: above every K the width allows
PAD = 37                               # sentinel elements on each side (odd: the slices are only element-aligned)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops, storage

    L = _native.load()
    return L, _native, ops, storage


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _framed(n, dtype, sentinel, off=0):
    """A buffer of PAD + off + n + PAD elements filled with ``sentinel``; returns (buffer, the n-element slice at PAD + off)."""
    buf = torch.full((PAD + off + n + PAD,), sentinel, dtype=dtype, device="cuda") if dtype != torch.int16 else \
        torch.full((PAD + off + n + PAD,), np.int16(np.uint16(sentinel)).item(), dtype=dtype, device="cuda")
    return buf, buf[PAD + off: PAD + off + n]


def _frame_intact(buf, lo, n, sentinel):
    host = buf.cpu().numpy()
    if host.dtype == np.int16:
        host = host.view(np.uint16)
    host = host.astype(np.uint64)
    s = np.uint64(sentinel)
    return bool((host[:lo] == s).all() and (host[lo + n:] == s).all())


def _labels_dev(lab, lb, off):
    """The indices as uint8 / int16 starting ``off`` elements into a device buffer (odd ``off``: off alignment)."""
    dt = torch.uint8 if lb == 1 else torch.int16
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.zeros(off + host.size + 8, dtype=dt, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return buf[off: off + host.size]


def _as_int(t, lb):
    h = t.cpu().numpy()
    return h.astype(np.int64) if lb == 1 else h.view(np.uint16).astype(np.int64)


def encode_raw(env, lab_d, lb, lengths, k, repeat=True):
    """nnc_huffman_chunk_offsets + nnc_huffman_encode into framed buffers; checks the frames, the zero tail and a repeat.
    Returns (chunk offsets int64 host, the framed word buffer, nwords of the stream)."""
    L, nat = env[0], env[1]
    n = lab_d.numel()
    lengths = np.ascontiguousarray(lengths, dtype=np.uint8)
    codes = codec_ref.canonical_codes(lengths)
    len_d = torch.from_numpy(lengths).cuda()
    codes_d = torch.from_numpy(codes.view(np.int32)).cuda()
    nchunks = int(L.nnc_codec_chunks(n))
    assert nchunks == (n + CHUNK - 1) // CHUNK
    obuf, off = _framed(nchunks + 1, torch.int64, np.int64(np.uint64(O_SENT)).item())
    nat.check(L.nnc_huffman_chunk_offsets(lab_d.data_ptr(), lb, n, len_d.data_ptr(), k, off.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _frame_intact(obuf, PAD, nchunks + 1, O_SENT), "a store outside the chunk offsets"
    off_h = off.cpu().numpy()
    total = int(off_h[-1])
    nwords = total // 32 + 2                      # what the header asks for
    sw = (total + 31) // 32
    wbuf, words = _framed(nwords, torch.int32, W_SENT)
    first = None
    for _ in range(2 if repeat else 1):
        nat.check(L.nnc_huffman_encode(lab_d.data_ptr(), lb, n, codes_d.data_ptr(), len_d.data_ptr(), k, off.data_ptr(), words.data_ptr(),
                                       nwords, _stream()))
        torch.cuda.synchronize()
        assert bool((wbuf[:PAD] == W_SENT).all()) and bool((wbuf[PAD + nwords:] == W_SENT).all()), "a store outside the words"
        assert not bool(words[sw:].ne(0).any()), "words behind the stream are not zero"
        if first is None:
            first = words.clone() if repeat else None
        else:
            assert torch.equal(first, words), "a repeated encode gave other words"
    return off_h, wbuf, sw


def decode_raw(env, words_d, off_h, n, lengths, k, lb, out_off):
    """nnc_huffman_decode of ``words_d`` (the stream plus its one look-ahead word) into framed labels; returns (labels, bad)."""
    L, nat = env[0], env[1]
    tb = int(L.nnc_huffman_decode_tables_bytes())
    tables = np.zeros(tb, dtype=np.uint8)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint8)
    nat.check(L.nnc_huffman_decode_tables(lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), k, tables.ctypes.data, tb))
    tables_d = torch.from_numpy(tables).cuda()
    off_d = torch.from_numpy(np.ascontiguousarray(off_h, dtype=np.int64)).cuda()
    dt = torch.uint8 if lb == 1 else torch.int16
    lbuf, out = _framed(n, dt, L_SENT[lb], out_off)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    nat.check(L.nnc_huffman_decode(words_d.data_ptr(), off_d.data_ptr(), n, tables_d.data_ptr(), k, out.data_ptr(), lb, bad.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _frame_intact(lbuf, PAD + out_off, n, L_SENT[lb]), "a store outside the decoded labels"
    return out, int(bad.item())


def roundtrip(env, lab, lb, lengths, k, in_off, out_off):
    """Encode ``lab`` through the raw ABI, compare offsets and words with the reference bit for bit, decode, compare the labels."""
    lab_d = _labels_dev(lab, lb, in_off)
    off_h, wbuf, sw = encode_raw(env, lab_d, lb, lengths, k)
    assert np.array_equal(off_h, codec_ref.chunk_offsets(lab, lengths))
    want, nb = codec_ref.stream_words(lab, lengths)
    assert nb == int(off_h[-1]) and want.size == sw
    assert np.array_equal(wbuf[PAD: PAD + sw].cpu().numpy().view(np.uint32), want)
    # the decoder gets exactly the stream and its one look-ahead word (the zero word the encoder left behind it)
    out, bad = decode_raw(env, wbuf[PAD: PAD + sw + 1], off_h, lab.size, lengths, k, lb, out_off)
    assert bad == 0 and np.array_equal(_as_int(out, lb), lab)
    return off_h


# ------------------------------------------------------------------ hand-chosen code lengths
def length_sets(k):
    """name -> lengths[k]: the 1..32 chain (on the last 33 symbols, so K - 1 is used), all 32, and {1, 32, 32, ...}."""
    out = {"all32": np.full(k, 32)}
    if k >= 2:
        out["one_then_32"] = np.array([1] + [32] * (k - 1))
    if k >= 33:
        chain = np.zeros(k, dtype=np.int64)
        chain[k - 33:] = list(range(1, 33)) + [32]
        out["chain"] = chain
    if k == 1:
        out["one"] = np.array([1])
    return out


def long_code_labels(lengths, n, rng):
    """n labels where codes of 31 and 32 bits start at every bit offset 0..31 (as far as the shorter codes allow) and sit on both
    sides of every chunk boundary, with random used symbols in between."""
    lengths = np.asarray(lengths, dtype=np.int64)
    used = np.flatnonzero(lengths)
    longs = [int(s) for s in used if lengths[s] >= 31]
    by_len = {int(lengths[s]): int(s) for s in used[::-1]}
    seq, pos = [], 0
    for b in range(32):
        for s in longs[:3]:
            gap = (b - pos) % 32
            if gap and gap in by_len:
                seq.append(by_len[gap]); pos += gap
            elif gap and 1 in by_len:
                seq += [by_len[1]] * gap; pos += gap
            seq.append(s); pos += int(lengths[s])
    lab = used[rng.randint(used.size, size=n)]
    head = np.array(seq[:n], dtype=np.int64)
    lab[: head.size] = head
    if longs:
        for c in range(CHUNK, n, CHUNK):              # long codes on both sides of every chunk boundary
            lab[c - 1] = longs[0]
            lab[c] = longs[-1]
            if c + 1 < n:
                lab[c + 1] = longs[0]
    return lab


CASES = [(k, lb, name) for k in (1, 2, 33, 256, 257, 1040) for lb in (1, 2) if not (lb == 1 and k > 256) for name in length_sets(k)]


@pytest.mark.parametrize("k,lb,name", CASES)
def test_dense_stream_with_hand_chosen_lengths(env, k, lb, name):
    lengths = length_sets(k)[name]
    rng = np.random.RandomState(k * 7 + lb)
    for i, n in enumerate((1, 1023, 1024, 1025, 3 * CHUNK + 7)):
        lab = long_code_labels(lengths, n, rng)
        roundtrip(env, lab, lb, lengths, k, in_off=(0, 1, 3, 1, 0)[i], out_off=(1, 0, 1, 3, 1)[i])
        if name == "chain" and n >= CHUNK:
            # the long codes really start at every bit offset and cross the chunk boundaries
            ls = lengths[lab]
            starts = np.cumsum(ls) - ls
            assert set((starts[ls >= 31] % 32).tolist()) == set(range(32))
            assert all(ls[c - 1: c + 2].min() >= 31 for c in range(CHUNK, n, CHUNK))
    # a stream of a whole number of words: the decoder reads its look-ahead word at the very end
    if name in ("all32", "one_then_32"):
        s = int(np.flatnonzero(lengths == 32)[-1])
        lab = np.full(2 * CHUNK + 5, s)
        off_h = roundtrip(env, lab, lb, lengths, k, in_off=1, out_off=1)
        assert off_h[-1] % 32 == 0


def test_whole_word_streams_of_mixed_lengths(env):
    """Streams of 1- and 31-bit codes that end exactly on a word boundary (and chunks that end on one too)."""
    k = 33
    lengths = length_sets(k)["chain"]
    one, l31 = int(np.flatnonzero(lengths == 1)[0]), int(np.flatnonzero(lengths == 31)[0])
    lab = np.array(([l31] + [one]) * 512 + [l31] * 32 + [one] * 32, dtype=np.int64)    # 512 * 32 + 32 * 31 + 32 bits
    assert int(lengths[lab].sum()) % 32 == 0
    for lb in (1, 2):
        roundtrip(env, lab, lb, lengths, k, in_off=1, out_off=3)


def test_n_zero_is_a_no_op(env):
    L, nat = env[0], env[1]
    for lb in (1, 2):
        lab_d = _labels_dev(np.zeros(0), lb, 1)
        lengths = np.full(4, 2, dtype=np.uint8)
        off_h, wbuf, sw = encode_raw(env, lab_d, lb, lengths, 4)
        assert off_h.tolist() == [0] and sw == 0
        assert (wbuf[PAD: PAD + 2] == 0).all()                       # the two words it was given, zeroed; nothing else
        out, bad = decode_raw(env, wbuf[PAD: PAD + 1], off_h, 0, lengths, 4, lb, 1)
        assert bad == 0 and out.numel() == 0
        # the sparse form: no entries, nothing written
        obuf, eoff = _framed(1, torch.int64, np.int64(np.uint64(O_SENT)).item())
        nat.check(L.nnc_sparse_entry_offsets(lab_d.data_ptr(), lb, 0, 2, 4, eoff.data_ptr(), _stream()))
        dbuf, delta = _framed(1, torch.uint8, 0xA5)
        nat.check(L.nnc_sparse_emit(lab_d.data_ptr(), lb, 0, 2, 4, eoff.data_ptr(), delta.data_ptr(), delta.data_ptr(), _stream()))
        bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        lbuf, outl = _framed(1, torch.uint8 if lb == 1 else torch.int16, L_SENT[lb])
        nat.check(L.nnc_sparse_expand(delta.data_ptr(), delta.data_ptr(), lb, eoff.data_ptr(), 0, 2, outl.data_ptr(), bad.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert eoff.cpu().tolist() == [0] and _frame_intact(obuf, PAD, 1, O_SENT)
        assert _frame_intact(dbuf, PAD - 1, 0, 0xA5) and _frame_intact(lbuf, PAD - 1, 0, L_SENT[lb]) and int(bad.item()) == 0


# ------------------------------------------------------------------ beyond 2^32 bits
def test_a_stream_beyond_2_pow_32_bits(env):
    """About 135 M uint8 indices, 32-bit codes with a few 31-bit ones: the stream passes 2^32 bits inside a code, in a chunk that
    starts mid-word.  Chunk offsets and the words around 2^32 against the reference, the whole stream round-tripped on the device."""
    L, nat, ops, storage = env
    n, k = 135_000_000, 256
    lengths = np.array([31] + [32] * (k - 1), dtype=np.uint8)
    rng = np.random.RandomState(32)
    lab = rng.randint(1, k, size=n, dtype=np.uint8)
    lab[rng.randint(0, n, size=20_000)] = 0
    lab[n - 1] = 255
    off_ref = codec_ref.chunk_offsets(lab, lengths)
    c = int(np.searchsorted(off_ref, 1 << 32, side="right")) - 1           # the chunk that holds bit 2^32
    ls = lengths[lab[c * CHUNK: (c + 1) * CHUNK]].astype(np.int64)
    starts = off_ref[c] + np.cumsum(ls) - ls
    i = int(np.searchsorted(starts, 1 << 32, side="right")) - 1
    assert off_ref[c] % 32 != 0, "the chunk around 2^32 should start mid-word"
    assert starts[i] < 1 << 32 < starts[i] + ls[i], "bit 2^32 should fall inside a code"
    lab_d = torch.from_numpy(lab).cuda()
    off_h, wbuf, sw = encode_raw(env, lab_d, 1, lengths, k, repeat=False)
    assert np.array_equal(off_h, off_ref) and off_h[-1] > 1 << 32
    lo, hi = int(off_h[c - 1]), int(off_h[c + 2])
    got = codec_ref.words_to_bits(wbuf[PAD + lo // 32: PAD + (hi + 31) // 32].cpu().numpy().view(np.uint32))
    want = codec_ref.stream_bits(lab[(c - 1) * CHUNK: (c + 2) * CHUNK], lengths)
    assert np.array_equal(got[lo % 32: lo % 32 + (hi - lo)], want)
    out, bad = decode_raw(env, wbuf[PAD: PAD + sw + 1], off_h, n, lengths, k, 1, 0)
    assert bad == 0 and torch.equal(out, lab_d)
    del out, wbuf, lab_d
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ through storage.encode_indices / decode_indices
def _lengths_of(ops, storage):
    def f(counts):
        counts = np.asarray(counts, dtype=np.int64)
        return storage._flatten_lengths(np.ascontiguousarray(ops.huffman_lengths(counts)[0], dtype=np.uint8), counts)
    return f


def _fib(m):
    c = [1, 1]
    while len(c) < m:
        c.append(c[-1] + c[-2])
    return np.array(c[:m], dtype=np.int64)


@pytest.mark.parametrize("case", ["fib33", "fib34", "k1040"])
def test_storage_codec_at_its_limits(env, case):
    L, nat, ops, storage = env
    rng = np.random.RandomState(len(case))
    if case.startswith("fib"):
        m = int(case[3:])
        k, lb = m, 1
        lab = rng.permutation(np.repeat(np.arange(m), _fib(m)))
    else:
        k, lb = KMAX, 2
        p = np.exp(-np.arange(k) * (6.0 / k)); p /= p.sum()
        lab = rng.choice(k, size=200_003, p=p)
        lab[[0, 1023, 1024, 200_002]] = k - 1
    lab_d = torch.from_numpy(lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)).cuda()
    words, chunk_bits, lengths, total_bits = storage.encode_indices(lab_d, k)
    want_len = _lengths_of(ops, storage)(np.bincount(lab, minlength=k))
    assert np.array_equal(lengths, want_len)
    if case == "fib33":
        assert int(lengths.max()) == 32
    elif case == "fib34":
        assert set(lengths.tolist()) == {6} and total_bits == 6 * lab.size        # the flattened fixed-width branch
    assert np.array_equal(np.concatenate([[0], np.cumsum(chunk_bits.astype(np.int64))]), codec_ref.chunk_offsets(lab, lengths))
    want, nb = codec_ref.stream_words(lab, lengths)
    assert nb == total_bits and np.array_equal(words.cpu().numpy().view(np.uint32), want)
    back = storage.decode_indices(words, chunk_bits, lab.size, lengths, k, lb)
    assert torch.equal(back, lab_d)


# ------------------------------------------------------------------ relative-index sparse entries
def gap_positions(D):
    """Stored positions of one chunk with gaps of exactly D, D + 1 and 2D, the first touching the chunk's start, the last its end."""
    pos, g = [D - 1], 0
    while pos[-1] + (D + 1, 2 * D, D)[g % 3] < CHUNK - 1 - 2 * D:
        pos.append(pos[-1] + (D + 1, 2 * D, D)[g % 3])
        g += 1
    if CHUNK - 1 - 2 * D > pos[-1]:
        pos.append(CHUNK - 1 - 2 * D)
    pos.append(CHUNK - 1)
    return pos


def sparse_labels(k, zero, D, rng):
    """Six chunks: every position stored, none, only position 0, only position 1023, the exact gaps, then a partial chunk."""
    others = np.array([s for s in range(k) if s != zero])
    lab = np.full(6 * CHUNK, zero, dtype=np.int64)
    lab[:CHUNK] = others[rng.randint(others.size, size=CHUNK)]
    lab[2 * CHUNK] = others[-1]
    lab[4 * CHUNK - 1] = others[0]
    for p in gap_positions(D):
        lab[4 * CHUNK + p] = others[rng.randint(others.size)]
    tail = 5 * CHUNK + 300
    lab[5 * CHUNK: tail] = np.where(rng.rand(300) < 0.3, others[rng.randint(others.size, size=300)], zero)
    return lab[:tail]


def sparse_raw(env, lab, lb, zero, db, off):
    """nnc_sparse_entry_offsets / emit / expand through framed buffers, each output against the reference."""
    L, nat = env[0], env[1]
    n = lab.size
    lab_d = _labels_dev(lab, lb, off)
    nchunks = (n + CHUNK - 1) // CHUNK
    obuf, eoff = _framed(nchunks + 1, torch.int64, np.int64(np.uint64(O_SENT)).item())
    nat.check(L.nnc_sparse_entry_offsets(lab_d.data_ptr(), lb, n, zero, db, eoff.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _frame_intact(obuf, PAD, nchunks + 1, O_SENT)
    wd, ws, wc = codec_ref.sparse_entries(lab, zero, db)
    eoff_h = eoff.cpu().numpy()
    assert np.array_equal(np.diff(eoff_h), wc) and eoff_h[0] == 0
    e = int(eoff_h[-1])
    dbuf, delta = _framed(e, torch.uint8, 0xA5)
    sbuf, sym = _framed(e, torch.uint8 if lb == 1 else torch.int16, L_SENT[lb], 1)
    nat.check(L.nnc_sparse_emit(lab_d.data_ptr(), lb, n, zero, db, eoff.data_ptr(), delta.data_ptr(), sym.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _frame_intact(dbuf, PAD, e, 0xA5) and _frame_intact(sbuf, PAD + 1, e, L_SENT[lb]), "a store outside the entries"
    assert np.array_equal(delta.cpu().numpy().astype(np.int64), wd) and np.array_equal(_as_int(sym, lb), ws)
    lbuf, out = _framed(n, torch.uint8 if lb == 1 else torch.int16, L_SENT[lb], 3)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    nat.check(L.nnc_sparse_expand(delta.data_ptr(), sym.data_ptr(), lb, eoff.data_ptr(), n, zero, out.data_ptr(), bad.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _frame_intact(lbuf, PAD + 3, n, L_SENT[lb]), "a store outside the expanded labels"
    assert int(bad.item()) == 0 and np.array_equal(_as_int(out, lb), lab)
    return wc


@pytest.mark.parametrize("db", range(1, 9))
@pytest.mark.parametrize("lb", [1, 2])
def test_sparse_entries_for_every_delta_bits(env, db, lb):
    D = 1 << db
    rng = np.random.RandomState(db * 3 + lb)
    k, zero = (16, 5) if lb == 1 else (300, 299)
    lab = sparse_labels(k, zero, D, rng)
    wc = sparse_raw(env, lab, lb, zero, db, off=lb)
    assert wc[0] == CHUNK and wc[1] == 0 and wc[2] == 1
    assert wc[3] == (CHUNK - 1) // D + 1                        # only position 1023: (1023 >> db) fillers and its own entry
    if db == 1:
        assert wc[3] == 512                                      # 511 fillers: the most a chunk can hold
    gaps = np.diff([-1] + gap_positions(D))
    assert {D, D + 1, 2 * D} <= set(gaps.tolist()) or D >= 256 and {D, 2 * D} <= set(gaps.tolist())


@pytest.mark.parametrize("db", [1, 4, 8])
def test_sparse_entries_at_kmax(env, db):
    rng = np.random.RandomState(db)
    lab = sparse_labels(KMAX, KMAX - 1, 1 << db, rng)
    sparse_raw(env, lab, 2, KMAX - 1, db, off=1)


# ------------------------------------------------------------------ pack_indices / unpack_indices
FORMS = ("dense", "sparse4", "sparse8")


def _pack_all(env, lab, k, lb):
    L, nat, ops, storage = env
    lab_d = torch.from_numpy(lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)).cuda()
    lengths_of = _lengths_of(ops, storage)
    counts = np.bincount(lab, minlength=k)
    zero = int(np.argmax(counts))
    for form in FORMS:
        body, bits, chosen = storage.pack_indices(lab_d, k, form=form)
        assert chosen == form
        want, wbits = codec_ref.index_bytes(lab, k, lengths_of, "dense" if form == "dense" else "sparse", zero, 4 if form == "sparse4" else 8)
        assert body == want and bits == wbits, form
        back, pos = storage.unpack_indices(body, 0, k, lab.size, lb, lab_d.device)
        assert pos == len(body) and torch.equal(back, lab_d), form
    return zero


def test_pack_indices_at_kmax(env):
    rng = np.random.RandomState(11)
    n = 50_000
    lab = np.where(rng.rand(n) < 0.9, 700, rng.randint(0, KMAX, size=n))
    lab[[3, 4000, n - 1]] = KMAX - 1
    assert _pack_all(env, lab, KMAX, 2) == 700


@pytest.mark.parametrize("n", [0, 1])
def test_pack_indices_of_zero_and_one_index(env, n):
    for k, lb in ((16, 1), (KMAX, 2)):
        _pack_all(env, np.full(n, k - 1, dtype=np.int64), k, lb)


def test_pack_indices_zero_cluster_with_a_tie(env):
    """The zero cluster is the most frequent index, the lowest on a tie (np.argmax): here 3, tied with 9, neither of them 0."""
    rng = np.random.RandomState(5)
    lab = np.concatenate([np.full(3000, 3), np.full(3000, 9), rng.randint(0, 16, size=500)])
    lab = lab[rng.permutation(lab.size)]
    counts = np.bincount(lab, minlength=16)
    top = counts.max()
    lab[np.flatnonzero(lab == 3)[: counts[3] - min(counts[3], counts[9])]] = 0   # make the tie exact
    lab[np.flatnonzero(lab == 9)[: counts[9] - min(counts[3], counts[9])]] = 0
    counts = np.bincount(lab, minlength=16)
    assert counts[3] == counts[9] == counts.max() and top >= counts[3]
    assert _pack_all(env, lab, 16, 1) == 3


def test_hand_built_file_loads_on_the_device(env, tmp_path):
    """A file built by the reference alone (dense, sparse and raw records) decodes to centers[labels] bit for bit."""
    L, nat, ops, storage = env
    lengths_of = _lengths_of(ops, storage)
    rng = np.random.RandomState(9)
    lab1 = rng.randint(0, 16, size=40 * 70)
    lab2 = np.where(rng.rand(5000) < 0.1, rng.randint(0, 300, size=5000), 7)
    c1, c2 = rng.randn(16).astype(np.float32), rng.randn(300).astype(np.float32)
    raw = rng.randn(3, 4).astype(np.float32)
    blob = codec_ref.file_bytes([codec_ref.record("a", (40, 70), c1, lab1, lengths_of),
                                 codec_ref.record("b", (50, 100), c2, lab2, lengths_of, form="sparse", zero=7, dbits=8),
                                 codec_ref.raw_record("c", raw)])
    path = tmp_path / "hand.nnc"
    path.write_bytes(blob)
    got = storage.load_compressed(str(path))
    assert np.array_equal(got["a"].cpu().numpy(), c1[lab1].reshape(40, 70))
    assert np.array_equal(got["b"].cpu().numpy(), c2[lab2].reshape(50, 100))
    assert np.array_equal(got["c"].cpu().numpy(), raw)


# ------------------------------------------------------------------ the encoders refuse indices >= k
def test_encoders_refuse_an_index_beyond_k(env, tmp_path):
    L, nat, ops, storage = env
    lab = np.zeros(3000, dtype=np.uint8)
    lab[1500] = 16
    lab_d = torch.from_numpy(lab).cuda()
    with pytest.raises(ValueError, match="index is >= k"):
        storage.encode_indices(lab_d, 16)
    with pytest.raises(ValueError, match="index is >= k"):
        storage.encode_sparse(lab_d, 0, 4, 16)
    with pytest.raises(ValueError, match="zero_symbol"):
        storage.encode_sparse(lab_d, 16, 4, 16)
    # without k the bound is NNC_KMAX: a 16-bit index of 1040 is refused, one of 1039 encoded
    wide = torch.from_numpy(np.full(5, 1039, dtype=np.int16)).cuda()
    assert storage.encode_sparse(wide, 0, 4)[1].numel() == 5
    wide[2] = KMAX
    with pytest.raises(ValueError, match="index is >= k"):
        storage.encode_sparse(wide, 0, 4)
    for form in FORMS + ("auto",):
        with pytest.raises(ValueError, match="index is >= k"):
            storage.pack_indices(lab_d, 16, form=form)
    model = types.SimpleNamespace(cluster_centers_=np.zeros((16, 1), np.float32), labels_compact_=lab_d, counts_device_=None)
    path = tmp_path / "bad.nnc"
    with pytest.raises(ValueError, match="index is >= k"):
        storage.save_compressed(str(path), {"w": ((3000,), model, None)})
    assert not path.exists()
    lab_d[1500] = 15                                       # in range again: it stores
    assert storage.save_compressed(str(path), {"w": ((3000,), model, None)}) > 0
