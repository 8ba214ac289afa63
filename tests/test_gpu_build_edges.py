"""Crafted edges of the device builders, build_cobs_kernel and build_bloom_kernel (GPU).

A mis-built bank misclassifies silently for as long as its file lives; the
other GPU tests compare the builders with the oracle on random shapes only.
Every image here is compared with two references that must agree with each
other: the oracle's build (oracle/xs_oracle.c) and a restatement in this file,
a plain loop over records, k-mers and hashes (COBS: oracle.xxh64 of
oracle.canonical_cobs, bit (doc - group start) of row hash % signature size;
rbloom: the index sequence of oracle.xxh3_64 of oracle.canonical_bio).

The restatement counts how often every bit is set, and the banks are sized so
that the comparison can see a lost k-mer: a k-mer whose every bit is also set
by another one could vanish from the build without changing the image.  So
the cases that are about record lengths assert, on the reference, a bound on
the fill and that each edge k-mer of each long record (its first and last, and
those on either side of the 256-k-mer unit edge) owns a bit no other k-mer sets.

B1  record lengths: exactly n k-mers for every n of the probes' edge table
    (15..17, 63..65, 255..257, 511..513), the empty record, k - 1 and k
    bytes, and N, lower-case and IUPAC bytes inside k-mers 255, 256 and 257,
    interleaved over the docs.
B2  doc bits at the byte, 32-bit word and group edges: exactly those bits, and
    no padding bit, are set.
B3  contention: 128 docs x hundreds of k-mers, all one canonical k-mer, OR
    into the same h rows.
B4  accumulation: build after build and build over an uploaded image OR into
    what is there.
B5  entry points: build_device and query_device back to back on one stream;
    a rec_doc entry equal to D (host: XS_ERR_ARG, nothing changes; device: that
    record is skipped).
B6  rbloom: the records of B1 and the accumulation of B4 at K up to 16, probed
    on both paths.  Filters of 1-63 bytes saturate (the smallest divisors and
    the word edges of the image are what they test); 4097 bytes holds all of
    B1's records at a fill of at most 0.8; 1 MiB + 1 byte is where every edge
    k-mer owns a bit.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import _reads
from test_gpu_probe_kernels import EDGE_KMERS, _acgt

pytestmark = pytest.mark.gpu

# (21, 7): the specialised build kernel; the others take <0,0>
KH = [(21, 7), (21, 10), (31, 1), (25, 16), (32, 3), (5, 2)]
# classic D = 9; compact page 1, 3 groups, D = 20: (D, page, sig).  A doc takes at most four of B1's records
# (B4), under 2,000 k-mers x 16 hashes = 32,000 rows: a column of 80,000 rows and more stays under
# 1 - exp(-32,000 / 80,000) = 0.33 full.  The images are 240 and 311 KB.
BANKS = {"classic": (9, None, [120_011]), "compact": (20, 1, [80_021, 131_072, 100_003])}
MAX_FILL = 0.33


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


def _page(D, page):
    return page if page is not None else (D + 7) // 8


def _pack(counts):
    return np.packbits(counts > 0, bitorder="little")


def _cobs_bits(oracle_mod, kmer, d, sig, P, h, base):
    """The bits (byte * 8 + bit of the file layout) one k-mer of doc d sets."""
    g, bit = divmod(d, 8 * P)
    c = oracle_mod.canonical_cobs(kmer)
    return [(int(base[g]) + (oracle_mod.xxh64(c, seed=j) % sig[g]) * P) * 8 + bit for j in range(h)]


def _restated_counts(oracle_mod, seqs, docs, sig, P, D, h, k):
    """Row set x doc bit: how many (record, k-mer, hash) set each bit of the file layout."""
    counts = np.zeros(sum(sig) * P * 8, np.int32)
    base = np.concatenate([[0], np.cumsum(np.asarray(sig, np.int64) * P)])
    for s, d in zip(seqs, docs):
        assert 0 <= d < D
        for i in range(len(s) - k + 1):
            np.add.at(counts, _cobs_bits(oracle_mod, s[i:i + k], d, sig, P, h, base), 1)
    return counts


def _restated_image(oracle_mod, seqs, docs, sig, P, D, h, k, image=None):
    img = _pack(_restated_counts(oracle_mod, seqs, docs, sig, P, D, h, k))
    return img if image is None else img | image


def _reference(oracle_mod, seqs, docs, sig, P, D, h, k, edges=False):
    """The oracle's image, held to the restatement.  edges: B1's records, where
    a lost edge k-mer of a long record must change the image."""
    ob = oracle_mod.CobsBank.empty(sig, P, D, h, k)
    ob.build(seqs, docs)
    counts = _restated_counts(oracle_mod, seqs, docs, sig, P, D, h, k)
    assert np.array_equal(ob.rows, _pack(counts)), "the oracle's build and its restatement differ"
    if edges:
        base = np.concatenate([[0], np.cumsum(np.asarray(sig, np.int64) * P)])
        fill = _column_fill(counts, sig, P, D)
        assert fill.max() <= MAX_FILL, f"a column is {fill.max():.2f} full"
        if k >= 21:  # 4^5 k-mers repeat within a record of hundreds: (5, 2) is held by the image alone
            for s, d in zip(seqs, docs):
                for i in _edge_kmers(len(s) - k + 1):
                    own = counts[_cobs_bits(oracle_mod, s[i:i + k], d, sig, P, h, base)]
                    assert (own == 1).any(), f"k-mer {i} of a record of {len(s) - k + 1} could be lost unseen"
    return ob


def _column_fill(counts, sig, P, D):
    """Fraction of set bits of every doc's column."""
    out, at = np.zeros(D), 0
    for g, s in enumerate(sig):
        ones = (counts[at:at + s * P * 8].reshape(s, P * 8) > 0).sum(axis=0)
        lo, hi = g * 8 * P, min(D, (g + 1) * 8 * P)
        out[lo:hi] = ones[:hi - lo] / s
        at += s * P * 8
    return out


def _edge_kmers(nk):
    """Of a record of >= 255 k-mers: its first and last k-mer, the last of its
    first unit (255) and the first of its second (256), and 257, which B1's odd
    record fills with non-ACGT bytes; of a shorter record, none."""
    return sorted({i for i in (0, 255, 256, 257, nk - 1) if i < nk}) if nk >= 255 else []


def _create(xs, k, h, sig, D, page):
    return xs.Bank.create_cobs(k, h, sig, D, page_size=page, compact=page is not None)


def _edge_records(rng, k):
    """B1: one record per edge k-mer count, the records without k-mers, and one
    whose k-mers 255, 256 and 257 each hold an N, a lower-case and an IUPAC byte
    (positions 257..259 lie in k-mers 255..257 for every k >= 5)."""
    recs = [_acgt(rng, k + n - 1) for n in EDGE_KMERS]
    odd = bytearray(_acgt(rng, k + 511))
    odd[257:260] = b"NaR"
    short = [b"", _acgt(rng, k - 1), _acgt(rng, k)]
    out = []
    for i, r in enumerate(recs + [bytes(odd)]):  # empty and short records between the others
        out.append(r)
        if i % 4 == 1:
            out.append(short[(i // 4) % 3])
    return out + short


# ------------------------------------------------------------------ B1
@pytest.mark.parametrize("bank", list(BANKS))
@pytest.mark.parametrize("k,h", KH)
def test_record_lengths(xs, oracle_mod, k, h, bank):
    D, page, sig = BANKS[bank]
    P = _page(D, page)
    rng = np.random.default_rng([k, h, D])
    seqs = _edge_records(rng, k)
    docs = [i % D for i in range(len(seqs))]
    assert set(docs) == set(range(D))
    ob = _reference(oracle_mod, seqs, docs, sig, P, D, h, k, edges=True)
    gb = _create(xs, k, h, sig, D, page)
    gb.build(seqs, docs)
    assert np.array_equal(gb.download(), ob.rows), "device-built bank differs"
    gb.close()


# ------------------------------------------------------------------ B2
DOC_BIT_CASES = [
    # D, page, sig, docs that take the record
    (130, None, [3001], [0, 7, 8, 31, 32, 63, 64, 127, 128, 129]),    # 17-byte page, 32-byte pitch
    (273, 17, [2999, 1024, 2047], [0, 135, 136, 271, 272]),           # first and last doc of each group
]


@pytest.mark.parametrize("k,h", KH)
@pytest.mark.parametrize("D,page,sig,into", DOC_BIT_CASES, ids=["classic130", "compact273"])
def test_doc_bits_at_byte_word_and_group_edges(xs, oracle_mod, D, page, sig, into, k, h):
    P = _page(D, page)
    assert P == 17 and (len(sig) - 1) * 8 * P < D <= len(sig) * 8 * P
    rng = np.random.default_rng([k, h, D])
    rec = _acgt(rng, k + 99)
    ob = _reference(oracle_mod, [rec] * len(into), into, sig, P, D, h, k)
    gb = _create(xs, k, h, sig, D, page)
    gb.build([rec] * len(into), into)
    got = gb.download()
    assert np.array_equal(got, ob.rows), "device-built bank differs"
    # every row is empty or holds exactly the bits of its group's docs; no other bit, no padding bit
    base = 0
    for g, s in enumerate(sig):
        want_row = np.zeros(P, np.uint8)
        for d in into:
            if g * 8 * P <= d < (g + 1) * 8 * P:
                want_row[(d - g * 8 * P) >> 3] |= 1 << ((d - g * 8 * P) & 7)
        part = got[base:base + s * P].reshape(s, P)
        touched = part.any(axis=1)
        assert 0 < int(touched.sum()) <= 100 * h
        assert (part[touched] == want_row).all() and not part[~touched].any()
        base += s * P
    gb.close()


# ------------------------------------------------------------------ B3
@pytest.mark.parametrize("k,h", KH)
def test_many_waves_or_one_word(xs, oracle_mod, k, h):
    """Every one of 128 docs inserts "A" * (k + 512) and "T" * (k + 10): 524
    k-mers a doc, all the canonical k-mer "A" * k, so at most h rows are
    touched, by every wave at once; they become all ones and nothing else is set."""
    D, sig = 128, [1009]
    seqs, docs = [], []
    for d in range(D):
        seqs += [b"A" * (k + 512), b"T" * (k + 10)]
        docs += [d, d]
    ob = _reference(oracle_mod, seqs[:2], [0, 0], sig, 16, D, h, k)  # one doc restated, the row set is the same
    rows = {oracle_mod.xxh64(b"A" * k, seed=j) % sig[0] for j in range(h)}
    assert set(np.flatnonzero(ob.rows.reshape(sig[0], 16).any(axis=1)).tolist()) == rows
    want = np.zeros((sig[0], 16), np.uint8)
    want[sorted(rows)] = 0xFF
    full = oracle_mod.CobsBank.empty(sig, 16, D, h, k)
    full.build(seqs, docs)
    assert np.array_equal(full.rows, want.reshape(-1)), "the oracle misses the closed form"
    gb = _create(xs, k, h, sig, D, None)
    gb.build(seqs, docs)
    assert np.array_equal(gb.download(), want.reshape(-1))
    gb.close()


# ------------------------------------------------------------------ B4
@pytest.mark.parametrize("bank", list(BANKS))
@pytest.mark.parametrize("k,h", KH)
def test_builds_accumulate(xs, oracle_mod, k, h, bank):
    D, page, sig = BANKS[bank]
    P = _page(D, page)
    rng = np.random.default_rng([k, h, D, 4])
    recs = _edge_records(rng, k)
    a, b = recs[0::2], recs[1::2]
    da, db = [i % D for i in range(len(a))], [(i + 4) % D for i in range(len(b))]
    img_a = _reference(oracle_mod, a, da, sig, P, D, h, k, edges=True).rows
    img_ab = _reference(oracle_mod, a + b, da + db, sig, P, D, h, k, edges=True).rows
    assert not np.array_equal(img_a, img_ab)
    gb = _create(xs, k, h, sig, D, page)
    gb.build(a, da)
    assert np.array_equal(gb.download(), img_a)
    gb.build(a, da)
    assert np.array_equal(gb.download(), img_a), "building the same records twice changed the image"
    gb.build(b, db)
    assert np.array_equal(gb.download(), img_ab), "build(A) then build(B) differs from build(A + B)"
    gb.close()
    # over an uploaded image of random bytes (1/16 of the bits set, padding bits among them: a lost
    # k-mer of A still shows)
    x = np.bitwise_and.reduce([np.frombuffer(rng.bytes(img_a.size), np.uint8) for _ in range(4)])
    assert not np.array_equal(x | img_a, x)
    gb = _create(xs, k, h, sig, D, page)
    gb.upload(x)
    gb.build(a, da)
    assert np.array_equal(gb.download(), x | img_a), "build over an uploaded image is not X | image(A)"
    gb.close()


# ------------------------------------------------------------------ B5
def _device_records(torch, seqs, docs):
    from xspect2_amd.packing import pack_sequences
    pr = pack_sequences(seqs)
    dev = torch.device("cuda", 0)
    d_seq = torch.from_numpy(pr.buf.copy()).to(dev)
    d_off = torch.from_numpy(pr.offsets.astype(np.int64)).to(dev)
    d_doc = torch.from_numpy(np.asarray(docs, dtype=np.int64).astype(np.int32)).to(dev)
    return pr, d_seq, d_off, d_doc


@pytest.mark.parametrize("bank", list(BANKS))
@pytest.mark.parametrize("k,h", KH)
def test_device_build_then_query_on_one_stream(xs, oracle_mod, k, h, bank):
    """build_device and query_device enqueued back to back on a non-default
    torch stream, with no synchronisation between them: the query sees the
    whole bank."""
    torch = pytest.importorskip("torch")
    D, page, sig = BANKS[bank]  # far from saturated: own reads 256, foreign 0
    P = _page(D, page)
    rng = np.random.default_rng([k, h, D, 5])
    seqs = [_acgt(rng, int(rng.integers(k + 255, k + 400))) for _ in range(2 * D)]
    docs = [i % D for i in range(len(seqs))]
    ob = _reference(oracle_mod, seqs, docs, sig, P, D, h, k)
    reads = [s[:k + 255] for s in seqs[:D]] + _reads(rng, 60, k) + [b"", seqs[0] * 2]
    want_h, want_n = ob.query(reads)
    pr, d_seq, d_off, d_doc = _device_records(torch, seqs, docs)
    qr, q_seq, q_off, _ = _device_records(torch, reads, [])
    dev = torch.device("cuda", 0)
    d_hits = torch.full((qr.n, D), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_nk = torch.full((qr.n,), -1, dtype=torch.int64, device=dev)
    d_tot = torch.full((D + 1,), -1, dtype=torch.int64, device=dev)
    gb = _create(xs, k, h, sig, D, page)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    gb.build_device(d_seq, int(pr.offsets[-1]), d_off, pr.n, d_doc, stream=st.cuda_stream)
    gb.query_device(q_seq, int(qr.offsets[-1]), q_off, qr.n, 1, d_hits, d_nk, d_tot, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_nk.cpu().numpy().view(np.uint64), want_n)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), want_h)
    tot = d_tot.cpu().numpy().view(np.uint64)
    assert np.array_equal(tot[:D], want_h.sum(axis=0, dtype=np.uint64)) and int(tot[D]) == int(want_n.sum())
    assert (want_h == 256).any()
    if k >= 21:  # a read of 256 5-mers finds most of them in every doc
        assert (want_h[:D] == 0).any()
    assert np.array_equal(gb.download(), ob.rows)
    gb.close()


@pytest.mark.parametrize("bank", list(BANKS))
@pytest.mark.parametrize("k,h", KH)
def test_rec_doc_equal_to_num_docs(xs, oracle_mod, k, h, bank):
    """A rec_doc entry equal to D.  Host build: XS_ERR_ARG and the image is
    unchanged (the other records of the call are not inserted either).
    build_device reads no entry back: that record alone is skipped."""
    torch = pytest.importorskip("torch")
    from xspect2_amd import _lib
    D, page, sig = BANKS[bank]
    P = _page(D, page)
    rng = np.random.default_rng([k, h, D, 6])
    first = [_acgt(rng, k + 100) for _ in range(D)]
    ob = _reference(oracle_mod, first, list(range(D)), sig, P, D, h, k)
    seqs = [_acgt(rng, int(rng.integers(k, 400))) for _ in range(12)]
    docs = [(5 * i) % D for i in range(len(seqs))]
    docs[0] = docs[7] = docs[-1] = D  # first, middle and last record
    gb = _create(xs, k, h, sig, D, page)
    gb.build(first, list(range(D)))
    with pytest.raises(_lib.XsError) as err:
        gb.build(seqs, docs)
    assert err.value.code == _lib.XS_ERR_ARG
    assert np.array_equal(gb.download(), ob.rows), "a refused build changed the image"
    pr, d_seq, d_off, d_doc = _device_records(torch, seqs, docs)
    gb.build_device(d_seq, int(pr.offsets[-1]), d_off, pr.n, d_doc, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    kept = [i for i, d in enumerate(docs) if d < D]
    assert len(kept) == len(seqs) - 3
    want = _restated_image(oracle_mod, [seqs[i] for i in kept], [docs[i] for i in kept], sig, P, D, h, k,
                           image=ob.rows)
    both = oracle_mod.CobsBank(ob.rows.copy(), sig, P, D, h, k)
    both.build([seqs[i] for i in kept], [docs[i] for i in kept])
    assert np.array_equal(both.rows, want), "the oracle's build and its restatement differ"
    assert not np.array_equal(want, ob.rows)
    assert np.array_equal(gb.download(), want), "build_device did not skip exactly the records of doc D"
    gb.close()


# ------------------------------------------------------------------ B6
BLOOM_BYTES = (1, 2, 3, 15, 16, 17, 63, 4097)
BLOOM_BIG = (1 << 20) + 1  # 3,058 k-mers x K <= 16 bits in 8.4 M: every edge k-mer owns a bit
BLOOM_K = (1, 7, 8, 9, 16)
BLOOM_KMER = (21, 31, 5, 32)
BLOOM_MAX_FILL = 0.8  # 4097 bytes, K = 16: 1 - exp(-3,058 * 16 / 32,776) = 0.78
# every filter size and every K at k = 21, every k at K = 7; every (k, K) at 4097 bytes and at 1 MiB + 1;
# (21, 7), (21, 8), (31, 7) straddle the probe dispatcher's pair, k = 21 / another k the builder's
BLOOM_CASES = sorted({(21, K, nb) for K in BLOOM_K for nb in BLOOM_BYTES} |
                     {(k, 7, nb) for k in BLOOM_KMER for nb in (1, 17)} |
                     {(k, K, nb) for k in BLOOM_KMER for K in BLOOM_K for nb in (4097, BLOOM_BIG)})
assert {(21, 7, 4097), (21, 8, 4097), (31, 7, 4097)} <= set(BLOOM_CASES)


def _bloom_bits(oracle_mod, bf, kmer):
    return bf.indexes(oracle_mod.xxh3_64(oracle_mod.canonical_bio(kmer)))


def _bloom_counts(oracle_mod, bf, seqs):
    """How many (record, k-mer, index function) set each bit of the filter."""
    counts = np.zeros(bf.bits.size * 8, np.int32)
    for s in seqs:
        for i in range(len(s) - bf.k + 1):
            np.add.at(counts, _bloom_bits(oracle_mod, bf, s[i:i + bf.k]), 1)
    return counts


@pytest.mark.parametrize("k,K,nbytes", BLOOM_CASES)
def test_bloom_build_and_probe_edges(xs, oracle_mod, k, K, nbytes):
    rng = np.random.default_rng([k, K, nbytes])
    recs = _edge_records(rng, k)
    a, b = recs[0::2], recs[1::2]
    bf_a = oracle_mod.BloomFilter(np.zeros(nbytes, np.uint8), K, k)
    bf_a.build(a)
    bf = oracle_mod.BloomFilter(bf_a.bits.copy(), K, k)
    bf.build(b)
    whole = oracle_mod.BloomFilter(np.zeros(nbytes, np.uint8), K, k)
    whole.build(a + b)
    assert np.array_equal(whole.bits, bf.bits)
    counts_a, counts = _bloom_counts(oracle_mod, bf, a), _bloom_counts(oracle_mod, bf, a + b)
    assert np.array_equal(_pack(counts_a), bf_a.bits) and np.array_equal(_pack(counts), bf.bits), \
        "the oracle's build and its restatement differ"
    if nbytes >= 4097:
        assert (counts > 0).mean() <= BLOOM_MAX_FILL
    if nbytes == BLOOM_BIG and k >= 21:  # a lost edge k-mer of a long record changes the filter (5-mers repeat)
        for s in a + b:
            for i in _edge_kmers(len(s) - k + 1):
                assert (counts[_bloom_bits(oracle_mod, bf, s[i:i + k])] == 1).any(), \
                    f"k-mer {i} of a record of {len(s) - k + 1} could be lost unseen"
    gb = xs.Bank.create_bloom(k, nbytes, K)
    gb.build(a)
    assert np.array_equal(gb.download(), bf_a.bits), "device-built filter differs"
    gb.build(a)
    assert np.array_equal(gb.download(), bf_a.bits), "building the same records twice changed the filter"
    gb.build(b)
    assert np.array_equal(gb.download(), bf.bits), "build(A) then build(B) differs from build(A + B)"
    x = np.bitwise_and.reduce([np.frombuffer(rng.bytes(nbytes), np.uint8) for _ in range(4)])
    over = xs.Bank.create_bloom(k, nbytes, K)
    over.upload(x)
    over.build(a)
    assert np.array_equal(over.download(), x | bf_a.bits), "build over an uploaded filter is not X | filter(A)"
    over.close()
    reads = recs + _reads(rng, 100, k, alphabet="ACGTacgtNRY") + [_acgt(rng, k + 1536)]
    direct = "bloom<21,7>" if (k, K) == (21, 7) else "bloom<0,0>"
    for part in (0, 3):
        gb.set_probe_options(bloom_part=part)
        for step in (1, 3):
            want_h, want_n = bf.query(reads, step=step)
            got_h, got_n = gb.query(reads, step=step)
            assert gb.probe_kernel() == ("bloompart" if part and K <= 8 else direct)
            assert np.array_equal(got_n, want_n)
            assert np.array_equal(got_h[:, 0], want_h)
            tot, nk = gb.query_totals(reads, step=step)
            assert int(tot[0]) == int(want_h.sum()) and nk == int(want_n.sum())
    if nbytes >= 4097 and k >= 21:
        assert 0 < int(want_h.sum()) < int(want_n.sum())
    gb.close()
