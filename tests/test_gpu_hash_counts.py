"""COBS banks of 10-16 hashes, set padding bits and tiny signature sizes (GPU).

check_term_and_hashes accepts h in 1..16 and the probes keep NH = 16 register
slots per k-mer, in four separately kept copies of the `j < h` loop
(cobs_hashes, wide, slots, general); the other GPU tests stop at h = 9.  Here:

A1  every `<0,0>` and `general` row of test_gpu_probe_kernels' table at
    (k, h) = (25, 16), and (21, 10), (31, 16), (25, 13) on one bank per
    family (the trained k with another h, the trained h's neighbour): the
    same kernel name, the same three images, plus the padding image of A4.
    The built image has 40,000-60,000 rows per group so that 16 ANDed rows
    still tell a document's own read (a full count) from a foreign one (0).
A2  every hash is consulted: doc d's bit is cleared in the row of hash j of
    a k-mer of its own, a different k-mer for each j < h, so the count is
    nk - h; a kernel that ANDs fewer than h rows reports more.
A3  classic banks of <= 128 docs and h > 8 are declined by the partitioned
    probe, whatever cobs_part says.
A4  padding bits (docs >= D in a classic row's last byte and in the unused
    tail of a compact bank's last group) that are set: accepted and ignored.
    An image of all 0xFF bytes counts nk for every doc below D, through the
    u32 and narrowed matrices, the totals and the best doc; an image of
    random bytes equals the oracle, which reads docs below D only; download
    returns the bytes as they were uploaded.
A5  signature sizes of 1, 2, 3 and 8 rows (fastmod and fastmod_small at the
    smallest divisors): saturated banks, equal to the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import _explain, _reads
from test_gpu_probe_kernels import (ROWS, STEPS, _acgt, _bank, _boundary_docs, _check, _edge_docs, _edge_lengths,
                                    _expect, _group_docs, _image, _read_set, _sigs)

pytestmark = pytest.mark.gpu

AMBIGUOUS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


def _general_rows():
    """The table's `<0,0>` and `general` rows, one per bank shape (D, page, G, kernel)."""
    seen, out = set(), []
    for D, _, _, page, G, kernel in ROWS:
        if ("0,0" in kernel or kernel == "general") and (D, page, G) not in seen:
            seen.add((D, page, G))
            out.append((D, page, G, kernel))
    return out


GENERAL_ROWS = _general_rows()
# one bank per family for the other (k, h): the trained k with another h, the
# trained h's neighbour; a classic bank of <= 128 docs with k = 21 or 31 must
# not go to fast<21,7> / fast<31,1>, a compact one of k = 31 not to <31,1>
OTHER_KH = ((21, 10), (31, 16), (25, 13))
FAMILY_BANKS = [(129, None, 1, "wide<0,0,C2,G1>"), (137, 17, 2, "wide<0,0,C2,G2>"), (128, None, 1, "slots<0,0,1,4>"),
                (9, 1, 2, "slots<0,0,4,1>"), (2049, None, 1, "general")]
assert all(b in GENERAL_ROWS for b in FAMILY_BANKS)
A1_CASES = [(D, 25, 16, page, G, kern) for D, page, G, kern in GENERAL_ROWS]
A1_CASES += [(D, k, h, page, G, kern) for D, page, G, kern in FAMILY_BANKS for k, h in OTHER_KH]


def _case_id(c):
    return f"{c[5]}-D{c[0]}-k{c[1]}h{c[2]}-p{c[3]}"


def _big_sigs(D, k, h, page, G):
    """Distinct signature sizes of 40,000-60,000 rows per group, seeded by the shape."""
    rng = np.random.default_rng([D, k, h, page or 0, G, 16])
    return [int(x) for x in rng.choice(np.arange(40_000, 60_001), size=G, replace=False)]


def _column_fill(rows, sig, P, D):
    """Fraction of set bits of every doc's column (docs below D) of a file-layout image."""
    out, base = np.zeros(D), 0
    for g, s in enumerate(sig):
        part = rows[base:base + s * P].reshape(s, P)
        ones = np.concatenate([((part >> b) & 1).sum(axis=0, dtype=np.int64)[:, None] for b in range(8)], axis=1)
        ones = ones.reshape(-1)  # doc (byte, bit) of the group -> count
        lo, hi = g * 8 * P, min(D, (g + 1) * 8 * P)
        out[lo:hi] = ones[:hi - lo] / s
        base += s * P
    return out


def _check_all_docs_count_nk(gb, reads, want_n, D, kernel):
    """The closed form of the padding image through every host output: u32 and
    narrowed hit matrices, totals, best doc."""
    for step in STEPS:
        nk = want_n[step]
        full = np.repeat(nk.astype(np.uint32)[:, None], D, axis=1)
        for dtype in (np.uint32, "auto"):
            got_h, got_n = gb.query(reads, step=step, hit_dtype=dtype)
            assert gb.probe_kernel() == kernel, f"routed to {gb.probe_kernel()}"
            assert np.array_equal(got_n, nk)
            assert got_h.shape == full.shape
            assert np.array_equal(got_h, full), f"{dtype} step {step}: " + _explain(got_h, full, reads)
        assert got_h.dtype == np.uint16  # reads of up to 513 k-mers: "auto" narrowed on the device
        tot, tk = gb.query_totals(reads, step=step)
        assert np.array_equal(tot, np.full(D, int(nk.sum()), np.uint64)) and tk == int(nk.sum())
        best, bh, bnk, btot = gb.query_best(reads, step=step, want_totals=True)
        # every doc shares the maximum (a row of zeros too): one doc is the best doc, more are a tie
        assert np.array_equal(best, np.full(len(reads), 0 if D == 1 else AMBIGUOUS, np.uint32))
        assert np.array_equal(bh, nk.astype(np.uint32)) and np.array_equal(bnk, nk)
        assert np.array_equal(btot[:D], tot) and int(btot[D]) == tk


def _padding_image_case(gb, oracle_mod, sig, P, D, h, k, reads, kernel):
    """A4 on one bank: all 0xFF bytes; the oracle is held to the closed form too."""
    ones = np.full(sum(sig) * P, 0xFF, np.uint8)
    ob = oracle_mod.CobsBank(ones, sig, P, D, h, k)
    gb.upload(ob.rows)
    assert np.array_equal(gb.download(), ones), "download differs from the uploaded bytes"
    want = _expect(ob, reads, closed_form_docs=list(range(D)))
    for small in (1, 0):
        gb.set_probe_options(small_calls=small)
        _check(gb, want, reads, kernel)
        _check_all_docs_count_nk(gb, reads, {s: want[s][1] for s in STEPS}, D, kernel)


# ------------------------------------------------------------------ A1 (+ A4 on its rows)
@pytest.mark.parametrize("D,k,h,page,G,kernel", A1_CASES, ids=[_case_id(c) for c in A1_CASES])
def test_probe_kernel_case_many_hashes(xs, oracle_mod, D, k, h, page, G, kernel):
    P, groups = _group_docs(D, page, G)
    assert len(groups) == G and groups[-1][0] < D <= G * 8 * P
    sig = _big_sigs(D, k, h, page, G)
    rng = np.random.default_rng([k, h, D, G, 16])
    longest = _edge_lengths(k)[-1]
    edge = _edge_docs(D, page, G)

    # 1. built image
    seqs = [_acgt(rng, longest if d in edge else int(rng.integers(k, 300))) for d in range(D)]
    ob = oracle_mod.CobsBank.empty(sig, P, D, h, k)
    ob.build(seqs, list(range(D)))
    fill = _column_fill(ob.rows, sig, P, D)
    assert fill.max() <= 0.60, f"a column is {fill.max():.2f} full: {h} ANDed rows would pass by chance"
    gb = _bank(xs, k, h, sig, D, page)
    gb.upload(ob.rows)
    sources = [seqs[d] for d in edge]
    reads = _read_set(rng, k, sources) + [s[:k + 255] for s in sources]  # one whole unit from every edge doc
    want = _expect(ob, reads, full_unit=True)
    want_h = want[1][0]
    if D > 1:  # a full count and a zero in the same row: the h rows tell the docs apart
        assert ((want_h == 256).any(axis=1) & (want_h == 0).any(axis=1)).any()
    for small in (1, 0):
        gb.set_probe_options(small_calls=small)
        _check(gb, want, reads, kernel)

    # 2. chosen documents, 3. all ones below D: closed forms
    reads = _read_set(rng, k, [_acgt(rng, longest)])
    for docs in (_boundary_docs(D, page, G), list(range(D))):
        ob = oracle_mod.CobsBank(_image(sig, D, page, G, docs), sig, P, D, h, k)
        gb.upload(ob.rows)
        want = _expect(ob, reads, closed_form_docs=docs)
        for small in (1, 0):
            gb.set_probe_options(small_calls=small)
            _check(gb, want, reads, kernel)

    # 4. all 0xFF: the padding bits set as well
    _padding_image_case(gb, oracle_mod, sig, P, D, h, k, reads, kernel)
    gb.close()


# ------------------------------------------------------------------ A2
A2_BANKS = [(129, None, 1, "wide<0,0,C2,G1>"), (137, 17, 2, "wide<0,0,C2,G2>"), (128, None, 1, "slots<0,0,1,4>"),
            (9, 1, 2, "slots<0,0,4,1>"), (129, 1, 17, "general"), (2049, None, 1, "general")]
A2_CASES = [(D, h, page, G, kern) for D, page, G, kern in A2_BANKS for h in (10, 16)]


@pytest.mark.parametrize("D,h,page,G,kernel", A2_CASES, ids=[f"{c[4]}-D{c[0]}-h{c[1]}-p{c[2]}" for c in A2_CASES])
def test_every_hash_is_consulted(xs, oracle_mod, D, h, page, G, kernel):
    """A read of 100 k-mers cut from the bank's last doc d.  For each j < h a
    different k-mer of the read loses doc d's bit in its row of hash j, a row
    no other (k-mer, hash) of the read maps to: exactly those h k-mers drop
    out, the count is nk - h.  A kernel that ANDs the rows of fewer than h
    hashes, or of the same hash twice, counts more."""
    k = 25
    P, groups = _group_docs(D, page, G)
    sig = _big_sigs(D, k, h, page, G)
    rng = np.random.default_rng([D, h, G, 2])
    d = D - 1
    seqs = [_acgt(rng, k + 199 if doc == d else int(rng.integers(k, 120))) for doc in range(D)]
    ob = oracle_mod.CobsBank.empty(sig, P, D, h, k)
    ob.build(seqs, list(range(D)))
    read = seqs[d][50:50 + k + 99]
    nk = 100
    g = d // (8 * P)
    bit = d - g * 8 * P
    base = sum(sig[:g]) * P
    R = np.array([[oracle_mod.xxh64(oracle_mod.canonical_cobs(read[i:i + k]), seed=j) % sig[g] for j in range(h)]
                  for i in range(nk)], dtype=np.int64)
    values, counts = np.unique(R, return_counts=True)
    single = set(values[counts == 1].tolist())
    chosen, used = [], set()
    for j in range(h):
        i = next(i for i in range(j * 5, nk) if i not in used and int(R[i, j]) in single)
        used.add(i)
        chosen.append(i)
    assert len(set(chosen)) == h
    rows = ob.rows.copy()
    for j, i in enumerate(chosen):
        byte = base + int(R[i, j]) * P + (bit >> 3)
        assert rows[byte] >> (bit & 7) & 1, "the built image lacks the bit to be cleared"
        rows[byte] &= ~np.uint8(1 << (bit & 7))
    ob = oracle_mod.CobsBank(rows, sig, P, D, h, k)
    reads = [read, seqs[d][:k + 255]] + _reads(rng, 20, k)
    want = _expect(ob, reads)
    assert int(want[1][1][0]) == nk and int(want[1][0][0, d]) == nk - h, "the oracle misses nk - h"
    gb = _bank(xs, k, h, sig, D, page)
    gb.upload(ob.rows)
    for small in (1, 0):
        gb.set_probe_options(small_calls=small)
        _check(gb, want, reads, kernel)
    gb.close()


# ------------------------------------------------------------------ A3
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("h", [9, 10, 16])
@pytest.mark.parametrize("D", [100, 128])
def test_partitioned_probe_declines_more_than_8_hashes(xs, oracle_mod, D, h, mode):
    """The partitioned COBS probe holds at most 8 hashes per k-mer: a classic
    bank of <= 128 docs with more takes a direct kernel at every cobs_part."""
    from xspect2_amd import _lib
    k, sig = 21, [45_007]
    rng = np.random.default_rng([D, h, mode])
    seqs = [_acgt(rng, int(rng.integers(300, 900))) for _ in range(D)]
    ob = oracle_mod.CobsBank.empty(sig, (D + 7) // 8, D, h, k)
    ob.build(seqs, list(range(D)))
    gb = xs.Bank.create_cobs(k, h, sig, D)
    gb.set_probe_options(cobs_part=mode)
    gb.upload(ob.rows)
    reads = _read_set(rng, k, [_acgt(rng, _edge_lengths(k)[-1])]) + [s[:k + 255] for s in seqs[::7]]
    want = _expect(ob, reads, full_unit=True)
    _check(gb, want, reads, "slots<0,0,1,4>")
    assert gb.probe_path() == _lib.XS_PATH_GATHER
    gb.close()


# ------------------------------------------------------------------ A4
PAD_TABLE = [r for r in ROWS if (r[1], r[2]) in ((21, 7), (31, 1))]
assert {r[5].split("<")[0] for r in PAD_TABLE} == {"fast", "vslice", "wide", "slots", "general"}
assert {(513, 64, 2), (1025, 64, 3), (1537, 64, 4)} <= {(r[0], r[3], r[4]) for r in PAD_TABLE}  # vslice, 512 (G - 1) + 1


@pytest.mark.parametrize("D,k,h,page,G,kernel", PAD_TABLE, ids=[_case_id(r) for r in PAD_TABLE])
def test_padding_image_counts_every_kmer_for_every_doc(xs, oracle_mod, D, k, h, page, G, kernel):
    P, _ = _group_docs(D, page, G)
    sig = _sigs(D, k, h, page, G)
    rng = np.random.default_rng([k, h, D, G, 0xFF])
    reads = _read_set(rng, k, [_acgt(rng, _edge_lengths(k)[-1])])
    gb = _bank(xs, k, h, sig, D, page)
    _padding_image_case(gb, oracle_mod, sig, P, D, h, k, reads, kernel)
    gb.close()


@pytest.mark.parametrize("mode", [0, 3, 4])
@pytest.mark.parametrize("D", [100, 121])
def test_padding_image_classic_partitioned(xs, oracle_mod, D, mode):
    """D = 100: 4 padding bits in a 13-byte row, whose top bits carry the
    partitioned probe's k-mer id; D = 121: 7 padding bits in a 16-byte row."""
    k, h, sig = 21, 7, [5_003]
    P = (D + 7) // 8
    rng = np.random.default_rng([D, mode, 0xFF])
    reads = _read_set(rng, k, [_acgt(rng, _edge_lengths(k)[-1])])
    gb = xs.Bank.create_cobs(k, h, sig, D)
    gb.set_probe_options(cobs_part=mode)
    _padding_image_case(gb, oracle_mod, sig, P, D, h, k, reads, "cobspart" if mode else "fast<21,7>")
    gb.close()


# one narrow bank (many padding bits) per family: D, k, h, page, G, cobs_part, kernel
RANDOM_IMAGE_CASES = [
    (1, 31, 1, None, 1, 0, "fast<31,1>"),
    (100, 21, 7, None, 1, 0, "fast<21,7>"),
    (100, 21, 7, None, 1, 3, "cobspart"),
    (121, 21, 7, None, 1, 4, "cobspart"),
    (513, 31, 1, 64, 2, 0, "vslice<31,2>"),
    (129, 25, 3, None, 1, 0, "wide<0,0,C2,G1>"),
    (137, 31, 1, 17, 2, 0, "wide<31,1,C2,G2>"),
    (9, 25, 3, 1, 2, 0, "slots<0,0,4,1>"),
    (1, 25, 3, None, 1, 0, "slots<0,0,1,4>"),
    (129, 31, 1, 1, 17, 0, "general"),
    (2049, 21, 7, None, 1, 0, "general"),
]


@pytest.mark.parametrize("D,k,h,page,G,mode,kernel", RANDOM_IMAGE_CASES,
                         ids=[f"{c[6]}-D{c[0]}-k{c[1]}h{c[2]}-part{c[5]}" for c in RANDOM_IMAGE_CASES])
def test_random_image_with_padding_bits_matches_oracle(xs, oracle_mod, D, k, h, page, G, mode, kernel):
    """Random bytes in every byte of the image, padding included (for h > 1
    three draws ORed, 7/8 of the bits set, so that h ANDed rows keep hits):
    the oracle reads docs below D only."""
    P, _ = _group_docs(D, page, G)
    sig = _sigs(D, k, h, page, G)
    rng = np.random.default_rng([D, k, h, G, mode])
    nb = sum(sig) * P
    img = np.frombuffer(rng.bytes(nb), np.uint8)
    if h > 1:
        img = img | np.frombuffer(rng.bytes(nb), np.uint8) | np.frombuffer(rng.bytes(nb), np.uint8)
    img = img.copy()
    for b in range(D - (G - 1) * 8 * P, 8 * P):  # the bank's last row: every padding bit set
        img[-P + (b >> 3)] |= 1 << (b & 7)
    ob = oracle_mod.CobsBank(img, sig, P, D, h, k)
    gb = xs.Bank.create_cobs(k, h, sig, D, page_size=page, compact=page is not None)
    gb.set_probe_options(cobs_part=mode)
    gb.upload(ob.rows)
    assert np.array_equal(gb.download(), ob.rows), "download differs from the uploaded bytes"
    reads = _read_set(rng, k, [_acgt(rng, _edge_lengths(k)[-1])])
    want = _expect(ob, reads)
    assert 0 < int(want[1][0].sum()) < int(want[1][1].sum()) * D
    for small in (1, 0):
        gb.set_probe_options(small_calls=small)
        _check(gb, want, reads, kernel)
    best, bh, bnk, btot = gb.query_best(reads, want_totals=True)
    want_h, want_n = want[1]
    m = want_h.max(axis=1)
    ties = (want_h == m[:, None]).sum(axis=1)
    assert np.array_equal(best, np.where(ties == 1, want_h.argmax(axis=1), AMBIGUOUS).astype(np.uint32))
    assert np.array_equal(bh, m) and np.array_equal(bnk, want_n)
    assert np.array_equal(btot[:D], want_h.sum(axis=0, dtype=np.uint64)) and int(btot[D]) == int(want_n.sum())
    gb.close()


# ------------------------------------------------------------------ A5
TINY = (1, 2, 3, 8)
# one classic and one compact bank per family, and the partitioned probe: D, k, h, page, G, cobs_part, kernel
TINY_BANKS = [
    (100, 21, 7, None, 1, 0, "fast<21,7>"),
    (100, 21, 7, None, 1, 3, "cobspart"),
    (512, 31, 1, None, 1, 0, "vslice<31,1>"),
    (513, 21, 1, 64, 2, 0, "vslice<0,2>"),
    (129, 25, 3, None, 1, 0, "wide<0,0,C2,G1>"),
    (137, 31, 1, 17, 2, 0, "wide<31,1,C2,G2>"),
    (128, 25, 16, None, 1, 0, "slots<0,0,1,4>"),
    (17, 25, 3, 1, 3, 0, "slots<0,0,4,1>"),
    (2049, 21, 7, None, 1, 0, "general"),
    (129, 25, 16, 1, 17, 0, "general"),
]
TINY_CASES = [b + (s,) for b in TINY_BANKS for s in TINY]


@pytest.mark.parametrize("D,k,h,page,G,mode,kernel,s", TINY_CASES,
                         ids=[f"{c[6]}-D{c[0]}-k{c[1]}h{c[2]}-part{c[5]}-sig{c[7]}" for c in TINY_CASES])
def test_tiny_signature_sizes(xs, oracle_mod, D, k, h, page, G, mode, kernel, s):
    """Groups of 1, 2, 3 and 8 rows (group g of a compact bank takes the g-th
    next of them): the banks saturate, which is the point; equality only."""
    P, _ = _group_docs(D, page, G)
    sig = [TINY[(TINY.index(s) + g) % len(TINY)] for g in range(G)]
    rng = np.random.default_rng([D, k, h, G, mode, s])
    seqs = [_acgt(rng, int(rng.integers(k, k + 3))) for _ in range(D)]  # 1-3 k-mers a doc: some bits stay clear
    ob = oracle_mod.CobsBank.empty(sig, P, D, h, k)
    ob.build(seqs, list(range(D)))
    gb = xs.Bank.create_cobs(k, h, sig, D, page_size=page, compact=page is not None)
    gb.set_probe_options(cobs_part=mode)
    gb.build(seqs, list(range(D)))
    assert np.array_equal(gb.download(), ob.rows), "device-built bank differs"
    reads = _read_set(rng, k, [_acgt(rng, _edge_lengths(k)[-1])]) + seqs[:20]
    want = _expect(ob, reads)
    for small in (1, 0):
        gb.set_probe_options(small_calls=small)
        _check(gb, want, reads, kernel)
    gb.close()
