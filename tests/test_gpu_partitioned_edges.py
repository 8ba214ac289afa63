"""The partitioned probes at their block, read and partition edges (GPU).

tests/test_gpu_parity.py runs cobspart and bloompart on seeded reads of random
length, which rarely put a read boundary on a bucket-block boundary.  Here
every batch is a named layout of tests/partition_layouts.py: reads of exactly
the k-mer counts that end on, one before and one after a block edge, fill the
resolve pass's LDS counter rows exactly or exceed them by one read (with
k-mer-holding reads or with empty ones), fit the bucket pass's staged read
offsets exactly or exceed them by one, leave a last block of 0, 1 or T-1
k-mers (mod T) behind leading, embedded and trailing empty reads, or span
many blocks with one read.  tests/test_partition_layouts.py asserts, without
a GPU, that each layout reaches the branch it is named after.

Bank images are closed forms wherever possible, so a failure isolates read
attribution, store-versus-add and zeroing from all hashing: every row with
the bits of a boundary set of docs (a read's count is its k-mer count on
those docs and 0 elsewhere), all ones, and dense random rows (the AND of a
k-mer's rows about half full) against the oracle.  The doc counts sit on
both sides of every nwords edge and of emb_max_docs; the signature and filter
sizes on the partition-count edges (one partition, a last partition of one
row or 64 bits, kCobsPadParts and one more, kPartMax and one row more).
"""
from __future__ import annotations

import numpy as np
import pytest

import partition_layouts as pl
from test_gpu_parity import _explain

pytestmark = pytest.mark.gpu

STEPS = (1, 3)
AMBIGUOUS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


_BATCHES: dict = {}


def _batches(T, k, word_phase=False):
    """name -> {step: reads} of every layout at block size T: built once per (T, k)."""
    key = (T, k, word_phase)
    if key not in _BATCHES:
        rng = np.random.default_rng([T, k])
        _BATCHES[key] = {name: {step: pl.make_reads(rng, counts, k, step) for step in STEPS}
                         for name, counts in pl.layouts(T, word_phase).items()}
    return _BATCHES[key]


# ---------------------------------------------------------------- COBS
COBS_CASES = [(1, 21, 7), (32, 21, 7), (33, 31, 1), (64, 21, 7), (65, 25, 3), (96, 16, 8), (97, 21, 7),
              (pl.EMB_MAX_DOCS, 21, 7), (pl.EMB_MAX_DOCS + 1, 21, 7), (128, 31, 8)]
COBS_SIG = 30_011


def _chosen_docs(D):
    return sorted(d for d in {0, 31, 32, 63, 64, 95, 96, D - 1} if 0 <= d < D)


def _image(sig, D, docs):
    """A classic bank image whose every row has exactly the bits of `docs` set."""
    row = np.zeros((D + 7) // 8, np.uint8)
    for d in docs:
        row[d >> 3] |= 1 << (d & 7)
    return np.tile(row, sig)


def _dense_image(rng, sig, D, h):
    """Random rows of bit density 0.5^(1/h): the AND of a k-mer's h rows is about half full."""
    P = (D + 7) // 8
    bits = rng.random((sig, 8 * P), dtype=np.float32) < 0.5 ** (1.0 / h)
    bits[:, D:] = False
    return np.packbits(bits, axis=1, bitorder="little").reshape(-1)


def _best(want_h):
    m = want_h.max(axis=1)
    ties = (want_h == m[:, None]).sum(axis=1)
    return np.where(ties == 1, want_h.argmax(axis=1), AMBIGUOUS).astype(np.uint32), m


def _check_cobs(gb, reads, step, want_h, want_n, what):
    """query, query_totals and query_best of one batch against the expectation."""
    D = want_h.shape[1]
    got_h, got_n = gb.query(reads, step=step)
    assert gb.probe_kernel() == "cobspart", f"{what}: routed to {gb.probe_kernel()}"
    assert np.array_equal(got_n, want_n), f"{what}: num_kmers differ"
    assert got_h.shape == want_h.shape
    assert np.array_equal(got_h, want_h), f"{what}: " + _explain(got_h, want_h, reads)
    tot, nk = gb.query_totals(reads, step=step)
    assert gb.probe_kernel() == "cobspart"
    assert np.array_equal(tot, want_h.sum(axis=0, dtype=np.uint64)), f"{what}: totals differ"
    assert nk == int(want_n.sum())
    best, bh, bnk, btot = gb.query_best(reads, step=step, want_totals=True)
    assert gb.probe_kernel() == "cobspart"
    want_best, want_max = _best(want_h)
    assert np.array_equal(bh, want_max), f"{what}: best hits differ"
    assert np.array_equal(best, want_best), f"{what}: best docs differ"
    assert np.array_equal(bnk, want_n)
    assert np.array_equal(btot[:D], want_h.sum(axis=0, dtype=np.uint64)) and int(btot[D]) == int(want_n.sum())


def _closed(ob, reads, step, counts, docs):
    """The closed form of a chosen-documents image, which the oracle is held to as well."""
    want_h = pl.closed_form(counts, ob.D, docs)
    want_n = np.asarray(counts, dtype=np.uint64)
    oh, on = ob.query(reads, step=step)
    assert np.array_equal(on, want_n) and np.array_equal(oh, want_h), "the oracle misses the closed form"
    return want_h, want_n


@pytest.mark.parametrize("D,k,h", COBS_CASES, ids=[f"D{c[0]}-k{c[1]}h{c[2]}" for c in COBS_CASES])
def test_cobspart_layouts(xs, oracle_mod, D, k, h):
    """Every layout at T = kCobsCK, steps 1 and 3, on the chosen-documents,
    all-ones and dense random images of one bank (30 k rows in 30 partitions)."""
    T, sig, P = pl.COBS_CK, COBS_SIG, (D + 7) // 8
    assert pl.cobs_plan(sig, h, 3)["P"] == 30
    lay = pl.layouts(T)
    batches = _batches(T, k)
    gb = xs.Bank.create_cobs(k, h, [sig], D)
    gb.set_probe_options(cobs_part=3)
    for docs in (_chosen_docs(D), list(range(D))):
        ob = oracle_mod.CobsBank(_image(sig, D, docs), [sig], P, D, h, k)
        gb.upload(ob.rows)
        for name, counts in lay.items():
            for step in STEPS:
                reads = batches[name][step]
                want_h, want_n = _closed(ob, reads, step, counts, docs)
                _check_cobs(gb, reads, step, want_h, want_n, f"{name}, step {step}, {len(docs)} docs set")
    ob = oracle_mod.CobsBank(_dense_image(np.random.default_rng([D, k, h]), sig, D, h), [sig], P, D, h, k)
    gb.upload(ob.rows)
    for name, counts in lay.items():
        for step in STEPS:
            reads = batches[name][step]
            want_h, want_n = ob.query(reads, step=step)
            assert np.array_equal(want_n, np.asarray(counts, dtype=np.uint64))
            full = want_h[want_n > 0] == want_n[want_n > 0, None]
            assert want_h.any() and not full.all(), "the dense image decides nothing"
            _check_cobs(gb, reads, step, want_h, want_n, f"{name}, step {step}, dense")
    gb.close()


@pytest.mark.parametrize("D,k,h", COBS_CASES, ids=[f"D{c[0]}-k{c[1]}h{c[2]}" for c in COBS_CASES])
def test_cobspart_layouts_in_workspace_ranges(xs, oracle_mod, D, k, h):
    """The long and off_by_one layouts in a 1 MiB workspace: the bucket blocks
    run in ranges of R (3 at h = 7 and 8, 8 at h = 3, 24 at h = 1) that reuse
    it.  The long read is 3 R blocks, so it crosses two range boundaries;
    off_by_one is repeated over at least 2 R + 1 blocks, as it is and one block
    later, so that range boundaries fall on read boundaries and inside edge
    reads (at R = 3: 3 T and 6 T lie between two reads as it is, and 3 T
    inside a read one block later).  The pass counters show at least 3
    ranges."""
    T, sig, P = pl.COBS_CK, COBS_SIG, (D + 7) // 8
    docs = _chosen_docs(D)
    ob = oracle_mod.CobsBank(_image(sig, D, docs), [sig], P, D, h, k)
    gb = xs.Bank.create_cobs(k, h, [sig], D)
    gb.set_probe_options(cobs_part=3, workspace_mib=1)
    gb.upload(ob.rows)
    gb.set_profiling(True)
    rng = np.random.default_rng([D, k, h, 1])
    R = pl.cobs_plan(sig, h, 3, 1 << 40, workspace_mib=1)["rblk"]
    assert R == {7: 3, 8: 3, 3: 8, 1: 24}[h]
    unit = pl.off_by_one_unit(T)
    obo = unit * (-(-(2 * R + 1) * T // sum(unit))) + [5]
    long = pl.long_layout(T, blocks=3 * R)
    for name, counts in (("long", long), ("off_by_one", obo), ("shifted", [T] + obo)):
        ko = pl.kofs(counts)
        edge = R * T  # the first range boundary, as a k-mer id
        assert ko[-1] > 2 * edge
        if name == "long":
            assert ko[1] < edge < 2 * edge < ko[2]           # inside the long read
        elif R == 3:
            crossed = any(ko[r] < edge < ko[r + 1] for r in range(len(counts)))
            assert crossed == (name == "shifted") and (name == "shifted" or 2 * edge in ko)
        for step in STEPS:
            reads = pl.make_reads(rng, counts, k, step)
            plan = pl.cobs_plan(sig, h, 3, pl.kbound(reads, step), workspace_mib=1)
            assert plan["rblk"] == R and plan["ranges"] >= 3
            want_h, want_n = _closed(ob, reads, step, counts, docs)
            gb.pass_stats()
            got_h, got_n = gb.query(reads, step=step)
            st = gb.pass_stats()
            assert gb.probe_kernel() == "cobspart"
            assert st["bucket"][1] == st["lookup"][1] == st["resolve"][1] >= 3
            assert np.array_equal(got_n, want_n)
            assert np.array_equal(got_h, want_h), f"{name}, step {step}: " + _explain(got_h, want_h, reads)
    gb.set_profiling(False)
    for step in STEPS:  # and totals / best doc, which take no hit matrix to the host
        reads = pl.make_reads(rng, long, k, step)
        want_h, want_n = _closed(ob, reads, step, long, docs)
        _check_cobs(gb, reads, step, want_h, want_n, f"long, step {step}, 1 MiB workspace")
    gb.close()


# 21-mers one of whose 7 rows is the bank's last row (found by hashing random
# 21-mers, about sig / h of them; the test checks the claim)
LAST_ROW_KMERS = {524_289: b"ACGCACTAACTAGGTACTGAT", 1_048_577: b"GTTACCGTTGGGTTAGCGACT"}

PART_EDGES = [(1024, 3), (1025, 3), (65_536, 3), (524_288, 4), (524_289, 4), (1_048_576, 4), (1_048_577, 4)]


def _rows_of(oracle_mod, reads, k, h, sig):
    """Row indices of every k-mer of `reads` at step 1, computed on the CPU."""
    out = []
    for r in reads:
        for i in range(len(r) - k + 1):
            c = oracle_mod.canonical_cobs(r[i:i + k])
            out += [oracle_mod.xxh64(c, seed=j) % sig for j in range(h)]
    return np.asarray(out, dtype=np.int64)


@pytest.mark.parametrize("sig,mode", PART_EDGES, ids=[f"sig{s}-mode{m}" for s, m in PART_EDGES])
def test_cobspart_partition_count_edges(xs, oracle_mod, sig, mode):
    """One partition, a last partition of one row, 64 whole partitions, 512
    (padded runs) against 513 (unpadded), kPartMax against one row more (the
    shift grows): dense random image, one batch of about 25 k k-mers whose
    rows reach every partition, against the oracle.  The power-of-two sizes
    are Barrett divisors of their own."""
    D, k, h = 100, 21, 7
    plan = pl.cobs_plan(sig, h, mode)
    rng = np.random.default_rng(sig)
    nb = sig * 13
    rows = (np.frombuffer(rng.bytes(nb), np.uint8) | np.frombuffer(rng.bytes(nb), np.uint8)
            | np.frombuffer(rng.bytes(nb), np.uint8)).reshape(sig, 13).copy()  # 7/8 of the bits: AND of 7 ~0.39
    rows[:, 12] &= 0x0F
    ob = oracle_mod.CobsBank(rows.reshape(-1), [sig], 13, D, h, k)
    reads = pl.make_reads(rng, [150] * 160 + [0, 1, 700], k, 1)
    if sig in LAST_ROW_KMERS:
        reads.insert(7, reads[7][:40] + LAST_ROW_KMERS[sig] + reads[7][40:80])
    ridx = _rows_of(oracle_mod, reads, k, h, sig)
    assert np.bincount(ridx >> plan["shift"], minlength=plan["P"]).min() >= 1, "a partition receives no entry"
    if plan["last_rows"] == 1:  # sig 1025 by itself, the large ones by the k-mer put in
        assert (ridx == sig - 1).any(), "no k-mer of the batch has the last partition's row"
    gb = xs.Bank.create_cobs(k, h, [sig], D)
    gb.set_probe_options(cobs_part=mode)
    gb.upload(ob.rows)
    for step in STEPS:
        want_h, want_n = ob.query(reads, step=step)
        full = want_h[want_n > 0] == want_n[want_n > 0, None]
        assert want_h.any() and not full.all()
        _check_cobs(gb, reads, step, want_h, want_n, f"sig {sig}, mode {mode}, step {step}")
    gb.close()


# ---------------------------------------------------------------- rbloom
BLOOM_CASES = [(21, 7), (31, 7), (16, 1), (25, 8)]
BLOOM_BYTES = 30_011
BLOOM_SIZES = [128, 136, 8192, 131_072, 131_080]


def _check_bloom(gb, reads, step, want_h, want_n, what):
    got_h, got_n = gb.query(reads, step=step)
    assert gb.probe_path() == 1 and gb.probe_kernel() == "bloompart", f"{what}: routed to {gb.probe_kernel()}"
    assert np.array_equal(got_n, want_n), f"{what}: num_kmers differ"
    assert got_h.shape == (len(reads), 1)
    assert np.array_equal(got_h[:, 0], want_h), f"{what}: " + _explain(got_h, want_h[:, None], reads)
    tot, nk = gb.query_totals(reads, step=step)
    assert gb.probe_path() == 1 and gb.probe_kernel() == "bloompart"
    assert int(tot[0]) == int(want_h.sum()) and nk == int(want_n.sum()), f"{what}: totals differ"
    best, bh, bnk, btot = gb.query_best(reads, step=step, want_totals=True)
    assert gb.probe_path() == 1 and gb.probe_kernel() == "bloompart"
    assert np.array_equal(bh, want_h) and np.array_equal(bnk, want_n), f"{what}: best hits differ"
    assert int(btot[0]) == int(want_h.sum()) and int(btot[1]) == int(want_n.sum())


def _bloom_case(xs, oracle_mod, k, K, nbytes):
    T = pl.PART_KMERS
    lay = pl.layouts(T, word_phase=True)
    batches = _batches(T, k, word_phase=True)
    gb = xs.Bank.create_bloom(k, nbytes, K)
    gb.set_probe_options(bloom_part=3)
    for fill in (0xFF, 0x00):  # closed forms: every k-mer a member, none
        gb.upload(np.full(nbytes, fill, dtype=np.uint8))
        for name, counts in lay.items():
            for step in STEPS:
                want_n = np.asarray(counts, dtype=np.uint64)
                want_h = want_n.astype(np.uint32) if fill else np.zeros(len(counts), dtype=np.uint32)
                _check_bloom(gb, batches[name][step], step, want_h, want_n, f"{name}, step {step}, fill {fill:#x}")
    rng = np.random.default_rng([k, K, nbytes])
    bits = np.packbits(rng.random(nbytes * 8, dtype=np.float32) < 0.5 ** (1.0 / K), bitorder="little")
    bf = oracle_mod.BloomFilter(bits, K, k)
    gb.upload(bf.bits)
    for name, counts in lay.items():
        for step in STEPS:
            reads = batches[name][step]
            want_h, want_n = bf.query(reads, step=step)
            assert np.array_equal(want_n, np.asarray(counts, dtype=np.uint64))
            assert 0 < int(want_h.sum()) < int(want_n.sum()), "the random filter decides nothing"
            _check_bloom(gb, reads, step, want_h, want_n, f"{name}, step {step}, random bits")
    gb.close()


@pytest.mark.parametrize("k,K", BLOOM_CASES, ids=[f"k{k}K{K}" for k, K in BLOOM_CASES])
def test_bloompart_layouts(xs, oracle_mod, k, K):
    """Every layout at T = kPartKmers (word_phase included), steps 1 and 3, on
    an all-ones, an all-zeros and a random filter of 30 011 bytes (235
    partitions of 1024 bits, the last one partial)."""
    assert pl.bloom_plan(BLOOM_BYTES)["P"] == 235
    _bloom_case(xs, oracle_mod, k, K, BLOOM_BYTES)


@pytest.mark.parametrize("nbytes", BLOOM_SIZES)
def test_bloompart_partition_count_edges(xs, oracle_mod, nbytes):
    """One partition, a last partition of 64 bits, 64 whole partitions,
    kPartMax of them, and 8 bytes more (the shift grows: 513 partitions)."""
    _bloom_case(xs, oracle_mod, 21, 7, nbytes)


# ---------------------------------------------------------------- more than one block per lookup group
def test_cobspart_many_blocks_per_call(xs, oracle_mod):
    """cobs_lookup_kernel takes gb bucket blocks per queue ticket; gb exceeds 1
    only when a range has at least twice as many blocks as one XCD has waves
    (about 1.1 M k-mers on an MI355X).  gb cannot be observed from outside:
    this case gives the call 1.3 M k-mers (the off_by_one and cnt_over units
    repeated, plus one block), which is over that size on this chip, and checks
    the closed form of the chosen-documents image, below and above
    emb_max_docs.  No oracle query."""
    T, k, h, sig = pl.COBS_CK, 21, 7, COBS_SIG
    counts = pl.repeated(T, 1_300_000)
    want_n = np.asarray(counts, dtype=np.uint64)
    rng = np.random.default_rng(13)
    batches = {step: pl.make_reads(rng, counts, k, step) for step in STEPS}
    for D in (100, 128):
        docs = _chosen_docs(D)
        want_h = pl.closed_form(counts, D, docs)
        gb = xs.Bank.create_cobs(k, h, [sig], D)
        gb.set_probe_options(cobs_part=3)
        gb.upload(_image(sig, D, docs))
        for step in STEPS:
            assert sum(len(r) for r in batches[step]) < pl.HOST_FIRST  # one chunk: the layout's k-mer ids
            _check_cobs(gb, batches[step], step, want_h, want_n, f"1.3 M k-mers, D {D}, step {step}")
        gb.close()


def test_bloompart_many_blocks_per_call(xs):
    """bloom_lookup_kernel takes groups of 64 bucket blocks per queue ticket:
    0.7 M k-mers (the off_by_one and cnt_over units at T = kPartKmers repeated,
    plus one block) are some 690 blocks, 11 groups per partition, the last one
    partial.  All-ones filter: hits == num_kmers.  Which group a block falls
    into cannot be observed from outside.  No oracle query."""
    T, k, K, nbytes = pl.PART_KMERS, 21, 7, BLOOM_BYTES
    counts = pl.repeated(T, 700_000)
    want_n = np.asarray(counts, dtype=np.uint64)
    rng = np.random.default_rng(14)
    gb = xs.Bank.create_bloom(k, nbytes, K)
    gb.set_probe_options(bloom_part=3)
    gb.upload(np.full(nbytes, 0xFF, dtype=np.uint8))
    for step in STEPS:
        reads = pl.make_reads(rng, counts, k, step)
        assert sum(len(r) for r in reads) < pl.HOST_FIRST
        _check_bloom(gb, reads, step, want_n.astype(np.uint32), want_n, f"0.7 M k-mers, step {step}")
    gb.close()
