"""MLST typing of contigs on the device: the chunk reduction
(xs_mlst_chunk_top_device) and the splitter (xs_mlst_split_device) alone, the
whole call (xs_mlst_type_contigs / _device) against the CPU oracle, its ranges
and bounded workspace, and ``predict_columnar`` of the MLST model by the new road.

Expected values come from the oracle only: ``oracle.sequence_splitter``,
``CobsBank.query`` over the chunks, and the rule of include/xspect_hip.h restated
in numpy below (``_chunk_rule``).  Every value is an integer and compared exactly."""
from __future__ import annotations

import numpy as np
import pytest

from xspect2_amd.file_io import Record, get_record_iterator, write_fasta

gpu = pytest.mark.gpu

K = 21
SENTINEL = 0x5A5A5A5A
NONE = 0xFFFFFFFF
THRESHOLD = 50
SMALL_RULE = (2000, 20000, 60000, THRESHOLD)  # long_len, scale10_len, scale100_len, threshold
LOCUS_DOCS = (40, 70, 130)
PAGE = 2  # 16 alleles per doc group
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


# ---------------------------------------------------------------- the rule, restated
def _chunk_rule(rows: np.ndarray, threshold: int):
    """(top, top_score, n_tied) of one record's chunk rows [chunks, D]: per allele the sum of the
    counts > threshold, the first chunk with such a count and that count; the largest sum > 0
    wins, ties by the lower first chunk, the higher first score, the lower doc."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, rows.shape[-1])
    D = rows.shape[1]
    if rows.shape[0] == 0:
        return NONE, 0, 0
    keep = rows > threshold
    total = (rows * keep).sum(axis=0)
    cand = np.flatnonzero(total > 0)
    if cand.size == 0:
        return NONE, 0, 0
    first = keep.argmax(axis=0)
    fscore = rows[first, np.arange(D)]
    best = min(cand, key=lambda d: (-int(total[d]), int(first[d]), -int(fscore[d]), int(d)))
    return int(best), int(total[best]), int((total == total[best]).sum())


def _row_rule(row: np.ndarray):
    """xs_mlst_type's rule for a record probed whole."""
    m = int(row.max())
    return int(row.argmax()), m, int((row == m).sum())


def _to_dev(torch_dev, a: np.ndarray):
    torch, dev = torch_dev
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 8:
        return torch.from_numpy(a.view(np.int64).reshape(-1)).to(dev)
    if a.dtype.itemsize == 1:
        return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
    return torch.from_numpy(a.view(np.int32).reshape(-1)).to(dev)


# ---------------------------------------------------------------- 1. the reduction alone
def _crafted(D: int, rng):
    """Owners' chunk rows made to break a wrong reduction (docs A < B < C where D allows)."""
    docs = sorted({0, D // 2, D - 1})
    A, B, C = (docs + [docs[-1]] * 2)[:3]
    owners = []

    def owner(n_chunks, cells):
        r = np.zeros((n_chunks, D), dtype=np.uint32)
        for c, d, v in cells:
            r[c, d] = v
        owners.append(r)

    owner(3, [(0, A, 100), (1, A, 90), (2, B, 150)])                       # 0 by sum: A (190 > 150)
    owner(2, [(1, A, 60), (0, B, 60)])                                     # 1 equal sums: the first chunk (B)
    owner(2, [(0, A, 60), (0, B, 70), (1, A, 70), (1, B, 60)])             # 2 same first chunk: higher score there (B)
    owner(1, [(0, C, 80), (0, B, 80), (0, A, 80)])                         # 3 equal on all three: the lower doc
    owner(1, [(0, A, THRESHOLD), (0, B, THRESHOLD + 1)])                   # 4 exactly the threshold is dropped
    owner(2, [(0, A, THRESHOLD), (1, B, 1), (1, C, THRESHOLD)])            # 5 nothing passes
    owner(0, [])                                                           # 6 no chunks
    owner(1, [(0, C, 77)])                                                 # 7 one chunk
    owner(2, [(0, A, 0x7FFFFFFF), (1, B, 0x90000000)])                     # 8 unsigned compares
    owner(3, [(0, A, 51), (1, A, 51), (2, B, 102)])                        # 9 n_tied over different first chunks
    owners.append(rng.integers(0, 121, (40, D), dtype=np.uint64).astype(np.uint32))  # many chunks, many passing
    for _ in range(300):  # more owners than one block's waves; counts around the threshold tie often
        owners.append(rng.integers(THRESHOLD - 4, THRESHOLD + 4, (int(rng.integers(0, 4)), D),
                                   dtype=np.uint64).astype(np.uint32))
    begin = np.concatenate([[0], np.cumsum([o.shape[0] for o in owners])]).astype(np.uint64)
    rows = np.concatenate(owners, axis=0)
    want = np.array([_chunk_rule(o, THRESHOLD) for o in owners], dtype=np.uint64).astype(np.uint32)
    return rows, begin, want, (A, B, C)


@gpu
@pytest.mark.parametrize("D", [1, 63, 64, 65, 258, 1430])
def test_chunk_top_crafted_rows(xs, torch_dev, D):
    """Crafted owners (see _crafted), with out_stride 1 and 3 over sentinel-prefilled
    outputs, n_tied null, and a rows base 4 but not 16 bytes aligned."""
    torch, dev = torch_dev
    rows, begin, want, (A, B, C) = _crafted(D, np.random.default_rng(40 + D))
    if D == 258:  # the restatement itself, on the cases written out above
        assert want[:10].tolist() == [[A, 190, 1], [B, 60, 2], [B, 130, 2], [A, 80, 3], [B, 51, 1], [NONE, 0, 0],
                                      [NONE, 0, 0], [C, 77, 1], [B, 0x90000000, 1], [A, 102, 2]]
    n_own, nc = begin.size - 1, rows.shape[0]
    d_begin = _to_dev(torch_dev, begin)
    s = torch.cuda.current_stream(dev).cuda_stream
    for off in (0, 1):
        flat = np.full(off + rows.size + 8, 0xFFFFFFFF, dtype=np.uint32)  # a read outside the matrix would win
        flat[off:off + rows.size] = rows.reshape(-1)
        big = _to_dev(torch_dev, flat)
        assert big.data_ptr() % 16 == 0
        d_hits = big[off:off + rows.size]
        for stride, want_tied in ((1, True), (3, True), (1, False)):
            outs = [torch.full((n_own * stride,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]
            xs.mlst_chunk_top_device(d_hits, nc, D, d_begin, n_own, THRESHOLD, outs[0], outs[1],
                                     outs[2] if want_tied else None, stride, stream=s)
            torch.cuda.synchronize(dev)
            got = [o.cpu().numpy().view(np.uint32) for o in outs]
            for c in range(3 if want_tied else 2):
                assert np.array_equal(got[c][0::stride], want[:, c]), (D, off, stride, c)
                for rest in range(1, stride):
                    assert (got[c][rest::stride] == SENTINEL).all(), (D, off, stride, c)
            if not want_tied:
                assert (got[2] == SENTINEL).all()


# ---------------------------------------------------------------- 2. the splitter alone
def _split_on_device(xs, torch_dev, records, index, width, rule):
    torch, dev = torch_dev
    from xspect2_amd.packing import pack_sequences
    pr = pack_sequences(records)
    lengths = [len(records[i]) for i in index]
    n_chunks, n_bytes = xs.mlst_split_size(lengths, width, K, rule)
    d_seqs = _to_dev(torch_dev, pr.buf[:max(pr.nbytes, 1)])
    d_offs = _to_dev(torch_dev, pr.offsets)
    d_index = _to_dev(torch_dev, np.asarray(index, dtype=np.uint32))
    text = torch.full((n_bytes + 64 + 16,), 0xEE, dtype=torch.uint8, device=dev)
    offs = torch.full((n_chunks + 1,), -1, dtype=torch.int64, device=dev)
    begin = torch.full((len(index) + 1,), -1, dtype=torch.int64, device=dev)
    xs.mlst_split_device(d_seqs, d_offs, d_index, len(index), width, K, text, offs, begin, rule,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return n_chunks, n_bytes, text.cpu().numpy(), offs.cpu().numpy().view(np.uint64), begin.cpu().numpy().view(np.uint64)


def _check_split(oracle_mod, got, records, index, widths):
    n_chunks, n_bytes, text, offs, begin = got
    parts = [oracle_mod.sequence_splitter(records[i], w, K) for i, w in zip(index, widths)]
    flat = [p for ps in parts for p in ps]
    assert n_chunks == len(flat) and n_bytes == sum(map(len, flat))
    assert begin.tolist() == np.concatenate([[0], np.cumsum([len(ps) for ps in parts])]).tolist()
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in flat])]).tolist()
    assert text[:n_bytes].tobytes() == b"".join(flat)
    assert (text[n_bytes:n_bytes + 64] == 0).all() and (text[n_bytes + 64:] == 0xEE).all()
    return parts


@gpu
def test_splitter_matches_oracle_at_the_edges(xs, torch_dev, oracle_mod):
    """k 21, W 450, S 430: a length of (m-1) S + W (the tail of k-1 bytes is appended to the last
    chunk, which repeats them), that length -1 and +1, W, W-1 (one chunk) and long_len; records
    not listed lie between the listed ones."""
    rng = np.random.default_rng(7)
    W, S = 450, 430
    lens = [4 * S + W, 4 * S + W - 1, 4 * S + W + 1, W, W - 1, SMALL_RULE[0], 9 * S + W]
    records, index = [], []
    for n in lens:
        records.append(ACGT[rng.integers(0, 4, 150)].tobytes())
        index.append(len(records))
        records.append(ACGT[rng.integers(0, 4, n)].tobytes())
    parts = _check_split(oracle_mod, _split_on_device(xs, torch_dev, records, index, W, SMALL_RULE), records, index,
                         [W] * len(index))
    assert [len(p) for p in parts] == [5, 5, 6, 1, 1, 5, 10]
    tail = records[index[0]][-(K - 1):]
    assert len(parts[0][-1]) == W + K - 1 and parts[0][-1].endswith(tail + tail)  # the repeat
    assert len(parts[1][-1]) == W - 1 and len(parts[2][-1]) == K


@gpu
def test_splitter_scales_with_the_record_length(xs, torch_dev, oracle_mod):
    """The small rule's scale boundaries: 19,999 / 20,000 bytes (W 450 / 4,500) and 59,999 /
    60,000 (4,500 / 45,000)."""
    rng = np.random.default_rng(8)
    lens = [19_999, 20_000, 59_999, 60_000]
    records = [ACGT[rng.integers(0, 4, n)].tobytes() for n in lens]
    index = list(range(4))
    widths = [450, 4500, 4500, 45000]
    parts = _check_split(oracle_mod, _split_on_device(xs, torch_dev, records, index, 450, SMALL_RULE), records, index,
                         widths)
    assert [len(p[0]) for p in parts] == widths


# ---------------------------------------------------------------- 3. the whole call against the oracle
def _alleles(rng, D, length):
    base = rng.integers(0, 4, length)
    out = []
    for _ in range(D):
        a = base.copy()
        pos = rng.choice(length, size=int(rng.integers(0, 12)), replace=False)
        a[pos] = (a[pos] + 1) % 4
        out.append(ACGT[a].tobytes())
    out[11] = out[4]  # an allele identical to another of its locus
    return out


def _expected(oracle_mod, obs, widths, records, rule, step):
    """(top, score, tied) [n, loci] and num_kmers [n] by the oracle."""
    long_len, s10, s100, thr = rule
    n, L = len(records), len(obs)
    out = np.zeros((3, n, L), dtype=np.uint32)
    dropped = 0  # chunk counts in 1 .. threshold
    for l, (ob, _) in enumerate(obs):
        short = [i for i, r in enumerate(records) if len(r) < long_len]
        rows = ob.query([records[i] for i in short], step=step)[0] if short else []
        for j, i in enumerate(short):
            out[:, i, l] = _row_rule(rows[j])
        for i, r in enumerate(records):
            if len(r) < long_len:
                continue
            if len(r) < 1_000_000:  # below its own boundaries the oracle's splitter takes the width as given
                w = widths[l] * (1 if len(r) < s10 else 10 if len(r) < s100 else 100)
            else:                   # from there it scales the width itself, by the reference's constants
                assert (s10, s100) == (1_000_000, 10_000_000)
                w = widths[l]
            crow = ob.query(oracle_mod.sequence_splitter(r, w, K), step=step)[0]
            dropped += int(((crow >= 1) & (crow <= thr)).sum())
            out[:, i, l] = _chunk_rule(crow, thr)
    nk = np.array([(len(r) - K) // step + 1 if len(r) >= K else 0 for r in records], dtype=np.uint64)
    return out[0], out[1], out[2], nk, dropped


def _scheme_data(oracle_mod, seed=20261021):
    rng = np.random.default_rng(seed)
    obs, alleles = [], []
    for li, D in enumerate(LOCUS_DOCS):
        al = _alleles(rng, D, 450 + 10 * li)
        terms = len(al[0]) - K + 1
        sig = [oracle_mod.signature_size(terms, 1, 0.001)] * ((D + 8 * PAGE - 1) // (8 * PAGE))
        ob = oracle_mod.CobsBank.empty(sig, PAGE, D, 1, K)
        ob.build(al, list(range(D)))
        obs.append((ob, sig))
        alleles.append(al)
    widths = [len(al[0]) for al in alleles]

    def rand(n):
        return ACGT[rng.integers(0, 4, n)].tobytes()

    def window():
        al = alleles[int(rng.integers(0, 3))]
        a = al[int(rng.integers(0, len(al)))]
        st = int(rng.integers(0, len(a) - 150 + 1))
        return a[st:st + 150]

    one_each = rand(700) + alleles[0][3] + rand(600) + alleles[1][5] + rand(500) + alleles[2][7] + rand(400)
    straddle = rand(300) + alleles[0][9] + rand(1500) + alleles[2][21] + rand(300)  # allele 9 over chunks 0 and 1 of locus 0
    twin = rand(900) + alleles[0][4] + rand(50) + alleles[1][11] + rand(800)  # alleles 4 and 11 are the same text
    fragment = rand(1200) + alleles[1][8][100:160] + rand(1300)                 # 40 k-mers: under the threshold
    random_contig = rand(3000)
    tail_len = 5 * 430 + 450  # locus 0: the repeated tail
    repeated = rand(1000) + alleles[0][17] + rand(tail_len - 1000 - len(alleles[0][17]) - 470) + alleles[2][2]
    assert len(repeated) == tail_len and len(fragment) >= SMALL_RULE[0]
    records = [one_each, straddle]                     # long records first, adjacent
    records += [window() for _ in range(40)]
    records += [b"", b"ACGTA", b"A" * (K - 1), rand(K - 1)]
    records += [twin] + [window() for _ in range(3)] + [fragment, random_contig]
    records += [rand(150) for _ in range(10)] + [repeated] + [window() for _ in range(5)]
    records += [rand(1999), rand(2000) + alleles[1][30]]  # either side of long_len; a long record last
    want = {step: _expected(oracle_mod, obs, widths, records, SMALL_RULE, step) for step in (1, 3)}
    return {"obs": obs, "alleles": alleles, "widths": widths, "records": records, "want": want}


@pytest.fixture(scope="module")
def scheme(oracle_mod):
    return _scheme_data(oracle_mod)


def _banks(xs, scheme, upload=True):
    out = []
    for (ob, sig), al, D in zip(scheme["obs"], scheme["alleles"], LOCUS_DOCS):
        gb = xs.Bank.create_cobs(K, 1, sig, D, [f"Allele_ID_{i + 1}" for i in range(D)], page_size=PAGE, compact=True)
        if upload:
            gb.upload(ob.rows)
        else:
            gb.build(al, np.arange(D, dtype=np.uint32))
        out.append(gb)
    return out


@pytest.fixture(scope="module")
def banks(xs, scheme):
    b = _banks(xs, scheme)
    yield b
    for gb in b:
        gb.close()


def test_inputs_exercise_the_rule(scheme):
    """On the oracle's expected values only, not on the output under test: among the long records
    there is a unique call, a call shared by several alleles with a non-zero score, a locus with no
    call, a chunk count in 1 .. threshold that the rule drops, and at every locus a top other than doc 0."""
    records = scheme["records"]
    long_ = np.array([len(r) >= SMALL_RULE[0] for r in records])
    assert long_.sum() == 7 and long_[0] and long_[1] and long_[-1] and not long_[-2]
    for step in (1, 3):
        top, score, tied, nk, dropped = scheme["want"][step]
        assert (nk == 0).sum() == 4 and nk.max() == (max(map(len, records)) - K) // step + 1
        assert ((tied[long_] == 1) & (score[long_] > THRESHOLD)).any()
        assert ((tied[long_] > 1) & (score[long_] > 0)).any()
        assert ((top[long_] == NONE) & (score[long_] == 0) & (tied[long_] == 0)).any()
        assert dropped > 0
        for l in range(3):
            assert ((top[long_, l] != 0) & (top[long_, l] != NONE)).any(), l
        assert (top[~long_] != NONE).all()  # short records never give NONE


def _check(got, want):
    for g, w, name in zip(got, want[:4], ("top", "score", "tied", "num_kmers")):
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:8].tolist())


@gpu
@pytest.mark.parametrize("step", [1, 3])
def test_type_contigs_matches_oracle(xs, scheme, banks, step):
    got = xs.mlst_type_contigs(banks, scheme["records"], scheme["widths"], step=step, rule=SMALL_RULE)
    _check(got, scheme["want"][step])


@gpu
def test_type_contigs_many_short_runs(xs, scheme, banks, oracle_mod):
    """Short and long records alternating, more runs of short records than are probed where they
    lie: the short ones are compacted first and their outputs scattered back."""
    rec = scheme["records"]
    long_ = [r for r in rec if len(r) >= SMALL_RULE[0]][:2]
    short = [r for r in rec if len(r) < SMALL_RULE[0]]
    records = []
    for i, r in enumerate(short + short[:20]):
        records += [r, long_[i % 2]]
    assert len(records) // 2 > 64
    want = _expected(oracle_mod, scheme["obs"], scheme["widths"], records, SMALL_RULE, 1)
    _check(xs.mlst_type_contigs(banks, records, scheme["widths"], rule=SMALL_RULE), want)


# ---------------------------------------------------------------- 4. the reference's constants
@gpu
def test_reference_constants(xs, scheme, banks, oracle_mod):
    """rule=None: a record of 999,999 bp is cut at the locus width, one of 1,000,000 bp at ten
    times that; a 9,999 bp record is probed whole and a 10,000 bp one chunked."""
    rng = np.random.default_rng(99)
    al = scheme["alleles"]

    def contig(n):
        a = ACGT[rng.integers(0, 4, n)].copy()
        for li in range(3):
            for d, pos in ((3 + li, n // 5 + 700 * li), (9 + li, n - 3_000 - 700 * li)):
                a[pos:pos + len(al[li][d])] = np.frombuffer(al[li][d], dtype=np.uint8)
        return a.tobytes()

    records = [contig(999_999), contig(1_000_000), contig(9_999), contig(10_000)]
    want = _expected(oracle_mod, scheme["obs"], scheme["widths"], records, (10_000, 1_000_000, 10_000_000, 50), 1)
    assert (want[0][[0, 1, 3]] != NONE).any()
    _check(xs.mlst_type_contigs(banks, records, scheme["widths"]), want)


# ---------------------------------------------------------------- 5. ranges
def _big_contigs(scheme, rng, n_contigs=4, size=500_000):
    al = scheme["alleles"]
    out = []
    for _ in range(n_contigs):
        a = ACGT[rng.integers(0, 4, size)].copy()
        for i, pos in enumerate(range(10_000, size - 1_000, 60_000)):
            li = i % 3
            t = al[li][int(rng.integers(0, len(al[li])))]
            a[pos:pos + len(t)] = np.frombuffer(t, dtype=np.uint8)
        out.append(a.tobytes())
    return out


@gpu
def test_ranges_equal_the_unbounded_call(xs, scheme, banks):
    """workspace_bytes of 100 rows of the widest locus (a 500 kbp contig is more than 1,000 chunks:
    cut across ranges) and of 1 (one chunk per range) give what the unbounded call gives."""
    rng = np.random.default_rng(123)
    mixed = scheme["records"]
    records = mixed[:30] + _big_contigs(scheme, rng, 1) + mixed[30:]
    whole = xs.mlst_type_contigs(banks, records, scheme["widths"])  # the reference's constants: W = the locus width
    assert (whole[0][30] != NONE).all() and whole[1][30].min() > 400
    ranged = xs.mlst_type_contigs(banks, records, scheme["widths"], workspace_bytes=100 * 130 * 4)
    for a, b in zip(whole, ranged):
        assert np.array_equal(a, b)
    small = xs.mlst_type_contigs(banks, mixed, scheme["widths"], rule=SMALL_RULE)
    _check(small, scheme["want"][1])
    for ws in (100 * 130 * 4, 1):  # the mixed batch's contigs are 6 - 9 chunks each: cut by ranges of 1
        for a, b in zip(small, xs.mlst_type_contigs(banks, mixed, scheme["widths"], workspace_bytes=ws, rule=SMALL_RULE)):
            assert np.array_equal(a, b), ws


@gpu
def test_type_contigs_workspace_is_bounded(xs, scheme, torch_dev):
    """Four 500 kbp contigs already in HBM, in ranges of 100 chunks, on fresh handles built on the
    device: all the device workspace the loci ever held (their builds, the outputs, a range's
    texts, rows and accumulators) stays below one locus' whole chunk matrix for that input."""
    torch, dev = torch_dev
    from xspect2_amd.packing import pack_sequences
    records = _big_contigs(scheme, np.random.default_rng(321))
    pr = pack_sequences(records)
    d_seqs = torch.from_numpy(pr.buf.copy()).to(dev)
    d_offs = torch.from_numpy(pr.offsets.astype(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    dr = xs.DeviceReads(d_seqs, pr.nbytes, d_offs, pr.n, host_offsets=pr.offsets)
    fresh = _banks(xs, scheme, upload=False)
    try:
        got = xs.mlst_type_contigs(fresh, dr, scheme["widths"], workspace_bytes=100 * 130 * 4)
        peaks = [gb.workspace_bytes()[1] for gb in fresh]
        chunks = xs.mlst_split_size([len(r) for r in records], scheme["widths"][2], K)[0]
        bound = chunks * 130 * 4
        print("workspace peaks", peaks, "bound", bound, "chunks", chunks)
        assert 0 < sum(peaks) < bound, peaks
        assert (got[0] != NONE).all() and (got[3] == 500_000 - K + 1).all()
    finally:
        for gb in fresh:
            gb.close()


# ---------------------------------------------------------------- 6. device reads
@gpu
def test_type_contigs_device_reads(xs, scheme, banks, torch_dev):
    """Reads already in HBM, with and without their offsets on the host, give what host reads give."""
    torch, dev = torch_dev
    from xspect2_amd.packing import pack_sequences
    pr = pack_sequences(scheme["records"])
    d_seqs = torch.from_numpy(pr.buf.copy()).to(dev)
    d_offs = torch.from_numpy(pr.offsets.astype(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    host = xs.mlst_type_contigs(banks, pr, scheme["widths"], step=3, rule=SMALL_RULE)
    _check(host, scheme["want"][3])
    for ho in (None, pr.offsets):
        dr = xs.DeviceReads(d_seqs, pr.nbytes, d_offs, pr.n, host_offsets=ho)
        for ws in (0, 100 * 130 * 4):
            got = xs.mlst_type_contigs(banks, dr, scheme["widths"], step=3, workspace_bytes=ws, rule=SMALL_RULE)
            for a, b in zip(host, got):
                assert np.array_equal(a, b), (ho is None, ws)


# ---------------------------------------------------------------- 7. the model
def _scheme_dir(tmp_path, rng, loci=3, alleles=40):
    root = tmp_path / "alleles"
    for li in range(loci):
        base = "".join(rng.choice(list("ACGT"), 450 + 10 * li))
        for a in range(1, alleles + 1):
            s = list(base)
            for p in rng.choice(len(s), size=int(rng.integers(0, 12)), replace=False):
                s[p] = "ACGT"[(("ACGT".index(s[p])) + 1) % 4]
            write_fasta([Record(f"L{li}_{a}", "".join(s))], root / f"Oxf_L{li}" / f"Allele_ID_{a}.fasta")
    return root


@gpu
def test_predict_columnar_types_contigs_on_the_device(tmp_path, monkeypatch):
    """Windows, whole alleles, contigs (one of the repeated-tail length, one whose alleles straddle
    chunk boundaries) and a random contig in one FASTA: ``predict_columnar(path)`` gives ``predict``'s
    "Strain type" per record, the in-memory records the same columns, and no batch of the device
    reader is copied back to the host."""
    from xspect2_amd import file_io
    from xspect2_amd.probabilistic_filter_mlst_model import ProbabilisticFilterMlstSchemeModel

    rng = np.random.default_rng(6)
    root = _scheme_dir(tmp_path, rng)
    url = "https://example/schemes/1"
    m = ProbabilisticFilterMlstSchemeModel(K, "MLST (Oxford)", tmp_path / "xspect_data", url, "abaumannii")
    m.strain_type_resolver = lambda flat, scheme_url: "ST" + "-".join(str(v) for v in flat.values())
    m.fit(root, page_size=2)

    def allele(li, a):
        return next(get_record_iterator(root / f"Oxf_L{li}" / f"Allele_ID_{a}.fasta")).seq

    def rand(n):
        return "".join(rng.choice(list("ACGT"), n))

    records = []
    for i in range(12):
        a = allele(i % 3, int(rng.integers(1, 41)))
        st = int(rng.integers(0, len(a) - 150 + 1))
        records.append(Record(f"w{i}", a[st:st + 150]))
    records += [Record(f"a{li}_{a}", allele(li, a)) for li in range(3) for a in (4, 17)]
    records.insert(5, Record("contig", "".join(allele(li, 7) + "A" * 3000 for li in range(3)) + rand(2000)))
    w0 = m.avg_locus_bp_size[0]
    tail_len = 23 * (w0 - K + 1) + w0  # locus 0: the tail of k-1 bytes joins the last chunk
    body = rand(300) + allele(0, 12) + rand(900) + allele(1, 33) + rand(1234) + allele(2, 25)
    records.append(Record("repeated_tail", body + rand(tail_len - len(body))))
    records.append(Record("random_contig", rand(12_000)))
    assert all(len(r.seq) >= 10_000 for r in records[-2:]) and len(records[5].seq) >= 10_000
    fa = tmp_path / "input.fasta"
    write_fasta(records, fa)

    want = m.predict(fa).hits
    assert file_io.file_reader_device(m.indices[0]) is not None  # the path is read by the device reader
    copied = []
    to_host = file_io.DeviceSeqBatch.to_host
    monkeypatch.setattr(file_io.DeviceSeqBatch, "to_host", lambda self: copied.append(1) or to_host(self))
    got = m.predict_columnar(fa)
    assert not copied
    resolver = m.strain_type_resolver
    assert list(got.ids) == [r.id for r in records]
    for i, rec in enumerate(records):
        assert got.strain_type(i, resolver, url) == want[rec.id][0]["Strain type"], rec.id
    i_rand = len(records) - 1
    assert (got.top_allele[i_rand] == NONE).all() and (got.n_tied[i_rand] == 0).all()
    assert (got.top_allele[:i_rand] != NONE).all()
    mem = m.predict_columnar(iter(records))
    assert np.array_equal(mem.top_allele, got.top_allele) and np.array_equal(mem.top_score, got.top_score)
    assert np.array_equal(mem.n_tied, got.n_tied) and np.array_equal(mem.sufficient, got.sufficient)
    m.close()
