"""The N best alleles per record and locus on the device: the row reduction
(xs_mlst_ranks_device) and the chunk reduction (xs_mlst_chunk_ranks_device) alone, the whole
call (xs_mlst_type_ranked / _device) against the CPU oracle's hit rows, and
``predict_columnar(limit=True)`` of the MLST model against ``predict(limit=True)``.

Expected values come from numpy restatements of the rule of include/xspect_hip.h
(``_row_ranks``, ``_chunk_ranks``) over rows made here or by the oracle.  Every value is an
integer and compared exactly."""
from __future__ import annotations

import json

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
RANKS = (1, 2, 5, 8)


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
def _row_ranks(rows: np.ndarray, N: int):
    """(allele, score) [n, N] of rows [n, D] probed whole: the stable argsort of -count, padded."""
    rows = np.asarray(rows, dtype=np.uint32)
    n, D = rows.shape
    order = np.argsort(-rows.astype(np.int64), axis=1, kind="stable")[:, :N]
    allele = np.full((n, N), NONE, dtype=np.uint32)
    score = np.zeros((n, N), dtype=np.uint32)
    allele[:, :order.shape[1]] = order
    score[:, :order.shape[1]] = np.take_along_axis(rows, order, axis=1)
    return allele, score


def _row_top(rows: np.ndarray):
    m = rows.max(axis=1)
    return rows.argmax(axis=1).astype(np.uint32), m.astype(np.uint32), (rows == m[:, None]).sum(axis=1).astype(np.uint32)


def _chunk_ranks(rows: np.ndarray, threshold: int, N: int):
    """(allele, score) [N] of one record's chunk rows [chunks, D]: the alleles with a sum > 0 of
    the counts > threshold, by sum descending, the lower first such chunk, the higher count
    there, the lower doc."""
    allele = np.full(N, NONE, dtype=np.uint32)
    score = np.zeros(N, dtype=np.uint32)
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, rows.shape[-1])
    if rows.shape[0] == 0:
        return allele, score
    keep = rows > threshold
    total = (rows * keep).sum(axis=0)
    first = keep.argmax(axis=0)
    fscore = rows[first, np.arange(rows.shape[1])]
    cand = sorted(np.flatnonzero(total > 0), key=lambda d: (-int(total[d]), int(first[d]), -int(fscore[d]), int(d)))[:N]
    allele[:len(cand)] = cand
    score[:len(cand)] = total[cand]
    return allele, score


def _to_dev(torch_dev, a: np.ndarray):
    torch, dev = torch_dev
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 8:
        return torch.from_numpy(a.view(np.int64).reshape(-1)).to(dev)
    if a.dtype.itemsize == 1:
        return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
    return torch.from_numpy(a.view(np.int32).reshape(-1)).to(dev)


def _matrix_at(torch_dev, rows: np.ndarray, off: int):
    """The matrix on the device, `off` counts past a 16-byte boundary inside a tensor of 0xFFFFFFFF:
    a read outside it would win a rank."""
    flat = np.full(off + rows.size + 8, 0xFFFFFFFF, dtype=np.uint32)
    flat[off:off + rows.size] = rows.reshape(-1)
    big = _to_dev(torch_dev, flat)
    assert big.data_ptr() % 16 == 0
    return big, big[off:off + rows.size]


def _sentinels(torch_dev, size):
    torch, dev = torch_dev
    return torch.full((max(size, 1),), SENTINEL, dtype=torch.int32, device=dev)


def _strided(t, n, stride, width):
    """[n, width] of a flat output written at `stride`; the slots between must still hold the sentinel."""
    a = t.cpu().numpy().view(np.uint32)[:n * stride].reshape(n, stride)
    assert (a[:, width:] == SENTINEL).all()
    return a[:, :width]


def _run_rows(xs, torch_dev, rows, N, off=0, want_top=(True, True, True), pad=3):
    """xs_mlst_ranks_device over sentinel-prefilled outputs at strides wider than needed."""
    torch, dev = torch_dev
    n, D = rows.shape
    keep, d_hits = _matrix_at(torch_dev, rows, off)
    rs_stride, top_stride = N + pad, 1 + (pad > 0)
    ra, rs = _sentinels(torch_dev, n * rs_stride), _sentinels(torch_dev, n * rs_stride)
    tops = [_sentinels(torch_dev, n * top_stride) for _ in range(3)]
    args = [t if w else None for t, w in zip(tops, want_top)]
    xs.mlst_ranks_device(d_hits, n, D, N, ra, rs, rs_stride, args[0], args[1], args[2], top_stride,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    out_top = []
    for t, w in zip(tops, want_top):
        if w:
            out_top.append(_strided(t, n, top_stride, 1)[:, 0])
        else:
            assert (t.cpu().numpy().view(np.uint32) == SENTINEL).all()
            out_top.append(None)
    return _strided(ra, n, rs_stride, N), _strided(rs, n, rs_stride, N), out_top


def _top_device(xs, torch_dev, rows):
    torch, dev = torch_dev
    n, D = rows.shape
    outs = [_sentinels(torch_dev, n) for _ in range(3)]
    xs.mlst_top_device(_to_dev(torch_dev, rows), n, D, *outs, 1, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return [o.cpu().numpy().view(np.uint32)[:n] for o in outs]


def _mixed_rows(rng, n, D):
    """Every second row over the whole uint32 range, the others over 0 .. 3 (ties beyond any N)."""
    rows = rng.integers(0, 1 << 32, (n, D), dtype=np.uint64).astype(np.uint32)
    rows[1::2] = rng.integers(0, 4, (len(rows[1::2]), D), dtype=np.uint64).astype(np.uint32)
    return rows


# ---------------------------------------------------------------- 1. the row kernel against numpy
@gpu
@pytest.mark.parametrize("D", [1, 2, 7, 63, 64, 65, 127, 258, 1430])
def test_row_ranks_match_numpy(xs, torch_dev, D):
    rng = np.random.default_rng(1000 + D)
    for n in (1, 5, 257):
        rows = _mixed_rows(rng, n, D)
        if n == 5:
            rows[2] = rng.integers(0, 4, D)  # an even row of ties as well
        top_dev = _top_device(xs, torch_dev, rows)
        for c, w in enumerate(_row_top(rows)):
            assert np.array_equal(top_dev[c], w), (D, n, c)
        for N in RANKS:
            want_a, want_s = _row_ranks(rows, N)
            for want_top in ((True, True, True), (False, True, True), (True, False, True), (True, True, False),
                             (False, False, False)):
                if n == 257 and want_top not in ((True, True, True), (False, False, False)):
                    continue
                ra, rs, tops = _run_rows(xs, torch_dev, rows, N, want_top=want_top)
                assert np.array_equal(ra, want_a), (D, n, N, np.argwhere(ra != want_a)[:4].tolist())
                assert np.array_equal(rs, want_s), (D, n, N, np.argwhere(rs != want_s)[:4].tolist())
                for c in range(3):
                    if want_top[c]:
                        assert np.array_equal(tops[c], top_dev[c]), (D, n, N, c)
            ra, rs, _ = _run_rows(xs, torch_dev, rows, N, pad=0)  # packed: rank_stride == n_ranks
            assert np.array_equal(ra, want_a) and np.array_equal(rs, want_s), (D, n, N)


@gpu
def test_row_ranks_more_rows_than_waves(xs, torch_dev):
    """70,000 rows of 3 counts: the grid stops at 65,536 waves, so a wave takes more than one row."""
    rows = _mixed_rows(np.random.default_rng(3), 70_000, 3)
    want_a, want_s = _row_ranks(rows, 5)
    assert (want_a[:, 3:] == NONE).all() and (want_a[:, :3] != NONE).all()
    ra, rs, tops = _run_rows(xs, torch_dev, rows, 5)
    assert np.array_equal(ra, want_a) and np.array_equal(rs, want_s)
    for got, want in zip(tops, _row_top(rows)):
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- 2. crafted rows
def _crafted_rows():
    """(name, row, off): one row each.  With D 1430 at off 0 the row has no head and a tail of 2
    (docs 1428, 1429) and lane 5 takes docs 20..23, 276..279, ...; at off 1 a head of 3 (docs
    0..2) and a tail of 3 (docs 1427..1429)."""
    D = 1430
    out = [("all zero", np.zeros(D, dtype=np.uint32), 0),
           ("ascending: every element inserts", np.arange(1, D + 1, dtype=np.uint32) * 3, 0),
           ("descending: none inserts behind a lane's first", np.arange(D, 0, -1, dtype=np.uint32) * 3, 0),
           ("ascending, head and tail", np.arange(1, D + 1, dtype=np.uint32), 1),
           ("descending, head and tail", np.arange(D, 0, -1, dtype=np.uint32), 3)]
    one_lane = np.full(D, 7, dtype=np.uint32)
    lane5 = [4 * (5 + 64 * t) + c for t in range(5) for c in range(4)]  # 20 docs of lane 5
    one_lane[lane5[:11]] = 1000  # more equal maxima than any N, all in one lane
    out.append(("equal maxima in one lane", one_lane, 0))
    head = np.full(D, 5, dtype=np.uint32)
    head[:3] = [900, 1000, 950]  # the three best in the head peel (N <= 3: all of them)
    head[700], head[1000] = 800, 800
    out.append(("the best in the head", head, 1))
    tail = np.full(D, 5, dtype=np.uint32)
    tail[1427:] = [950, 1000, 1000]  # the three best in the tail peel
    tail[3], tail[4] = 800, 801
    out.append(("the best in the tail", tail, 1))
    tail2 = np.zeros(D, dtype=np.uint32)
    tail2[1428:] = [9, 9]
    out.append(("the best in a tail of two", tail2, 0))
    big = np.full(D, 3, dtype=np.uint32)
    big[[10, 500, 501, 1429, 77, 0]] = [0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0x80000001, 0xFFFFFFFE]
    out.append(("counts from 2^31 beside small ones", big, 2))
    for D_small in (1, 2, 3, 4, 7):  # D < N
        out.append((f"D {D_small} below N", np.arange(D_small, dtype=np.uint32)[::-1].copy() * 0x20000000, D_small % 4))
    return out


@gpu
@pytest.mark.parametrize("N", [1, 2, 3, 5, 8])
def test_row_ranks_crafted(xs, torch_dev, N):
    for name, row, off in _crafted_rows():
        rows = row.reshape(1, -1)
        want_a, want_s = _row_ranks(rows, N)
        ra, rs, tops = _run_rows(xs, torch_dev, rows, N, off=off)
        assert np.array_equal(ra, want_a) and np.array_equal(rs, want_s), (name, N, ra.tolist(), want_a.tolist())
        for got, want in zip(tops, _row_top(rows)):
            assert np.array_equal(got, want), (name, N)
    # the restatement itself, on rows written out above
    rows = {name: row for name, row, _ in _crafted_rows()}
    assert _row_ranks(rows["all zero"].reshape(1, -1), 3)[0].tolist() == [[0, 1, 2]]
    assert _row_ranks(rows["equal maxima in one lane"].reshape(1, -1), 3)[0].tolist() == [[20, 21, 22]]
    assert _row_ranks(rows["the best in the tail"].reshape(1, -1), 3)[0].tolist() == [[1428, 1429, 1427]]
    a, s = _row_ranks(rows["counts from 2^31 beside small ones"].reshape(1, -1), 8)
    assert a.tolist() == [[500, 1429, 0, 77, 10, 501, 1, 2]] and s[0, :2].tolist() == [0xFFFFFFFF] * 2
    assert _row_ranks(rows["D 2 below N"].reshape(1, -1), 3)[0].tolist() == [[0, 1, NONE]]


# ---------------------------------------------------------------- 3. unaligned base
@gpu
@pytest.mark.parametrize("off", [1, 2, 3])
def test_row_ranks_unaligned_base(xs, torch_dev, off):
    """The matrix starts 1, 2 or 3 counts past a 16-byte boundary, 0xFFFFFFFF all around it."""
    rng = np.random.default_rng(50 + off)
    for n, D in ((1, 1), (1, 2), (5, 7), (3, 65), (4, 258), (2, 1430)):
        rows = rng.integers(0, 1000, (n, D), dtype=np.uint64).astype(np.uint32)
        for N in (5, 8):
            want_a, want_s = _row_ranks(rows, N)
            ra, rs, tops = _run_rows(xs, torch_dev, rows, N, off=off)
            assert np.array_equal(ra, want_a) and np.array_equal(rs, want_s), (off, n, D, N)
            for got, want in zip(tops, _row_top(rows)):
                assert np.array_equal(got, want), (off, n, D, N)


# ---------------------------------------------------------------- 4. the owner kernel
def _crafted_owners(D: int, rng):
    docs = sorted({0, D // 2, D - 1})
    A, B, C = (docs + [docs[-1]] * 2)[:3]
    owners = []

    def owner(n_chunks, cells):
        r = np.zeros((n_chunks, D), dtype=np.uint32)
        for c, d, v in cells:
            r[c, d] = v
        owners.append(r)

    owner(3, [(0, A, 100), (1, A, 90), (2, B, 150)])                       # 0 by sum: A (190), B (150)
    owner(2, [(1, A, 60), (0, B, 60)])                                     # 1 equal sums: the first chunk (B, A)
    owner(2, [(0, A, 60), (0, B, 70), (1, A, 70), (1, B, 60)])             # 2 same first chunk: higher count there (B, A)
    owner(1, [(0, C, 80), (0, B, 80), (0, A, 80)])                         # 3 equal on all three: by doc
    owner(1, [(0, A, THRESHOLD), (0, B, THRESHOLD + 1)])                   # 4 exactly the threshold is dropped
    owner(2, [(0, A, THRESHOLD), (1, B, 1), (1, C, THRESHOLD)])            # 5 nothing passes
    owner(0, [])                                                           # 6 no rows
    owner(1, [(0, C, 77)])                                                 # 7 one allele: fewer than N
    owner(2, [(0, A, 0x7FFFFFFF), (1, B, 0x90000000)])                     # 8 unsigned compares
    owner(3, [(0, A, 51), (1, A, 51), (2, B, 102)])                        # 9 equal sums over different first chunks
    owners.append(rng.integers(0, 121, (40, D), dtype=np.uint64).astype(np.uint32))  # many chunks, many passing
    for _ in range(300):  # more owners than one block's waves; counts around the threshold tie often
        owners.append(rng.integers(THRESHOLD - 4, THRESHOLD + 4, (int(rng.integers(0, 4)), D),
                                   dtype=np.uint64).astype(np.uint32))
    owners.append(np.zeros((0, D), dtype=np.uint32))  # the last owner has no rows either
    begin = np.concatenate([[0], np.cumsum([o.shape[0] for o in owners])]).astype(np.uint64)
    return owners, np.concatenate(owners, axis=0), begin, (A, B, C)


@gpu
@pytest.mark.parametrize("D", [1, 65, 258])
def test_chunk_ranks_crafted_owners(xs, torch_dev, D):
    torch, dev = torch_dev
    owners, rows, begin, (A, B, C) = _crafted_owners(D, np.random.default_rng(70 + D))
    n_own, nc = len(owners), rows.shape[0]
    d_begin = _to_dev(torch_dev, begin)
    s = torch.cuda.current_stream(dev).cuda_stream
    for N in RANKS:
        want = [_chunk_ranks(o, THRESHOLD, N) for o in owners]
        want_a, want_s = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        if D == 258 and N == 2:  # the restatement itself, on the cases written out above
            assert want_a[:10].tolist() == [[A, B], [B, A], [B, A], [A, B], [B, NONE], [NONE, NONE], [NONE, NONE],
                                            [C, NONE], [B, A], [A, B]]
            assert want_s[:5].tolist() == [[190, 150], [60, 60], [130, 130], [80, 80], [51, 0]]
        for off in (0, 1):
            keep, d_hits = _matrix_at(torch_dev, rows, off)
            for stride in (N, N + 2):
                ra, rs = _sentinels(torch_dev, n_own * stride), _sentinels(torch_dev, n_own * stride)
                xs.mlst_chunk_ranks_device(d_hits, nc, D, d_begin, n_own, THRESHOLD, N, ra, rs, stride, stream=s)
                torch.cuda.synchronize(dev)
                got_a, got_s = _strided(ra, n_own, stride, N), _strided(rs, n_own, stride, N)
                assert np.array_equal(got_a, want_a), (D, N, off, stride, np.argwhere(got_a != want_a)[:4].tolist())
                assert np.array_equal(got_s, want_s), (D, N, off, stride)
    # rank 0 is xs_mlst_chunk_top_device's call
    top, score = _sentinels(torch_dev, n_own), _sentinels(torch_dev, n_own)
    xs.mlst_chunk_top_device(_to_dev(torch_dev, rows), nc, D, d_begin, n_own, THRESHOLD, top, score, None, 1, stream=s)
    torch.cuda.synchronize(dev)
    assert np.array_equal(top.cpu().numpy().view(np.uint32)[:n_own], want_a[:, 0])
    assert np.array_equal(score.cpu().numpy().view(np.uint32)[:n_own], want_s[:, 0])


# ---------------------------------------------------------------- 5. the whole call against the oracle
def _alleles(rng, D, length):
    base = rng.integers(0, 4, length)
    out = []
    for _ in range(D):
        a = base.copy()
        pos = rng.choice(length, size=int(rng.integers(0, 12)), replace=False)
        a[pos] = (a[pos] + 1) % 4
        out.append(ACGT[a].tobytes())
    out[11] = out[4]  # an allele identical to another of its locus
    out[20] = ACGT[rng.integers(0, 4, length)].tobytes()  # and one unlike all others: alone above the threshold
    return out


def _expected(oracle_mod, obs, widths, records, rule, step, N):
    """(rank_allele, rank_score) [n, loci, N] from the oracle's hit rows."""
    long_len, s10, s100, thr = rule
    n, L = len(records), len(obs)
    ra = np.zeros((n, L, N), dtype=np.uint32)
    rs = np.zeros((n, L, N), dtype=np.uint32)
    short = [i for i, r in enumerate(records) if len(r) < long_len]
    for l, ob in enumerate(obs):
        if short:
            ra[short, l], rs[short, l] = _row_ranks(ob.query([records[i] for i in short], step=step)[0], N)
        for i, r in enumerate(records):
            if len(r) >= long_len:
                w = widths[l] * (1 if len(r) < s10 else 10 if len(r) < s100 else 100)
                ra[i, l], rs[i, l] = _chunk_ranks(ob.query(oracle_mod.sequence_splitter(r, w, K), step=step)[0], thr, N)
    return ra, rs


@pytest.fixture(scope="module")
def scheme(oracle_mod):
    rng = np.random.default_rng(20261022)
    obs, sigs, alleles = [], [], []
    for li, D in enumerate(LOCUS_DOCS):
        al = _alleles(rng, D, 450 + 10 * li)
        sig = [oracle_mod.signature_size(len(al[0]) - K + 1, 1, 0.001)] * ((D + 8 * PAGE - 1) // (8 * PAGE))
        ob = oracle_mod.CobsBank.empty(sig, PAGE, D, 1, K)
        ob.build(al, list(range(D)))
        obs.append(ob)
        sigs.append(sig)
        alleles.append(al)

    def rand(n):
        return ACGT[rng.integers(0, 4, n)].tobytes()

    def window():
        al = alleles[int(rng.integers(0, 3))]
        a = al[int(rng.integers(0, len(al)))]
        st = int(rng.integers(0, len(a) - 150 + 1))
        return a[st:st + 150]

    one_each = rand(700) + alleles[0][3] + rand(600) + alleles[1][5] + rand(500) + alleles[2][7] + rand(400)
    two_each = rand(300) + alleles[0][9] + rand(900) + alleles[0][22] + rand(700) + alleles[2][21] + alleles[2][90] + rand(300)
    twin = rand(900) + alleles[0][4] + rand(50) + alleles[1][11] + rand(800)  # alleles 4 and 11 are the same text
    fragment = rand(1200) + alleles[1][8][100:160] + rand(1300)                 # 40 k-mers: under the threshold
    lonely = rand(800) + alleles[1][20] + rand(900)                             # one allele passes: fewer than N
    records = [one_each, two_each] + [window() for _ in range(20)] + [b"", b"ACGTA", rand(K - 1)]
    records += [twin] + [window() for _ in range(3)] + [fragment, lonely, rand(3000)] + [rand(150) for _ in range(4)]
    records += [rand(1999), rand(2000) + alleles[1][30]]  # either side of long_len; a long record last
    return {"obs": obs, "sigs": sigs, "alleles": alleles, "widths": [len(al[0]) for al in alleles], "records": records}


@pytest.fixture(scope="module")
def banks(xs, scheme):
    out = []
    for ob, sig, D in zip(scheme["obs"], scheme["sigs"], LOCUS_DOCS):
        gb = xs.Bank.create_cobs(K, 1, sig, D, [f"Allele_ID_{i + 1}" for i in range(D)], page_size=PAGE, compact=True)
        gb.upload(ob.rows)
        out.append(gb)
    yield out
    for gb in out:
        gb.close()


def _check_ranked(xs, banks, scheme, records, want, N, step=1, reads=None, **kw):
    """The ranked call equals the restatement, its four first outputs xs_mlst_type_contigs' bit for bit."""
    reads = records if reads is None else reads
    plain = xs.mlst_type_contigs(banks, reads, scheme["widths"], step=step, rule=SMALL_RULE, **kw)
    got = xs.mlst_type_ranked(banks, reads, scheme["widths"], N, step=step, rule=SMALL_RULE, **kw)
    for a, b, name in zip(plain, got[:4], ("top", "score", "tied", "num_kmers")):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (name, N, step, kw)
    ra, rs = got[4], got[5]
    assert ra.shape == rs.shape == (len(records), len(banks), N)
    assert np.array_equal(ra[:, :, 0], got[0]) and np.array_equal(rs[:, :, 0], got[1]), (N, step, kw)
    assert np.array_equal(ra, want[0]), (N, step, kw, np.argwhere(ra != want[0])[:6].tolist())
    assert np.array_equal(rs, want[1]), (N, step, kw, np.argwhere(rs != want[1])[:6].tolist())
    return got


@gpu
@pytest.mark.parametrize("step", [1, 3])
def test_type_ranked_matches_oracle(xs, scheme, banks, oracle_mod, step):
    """Whole workspace, then one of 7 rows of the widest locus (the run of 23 short reads goes in
    several pieces, and a contig of 8 chunks is cut by a range end), then of one row."""
    records = scheme["records"]
    long_ = np.array([len(r) >= SMALL_RULE[0] for r in records])
    for N in (5, 8) if step == 1 else (2,):
        want = _expected(oracle_mod, scheme["obs"], scheme["widths"], records, SMALL_RULE, step, N)
        if N == 5:  # the inputs exercise the rule: a long record with several ranks, one with none, one short of N
            filled = (want[0][long_] != NONE).sum(axis=2)
            assert (filled >= 2).any() and (filled == 0).any() and ((filled > 0) & (filled < N)).any()
            assert (want[0][~long_] != NONE).all()
        for ws in (0, 7 * 130 * 4, 1):
            _check_ranked(xs, banks, scheme, records, want, N, step=step, workspace_bytes=ws)


@gpu
def test_type_ranked_many_short_runs(xs, scheme, banks, oracle_mod):
    """Short and long records alternating, more than 64 runs of short records: the short ones are
    compacted first and their ranks scattered back at loci x N columns."""
    rec = scheme["records"]
    long_ = [r for r in rec if len(r) >= SMALL_RULE[0]][:2]
    short = [r for r in rec if len(r) < SMALL_RULE[0]]
    records = []
    for i, r in enumerate((short * 3)[:70]):
        records += [r, long_[i % 2]]
    assert len(records) // 2 > 64
    for N in (1, 5):
        want = _expected(oracle_mod, scheme["obs"], scheme["widths"], records, SMALL_RULE, 1, N)
        for ws in (0, 7 * 130 * 4):
            _check_ranked(xs, banks, scheme, records, want, N, workspace_bytes=ws)


@gpu
def test_type_ranked_device_reads(xs, scheme, banks, oracle_mod, torch_dev):
    """Reads already in HBM, with and without their offsets on the host, give what host reads give."""
    torch, dev = torch_dev
    from xspect2_amd.packing import pack_sequences
    records = scheme["records"]
    pr = pack_sequences(records)
    d_seqs = torch.from_numpy(pr.buf.copy()).to(dev)
    d_offs = torch.from_numpy(pr.offsets.astype(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    want = _expected(oracle_mod, scheme["obs"], scheme["widths"], records, SMALL_RULE, 3, 5)
    host = _check_ranked(xs, banks, scheme, records, want, 5, step=3, reads=pr)
    for ho in (None, pr.offsets):
        dr = xs.DeviceReads(d_seqs, pr.nbytes, d_offs, pr.n, host_offsets=ho)
        for ws in (0, 7 * 130 * 4):
            got = _check_ranked(xs, banks, scheme, records, want, 5, step=3, reads=dr, workspace_bytes=ws)
            for a, b in zip(host, got):
                assert np.array_equal(a, b), (ho is None, ws)


# ---------------------------------------------------------------- 6. the model
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
def test_predict_columnar_limit_gives_predicts_all_results(tmp_path):
    """Read-length windows, whole alleles, a contig of more than 10 kbp with two alleles per locus
    and a random contig (no call) in one FASTA: for every record with a call at every locus,
    ``predict_columnar(path, limit=True).to_mlst_result()`` holds ``predict(path, limit=True)``'s
    "Strain type" and "All results", in the same order."""
    from xspect2_amd.probabilistic_filter_mlst_model import ProbabilisticFilterMlstSchemeModel

    rng = np.random.default_rng(16)
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
    contig = "".join(rand(1500) + allele(li, 7) + rand(1200) + allele(li, 31) for li in range(3)) + rand(2500)
    records.insert(5, Record("contig", contig))
    records.append(Record("random_contig", rand(12_000)))
    assert len(contig) >= 10_000
    fa = tmp_path / "input.fasta"
    write_fasta(records, fa)

    want = m.predict(fa, limit=True).hits
    got = m.predict_columnar(fa, limit=True)
    assert got.rank_allele.shape == (len(records), 3, 5)
    res = got.to_mlst_result(m.strain_type_resolver, url)
    assert list(res.hits) == [r.id for r in records] == list(want)
    called = [i for i in range(len(records)) if (got.top_allele[i] != NONE).all()]
    assert len(called) >= 0.8 * len(records) and 5 in called and len(records) - 1 not in called
    for i in called:
        rid = records[i].id
        assert res.hits[rid] == want[rid], rid
        assert json.dumps(res.hits[rid]) == json.dumps(want[rid]), rid  # the dicts' order too
    all_contig = want["contig"][1]["All results"]
    assert all(len(v) >= 2 for v in all_contig.values())  # the contig's runners-up are there to compare
    assert all(len(v) == 5 for v in want["w0"][1]["All results"].values())
    # limit_number below the default, and the unranked call as before
    two = m.predict_columnar(fa, limit=True, limit_number=2)
    assert np.array_equal(two.rank_allele, got.rank_allele[:, :, :2])
    assert np.array_equal(two.rank_score, got.rank_score[:, :, :2])
    plain = m.predict_columnar(fa)
    assert plain.rank_allele is None and plain.rank_score is None
    assert list(plain.to_dict()) == ["Scheme", "Steps", "Input_source", "ids", "loci", "locus_size", "top_allele",
                                     "top_score", "n_tied", "sufficient"]
    for name in ("top_allele", "top_score", "n_tied", "sufficient"):
        assert np.array_equal(getattr(plain, name), getattr(got, name)), name
    m.close()
