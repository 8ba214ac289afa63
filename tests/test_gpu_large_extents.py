"""Banks, filters and batches that cross the 2^32 boundaries (GPU).

Every other test stays below 2^32 in each of: a filter's bit index, a byte
offset into a bank image, an index into the hit matrix, a read's offset in the
sequence buffer.  The kernels carry all four in 64 bits by hand (`(uint64_t)rj *
pitch`, `gd.base + row * pitch`, `bits + (p << (shift - 5))`, `hits[(uint64_t)r
* D + d]`, `seq + seq_bytes`); an edit that narrows one of them to 32 bits
passes every other test and returns wrong counts on the first model a little
larger than the benchmark's.  Each case here is the smallest that crosses one
boundary with enough of its input beyond it:

    B1  rbloom of 805,306,411 bytes: bit indices past 2^32; partitions 256 and up
        of the production plan start past bit 2^32
    B2  rbloom of 2^31 + 65 bytes: the first plan of 2^25-bit partitions
    B3  classic, 100 docs, 2^28 rows: the fast kernel's 32-bit row offset at its
        limit (the last row at byte 2^32 - 16)
    B4  classic, 100 docs, 300,000,007 rows: a 4.8 GB image; build, repack from
        13 to 16 bytes a row, the slots kernels fast declines to, cobspart at
        shift 19
    B5  classic, 1000 docs, config 2's signature size: 4.9 GB at 128 bytes a row
    B6  compact, two groups: the second group's base at byte 4.56e9
    B7  a hit matrix of 4096 x 513 reads x 2048 docs: 4.3e9 cells
    B8  a read buffer of 2^32 + 64 KiB bytes: offsets, the buffer's end and
        sampled positions past 2^32

Every bank is built on the device from documents (Bank.build), downloaded and
compared with the oracle-built image, then probed with true-positive reads
(150 bp windows of the documents) and foreign ones against the oracle.  True
positives make a wrapped offset visible: the images are sparse, and a row or
word read from the wrong place is zero.  Each case first asserts on the CPU,
with the oracle's own hashes, that at least 1000 of the rows (bits) its
true-positive k-mers probe lie past the boundary it names.

Not covered, here or anywhere: a group of 2^30 rows and more (137 GB at 128
bytes a row), more than 2^32 sampled k-mers in one call, a filter over 2^42
bits.
"""
from __future__ import annotations

import numpy as np
import pytest

import partition_layouts as pl
from test_gpu_parity import _explain, _reads

pytestmark = pytest.mark.gpu

TWO32 = 1 << 32
STEPS = (1, 3)
AMBIGUOUS = 0xFFFFFFFF
POISON = 0x5A
GATHER, PARTITIONED = 0, 1


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    assert (_lib.XS_PATH_GATHER, _lib.XS_PATH_PARTITIONED) == (GATHER, PARTITIONED)
    return bank_mod


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "torch sees no GPU"
    return t


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _windows(rng, seqs, order, n, length=150):
    """n error-free windows, window i from document order[i % len(order)]; and those documents."""
    out, docs = [], []
    for i in range(n):
        d = order[i % len(order)]
        st = int(rng.integers(0, len(seqs[d]) - length + 1))
        out.append(seqs[d][st:st + length])
        docs.append(d)
    return out, np.asarray(docs)


def _assert_same_image(got, want, what):
    """Two sparse byte images are equal: the non-zero 64-bit words lie at the
    same places and hold the same values (a scan each, no copy)."""
    assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    n8 = got.size // 8 * 8
    g, w = got[:n8].view(np.uint64), want[:n8].view(np.uint64)
    gi, wi = np.flatnonzero(g), np.flatnonzero(w)
    assert wi.size > 1000, f"{what}: the oracle's image is empty"
    if gi.size != wi.size or not np.array_equal(gi, wi):
        only = np.setxor1d(gi, wi)
        first = int(only[0])
        raise AssertionError(f"{what}: {gi.size} non-zero words on the device, {wi.size} in the oracle's image; "
                             f"the first difference at byte {first * 8} ({'past' if first * 8 >= TWO32 else 'below'} "
                             f"2^32), {int((only * 8 >= TWO32).sum())} of {only.size} differences past 2^32")
    bad = np.flatnonzero(g[gi] != w[wi])
    assert bad.size == 0, f"{what}: {bad.size} words differ, the first at byte {int(gi[bad[0]]) * 8}"
    assert np.array_equal(got[n8:], want[n8:]), f"{what}: the last {got.size - n8} bytes differ"
    return wi


# ---------------------------------------------------------------- rbloom: B1, B2
def _bloom_bits(oracle_mod, bf, reads, k):
    """Bit indices every k-mer of `reads` probes (step 1), by the oracle's own hash and index generator."""
    out = []
    for r in reads:
        for i in range(len(r) - k + 1):
            out += bf.indexes(oracle_mod.xxh3_64(oracle_mod.canonical_bio(r[i:i + k])))
    return np.asarray(out, dtype=np.uint64)


def _check_bloom(gb, reads, bf, mode, kernel, path, what):
    gb.set_probe_options(bloom_part=mode)
    for step in STEPS:
        want_h, want_n = bf.query(reads, step=step)
        got_h, got_n = gb.query(reads, step=step)
        assert (gb.probe_kernel(), gb.probe_path()) == (kernel, path), f"{what}: routed to {gb.probe_kernel()}"
        assert np.array_equal(got_n, want_n), f"{what}, step {step}: num_kmers differ"
        assert got_h.shape == (len(reads), 1)
        assert np.array_equal(got_h[:, 0], want_h), f"{what}, step {step}: " + _explain(got_h, want_h[:, None], reads)
        tot, nk = gb.query_totals(reads, step=step)
        assert (gb.probe_kernel(), gb.probe_path()) == (kernel, path)
        assert int(tot[0]) == int(want_h.sum()) and nk == int(want_n.sum()), f"{what}, step {step}: totals differ"


BLOOM_CASES = [
    # nbytes, production shift, ((bloom_part, kernel, path), ...)
    pytest.param(805_306_411, 24, ((0, "bloom<21,7>", GATHER), (2, "bloompart", PARTITIONED), (3, "bloompart", PARTITIONED)),
                 id="B1-805306411"),
    pytest.param((1 << 31) + 65, 25, ((0, "bloom<21,7>", GATHER), (2, "bloompart", PARTITIONED)), id="B2-2gib+65"),
]


@pytest.mark.parametrize("nbytes,shift,routes", BLOOM_CASES)
def test_rbloom_filter_past_2_32_bits(xs, oracle_mod, nbytes, shift, routes):
    """B1, B2.  40 documents of 2.5 kbp built into the filter on the device: the
    image equals the oracle's; 40 true-positive windows and 60 foreign reads
    equal the oracle on every path.  Of the 36,400 bits the true positives
    probe, a third (B1) and three quarters (B2) lie past 2^32, in partitions
    of the production plan that start past it."""
    k, K = 21, 7
    plan = pl.bloom_plan(nbytes, 2)
    assert plan["shift"] == shift and nbytes * 8 > TWO32
    rng = np.random.default_rng(nbytes)
    docs = [_acgt(rng, 2500) for _ in range(40)]
    bf = oracle_mod.BloomFilter(np.zeros(nbytes, dtype=np.uint8), K, k)
    bf.build(docs)
    tp, _ = _windows(rng, docs, list(range(40)), 40)
    bits = _bloom_bits(oracle_mod, bf, tp, k)
    past = bits[bits >= TWO32]
    assert past.size >= 1000, past.size
    assert np.unique(past >> np.uint64(shift)).size >= 100  # spread over the partitions past bit 2^32
    reads = tp + _reads(rng, 60, k)

    gb = xs.Bank.create_bloom(k, nbytes, K)
    try:
        gb.build(docs)
        words = _assert_same_image(gb.download(), bf.bits, "filter image")
        assert (words >= TWO32 // 64).sum() > words.size // 4  # the built bits past 2^32 are there
        want_h, want_n = bf.query(tp)
        assert np.array_equal(want_h, want_n) and (want_n == 150 - k + 1).all()  # no false negatives
        for mode, kernel, path in routes:
            _check_bloom(gb, reads, bf, mode, kernel, path, f"bloom_part={mode}")
    finally:
        gb.close()


# ---------------------------------------------------------------- COBS images: B3 - B6
def _cobs_offsets(oracle_mod, reads, k, h, sig, pitch):
    """Byte offsets into the device image of every row the k-mers of `reads`
    probe (step 1): each k-mer's h rows in every group, at the device's pitch."""
    bases = np.concatenate([[0], np.cumsum([s * pitch for s in sig])])
    out = []
    for r in reads:
        for i in range(len(r) - k + 1):
            c = oracle_mod.canonical_cobs(r[i:i + k])
            hv = [oracle_mod.xxh64(c, seed=j) for j in range(h)]
            for g, s in enumerate(sig):
                out += [int(bases[g]) + (v % s) * pitch for v in hv]
    return np.asarray(out, dtype=np.uint64)


def _check_cobs(gb, reads, want, mode, kernel, path, what):
    gb.set_probe_options(cobs_part=mode)
    for step in STEPS:
        want_h, want_n = want[step]
        got_h, got_n = gb.query(reads, step=step)
        assert (gb.probe_kernel(), gb.probe_path()) == (kernel, path), f"{what}: routed to {gb.probe_kernel()}"
        assert np.array_equal(got_n, want_n), f"{what}, step {step}: num_kmers differ"
        assert got_h.shape == want_h.shape
        assert np.array_equal(got_h, want_h), f"{what}, step {step}: " + _explain(got_h, want_h, reads)
        tot, nk = gb.query_totals(reads, step=step)
        assert (gb.probe_kernel(), gb.probe_path()) == (kernel, path)
        assert np.array_equal(tot, want_h.sum(axis=0, dtype=np.uint64)), f"{what}, step {step}: totals differ"
        assert nk == int(want_n.sum())


COBS_CASES = [
    # D, k, h, page (None: classic), sig, doc bytes, true positives, boundary (byte offset), image bytes on the
    # device at the least, upload (the oracle's image uploaded into a fresh bank and probed as well),
    # ((cobs_part, kernel, path), ...)
    pytest.param(100, 21, 7, None, [1 << 28], 600, 30, 1 << 31, TWO32, False,
                 ((0, "fast<21,7>", GATHER), (2, "cobspart", PARTITIONED)), id="B3-fast-at-its-limit"),
    pytest.param(100, 21, 7, None, [300_000_007], 600, 30, TWO32, 4_800_000_000, False,
                 ((0, "slots<21,7,1,4>", GATHER), (2, "cobspart", PARTITIONED)), id="B4-slots-21-7"),
    pytest.param(100, 31, 1, None, [300_000_007], 600, 100, TWO32, 4_800_000_000, True,
                 ((0, "slots<31,1,1,4>", GATHER), (2, "cobspart", PARTITIONED)), id="B4-slots-31-1"),
    pytest.param(1000, 21, 7, None, [38_371_819], 200, 30, TWO32, 4_900_000_000, False,
                 ((0, "wide<21,7,C8,G1>", GATHER),), id="B5-wide-pitch-128"),
    pytest.param(200, 25, 3, 16, [285_000_001, 5_000_011], 600, 32, TWO32, 4_600_000_000, False,
                 ((0, "slots<0,0,4,1>", GATHER),), id="B6-compact-group-base"),
]


@pytest.mark.parametrize("D,k,h,page,sig,doc_len,n_tp,boundary,image_bytes,upload,routes", COBS_CASES)
def test_cobs_image_past_2_32_bytes(xs, oracle_mod, D, k, h, page, sig, doc_len, n_tp, boundary, image_bytes, upload,
                                    routes):
    """B3 - B6.  One document per doc built into the bank on the device: the
    downloaded image equals the oracle's; true-positive windows from the
    first, last and group-edge documents and 50 foreign reads equal the oracle
    on every path, and each true positive has its full count on its own doc.
    `boundary` is the byte offset the case is about: 2^32, and for B3 2^31 (the
    upper half of the fast kernel's 32-bit offsets, whose top is the last row).
    One case (B4, one hash) then uploads the oracle's image into a fresh bank,
    13 to 16 bytes a row past 2^32 in the other direction, and probes that."""
    P = page if page is not None else (D + 7) // 8
    G = len(sig)
    rng = np.random.default_rng([D, k, h, sig[0] % 1000])
    seqs = [_acgt(rng, doc_len) for _ in range(D)]
    ob = oracle_mod.CobsBank.empty(sig, P, D, h, k)
    ob.build(seqs, list(range(D)))
    edge = sorted({0, D - 1} | {min(D, g * 8 * P) - 1 for g in range(1, G + 1)} | {g * 8 * P for g in range(G)})
    order = edge + [int(d) for d in rng.permutation(D)]
    tp, tp_docs = _windows(rng, seqs, order, n_tp)
    reads = tp + _reads(rng, 50, k)
    want = {step: ob.query(reads, step=step) for step in STEPS}
    wh, wn = want[1]
    assert (wh[np.arange(n_tp), tp_docs] == wn[:n_tp]).all() and (wn[:n_tp] == 150 - k + 1).all()
    assert int(wh[n_tp:].sum()) < int(wn[n_tp:].sum())  # the foreign reads are not members

    gb = xs.Bank.create_cobs(k, h, sig, D, page_size=page, compact=page is not None)
    try:
        pitch = int(gb.info.device_row_pitch)
        assert sum(sig) * pitch >= image_bytes > TWO32 - 1 and int(gb.info.num_groups) == G
        offs = _cobs_offsets(oracle_mod, tp, k, h, sig, pitch)
        assert int((offs >= boundary).sum()) >= 1000, int((offs >= boundary).sum())
        if G > 1:  # B6: rows of the second group, all past 2^32, and rows of the first on both sides
            base1 = sig[0] * pitch
            assert base1 > TWO32 and (offs >= base1).sum() >= 1000 and ((offs >= TWO32) & (offs < base1)).sum() >= 100
            assert {int(d) >= 8 * P for d in tp_docs} == {False, True}  # true positives from docs of both groups
        gb.build(seqs, list(range(D)))
        words = _assert_same_image(gb.download(), ob.rows, "bank image")
        # built rows past the boundary (row r lies at byte r * P of the file layout, at r * pitch on the device)
        assert int((words.astype(np.uint64) * np.uint64(8) >= (boundary // pitch) * P).sum()) >= 1000
        for mode, kernel, path in routes:
            _check_cobs(gb, reads, want, mode, kernel, path, f"cobs_part={mode}")
        if upload:  # a fresh bank: rows the upload put in the wrong place would otherwise find the built ones
            gb.close()
            gb = xs.Bank.create_cobs(k, h, sig, D, page_size=page, compact=page is not None)
            assert P != pitch
            gb.upload(ob.rows)
            mode, kernel, path = routes[0]
            _check_cobs(gb, reads, want, mode, kernel, path, "uploaded image")
    finally:
        gb.close()


# ---------------------------------------------------------------- B7: the hit matrix
def _best(want_h):
    m = want_h.max(axis=1)
    ties = (want_h == m[:, None]).sum(axis=1)
    return np.where(ties == 1, want_h.argmax(axis=1), AMBIGUOUS).astype(np.uint32), m


class _Poisoned:
    """`count` elements of a torch dtype between two guards of 256 bytes, every byte POISON."""

    def __init__(self, torch, count, dtype):
        self.size = count * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((self.size + 512,), POISON, dtype=torch.uint8, device="cuda")
        self.body = self.raw[256:256 + self.size].view(dtype)

    def guards_intact(self):
        return bool((self.raw[:256] == POISON).all()) and bool((self.raw[256 + self.size:] == POISON).all())


def test_hit_matrix_of_more_than_2_32_cells(xs, oracle_mod, torch):
    """B7.  4096 distinct reads of k - 2 .. k + 40 bytes (empty ones included),
    half of them cut from the documents, repeated 513 times: 2,101,248 reads x
    2048 docs = 4,303,355,904 cells (17.2 GB on the device, poisoned first;
    nothing of it comes to the host).  The 4096 rows of the last repeat start
    at cell 2^32 exactly.  Every repeat equals the oracle's 4096 x 2048 matrix,
    num_kmers and totals are 513 times the oracle's, and xs_best_device over
    the same matrix equals the numpy best of the oracle's rows."""
    D, k, h, sig, U, REP = 2048, 21, 7, [3001], 4096, 513
    n = U * REP
    assert n * D > TWO32 and (n - U) * D == TWO32
    rng = np.random.default_rng(7)
    seqs = [_acgt(rng, 100) for _ in range(D)]
    ob = oracle_mod.CobsBank.empty(sig, D // 8, D, h, k)
    ob.build(seqs, list(range(D)))
    lens = rng.integers(k - 2, k + 41, U)
    lens[rng.integers(0, U, 40)] = 0
    lens[[0, U - 1]] = (k + 40, k)  # the batch's first and last read hold k-mers
    unit = []
    for i, L in enumerate(lens):
        st = int(rng.integers(0, 100 - int(L) + 1))  # even reads: a window of doc i / 2, every doc once
        unit.append(seqs[i // 2][st:st + int(L)] if i % 2 == 0 else _acgt(rng, int(L)))
    assert len(set(r for r in unit if r)) == sum(1 for r in unit if r)  # distinct
    want_h, want_n = ob.query(unit)
    assert int((want_h.max(axis=1) > 0).sum()) >= 1000  # rows past cell 2^32 that hold counts
    assert (want_n == 0).sum() >= 40 and int(want_n.max()) == 41
    want_best, want_max = _best(want_h)
    assert (want_best != AMBIGUOUS).sum() >= 500 and (want_best == AMBIGUOUS).sum() >= 40

    gb = xs.Bank.create_cobs(k, h, sig, D)
    try:
        gb.set_probe_options(cobs_part=0)
        gb.build(seqs, list(range(D)))
        assert np.array_equal(gb.download(), ob.rows)
        text = np.frombuffer(b"".join(unit), dtype=np.uint8)
        uo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        B = int(uo[-1])
        d_seqs = torch.from_numpy(text.copy()).cuda().repeat(REP)
        d_offs = torch.cat([(torch.arange(REP, dtype=torch.int64, device="cuda")[:, None] * B
                             + torch.from_numpy(uo[:-1]).cuda()[None, :]).reshape(-1),
                            torch.tensor([REP * B], dtype=torch.int64, device="cuda")])
        assert d_offs.numel() == n + 1 and d_seqs.numel() == REP * B
        hits = _Poisoned(torch, n * D, torch.int32)
        nk = _Poisoned(torch, n, torch.int64)
        tot = _Poisoned(torch, D + 1, torch.int64)
        s = torch.cuda.current_stream().cuda_stream
        gb.query_device(d_seqs, REP * B, d_offs, n, 1, hits.body, nk.body, tot.body, stream=s)
        torch.cuda.synchronize()
        assert gb.probe_kernel() == "wide<21,7,C16,G1>"
        assert hits.guards_intact() and nk.guards_intact() and tot.guards_intact()
        d_want = torch.from_numpy(want_h.view(np.int32)).cuda()
        slabs = hits.body.view(REP, U, D)
        for a in range(0, REP, 27):  # 19 slabs of 27 repeats
            same = (slabs[a:a + 27] == d_want[None]).flatten(1).all(dim=1)
            assert bool(same.all()), f"repeat {a + int((~same).nonzero()[0])} of {REP} differs from the oracle's matrix"
        d_n = torch.from_numpy(want_n.view(np.int64)).cuda()
        assert bool((nk.body.view(REP, U) == d_n[None]).all())
        want_tot = np.append(want_h.sum(axis=0, dtype=np.uint64), want_n.sum()) * np.uint64(REP)
        assert np.array_equal(tot.body.cpu().numpy().view(np.uint64), want_tot)

        best = _Poisoned(torch, n, torch.int32)
        bh = _Poisoned(torch, n, torch.int32)
        xs.best_device(hits.body, n, D, best.body, bh.body, stream=s)
        torch.cuda.synchronize()
        assert best.guards_intact() and bh.guards_intact() and hits.guards_intact()
        assert bool((best.body.view(REP, U) == torch.from_numpy(want_best.view(np.int32)).cuda()[None]).all())
        assert bool((bh.body.view(REP, U) == torch.from_numpy(want_max.view(np.int32)).cuda()[None]).all())
        assert bool((slabs[REP - 1] == d_want).all())  # the reduction left the matrix alone
    finally:
        gb.close()


# ---------------------------------------------------------------- B8: the read buffer
def test_read_buffer_past_2_32_bytes(xs, oracle_mod, torch):
    """B8.  A buffer of 2^32 + 64 KiB bytes (a 64 MiB random ACGT block tiled on
    the device: byte p is block[p mod 2^26] below 2^32 and block[(p + 2^25) mod
    2^26] from there on, so an offset wrapped at 2^32 finds other bytes).  Read 0 is 2^32 - 4096 bytes long;
    463 reads of 150 bp and one of 182 follow, straddling and passing 2^32, the
    last one ending on the buffer's last byte.  One call at step 2^20 + 3: read
    0 has 4096 sampled k-mers at positions up to 2^32 - 1,036,291 (several work
    units), every other read one, at its offset.  Every second sampled window is
    inserted into the bank, so half the k-mers are true positives; the
    expected row of read 0 is the sum of the oracle's rows of its 4096 windows
    taken from the block.  Through the direct and the partitioned probe of a
    classic bank and of an rbloom filter.  (A step-1 call over this buffer is
    4.3e9 k-mers, which the oracle cannot follow.)"""
    k, BLOCK, TAIL, step = 21, 1 << 26, 1 << 16, (1 << 20) + 3
    total = TWO32 + TAIL
    rng = np.random.default_rng(8)
    block = np.frombuffer(_acgt(rng, BLOCK), dtype=np.uint8)
    offs = [0, TWO32 - 4096]
    while total - offs[-1] >= 300:
        offs.append(offs[-1] + 150)
    offs.append(total)
    offs = np.asarray(offs, dtype=np.int64)
    n = offs.size - 1
    lens = np.diff(offs)
    assert n == 465 and int(lens[-1]) == 182 and (lens[1:-1] == 150).all()
    assert (offs[:-1] >= TWO32).sum() >= 400 and ((offs[:-1] < TWO32) & (offs[1:] > TWO32)).sum() == 1
    want_n = np.asarray([pl.num_kmers(int(L), k, step) for L in lens], dtype=np.uint64)
    assert int(want_n[0]) == 4096 and (want_n[1:] == 1).all()
    assert int(want_n[0]) > 2 * pl.SEG_KMERS  # several work units: the row is zeroed and added to
    pos = np.concatenate([np.arange(int(want_n[0]), dtype=np.int64) * step, offs[1:-1]])  # every sampled position
    owner = np.concatenate([np.zeros(int(want_n[0]), dtype=np.int64), np.arange(1, n)])
    assert int(pos[int(want_n[0]) - 1]) > TWO32 - (1 << 21) and (pos[:4096] >= 1 << 31).sum() >= 2000

    def byte_at(p):
        return block[np.where(p < TWO32, p, p + BLOCK // 2) % BLOCK]

    windows = [byte_at(p + np.arange(k)).tobytes() for p in pos]
    assert sum(1 for p, w in zip(pos, windows) if p >= TWO32 and w != byte_at(p - TWO32 + np.arange(k)).tobytes()) >= 400
    assert len(set(windows)) == len(windows)
    members = windows[::2]
    assert sum(1 for p in pos[::2] if p >= TWO32) >= 200  # true positives at offsets past 2^32

    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_block = torch.from_numpy(block.copy()).cuda()
    buf[:TWO32].view(TWO32 // BLOCK, BLOCK).copy_(d_block[None].expand(TWO32 // BLOCK, BLOCK))
    buf[TWO32:].copy_(d_block[BLOCK // 2:BLOCK // 2 + TAIL])
    for p in (0, BLOCK - 1, BLOCK, TWO32 - 1, TWO32, total - 1):
        assert int(buf[p]) == int(byte_at(np.asarray(p)))
    d_offs = torch.from_numpy(offs).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def rows_of(per_window):  # per sampled window -> per read
        out = np.zeros((n,) + per_window.shape[1:], dtype=np.uint32)
        np.add.at(out, owner, per_window)
        return out

    def run(gb, cols, what, want_h):
        hits = _Poisoned(torch, n * cols, torch.int32)
        nk = _Poisoned(torch, n, torch.int64)
        tot = _Poisoned(torch, cols + 1, torch.int64)
        gb.query_device(buf, total, d_offs, n, step, hits.body, nk.body, tot.body, stream=s)
        torch.cuda.synchronize()
        assert hits.guards_intact() and nk.guards_intact() and tot.guards_intact(), what
        got_n = nk.body.cpu().numpy().view(np.uint64)
        got_h = hits.body.cpu().numpy().view(np.uint32).reshape(n, cols)
        assert np.array_equal(got_n, want_n), f"{what}: num_kmers differ"
        bad = np.flatnonzero((got_h != want_h).any(axis=1))
        if bad.size:
            r = int(bad[0])
            d = int(np.flatnonzero(got_h[r] != want_h[r])[0])
            raise AssertionError(f"{what}: {bad.size} rows differ, the first read {r} at offset {int(offs[r])}: "
                                 f"doc {d} has {int(got_h[r, d])} against {int(want_h[r, d])}")
        want_tot = np.append(want_h.sum(axis=0, dtype=np.uint64), want_n.sum())
        assert np.array_equal(tot.body.cpu().numpy().view(np.uint64), want_tot), f"{what}: totals differ"

    # a classic bank: window i of the members goes to doc i mod D
    D, h, sig = 100, 7, [200_003]
    docs = [i % D for i in range(len(members))]
    ob = oracle_mod.CobsBank.empty(sig, 13, D, h, k)
    ob.build(members, docs)
    per, one = ob.query(windows)
    assert (one == 1).all() and (per[::2][np.arange(len(members)), docs] == 1).all() and int(per[1::2].sum()) < 50
    want_h = rows_of(per)
    assert int(want_h[0].sum()) >= 2048 and int(want_h[1:].sum()) >= 200
    gb = xs.Bank.create_cobs(k, h, sig, D)
    try:
        gb.build(members, docs)
        assert np.array_equal(gb.download(), ob.rows)
        for mode, kernel, path in ((0, "fast<21,7>", GATHER), (2, "cobspart", PARTITIONED)):
            gb.set_probe_options(cobs_part=mode)
            run(gb, D, f"cobs_part={mode}", want_h)
            assert (gb.probe_kernel(), gb.probe_path()) == (kernel, path), gb.probe_kernel()
    finally:
        gb.close()

    # an rbloom filter of 16 MiB + 8 bytes: the smallest the production plan partitions
    K, nbytes = 7, (16 << 20) + 8
    bf = oracle_mod.BloomFilter(np.zeros(nbytes, dtype=np.uint8), K, k)
    bf.build(members)
    per, one = bf.query(windows)
    assert (one == 1).all() and (per[::2] == 1).all() and int(per[1::2].sum()) == 0
    want_h = rows_of(per[:, None])
    assert int(want_h[0, 0]) == 2048
    gb = xs.Bank.create_bloom(k, nbytes, K)
    try:
        gb.build(members)
        assert np.array_equal(gb.download(), bf.bits)
        for mode, kernel, path in ((0, "bloom<21,7>", GATHER), (2, "bloompart", PARTITIONED)):
            gb.set_probe_options(bloom_part=mode)
            run(gb, 1, f"bloom_part={mode}", want_h)
            assert (gb.probe_kernel(), gb.probe_path()) == (kernel, path), gb.probe_kernel()
    finally:
        gb.close()
