"""The named read layouts of tests/partition_layouts.py reach the edges they
are named after (no GPU).

Every claim is asserted from the numpy restatement of the block -> read map,
for both block sizes (kCobsCK and kPartKmers, read from the shipped sources).
The last tests show once, off the GPU, that the layouts put distinct reads on
both sides of every edge: the count vectors two plausible bugs would give
(a block's first k-mer attributed to the read before; an atomically added row
stored as well, so it doubles) differ from the expected ones, so the GPU
comparison in tests/test_gpu_partitioned_edges.py fails on them.
"""
from __future__ import annotations

import numpy as np
import pytest

import partition_layouts as pl

BLOCK_SIZES = [pl.COBS_CK, pl.PART_KMERS]


def test_constants_come_from_the_sources():
    assert pl.COBS_CK in (1024, 2048, 4096) and pl.PART_KMERS % 32 == 0
    assert pl.SEG_KMERS % 32 == 0 and pl.SEG_KMERS < pl.PART_KMERS
    assert pl.COBS_CK == 1 << pl.ID_BITS               # an entry's low bits name its k-mer in the block
    assert pl.EMB_MAX_DOCS == 128 - pl.ID_BITS
    assert pl.cnt_reads(pl.COBS_CK) * pl.CNT_DIV == pl.COBS_CK
    assert pl.COBS_PAD_PARTS < pl.PART_MAX
    assert pl.STAGE_READS > pl.cnt_reads(pl.COBS_CK) + 1
    with pytest.raises(AssertionError, match="not found"):
        pl._const("xs_internal.h", "kNoSuchConstant")


def test_restated_rule_on_a_worked_example():
    T = 8
    counts = [3, 0, 5, 0, 0, 9, 7]                     # k-mer ids 0-2 | - | 3-7 | - | - | 8-16 | 17-23
    assert pl.kofs(counts).tolist() == [0, 3, 3, 8, 8, 8, 17, 24]
    assert pl.blk_read(counts, T).tolist() == [0, 5, 5]  # k-mers 0, 8 and 16
    assert pl.block_table(counts, T) == [(0, 5), (5, 5), (5, 6)]  # 24 = 3 T: the last block takes n - 1
    assert pl.block_table(counts + [0, 0], T)[-1] == (5, 8)       # ... trailing empty reads included
    assert pl.block_table(counts + [1], T) == [(0, 5), (5, 5), (5, 7), (7, 7)]


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("k", [16, 21, 31])
def test_reads_have_the_layouts_counts(k, step):
    rng = np.random.default_rng(k + step)
    counts = pl.layouts(pl.PART_KMERS, word_phase=True)["tails_1"] + [1, 2, 3]
    lens = pl.read_lengths(counts, k, step)
    reads = pl.make_reads(rng, counts, k, step)
    assert [len(r) for r in reads] == lens
    zero = {L for L, c in zip(lens, counts) if c == 0}
    assert zero == {0, k - 1}
    if step == 3:  # every slack 0..step-1 occurs: the ceil rule of num_kmers is pinned
        assert {(L - k) % step for L, c in zip(lens, counts) if c} == {0, 1, 2}


def _nr(counts, T, B):
    lo, hi = pl.block_reads(counts, T, B)
    return hi - lo + 1


@pytest.mark.parametrize("T", BLOCK_SIZES)
def test_exact(T):
    c = pl.layouts(T)["exact"]
    ko = pl.kofs(c)
    assert all(x == T for x in c) and (ko % T == 0).all()
    tab = pl.block_table(c, T)
    assert tab == [(b, b + 1) for b in range(len(c) - 1)] + [(len(c) - 1, len(c) - 1)]
    assert set(pl.read_classes(c, T)) == {"stored"}


@pytest.mark.parametrize("T", BLOCK_SIZES)
def test_off_by_one(T):
    c = pl.layouts(T)["off_by_one"]
    ko = pl.kofs(c)
    starts, ends = ko[:-1] % T, ko[1:] % T
    assert {T - 1, 0, 1} <= set(ends.tolist()) and {0, 1} <= set(starts.tolist())
    ones = [int(ko[r] % T) for r, x in enumerate(c) if x == 1]
    assert 0 in ones and T - 1 in ones                 # a 1-k-mer read first and last in a block
    cls = pl.read_classes(c, T)
    assert {"stored", "added"} == set(cls)
    # a stored read next to an added one on both sides of an edge
    assert any(a != b for a, b in zip(cls, cls[1:]))
    assert sum(pl.off_by_one_unit(T)) % T == 0         # the unit repeats block-aligned


@pytest.mark.parametrize("T", BLOCK_SIZES)
def test_cnt_edges(T):
    L = pl.layouts(T)
    cnt = pl.cnt_reads(T)
    for name, want in (("cnt_fit", cnt), ("cnt_over", cnt + 1), ("cnt_fit_empty", cnt), ("cnt_over_empty", cnt + 1)):
        c = L[name]
        assert len(pl.blk_read(c, T)) == 3 and pl.kofs(c)[-1] > 2 * T  # block 1 is not the last
        assert _nr(c, T, 1) == want, name
        lo, hi = pl.block_reads(c, T, 1)
        empties = sum(1 for x in c[lo:hi] if x == 0)
        assert empties == {"cnt_fit": 0, "cnt_over": 0, "cnt_fit_empty": 3, "cnt_over_empty": 4}[name]
        assert sum(c[lo:hi]) == T and pl.kofs(c)[lo] == T  # its reads fill it exactly
        cls = pl.read_classes(c, T)[lo:hi]
        assert {x for x in cls if x != "empty"} == ({"stored"} if want == cnt else {"added"})
    assert sum(L["cnt_fit"][1:cnt]) == T
    if T == 2048:
        assert sorted(L["cnt_fit"][1:-1]) == [66] * 30 + [68] and L["cnt_over"][1:-1] == [64] * 32


@pytest.mark.parametrize("T", BLOCK_SIZES)
def test_stage_edges(T):
    L = pl.layouts(T)
    for name, want in (("stage_fit", pl.STAGE_READS), ("stage_over", pl.STAGE_READS + 1)):
        c = L[name]
        assert pl.kofs(c)[-1] > 2 * T
        assert _nr(c, T, 1) + 1 == want, name
        assert all(x > 0 for x in c)
    if T == 2048:
        assert sorted(L["stage_fit"][1:-1]) == [8] * 252 + [16] * 2
        assert sorted(L["stage_over"][1:-1]) == [8] * 254 + [16]
    if T == 1024:
        assert sorted(L["stage_fit"][1:-1]) == [4] * 252 + [8] * 2


@pytest.mark.parametrize("T", BLOCK_SIZES)
def test_tails(T):
    L = pl.layouts(T)
    for name, target in (("tails_0", 0), ("tails_1", 1), ("tails_m1", T - 1)):
        c = L[name]
        Nk = int(pl.kofs(c)[-1])
        assert Nk % T == target and Nk > 2 * T
        assert c[:3] == [0, 0, 0] and c[-4:] == [0, 0, 0, 0]
        runs = "".join("0" if x == 0 else "x" for x in c).strip("0")
        assert "00000" in runs                         # a run of empty reads in the middle
        tab = pl.block_table(c, T)
        assert tab[-1][1] == len(c) - 1                # the last block covers the trailing empty reads
        assert tab[0][0] == 3                          # the leading ones belong to no block
        if target == 0:                                # a full last block: g0 + T == Nk
            assert len(tab) == Nk // T and tab[-2][1] == tab[-1][0]
        if target == 1:                                # a last block of one k-mer
            assert c[tab[-1][0]] > 1 and tab[-1][0] == tab[-2][1]


@pytest.mark.parametrize("T", BLOCK_SIZES)
def test_long(T):
    c = pl.layouts(T)["long"]
    assert c[0] == 7 and c[1] == 5 * T + 3 and c[2:42] == [0] * 40 and c[-1] == T - 10
    ko = pl.kofs(c)
    assert ko[1] % T and ko[1] % pl.SEG_KMERS and ko[2] % T and ko[2] % pl.SEG_KMERS  # unaligned both ends
    tab = pl.block_table(c, T)
    assert tab[1:5] == [(1, 1)] * 4                    # blocks wholly inside the long read
    assert tab[5] == (1, len(c) - 1)                   # ... and the one that spans the 40 empty reads
    assert pl.read_classes(c, T)[1] == "added"


def test_word_phase():
    c = pl.layouts(pl.PART_KMERS, word_phase=True)["word_phase"]
    ko = pl.kofs(c)
    assert [int(x) % 32 for x in ko[1:4]] == [1, 31, 0]
    assert all(x > pl.SEG_KMERS for x in c[1:4])


def test_repeated_layout_is_block_aligned():
    for T, kmers in ((pl.COBS_CK, 1_300_000), (pl.PART_KMERS, 700_000)):
        c = pl.repeated(T, kmers)
        Nk = int(pl.kofs(c)[-1])
        assert Nk % T == 0 and kmers + T <= Nk < kmers + 8 * T
        unit = pl.off_by_one_unit(T) + pl.cnt_over_unit(T)
        tab = pl.block_table(c, T)
        per = sum(unit) // T
        # every repetition meets the same edges as the first
        base = [(lo, hi) for lo, hi in tab[:per]]
        assert tab[per:2 * per] == [(lo + len(unit), hi + len(unit)) for lo, hi in base]
        assert tab[per - 1][1] - tab[per - 1][0] + 1 == pl.cnt_reads(T) + 1
        # one host chunk, so the call's k-mer ids are the layout's
        assert 3 * Nk + 32 * len(c) < pl.HOST_FIRST


def test_plans_of_the_partition_edges():
    want = {(1024, 3): (10, 1, 4, 1024), (1025, 3): (10, 2, 4, 1), (65_536, 3): (10, 64, 4, 1024),
            (524_288, 4): (10, 512, 4, 1024), (524_289, 4): (10, 513, 1, 1), (1_048_576, 4): (10, 1024, 1, 1024),
            (1_048_577, 4): (11, 513, 1, 1)}
    assert pl.COBS_PAD_PARTS == 512 and pl.PART_MAX == 1024
    for (sig, mode), (shift, P, pad, last) in want.items():
        p = pl.cobs_plan(sig, 7, mode)
        assert (p["shift"], p["P"], p["pad"], p["last_rows"]) == (shift, P, pad, last), (sig, mode)
    assert [pl.bloom_plan(n)["P"] for n in (128, 136, 8192, 131_072, 131_080)] == [1, 2, 64, 1024, 513]
    assert pl.bloom_plan(136)["last_bits"] == 64 and pl.bloom_plan(131_080)["shift"] == 11


# ---- sensitivity: a plausible bug changes a cell of the expected matrix ------------------------
@pytest.mark.parametrize("T", BLOCK_SIZES)
@pytest.mark.parametrize("name", ["exact", "off_by_one", "cnt_fit", "stage_over"])
def test_a_misattributed_edge_kmer_changes_the_matrix(T, name):
    c = pl.layouts(T)[name]
    bad = pl.misattribute_edge_kmers(c, T)
    assert sum(bad) == sum(c)                          # totals alone would not notice
    want, got = pl.closed_form(c, 3, [0, 2]), pl.closed_form(bad, 3, [0, 2])
    assert not np.array_equal(got, want)
    assert (got != want).any(axis=1).sum() >= 2        # reads on both sides of an edge


@pytest.mark.parametrize("T", BLOCK_SIZES)
@pytest.mark.parametrize("name", ["off_by_one", "cnt_over", "long"])
def test_a_doubled_edge_row_changes_the_matrix(T, name):
    c = pl.layouts(T)[name]
    bad = pl.double_added_rows(c, T)
    want, got = pl.closed_form(c, 3, [0, 2]), pl.closed_form(bad, 3, [0, 2])
    assert not np.array_equal(got, want)
    assert np.array_equal(got[:, 1], want[:, 1])       # ... only on the docs the image holds
    stored = [i for i, cls in enumerate(pl.read_classes(c, T)) if cls == "stored"]
    assert np.array_equal(got[stored], want[stored])
