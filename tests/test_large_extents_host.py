"""Filters and plans past 2^32, on the CPU: what tests/test_gpu_large_extents.py relies on.

1. The C oracle's rbloom bit indices past 2^32 bits equal the big-integer
   restatement (bloom_indexes_py), and a filter of that size built from a
   genome has no false negatives: the oracle is the yardstick of every GPU
   case over a filter of more than 2^32 bits, so its own 64-bit arithmetic is
   pinned first.  The two sizes are the GPU cases': 805,306,411 bytes (6.4e9
   bits, the first size over 2^32 bits whose production plan has more than
   256 partitions) and 2^31 + 65 bytes (the first plan of 2^25-bit
   partitions).  np.zeros of that size is mapped lazily: only the pages the
   build touches become resident.
2. The plan restatement of tests/partition_layouts.py at those sizes: the
   production rbloom plan (part_shift(mbits, 24, 20)) and the COBS plan of a
   signature over 2^27 rows.
"""
from __future__ import annotations

import numpy as np
import pytest

import partition_layouts as pl

BLOOM_SIZES = (805_306_411, (1 << 31) + 65)
K, NHASH = 21, 7


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


@pytest.mark.parametrize("nbytes", BLOOM_SIZES)
def test_oracle_bit_indices_past_2_32(oracle_mod, nbytes):
    """2000 k-mers x 7 indices: every one equals the big-integer restatement,
    lies inside the filter, and at least a quarter lie past 2^32."""
    rng = np.random.default_rng(nbytes)
    bf = oracle_mod.BloomFilter(np.zeros(nbytes, dtype=np.uint8), NHASH, K)
    mbits = nbytes * 8
    text = _acgt(rng, 2000 + K - 1)
    past = 0
    for i in range(2000):
        h = oracle_mod.xxh3_64(oracle_mod.canonical_bio(text[i:i + K]))
        got = bf.indexes(h)
        assert got == oracle_mod.bloom_indexes_py(h, NHASH, mbits), (i, h)
        assert all(0 <= x < mbits for x in got)
        past += sum(x >= 1 << 32 for x in got)
    assert past >= 14000 // 4, past  # (mbits - 2^32) / mbits of them: a third and three quarters
    assert abs(past / 14000 - (mbits - (1 << 32)) / mbits) < 0.02


@pytest.mark.parametrize("nbytes", BLOOM_SIZES)
def test_oracle_filter_past_2_32_bits_has_no_false_negatives(oracle_mod, nbytes):
    """A 20 kbp genome built into a zeroed filter of that size: every window of
    it is a member with all its k-mers, bits are set past byte 2^29 (bit 2^32),
    and their number is at most 7 per k-mer."""
    rng = np.random.default_rng(nbytes + 1)
    genome = _acgt(rng, 20_000)
    bf = oracle_mod.BloomFilter(np.zeros(nbytes, dtype=np.uint8), NHASH, K)
    bf.build([genome])
    nk = len(genome) - K + 1
    hits, n = bf.query([genome] + [genome[i:i + 150] for i in range(0, 19_850, 997)])
    assert np.array_equal(hits, n) and int(n[0]) == nk and (n[1:] == 150 - K + 1).all()
    foreign, fn = bf.query([_acgt(rng, 20_000)])
    assert int(foreign[0]) == 0 and int(fn[0]) == nk  # 1.4e5 bits of 6e9 and more: no false positive
    words = bf.bits[:nbytes // 8 * 8].view(np.uint64)
    idx = np.flatnonzero(words)
    set_bits = int(np.unpackbits(words[idx].view(np.uint8)).sum()) + int(np.unpackbits(bf.bits[nbytes // 8 * 8:]).sum())
    assert nk * NHASH * 0.99 < set_bits <= nk * NHASH
    assert (idx >= (1 << 32) // 64).sum() > set_bits // 4


# ---------------------------------------------------------------- plans
def test_production_bloom_plan_over_2_32_bits():
    """805,306,411 bytes: 2^24-bit partitions, 384 whole ones and a last one of
    344 bits; partitions 256 and up start past bit 2^32."""
    nbytes = BLOOM_SIZES[0]
    plan = pl.bloom_plan(nbytes, 2)
    assert plan["shift"] == 24 and nbytes * 8 >> 24 == 384
    assert plan["P"] == 385 and plan["last_bits"] == 344
    assert 256 << plan["shift"] == 1 << 32 and plan["P"] > 256
    assert pl.bloom_plan(nbytes, 1) == plan


def test_production_bloom_plan_takes_2_25_bit_partitions_over_2_gib():
    """2^31 bytes are kPartMax partitions of 2^24 bits; 65 bytes more are 513 of
    2^25 bits, the last one of 520 bits."""
    assert pl.PART_MAX == 1024
    below = pl.bloom_plan(1 << 31, 2)
    assert below == {"shift": 24, "P": 1024, "last_bits": 1 << 24}
    plan = pl.bloom_plan(BLOOM_SIZES[1], 2)
    assert plan == {"shift": 25, "P": 513, "last_bits": 520}
    assert pl.bloom_plan((1 << 31) + 8, 2)["shift"] == 25  # one 64-bit word over: the first size that doubles


def test_bloom_plan_keeps_its_small_filter_behaviour():
    """Mode 3 (the default of the helper) is what it was; production sizes under
    64 partitions of 2^24 bits take smaller ones, down to 2^20 bits."""
    assert pl.bloom_plan(30_011) == {"shift": 10, "P": 235, "last_bits": 30_011 * 8 - (234 << 10)}
    assert pl.bloom_plan(131_080)["shift"] == 11 and pl.bloom_plan(131_072)["P"] == 1024
    assert pl.bloom_plan(16 << 20, 2) == {"shift": 21, "P": 64, "last_bits": 1 << 21}
    assert pl.bloom_plan(1 << 20, 2)["shift"] == 20
    assert pl.bloom_plan(479_000_000, 2)["shift"] == 24  # the genus filter of tests/test_gpu_fullsize.py


def test_cobs_plan_of_a_signature_over_2_27_rows():
    """300,000,007 rows: 573 partitions of 2^19 rows in every mode that starts
    from 2^17; 2^28 rows: 1024 of 2^18.  A row in its partition and a k-mer id
    fit one 32-bit entry up to the planner's limit of 2^30 rows."""
    for mode in (1, 2, 3):
        plan = pl.cobs_plan(300_000_007, 7, mode)
        assert plan["shift"] == 19 and plan["P"] == 573 and plan["pad"] == 1
        assert plan["last_rows"] == 300_000_007 - (572 << 19)
    assert pl.cobs_plan(1 << 28, 7, 2)["shift"] == 18 and pl.cobs_plan(1 << 28, 7, 2)["P"] == 1024
    assert pl.cobs_plan((1 << 28) + 1, 7, 2)["shift"] == 19
    for sig in (1 << 27, (1 << 27) + 1, 1 << 28, 300_000_007, 38_371_819, (1 << 30) - 1):
        for mode in (2, 3, 4):
            plan = pl.cobs_plan(sig, 7, mode)
            assert plan["shift"] + pl.ID_BITS < 32 and plan["P"] <= pl.PART_MAX
            assert 0 < plan["last_rows"] <= 1 << plan["shift"]
    assert pl.cobs_plan((1 << 30) - 1, 7, 2)["shift"] == 20
    for nbytes in BLOOM_SIZES + (1 << 31, 1 << 33):
        for mode in (2, 3):
            assert pl.bloom_plan(nbytes, mode)["shift"] <= 32 and pl.bloom_plan(nbytes, mode)["P"] <= pl.PART_MAX


def test_cobs_plan_keeps_its_small_bank_behaviour():
    assert pl.cobs_plan(30_011, 7, 3)["P"] == 30 and pl.cobs_plan(30_011, 7, 3)["shift"] == 10
    assert pl.cobs_plan(1_048_577, 7, 4)["shift"] == 11
    assert pl.cobs_plan(30_011, 7, 2)["shift"] == 13  # production: partitions of 2^13 rows at the least
    assert pl.cobs_plan(38_371_819, 7, 1) == pl.cobs_plan(38_371_819, 7, 2)
    assert pl.cobs_plan(38_371_819, 7, 2)["shift"] == 17 and pl.cobs_plan(38_371_819, 7, 2)["P"] == 293
