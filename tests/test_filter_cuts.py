"""The rounding cuts of the device filter (xs_filter_cuts) and the arguments the
filter calls refuse, without a GPU.

``round(x, 2)`` is monotone in the double x, so cut[c] = the smallest double
with ``round(x, 2) >= c / 100`` reproduces the reference's keep decision
(``result.py:92-149``) by comparison.  The expected values here are Python's own
``round`` on Python floats (numpy's scalar rounding differs on some halves).
"""
from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def cuts():
    from xspect2_amd.bank import filter_cuts
    return filter_cuts().tolist()


def test_every_cut_is_the_first_double_that_rounds_up(cuts):
    assert len(cuts) == 101 and cuts[0] == 0.0
    for c in range(1, 101):
        assert round(cuts[c], 2) >= c / 100, c
        assert round(math.nextafter(cuts[c], -1), 2) < c / 100, c
    assert all(a < b for a, b in zip(cuts, cuts[1:]))


def test_exact_halves_go_to_the_even_centi_value(cuts):
    """Only 1/8, 3/8, 5/8 and 7/8 are binary halves between two centi-values; the
    odd one loses the tie, so its cut starts one ulp above the half."""
    halves = [c for c in range(1, 101) if (2 * c - 1) * 8 % 200 == 0]
    assert halves == [13, 38, 63, 88]
    for c in halves:
        half = (2 * c - 1) / 200
        assert half in (0.125, 0.375, 0.625, 0.875)
        assert round(half, 2) == (c - 1) / 100 if c % 2 else round(half, 2) == c / 100
        assert cuts[c] == (math.nextafter(half, 1) if c % 2 else half), c


def test_centi_by_counting_cuts_equals_python_round(cuts):
    rng = np.random.default_rng(11)
    pairs = [(h, n) for n in range(1, 120) for h in range(n + 1)]
    big = rng.integers(1 << 20, (1 << 32) + 1000, 4000)
    pairs += [(int(rng.integers(0, n + 1)), int(n)) for n in big]
    table = np.asarray(cuts)
    for h, n in pairs:
        x = h / n
        assert int(np.searchsorted(table, x, side="right")) - 1 == round(round(x, 2) * 100), (h, n)


def test_cuts_need_room_for_101():
    from xspect2_amd import _lib
    buf = np.zeros(101)
    assert _lib.load().xs_filter_cuts(buf.ctypes.data, 100) == _lib.XS_ERR_ARG
    assert _lib.load().xs_filter_cuts(None, 101) == _lib.XS_ERR_ARG


@pytest.mark.parametrize("threshold,label,docs", [(-0.5, 0, 3), (1.0000001, 0, 3), (float("nan"), 0, 3), (0.7, 3, 3)])
def test_refused_arguments(threshold, label, docs):
    """A threshold outside [0, 1] that is not -1 and a label past the docs are
    argument errors, reported before any device work (n = 0, no pointers)."""
    from xspect2_amd import _lib
    rc = _lib.load().xs_filter_keep_device(None, None, 0, docs, label, None, ctypes.c_double(threshold), None, None,
                                           None)
    assert rc == _lib.XS_ERR_ARG
    assert b"threshold" in _lib.load().xs_last_error() or b"label_doc" in _lib.load().xs_last_error()


def test_filter_sources_are_built_without_fast_math():
    """x = h / n must be an IEEE double division on the device."""
    from xspect2_amd import build
    assert {"xs_filter.cpp", "xs_filter.hip"} <= set(build.SOURCE_NAMES)
    flags = " ".join(build._flags())
    assert not re.search(r"fast-math|-Ofast|unsafe-fp|fp-model|no-honor|approx|daz|-ffp-contract=fast", flags), flags
    src = (ROOT / "xspect2_amd" / "csrc" / "xs_filter.hip").read_text()
    assert "__fdividef" not in src and "__frcp" not in src and "#pragma clang fp" not in src


def test_scan_block_constant_matches_the_kernel():
    from xspect2_amd.bank import FILTER_COMPACT_BLOCK
    head = (ROOT / "xspect2_amd" / "csrc" / "xs_internal.h").read_text()
    assert int(re.search(r"kCompactBlock\s*=\s*(\d+)", head).group(1)) == FILTER_COMPACT_BLOCK


def test_filter_result_kept_ids_follow_the_reference():
    from xspect2_amd.packing import PackedIds
    from xspect2_amd.result import FilterResult, ModelResult

    ids = ["a", "b", "a", "misclassified", "c"]
    keep = np.array([1, 0, 0, 1, 1], dtype=np.uint8)
    hits = {rid: {"x": int(k)} for rid, k in zip(ids, keep)}  # later records overwrite, the first position stays
    want = ModelResult("m", hits, {rid: 1 for rid in ids}).get_filtered_subsequence_labels("x", 1.0)
    for form in (ids, PackedIds.of(ids)):
        res = FilterResult("m", form, "x", 1.0, keep, keep.astype(np.uint32), np.ones(5, np.uint64))
        assert res.kept_ids() == want == ["c"]
    plain = FilterResult("m", ["r0", "r1", "r2"], "x", 0.5, [0, 1, 1], [0, 5, 9], [9, 9, 9])
    assert plain.kept_ids() == ["r1", "r2"] and plain.kept_index().tolist() == [1, 2]
