"""The poisoned, guarded output buffer of tests/partition_layouts.py catches
what it is there to catch (no GPU, numpy only).

tests/test_gpu_output_buffers.py lays every output of a query over an
allocation full of a poison byte and compares the body with a closed form.
Here a correct matrix is written into such a buffer by a model of each way the
zeroing rules and the stores of the probe paths can disagree, and the same
comparison must fail, for both poisons, naming the class of the row:

(a) a row of each read class left untouched;
(b) a row of each class added without being zeroed first;
(c) one element written before the body and one after it;
(d) a whole-row store that skips its zero cells.

The batches and layouts of the GPU file are also held to the read classes
they claim, so the GPU cases cannot lose a class unnoticed.
"""
from __future__ import annotations

import numpy as np
import pytest

import partition_layouts as pl

MIXED = [0, 1, 0, 0, 256, 257, 0, 512, 513, 255, 0, 64, 769, 0]
DOCS = [0, 31, 32, 63, 64, 96]
D = 97  # odd: rows are 4-byte aligned only


def _first(classes, cls):
    return classes.index(cls)


def _laid(byte, phase, dtype=np.uint32, counts=MIXED, docs=DOCS):
    want = pl.closed_form(counts, D, docs).astype(dtype)
    g = pl.GuardedArray(want.size, dtype, byte, phase)
    return g, g.body.reshape(want.shape), want


def test_unit_classes():
    assert pl.SEG_KMERS == 256
    assert pl.unit_classes([0, 1, 255, 256, 257, 512, 513]) == ["empty", "whole", "whole", "whole", "split", "split",
                                                              "split"]
    assert set(pl.unit_classes(MIXED)) == {"empty", "whole", "split"}
    cls = pl.unit_classes(MIXED)
    assert cls[0] == cls[-1] == "empty" and cls[2] == cls[3] == "empty"  # first, last, doubled
    assert cls[5] == "split" and cls[6] == "empty" and cls[7] == "split"  # between split reads


@pytest.mark.parametrize("dtype,phase", [(np.uint32, 0), (np.uint32, 4), (np.uint64, 0), (np.uint64, 8), (np.uint8, 1),
                                         (np.uint16, 2)])
@pytest.mark.parametrize("byte", pl.POISON_BYTES)
def test_guarded_array_layout(byte, dtype, phase):
    g = pl.GuardedArray(7 * 3, dtype, byte, phase)
    size = np.dtype(dtype).itemsize
    assert g.ptr % 16 == phase and g.body.size == 21
    assert g.off >= pl.GUARD_ELEMS * size and g.raw.size - g.off - g.nbytes >= pl.GUARD_ELEMS * size
    assert (g.body == pl.poison_of(byte, dtype)).all()
    assert pl.poison_of(byte, np.uint32) in (0xFFFFFFFF, 0x5A5A5A5A)
    assert pl.poison_of(byte, np.uint64) in (0xFFFFFFFFFFFFFFFF, 0x5A5A5A5A5A5A5A5A)
    g.body[:] = 3
    assert (g.check() == 3).all()  # a correct writer passes


@pytest.mark.parametrize("phase", [0, 4])
@pytest.mark.parametrize("byte", pl.POISON_BYTES)
def test_a_correct_writer_passes(byte, phase):
    g, body, want = _laid(byte, phase)
    pl.write_rows(body, want)
    got = g.check("correct").reshape(want.shape)
    assert pl.explain_rows(got, want, pl.unit_classes(MIXED), byte) is None
    pl.assert_rows(got, want, pl.unit_classes(MIXED), byte)


@pytest.mark.parametrize("cls", ["empty", "whole", "split"])
@pytest.mark.parametrize("byte", pl.POISON_BYTES)
def test_a_untouched_row_is_caught(byte, cls):
    classes = pl.unit_classes(MIXED)
    g, body, want = _laid(byte, 4)
    r = _first(classes, cls)
    pl.write_rows(body, want, untouched={r})
    got = g.check().reshape(want.shape)
    msg = pl.explain_rows(got, want, classes, byte)
    assert msg is not None and f"first row {r} ({cls})" in msg and "never written" in msg
    with pytest.raises(AssertionError, match=cls):
        pl.assert_rows(got, want, classes, byte, "model a")


@pytest.mark.parametrize("cls", ["empty", "whole", "split"])
@pytest.mark.parametrize("byte", pl.POISON_BYTES)
def test_b_row_added_without_zeroing_is_caught(byte, cls):
    """An empty read's row added onto the poison gets nothing added: it reads
    as never written.  A row with counts reads as poison + c (0xFF..: c - 1)."""
    classes = pl.unit_classes(MIXED)
    g, body, want = _laid(byte, 0)
    r = _first(classes, cls)
    pl.write_rows(body, want, added={r})
    got = g.check().reshape(want.shape)
    msg = pl.explain_rows(got, want, classes, byte)
    assert msg is not None and f"first row {r} ({cls})" in msg
    if cls != "empty":
        c = MIXED[r]
        assert int(got[r, DOCS[0]]) == (c - 1 if byte == 0xFF else 0x5A5A5A5A + c)
        assert int(got[r, 1]) == pl.poison_of(byte, np.uint32)  # a cell no add touches
    with pytest.raises(AssertionError, match=cls):
        pl.assert_rows(got, want, classes, byte, "model b")


@pytest.mark.parametrize("dtype,phase", [(np.uint32, 4), (np.uint64, 8), (np.uint8, 1)])
@pytest.mark.parametrize("byte", pl.POISON_BYTES)
def test_c_writes_outside_the_body_are_caught(byte, dtype, phase):
    for where in ("before", "after"):
        g = pl.GuardedArray(33, dtype, byte, phase)
        g.body[:] = 1
        size = np.dtype(dtype).itemsize
        lo = g.off - size if where == "before" else g.off + g.nbytes
        g.raw[lo:lo + size].view(dtype)[0] = 0  # the correct value of a zero cell, one element out of range
        with pytest.raises(AssertionError, match="before the output" if where == "before" else "past the output"):
            g.check("model c")
    g = pl.GuardedArray(33, dtype, byte, phase)  # the far end of each guard counts as well
    g.raw[0] ^= 1
    with pytest.raises(AssertionError, match="before the output"):
        g.check()
    g = pl.GuardedArray(33, dtype, byte, phase)
    g.raw[-1] ^= 1
    with pytest.raises(AssertionError, match="past the output"):
        g.check()


@pytest.mark.parametrize("cls", ["whole", "split"])
@pytest.mark.parametrize("byte", pl.POISON_BYTES)
def test_d_whole_row_store_skipping_zero_cells_is_caught(byte, cls):
    classes = pl.unit_classes(MIXED)
    g, body, want = _laid(byte, 4)
    r = _first(classes, cls)
    pl.write_rows(body, want, sparse={r})
    got = g.check().reshape(want.shape)
    assert np.array_equal(got[r, DOCS], want[r, DOCS])  # its counts are all there
    msg = pl.explain_rows(got, want, classes, byte)
    assert msg is not None and f"first row {r} ({cls})" in msg and "never written" in msg
    # on a buffer of zeros, which a fresh allocation usually is, the same writer passes
    zeros = np.zeros_like(want)
    pl.write_rows(zeros, want, sparse={r}, untouched={_first(classes, "empty")})
    assert np.array_equal(zeros, want)


@pytest.mark.parametrize("byte", pl.POISON_BYTES)
def test_models_on_the_partitioned_classes(byte):
    """The same models on a partitioned layout's classes (empty, stored, added)."""
    T = pl.COBS_CK
    counts = pl.layouts(T)["tails_1"]
    classes = pl.read_classes(counts, T)
    assert set(classes) == {"empty", "stored", "added"}
    for cls in ("empty", "stored", "added"):
        r = classes.index(cls)
        for kind in ("untouched", "added", "sparse"):
            if kind == "sparse" and cls == "empty":
                continue  # a row of zeros only: the same as untouched
            g, body, want = _laid(byte, 0, counts=counts)
            pl.write_rows(body, want, **{kind: {r}})
            with pytest.raises(AssertionError, match=rf"first row {r} \({cls}\)"):
                pl.assert_rows(g.check().reshape(want.shape), want, classes, byte, kind)


def test_narrow_poisons_are_no_valid_count():
    """One-byte hit rows: 0xFF and 0x5A are counts a read can have, so the
    batches of the narrow cases avoid 90 and 255 k-mers per read."""
    import test_gpu_output_buffers as ob
    for counts in ob.NARROW_BATCHES.values():
        assert not {90, 255} & set(counts) and max(counts) <= 0xFF


def test_batches_hold_the_classes_they_claim():
    import test_gpu_output_buffers as ob
    for name, (counts, classes) in ob.BATCHES.items():
        assert set(pl.unit_classes(counts)) == set(classes), name
    assert ob.BATCHES["mixed"][0] == MIXED
    seen = set()
    for name, counts in pl.layouts(pl.COBS_CK).items():
        cls = set(pl.read_classes(counts, pl.COBS_CK))
        assert cls == set(ob.COBS_LAYOUT_CLASSES[name]), (name, cls)
        seen |= cls
    assert seen == {"empty", "stored", "added"}
    for name, counts in pl.layouts(pl.PART_KMERS, word_phase=True).items():
        assert set(pl.unit_classes(counts)) == set(ob.BLOOM_LAYOUT_CLASSES[name]), name
