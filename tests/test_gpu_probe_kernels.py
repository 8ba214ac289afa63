"""One named parity case per compiled direct COBS probe kernel (GPU).

The direct COBS probe is 57 separately compiled instantiations (fast, vslice,
wide, slots, general), chosen at run time by the bank's shape; each has its own
lane, chunk and group arithmetic.  Every table row below names the kernel its
bank must route to (Bank.probe_kernel, taken from the same table entry as the
launched function) and compares it with the oracle on three bank images:

1. built: documents hashed into the bank; true-positive reads are cut from the
   first, middle and last document of every group, so full counts (256 per
   unit) land on the group edges and on the bank's last doc;
2. chosen documents: every row has exactly the bits of a boundary set of docs
   set, so a read's count is its k-mer count on those docs and 0 elsewhere,
   whatever the hashes are: the doc-index mapping of the kernel alone;
3. all ones: every doc bit below D set, every counter of every lane at its
   maximum at once.

Reads have exactly n k-mers for n at the carry-save batch, 64-lane tile and
256-k-mer unit edges, at steps 1 and 3.  The completeness test holds the
table, plus the instantiations no bank of test size reaches, to the list the
library itself reports.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import _explain, _pair, _reads

pytestmark = pytest.mark.gpu

STEPS = (1, 3)
EDGE_KMERS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513)
KH = {(21, 7): "21,7", (31, 1): "31,1", (25, 3): "0,0"}


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


def _rows():
    """(D, k, h, page, G, kernel): page None = classic.  Per instantiation the
    narrowest bank that still routes to it and the widest."""
    t = []
    # fast: classic, <= 128 docs, the two trained (k, h)
    for k, h in ((21, 7), (31, 1)):
        for D in (1, 128):
            t.append((D, k, h, None, 1, f"fast<{k},{h}>"))
    # vslice: one hash, 1-4 groups of 64-byte pages; KT = 31 or any other k
    for k, kt in ((31, "31"), (21, "0")):
        for G in (1, 2, 3, 4):
            for D in (512 * (G - 1) + 1, 512 * G):
                t.append((D, k, 1, 64, G, f"vslice<{kt},{G}>"))
    # ... and classic banks of 505-512 docs with one hash (their page is 64 bytes)
    t.append((512, 31, 1, None, 1, "vslice<31,1>"))
    t.append((509, 21, 1, None, 1, "vslice<0,1>"))
    # wide, one group: classic banks of 2..16 data chunks
    for (k, h), kh in KH.items():
        for C, widths in ((2, (129, 256)), (4, (257, 504, 512)), (8, (513, 1024)), (16, (1025, 2048))):
            for D in widths:
                if D == 512 and h == 1:
                    continue  # one hash and a 64-byte page: vslice (above)
                t.append((D, k, h, None, 1, f"wide<{kh},C{C},G1>"))
    # wide, 2-4 groups of 2..4-chunk pages
    for (k, h), kh in (((31, 1), "31,1"), ((25, 3), "0,0")):
        for G in (2, 3, 4):
            for C, pages in ((2, (17, 32)), (4, (33, 63 if h == 1 else 64))):
                t.append(((G - 1) * 8 * pages[0] + 1, k, h, pages[0], G, f"wide<{kh},C{C},G{G}>"))
                t.append((G * 8 * pages[1], k, h, pages[1], G, f"wide<{kh},C{C},G{G}>"))
    t.append((2 * 8 * 33 + 1, 21, 7, 33, 3, "wide<0,0,C4,G3>"))  # species (k, h) on a compact bank
    # slots: compact banks of more groups than wide takes, or of one-chunk pages
    for (k, h), kh in (((31, 1), "31,1"), ((25, 3), "0,0")):
        for gm, cm, page, groups in ((4, 1, 1, (2, 4)), (8, 1, 1, (5, 8)), (16, 1, 1, (9, 16)), (8, 2, 17, (5, 8))):
            t.append(((groups[0] - 1) * 8 * page + 1, k, h, page, groups[0], f"slots<{kh},{gm},{cm}>"))
            t.append((groups[1] * 8 * page, k, h, page, groups[1], f"slots<{kh},{gm},{cm}>"))
    # ... and classic banks of <= 128 docs whose (k, h) the fast kernel is not compiled for
    t.append((1, 25, 3, None, 1, "slots<0,0,1,4>"))
    t.append((128, 25, 3, None, 1, "slots<0,0,1,4>"))
    # general: one row per reason it is taken
    t.append((2049, 21, 7, None, 1, "general"))       # classic rows of 17 chunks
    t.append((16 * 8 + 1, 31, 1, 1, 17, "general"))   # 17 groups of one chunk
    t.append((8 * 136 + 1, 25, 3, 17, 9, "general"))  # 9 groups of two chunks
    t.append((4 * 264 + 1, 31, 1, 33, 5, "general"))  # 5 groups of three chunks
    t.append((520 + 1, 21, 7, 65, 2, "general"))      # 2 groups of five chunks
    return t


ROWS = _rows()

# Compiled, but only reached by a bank with a group of >= 2^30 rows
# (fastmod_small's limit in wide and vslice; 137 GB at 128 bytes a row): every
# smaller bank of their shape is taken by vslice or wide first.  No bank XspecT
# trains is that large; DESIGN.md lists them.  slots<21,7,1,4> and
# slots<31,1,1,4>, which take the classic banks of <= 128 docs over the fast
# kernel's limit of 2^28 rows, have their case in
# tests/test_gpu_large_extents.py (B4: 300,000,007 rows, a 4.8 GB image).
LARGE_EXTENT_CASES = {"slots<21,7,1,4>", "slots<31,1,1,4>"}
UNREACHABLE_AT_TEST_SIZE = {
    "slots<21,7,1,8>": "classic 513-1024 docs: wide<C8> takes it below 2^30 rows",
    "slots<31,1,1,8>": "classic 513-1024 docs: wide<C8> takes it below 2^30 rows",
    "slots<0,0,1,8>": "classic 513-1024 docs: wide<C8> takes it below 2^30 rows",
    "slots<0,0,2,4>": "2 groups of 3-4 chunks: wide<C4,G2> (or vslice) takes it below 2^30 rows",
    "slots<0,0,3,4>": "3 groups of 3-4 chunks: wide<C4,G3> (or vslice) takes it below 2^30 rows",
    "slots<0,0,4,4>": "4 groups of 3-4 chunks: wide<C4,G4> (or vslice) takes it below 2^30 rows",
    "slots<31,1,2,4>": "2 groups of 3-4 chunks: wide<C4,G2> or vslice takes it below 2^30 rows",
    "slots<31,1,3,4>": "3 groups of 3-4 chunks: wide<C4,G3> or vslice takes it below 2^30 rows",
    "slots<31,1,4,4>": "4 groups of 3-4 chunks: wide<C4,G4> or vslice takes it below 2^30 rows",
    "slots<0,0,4,2>": "2-4 groups of 2 chunks: wide<C2> takes it below 2^30 rows",
    "slots<31,1,4,2>": "2-4 groups of 2 chunks: wide<C2> takes it below 2^30 rows",
}


def _sigs(D, k, h, page, G):
    """Distinct signature sizes of 500-3000 rows per group, seeded by the shape.
    Two divisors Barrett reduction can get wrong stand in the table: 1024 (a
    power of two) in the first one-group row and 2047 (2^11 - 1) in the first
    group of every compact bank of three groups."""
    rng = np.random.default_rng([D, k, h, page or 0, G])
    sig = [int(x) for x in rng.choice(np.arange(500, 3001), size=G, replace=False)]
    if G == 1 and D in (1, 512, 1024):
        sig[0] = 1024
    if G == 3:
        sig[0] = 2047
    return sig


def _group_docs(D, page, G):
    P = page if page is not None else (D + 7) // 8
    return P, [(g * 8 * P, min(D, (g + 1) * 8 * P)) for g in range(G)]


def _edge_docs(D, page, G):
    """First, middle and last document of every group."""
    P, groups = _group_docs(D, page, G)
    out = []
    for lo, hi in groups:
        out += [lo] + ([lo + 4 * P] if lo + 4 * P < hi else []) + [hi - 1]
    return sorted(set(out))


def _boundary_docs(D, page, G):
    """The docs of the chosen-document image: the 32- and 64-doc edges of the
    transposes and stores, the bank's last doc, both ends of every group."""
    _, groups = _group_docs(D, page, G)
    s = {0, 31, 32, 63, 64, D - 1} | {lo for lo, _ in groups} | {hi - 1 for _, hi in groups}
    return sorted(d for d in s if 0 <= d < D)


def _image(sig, D, page, G, docs):
    """A bank image (file layout) whose every row has exactly the bits of `docs` set."""
    P, groups = _group_docs(D, page, G)
    parts = []
    for g, (lo, hi) in enumerate(groups):
        row = np.zeros(P, np.uint8)
        for d in docs:
            if lo <= d < hi:
                row[(d - lo) >> 3] |= 1 << ((d - lo) & 7)
        parts.append(np.tile(row, sig[g]))
    return np.concatenate(parts)


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _edge_lengths(k):
    return sorted({k + (n - 1) * s for n in EDGE_KMERS for s in STEPS})


def _read_set(rng, k, sources):
    """Reads of exactly n k-mers at step 1 and at step 3 for every n of
    EDGE_KMERS, each cut from the next of `sources` (all at least as long as the
    longest of them); the empty read, k - 1 and k bytes; N, IUPAC and lower
    case; about 100 random reads."""
    reads = [sources[i % len(sources)][:L] for i, L in enumerate(_edge_lengths(k))]
    reads += [b"", sources[0][:k - 1], sources[-1][:k]]
    odd = bytearray(sources[0][:200])
    for i, c in zip(range(3, 200, 9), b"NnacgtRYKMSWryNacgtnBDHV"):
        odd[i] = c
    reads += [bytes(odd)]
    reads += _reads(rng, 100, k)
    return reads


def _expect(ob, reads, closed_form_docs=None, full_unit=False):
    """The oracle's answer at every step, computed once per image.
    closed_form_docs: the docs whose count must be the read's k-mer count
    (every other doc 0), which the oracle itself is held to."""
    want = {}
    for step in STEPS:
        want_h, want_n = ob.query(reads, step=step)
        if closed_form_docs is not None:
            closed = np.zeros_like(want_h)
            closed[:, closed_form_docs] = want_n.astype(np.uint32)[:, None]
            assert np.array_equal(want_h, closed), "the oracle misses the closed form"
        if full_unit and step == 1:
            assert int(want_h.max()) >= 256  # a full unit's count is really there
        want[step] = (want_h, want_n)
    return want


def _check(gb, want, reads, kernel):
    """Hits, k-mer counts, totals and the kernel's name, at every step."""
    for step in STEPS:
        want_h, want_n = want[step]
        got_h, got_n = gb.query(reads, step=step)
        assert gb.probe_kernel() == kernel, f"step {step}: routed to {gb.probe_kernel()}"
        assert np.array_equal(got_n, want_n), f"num_kmers differ (step {step})"
        assert got_h.shape == want_h.shape
        assert np.array_equal(got_h, want_h), f"step {step}: " + _explain(got_h, want_h, reads)
        tot, nk = gb.query_totals(reads, step=step)
        assert gb.probe_kernel() == kernel
        assert np.array_equal(tot, want_h.sum(axis=0, dtype=np.uint64)), f"totals differ (step {step})"
        assert nk == int(want_n.sum())


def _bank(xs, k, h, sig, D, page):
    gb = xs.Bank.create_cobs(k, h, sig, D, page_size=page, compact=page is not None)
    gb.set_probe_options(cobs_part=0)
    return gb


@pytest.mark.parametrize("D,k,h,page,G,kernel", ROWS, ids=[f"{r[5]}-D{r[0]}-k{r[1]}h{r[2]}-p{r[3]}" for r in ROWS])
def test_probe_kernel_case(xs, oracle_mod, D, k, h, page, G, kernel):
    P, groups = _group_docs(D, page, G)
    assert len(groups) == G and groups[-1][0] < D <= G * 8 * P
    sig = _sigs(D, k, h, page, G)
    rng = np.random.default_rng([k, h, D, G])
    longest = _edge_lengths(k)[-1]
    edge = _edge_docs(D, page, G)

    # 1. built image: the edge docs are long enough to give every edge read,
    # the others short (a column is one doc's own filter)
    seqs = [_acgt(rng, longest if d in edge else int(rng.integers(k, 300))) for d in range(D)]
    ob = oracle_mod.CobsBank.empty(sig, P, D, h, k)
    ob.build(seqs, list(range(D)))
    gb = _bank(xs, k, h, sig, D, page)
    gb.upload(ob.rows)
    sources = [seqs[d] for d in edge]
    reads = _read_set(rng, k, sources) + [s[:k + 255] for s in sources]  # one whole unit from every edge doc
    want = _expect(ob, reads, full_unit=True)
    for small in (1, 0):  # one round trip (units taken one at a time); the chunked pipeline (four at a time)
        gb.set_probe_options(small_calls=small)
        _check(gb, want, reads, kernel)

    # 2. chosen documents, 3. all ones: closed forms, whatever the hashes are
    reads = _read_set(rng, k, [_acgt(rng, longest)])
    for docs in (_boundary_docs(D, page, G), list(range(D))):
        ob = oracle_mod.CobsBank(_image(sig, D, page, G, docs), sig, P, D, h, k)
        gb.upload(ob.rows)
        want = _expect(ob, reads, closed_form_docs=docs)
        for small in (1, 0):
            gb.set_probe_options(small_calls=small)
            _check(gb, want, reads, kernel)
    gb.close()


def test_vslice_takes_512_doc_slices_of_a_classic_bank(xs, oracle_mod, tmp_path):
    """A classic bank of 1024 docs with one hash, reopened as the doc slices
    [0, 512) and [512, 1024): each slice's page is 64 bytes, so both take the
    bit-sliced kernel; side by side they are the whole bank's hits."""
    from xspect2_amd import _lib
    D, k, h, sig = 1024, 31, 1, [2047]
    ob, gb, seqs, _ = _pair(xs, oracle_mod, D, k, h, sig, seed=1024, per_doc=1)
    path = tmp_path / "index.cobs_classic"
    gb.save(path)
    gb.close()
    rng = np.random.default_rng(31)
    longest = _edge_lengths(k)[-1]
    sources = [s for s in (seqs[0], seqs[511], seqs[512], seqs[1023])]
    reads = [s[:300] for s in sources] + _read_set(rng, k, [_acgt(rng, longest)])
    for step in STEPS:
        want_h, want_n = ob.query(reads, step=step)
        parts = []
        for lo, hi in ((0, 512), (512, 1024)):
            b = xs.Bank.open(path, _lib.XS_BANK_COBS_CLASSIC, docs=(lo, hi))
            b.set_probe_options(cobs_part=0)
            hh, nn = b.query(reads, step=step)
            assert b.probe_kernel() == "vslice<31,1>"
            assert np.array_equal(nn, want_n)
            parts.append(hh)
            b.close()
        got_h = np.concatenate(parts, axis=1)
        assert np.array_equal(got_h, want_h), _explain(got_h, want_h, reads)


def test_every_compiled_kernel_has_a_case(xs):
    """The table's kernels, the two with a case among the large banks of
    tests/test_gpu_large_extents.py, plus the 11 no bank of test size reaches
    are exactly the instantiations the library compiled: a new instantiation
    needs a case, a case whose kernel is gone fails."""
    import test_gpu_large_extents as large
    compiled = xs.probe_kernel_names()
    assert len(compiled) == len(set(compiled)) == 57
    covered = {r[5] for r in ROWS}
    large_routes = {route[1] for case in large.COBS_CASES for route in case.values[-1]}
    assert LARGE_EXTENT_CASES <= large_routes and not covered & LARGE_EXTENT_CASES
    covered |= LARGE_EXTENT_CASES
    assert len(covered) == 46 and len(UNREACHABLE_AT_TEST_SIZE) == 11
    assert not covered & set(UNREACHABLE_AT_TEST_SIZE)
    assert covered | set(UNREACHABLE_AT_TEST_SIZE) == set(compiled)
