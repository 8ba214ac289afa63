"""Bank files onto the device (xs_bank_open / xs_bank_open_docs, GPU).

A model load reads the whole index (ProbabilisticFilterModel.load,
probabilistic_filter_model.py:351-391); the library streams the payload in
32 MiB pieces through a ring of three pinned slots.  These cases make the
ring wrap several times, with a last piece that is not a whole piece and
rows (13 B for 100 docs) that straddle the pieces: the opened image, read
back, equals the bytes saved, for a classic bank, a compact bank and an
rbloom filter; doc slices equal the file's byte columns cut on the host.

Corrupt files (second half): every curated bad file is refused with its code
before any device work, the valid file then opens in the same process and
answers as the oracle does, and the model classes' loads raise on a corrupt
index and work on the intact one.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bank_mod():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


def _roundtrip(bank_mod, b, tmp_path, kind, name):
    rng = np.random.default_rng(sum(name.encode()))
    payload = rng.integers(0, 256, b.payload_bytes(), dtype=np.uint8)
    b.upload(payload)
    path = tmp_path / name
    b.save(path)
    b.close()
    got = bank_mod.Bank.open(path, kind, device=0)
    try:
        assert np.array_equal(got.download(), payload)
    finally:
        got.close()
    return path, payload


def test_classic_file_over_many_pieces(bank_mod, tmp_path):
    """100 docs (13-B rows padded to 16 on the device), 9,000,011 rows:
    117 MB of payload, 3.5 pieces; then doc slices of it."""
    from xspect2_amd._lib import XS_BANK_COBS_CLASSIC
    D, S = 100, 9_000_011
    b = bank_mod.Bank.create_cobs(21, 7, [S], D, [f"d{i}" for i in range(D)])
    path, payload = _roundtrip(bank_mod, b, tmp_path, XS_BANK_COBS_CLASSIC, "big.cobs_classic")
    rows = payload.reshape(S, 13)
    for lo, hi in ((0, 8), (8, 64), (96, 100), (0, 100)):
        sl = bank_mod.Bank.open(path, XS_BANK_COBS_CLASSIC, device=0, docs=(lo, hi))
        try:
            # the open staged one ~32 MiB piece of whole rows at a time, never the whole 117 MB
            # of rows (config 5's split is for banks one GPU cannot hold), and kept none
            held, peak = sl.workspace_bytes()
            assert held == 0 and 0 < peak <= 33 << 20 < S * 13, (lo, hi, held, peak)
            want = np.ascontiguousarray(rows[:, lo // 8: lo // 8 + (hi - lo + 7) // 8])
            assert np.array_equal(sl.download(), want.reshape(-1)), (lo, hi)
        finally:
            sl.close()


def test_compact_file_over_many_pieces(bank_mod, tmp_path):
    """A compact bank of 3 groups (64-B rows) of different signature sizes:
    ~105 MB of payload."""
    from xspect2_amd._lib import XS_BANK_COBS_COMPACT
    D = 1430
    b = bank_mod.Bank.create_cobs(31, 1, [700_001, 500_003, 440_009], D, [f"a{i}" for i in range(D)],
                                  page_size=64, compact=True)
    _roundtrip(bank_mod, b, tmp_path, XS_BANK_COBS_COMPACT, "big.cobs_compact")


def test_rbloom_file_over_many_pieces(bank_mod, tmp_path):
    """An rbloom filter of 100 MB + 7 bytes."""
    from xspect2_amd._lib import XS_BANK_RBLOOM
    b = bank_mod.Bank.create_bloom(21, 100_000_007, 7)
    _roundtrip(bank_mod, b, tmp_path, XS_BANK_RBLOOM, "big.bloom")


def test_failed_save_leaves_the_existing_file(bank_mod, tmp_path):
    """xs_bank_save writes beside the destination and renames the file over it
    once whole: a save that fails (here: the temporary name is
    taken by a directory) returns an error and leaves the model already at
    the path byte for byte, with no partial file; a save that succeeds
    replaces it and leaves nothing else behind."""
    import os

    from xspect2_amd import _lib
    from xspect2_amd._lib import XS_BANK_COBS_CLASSIC
    D, S = 100, 300_007
    b = bank_mod.Bank.create_cobs(21, 7, [S], D, [f"d{i}" for i in range(D)])
    rng = np.random.default_rng(5)
    old = rng.integers(0, 256, b.payload_bytes(), dtype=np.uint8)
    b.upload(old)
    path = tmp_path / "m.cobs_classic"
    b.save(path)
    before = path.read_bytes()
    new = rng.integers(0, 256, b.payload_bytes(), dtype=np.uint8)
    b.upload(new)
    blocker = tmp_path / f"m.cobs_classic.xs-part-{os.getpid()}"
    blocker.mkdir()
    rc = _lib.load().xs_bank_save(b.handle, str(path).encode())
    assert rc == _lib.XS_ERR_IO, rc
    assert path.read_bytes() == before
    blocker.rmdir()
    b.save(path)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["m.cobs_classic"]
    got = bank_mod.Bank.open(path, XS_BANK_COBS_CLASSIC, device=0)
    try:
        assert np.array_equal(got.download(), new)
    finally:
        got.close()
        b.close()


# ---- corrupt files are refused, and a healthy open follows in the same process ------------------------------------
# Valid files come from the oracle's writers over oracle-built banks, never from xs_bank_save.  A handle is never
# queried, built into or downloaded unless oracle.bank_file_geometry accepts its file: a file the reference reader
# refuses must be refused by the library, and a handle it hands out for one is closed and fails the test there.
def _dna(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _flip(data, off, bit):
    v = int.from_bytes(data[off:off + 8], "little") ^ 1 << bit
    return data[:off] + v.to_bytes(8, "little") + data[off + 8:]


def _put(data, off, width, value):
    return data[:off] + value.to_bytes(width, "little") + data[off + width:]


def _oracle_file(oracle, kind):
    """(file bytes, oracle bank, doc sequences) of one small oracle-built bank of this kind."""
    rng = np.random.default_rng(40 + len(kind))
    if kind == "classic":
        docs = [_dna(rng, 120) for _ in range(64)]       # 64 docs: 8-byte rows, a power of two
        ob = oracle.CobsBank.empty([521], 8, 64, 7, 21)
        ob.build(docs, list(range(64)))
        return oracle.cobs_classic_file([f"GCF_{i:09d}" for i in range(64)], 21, 7, 521, ob.rows), ob, docs
    if kind == "compact":
        docs = [_dna(rng, 100) for _ in range(150)]      # 3 groups of 64 docs (8-byte pages), the last partial
        ob = oracle.CobsBank.empty([211, 157, 181], 8, 150, 1, 31)
        ob.build(docs, list(range(150)))
        return oracle.cobs_compact_file([f"Allele_ID_{i}" for i in range(150)], 31, 1, [211, 157, 181], 8,
                                        ob.rows), ob, docs
    docs = [_dna(rng, 400) for _ in range(4)]
    ob = oracle.BloomFilter(np.zeros(2003, dtype=np.uint8), 7, 21)
    ob.build(docs)
    return oracle.rbloom_file(7, ob.bits), ob, docs


def _corruptions(kind, data, geom):
    """{name: (bytes, expected code name)}: the curated bad files of one valid file."""
    off = geom["payload_offset"]
    if kind == "rbloom":  # no length and no magic in the layout: what can be wrong is K and the file's end
        return {"K + 2^32": (_put(data, 0, 8, 2**32 + 7), "UNSUPPORTED"), "K = 0": (_put(data, 0, 8, 0), "UNSUPPORTED"),
                "no filter bytes": (data[:8], "FORMAT"), "cut inside K": (data[:5], "FORMAT")}
    sig_at = [31] if kind == "classic" else [35 + 16 * g for g in range(geom["groups"])]
    h_at = [39] if kind == "classic" else [43 + 16 * g for g in range(geom["groups"])]
    docs_at = 22 if kind == "classic" else 43 + 16 * geom["groups"]
    bad = {"payload one byte short": (data[:-1], "FORMAT"), "payload one byte long": (data + b"\0", "FORMAT"),
           "payload cut in half": (data[:off + (len(data) - off) // 2], "FORMAT"),
           "wrong magic": (b"COBZ" + data[4:], "FORMAT"),
           "num_docs + 8, names unchanged": (_put(data, docs_at, 4, geom["docs"] + 8), "FORMAT")}
    for g, at in enumerate(sig_at):
        for bit in (61, 62, 63):  # 8-byte pages: sum(sig) * page is unchanged modulo 2^64
            bad[f"sig{g} bit {bit}"] = (_flip(data, at, bit), "FORMAT")
    many = data
    for at in h_at:  # every group's, or the header is refused as mixed
        many = _put(many, at, 8, 2**32 + geom["h"])
    bad["num_hashes + 2^32"] = (many, "UNSUPPORTED")
    return bad


def _refused(lib_mod, oracle, path, kind_name, data, code_name, what, docs=False):
    """Opens a bad file (written to `path`) and checks the refusal; never keeps a handle of it."""
    import ctypes
    kind = {"classic": 0, "compact": 1, "rbloom": 2}[kind_name]
    with pytest.raises(oracle.BankFileError):  # the reference reader refuses it: the library must
        oracle.bank_file_geometry(data, kind_name)
    path.write_bytes(data)
    lib = lib_mod.load()
    h = ctypes.c_void_p(0xDEAD)
    if docs:
        rc = lib.xs_bank_open_docs(str(path).encode(), 0, 0, 8, ctypes.byref(h))
    else:
        rc = lib.xs_bank_open(str(path).encode(), kind, 0, ctypes.byref(h))
    if rc == lib_mod.XS_OK:
        lib.xs_bank_close(h)
        pytest.fail(f"{what}: a file the reference reader refuses was opened")
    assert rc == getattr(lib_mod, "XS_ERR_" + code_name), (what, rc, lib.xs_last_error())
    assert h.value is None, what
    assert str(path).encode() in lib.xs_last_error(), (what, lib.xs_last_error())


@pytest.mark.parametrize("kind_name", ["classic", "compact", "rbloom"])
def test_corrupt_files_are_refused_then_the_valid_file_opens(bank_mod, oracle_mod, tmp_path, kind_name):
    """The curated refusals (payload short, long and halved; the high signature bits that used to wrap the payload
    check; a hash count of 2^32 + 7; a wrong magic; more docs than names), each with its code, a NULL handle and
    the path in the message, for classic through xs_bank_open_docs too.  Then the valid file, in the same process:
    its info equals the reference reader's geometry and xs_bank_file_info's, its image the payload, and 50 reads
    give the oracle's hits and k-mer counts at steps 1 and 3."""
    from xspect2_amd import _lib
    kind = {"classic": 0, "compact": 1, "rbloom": 2}[kind_name]
    data, ob, docs = _oracle_file(oracle_mod, kind_name)
    assert len(data) < 16 << 10
    geom = oracle_mod.bank_file_geometry(data, kind_name)
    bad_path = tmp_path / "bad.bank"
    for what, (bad, code) in _corruptions(kind_name, data, geom).items():
        _refused(_lib, oracle_mod, bad_path, kind_name, bad, code, what)
        if kind_name == "classic":
            _refused(_lib, oracle_mod, bad_path, kind_name, bad, code, what + " (docs)", docs=True)
    path = tmp_path / "good.bank"
    path.write_bytes(data)
    finf, foff, fnames = bank_mod.Bank.file_info(path, kind, names=True)
    b = bank_mod.Bank.open(path, kind, device=0, term_size=21 if kind_name == "rbloom" else None)
    try:
        inf = b.info
        for name, _ in inf._fields_:
            if name != "device":
                assert getattr(inf, name) == getattr(finf, name), name
        assert (inf.device, finf.device) == (0, -1)
        assert (inf.term_size, inf.num_hashes, inf.num_docs, inf.num_groups, inf.page_size, foff) == \
            (geom["k"], geom["h"], geom["docs"], geom["groups"], geom["page"], geom["payload_offset"])
        assert [n.encode() for n in b.doc_names] == fnames == geom["names"]
        payload = np.frombuffer(data, dtype=np.uint8)[foff:]
        if kind_name == "rbloom":
            assert inf.bloom_bits == 8 * payload.size and inf.device_bytes == (payload.size + 15) // 16 * 16 + 16
        else:
            assert b.signature_sizes() == geom["sig"] and inf.signature_rows == sum(geom["sig"])
            assert inf.signature_rows * inf.page_size == payload.size  # exact: nothing wrapped
            assert inf.device_bytes == inf.signature_rows * inf.device_row_pitch and inf.device_row_pitch == 16
        assert np.array_equal(b.download(), payload)
        rng = np.random.default_rng(7)
        reads = []
        for i in range(30):  # cut from the docs, and random ones; some shorter than k
            d = docs[int(rng.integers(len(docs)))]
            s = int(rng.integers(0, len(d) - 40))
            reads.append(d[s:s + int(rng.integers(15, 90))])
        reads += [_dna(rng, int(rng.integers(10, 120))) for _ in range(20)]
        assert len(reads) == 50
        for step in (1, 3):
            want, wnk = ob.query([r.encode() for r in reads], step=step)
            got, gnk = b.query(reads, step=step)
            assert np.array_equal(got.reshape(want.shape), want) and np.array_equal(gnk, wnk), step
        assert int(ob.query([r.encode() for r in reads])[0].sum()) > 0
    finally:
        b.close()


def _load_refused(load, json_path, index_path, bad, code):
    """A model load over a corrupt index raises XsError with `code`; with the intact bytes back, it loads."""
    from xspect2_amd import _lib
    good = index_path.read_bytes()
    index_path.write_bytes(bad)
    try:
        with pytest.raises(_lib.XsError) as e:
            load(json_path)
        assert e.value.code == code and str(index_path) in str(e.value)
    finally:
        index_path.write_bytes(good)
    return load(json_path)


def test_model_loads_refuse_corrupt_indices(bank_mod, oracle_mod, tmp_path):
    """ProbabilisticFilterModel.load, ProbabilisticSingleFilterModel.load and the MLST scheme's load over an index
    that was truncated, or whose signature size had the bit flipped that used to wrap the payload check: XsError
    with the format code, no crash, and the next load of the intact model answers as the fitted one."""
    from xspect2_amd import _lib
    from xspect2_amd.file_io import Record, write_fasta
    from xspect2_amd.probabilistic_filter_mlst_model import ProbabilisticFilterMlstSchemeModel
    from xspect2_amd.probabilistic_filter_model import ProbabilisticFilterModel
    from xspect2_amd.probabilistic_single_filter_model import ProbabilisticSingleFilterModel
    F = _lib.XS_ERR_FORMAT
    rng = np.random.default_rng(77)
    base = tmp_path / "xspect_data"
    # species: 64 genomes, so rows of 8 bytes and bits 61..63 of the signature size wrap the product
    sp = tmp_path / "species"
    sp.mkdir()
    genomes = [_dna(rng, 400) for _ in range(64)]
    for i, g in enumerate(genomes):
        write_fasta([Record(f"c{i}", g)], sp / f"GCF_{i:09d}.1_genomic.fna", width=80)
    m = ProbabilisticFilterModel(21, "Test Filter", "J", "j@x", "Species", base)
    m.fit(sp)
    m.save()
    read = genomes[5][100:250]
    want = m.calculate_hits(read)
    index = Path(m.get_cobs_index_path())
    js = base / (m.slug() + ".json")
    data = index.read_bytes()
    geom = oracle_mod.bank_file_geometry(data, "classic")
    assert geom["page"] == 8 and geom["docs"] == 64
    m.index.close()
    for bad in (data[:len(data) // 2], data[:30], _flip(data, 31, 61), _flip(data, 31, 63)):
        with pytest.raises(oracle_mod.BankFileError):
            oracle_mod.bank_file_geometry(bad, "classic")
        loaded = _load_refused(ProbabilisticFilterModel.load, js, index, bad, F)
        assert loaded.calculate_hits(read) == want
        loaded.index.close()
    # genus: an rbloom filter has no signature size; a file cut inside K, or to K alone
    fa = tmp_path / "concatenated_assembly.fna"
    write_fasta([Record("a", genomes[0] + genomes[1])], fa)
    g = ProbabilisticSingleFilterModel(21, "Genus Filter", "J", "j@x", "Genus", base)
    g.fit(fa, "Acinetobacter")
    g.save()
    gwant = g.calculate_hits(genomes[0][10:60])
    gdata = g.bloom_path().read_bytes()
    g.bf.close()
    for bad, code in ((gdata[:5], F), (gdata[:8], F), (_put(gdata, 0, 8, 2**32 + int.from_bytes(gdata[:8], "little")),
                                                     _lib.XS_ERR_UNSUPPORTED)):
        with pytest.raises(oracle_mod.BankFileError):
            oracle_mod.bank_file_geometry(bad, "rbloom")
        loaded = _load_refused(ProbabilisticSingleFilterModel.load, base / (g.slug() + ".json"), g.bloom_path(), bad,
                               code)
        assert loaded.calculate_hits(genomes[0][10:60]) == gwant
        loaded.bf.close()
    # MLST: 2 loci of 40 alleles in 2-byte pages (3 groups): bit 63 of a signature size wraps the product
    root = tmp_path / "alleles"
    for li in range(2):
        locus = _dna(rng, 300 + 20 * li)
        for a in range(1, 41):
            s = list(locus)
            for p in rng.choice(len(s), size=int(rng.integers(1, 9)), replace=False):
                s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
            write_fasta([Record(f"L{li}_{a}", "".join(s))], root / f"Oxf_L{li}" / f"Allele_ID_{a}.fasta")
    s = ProbabilisticFilterMlstSchemeModel(21, "MLST (Oxford)", base, "https://example/schemes/1", "abaumannii")
    s.strain_type_resolver = lambda flat, url: None
    s.fit(root, page_size=2)
    s.save()
    sjs = base / (s.slug() + ".json")
    allele = "".join(rng.choice(list("ACGT"), 310))
    swant = s.calculate_hits(allele)
    lpath = s.get_cobs_index_path("Oxf_L1")  # the second locus: the first one opens before the refusal
    ldata = lpath.read_bytes()
    lgeom = oracle_mod.bank_file_geometry(ldata, "compact")
    assert lgeom["page"] == 2 and lgeom["groups"] == 3
    for bank in s.indices:
        bank.close()
    for bad in (ldata[:len(ldata) // 2], ldata[:40], _flip(ldata, 35 + 16, 63)):
        with pytest.raises(oracle_mod.BankFileError):
            oracle_mod.bank_file_geometry(bad, "compact")
        loaded = _load_refused(ProbabilisticFilterMlstSchemeModel.load, sjs, lpath, bad, F)
        loaded.strain_type_resolver = s.strain_type_resolver
        assert loaded.calculate_hits(allele) == swant
        for bank in loaded.indices:
            bank.close()


def test_a_bank_of_9000_docs_opens_in_slices_only(bank_mod, oracle_mod, tmp_path):
    """A classic index of more docs than one handle takes (8192): xs_bank_file_info reports it as the reference
    reader does, xs_bank_open refuses it as unsupported, and the slices distributed.doc_slice deals out open and
    hold the file's byte columns."""
    from xspect2_amd import _lib
    from xspect2_amd._lib import XS_BANK_COBS_CLASSIC
    from xspect2_amd.distributed import cobs_classic_docs, doc_slice
    D, S = 9000, 257
    rows = np.random.default_rng(12).integers(0, 256, (S, (D + 7) // 8), dtype=np.uint8)
    names = [f"d{i}" for i in range(D)]
    path = tmp_path / "index.cobs_classic"
    path.write_bytes(oracle_mod.cobs_classic_file(names, 21, 7, S, rows))
    assert oracle_mod.bank_file_geometry(path.read_bytes(), "classic")["docs"] == D == cobs_classic_docs(path)
    with pytest.raises(_lib.XsError) as e:
        bank_mod.Bank.open(path, XS_BANK_COBS_CLASSIC, device=0)
    assert e.value.code == _lib.XS_ERR_UNSUPPORTED
    for rank in range(2):
        lo, hi = doc_slice(D, rank, 2)
        sl = bank_mod.Bank.open(path, XS_BANK_COBS_CLASSIC, device=0, docs=(lo, hi))
        try:
            assert sl.num_docs == hi - lo and sl.doc_names == names[lo:hi]
            want = np.ascontiguousarray(rows[:, lo // 8: lo // 8 + (hi - lo + 7) // 8])
            assert np.array_equal(sl.download(), want.reshape(-1)), (lo, hi)
        finally:
            sl.close()
