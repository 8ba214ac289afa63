"""Bank file headers (xs_bank_file_info, xs_bank_open, xs_bank_open_docs; no GPU).

Every refusal of a bank file happens on the host, before the first HIP call,
so the header reader is tested here without a device.  Valid files come from
the oracle's spec writers only (never from xs_bank_save); each is mutated
three ways (every truncation length, every single-bit flip of the header,
every numeric field set to a list of edge values) and the library's outcome on
every mutation is compared with oracle.bank_file_geometry, a reader of the
same layouts in Python integers that shares no code with the library: the
same class of refusal, or XS_OK with equal geometry and names.

What the sweeps pinned when they were written: a flipped high bit of a
signature size used to leave sum(sig) * page unchanged modulo 2^64 whenever
the page size is a power of two, and the file opened with rows far outside
its image; num_hashes and rbloom's K were cut to 32 bits before their range
check; the names loop ran num_docs times whatever the file held.
"""
from __future__ import annotations

import ctypes
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
KIND = {"classic": 0, "compact": 1, "rbloom": 2}


def _pitch(page: int) -> int:
    """Device bytes per row: 16, 32, 64 or a multiple of 128 (Bank image)."""
    p16 = (page + 15) // 16 * 16
    return (16 if p16 <= 16 else 32 if p16 <= 32 else 64) if p16 <= 64 else (p16 + 127) // 128 * 128


def _classic(oracle, docs, sig, seed):
    rows = np.random.default_rng(seed).integers(0, 256, (sig, (docs + 7) // 8), dtype=np.uint8)
    data = oracle.cobs_classic_file([f"d{i}" for i in range(docs)], 21, 7, sig, rows)
    fields = {"version": (18, 4), "num_docs": (22, 4), "term_size": (26, 4), "canonicalize": (30, 1),
              "sig0": (31, 8), "num_hashes0": (39, 8)}
    return data, fields


def _compact(oracle, docs, sig, page, seed):
    rows = np.random.default_rng(seed).integers(0, 256, (sum(sig), page), dtype=np.uint8)
    data = oracle.cobs_compact_file([f"a{i}" for i in range(docs)], 31, 3, sig, page, rows)
    G = len(sig)
    fields = {"version": (18, 4), "term_size": (22, 4), "canonicalize": (26, 1), "num_groups": (27, 8),
              "page_size": (35 + 16 * G, 8), "num_docs": (43 + 16 * G, 4)}
    for g in range(G):
        fields[f"sig{g}"] = (35 + 16 * g, 8)
        fields[f"num_hashes{g}"] = (43 + 16 * g, 8)
    return data, fields


class Case:
    """One valid file: its bytes, its numeric fields {name: (offset, width)} and the header bytes swept by bit."""

    def __init__(self, name, kind, data, fields, flip_bytes=None):
        self.name, self.kind, self.data, self.fields = name, kind, data, fields
        import oracle
        self.geom = oracle.bank_file_geometry(data, kind)
        self.header = self.geom["payload_offset"]
        self.flip_bytes = list(range(self.header)) if flip_bytes is None else flip_bytes


@pytest.fixture(scope="module")
def cases(oracle_mod):
    o = oracle_mod
    out = [Case("classic64", "classic", *_classic(o, 64, 257, 1)),      # page 8: a power of two
           Case("classic100", "classic", *_classic(o, 100, 101, 2)),    # page 13
           Case("compact8", "compact", *_compact(o, 150, [37, 11, 23], 8, 3))]
    data, fields = _compact(o, 1430, [5, 3, 4], 64, 4)                  # an MLST locus' 64-byte pages
    numeric = sorted(b for off, w in fields.values() for b in range(off, off + w))
    out.append(Case("compact64", "compact", data, fields, flip_bytes=numeric))  # its 5.6 KB of names are not swept
    bits = np.random.default_rng(5).integers(0, 256, 1000, dtype=np.uint8)
    out.append(Case("rbloom", "rbloom", o.rbloom_file(7, bits), {"K": (0, 8)}))
    for c in out:
        assert len(c.flip_bytes) < 1024, c.name
    return {c.name: c for c in out}


NAMES = ["classic64", "classic100", "compact8", "compact64", "rbloom"]


class Checker:
    """Runs one mutated file through the reference reader and the library and compares them."""

    def __init__(self, tmp_path):
        from xspect2_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.path = tmp_path / "mutated.bank"
        self.accepted = self.refused = 0

    def library(self, data: bytes, kind: str):
        """(rc, BankInfo, payload offset) of xs_bank_file_info on a file of these bytes."""
        self.path.write_bytes(data)
        inf, off = self._lib.BankInfo(), ctypes.c_uint64(0)
        rc = self.lib.xs_bank_file_info(str(self.path).encode(), KIND[kind], ctypes.byref(inf), ctypes.byref(off))
        return rc, inf, off.value

    def check(self, data: bytes, kind: str, what) -> bool:
        """True: both accept the file; False: both refuse it with the same class.  Anything else fails."""
        import oracle
        from xspect2_amd.bank import Bank
        _lib = self._lib
        try:
            want = oracle.bank_file_geometry(data, kind)
        except oracle.BankFileError as e:
            want = e
        rc, inf, off = self.library(data, kind)
        if isinstance(want, oracle.BankFileError):
            code = {"format": _lib.XS_ERR_FORMAT, "unsupported": _lib.XS_ERR_UNSUPPORTED}[want.kind]
            assert rc == code, (what, rc, str(want), self.lib.xs_last_error())
            assert str(self.path).encode() in self.lib.xs_last_error(), what
            # the opens refuse the same file with the same code, before any HIP call, and hand out no handle
            h = ctypes.c_void_p(0xDEAD)
            assert self.lib.xs_bank_open(str(self.path).encode(), KIND[kind], 0, ctypes.byref(h)) == code, what
            assert h.value is None, what
            if kind == "classic":
                h = ctypes.c_void_p(0xDEAD)
                assert self.lib.xs_bank_open_docs(str(self.path).encode(), 0, 0, 8, ctypes.byref(h)) == code, what
                assert h.value is None, what
            self.refused += 1
            return False
        assert rc == _lib.XS_OK, (what, rc, self.lib.xs_last_error(), want)
        rows = sum(want["sig"])
        got = {"k": inf.term_size, "h": inf.num_hashes, "docs": inf.num_docs, "groups": inf.num_groups,
               "page": inf.page_size, "rows": inf.signature_rows, "payload_offset": off,
               "canonicalize": inf.canonicalize, "device": inf.device, "kind": inf.kind}
        exp = {"k": want["k"], "h": want["h"], "docs": want["docs"], "groups": want["groups"], "page": want["page"],
               "rows": rows, "payload_offset": want["payload_offset"], "canonicalize": 1, "device": -1,
               "kind": KIND[kind]}
        assert got == exp, what
        if kind == "rbloom":
            nbytes = len(data) - 8
            assert (inf.bloom_bits, inf.device_bytes, inf.device_row_pitch) == \
                (8 * nbytes, (nbytes + 15) // 16 * 16 + 16, 0), what
        else:
            pitch = _pitch(want["page"])
            assert (inf.bloom_bits, inf.device_bytes, inf.device_row_pitch) == (0, rows * pitch, pitch), what
            assert rows * want["page"] == len(data) - off, what  # exact, in unbounded integers
        assert Bank.file_info(self.path, KIND[kind], names=True)[2] == want["names"], what
        self.accepted += 1
        return True


def _set(data: bytes, off: int, width: int, value: int) -> bytes:
    return data[:off] + value.to_bytes(width, "little") + data[off + width:]


def _get(data: bytes, off: int, width: int) -> int:
    return int.from_bytes(data[off:off + width], "little")


@pytest.mark.parametrize("name", NAMES)
def test_every_truncation_matches_the_reference_reader(cases, tmp_path, name):
    """The file cut at every length from 0 to its own: only the whole COBS file opens.  An rbloom file carries
    no length, so every cut that leaves K and one filter byte is a smaller filter."""
    c, ck = cases[name], Checker(tmp_path)
    for n in range(len(c.data) + 1):
        whole = n > 8 if c.kind == "rbloom" else n == len(c.data)
        assert ck.check(c.data[:n], c.kind, (name, "cut at", n)) == whole, (name, n)
    assert ck.accepted == (len(c.data) - 8 if c.kind == "rbloom" else 1) and ck.accepted + ck.refused == len(c.data) + 1


def _must_refuse(c: Case, byte: int) -> bool:
    """Flips in a magic, the version, num_docs, a signature size, the group count or the page size can never
    give a valid file: a check of the reference reader itself."""
    if c.kind == "rbloom":
        return False
    trailer = c.data.rindex(b"_INDEX", 0, c.header) - 7  # "CLASSIC_INDEX" / "COMPACT_INDEX" before the padding
    if byte < 18 or trailer <= byte < trailer + 13:
        return True  # the magic and the trailer
    return any(off <= byte < off + w for f, (off, w) in c.fields.items()
               if f in ("version", "num_docs", "num_groups", "page_size") or f.startswith("sig"))


@pytest.mark.parametrize("name", NAMES)
def test_every_header_bit_flip_matches_the_reference_reader(cases, tmp_path, name):
    c, ck = cases[name], Checker(tmp_path)
    buf = bytearray(c.data)
    for byte in c.flip_bytes:
        for bit in range(8):
            buf[byte] ^= 1 << bit
            ok = ck.check(bytes(buf), c.kind, (name, "flip", byte, bit))
            buf[byte] ^= 1 << bit
            assert not (ok and _must_refuse(c, byte)), (name, byte, bit)
    assert ck.accepted + ck.refused == 8 * len(c.flip_bytes)
    assert ck.accepted > 0 and ck.refused > 0, (name, ck.accepted, ck.refused)


@pytest.mark.parametrize("name", NAMES)
def test_every_numeric_field_at_its_edges_matches_the_reference_reader(cases, tmp_path, name):
    c, ck = cases[name], Checker(tmp_path)
    for field, (off, w) in c.fields.items():
        v = _get(c.data, off, w)
        for value in (0, 1, v - 1, v + 1, 2**31, 2**32 - 1, 2**32 + v, 2**61 + v, 2**63, 2**64 - 1):
            if 0 <= value < 1 << 8 * w:  # as far as the field is wide
                ck.check(_set(c.data, off, w, value), c.kind, (name, field, value))
    assert ck.accepted > 0 and ck.refused > 0, (name, ck.accepted, ck.refused)


def test_the_wraps_the_old_reader_accepted_are_refused(cases, tmp_path):
    """The cases by name: sum(sig) * page unchanged modulo 2^64 (bits 61..63 of a signature size at page 8, bits
    58..63 at page 64), and a hash count of 2^32 + its value."""
    from xspect2_amd import _lib
    ck = Checker(tmp_path)
    for name, bits in (("classic64", (61, 62, 63)), ("compact8", (61, 62, 63)), ("compact64", range(58, 64))):
        c = cases[name]
        for field, (off, w) in c.fields.items():
            if field.startswith("sig"):
                for bit in bits:
                    data = _set(c.data, off, w, _get(c.data, off, w) ^ 1 << bit)
                    assert ck.library(data, c.kind)[0] == _lib.XS_ERR_FORMAT, (name, field, bit)
                    assert not ck.check(data, c.kind, (name, field, bit))
    for name in NAMES:
        c = cases[name]
        data = c.data
        for field, (off, w) in c.fields.items():
            if field.startswith("num_hashes") or field == "K":
                data = _set(data, off, w, 2**32 + _get(c.data, off, w))  # every group's: not "mixed"
        assert ck.library(data, c.kind)[0] == _lib.XS_ERR_UNSUPPORTED, name
        assert not ck.check(data, c.kind, (name, "hashes + 2^32"))


def test_kept_refusals(cases, tmp_path):
    """The refusals from before the header unit, each by name and code."""
    from xspect2_amd import _lib
    F, U = _lib.XS_ERR_FORMAT, _lib.XS_ERR_UNSUPPORTED
    ck = Checker(tmp_path)
    c, k = cases["classic100"], cases["compact8"]

    def expect(case, data, code, what):
        assert ck.library(data, case.kind)[0] == code, (what, ck.lib.xs_last_error())
        assert not ck.check(data, case.kind, what)

    def field(case, name, value):
        return _set(case.data, *case.fields[name], value)

    for case in (c, k):
        expect(case, field(case, "version", 2), F, "version 2")
        expect(case, field(case, "version", 0), F, "version 0")
        expect(case, b"COBZ:" + case.data[5:], F, "bad magic")
        expect(case, field(case, "num_docs", 0), F, "zero docs")
        expect(case, field(case, "sig0", 0), F, "zero signature size")
        expect(case, field(case, "term_size", 0), U, "term_size 0")
        expect(case, field(case, "term_size", 33), U, "term_size 33")
        expect(case, field(case, "canonicalize", 0), U, "canonicalize 0")
        expect(case, field(case, "num_hashes0", 17) if case is c else
               _set(_set(field(case, "num_hashes0", 17), *case.fields["num_hashes1"], 17),
                    *case.fields["num_hashes2"], 17), U, "num_hashes 17")
        expect(case, case.data + b"\0", F, "payload one byte long")
        expect(case, case.data[:-1], F, "payload one byte short")
        trailer = case.data.rindex(b"_INDEX", 0, case.header)
        expect(case, case.data[:trailer] + b"_INDEY" + case.data[trailer + 6:], F, "bad trailer")
    expect(k, field(k, "num_hashes1", 4), F, "mixed num_hashes")
    expect(k, field(k, "page_size", 0), F, "zero page size")
    expect(k, field(k, "num_groups", 2), F, "groups do not cover the docs")
    expect(k, field(k, "num_groups", 0), F, "zero groups")
    r = cases["rbloom"]
    expect(r, r.data[:8], F, "rbloom without filter bytes")
    expect(r, _set(r.data, 0, 8, 0), U, "K = 0")
    expect(r, _set(r.data, 0, 8, 17), U, "K = 17")


def test_file_info_is_what_the_python_side_reports(cases, tmp_path):
    """Bank.file_info and distributed.cobs_classic_docs (which keeps its ValueError contract) on the valid files."""
    from xspect2_amd import _lib
    from xspect2_amd.bank import Bank
    from xspect2_amd.distributed import cobs_classic_docs
    p = tmp_path / "index.cobs_classic"
    p.write_bytes(cases["classic100"].data)
    inf, off = Bank.file_info(p, _lib.XS_BANK_COBS_CLASSIC)
    assert (inf.num_docs, inf.page_size, inf.signature_rows, inf.device_row_pitch, inf.device_bytes, inf.device) == \
        (100, 13, 101, 16, 101 * 16, -1)
    assert off == cases["classic100"].header
    assert cobs_classic_docs(p) == 100
    for bad in (cases["classic100"].data[:40], cases["compact8"].data, b""):
        p.write_bytes(bad)
        with pytest.raises(ValueError):
            cobs_classic_docs(p)
    with pytest.raises(_lib.XsError) as e:
        Bank.file_info(tmp_path / "missing", _lib.XS_BANK_RBLOOM)
    assert e.value.code == _lib.XS_ERR_IO
    inf = _lib.BankInfo()
    assert _lib.load().xs_bank_file_info(str(p).encode(), 7, ctypes.byref(inf), None) == _lib.XS_ERR_ARG
    assert _lib.load().xs_bank_file_info(None, 0, ctypes.byref(inf), None) == _lib.XS_ERR_ARG


def test_a_bank_of_more_docs_than_one_handle_takes_is_read_and_opens_in_slices(oracle_mod, tmp_path):
    """A classic index of 9000 docs: a valid file that one handle cannot hold (the probe's LDS counters take 8192
    docs).  xs_bank_file_info and distributed.cobs_classic_docs report it, as the reference reader does, because
    the column split (load_docs_slice) takes its doc count from there; xs_bank_open refuses it as unsupported
    before any HIP call; xs_bank_open_docs passes every header check for a slice that fits (without a GPU it then
    fails in HIP, with one it opens) and refuses a slice that does not."""
    from xspect2_amd import _lib
    from xspect2_amd.bank import Bank
    from xspect2_amd.distributed import cobs_classic_docs, doc_slice
    D, S = 9000, 3
    rows = np.random.default_rng(6).integers(0, 256, (S, (D + 7) // 8), dtype=np.uint8)
    data = oracle_mod.cobs_classic_file([f"d{i}" for i in range(D)], 21, 7, S, rows)
    want = oracle_mod.bank_file_geometry(data, "classic")
    assert want["docs"] == D
    p = tmp_path / "index.cobs_classic"
    p.write_bytes(data)
    inf, off, names = Bank.file_info(p, _lib.XS_BANK_COBS_CLASSIC, names=True)
    assert (inf.num_docs, inf.page_size, inf.signature_rows, off, names) == \
        (D, want["page"], S, want["payload_offset"], want["names"])
    assert (inf.device_row_pitch, inf.device_bytes) == (_pitch(1125), S * _pitch(1125))
    assert cobs_classic_docs(p) == D
    assert doc_slice(cobs_classic_docs(p), 1, 2) == (4496, 9000)
    lib = _lib.load()
    h = ctypes.c_void_p(0xDEAD)
    assert lib.xs_bank_open(str(p).encode(), 0, 0, ctypes.byref(h)) == _lib.XS_ERR_UNSUPPORTED
    assert h.value is None and b"LDS counter budget" in lib.xs_last_error()
    h = ctypes.c_void_p(0xDEAD)
    assert lib.xs_bank_open_docs(str(p).encode(), 0, 0, D, ctypes.byref(h)) == _lib.XS_ERR_UNSUPPORTED  # the whole
    assert h.value is None
    h = ctypes.c_void_p(0xDEAD)
    rc = lib.xs_bank_open_docs(str(p).encode(), 0, 0, 4096, ctypes.byref(h))
    if rc == _lib.XS_OK:
        lib.xs_bank_close(h)
    else:  # no refusal of the file: the call got as far as the device
        assert rc == _lib.XS_ERR_HIP and h.value is None, (rc, lib.xs_last_error())


_NAMES_LOOP_CHILD = r"""
import ctypes, resource, sys
sys.path.insert(0, sys.argv[1])
resource.setrlimit(resource.RLIMIT_DATA, (8 << 30, 8 << 30))
from xspect2_amd import _lib
lib = _lib.load()
before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
codes = []
for path, kind in ((sys.argv[2], 0), (sys.argv[3], 1)):
    h = ctypes.c_void_p(0xDEAD)
    codes.append(lib.xs_bank_open(path.encode(), kind, 0, ctypes.byref(h)))
    assert h.value is None
    inf = _lib.BankInfo()
    codes.append(lib.xs_bank_file_info(path.encode(), kind, ctypes.byref(inf), None))
h = ctypes.c_void_p(0xDEAD)
codes.append(lib.xs_bank_open_docs(sys.argv[2].encode(), 0, 0, 8, ctypes.byref(h)))
assert h.value is None
grown = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before
print("codes", *codes, "grown_kib", grown)
"""


def test_a_header_that_claims_four_billion_names_is_refused_at_once(tmp_path):
    """A 47-byte classic header (and the compact one) with num_docs = 0xFFFFFFFF: XS_ERR_FORMAT with work and memory
    in proportion to the file, not to the claim.  The reader used to run its names loop num_docs times on a failed
    stream: 1.4 s and 991 MiB for 20,000,000 names.  64 MiB is a cap, not a measurement (refused opens of ordinary
    files grow the process by 0..1 MiB); the child's RLIMIT_DATA and the timeout make a regression fail fast."""
    from xspect2_amd import _lib
    classic = b"COBS:CLASSIC_INDEX" + struct.pack("<IIIBQQ", 1, 0xFFFFFFFF, 21, 1, 257, 7)
    assert len(classic) == 47
    compact = b"COBS:COMPACT_INDEX" + struct.pack("<IIBQQQQI", 1, 21, 1, 1, 257, 7, 1 << 29, 0xFFFFFFFF)
    (tmp_path / "c.cobs_classic").write_bytes(classic)
    (tmp_path / "c.cobs_compact").write_bytes(compact)
    res = subprocess.run([sys.executable, "-c", _NAMES_LOOP_CHILD, str(ROOT), str(tmp_path / "c.cobs_classic"),
                          str(tmp_path / "c.cobs_compact")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    words = res.stdout.split()
    assert [int(x) for x in words[1:6]] == [_lib.XS_ERR_FORMAT] * 5, res.stdout
    assert int(words[-1]) <= 64 << 10, res.stdout  # ru_maxrss is in KiB


def _create_cobs(kind, k, h, docs, page, groups, sig, names=None):
    from xspect2_amd import _lib
    sig_arr = (ctypes.c_uint64 * max(1, len(sig)))(*sig)
    h_out = ctypes.c_void_p(0xDEAD)
    rc = _lib.load().xs_bank_create_cobs(0, kind, k, h, docs, page, groups, ctypes.cast(sig_arr, ctypes.c_void_p),
                                         ctypes.cast(names, ctypes.c_void_p) if names is not None else None,
                                         ctypes.byref(h_out))
    assert h_out.value is None
    return rc


def test_create_cobs_refuses_what_does_not_multiply_out():
    """xs_bank_create_cobs checks its geometry without wrapping, before it reads sig's num_groups entries or the
    names, and before any HIP call: sizes beyond 64 bits are XS_ERR_ARG, k and h out of range XS_ERR_UNSUPPORTED,
    and *out stays NULL.  sig holds one or three entries whatever num_groups claims."""
    from xspect2_amd import _lib
    A, U, F = _lib.XS_ERR_ARG, _lib.XS_ERR_UNSUPPORTED, _lib.XS_ERR_FORMAT
    # sum(sig) * page: 2^61 * 8, and the image's sum(sig) * pitch alone: 2^60 * 16 (page 8, pitch 16)
    assert _create_cobs(0, 21, 7, 64, 8, 1, [2**61]) == A
    assert _create_cobs(0, 21, 7, 64, 8, 1, [2**60]) == A
    assert _create_cobs(0, 21, 7, 64, 8, 1, [257 + 2**61]) == A
    assert _create_cobs(1, 31, 3, 150, 8, 3, [2**63, 2**63, 5]) == A        # sum(sig)
    assert _create_cobs(1, 31, 3, 1430, 64, 3, [2**58, 3, 4]) == A          # sum(sig) * 64
    # G * 8 * page: num_groups 2^61 (sig has 3 entries: they must not be read), page 2^61, both
    assert _create_cobs(1, 31, 3, 150, 8, 2**61, [5, 3, 4]) == A
    assert _create_cobs(1, 31, 3, 150, 2**61, 3, [5, 3, 4]) == A
    assert _create_cobs(1, 31, 3, 150, 2**32, 2**32, [5, 3, 4]) == A
    assert _create_cobs(1, 31, 3, 150, 2**64 - 1, 2**64 - 1, [5, 3, 4]) == A
    # groups that fit 64 bits and do not cover the docs, docs the classic rule's (D + 7) / 8 would wrap on
    assert _create_cobs(1, 31, 3, 150, 8, 2**40, [5, 3, 4]) == F
    assert _create_cobs(0, 21, 7, 2**64 - 1, 0, 1, [5]) == A
    assert _create_cobs(0, 21, 7, 2**64 - 1, 2**61, 1, [5]) == A            # 8 * page
    assert _create_cobs(0, 21, 7, 2**61, 2**58, 1, [5]) == U                # more docs than the LDS counters hold
    # a NULL name among the names
    names = (ctypes.c_char_p * 64)(*[b"d%d" % i for i in range(64)])
    names[63] = None
    assert _create_cobs(0, 21, 7, 64, 8, 1, [257], names) == A
    assert b"doc_names[63]" in _lib.load().xs_last_error()
    for h in (0, 17):
        assert _create_cobs(0, 21, h, 64, 8, 1, [257]) == U
    for k in (0, 33):
        assert _create_cobs(0, k, 7, 64, 8, 1, [257]) == U
    assert _create_cobs(0, 21, 7, 0, 0, 1, [257]) == F                       # no documents, as before
    assert _create_cobs(0, 21, 7, 64, 8, 1, [0]) == F                        # zero signature size, as before


def test_create_bloom_refuses_bad_arguments():
    from xspect2_amd import _lib

    def create(k, nbytes, K):
        h = ctypes.c_void_p(0xDEAD)
        rc = _lib.load().xs_bank_create_bloom(0, k, nbytes, K, ctypes.byref(h))
        assert h.value is None
        return rc

    for K in (0, 17):
        assert create(21, 1000, K) == _lib.XS_ERR_UNSUPPORTED
    for k in (0, 33):
        assert create(k, 1000, 7) == _lib.XS_ERR_UNSUPPORTED
    for nbytes in (2**61, 2**64 - 1, 2**64 - 16):  # the bit count, the padded image
        assert create(21, nbytes, 7) == _lib.XS_ERR_ARG
    assert create(21, 0, 7) == _lib.XS_ERR_FORMAT  # an empty filter, as before
