"""Native FASTA/FASTQ reader (xs_fastx_*) against the pure-Python restatement
of Biopython's parsers (oracle/fastx.py).  CPU only: the reader is host code.

Files are generated with the edge cases Bio.SeqIO meets in practice: text
before the first record, empty records, wrapped lines, CRLF, spaces and tabs
inside sequence lines, headers without descriptions, blank lines between FASTQ
records, '@' and '+' as quality characters, and files large enough that one
batch is split over many threads.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
import fastx as ofx  # noqa: E402  (test-only checker)

from xspect2_amd.file_io import FastxReader, get_record_iterator, read_batches  # noqa: E402


def _pick(rng, alphabet: bytes, n: int) -> bytes:
    return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n).tobytes()


def _fasta_text(rng, n, wrap=True, crlf=False, junk=True) -> bytes:
    out = [b"; leading text the parser skips\n"] if junk else []
    nl = b"\r\n" if crlf else b"\n"
    for i in range(n):
        L = int(rng.integers(0, 400))
        seq = _pick(rng, b"ACGTNacgtn", L)
        desc = [b"", b" some description", b"\tdesc with tab", b"   "][i % 4]
        out.append(b">read_%d%s" % (i, desc) + nl)
        if wrap and L:
            w = int(rng.integers(10, 80))
            for j in range(0, L, w):
                piece = seq[j:j + w]
                if i % 7 == 3:
                    piece = piece[:3] + b" " + piece[3:]  # spaces inside lines are dropped
                out.append(piece + (b"  " if i % 5 == 1 else b"") + nl)
        elif L:
            out.append(seq + nl)
    return b"".join(out)


def _fastq_text(rng, n, crlf=False, blank=False) -> bytes:
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n):
        L = int(rng.integers(0, 300))
        seq = _pick(rng, b"ACGTN", L)
        qual = _pick(rng, b"@+!#ABCDEFGHIJ", L)  # '@' / '+' start quality lines too
        cap = b"read_%d x" % i if i % 3 == 0 else b""
        out.append(b"@read_%d x" % i + nl + seq + nl + b"+" + cap + nl + qual + nl)
        if blank and i % 11 == 0:
            out.append(nl)
    return b"".join(out)


def _wrapped_fastq(rng, n) -> bytes:
    out = []
    for i in range(n):
        L = int(rng.integers(1, 200))
        seq = _pick(rng, b"ACGT", L)
        qual = _pick(rng, b"@+IJ", L)
        w = 60
        out.append(b"@w%d\n" % i + b"\n".join(seq[j:j + w] for j in range(0, L, w)) + b"\n+\n"
                   + b"\n".join(qual[j:j + w] for j in range(0, L, w)) + b"\n")
    return b"".join(out)


def _native(path, max_bytes, threads=0):
    got = []
    with FastxReader(path, threads=threads) as rd:
        for b in rd.batches(max_bytes):
            buf, o = b.packed.buf, b.packed.offsets.tolist()
            raw = buf[:o[-1]].tobytes()
            got += [(i.encode(), raw[o[j]:o[j + 1]]) for j, i in enumerate(b.ids())]
    return got


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("max_bytes", [1, 4096, 1 << 30])
def test_fasta_matches_restatement(tmp_path, crlf, max_bytes):
    rng = np.random.default_rng(7 + crlf)
    p = tmp_path / "x.fasta"
    p.write_bytes(_fasta_text(rng, 3000, crlf=crlf))
    want = ofx.parse_file(p)
    assert _native(p, max_bytes) == want


@pytest.mark.parametrize("max_bytes", [1, 5000, 1 << 30])
def test_fastq_matches_restatement(tmp_path, max_bytes):
    rng = np.random.default_rng(3)
    p = tmp_path / "x.fq"
    p.write_bytes(_fastq_text(rng, 4000, blank=True))
    want = ofx.parse_file(p)
    assert _native(p, max_bytes) == want


def test_multithreaded_split_large_files(tmp_path):
    """> 1 MiB per part: batches are cut into many parts parsed concurrently."""
    rng = np.random.default_rng(11)
    fa = tmp_path / "big.fa"
    fa.write_bytes(_fasta_text(rng, 60_000, junk=False))
    fq = tmp_path / "big.fastq"
    fq.write_bytes(_fastq_text(rng, 60_000, crlf=True))
    assert fa.stat().st_size > 8 << 20 and fq.stat().st_size > 8 << 20
    for p in (fa, fq):
        want = ofx.parse_file(p)
        for threads in (1, 8):
            for mb in (3 << 20, 1 << 30):
                assert _native(p, mb, threads) == want


def test_wrapped_fastq_is_parsed_sequentially(tmp_path):
    p = tmp_path / "w.fastq"
    p.write_bytes(_wrapped_fastq(np.random.default_rng(5), 20_000))
    want = ofx.parse_file(p)
    assert _native(p, 1 << 30, 8) == want
    assert _native(p, 10_000, 8) == want


@pytest.mark.parametrize("text,msg", [
    (b"ACGT\n", "should start with '@'"),
    (b"@a\nACGT\n", "End of file without quality"),
    (b"@a\n", "Unexpected end of file"),
    (b"@a\nACGT\n+b\nIIII\n", "captions differ"),
    (b"@a\nAC GT\n+\nIIIII\n", "Whitespace is not allowed"),
    (b"@a\nACGT\n+\nIII\n", "Lengths of sequence and quality"),
])
def test_fastq_errors_match(tmp_path, text, msg):
    p = tmp_path / "bad.fq"
    p.write_bytes(text)
    with pytest.raises(ValueError, match=msg):
        ofx.parse_file(p)
    with pytest.raises(ValueError, match=msg):
        _native(p, 1 << 30)


def test_empty_and_headerless_files(tmp_path):
    for name, text in [("e.fasta", b""), ("n.fasta", b"no records here\n"), ("e.fq", b""), ("b.fq", b"\n\n")]:
        p = tmp_path / name
        p.write_bytes(text)
        assert _native(p, 1 << 20) == ofx.parse_file(p) == []


def _rows(b):
    o = b.packed.offsets.tolist()
    raw = b.packed.buf[:o[-1]].tobytes()
    return [(i.encode(), raw[o[j]:o[j + 1]]) for j, i in enumerate(b.ids())]


def test_double_buffered_batches_stay_valid(tmp_path):
    """A batch stays intact while the next one is parsed (xs_fastx_next contract)."""
    rng = np.random.default_rng(2)
    p = tmp_path / "d.fasta"
    p.write_bytes(_fasta_text(rng, 2000, junk=False))
    want = ofx.parse_file(p)
    seen = []
    with FastxReader(p) as rd:
        prev = rd.next_batch(20_000)
        while prev.n:
            cur = rd.next_batch(20_000)  # parsed into the other buffer
            seen += _rows(prev)
            prev = cur
    assert seen == want
    # the pipelined generator yields the same records
    assert [r for b in read_batches(p, max_bytes=20_000) for r in _rows(b)] == want


def test_get_record_iterator_contract(tmp_path):
    with pytest.raises(ValueError, match="Path object"):
        get_record_iterator(str(tmp_path))
    with pytest.raises(ValueError, match="does not exist"):
        get_record_iterator(tmp_path / "missing.fasta")
    with pytest.raises(ValueError, match="must be a file"):
        get_record_iterator(tmp_path)
    bad = tmp_path / "x.txt"
    bad.write_text(">a\nAC\n")
    with pytest.raises(ValueError, match="Invalid file format"):
        get_record_iterator(bad)
    ok = tmp_path / "x.fna"
    ok.write_text(">a b\nAC\nGT\n>c\nT\n")
    assert [(r.id, r.seq) for r in get_record_iterator(ok)] == [("a", "ACGT"), ("c", "T")]


def _native_part(path, part, parts, max_bytes=1 << 30, threads=0):
    got = []
    with FastxReader(path, threads=threads, part=part, parts=parts) as rd:
        for b in rd.batches(max_bytes):
            got += _rows(b)
    return got


@pytest.mark.parametrize("kind", ["fasta", "fasta_crlf", "fastq", "fastq_blank", "fastq_wrapped", "tiny"])
def test_byte_range_parts_stitch_to_the_whole_file(tmp_path, kind):
    """xs_fastx_open_range: each rank of a read-sharded job parses only its
    part of the file; the parts, concatenated in part order, are exactly the
    whole file's records (ids and sequences), for 1-9 parts, more parts than
    records, every batch size and thread count."""
    rng = np.random.default_rng(len(kind))
    text = {"fasta": lambda: _fasta_text(rng, 3000),
            "fasta_crlf": lambda: _fasta_text(rng, 2000, crlf=True),
            "fastq": lambda: _fastq_text(rng, 3000),
            "fastq_blank": lambda: _fastq_text(rng, 3000, crlf=True, blank=True),
            "fastq_wrapped": lambda: _wrapped_fastq(rng, 3000),
            "tiny": lambda: b">a\nACGT\n>b\nGG\n"}[kind]()
    p = tmp_path / ("x.fq" if "fastq" in kind else "x.fasta")
    p.write_bytes(text)
    want = ofx.parse_file(p)
    for parts in (1, 2, 3, 5, 9):
        got = [_native_part(p, i, parts, mb, th) for i in range(parts)
               for mb, th in [((1 << 30) if i % 2 else 7000, 1 + i % 3)]]
        assert [r for g in got for r in g] == want, parts
        if len(want) >= 100 and parts > 1:
            sizes = [len(g) for g in got]
            assert min(sizes) > 0 and max(sizes) <= 2 * len(want) / parts + 10  # balanced by bytes
    with pytest.raises(ValueError):
        FastxReader(p, part=3, parts=3)


def test_byte_range_parts_of_a_large_file(tmp_path):
    """Parts larger than 1 MiB are themselves parsed by several threads."""
    rng = np.random.default_rng(17)
    p = tmp_path / "big.fastq"
    p.write_bytes(_fastq_text(rng, 60_000))
    want = ofx.parse_file(p)
    got = [r for i in range(3) for r in _native_part(p, i, 3, 3 << 20, 8)]
    assert got == want


# ---- the forks of the FASTQ record walk (xs_fastx_parse.cpp) ------------------------------
# parse_fastq, the sequential cut point and the wrapped-file detection are written on one
# walk of a record; each case below takes one of its forks and is checked against the
# restatement, whole and in byte-range parts.

def _stitched(p, parts, max_bytes=1 << 30, threads=1):
    return [r for i in range(parts) for r in _native_part(p, i, parts, max_bytes, threads)]


def _fastq_with_empty_records(rng, n, wrapped, quality_line) -> bytes:
    """n records; the first, the last and every 50th have an empty sequence (an empty
    sequence line, then '+'), followed by an empty quality line or by none."""
    out = []
    for i in range(n):
        if i in (0, n - 1) or i % 50 == 25:
            out.append(b"@empty_%d e\n\n+\n" % i + (b"\n" if quality_line else b""))
            continue
        L = int(rng.integers(1, 200))
        seq, qual = _pick(rng, b"ACGTN", L), _pick(rng, b"@+IJ", L)
        w = 60 if wrapped else L
        out.append(b"@r%d x\n" % i + b"\n".join(seq[j:j + w] for j in range(0, L, w)) + b"\n+\n"
                   + b"\n".join(qual[j:j + w] for j in range(0, L, w)) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("quality_line", [True, False])
@pytest.mark.parametrize("wrapped", [False, True])
def test_fastq_records_with_an_empty_sequence(tmp_path, wrapped, quality_line):
    """No quality line is read for an empty sequence: an empty one that follows is a blank
    line before the next record, in four-line and in wrapped files alike."""
    p = tmp_path / "e.fastq"
    p.write_bytes(_fastq_with_empty_records(np.random.default_rng(23), 400, wrapped, quality_line))
    want = ofx.parse_file(p)
    assert len(want) == 400 and want[0] == (b"empty_0", b"") and want[-1] == (b"empty_399", b"")
    assert sum(1 for _, s in want if not s) == 10
    for mb in (1, 3000, 1 << 30):
        assert _native(p, mb, 1) == want
    for parts in (2, 3, 7):
        assert _stitched(p, parts, 3000 if parts == 3 else 1 << 30) == want, parts


def _wrapped_fastq_hard(rng, n, blank) -> bytes:
    """Wrapped records whose every quality line begins with '@' or '+' (what a cut by
    pattern would take for a header or a '+' line), with blank lines between records."""
    out = []
    for i in range(n):
        L = int(rng.integers(61, 300))
        seq, qual = _pick(rng, b"ACGT", L), bytearray(_pick(rng, b"@+IJ", L))
        for j in range(0, L, 60):
            qual[j] = b"@+"[(i + j // 60) % 2]
        out.append(b"@w%d\n" % i + b"\n".join(seq[j:j + 60] for j in range(0, L, 60)) + b"\n+w%d\n" % i
                   + b"\n".join(bytes(qual[j:j + 60]) for j in range(0, L, 60)) + b"\n")
        if blank and i % 3 == 0:
            out.append(b"\n" * (1 + i % 2) if i % 2 else b" \r\n")
    return b"".join(out)


@pytest.mark.parametrize("blank", [False, True])
def test_wrapped_fastq_quality_lines_that_look_like_headers(tmp_path, blank):
    p = tmp_path / "w.fastq"
    p.write_bytes(_wrapped_fastq_hard(np.random.default_rng(29 + blank), 300, blank))
    want = ofx.parse_file(p)
    assert len(want) == 300
    assert _native(p, 1 << 30, 1) == want and _native(p, 2000, 8) == want
    for parts in (2, 3, 7):
        assert _stitched(p, parts, 2000 if parts == 3 else 1 << 30, 1 + parts % 3) == want, parts


def test_wrapped_fastq_malformed_record_in_a_middle_part(tmp_path):
    """A quality shorter than its sequence in the middle of a wrapped file opened in three
    parts: the part before it yields its records, the part that holds it yields the batches
    before its and then raises the host reader's error, and every part does what the
    restatement does on the same bytes."""
    rng = np.random.default_rng(31)
    good = _wrapped_fastq(rng, 150)
    bad = b"@short\n" + b"ACGT" * 40 + b"\n+\n" + b"I" * 100 + b"\n"  # then '@w..' lines read as quality
    p = tmp_path / "m.fastq"
    data = good + bad + _wrapped_fastq(rng, 150)
    p.write_bytes(data)
    with pytest.raises(ValueError, match="Lengths of sequence and quality"):
        ofx.parse_file(p)
    # each part's byte range, as its batches report it (text_bytes = the part's end)
    ends = []
    for part in range(2):
        with FastxReader(p, threads=1, part=part, parts=3) as rd:
            ends.append(rd.next_batch(1000).text_bytes)
    assert 0 < ends[0] < len(good) < ends[1] < len(data)
    cuts = [0] + ends + [len(data)]
    assert _native_part(p, 0, 3) == ofx.parse_fastq(data[:cuts[1]]) and len(_native_part(p, 0, 3)) > 50
    before = []
    with pytest.raises(ValueError, match=r"Lengths of sequence and quality values differs \(160 and \d+\)"):
        with FastxReader(p, threads=1, part=1, parts=3) as rd:
            for b in rd.batches(1000):
                before += _rows(b)
    # the batch that holds the malformed record is lost with it: a window of 1,000 bytes
    # and the record that crosses its end (a sequence is shorter than 200)
    held = ofx.parse_fastq(data[cuts[1]:len(good)])
    assert len(before) > 10 and before == held[:len(before)]
    assert sum(len(s) for _, s in held[len(before):]) < 1000 + 200
    with pytest.raises(ValueError, match="Lengths of sequence and quality"):
        ofx.parse_fastq(data[cuts[1]:cuts[2]])
    try:
        want_last = ofx.parse_fastq(data[cuts[2]:])
    except ValueError:
        with pytest.raises(ValueError):
            _native_part(p, 2, 3)
    else:
        assert _native_part(p, 2, 3) == want_last


def test_fastq_wrapped_only_after_the_detection_window(tmp_path):
    """The wrapped-file detection looks at the first 1,000 records (or 1 MiB).  A file
    whose first 1,000 records have four lines and whose record 1,001 is wrapped counts as
    a four-line file; read whole by one thread it is still parsed by the record rules and
    yields the restatement's records."""
    rng = np.random.default_rng(37)
    p = tmp_path / "late.fastq"
    p.write_bytes(_fastq_text(rng, 1000) + _wrapped_fastq(rng, 200))
    assert p.stat().st_size < 1 << 20
    want = ofx.parse_file(p)
    assert len(want) == 1200
    assert _native(p, 1 << 30, 1) == want
    assert _stitched(p, 1, 1 << 30, 1) == want
