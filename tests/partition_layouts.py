"""Read layouts that put read boundaries on the partitioned probes' edges.

Helper of tests/test_partition_layouts.py, tests/test_output_buffer_checker.py
and tests/test_large_extents_host.py (CPU), tests/test_gpu_partitioned_edges.py,
tests/test_gpu_output_buffers.py and tests/test_gpu_large_extents.py (GPU); it
needs no GPU and no library.

The partitioned probes (xs_probe_cobspart.hip, xs_probe_bloompart.hip) give
every sampled k-mer of a call a global id and work on bucket blocks of T
consecutive ids (T = kCobsCK for COBS, kPartKmers for rbloom).  Which code a
block runs depends on the reads it touches:

    blk_read[b] = the read holding k-mer b*T
    lo = blk_read[B]
    hi = blk_read[B+1] if (B+1)*T < Nk else n-1

`hi - lo + 1` against cnt_reads (LDS counters or global atomics in the COBS
resolve pass), `hi - lo + 2` against kStageReads (read offsets staged in LDS
or a global binary search per k-mer in both bucket passes), and whether a
read's k-mers lie in one block (its row stored) or two (zeroed beforehand,
added atomically by each).  This module restates that rule in numpy, reads
the constants from the shipped sources (a change of block size moves the
layouts with it), and names layouts, lists of per-read k-mer counts, built
to land on each of those edges.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parents[1] / "xspect2_amd" / "csrc"


# ---------------------------------------------------------------- constants
def _src(name: str) -> str:
    return (CSRC / name).read_text()


def _const(file: str, name: str) -> int:
    """`constexpr <type> name = <int>[u] [<< <int>];` of a shipped source."""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)u?(?:\s*<<\s*(\d+))?\s*;", _src(file))
    assert m, f"{file}: constant {name} not found"
    return int(m.group(1)) << int(m.group(2) or 0)


def _cnt_reads_div() -> int:
    m = re.search(r"cnt_reads\(\)\s*\{\s*return\s+CK\s*/\s*(\d+)\s*;", _src("xs_probe_cobspart.hip"))
    assert m, "xs_probe_cobspart.hip: cnt_reads() is no longer CK / <int>"
    return int(m.group(1))


def _id_bits(ck: int) -> int:
    m = re.search(r"id_bits\(\)\s*\{\s*return\s+([^;]*);", _src("xs_probe_cobspart.hip"))
    assert m, "xs_probe_cobspart.hip: id_bits() not found"
    expr = m.group(1)
    pairs = re.findall(r"CK\s*==\s*(\d+)\s*\?\s*(\d+)", expr)
    last = re.search(r":\s*(\d+)\s*$", expr)
    assert pairs and last, f"xs_probe_cobspart.hip: id_bits() has another form: {expr!r}"
    for size, bits in pairs:
        if int(size) == ck:
            return int(bits)
    return int(last.group(1))


def _emb_base() -> int:
    m = re.search(r"emb_max_docs\(\)\s*\{\s*return\s+(\d+)\s*-\s*id_bits<CK>\(\)\s*;", _src("xs_probe_cobspart.hip"))
    assert m, "xs_probe_cobspart.hip: emb_max_docs() is no longer <int> - id_bits<CK>()"
    return int(m.group(1))


COBS_CK = _const("xs_probe_cobspart.hip", "kCobsCK")       # k-mers per COBS bucket block
PART_KMERS = _const("xs_internal.h", "kPartKmers")         # k-mers per rbloom bucket block
STAGE_READS = _const("xs_part.h", "kStageReads")           # read offsets a bucket block stages in LDS
SEG_KMERS = _const("xs_internal.h", "kSegKmers")           # k-mers per work unit (rbloom count pass)
COBS_PAD_PARTS = _const("xs_internal.h", "kCobsPadParts")  # partitions up to which runs are padded
PART_MAX = _const("xs_internal.h", "kPartMax")             # partitions of a plan at the most
HOST_FIRST = _const("xs_query.cpp", "kHostFirst")          # sequence bytes of a host batch's first chunk
CNT_DIV = _cnt_reads_div()
ID_BITS = _id_bits(COBS_CK)
EMB_MAX_DOCS = _emb_base() - ID_BITS                       # docs up to which the k-mer id rides in the row


def cnt_reads(T: int) -> int:
    """Reads per block with LDS counter rows (cnt_reads<CK>())."""
    return T // CNT_DIV


# ---------------------------------------------------------------- the rule
def num_kmers(length: int, k: int, step: int) -> int:
    return max(0, -(-(length - k + 1) // step))


def kofs(counts) -> np.ndarray:
    """First global k-mer id of every read, and the total (n + 1 entries)."""
    out = np.zeros(len(counts) + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.asarray(counts, dtype=np.int64))
    return out


def blk_read(counts, T: int) -> np.ndarray:
    """blk_read[b] = the read holding k-mer b*T, for every block with a k-mer."""
    ko = kofs(counts)
    nb = -(-int(ko[-1]) // T)
    return np.searchsorted(ko, np.arange(nb, dtype=np.int64) * T, side="right") - 1


def block_reads(counts, T: int, B: int) -> tuple[int, int]:
    """(lo, hi) of bucket block B."""
    br = blk_read(counts, T)
    Nk = int(kofs(counts)[-1])
    assert 0 <= B < len(br)
    return int(br[B]), int(br[B + 1]) if (B + 1) * T < Nk else len(counts) - 1


def block_table(counts, T: int) -> list[tuple[int, int]]:
    return [block_reads(counts, T, B) for B in range(len(blk_read(counts, T)))]


def read_classes(counts, T: int) -> list[str]:
    """What the COBS resolve pass does with every read's hit row:
    "empty" (no k-mers: zeroed), "stored" (all k-mers in one block whose reads
    fit the LDS counters: stored once, never zeroed) or "added" (k-mers in two
    blocks or more, or in a block with more reads than counter rows: zeroed,
    then added atomically)."""
    ko = kofs(counts)
    tab = block_table(counts, T)
    out = []
    for r, c in enumerate(counts):
        if c == 0:
            out.append("empty")
            continue
        b0, b1 = int(ko[r]) // T, (int(ko[r + 1]) - 1) // T
        lo, hi = tab[b0]
        out.append("added" if b0 != b1 or hi - lo + 1 > cnt_reads(T) else "stored")
    return out


# ---------------------------------------------------------------- layouts
def _split(T: int, reads: int) -> list[int]:
    """`reads` k-mer-holding reads that fill one block exactly: equal counts,
    the remainder added to the last ones (2048 over 254 reads: 252 x 8 + 2 x 16)."""
    base = T // reads
    assert base >= 1
    out = [base] * reads
    extra, i = T - base * reads, reads - 1
    while extra > 0:
        add = min(base, extra)
        out[i] += add
        extra -= add
        i -= 1
    assert sum(out) == T
    return out


def off_by_one_unit(T: int) -> list[int]:
    """9 reads over 6 blocks: ends at T-1, T and T+1 past an edge, starts on an
    edge and one k-mer after it, reads of 1 k-mer first and last in a block."""
    return [T - 1,  # ends one k-mer before the edge
            1,      # the block's last k-mer: ends on the edge
            1,      # the next block's first k-mer: starts on the edge
            T,      # starts one after an edge, ends one after the next
            T - 1,  # starts one after an edge, ends on one
            T + 1,  # starts on an edge, ends one after the next
            T - 2,  # ends one before an edge
            1,      # last k-mer of its block
            T]      # one whole block


def cnt_over_unit(T: int) -> list[int]:
    """cnt_reads reads that fill one block: with the next block's first read one too many."""
    return [T // cnt_reads(T)] * cnt_reads(T)


def long_layout(T: int, blocks: int = 5) -> list[int]:
    return [7, blocks * T + 3] + [0] * 40 + [T - 10]


def _tails(T: int, target: int) -> list[int]:
    body = [T // 2 + 7, 0, 0, 0, 0, 0, T, 0, T]
    last = (target - sum(body)) % T or T
    return [0, 0, 0] + body + [0, 0, last] + [0, 0, 0, 0]


def layouts(T: int, word_phase: bool = False) -> dict[str, list[int]]:
    """Every named layout for block size T: name -> k-mers per read (0 = an
    empty or sub-k read).  `word_phase` adds the rbloom count pass's layout."""
    cnt = cnt_reads(T)
    fit = _split(T, cnt - 1)
    out = {
        "exact": [T] * 5,
        "off_by_one": off_by_one_unit(T) + [5],
        # block 1 holds cnt - 1 reads; with block 2's first read hi - lo + 1 == cnt
        "cnt_fit": [T] + fit + [T // 2],
        "cnt_over": [T] + cnt_over_unit(T) + [T // 2],
        # the same edge with empty reads making up the count: one in the middle of
        # the block, the others between its last k-mer and the next block's first read
        "cnt_fit_empty": [T] + _with_empties(_split(T, cnt - 4), 3) + [T // 2],
        "cnt_over_empty": [T] + _with_empties(_split(T, cnt - 4), 4) + [T // 2],
        "stage_fit": [T] + _split(T, STAGE_READS - 2) + [T // 2],
        "stage_over": [T] + _split(T, STAGE_READS - 1) + [T // 2],
        "tails_0": _tails(T, 0),
        "tails_1": _tails(T, 1),
        "tails_m1": _tails(T, T - 1),
        "long": long_layout(T),
    }
    if word_phase:
        # first global k-mer ids 1, 31 and 32 (mod 32), each read longer than one work unit
        out["word_phase"] = [1, SEG_KMERS + 62, SEG_KMERS + 33, SEG_KMERS + 44, 9]
    return out


def _with_empties(reads: list[int], empties: int) -> list[int]:
    mid = len(reads) // 2
    return reads[:mid] + [0] + reads[mid:] + [0] * (empties - 1)


def repeated(T: int, kmers: int) -> list[int]:
    """The off_by_one and cnt_over units, repeated to at least `kmers` k-mers, plus one block."""
    unit = off_by_one_unit(T) + cnt_over_unit(T)
    return unit * (-(-kmers // sum(unit))) + [T]


# ---------------------------------------------------------------- reads
def read_lengths(counts, k: int, step: int) -> list[int]:
    """A read of c k-mers is k + (c-1)*step bytes plus 0..step-1 slack bytes
    (num_kmers rounds up, so the slack must not add a k-mer); a read of 0
    k-mers is empty or k-1 bytes long, in turn."""
    out, z = [], 0
    for i, c in enumerate(counts):
        if c == 0:
            out.append((0, k - 1)[z % 2])
            z += 1
        else:
            out.append(k + (c - 1) * step + i % step)
    assert [num_kmers(L, k, step) for L in out] == list(counts)
    return out


def make_reads(rng, counts, k: int, step: int) -> list[bytes]:
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = read_lengths(counts, k, step)
    buf = acgt[rng.integers(0, 4, sum(lens))].tobytes()
    ofs = np.concatenate([[0], np.cumsum(lens)])
    return [buf[int(ofs[i]):int(ofs[i + 1])] for i in range(len(lens))]


# ---------------------------------------------------------------- plans
def part_shift(size: int, pref: int, floor: int) -> int:
    """part_shift of xs_part.h: 2^pref units per partition, halved down to 2^floor
    while that leaves fewer than 64 partitions, doubled while more than kPartMax."""
    def parts(s):
        return (size + (1 << s) - 1) >> s

    shift = pref
    while shift > floor and parts(shift) < 64:
        shift -= 1
    while parts(shift) > PART_MAX:
        shift += 1
    return shift


def cobs_plan(sig: int, h: int, mode: int, kbound: int = 0, workspace_mib: int | None = None) -> dict:
    """cobs_part_plan restated: partition shift and count, run padding, entries
    per block, and blocks per workspace range.  Modes 1 and 2 (production:
    2^17-row partitions down to 2^13), 3 (down to 2^10) and 4 (2^10 rows);
    any signature size the planner takes (below 2^30 rows)."""
    assert mode in (1, 2, 3, 4) and 0 < sig < 1 << 30
    shift = part_shift(sig, 10, 10) if mode == 4 else part_shift(sig, 17, 10 if mode == 3 else 13)
    assert shift + ID_BITS < 32, "the planner declines: a row and a k-mer id no longer fit one entry"
    P = (sig + (1 << shift) - 1) >> shift
    pad = 4 if P <= COBS_PAD_PARTS else 1
    stride = (COBS_CK * h + (pad - 1) * P + 7) // 8 * 8
    plan = {"shift": shift, "P": P, "pad": pad, "stride": stride, "last_rows": sig - ((P - 1) << shift)}
    if workspace_mib is not None:
        nblk = -(-kbound // COBS_CK)
        plan["nblk"] = nblk
        plan["rblk"] = max(1, min(nblk, (max(1, workspace_mib) << 20) // (stride * 20), ((1 << 32) - 1) // stride))
        plan["ranges"] = -(-nblk // plan["rblk"])
    return plan


def kbound(reads, step: int) -> int:
    """The planner's bound on a call's k-mers: bytes / step + reads + 1."""
    return sum(len(r) for r in reads) // step + len(reads) + 1


def bloom_plan(nbytes: int, mode: int = 3) -> dict:
    """bloom_part_plan restated: mode 3, partitions of 1024 bits, doubled while
    over kPartMax; modes 1 and 2 (production), 2^24-bit partitions down to 2^20
    while fewer than 64, doubled while over kPartMax."""
    assert mode in (1, 2, 3)
    mbits = nbytes * 8
    shift = part_shift(mbits, 10, 10) if mode == 3 else part_shift(mbits, 24, 20)
    P = (mbits + (1 << shift) - 1) >> shift
    return {"shift": shift, "P": P, "last_bits": mbits - ((P - 1) << shift)}


# ---------------------------------------------------------------- expectations
def closed_form(counts, D: int, docs) -> np.ndarray:
    """Hit matrix on an image whose every row has exactly the bits of `docs`."""
    out = np.zeros((len(counts), D), dtype=np.uint32)
    out[:, list(docs)] = np.asarray(counts, dtype=np.uint32)[:, None]
    return out


def misattribute_edge_kmers(counts, T: int) -> list[int]:
    """What a probe would count that gave every block's first k-mer to the read
    holding the k-mer before it."""
    ko = kofs(counts)
    out = list(counts)
    for g in range(T, int(ko[-1]), T):
        a = int(np.searchsorted(ko, g - 1, side="right")) - 1
        b = int(np.searchsorted(ko, g, side="right")) - 1
        if a != b:
            out[a] += 1
            out[b] -= 1
    return out


def double_added_rows(counts, T: int) -> list[int]:
    """What a probe would count that stored an "added" read's row and then added
    to it as well (or never zeroed it after an equal earlier call)."""
    return [2 * c if cls == "added" else c for c, cls in zip(counts, read_classes(counts, T))]


# ---------------------------------------------------------------- output buffers
# No probe path clears the hit matrix: a row is stored whole by the kernel that
# owns every k-mer of its read, and otherwise zeroed by separate code and built
# up with atomicAdd (skipped when the count is 0).  Whether the two agree shows
# only when the output does not happen to hold zeros already, so the tests of
# tests/test_gpu_output_buffers.py hand over outputs laid out as
# [head guard | body | tail guard] in one allocation, every byte a poison.
GUARD_ELEMS = 64            # elements of the output's type in each guard, at the least
POISON_BYTES = (0xFF, 0x5A)  # every byte: 0xFFFFFFFF (a count c added onto it wraps to c - 1) and 0x5A5A5A5A (+ c)


def unit_classes(counts) -> list[str]:
    """What the direct probes do with every read's hit row: "empty" (no work
    unit: zeroed, never visited), "whole" (one unit of up to kSegKmers k-mers:
    stored, never zeroed) or "split" (two units or more: zeroed, then added
    atomically by each).  The direct-path counterpart of read_classes."""
    out = []
    for c in counts:
        s = -(-int(c) // SEG_KMERS)
        out.append("empty" if s == 0 else "whole" if s == 1 else "split")
    return out


def poison_of(byte: int, dtype) -> int:
    """The value an untouched element of `dtype` reads as."""
    return int.from_bytes(bytes([byte]) * np.dtype(dtype).itemsize, "little")


def guarded_bytes(count: int, dtype) -> int:
    """Bytes of one allocation that holds `count` elements between two guards at any phase."""
    return (count + 2 * GUARD_ELEMS) * np.dtype(dtype).itemsize + 16


def body_offset(addr: int, dtype, phase: int) -> int:
    """Byte offset of the body in an allocation at `addr`: the first one past a
    whole head guard at which the body's address is `phase` (mod 16)."""
    size = np.dtype(dtype).itemsize
    assert phase % size == 0 and 0 <= phase < 16
    off = GUARD_ELEMS * size
    return off + (phase - (addr + off)) % 16


def check_guards(raw: np.ndarray, off: int, nbytes: int, byte: int, what: str = "") -> None:
    """Both guards of a guarded allocation (all of it, as bytes) still hold the poison."""
    assert raw.dtype == np.uint8 and raw.ndim == 1 and off + nbytes <= raw.size
    head = np.flatnonzero(raw[:off] != byte)
    tail = np.flatnonzero(raw[off + nbytes:] != byte)
    assert head.size == 0, (f"{what}: {head.size} byte(s) written before the output, the nearest "
                            f"{off - int(head[-1])} byte(s) before its first element")
    assert tail.size == 0, (f"{what}: {tail.size} byte(s) written past the output, the nearest "
                            f"{int(tail[0])} byte(s) after its last element")


class GuardedArray:
    """A host output of `count` elements of `dtype` between two guards, every
    byte of the allocation `byte`; `body` is what the library is handed, at an
    address of `phase` (mod 16).  alloc(nbytes) -> uint8 array of 16-byte
    aligned memory (numpy's own by default; pinned memory for one case)."""

    def __init__(self, count: int, dtype, byte: int, phase: int = 0, alloc=None):
        self.dtype, self.byte = np.dtype(dtype), byte
        total = guarded_bytes(count, dtype)
        self.raw = alloc(total) if alloc is not None else np.empty(total, dtype=np.uint8)
        assert self.raw.dtype == np.uint8 and self.raw.size == total
        self.raw[:] = byte
        self.off = body_offset(self.raw.ctypes.data, dtype, phase)
        self.nbytes = count * self.dtype.itemsize
        self.body = self.raw[self.off:self.off + self.nbytes].view(self.dtype)
        assert self.body.ctypes.data % 16 == phase and self.off + self.nbytes + GUARD_ELEMS * self.dtype.itemsize <= total

    @property
    def ptr(self) -> int:
        return self.body.ctypes.data

    def check(self, what: str = "") -> np.ndarray:
        check_guards(self.raw, self.off, self.nbytes, self.byte, what)
        return self.body.copy()


def explain_rows(got, want, classes, byte: int | None) -> str | None:
    """None when the matrices are equal; else the first wrong row, its read
    class, and what its first wrong cell looks like against the poison (byte
    None: the output was not poisoned, it held an earlier answer)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"shape {got.shape} against {want.shape}"
    g2, w2 = got.reshape(len(classes), -1), want.reshape(len(classes), -1)
    bad = np.flatnonzero((g2 != w2).any(axis=1))
    if bad.size == 0:
        return None
    r = int(bad[0])
    d = int(np.flatnonzero(g2[r] != w2[r])[0])
    g, w = int(g2[r, d]), int(w2[r, d])
    looks = "a wrong value"
    if byte is not None:
        p = poison_of(byte, got.dtype)
        mask = (1 << (8 * got.dtype.itemsize)) - 1
        looks = ("never written" if g == p else "added onto what the buffer held" if g == (p + w) & mask and w
                 else looks)
    return (f"{bad.size} of {len(classes)} rows differ, first row {r} ({classes[r]}): cell {d} is {g:#x}, "
            f"want {w:#x}: {looks}; classes of the wrong rows {sorted({classes[int(i)] for i in bad})}")


def assert_rows(got, want, classes, byte: int | None, what: str = "") -> None:
    msg = explain_rows(got, want, classes, byte)
    assert msg is None, f"{what}: {msg}"


def write_rows(body: np.ndarray, want: np.ndarray, untouched=(), added=(), sparse=()) -> None:
    """Model of a library writing the matrix `want` into the output `body`
    (same shape): rows `untouched` are never written, rows `added` are added
    onto what the buffer held (not zeroed first), rows `sparse` are stored
    without their zero cells; every other row is stored whole."""
    assert body.shape == want.shape
    for r in range(want.shape[0]):
        if r in untouched:
            continue
        if r in added:
            body[r] += want[r].astype(body.dtype)  # wraps, as the device's unsigned add does
        elif r in sparse:
            nz = want[r] != 0
            body[r][nz] = want[r][nz]
        else:
            body[r] = want[r]
