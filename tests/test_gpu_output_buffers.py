"""Every query and device call writes all of its outputs and nothing else (GPU).

No probe path clears the hit matrix.  A kernel stores a row whole only when it
owns every k-mer of the read; every other row is zeroed by separate code first
and built up with atomicAdd, which is skipped for a count of 0.  Four copies
of that zeroing rule have to agree with the stores they pair
with, and a disagreement leaves a row unwritten or added onto whatever the
buffer held: invisible in a fresh allocation, which is usually zero, and on
images whose stale answer happens to be the right one.

So every output here is the body of one allocation [head guard | body | tail
guard] filled with a poison byte (0xFF: a count c added onto it wraps to
c - 1; 0x5A: poison + c), at both 16-byte phases, and compared with a closed
form: the chosen-documents image (a read's k-mer count on those docs, 0
elsewhere: cells no atomicAdd touches) and the all-zero image (nothing is ever
added: every cell depends on the zeroing rule or on a store writing its
zeros).  The odd doc counts of the table (1, 129, 509, 1025, 2049, ...; 33 and
97 on the partitioned probe) leave rows unaligned in both phases.  Failure
messages name the class of the first wrong row (partition_layouts.unit_classes
and read_classes); tests/test_output_buffer_checker.py shows without a GPU
that the comparison catches each kind of disagreement.

1. the direct COBS kernels, every row of test_gpu_probe_kernels.ROWS, through
   xs_query_device;
2. the partitioned COBS probe, every layout, also in workspace ranges;
3. rbloom, direct and partitioned, on all-ones, all-zero and built filters;
4. the host entry points through ctypes (xs_query, xs_query_hits at 1 and 2
   bytes, xs_query_totals, xs_query_best), small and regular calls, and one
   batch larger than the first staging chunk;
5. one handle call after call, all-ones image first: the library's own last
   answer is the stale data, in the caller's buffers and in its workspace;
6. xs_best_device and xs_gather_reads_device at their edges.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import partition_layouts as pl
from test_gpu_probe_kernels import ROWS, _bank, _boundary_docs, _group_docs, _image, _sigs
from test_gpu_small_calls import _best

pytestmark = pytest.mark.gpu

STEPS = (1, 3)
COMBOS = [(byte, phase) for byte in pl.POISON_BYTES for phase in (0, 1)]  # phase: 0 or one element past 16 bytes

# name -> (k-mers per read, the unit classes the batch holds)
BATCHES = {
    "mixed": ([0, 1, 0, 0, 256, 257, 0, 512, 513, 255, 0, 64, 769, 0], ("empty", "whole", "split")),
    "all_whole": ([130] * 40, ("whole",)),       # no row qualifies for zeroing: query_small issues no memset
    "all_empty": ([0] * 5, ("empty",)),          # 0 bytes and k - 1 bytes in turn
    "one_empty": ([0], ("empty",)),
    "one_whole": ([1], ("whole",)),
    "one_split": ([257], ("split",)),
    "split_ends": ([600, 5, 0, 5, 600], ("empty", "whole", "split")),
}
# one-byte hit rows hold up to 255 k-mers per read; 90 (0x5A) and 255 would equal a poison
NARROW_BATCHES = {"narrow_mixed": [0, 1, 0, 0, 254, 64, 0, 130, 253, 0], "all_whole": [130] * 40, "all_empty": [0] * 5,
                  "one_empty": [0], "one_whole": [1]}

COBS_LAYOUT_CLASSES = {
    "exact": ("stored",), "off_by_one": ("stored", "added"), "cnt_fit": ("stored",), "cnt_over": ("stored", "added"),
    "cnt_fit_empty": ("empty", "stored"), "cnt_over_empty": ("empty", "stored", "added"),
    "stage_fit": ("stored", "added"), "stage_over": ("stored", "added"), "tails_0": ("empty", "stored", "added"),
    "tails_1": ("empty", "stored", "added"), "tails_m1": ("empty", "stored", "added"),
    "long": ("empty", "stored", "added"),
}
BLOOM_LAYOUT_CLASSES = {
    "exact": ("split",), "off_by_one": ("whole", "split"), "cnt_fit": ("whole", "split"),
    "cnt_over": ("whole", "split"), "cnt_fit_empty": ("empty", "whole", "split"),
    "cnt_over_empty": ("empty", "whole", "split"), "stage_fit": ("whole", "split"), "stage_over": ("whole", "split"),
    "tails_0": ("empty", "split"), "tails_1": ("empty", "split"), "tails_m1": ("empty", "split"),
    "long": ("empty", "whole", "split"), "word_phase": ("whole", "split"),
}
COBS_SIG = 30_011
BLOOM_BYTES = 30_011
COBS_PART_CASES = [(1, 21, 7), (33, 31, 1), (97, 21, 7), (pl.EMB_MAX_DOCS, 21, 7), (pl.EMB_MAX_DOCS + 1, 21, 7),
                   (128, 31, 8)]


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "torch sees no GPU"
    return t


# ---------------------------------------------------------------- guarded device outputs
class DevGuarded:
    """pl.GuardedArray on the device: one uint8 tensor full of `byte`, the body
    `count` elements of `dtype` at address `phase` elements past a 16-byte
    boundary; the library gets the body's raw pointer."""

    def __init__(self, torch, count, dtype, byte, phase):
        self.dtype, self.byte = np.dtype(dtype), byte
        self.raw = torch.full((pl.guarded_bytes(count, dtype),), byte, dtype=torch.uint8, device="cuda")
        self.off = pl.body_offset(self.raw.data_ptr(), dtype, phase * self.dtype.itemsize)
        self.nbytes = count * self.dtype.itemsize
        self.ptr = self.raw.data_ptr() + self.off
        assert self.ptr % 16 == phase * self.dtype.itemsize
        assert self.off + self.nbytes + pl.GUARD_ELEMS * self.dtype.itemsize <= self.raw.numel()

    def put(self, torch, values):
        """Lay input values (a hit matrix to reduce, reads to gather) over the body."""
        v = np.ascontiguousarray(values, dtype=self.dtype).reshape(-1).view(np.uint8)
        assert v.size == self.nbytes
        if v.size:
            self.raw[self.off:self.off + self.nbytes] = torch.from_numpy(v.copy()).to("cuda")

    def check(self, what=""):
        raw = self.raw.cpu().numpy()
        pl.check_guards(raw, self.off, self.nbytes, self.byte, what)
        return raw[self.off:self.off + self.nbytes].view(self.dtype).copy()


def _host_phase(dtype, phase):
    return phase * np.dtype(dtype).itemsize


# ---------------------------------------------------------------- reads
_READS: dict = {}


def _pack(reads):
    """Packed host reads: the bytes (64 spare ones behind, never an empty buffer) and n + 1 offsets."""
    buf = np.frombuffer(b"".join(reads) + b"\0" * 64, dtype=np.uint8).copy()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    return buf, offs


def _batch(torch, k, name, counts, step, reads=None):
    """One batch on the host and on the device, built once per (k, name, step)."""
    key = (k, name, step)
    if key not in _READS:
        if reads is None:
            rng = np.random.default_rng([k, step, len(counts), sum(counts)])
            reads = pl.make_reads(rng, counts, k, step)
        buf, offs = _pack(reads)
        seq_bytes = int(offs[-1])
        _READS[key] = SimpleNamespace(
            reads=reads, counts=list(counts), n=len(reads), buf=buf, offs=offs, seq_bytes=seq_bytes,
            d_seqs=torch.from_numpy(buf[:max(1, seq_bytes)].copy()).to("cuda"),  # tight: ends at the last read byte
            d_offs=torch.from_numpy(offs.astype(np.int64)).to("cuda"))
    b = _READS[key]
    assert b.counts == list(counts)
    return b


# ---------------------------------------------------------------- the device call
OUTPUTS = (("hits", "nk", "tot"), ("hits",), ("tot",))


def _query_device(torch, gb, b, cols, step, byte, phase, outputs):
    out = SimpleNamespace(hits=None, nk=None, tot=None)
    if "hits" in outputs:
        out.hits = DevGuarded(torch, b.n * cols, np.uint32, byte, phase)
    if "nk" in outputs:
        out.nk = DevGuarded(torch, b.n, np.uint64, byte, phase)
    if "tot" in outputs:
        out.tot = DevGuarded(torch, cols + 1, np.uint64, byte, phase)
    _run_device(torch, gb, b, step, out)
    return out


def _run_device(torch, gb, b, step, out):
    gb.query_device(b.d_seqs.data_ptr(), b.seq_bytes, b.d_offs.data_ptr(), b.n, step,
                    out.hits.ptr if out.hits else None, out.nk.ptr if out.nk else None,
                    out.tot.ptr if out.tot else None, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _check_device(out, b, want, classes, what):
    """Every output present equals the closed form `want` (n x cols), every guard is intact."""
    cols = want.shape[1]
    if out.hits:
        got = out.hits.check(f"{what}: hits").reshape(want.shape)
        pl.assert_rows(got, want, classes, out.hits.byte, f"{what}: hits")
    if out.nk:
        got = out.nk.check(f"{what}: num_kmers")
        assert np.array_equal(got, np.asarray(b.counts, dtype=np.uint64)), f"{what}: num_kmers differ: {got[:8]}"
    if out.tot:
        got = out.tot.check(f"{what}: totals")
        assert np.array_equal(got[:cols], want.sum(axis=0, dtype=np.uint64)), f"{what}: totals differ: {got[:8]}"
        assert int(got[cols]) == sum(b.counts), f"{what}: k-mer total {int(got[cols]):#x}"


def _device_cases(torch, gb, b, want, classes, step, kernel, what, outputs=OUTPUTS, crossed=True):
    """All outputs present: both poisons at both phases (crossed), or each
    poison and each phase once, the pairing swapped between the steps; the
    hits-only and totals-only calls always the latter."""
    once = COMBOS[::3] if step == STEPS[0] else COMBOS[1:3]
    for outs in outputs:
        for byte, phase in (COMBOS if crossed and outs == OUTPUTS[0] else once):
            out = _query_device(torch, gb, b, want.shape[1], step, byte, phase, outs)
            assert gb.probe_kernel() == kernel, f"{what}: routed to {gb.probe_kernel()}"
            _check_device(out, b, want, classes, f"{what}, poison {byte:#x}, phase {phase}, outputs {'+'.join(outs)}")


def _hold_oracle(ob, b, step, want):
    oh, on = ob.query(b.reads, step=step)
    assert np.array_equal(on, np.asarray(b.counts, dtype=np.uint64)) and np.array_equal(oh, want), \
        "the oracle misses the closed form"


# ---------------------------------------------------------------- 1. direct COBS kernels
@pytest.mark.parametrize("D,k,h,page,G,kernel", ROWS, ids=[f"{r[5]}-D{r[0]}-k{r[1]}h{r[2]}-p{r[3]}" for r in ROWS])
def test_direct_cobs_device_outputs(xs, oracle_mod, torch, D, k, h, page, G, kernel):
    """Every table row's kernel, chosen-documents and all-zero images, every
    batch at steps 1 and 3: hits, k-mer counts and totals all present, hits
    alone, totals alone."""
    P, _ = _group_docs(D, page, G)
    sig = _sigs(D, k, h, page, G)
    gb = _bank(xs, k, h, sig, D, page)
    for docs in (_boundary_docs(D, page, G), []):
        image = _image(sig, D, page, G, docs)
        assert image.any() == bool(docs)
        ob = oracle_mod.CobsBank(image, sig, P, D, h, k)
        gb.upload(ob.rows)
        for name, (counts, claimed) in BATCHES.items():
            classes = pl.unit_classes(counts)
            assert set(classes) == set(claimed), name
            want = pl.closed_form(counts, D, docs)
            for step in STEPS:
                b = _batch(torch, k, name, counts, step)
                if name == "mixed":
                    _hold_oracle(ob, b, step, want)
                _device_cases(torch, gb, b, want, classes, step, kernel, f"{name}, step {step}, {len(docs)} docs set",
                              crossed=D <= 512)  # the wider banks: each poison and phase once per step
    gb.close()


def test_a_call_without_reads_zeroes_the_totals_and_nothing_else(xs, torch):
    """n = 0: xs_query_device clears the D + 1 totals (the fourth rule) and
    leaves hits and k-mer counts alone; the host calls clear theirs."""
    D = 97
    gb = xs.Bank.create_cobs(21, 7, [COBS_SIG], D)
    lib = _lib(xs)
    d_offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    offs = np.zeros(1, dtype=np.uint64)
    for byte, phase in COMBOS:
        hits, nk, tot = (DevGuarded(torch, 4 * D, np.uint32, byte, phase), DevGuarded(torch, 4, np.uint64, byte, phase),
                         DevGuarded(torch, D + 1, np.uint64, byte, phase))
        gb.query_device(None, 0, d_offs, 0, 1, hits.ptr, nk.ptr, tot.ptr, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert not tot.check("n = 0: totals").any()
        assert (hits.check("n = 0") == pl.poison_of(byte, np.uint32)).all()
        assert (nk.check("n = 0") == pl.poison_of(byte, np.uint64)).all()
        h_tot, h_nk = pl.GuardedArray(D, np.uint64, byte, 8 * phase), pl.GuardedArray(1, np.uint64, byte, 8 * phase)
        _ok(xs, lib.xs_query_totals(gb.handle, None, offs.ctypes.data, 0, 1, h_tot.ptr, h_nk.ptr))
        assert not h_tot.check("n = 0: xs_query_totals").any() and int(h_nk.check()[0]) == 0
        best, b_tot = pl.GuardedArray(4, np.uint32, byte, 4 * phase), pl.GuardedArray(D + 1, np.uint64, byte, 8 * phase)
        _ok(xs, lib.xs_query_best(gb.handle, None, offs.ctypes.data, 0, 1, best.ptr, None, None, b_tot.ptr))
        assert not b_tot.check("n = 0: xs_query_best").any()
        assert (best.check() == pl.poison_of(byte, np.uint32)).all()
    gb.close()


def test_all_empty_alternates_read_lengths(torch):
    b = _batch(torch, 21, "all_empty", BATCHES["all_empty"][0], 1)
    assert [len(r) for r in b.reads] == [0, 20, 0, 20, 0]


# ---------------------------------------------------------------- 2. partitioned COBS
def _cobs_image(D, docs):
    return _image([COBS_SIG], D, None, 1, docs)


def _part_docs(D):
    return sorted(d for d in {0, 31, 32, 63, 64, 95, 96, D - 1} if 0 <= d < D)


@pytest.mark.parametrize("D,k,h", COBS_PART_CASES, ids=[f"D{c[0]}-k{c[1]}h{c[2]}" for c in COBS_PART_CASES])
def test_cobspart_device_outputs(xs, oracle_mod, torch, D, k, h):
    """Every layout at T = kCobsCK, steps 1 and 3, both images, 30 partitions."""
    T = pl.COBS_CK
    assert pl.cobs_plan(COBS_SIG, h, 3)["P"] == 30
    gb = xs.Bank.create_cobs(k, h, [COBS_SIG], D)
    gb.set_probe_options(cobs_part=3)
    seen = set()
    for docs in (_part_docs(D), []):
        ob = oracle_mod.CobsBank(_cobs_image(D, docs), [COBS_SIG], (D + 7) // 8, D, h, k)
        gb.upload(ob.rows)
        for name, counts in pl.layouts(T).items():
            classes = pl.read_classes(counts, T)
            assert set(classes) == set(COBS_LAYOUT_CLASSES[name]), name
            seen |= set(classes)
            want = pl.closed_form(counts, D, docs)
            for step in STEPS:
                b = _batch(torch, k, "cobs_" + name, counts, step)
                if name == "tails_1":
                    _hold_oracle(ob, b, step, want)
                _device_cases(torch, gb, b, want, classes, step, "cobspart",
                              f"{name}, step {step}, {len(docs)} docs set",
                              outputs=OUTPUTS if name in ("tails_1", "cnt_over_empty", "long") else OUTPUTS[:1])
    assert seen == {"empty", "stored", "added"}
    gb.close()


def test_cobspart_device_outputs_in_workspace_ranges(xs, oracle_mod, torch):
    """A 1 MiB workspace: the zeroing kernel runs once per call, the resolve
    pass once per range of R = 3 blocks.  The long read crosses two range
    boundaries; the repeated off_by_one unit puts range boundaries between
    reads and, one block later, inside them."""
    D, k, h, T = 97, 21, 7, pl.COBS_CK
    R = pl.cobs_plan(COBS_SIG, h, 3, 1 << 40, workspace_mib=1)["rblk"]
    assert R == 3
    unit = pl.off_by_one_unit(T)
    obo = unit * (-(-(2 * R + 1) * T // sum(unit))) + [5]
    batches = {"long": pl.long_layout(T, blocks=3 * R), "off_by_one": obo, "shifted": [T] + obo}
    gb = xs.Bank.create_cobs(k, h, [COBS_SIG], D)
    gb.set_probe_options(cobs_part=3, workspace_mib=1)
    for docs in (_part_docs(D), []):
        ob = oracle_mod.CobsBank(_cobs_image(D, docs), [COBS_SIG], (D + 7) // 8, D, h, k)
        gb.upload(ob.rows)
        for name, counts in batches.items():
            classes = pl.read_classes(counts, T)
            assert {"stored", "added"} <= set(classes)
            want = pl.closed_form(counts, D, docs)
            for step in STEPS:
                b = _batch(torch, k, "ranges_" + name, counts, step)
                plan = pl.cobs_plan(COBS_SIG, h, 3, pl.kbound(b.reads, step), workspace_mib=1)
                assert plan["rblk"] == R and plan["ranges"] >= 3
                if name == "long":
                    _hold_oracle(ob, b, step, want)
                _device_cases(torch, gb, b, want, classes, step, "cobspart",
                              f"{name}, step {step}, {len(docs)} docs set, 1 MiB workspace")
    gb.close()


# ---------------------------------------------------------------- 3. rbloom
_GENOME: dict = {}


def _genome():
    if "g" not in _GENOME:
        rng = np.random.default_rng(20_000)
        _GENOME["g"] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 20_000)].tobytes()
    return _GENOME["g"]


def _member_reads(reads, k):
    """The same lengths with every second read cut from the genome and every
    third one half genome, half foreign: counts of 0, of all and in between."""
    g, out = _genome(), []
    for i, r in enumerate(reads):
        L = len(r)
        assert L <= len(g)
        s = (977 * i) % (len(g) - L + 1)
        if i % 3 == 2 and L >= 2 * k:
            out.append(g[s:s + L // 2] + r[L // 2:])
        elif i % 2 == 0:
            out.append(g[s:s + L])
        else:
            out.append(r)
    return out


def _bloom_images(oracle_mod, k, K):
    bf = oracle_mod.BloomFilter(np.zeros(BLOOM_BYTES, dtype=np.uint8), K, k)
    bf.build([_genome()])
    return {"ones": np.full(BLOOM_BYTES, 0xFF, dtype=np.uint8), "zero": np.zeros(BLOOM_BYTES, dtype=np.uint8),
            "built": bf}


def _bloom_cases(xs, oracle_mod, torch, k, K, part, kernel, batches, tag):
    gb = xs.Bank.create_bloom(k, BLOOM_BYTES, K)
    gb.set_probe_options(bloom_part=part)
    between = False
    for image, payload in _bloom_images(oracle_mod, k, K).items():
        gb.upload(payload.bits if image == "built" else payload)
        for name, (counts, claimed) in batches.items():
            classes = pl.unit_classes(counts)
            assert set(classes) == set(claimed), name
            for step in STEPS:
                b = _batch(torch, k, tag + name, counts, step)
                if image == "built":
                    b = _batch(torch, k, tag + "members_" + name, counts, step, reads=_member_reads(b.reads, k))
                    wh, wn = payload.query(b.reads, step=step)
                    assert np.array_equal(wn, np.asarray(counts, dtype=np.uint64))
                    between |= bool(((wh > 0) & (wh < wn)).any())
                    want = wh.astype(np.uint32)[:, None]
                else:
                    want = pl.closed_form(counts, 1, [0] if image == "ones" else [])
                _device_cases(torch, gb, b, want, classes, step, kernel, f"{name}, step {step}, {image} filter",
                              outputs=OUTPUTS if part == 0 or name in ("cnt_over_empty", "long", "word_phase")
                              else OUTPUTS[:1])
    assert between, "the built filter gives no count strictly between 0 and the k-mer count"
    gb.close()


@pytest.mark.parametrize("k,K,kernel", [(21, 7, "bloom<21,7>"), (31, 5, "bloom<0,0>")])
def test_bloom_direct_device_outputs(xs, oracle_mod, torch, k, K, kernel):
    _bloom_cases(xs, oracle_mod, torch, k, K, 0, kernel, BATCHES, "bloom_")


def test_bloompart_device_outputs(xs, oracle_mod, torch):
    """Every layout at T = kPartKmers, word_phase included, filter of 30 011
    bytes (235 partitions): the count pass follows the unit rule."""
    assert pl.bloom_plan(BLOOM_BYTES)["P"] == 235
    lay = {name: (counts, BLOOM_LAYOUT_CLASSES[name]) for name, counts in pl.layouts(pl.PART_KMERS, word_phase=True).items()}
    _bloom_cases(xs, oracle_mod, torch, 21, 7, 3, "bloompart", lay, "bpart_")


# ---------------------------------------------------------------- the eight paths of the host and repeat cases
def _row(kernel):
    """The widest table row of a kernel."""
    return [r for r in ROWS if r[5] == kernel][-1]


PATHS = {  # name -> kernel its bank must route to
    "fast": "fast<21,7>", "vslice": "vslice<31,3>", "wide": "wide<21,7,C2,G1>", "slots": "slots<0,0,8,1>",
    "general": "general", "cobspart": "cobspart", "bloom": "bloom<21,7>", "bloompart": "bloompart",
}


def _path(xs, name):
    """(bank, kernel, cols, k, {image: (payload, docs)}) of one path; `ones` is every doc set."""
    kernel = PATHS[name]
    if name in ("bloom", "bloompart"):
        gb = xs.Bank.create_bloom(21, BLOOM_BYTES, 7)
        gb.set_probe_options(bloom_part=3 if name == "bloompart" else 0)
        images = {"ones": (np.full(BLOOM_BYTES, 0xFF, dtype=np.uint8), [0]),
                  "zero": (np.zeros(BLOOM_BYTES, dtype=np.uint8), []),
                  "chosen": (np.full(BLOOM_BYTES, 0xFF, dtype=np.uint8), [0])}  # one column: chosen = all of it
        return gb, kernel, 1, 21, images
    if name == "cobspart":
        D, k, h, page, G, sig = 97, 21, 7, None, 1, [COBS_SIG]
        gb = xs.Bank.create_cobs(k, h, sig, D)
        gb.set_probe_options(cobs_part=3)
        chosen = _part_docs(D)
    else:
        D, k, h, page, G, _ = _row(kernel)
        sig = _sigs(D, k, h, page, G)
        gb = _bank(xs, k, h, sig, D, page)
        chosen = _boundary_docs(D, page, G)
    images = {"ones": (_image(sig, D, page, G, list(range(D))), list(range(D))),
              "zero": (_image(sig, D, page, G, []), []), "chosen": (_image(sig, D, page, G, chosen), chosen)}
    return gb, kernel, D, k, images


def _path_classes(name, counts):
    return pl.read_classes(counts, pl.COBS_CK) if name == "cobspart" else pl.unit_classes(counts)


# ---------------------------------------------------------------- 4. host API outputs
def _lib(xs):
    return xs._lib.load()


def _ok(xs, rc):
    assert rc == 0, f"rc {rc}: {_lib(xs).xs_last_error().decode()}"


def _host_query_cases(xs, gb, kernel, b, cols, step, want, classes, what, alloc=None, combos=COMBOS):
    """xs_query, xs_query_hits (1 and 2 bytes), xs_query_totals and xs_query_best
    on one batch: exact outputs, intact guards, the path's kernel."""
    lib, n = _lib(xs), b.n
    nk_want = np.asarray(b.counts, dtype=np.uint64)
    tot_want = want.sum(axis=0, dtype=np.uint64)
    args = (gb.handle, b.buf.ctypes.data, b.offs.ctypes.data, n, step)
    for byte, phase in combos:
        tag = f"{what}, poison {byte:#x}, phase {phase}"

        def arr(count, dtype):
            return pl.GuardedArray(count, dtype, byte, _host_phase(dtype, phase), alloc)

        # xs_query: both outputs, then each alone
        for with_hits, with_nk in ((True, True), (True, False), (False, True)):
            hits, nk = arr(n * cols, np.uint32), arr(n, np.uint64)
            _ok(xs, lib.xs_query(*args, hits.ptr if with_hits else None, nk.ptr if with_nk else None))
            assert gb.probe_kernel() == kernel, f"{tag}: routed to {gb.probe_kernel()}"
            got_h, got_n = hits.check(f"{tag}: xs_query hits"), nk.check(f"{tag}: xs_query num_kmers")
            if with_hits:
                pl.assert_rows(got_h.reshape(want.shape), want, classes, byte, f"{tag}: xs_query")
            else:
                assert (got_h == pl.poison_of(byte, np.uint32)).all()
            assert np.array_equal(got_n, nk_want if with_nk else np.full(n, pl.poison_of(byte, np.uint64), np.uint64))
        # xs_query_hits: the guards sit one byte / one halfword past the matrix
        for dtype in (np.uint8, np.uint16):
            size = np.dtype(dtype).itemsize
            hits, nk = arr(n * cols, dtype), arr(n, np.uint64)
            rc = lib.xs_query_hits(*args, hits.ptr, size, nk.ptr)
            if max(b.counts) >= 1 << (8 * size):  # refused before anything is written
                assert rc == xs._lib.XS_ERR_ARG
                assert (hits.check(tag) == pl.poison_of(byte, dtype)).all()
                assert (nk.check(tag) == pl.poison_of(byte, np.uint64)).all()
                continue
            _ok(xs, rc)
            assert gb.probe_kernel() == kernel
            got_h = hits.check(f"{tag}: xs_query_hits {size} hits").reshape(want.shape)
            pl.assert_rows(got_h, want.astype(dtype), classes, byte, f"{tag}: xs_query_hits {size}")
            assert np.array_equal(nk.check(f"{tag}: xs_query_hits {size} num_kmers"), nk_want)
        # xs_query_totals: D sums, the k-mer total apart
        tot, nkt = arr(cols, np.uint64), arr(1, np.uint64)
        _ok(xs, lib.xs_query_totals(*args, tot.ptr, nkt.ptr))
        assert gb.probe_kernel() == kernel
        assert np.array_equal(tot.check(f"{tag}: xs_query_totals"), tot_want), f"{tag}: totals differ"
        assert int(nkt.check(f"{tag}: xs_query_totals k-mers")[0]) == sum(b.counts)
        # xs_query_best: with and without each optional output
        best_want, max_want = _best(want)
        for opt in (("bh", "nk", "tot"), ("nk", "tot"), ("bh", "tot"), ("bh", "nk"), ()):
            best, bh, nk, tot = arr(n, np.uint32), arr(n, np.uint32), arr(n, np.uint64), arr(cols + 1, np.uint64)
            _ok(xs, lib.xs_query_best(*args, best.ptr, bh.ptr if "bh" in opt else None, nk.ptr if "nk" in opt else None,
                                      tot.ptr if "tot" in opt else None))
            assert gb.probe_kernel() == kernel
            t = f"{tag}: xs_query_best with {opt}"
            assert np.array_equal(best.check(t + " best_doc"), best_want), f"{t}: best docs differ"
            got = {"bh": bh.check(t + " best_hits"), "nk": nk.check(t + " num_kmers"), "tot": tot.check(t + " totals")}
            full = {"bh": max_want, "nk": nk_want, "tot": np.concatenate([tot_want, [np.uint64(sum(b.counts))]])}
            for key, g in got.items():
                if key in opt:
                    assert np.array_equal(g, full[key]), f"{t}: {key} differs"
                else:
                    assert (g == pl.poison_of(byte, g.dtype)).all(), f"{t}: {key} written though NULL was passed"


@pytest.mark.parametrize("small", [1, 0], ids=["small", "regular"])
@pytest.mark.parametrize("name", list(PATHS))
def test_host_api_outputs(xs, oracle_mod, torch, name, small):
    gb, kernel, cols, k, images = _path(xs, name)
    gb.set_probe_options(small_calls=small)
    batches = {**{n: c for n, (c, _) in BATCHES.items()}, **NARROW_BATCHES}
    for image in ("chosen", "zero"):
        payload, docs = images[image]
        gb.upload(payload)
        for bname, counts in batches.items():
            classes = _path_classes(name, counts)
            want = pl.closed_form(counts, cols, docs)
            for step in STEPS:
                b = _batch(torch, k, bname, counts, step)
                _host_query_cases(xs, gb, kernel, b, cols, step, want, classes, f"{name}, {bname}, step {step}, {image}",
                                  combos=COMBOS if bname in ("mixed", "narrow_mixed") else COMBOS[::3])
    gb.close()


def test_host_api_outputs_in_pinned_memory(xs, torch):
    """The same with every output in pinned memory (rows arrive by DMA as they are)."""
    gb, kernel, cols, k, images = _path(xs, "fast")

    def pinned(nbytes):
        return xs.pinned_empty(nbytes, np.uint8)

    for small in (1, 0):
        gb.set_probe_options(small_calls=small)
        for image in ("chosen", "zero"):
            payload, docs = images[image]
            gb.upload(payload)
            for bname in ("mixed", "narrow_mixed"):
                counts = {**{n: c for n, (c, _) in BATCHES.items()}, **NARROW_BATCHES}[bname]
                b = _batch(torch, k, bname, counts, 1)
                _host_query_cases(xs, gb, kernel, b, cols, 1, pl.closed_form(counts, cols, docs),
                                  pl.unit_classes(counts), f"pinned, {bname}, {image}, small_calls {small}", alloc=pinned)
    gb.close()


def test_host_batch_over_the_first_staging_chunk(xs, oracle_mod, torch):
    """60 k reads of 150 bp (9 MB, over kHostFirst) with a handful of empty
    ones, D = 8, h = 1: the reads arrive through the staging ring, the hit rows
    leave through the chunked copier, whose last chunk stops at the last row."""
    D, k, h, sig, n = 8, 31, 1, [5_003], 60_000
    docs = [0, 3, 7]
    rng = np.random.default_rng(60)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n * 150)].tobytes()
    reads = [text[i * 150:(i + 1) * 150] for i in range(n)]
    for i in (0, 1, 777, 30_000, n - 1):
        reads[i] = b"" if i % 2 else reads[i][:k - 1]
    counts = [pl.num_kmers(len(r), k, 1) for r in reads]
    assert sum(len(r) for r in reads) > pl.HOST_FIRST and set(counts) == {0, 120}
    classes = pl.unit_classes(counts)
    b = _batch(torch, k, "over_first_chunk", counts, 1, reads=reads)
    want = pl.closed_form(counts, D, docs)
    image = _image(sig, D, None, 1, docs)
    ob = oracle_mod.CobsBank(image, sig, 1, D, h, k)
    oh, on = ob.query(reads[:2000] + reads[-2000:])
    assert np.array_equal(oh, np.concatenate([want[:2000], want[-2000:]])), "the oracle misses the closed form"
    assert np.array_equal(on, np.asarray(counts[:2000] + counts[-2000:], dtype=np.uint64))
    gb = xs.Bank.create_cobs(k, h, sig, D)
    gb.set_probe_options(cobs_part=0)
    gb.upload(image)
    lib = _lib(xs)
    args = (gb.handle, b.buf.ctypes.data, b.offs.ctypes.data, n, 1)

    def pinned(nbytes):
        return xs.pinned_empty(nbytes, np.uint8)

    for byte, phase, dtype, alloc in ((0xFF, 1, np.uint32, None), (0x5A, 1, np.uint8, None), (0xFF, 0, np.uint8, None),
                                      (0x5A, 0, np.uint16, None), (0xFF, 1, np.uint8, pinned)):
        hits = pl.GuardedArray(n * D, dtype, byte, _host_phase(dtype, phase), alloc)
        nk = pl.GuardedArray(n, np.uint64, byte, 8 * phase, alloc)
        _ok(xs, lib.xs_query_hits(*args, hits.ptr, np.dtype(dtype).itemsize, nk.ptr))
        assert gb.probe_kernel() == "fast<31,1>"
        what = f"9 MB batch, {np.dtype(dtype).name} hits, poison {byte:#x}, phase {phase}, pinned {alloc is not None}"
        pl.assert_rows(hits.check(what).reshape(want.shape), want.astype(dtype), classes, byte, what)
        assert np.array_equal(nk.check(what), np.asarray(counts, dtype=np.uint64))
    gb.close()


# ---------------------------------------------------------------- 5. one handle, call after call
def _rotations(name):
    """The batches of phase B: rotations of `mixed`, or of a layout that holds every class."""
    if name == "cobspart":
        base = pl.layouts(pl.COBS_CK)["tails_1"]
    elif name == "bloompart":
        base = pl.layouts(pl.PART_KMERS, word_phase=True)["cnt_over_empty"]
    else:
        base = BATCHES["mixed"][0]
    assert len(set(_path_classes(name, base))) == 3
    return [base[r:] + base[:r] for r in (0, 5)]


@pytest.mark.parametrize("mode", ["host_small", "host_regular", "device"])
@pytest.mark.parametrize("name", list(PATHS))
def test_same_handle_same_buffers_call_after_call(xs, torch, name, mode):
    """A: the all-ones image and a batch of whole reads, every cell a nonzero
    count.  B: the all-zero image, then the chosen-documents image; on each a
    batch of as many reads whose classes are a rotation of `mixed` (or of a
    partitioned layout), then A's batch again.  The order all-ones -> chosen,
    with nothing cleared in between: through the host API (the handle's own hit
    matrix and small-call buffer) and through xs_query_device into the same
    output tensors, never refilled."""
    gb, kernel, cols, k, images = _path(xs, name)
    gb.set_probe_options(small_calls=1 if mode == "host_small" else 0)
    for ri, rot in enumerate(_rotations(name)):
        n = len(rot)
        a_counts = [130] * n
        batch_a = _batch(torch, k, f"whole_{n}", a_counts, 1)
        batch_b = _batch(torch, k, f"rot_{name}_{ri}", rot, 1)
        assert set(pl.unit_classes(a_counts)) == {"whole"}
        classes = {id(batch_a): _path_classes(name, a_counts), id(batch_b): _path_classes(name, rot)}
        changed = sum(x != y for x, y in zip(classes[id(batch_a)], classes[id(batch_b)]))
        assert changed >= n // 3, "the rotation leaves nearly every row in its class"
        out = SimpleNamespace(hits=DevGuarded(torch, n * cols, np.uint32, 0x5A, ri),
                              nk=DevGuarded(torch, n, np.uint64, 0x5A, ri),
                              tot=DevGuarded(torch, cols + 1, np.uint64, 0x5A, ri)) if mode == "device" else None
        for image, order in (("ones", (batch_a,)), ("zero", (batch_b, batch_a)), ("chosen", (batch_b, batch_a))):
            payload, docs = images[image]
            gb.upload(payload)
            for b in order:
                want = pl.closed_form(b.counts, cols, docs)
                if image == "ones":
                    assert want.all()
                what = f"{name}, {mode}, rotation {ri}, {image} image, batch {'A' if b is batch_a else 'B'}"
                if mode == "device":
                    _run_device(torch, gb, b, 1, out)
                    assert gb.probe_kernel() == kernel
                    _check_device(out, b, want, classes[id(b)], what)
                    continue
                got_h, got_n = gb.query(b.reads, step=1)
                assert gb.probe_kernel() == kernel, f"{what}: routed to {gb.probe_kernel()}"
                pl.assert_rows(got_h, want, classes[id(b)], None, what)
                assert np.array_equal(got_n, np.asarray(b.counts, dtype=np.uint64))
                best, bh, bn, btot = gb.query_best(b.reads, step=1, want_totals=True)
                assert gb.probe_kernel() == kernel
                wb, wm = _best(want)
                assert np.array_equal(best, wb) and np.array_equal(bh, wm), f"{what}: best doc differs"
                assert np.array_equal(btot[:cols], want.sum(axis=0, dtype=np.uint64)) and int(btot[cols]) == sum(b.counts)
    gb.close()


# ---------------------------------------------------------------- 6. xs_best_device
def _best_rows(D, rng):
    """Crafted rows for a matrix of D docs (those that fit D), low noise of 0..6 under each."""
    def noise():
        return rng.integers(0, 7, D).astype(np.uint32)

    rows = [np.zeros(D, np.uint32)]                       # all zero: ambiguous, doc 0 at D = 1
    for d in sorted({0, 63, 64, D - 1}):
        if d < D:                                         # a single maximum
            r = noise()
            r[d] = 9
            rows.append(r)
    for d in sorted({0, D - 65}):
        if 0 <= d and d + 64 < D:                         # two equal maxima in one lane
            r = noise()
            r[d] = r[d + 64] = 9
            rows.append(r)
    if D >= 2:                                            # ... and in different lanes
        for a, c in ((0, 1), (min(1, D - 2), D - 1)):
            r = noise()
            r[a] = r[c] = 9
            rows.append(r)
    for big in (0x80000000, 0xFFFFFFFF):                  # a signed comparison would show here
        r = noise()
        if D >= 2:
            r[0] = 0x7FFFFFFF
        r[D - 1] = big
        rows.append(r)
        if D >= 2:
            r = r.copy()
            r[D // 2 - (D // 2 == D - 1)] = big           # tied
            rows.append(r)
    # a maximum unique only within its row: the next row starts with the same value
    r = noise()
    r[0] = 9
    rows.append(r)
    r = noise()
    r[0] = 9
    if D >= 2:
        r[D - 1] = 9
    rows.append(r)
    r = noise()                                           # the last row: its maximum in the last cell, then the guard
    r[D - 1] = 9
    rows.append(r)
    return np.stack(rows)


def _best_cases(xs, torch, hits, what):
    n, D = hits.shape
    want_best, want_max = _best(hits)
    for byte, phase in COMBOS:
        d_hits = DevGuarded(torch, n * D, np.uint32, byte, phase)
        d_hits.put(torch, hits)
        for with_hits in (True, False):
            best, bh = DevGuarded(torch, n, np.uint32, byte, phase), DevGuarded(torch, n, np.uint32, byte, phase)
            xs.best_device(d_hits.ptr, n, D, best.ptr, bh.ptr if with_hits else None,
                           stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            tag = f"{what}, poison {byte:#x}, phase {phase}, best_hits {with_hits}"
            got = best.check(tag + ": best_doc")
            bad = np.flatnonzero(got != want_best)
            assert bad.size == 0, f"{tag}: row {bad[0]} gives {got[bad[0]]:#x}, want {want_best[bad[0]]:#x}: {hits[bad[0]][:8]}"
            got = bh.check(tag + ": best_hits")
            assert np.array_equal(got, want_max if with_hits else np.full(n, pl.poison_of(byte, np.uint32), np.uint32)), tag
        assert np.array_equal(d_hits.check(tag + ": the input").reshape(n, D), hits)


@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 129, 1430])
def test_best_device_crafted_rows(xs, torch, D):
    rows = _best_rows(D, np.random.default_rng(D))
    want_best, _ = _best(rows)
    assert want_best[0] == (0 if D == 1 else 0xFFFFFFFF)
    assert want_best[-1] == D - 1 and want_best[-3] == 0
    if D >= 2:
        assert (want_best == 0xFFFFFFFF).sum() >= 5 and (want_best == D - 1).sum() >= 3
    _best_cases(xs, torch, rows, f"D {D}, {len(rows)} crafted rows")
    _best_cases(xs, torch, rows[:5], f"D {D}, 5 rows")
    for r in (0, len(rows) - 4, len(rows) - 1):
        _best_cases(xs, torch, rows[r:r + 1], f"D {D}, row {r} alone")


def test_best_device_stride_loop(xs, torch):
    """70 000 rows: over the launch's 65 536 waves, so the stride loop runs."""
    rng = np.random.default_rng(70_000)
    hits = rng.integers(0, 4, (70_000, 3)).astype(np.uint32)
    hits[-1] = (1, 2, 3)
    hits[65_536] = (0xFFFFFFFF, 0x80000000, 0x7FFFFFFF)
    best, _ = _best(hits)
    assert 0.2 < (best == 0xFFFFFFFF).mean() < 0.8
    _best_cases(xs, torch, hits, "70 000 rows")


# ---------------------------------------------------------------- 6. xs_gather_reads_device
def _gather_case(xs, torch, lengths, index, byte, src_phase, out_phase, what):
    rng = np.random.default_rng(len(index) + byte)
    src = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lengths]
    buf, offs = _pack(src)
    total = int(offs[-1])
    d_src = DevGuarded(torch, total, np.uint8, byte, src_phase)
    d_src.put(torch, buf[:total])
    out_offs = np.zeros(len(index) + 1, dtype=np.uint64)
    np.cumsum([len(src[i]) + 3 for i in index], out=out_offs[1:])  # a 3-byte gap after every read
    out = DevGuarded(torch, int(out_offs[-1]), np.uint8, byte, out_phase)
    assert d_src.ptr % 2 == 1 and out.ptr % 2 == 1
    d_offs = torch.from_numpy(offs.astype(np.int64)).to("cuda")
    d_index = torch.from_numpy(np.asarray(index, dtype=np.int32)).to("cuda")
    d_out_offs = torch.from_numpy(out_offs.astype(np.int64)).to("cuda")
    xs.gather_reads_device(d_src.ptr, d_offs, d_index, len(index), out.ptr, d_out_offs,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.check(what)
    want = np.full(int(out_offs[-1]), byte, dtype=np.uint8)  # the gaps keep the fill
    for j, i in enumerate(index):
        o = int(out_offs[j])
        want[o:o + len(src[i])] = np.frombuffer(src[i], dtype=np.uint8)
    bad = np.flatnonzero(got != want)
    if bad.size:
        j = int(np.searchsorted(out_offs, bad[0], side="right")) - 1
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {bad[0] - int(out_offs[j])} of output "
                             f"read {j} (input read {index[j]}, {len(src[index[j]])} bytes)")
    assert np.array_equal(d_src.check(what + ": the input"), buf[:total])


@pytest.mark.parametrize("byte", [0xEE, *pl.POISON_BYTES])
def test_gather_reads_device_edges(xs, torch, byte):
    """Reads of 0 to 100 003 bytes of all 256 values; an index in descending
    order with repeats, the empty reads first and last; 3-byte gaps; source and
    output at odd addresses."""
    lengths = [0, 1, 63, 64, 65, 150, 100_003, 0]
    index = [7, 6, 6, 5, 4, 3, 2, 1, 1, 0]
    assert lengths[index[0]] == lengths[index[-1]] == 0 and index == sorted(index, reverse=True)
    for src_phase, out_phase in ((1, 7), (15, 1)):
        _gather_case(xs, torch, lengths, index, byte, src_phase, out_phase,
                     f"fill {byte:#x}, source phase {src_phase}, output phase {out_phase}")


def test_gather_reads_device_stride_loop(xs, torch):
    """70 000 output reads of 0-20 bytes: over the launch's 65 536 waves."""
    rng = np.random.default_rng(7)
    lengths = [int(x) for x in rng.integers(0, 21, 1000)]
    index = [int(x) for x in rng.integers(0, 1000, 70_000)]
    _gather_case(xs, torch, lengths, index, 0xEE, 3, 5, "70 000 reads")


def test_gather_reads_device_of_nothing(xs, torch):
    """m = 0 with every pointer NULL is allowed: XS_OK, nothing written."""
    lib = _lib(xs)
    _ok(xs, lib.xs_gather_reads_device(None, None, None, 0, None, None, None))
    out = DevGuarded(torch, 16, np.uint8, 0xEE, 1)
    d_offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    _ok(xs, lib.xs_gather_reads_device(None, None, None, 0, ctypes.c_void_p(out.ptr), ctypes.c_void_p(d_offs.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert (out.check("m = 0") == 0xEE).all()
