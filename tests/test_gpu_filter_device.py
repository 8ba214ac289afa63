"""Read filtering on the device (GPU): the keep kernel, the compaction, the host
call that probes and decides, the one-pass filter_genus / filter_species and
the fused pipeline's hand-off.

Reference: ``ModelResult.get_filter_mask`` / ``get_filtered_subsequence_labels``
(``src/xspect/models/result.py:92-149``), ``filter_sequences``
(``file_io.py:166-191``) and the pipeline's hand-off (``main.py:116-145``).
The expected value of every keep decision is Python's own ``round(h / n, 2)``
on Python floats, never the cut table.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import partition_layouts as pl
from test_gpu_filter import K, _reads, models  # noqa: F401  (models: the fixture)
from test_gpu_output_buffers import DevGuarded

pytestmark = pytest.mark.gpu

THRESHOLDS = [c / 100 for c in range(101)] + [0.295, math.nextafter(0.29, 1), 0.7, 1.0, -1]


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


def _rounded(h, n) -> np.ndarray:
    """Python's round(h / n, 2) per pair (0.0 where n == 0), over the distinct pairs."""
    h, n = np.asarray(h, dtype=np.uint64).reshape(-1), np.asarray(n, dtype=np.uint64).reshape(-1)
    pairs, inv = np.unique(np.stack([h, n], axis=1), axis=0, return_inverse=True)
    vals = np.array([round(int(a) / int(b), 2) if b else 0.0 for a, b in pairs.tolist()], dtype=np.float64)
    return vals[np.asarray(inv).reshape(-1)]


def _expected(hits, nk, label, threshold, mask=None) -> np.ndarray:
    if len(nk) == 0:
        return np.zeros(0, dtype=np.uint8)
    hits = np.asarray(hits).reshape(len(nk), -1)
    score = _rounded(hits[:, label], nk)
    if threshold == -1:
        cols = np.arange(hits.shape[1]) if mask is None else np.flatnonzero(mask)
        keep = score == _rounded(hits[:, cols].max(axis=1), nk)
    else:
        keep = score >= threshold
    return (keep & (np.asarray(nk) > 0)).astype(np.uint8)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to("cuda")


def _keep_device(xs, torch, hits, nk, D, label, threshold, mask=None, byte=0x5A):
    """filter_keep_device into poisoned, guarded outputs: (keep, label_hits)."""
    n = len(nk)
    keep = DevGuarded(torch, n, np.uint8, byte, 1)
    lh = DevGuarded(torch, n, np.uint32, byte, 1)
    d_mask = _dev(torch, np.asarray(mask, dtype=np.uint8)) if mask is not None else None
    xs.filter_keep_device(_dev(torch, np.asarray(hits, dtype=np.uint32)) if n else None,
                          _dev(torch, np.asarray(nk, dtype=np.uint64)) if n else None, n, D, label, threshold,
                          keep.ptr, lh.ptr, d_mask)
    torch.cuda.synchronize()
    return keep.check("keep"), lh.check("label_hits")


# ---------------------------------------------------------------- 1. the keep kernel, exhaustive
@pytest.fixture(scope="module")
def pairs():
    h, n = [], []
    for b in range(1, 301):
        h += range(b + 1)
        n += [b] * (b + 1)
    rng = np.random.default_rng(5)
    big = np.concatenate([rng.integers(1 << 20, 10**7 + 1, 1000), (1 << 32) + rng.integers(0, 1000, 1000)])
    bh = (rng.random(2000) * (np.minimum(big, (1 << 32) - 1) + 1)).astype(np.uint64)
    bh[:200] = np.minimum(big[:200], (1 << 32) - 1)   # h = n (score 1.0) where it fits
    h, n = np.array(h + bh.tolist(), dtype=np.uint64), np.array(n + big.tolist(), dtype=np.uint64)
    assert (h <= n).all() and h.max() < 1 << 32 and len(h) == 45_450 + 2000
    return h, n, _rounded(h, n)


def test_keep_kernel_every_pair_one_column(xs, torch, pairs):
    h, n, score = pairs
    d_h, d_n = _dev(torch, h.astype(np.uint32)), _dev(torch, n)
    d_keep = torch.empty(len(h), dtype=torch.uint8, device="cuda")
    for t in THRESHOLDS:
        d_keep.fill_(0x5A)
        xs.filter_keep_device(d_h, d_n, len(h), 1, 0, t, d_keep)
        want = np.ones(len(h), dtype=np.uint8) if t == -1 else (score >= t).astype(np.uint8)
        got = d_keep.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (t, [(int(h[i]), int(n[i]), int(got[i])) for i in bad[:5]])


def test_keep_kernel_every_pair_three_columns(xs, torch, pairs):
    """The label between h - 1 and h + 1 (clipped to [0, n]): the column is picked
    by index, and in max mode a neighbour one hit above decides."""
    h, n, score = pairs
    cap = np.minimum(n, (1 << 32) - 1)
    rows = np.stack([np.where(h > 0, h - 1, 0), h, np.minimum(h + 1, cap)], axis=1).astype(np.uint32)
    d_rows, d_n = _dev(torch, rows), _dev(torch, n)
    d_keep = torch.empty(len(h), dtype=torch.uint8, device="cuda")
    d_lh = torch.empty(len(h), dtype=torch.int32, device="cuda")
    top = _rounded(rows.max(axis=1), n)
    for t in THRESHOLDS:
        d_keep.fill_(0x5A)
        xs.filter_keep_device(d_rows, d_n, len(h), 3, 1, t, d_keep, d_lh)
        want = (score == top) if t == -1 else (score >= t)
        got = d_keep.cpu().numpy()
        bad = np.flatnonzero(got != want.astype(np.uint8))
        assert bad.size == 0, (t, [(rows[i].tolist(), int(n[i]), int(got[i])) for i in bad[:5]])
    assert np.array_equal(d_lh.cpu().numpy().view(np.uint32), rows[:, 1])
    assert 0 < int(((score == top) & (rows[:, 2] > rows[:, 1])).sum()) < len(h)  # both outcomes occur


def test_keep_kernel_named_cases(xs, torch):
    """The four binary halves go to the even centi-value, as Python rounds them;
    150 and 151 of 300 both round to 0.5, so the label ties the maximum."""
    assert [round(x, 2) for x in (1 / 8, 3 / 8, 5 / 8, 7 / 8)] == [0.12, 0.38, 0.62, 0.88]
    h, n = [1, 3, 5, 7], [8, 8, 8, 8]
    for t, want in ((0.12, [1, 1, 1, 1]), (0.13, [0, 1, 1, 1]), (0.38, [0, 1, 1, 1]), (0.39, [0, 0, 1, 1]),
                    (0.62, [0, 0, 1, 1]), (0.63, [0, 0, 0, 1]), (0.88, [0, 0, 0, 1]), (0.89, [0, 0, 0, 0])):
        got, _ = _keep_device(xs, torch, h, n, 1, 0, t)
        assert got.tolist() == want == _expected(h, n, 0, t).tolist(), t
    rows = [[150, 151], [151, 150], [148, 151]]
    assert round(150 / 300, 2) == round(151 / 300, 2) == 0.5 != round(148 / 300, 2)
    got, lh = _keep_device(xs, torch, rows, [300] * 3, 2, 0, -1)
    assert got.tolist() == [1, 1, 0] and lh.tolist() == [150, 151, 148]


# ---------------------------------------------------------------- 2. row shapes and masks
@pytest.mark.parametrize("D", [1, 2, 16, 17, 100, 129])  # 16 | 17: a thread | a wavefront per row in max mode
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_keep_kernel_shapes_masks_and_empty_reads(xs, torch, D, n):
    rng = np.random.default_rng([D, n])
    nk = rng.integers(1, 200, n).astype(np.uint64)
    nk[rng.random(n) < 0.1] = 0                                  # reads without k-mers are never kept
    hits = (rng.random((n, D)) * (nk[:, None] + 1)).astype(np.uint32)
    label = D // 2
    for byte, t in zip(pl.POISON_BYTES, (0.5, -1)):
        keep, lh = _keep_device(xs, torch, hits, nk, D, label, t, byte=byte)
        assert np.array_equal(keep, _expected(hits, nk, label, t)), (D, n, t)
        assert np.array_equal(lh, hits[:, label])
    if D > 1 and n:
        # one column holds every row's maximum and the label the largest of the rest: masked out, the
        # label is the maximum
        top = D - 1 if label != D - 1 else 0
        hits[:, top] = 0
        hits[:, label] = hits.max(axis=1)
        hits[:, top] = nk.astype(np.uint32)
        mask = np.ones(D, dtype=np.uint8)
        mask[top] = 0
        keep, _ = _keep_device(xs, torch, hits, nk, D, label, -1, mask)
        want = _expected(hits, nk, label, -1, mask)
        assert np.array_equal(keep, want)
        assert not np.array_equal(want, _expected(hits, nk, label, -1)) or n == 1
        mask[:] = 1
        mask[label] = 0
        with pytest.raises(xs._lib.XsError) as e:
            _keep_device(xs, torch, hits, nk, D, label, -1, mask)
        assert e.value.code == xs._lib.XS_ERR_ARG


# ---------------------------------------------------------------- 3. compaction
B = 1024  # the scan's block size; test_filter_cuts.py holds it to the kernel's constant

PATTERNS = ("none", "all", "alternating", "last", "p01", "p50", "p99")


def _pattern(name, n, rng):
    if name == "none":
        return np.zeros(n, dtype=np.uint8)
    if name == "all":
        return np.ones(n, dtype=np.uint8)
    if name == "alternating":
        return (np.arange(n) & 1).astype(np.uint8)
    if name == "last":
        k = np.zeros(n, dtype=np.uint8)
        k[-1:] = 1
        return k
    return (rng.random(n) < int(name[1:]) / 100).astype(np.uint8) * np.uint8(rng.integers(1, 256))  # any non-zero byte


def _compact(xs, torch, keep, offs, byte):
    n = len(keep)
    idx = DevGuarded(torch, n, np.uint32, byte, 1)
    out = DevGuarded(torch, n + 1, np.uint64, byte, 1)
    cnt = DevGuarded(torch, 2, np.uint64, byte, 0)
    xs.filter_compact_device(_dev(torch, keep) if n else None, _dev(torch, offs), n, idx.ptr, out.ptr, cnt.ptr)
    torch.cuda.synchronize()
    return idx.check("index"), out.check("out_offsets"), cnt.check("counts")


def _check_compact(got, keep, offs, byte):
    idx, out, cnt = got
    want_idx = np.flatnonzero(keep).astype(np.uint32)
    m = want_idx.size
    want_out = np.zeros(m + 1, dtype=np.uint64)
    np.cumsum(np.diff(offs)[want_idx], out=want_out[1:])
    assert cnt.tolist() == [m, int(want_out[-1])]
    assert np.array_equal(idx[:m], want_idx) and np.array_equal(out[:m + 1], want_out)
    assert (idx[m:] == pl.poison_of(byte, np.uint32)).all(), "index written past m"
    assert (out[m + 1:] == pl.poison_of(byte, np.uint64)).all(), "out_offsets written past m + 1"


@pytest.mark.parametrize("n", [0, 1, B - 1, B, B + 1, B * B + 1])
def test_compaction_equals_flatnonzero_and_cumsum(xs, torch, n):
    assert B == xs.FILTER_COMPACT_BLOCK
    rng = np.random.default_rng(n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(rng.integers(0, 300, n), out=offs[1:])
    offs += np.uint64(17)  # offsets need not start at 0
    for i, name in enumerate(PATTERNS):
        keep = _pattern(name, n, rng)
        byte = pl.POISON_BYTES[i & 1]
        _check_compact(_compact(xs, torch, keep, offs, byte), keep, offs, byte)


def test_compaction_holds_64_bit_sums(xs, torch):
    """Four reads of 2^31 bytes: only the offsets are read, so no text is needed."""
    offs = (np.arange(5, dtype=np.uint64) << np.uint64(31))
    for keep in ([1, 1, 1, 1], [0, 1, 0, 1]):
        keep = np.array(keep, dtype=np.uint8)
        got = _compact(xs, torch, keep, offs, 0xFF)
        _check_compact(got, keep, offs, 0xFF)
    assert got[2].tolist() == [2, 1 << 32]


# ---------------------------------------------------------------- 4. Bank.query_keep against oracle rows
def _query_keep_guarded(bank, pr, step, label, threshold, mask, byte):
    """xs_query_keep through ctypes with every output poisoned between guards."""
    from xspect2_amd._lib import check, load
    n, D = pr.n, bank.num_docs
    room = max(n, 1)  # n = 0: one element each, which has to stay as it is
    keep = pl.GuardedArray(room, np.uint8, byte, 1)
    lh = pl.GuardedArray(room, np.uint32, byte, 4)
    nk = pl.GuardedArray(room, np.uint64, byte, 8)
    tot = pl.GuardedArray(D + 1, np.uint64, byte, 8)
    check(load().xs_query_keep(bank.handle, pr.buf.ctypes.data, pr.offsets.ctypes.data, n, step, label,
                               mask.ctypes.data if mask is not None else None, float(threshold), keep.ptr, lh.ptr,
                               nk.ptr, tot.ptr))
    return keep.check("keep"), lh.check("label_hits"), nk.check("num_kmers"), tot.check("totals")


def _check_query_keep(bank, seqs, rows, nks, label, mask=None, ranges=False):
    from xspect2_amd._lib import XS_PATH_PARTITIONED
    from xspect2_amd.packing import pack_sequences
    pr = pack_sequences(seqs)
    for step in (1, 3):
        want_rows, want_nk = rows[step], nks[step]
        want_tot = np.append(want_rows.sum(axis=0, dtype=np.uint64), want_nk.sum(dtype=np.uint64))
        for byte, t in zip(pl.POISON_BYTES, (0.7, -1)):
            if ranges:
                bank.pass_stats()
            keep, lh, nk, tot = _query_keep_guarded(bank, pr, step, label, t, mask, byte)
            assert np.array_equal(nk, want_nk) and np.array_equal(lh, want_rows[:, label])
            assert np.array_equal(tot, want_tot)
            assert np.array_equal(keep, _expected(want_rows, want_nk, label, t, mask)), (step, t)
            if ranges:
                assert bank.probe_path() == XS_PATH_PARTITIONED and bank.pass_stats()["lookup"][1] >= 2
        got = bank.query_keep(pr, label, 0.7, step, doc_mask=mask, want_totals=True)
        assert np.array_equal(got[0], _expected(want_rows, want_nk, label, 0.7, mask)) and np.array_equal(got[3], want_tot)
    empty = _query_keep_guarded(bank, pack_sequences([]), 1, label, 0.7, mask, 0x5A)
    assert not empty[3].any()
    assert [int(a[0]) for a in empty[:3]] == [pl.poison_of(0x5A, t) for t in (np.uint8, np.uint32, np.uint64)]


def test_query_keep_equals_oracle_rows(models, oracle_mod):  # noqa: F811
    import fastx as ofx
    from xspect2_amd.classify import genus_model_path, species_model_path
    from xspect2_amd.probabilistic_filter_model import training_files
    from xspect2_amd.probabilistic_filter_svm_model import ProbabilisticFilterSVMModel
    from xspect2_amd.probabilistic_single_filter_model import ProbabilisticSingleFilterModel

    tmp_path, genomes, gfa, sdir = models
    seqs = [s for _, s in ofx.parse_file(_reads(tmp_path, genomes, "fq", False))]
    gseqs = [s for _, s in ofx.parse_file(gfa)]
    nbytes, Kh = oracle_mod.BloomFilter.params(sum(map(len, gseqs)) - K + 1, 0.01)
    bf = oracle_mod.BloomFilter(np.zeros(nbytes, dtype=np.uint8), Kh, K)
    bf.build(gseqs)
    files = training_files(sdir)
    docs = [s for f in files for _, s in ofx.parse_file(f)]
    D = len(files)
    ob = oracle_mod.CobsBank.empty([oracle_mod.signature_size(max(len(s) - K + 1 for s in docs), 7, 0.01)],
                                   (D + 7) // 8, D, 7, K)
    ob.build(docs, list(range(D)))
    grows, gnks, srows, snks = {}, {}, {}, {}
    for step in (1, 3):
        h, n = bf.query(seqs, step=step)
        grows[step], gnks[step] = np.asarray(h, dtype=np.uint32).reshape(-1, 1), np.asarray(n, dtype=np.uint64)
        h, n = ob.query(seqs, step=step)
        srows[step], snks[step] = np.asarray(h, dtype=np.uint32).reshape(-1, D), np.asarray(n, dtype=np.uint64)

    genus = ProbabilisticSingleFilterModel.load(genus_model_path("Acinetobacter"))
    species = ProbabilisticFilterSVMModel.load(species_model_path("Acinetobacter"))
    try:
        mask = np.array([1, 0, 1, 1], dtype=np.uint8)
        for small in (1, 0):  # 400 reads: the one-round-trip call, then the chunked pipeline
            genus.bf.set_probe_options(small_calls=small)
            species.index.set_probe_options(small_calls=small)
            _check_query_keep(genus.bf, seqs, grows, gnks, 0)
            _check_query_keep(species.index, seqs, srows, snks, 2)
            _check_query_keep(species.index, seqs, srows, snks, 0, mask)
        # a workspace small enough that the partitioned probe runs in ranges
        species.index.set_probe_options(cobs_part=3, workspace_mib=1)
        species.index.set_profiling(True)
        _check_query_keep(species.index, seqs * 4, {s: np.tile(r, (4, 1)) for s, r in srows.items()},
                          {s: np.tile(v, 4) for s, v in snks.items()}, 1, ranges=True)
        species.index.set_profiling(False)
        # the model call on the same reads: ids, keep and the reference's id list
        inp = _reads(tmp_path, genomes, "fq", False)
        name = files[2].stem
        res = species.filter_columnar(inp, name, 0.7)
        assert np.array_equal(res.keep, _expected(srows[1], snks[1], 2, 0.7))
        assert res.kept_ids() == species.predict_columnar(inp).get_filtered_subsequence_labels(name, 0.7)
        nan = species.filter_columnar(inp, name, float("nan"))  # passes the reference's range check, keeps nothing
        assert not nan.keep.any() and nan.kept_ids() == [] and len(nan) == len(seqs)
        assert np.array_equal(nan.label_hits, srows[1][:, 2]) and np.array_equal(nan.num_kmers, snks[1])
        with pytest.raises(KeyError):
            species.filter_columnar(inp, name, 0.7, exclude_ids=[name])
        with pytest.raises(ValueError, match="between 0 and 1"):
            species.filter_columnar(inp, name, 1.5)
    finally:
        genus.close()
        species.close()


# ---------------------------------------------------------------- 5. filter_genus / filter_species in one pass
CASES = [("fa", 0.0, 1), ("fq", 0.7, 1), ("fq", 1.0, 2), ("fa", -1, 2)]


def _fa(tmp_path, genomes, fmt, dup, name):
    p = _reads(tmp_path, genomes, "fasta" if fmt == "fa" else fmt, dup, name=name)
    return p.rename(p.with_suffix(".fa")) if fmt == "fa" else p


def _same_file(a, b):
    assert a.exists() == b.exists()
    assert not a.exists() or a.read_bytes() == b.read_bytes()
    assert not a.with_name(a.name + ".partial").exists()


def test_one_pass_filter_equals_two_pass(models, monkeypatch):  # noqa: F811
    from xspect2_amd import filter_sequences as fs
    from xspect2_amd.probabilistic_filter_model import ProbabilisticFilterModel
    from xspect2_amd.probabilistic_filter_svm_model import ProbabilisticFilterSVMModel

    tmp_path, genomes, _, _ = models
    out = tmp_path / "out"
    out.mkdir()
    for i, (fmt, t, step) in enumerate(CASES):  # the two-pass files first (they need predict_columnar)
        inp = _fa(tmp_path, genomes, fmt, False, f"r{i}")
        fs.filter_genus("Acinetobacter", inp, out / f"g2_{i}.fasta", t, out / f"g_{i}.json", step)
        fs.filter_species("Acinetobacter", "471", inp, out / f"s2_{i}.fasta", t, out / f"s_{i}.json", step)

    def no_matrix(*a, **k):
        raise AssertionError("the one-pass path must not bring the hit matrix to the host")

    with monkeypatch.context() as mp:
        mp.setattr(ProbabilisticFilterModel, "predict_columnar", no_matrix)
        mp.setattr(ProbabilisticFilterSVMModel, "predict_columnar", no_matrix)
        for i, (fmt, t, step) in enumerate(CASES):
            inp = tmp_path / f"r{i}.{fmt}"
            fs.filter_genus("Acinetobacter", inp, out / f"g1_{i}.fasta", t, None, step)
            fs.filter_species("Acinetobacter", "471", inp, out / f"s1_{i}.fasta", t, sparse_sampling_step=step)
    kept = 0
    for i in range(len(CASES)):
        _same_file(out / f"g1_{i}.fasta", out / f"g2_{i}.fasta")
        _same_file(out / f"s1_{i}.fasta", out / f"s2_{i}.fasta")
        kept += (out / f"g1_{i}.fasta").exists() + (out / f"s1_{i}.fasta").exists()
    assert kept >= 6


def test_one_pass_filter_falls_back_and_fails_like_the_reference(models, monkeypatch, capsys):  # noqa: F811
    from xspect2_amd import filter_sequences as fs
    from xspect2_amd.probabilistic_filter_model import ProbabilisticFilterModel

    tmp_path, genomes, _, _ = models
    out = tmp_path / "out"
    out.mkdir()
    dup = _fa(tmp_path, genomes, "fq", True, "dup")  # repeated ids: filtered by id over the whole file
    calls = []
    real = ProbabilisticFilterModel.predict_columnar
    monkeypatch.setattr(ProbabilisticFilterModel, "predict_columnar",
                        lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    fs.filter_genus("Acinetobacter", dup, out / "d1.fasta", 0.7)
    assert calls == [1]
    fs.filter_genus("Acinetobacter", dup, out / "d2.fasta", 0.7, out / "d.json")
    _same_file(out / "d1.fasta", out / "d2.fasta")
    assert "Saved filtered sequences from dup.fq as d1.fasta" in capsys.readouterr().out
    # nothing kept: the reference's message and no file
    rng = np.random.default_rng(1)
    foreign = tmp_path / "foreign.fa"
    foreign.write_text("".join(f">f{i}\n{''.join(rng.choice(list('ACGT'), 120))}\n" for i in range(50)))
    fs.filter_genus("Acinetobacter", foreign, out / "none.fasta", 0.7)
    assert "No sequences found for the given genus in foreign.fa." in capsys.readouterr().out
    assert not (out / "none.fasta").exists() and not (out / "none.fasta.partial").exists()
    # a read of length k, after reads that are kept
    short = tmp_path / "short.fa"
    short.write_text(f">ok\n{genomes[0][:150]}\n>short\n{genomes[0][:K]}\n")
    with pytest.raises(ValueError, match="Invalid sequence, must be longer than k"):
        fs.filter_genus("Acinetobacter", short, out / "short.fasta", 0.7)
    assert not (out / "short.fasta").exists() and not (out / "short.fasta.partial").exists()


# ---------------------------------------------------------------- 6. the fused pipeline's hand-off
def test_pipeline_hand_off_on_the_device(tmp_path):
    from test_pipeline import _models
    from xspect2_amd.file_io import read_batches
    from xspect2_amd.pipeline import reference_pipeline, run_pipeline

    genus, species, gtxt = _models(tmp_path, 21, 21)
    rng = np.random.default_rng(9)
    inp = tmp_path / "reads.fq"
    with open(inp, "w") as fh:
        for i in range(1200):
            if 300 <= i < 900:  # foreign reads: no genus k-mer, none kept
                rid, seq = f"x{i}", "".join(rng.choice(list("ACGT"), 150))
            else:
                s = int(rng.integers(0, 29_000))
                rid, seq = f"g{i}", gtxt[i % 2][s:s + 150]
            fh.write(f"@{rid}\n{seq}\n+\n{'I' * 150}\n")
    batch_bytes = inp.stat().st_size // 5 + 1
    per_batch = [b.ids() for b in read_batches(inp, batch_bytes)]
    assert len(per_batch) >= 3 and any(all(r.startswith("x") for r in ids) for ids in per_batch)
    got = run_pipeline(genus, species, inp, tmp_path / "fused", threshold=0.7, run_id="r1", batch_bytes=batch_bytes,
                       log=lambda *a: None)
    want = reference_pipeline(genus, species, inp, tmp_path / "ref", threshold=0.7, run_id="r1", log=lambda *a: None)
    for key in ("genus", "filtered", "species"):
        assert [p.name for p in got[key]] == [p.name for p in want[key]] and got[key], key
        for a, b in zip(got[key], want[key]):
            assert a.read_bytes() == b.read_bytes(), (key, a.name)
    assert got["filtered"][0].read_bytes().count(b">") >= 500
    genus.close()
    species.close()
