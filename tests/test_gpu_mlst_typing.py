"""MLST typing on the device (GPU): the per-row top-allele reduction
(xs_mlst_top_device) against numpy, xs_mlst_type / xs_mlst_type_device against
the CPU oracle's hit rows, the bounded workspace of the chunked call, and
``predict_columnar`` of the MLST model against ``predict``.

The rule (include/xspect_hip.h): top = the lowest doc holding the row's
maximum, top_score = that maximum, n_tied = the docs holding it; every value is
an integer and compared exactly."""
from __future__ import annotations

import json

import numpy as np
import pytest

from xspect2_amd.file_io import Record, get_record_iterator, write_fasta

pytestmark = pytest.mark.gpu

K = 21
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def xs():
    from xspect2_amd import _lib
    from xspect2_amd import bank as bank_mod
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bank_mod


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _expected(rows: np.ndarray):
    """(top, top_score, n_tied) of uint32 rows: np.argmax returns the first maximum."""
    rows = np.asarray(rows, dtype=np.uint32)
    m = rows.max(axis=1)
    return rows.argmax(axis=1).astype(np.uint32), m, (rows == m[:, None]).sum(axis=1).astype(np.uint32)


def _to_dev(torch_dev, a: np.ndarray):
    torch, dev = torch_dev
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).to(dev)


def _reduce(xs, torch_dev, d_hits, n, D, out_stride=1, want_tied=True):
    """xs_mlst_top_device over a flat device tensor; outputs prefilled with SENTINEL, whole arrays back."""
    torch, dev = torch_dev
    outs = [torch.full((max(n * out_stride, 1),), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]
    s = torch.cuda.current_stream(dev).cuda_stream
    xs.mlst_top_device(d_hits, n, D, outs[0], outs[1], outs[2] if want_tied else None, out_stride, stream=s)
    torch.cuda.synchronize(dev)
    return [o.cpu().numpy().view(np.uint32)[:n * out_stride] for o in outs]


@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 127, 258, 1430])
def test_top_kernel_matches_numpy(xs, torch_dev, D):
    """Seeded random uint32 rows, n = 1, 5 and 257 (more than one block's waves):
    half the rows over the whole uint32 range, half over 0..3 so that maxima tie;
    with out_stride 3 only every third output element may change; n_tied may be null."""
    rng = np.random.default_rng(1000 + D)
    for n in (1, 5, 257):
        rows = rng.integers(0, 1 << 32, (n, D), dtype=np.uint64).astype(np.uint32)
        rows[1::2] = rng.integers(0, 4, rows[1::2].shape)
        want = _expected(rows)
        d_hits = _to_dev(torch_dev, rows)
        for got, exp in zip(_reduce(xs, torch_dev, d_hits, n, D), want):
            assert np.array_equal(got, exp), (n, D)
        strided = _reduce(xs, torch_dev, d_hits, n, D, out_stride=3)
        for got, exp in zip(strided, want):
            assert np.array_equal(got[0::3], exp), (n, D)
            assert (got[1::3] == SENTINEL).all() and (got[2::3] == SENTINEL).all(), (n, D)
        top, score, tied = _reduce(xs, torch_dev, d_hits, n, D, want_tied=False)
        assert np.array_equal(top, want[0]) and np.array_equal(score, want[1]) and (tied == SENTINEL).all()


def test_top_kernel_crafted_rows(xs, torch_dev):
    """Rows made to break a wrong reduction: all zero (top 0, n_tied D); the
    maximum only in the last doc; equal maxima in docs 6 and 70 (one lane at
    stride 64) and in docs 70 and 5 (two lanes); counts >= 2^31 and 0xFFFFFFFF
    beside smaller ones (a signed compare orders them last)."""
    D = 131
    rows = np.zeros((7, D), dtype=np.uint32)
    rows[1, D - 1] = 9
    rows[2, [6, 70]] = 40
    rows[2, 100] = 39
    rows[3, [70, 5]] = 17
    rows[4, :] = 5
    rows[4, 9] = 0xFFFFFFFF
    rows[5, 1] = 0x7FFFFFFF
    rows[5, 3] = 0x80000000
    rows[6, :] = 0x80000001
    rows[6, [2, 64, 130]] = 0xFFFFFFFE
    want = _expected(rows)
    assert want[0].tolist() == [0, D - 1, 6, 5, 9, 3, 2] and want[2].tolist() == [D, 1, 2, 2, 1, 1, 3]
    for got, exp in zip(_reduce(xs, torch_dev, _to_dev(torch_dev, rows), 7, D), want):
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("D", [5, 64, 1430])
def test_top_kernel_unaligned_base(xs, torch_dev, D):
    """A matrix whose first count lies 1, 2 or 3 counts past a 16-byte boundary
    (a slice of a larger tensor): every row's head peel differs from the aligned case."""
    rng = np.random.default_rng(77 + D)
    n = 9
    rows = rng.integers(0, 6, (n, D), dtype=np.uint64).astype(np.uint32)
    rows[0, D - 1] = 7
    rows[1, 0] = 7
    want = _expected(rows)
    for off in (1, 2, 3):
        flat = np.full(off + n * D + 8, 0xFFFFFFFF, dtype=np.uint32)  # a read outside the slice would win
        flat[off:off + n * D] = rows.reshape(-1)
        big = _to_dev(torch_dev, flat)
        assert big.data_ptr() % 16 == 0
        for got, exp in zip(_reduce(xs, torch_dev, big[off:off + n * D], n, D), want):
            assert np.array_equal(got, exp), (D, off)


# ---------------------------------------------------------------- xs_mlst_type against the oracle
LOCUS_DOCS = (40, 70, 130)
PAGE = 2  # 16 alleles per doc group


def _alleles(rng, D, length):
    base = rng.integers(0, 4, length)
    out = []
    for _ in range(D):
        a = base.copy()
        pos = rng.choice(length, size=int(rng.integers(0, 12)), replace=False)
        a[pos] = (a[pos] + 1) % 4
        out.append(np.frombuffer(b"ACGT", dtype=np.uint8)[a].tobytes())
    return out


def _scheme_data(oracle_mod, seed=20261020):
    """Three compact loci built by the oracle, the reads, and per step and locus the
    oracle's hit rows with their expected (top, top_score, n_tied); computed once."""
    rng = np.random.default_rng(seed)
    obs, alleles = [], []
    for li, D in enumerate(LOCUS_DOCS):
        al = _alleles(rng, D, 450 + 10 * li)
        terms = len(al[0]) - K + 1
        sig = [oracle_mod.signature_size(terms, 1, 0.001)] * ((D + 8 * PAGE - 1) // (8 * PAGE))
        ob = oracle_mod.CobsBank.empty(sig, PAGE, D, 1, K)
        ob.build(al, list(range(D)))
        obs.append((ob, sig))
        alleles.append(al)

    def window():
        al = alleles[int(rng.integers(0, 3))]
        a = al[int(rng.integers(0, len(al)))]
        st = int(rng.integers(0, len(a) - 150 + 1))
        return a[st:st + 150]

    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = [window() for _ in range(200)]
    reads += [acgt[rng.integers(0, 4, 150)].tobytes() for _ in range(90)]
    reads += [b"", b"ACGTA", b"A" * (K - 1), acgt[rng.integers(0, 4, K - 1)].tobytes()]  # no k-mers
    long_read = alleles[0][3] + alleles[1][5] + alleles[2][7] + alleles[0][9]
    reads.insert(137, long_read + acgt[rng.integers(0, 4, 2000 - len(long_read))].tobytes())  # 2 kbp: several work units
    many = [window() for _ in range(2000)]
    want = {}
    for step in (1, 3):
        rows = [ob.query(reads, step=step) for ob, _ in obs]
        want[step] = ([r[0] for r in rows], rows[0][1])
    return {"obs": obs, "alleles": alleles, "reads": reads, "many": many, "want": want}


@pytest.fixture(scope="module")
def scheme(oracle_mod):
    return _scheme_data(oracle_mod)


def _banks(xs, scheme, upload=True):
    """The loci on the device: the oracle's images uploaded, or (upload=False) built there from
    the alleles, which stages a few tens of KB where an upload stages the whole image."""
    out = []
    for (ob, sig), al, D in zip(scheme["obs"], scheme["alleles"], LOCUS_DOCS):
        gb = xs.Bank.create_cobs(K, 1, sig, D, [f"Allele_ID_{i + 1}" for i in range(D)], page_size=PAGE, compact=True)
        if upload:
            gb.upload(ob.rows)
        else:
            gb.build(al, np.arange(D, dtype=np.uint32))
        out.append(gb)
    return out


@pytest.fixture(scope="module")
def banks(xs, scheme):
    b = _banks(xs, scheme)
    yield b
    for gb in b:
        gb.close()


def _check_typing(got, rows_per_locus, num_kmers):
    top, score, tied, nk = got
    assert top.shape == score.shape == tied.shape == (len(num_kmers), len(rows_per_locus))
    for l, rows in enumerate(rows_per_locus):
        wt, ws, wn = _expected(rows)
        assert np.array_equal(top[:, l], wt) and np.array_equal(score[:, l], ws) and np.array_equal(tied[:, l], wn), l
    assert np.array_equal(nk, num_kmers)


def test_inputs_exercise_the_rule(scheme):
    """On the oracle's rows, not on the output under test: some row has a non-zero
    maximum shared by several alleles, some row's top is not doc 0, some row is all zero."""
    assert len(scheme["reads"]) == 295  # chunks of 100 reads: 100, 100 and a ragged 95
    for step in (1, 3):
        rows_per_locus, nk = scheme["want"][step]
        assert (nk == 0).sum() == 4 and nk.max() == (2000 - K) // step + 1
        for rows in rows_per_locus:
            top, score, tied = _expected(rows)
            assert ((tied > 1) & (score > 0)).any()
            assert (top != 0).any()
            assert ((score == 0) & (tied == rows.shape[1])).any()


@pytest.mark.parametrize("step", [1, 3])
def test_mlst_type_matches_oracle(xs, scheme, banks, step):
    rows_per_locus, nk = scheme["want"][step]
    _check_typing(xs.mlst_type(banks, scheme["reads"], step=step), rows_per_locus, nk)


def test_mlst_type_chunked_equals_unchunked(xs, scheme, banks):
    """workspace_bytes of 100 rows of the widest locus: chunks of 100, 100 and 95
    reads; workspace_bytes = 1: one read per chunk (the first 20 reads)."""
    reads = scheme["reads"]
    whole = xs.mlst_type(banks, reads)
    rows_per_locus, nk = scheme["want"][1]
    _check_typing(whole, rows_per_locus, nk)
    chunked = xs.mlst_type(banks, reads, workspace_bytes=100 * 130 * 4)
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)
    single = xs.mlst_type(banks, reads[:20], workspace_bytes=1)
    for a, b in zip(whole, single):
        assert np.array_equal(a[:20], b)


def test_mlst_type_workspace_is_bounded(xs, scheme):
    """2,000 reads in chunks of 100 on fresh handles (built on the device: an upload
    would stage each locus' whole image in the workspace): all the device workspace
    the loci ever held, their builds included (reads, offsets, outputs, the rows
    buffer), stays below the 2,000 x 130 x 4 bytes one locus' whole hit matrix takes."""
    fresh = _banks(xs, scheme, upload=False)
    try:
        reads = scheme["many"]
        got = xs.mlst_type(fresh, reads, workspace_bytes=100 * 130 * 4)
        peaks = [gb.workspace_bytes()[1] for gb in fresh]
        print("workspace peaks", peaks, "bound", len(reads) * 130 * 4)
        assert 0 < sum(peaks) < len(reads) * 130 * 4, peaks
        rows = [ob.query(reads)[0] for ob, _ in scheme["obs"]]
        _check_typing(got, rows, np.full(len(reads), 150 - K + 1, dtype=np.uint64))
    finally:
        for gb in fresh:
            gb.close()


def test_mlst_type_device_reads(xs, scheme, banks, torch_dev):
    """Reads already in HBM (two torch tensors) give what the host reads give, chunked or not."""
    torch, dev = torch_dev
    from xspect2_amd.packing import pack_sequences
    pr = pack_sequences(scheme["reads"])
    d_seqs = torch.from_numpy(pr.buf.copy()).to(dev)
    d_offs = torch.from_numpy(pr.offsets.astype(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    dr = xs.DeviceReads(d_seqs, pr.nbytes, d_offs, pr.n)
    host = xs.mlst_type(banks, pr, step=3)
    for ws in (0, 100 * 130 * 4):
        for a, b in zip(host, xs.mlst_type(banks, dr, step=3, workspace_bytes=ws)):
            assert np.array_equal(a, b), ws


def test_mlst_type_argument_errors(xs, banks):
    """Loci that cannot be typed together are XS_ERR_ARG: the same handle twice,
    another k, an rbloom bank; no reads is not an error."""
    from xspect2_amd._lib import XsError
    reads = [b"ACGT" * 40]
    with pytest.raises(XsError, match="same handle"):
        xs.mlst_type([banks[0], banks[1], banks[0]], reads)
    other_k = xs.Bank.create_cobs(31, 1, [1000], 8, None, page_size=1, compact=True)
    bloom = xs.Bank.create_bloom(K, 1024, 3)
    try:
        with pytest.raises(XsError, match="another k"):
            xs.mlst_type([banks[0], other_k], reads)
        with pytest.raises(XsError, match="COBS"):
            xs.mlst_type([banks[0], bloom], reads)
    finally:
        other_k.close()
        bloom.close()
    with pytest.raises(ValueError):
        xs.mlst_type(banks, reads, step=0)
    top, score, tied, nk = xs.mlst_type(banks, [])
    assert top.shape == score.shape == tied.shape == (0, 3) and nk.shape == (0,)


# ---------------------------------------------------------------- the model
def _scheme_dir(tmp_path, rng, loci=3, alleles=40):
    root = tmp_path / "alleles"
    for li in range(loci):
        base = "".join(rng.choice(list("ACGT"), 450 + 10 * li))
        for a in range(1, alleles + 1):
            s = list(base)
            for p in rng.choice(len(s), size=int(rng.integers(0, 12)), replace=False):
                s[p] = "ACGT"[(("ACGT".index(s[p])) + 1) % 4]
            write_fasta([Record(f"L{li}_{a}", "".join(s))], root / f"Oxf_L{li}" / f"Allele_ID_{a}.fasta")
    return root


def test_predict_columnar_matches_predict(tmp_path):
    """Allele windows, whole alleles, a 12 kbp contig of alleles and a 12 kbp
    random contig ("N/A" at every locus) in one FASTA: for every record
    ``predict_columnar(path).strain_type(i, ...)`` is ``predict(path)``'s
    "Strain type" dict, ``sufficient`` says whether it carries "ST_Name", and
    ``resolve_unique`` asks the resolver once per distinct sufficient profile."""
    from xspect2_amd._lib import XS_MLST_NONE
    from xspect2_amd.probabilistic_filter_mlst_model import ProbabilisticFilterMlstSchemeModel

    rng = np.random.default_rng(5)
    root = _scheme_dir(tmp_path, rng)
    url = "https://example/schemes/1"
    m = ProbabilisticFilterMlstSchemeModel(K, "MLST (Oxford)", tmp_path / "xspect_data", url, "abaumannii")
    calls = []

    def resolver(flat, scheme_url):
        calls.append((tuple(flat.items()), scheme_url))
        return "ST" + "-".join(str(v) for v in flat.values())

    m.strain_type_resolver = resolver
    m.fit(root, page_size=2)

    def allele(li, a):
        return next(get_record_iterator(root / f"Oxf_L{li}" / f"Allele_ID_{a}.fasta")).seq

    records = []
    for i in range(24):
        a = allele(i % 3, int(rng.integers(1, 41)))
        st = int(rng.integers(0, len(a) - 150 + 1))
        records.append(Record(f"w{i}", a[st:st + 150]))
    records += [Record(f"a{li}_{a}", allele(li, a)) for li in range(3) for a in (4, 17)]
    records.append(Record("a0_4_again", allele(0, 4)))
    contig = "".join(allele(li, 7) + "A" * 3000 for li in range(3))
    records.insert(9, Record("contig", contig))
    records.append(Record("random_contig", "".join(rng.choice(list("ACGT"), 12_000))))
    assert len(contig) >= 10_000
    fa = tmp_path / "input.fasta"
    write_fasta(records, fa)

    want = m.predict(fa).hits
    n_predict_calls = len(calls)
    got = m.predict_columnar(fa)
    assert len(calls) == n_predict_calls  # typing alone resolves nothing
    assert list(got.ids) == [r.id for r in records] and got.loci == list(m.loci)
    assert got.locus_size == m.avg_locus_bp_size and got.steps == 1
    for i, rec in enumerate(records):
        st = want[rec.id][0]["Strain type"]
        assert got.strain_type(i, resolver, url) == st, rec.id
        assert bool(got.sufficient[i]) == ("ST_Name" in st), rec.id
    assert got.sufficient.sum() >= 8 and (~got.sufficient).sum() >= 25
    i_rand = len(records) - 1
    assert (got.top_allele[i_rand] == XS_MLST_NONE).all() and (got.n_tied[i_rand] == 0).all()
    assert (got.top_allele[:i_rand] != XS_MLST_NONE).all() and (got.n_tied[:i_rand] >= 1).all()
    assert got.to_mlst_hits(resolver, url) == {rid: h[0]["Strain type"] for rid, h in want.items()}

    # one resolver call per distinct profile among the sufficient records
    profiles = {tuple(int(next(iter(st[locus])).split("_")[-1]) for locus in m.loci)
                for st in (h[0]["Strain type"] for h in want.values()) if "ST_Name" in st}
    del calls[:]
    names = got.resolve_unique(resolver, url)
    assert len(calls) == len(profiles) < int(got.sufficient.sum())
    assert {c[0] for c in calls} == {tuple(zip(m.loci, p)) for p in profiles} and {c[1] for c in calls} == {url}
    assert names == [want[r.id][0]["Strain type"].get("ST_Name") for r in records]

    # records handed over in memory take the host path: the same columns
    mem = m.predict_columnar(iter(records), step=1)
    assert np.array_equal(mem.top_allele, got.top_allele) and np.array_equal(mem.top_score, got.top_score)
    assert np.array_equal(mem.n_tied, got.n_tied) and np.array_equal(mem.sufficient, got.sufficient)
    one = m.predict_columnar(Record("<unknown id>", allele(1, 17)))
    assert list(one.ids) == ["test"] and one.strain_type(0, resolver, url) == want["a1_17"][0]["Strain type"]

    # the JSON names the same alleles and scores
    got.save(tmp_path / "out" / "typing.json")
    d = json.loads((tmp_path / "out" / "typing.json").read_text())
    assert d == json.loads(json.dumps(got.to_dict())) and d["ids"] == [r.id for r in records]
    for i, rec in enumerate(records):
        st = want[rec.id][0]["Strain type"]
        for locus in m.loci:
            assert {d["top_allele"][locus][i]: d["top_score"][locus][i]} == st[locus], (rec.id, locus)
        assert d["sufficient"][i] == ("ST_Name" in st)

    # the errors predict raises
    short = tmp_path / "short.fasta"
    write_fasta([records[0], Record("k", "ACGT" * 5 + "A")], short)  # 21 bases: not longer than k
    for bad in (iter([Record("k", "A" * K)]), short):
        with pytest.raises(ValueError, match="Invalid sequence, must be longer than k"):
            m.predict_columnar(bad)
    with pytest.raises(ValueError, match="Invalid sequence input"):
        m.predict_columnar([records[0]])
    untrained = ProbabilisticFilterMlstSchemeModel(K, "MLST (Oxford)", tmp_path / "none", url, "abaumannii")
    for inp in (iter([records[0]]), fa):
        with pytest.raises(ValueError, match="The model has not been trained yet"):
            untrained.predict_columnar(inp)
    m.close()
