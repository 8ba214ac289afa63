"""The ranked MLST entry points without a device: their argument errors come back as XS_ERR_ARG
with a message before any device work (as test_mlst_contigs_args.py checks for the contig calls),
``MlstColumnarResult`` with and without ranks, and ``predict_columnar``'s ``limit_number`` bounds."""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest

NONE = 0xFFFFFFFF


def test_ranked_typing_argument_errors_without_gpu():
    from xspect2_amd import _lib
    lib = _lib.load()
    assert _lib.XS_MLST_MAX_RANKS == 8
    buf = np.zeros(16, dtype=np.uint32)  # stands in for every non-null pointer: never dereferenced
    p = buf.ctypes.data
    offs = np.zeros(2, dtype=np.uint64)
    o = offs.ctypes.data
    width = np.full(1, 450, dtype=np.uint64)
    w = width.ctypes.data
    loci = (ctypes.c_void_p * 1)(None)
    bad_scale = _lib.MlstChunkRule(10_000, 10, 9, 50, 0)
    host = (lib.xs_mlst_type_ranked, lambda r, wd: (wd, r, p, o))
    dev = (lib.xs_mlst_type_ranked_device, lambda r, wd, nbytes=8: (wd, r, p, nbytes, o, None))

    def tail(n_ranks=5, step=1, top=p, ra=p, rs=p):  # n, step, workspace, n_ranks, top, score, tied, nk, ranks
        return (1, step, 0, n_ranks, top, p, None, None, ra, rs)

    for fn, reads in (host, dev):
        for bad in (0, 9, 1 << 31):
            assert fn(loci, 1, *reads(None, w), *tail(n_ranks=bad)) == _lib.XS_ERR_ARG
            assert b"n_ranks" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), *tail(ra=None)) == _lib.XS_ERR_ARG
        assert b"rank outputs" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), *tail(rs=None)) == _lib.XS_ERR_ARG
        assert b"rank outputs" in lib.xs_last_error()
        # the contig calls' own errors
        assert fn(loci, 1, *reads(None, None), *tail()) == _lib.XS_ERR_ARG
        assert b"locus_width" in lib.xs_last_error()
        assert fn(loci, 1, *reads(ctypes.byref(bad_scale), w), *tail()) == _lib.XS_ERR_ARG
        assert b"scale10_len" in lib.xs_last_error()
        assert fn(None, 1, *reads(None, w), *tail()) == _lib.XS_ERR_ARG
        assert b"null argument" in lib.xs_last_error()
        assert fn(loci, 0, *reads(None, w), *tail()) == _lib.XS_ERR_ARG
        assert b"n_loci" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), *tail()) == _lib.XS_ERR_ARG  # a null handle
        assert b"null argument" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), *tail(step=0)) == _lib.XS_ERR_ARG
        assert b"step" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), *tail(top=None)) == _lib.XS_ERR_ARG
    big = np.array([0, (1 << 32) - 64], dtype=np.uint64)
    assert lib.xs_mlst_type_ranked(loci, 1, w, None, p, big.ctypes.data, *tail()) == _lib.XS_ERR_ARG
    assert b"sequence bytes" in lib.xs_last_error()
    assert lib.xs_mlst_type_ranked_device(loci, 1, *dev[1](None, w, (1 << 32) - 64), *tail()) == _lib.XS_ERR_ARG
    assert b"sequence bytes" in lib.xs_last_error()
    assert lib.xs_mlst_type_ranked(loci, 1, w, None, p, None, *tail()) == _lib.XS_ERR_ARG  # no offsets
    assert lib.xs_mlst_type_ranked_device(loci, 1, w, None, None, 8, o, None, *tail()) == _lib.XS_ERR_ARG  # no reads


def test_rank_reductions_argument_errors_without_gpu():
    from xspect2_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    rows = lib.xs_mlst_ranks_device  # d_hits, n, num_docs, n_ranks, top, score, tied, top_stride, ra, rs, rank_stride, stream
    assert rows(None, 1, 4, 5, None, None, None, 1, p, p, 5, None) == _lib.XS_ERR_ARG
    assert b"null argument" in lib.xs_last_error()
    assert rows(p, 1, 4, 5, None, None, None, 1, None, p, 5, None) == _lib.XS_ERR_ARG
    assert rows(p, 1, 4, 5, None, None, None, 1, p, None, 5, None) == _lib.XS_ERR_ARG
    assert rows(p, 1, 0, 5, None, None, None, 1, p, p, 5, None) == _lib.XS_ERR_ARG
    assert b"num_docs" in lib.xs_last_error()
    for bad in (0, 9):
        assert rows(p, 1, 4, bad, None, None, None, 1, p, p, 9, None) == _lib.XS_ERR_ARG
        assert b"n_ranks" in lib.xs_last_error()
    assert rows(p, 1, 4, 5, None, None, None, 1, p, p, 4, None) == _lib.XS_ERR_ARG
    assert b"rank_stride" in lib.xs_last_error()
    assert rows(p, 1, 4, 5, p, None, None, 0, p, p, 5, None) == _lib.XS_ERR_ARG
    assert b"top_stride" in lib.xs_last_error()
    chunks = lib.xs_mlst_chunk_ranks_device  # d_hits, n_chunks, num_docs, begin, n_owners, threshold, n_ranks, ra, rs, stride
    assert chunks(None, 1, 4, p, 1, 50, 5, p, p, 5, None) == _lib.XS_ERR_ARG
    assert b"null argument" in lib.xs_last_error()
    assert chunks(p, 1, 4, None, 1, 50, 5, p, p, 5, None) == _lib.XS_ERR_ARG
    assert chunks(p, 1, 4, p, 1, 50, 5, None, p, 5, None) == _lib.XS_ERR_ARG
    assert chunks(p, 1, 4, p, 1, 50, 5, p, None, 5, None) == _lib.XS_ERR_ARG
    assert chunks(p, 1, 0, p, 1, 50, 5, p, p, 5, None) == _lib.XS_ERR_ARG
    assert b"num_docs" in lib.xs_last_error()
    for bad in (0, 9):
        assert chunks(p, 1, 4, p, 1, 50, bad, p, p, 9, None) == _lib.XS_ERR_ARG
        assert b"n_ranks" in lib.xs_last_error()
    assert chunks(p, 1, 4, p, 1, 50, 5, p, p, 4, None) == _lib.XS_ERR_ARG
    assert b"rank_stride" in lib.xs_last_error()
    assert chunks(p, 1 << 32, 4, p, 1, 50, 5, p, p, 5, None) == _lib.XS_ERR_ARG
    assert b"chunks" in lib.xs_last_error()


def test_python_wrapper_rejects_ranks_out_of_range():
    from xspect2_amd.bank import mlst_type_ranked
    for bad in (0, 9):
        with pytest.raises(ValueError, match="1 .. 8"):
            mlst_type_ranked([], [b"ACGT"], [], bad)


# ---------------------------------------------------------------- MlstColumnarResult
LOCI = ["Oxf_a", "Oxf_b"]
NAMES = [[f"a_{i}" for i in range(1, 5)], [f"b_{i}" for i in range(1, 4)]]
TOP = np.array([[2, 0], [1, NONE]], dtype=np.uint32)
SCORE = np.array([[130, 90], [60, 0]], dtype=np.uint64)
TIED = np.array([[1, 2], [1, 0]], dtype=np.uint32)
RANK_A = np.array([[[2, 0, 3], [0, 1, NONE]], [[1, NONE, NONE], [NONE, NONE, NONE]]], dtype=np.uint32)
RANK_S = np.array([[[130, 120, 0], [90, 90, 0]], [[60, 0, 0], [0, 0, 0]]], dtype=np.uint32)
KEYS = ["Scheme", "Steps", "Input_source", "ids", "loci", "locus_size", "top_allele", "top_score", "n_tied", "sufficient"]


def _result(**kw):
    from xspect2_amd.result import MlstColumnarResult
    return MlstColumnarResult("MLST (Oxford)", 1, ["r0", "r1"], LOCI, NAMES, [200, 200], TOP, SCORE, TIED, None, **kw)


def test_columnar_result_without_ranks_is_unchanged():
    res = _result()
    assert res.rank_allele is None and res.rank_score is None
    assert list(res.to_dict()) == KEYS
    with pytest.raises(ValueError, match="no ranks"):
        res.all_results(0)
    with pytest.raises(ValueError, match="no ranks"):
        res.to_mlst_result()


def test_columnar_result_with_ranks():
    from xspect2_amd.result import MlstResult
    res = _result(rank_allele=RANK_A, rank_score=RANK_S)
    assert res.rank_allele.dtype == np.uint32 and res.rank_score.dtype == np.uint64
    all0 = res.all_results(0)
    assert all0 == {"Oxf_a": {"a_3": 130, "a_1": 120, "a_4": 0}, "Oxf_b": {"b_1": 90, "b_2": 90}}
    assert list(all0["Oxf_a"]) == ["a_3", "a_1", "a_4"] and list(all0) == LOCI  # rank order, locus order
    assert res.all_results(1) == {"Oxf_a": {"a_2": 60}}  # the "N/A" locus is left out
    resolver = lambda profile, url: f"ST{profile['Oxf_a']}{profile['Oxf_b']}@{url}"
    mr = res.to_mlst_result(resolver, "u")
    assert isinstance(mr, MlstResult) and mr.scheme_model == "MLST (Oxford)" and mr.steps == 1
    assert list(mr.hits) == ["r0", "r1"]
    assert mr.hits["r0"] == [{"Strain type": res.strain_type(0, resolver, "u")}, {"All results": all0}]
    assert mr.hits["r0"][0]["Strain type"]["ST_Name"] == "ST31@u"
    assert mr.hits["r1"][0]["Strain type"]["Oxf_b"] == {"N/A": 0}
    d = res.to_dict()
    assert list(d) == KEYS + ["ranked_alleles", "ranked_scores"]
    assert d["ranked_alleles"] == {"Oxf_a": [["a_3", "a_1", "a_4"], ["a_2", "N/A", "N/A"]],
                                   "Oxf_b": [["b_1", "b_2", "N/A"], ["N/A", "N/A", "N/A"]]}
    assert d["ranked_scores"] == {"Oxf_a": [[130, 120, 0], [60, 0, 0]], "Oxf_b": [[90, 90, 0], [0, 0, 0]]}
    assert {k: d[k] for k in KEYS} == _result().to_dict()


def test_columnar_result_rank_shape_errors():
    with pytest.raises(ValueError, match="come together"):
        _result(rank_allele=RANK_A)
    with pytest.raises(ValueError, match="come together"):
        _result(rank_score=RANK_S)
    for ra, rs in ((RANK_A[:1], RANK_S[:1]), (RANK_A[:, :1], RANK_S[:, :1]), (RANK_A, RANK_S[:, :, :2]),
                   (RANK_A[:, :, :0], RANK_S[:, :, :0]), (RANK_A.reshape(2, 6), RANK_S.reshape(2, 6))):
        with pytest.raises(ValueError, match="n_ranks"):
            _result(rank_allele=ra, rank_score=rs)


def test_limit_number_outside_the_cap_raises(tmp_path):
    from xspect2_amd.probabilistic_filter_mlst_model import ProbabilisticFilterMlstSchemeModel
    m = ProbabilisticFilterMlstSchemeModel(21, "MLST (Oxford)", Path(tmp_path), "https://example/schemes/1", "abaumannii")
    for bad in (0, 9):
        with pytest.raises(ValueError, match="XS_MLST_MAX_RANKS"):
            m.predict_columnar(iter([]), limit=True, limit_number=bad)
    # within the cap the call goes on to the model's own checks
    with pytest.raises(ValueError, match="not been trained"):
        m.predict_columnar(iter([]), limit=True, limit_number=8)
