"""MlstColumnarResult over hand-made arrays, and the argument errors of the
MLST typing entry points of the C ABI (CPU only: nothing here reaches a device)."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import pytest

from xspect2_amd._lib import XS_MLST_NONE
from xspect2_amd.result import MLST_UNRELIABLE, MlstColumnarResult

LOCI = ["Oxf_gltA", "Oxf_gyrB"]
NAMES = [["Allele_ID_3", "Allele_ID_10", "Allele_ID_7"], ["Allele_ID_1", "Allele_ID_22"]]
SIZES = [401, 300]  # half: 200.5 and 150.0
NONE = XS_MLST_NONE


def _result():
    #            gltA            gyrB
    top = [[1, 0],       # r0: sufficient by gyrB at exactly half its size (150 >= 150.0)
           [2, 1],       # r1: 200 < 200.5 and 149 < 150: insufficient
           [2, NONE],    # r2: "N/A" beside a sufficient locus
           [NONE, NONE],  # r3: "N/A" everywhere
           [1, 0],       # r4: r0's profile again
           [0, 1]]       # r5: sufficient by gltA (201 >= 200.5), another profile
    score = [[10, 150], [200, 149], [380, 0], [0, 0], [300, 20], [201, 0]]
    tied = [[1, 2], [1, 1], [1, 0], [0, 0], [3, 1], [1, 2]]
    return MlstColumnarResult("MLST (Oxford)", 1, [f"r{i}" for i in range(6)], LOCI, NAMES, SIZES,
                              np.array(top, dtype=np.uint32), np.array(score), np.array(tied))


def test_sufficient_is_at_least_half_the_locus_size():
    r = _result()
    assert r.sufficient.tolist() == [True, False, True, False, True, True]
    assert r.top_allele.dtype == np.uint32 and r.top_score.dtype == np.uint64 and r.n_tied.dtype == np.uint32


def test_allele_numbers_and_missing():
    assert _result().allele_numbers().tolist() == [[10, 1], [7, 22], [7, -1], [-1, -1], [10, 1], [3, 22]]


def test_strain_type_dicts():
    r = _result()
    calls = []

    def resolver(profile, url):
        calls.append((dict(profile), url))
        return "ST" + "-".join(str(v) for v in profile.values())

    assert r.strain_type(0, resolver, "u") == {"Oxf_gltA": {"Allele_ID_10": 10}, "Oxf_gyrB": {"Allele_ID_1": 150},
                                               "ST_Name": "ST10-1"}
    assert calls == [({"Oxf_gltA": 10, "Oxf_gyrB": 1}, "u")]
    assert r.strain_type(1, resolver, "u") == {"Oxf_gltA": {"Allele_ID_7": 200}, "Oxf_gyrB": {"Allele_ID_22": 149},
                                               "Attention:": MLST_UNRELIABLE}
    # "N/A" beside a sufficient locus: no lookup, ST_Name None
    assert r.strain_type(2, resolver, "u") == {"Oxf_gltA": {"Allele_ID_7": 380}, "Oxf_gyrB": {"N/A": 0},
                                               "ST_Name": None}
    assert r.strain_type(3, resolver, "u") == {"Oxf_gltA": {"N/A": 0}, "Oxf_gyrB": {"N/A": 0},
                                               "Attention:": MLST_UNRELIABLE}
    assert len(calls) == 1
    assert r.strain_type(0)["ST_Name"] is None  # no resolver
    assert list(r.strain_type(0)) == LOCI + ["ST_Name"]  # key order as predict() builds it
    hits = r.to_mlst_hits(resolver, "u")
    assert list(hits) == list(r.ids) and hits["r5"]["ST_Name"] == "ST3-22"


def test_resolve_unique_groups_profiles():
    r = _result()
    calls = []

    def resolver(profile, url):
        calls.append(tuple(profile.items()))
        return "ST" + "-".join(str(v) for v in profile.values())

    assert r.resolve_unique(resolver, "u") == ["ST10-1", None, None, None, "ST10-1", "ST3-22"]
    assert sorted(calls) == [(("Oxf_gltA", 3), ("Oxf_gyrB", 22)), (("Oxf_gltA", 10), ("Oxf_gyrB", 1))]


def test_json_layout(tmp_path):
    r = _result()
    r.save(tmp_path / "out" / "typing.json")
    d = json.loads((tmp_path / "out" / "typing.json").read_text())
    assert d == json.loads(json.dumps(r.to_dict()))
    assert list(d) == ["Scheme", "Steps", "Input_source", "ids", "loci", "locus_size", "top_allele", "top_score",
                       "n_tied", "sufficient"]
    assert d["ids"] == [f"r{i}" for i in range(6)] and d["loci"] == LOCI and d["locus_size"] == SIZES
    assert d["top_allele"]["Oxf_gyrB"] == ["Allele_ID_1", "Allele_ID_22", "N/A", "N/A", "Allele_ID_1", "Allele_ID_22"]
    assert d["top_score"]["Oxf_gltA"] == [10, 200, 380, 0, 300, 201]
    assert d["n_tied"]["Oxf_gyrB"] == [2, 1, 0, 0, 1, 2]
    assert d["sufficient"] == [True, False, True, False, True, True]


def test_shapes_are_checked():
    with pytest.raises(ValueError):
        MlstColumnarResult("s", 1, ["a", "b"], LOCI, NAMES, SIZES, np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((3, 2)))
    empty = MlstColumnarResult("s", 1, [], LOCI, NAMES, SIZES, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)))
    assert empty.sufficient.shape == (0,) and empty.resolve_unique(lambda p, u: "x") == []
    assert empty.to_dict()["top_allele"] == {"Oxf_gltA": [], "Oxf_gyrB": []}


def test_typing_argument_errors_without_gpu():
    """xs_mlst_top_device / xs_mlst_type / xs_mlst_type_device report null
    pointers, n_loci == 0 and out_stride == 0 as XS_ERR_ARG before any device
    work (as test_version_and_errors_without_gpu does for xs_bank_open)."""
    from xspect2_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint32)  # stands in for every non-null pointer: never dereferenced
    p = buf.ctypes.data
    offs = np.zeros(2, dtype=np.uint64)
    assert lib.xs_mlst_top_device(None, 1, 4, p, p, None, 1, None) == _lib.XS_ERR_ARG
    assert b"null argument" in lib.xs_last_error()
    assert lib.xs_mlst_top_device(p, 1, 4, None, p, None, 1, None) == _lib.XS_ERR_ARG
    assert lib.xs_mlst_top_device(p, 1, 4, p, None, None, 1, None) == _lib.XS_ERR_ARG
    assert lib.xs_mlst_top_device(p, 1, 4, p, p, None, 0, None) == _lib.XS_ERR_ARG
    assert b"out_stride" in lib.xs_last_error()
    assert lib.xs_mlst_top_device(p, 1, 0, p, p, None, 1, None) == _lib.XS_ERR_ARG
    assert b"num_docs" in lib.xs_last_error()
    loci = (ctypes.c_void_p * 1)(None)
    for fn, reads in ((lib.xs_mlst_type, (p, offs.ctypes.data)), (lib.xs_mlst_type_device, (p, 8, offs.ctypes.data))):
        assert fn(None, 1, *reads, 1, 1, 0, p, p, None, None) == _lib.XS_ERR_ARG
        assert b"null argument" in lib.xs_last_error()
        assert fn(loci, 0, *reads, 1, 1, 0, p, p, None, None) == _lib.XS_ERR_ARG
        assert b"n_loci" in lib.xs_last_error()
        assert fn(loci, 1, *reads, 1, 1, 0, p, p, None, None) == _lib.XS_ERR_ARG  # a null handle
        assert b"null argument" in lib.xs_last_error()
        assert fn(loci, 1, *reads, 1, 1, 0, None, p, None, None) == _lib.XS_ERR_ARG  # no output
    assert lib.xs_mlst_type(loci, 1, p, None, 1, 1, 0, p, p, None, None) == _lib.XS_ERR_ARG  # no offsets
    assert lib.xs_mlst_type_device(loci, 1, None, 8, offs.ctypes.data, 1, 1, 0, p, p, None, None) == _lib.XS_ERR_ARG
