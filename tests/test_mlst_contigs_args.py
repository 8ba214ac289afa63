"""The contig typing entry points without a device: their argument errors come back as
XS_ERR_ARG with a message before any device work (as test_typing_argument_errors_without_gpu
checks for xs_mlst_type), and the splitter's sizing, a closed form of the lengths, agrees
with ``oracle.sequence_splitter``."""
from __future__ import annotations

import ctypes

import numpy as np


def _rule(_lib, long_len=10_000, scale10=1_000_000, scale100=10_000_000, threshold=50):
    return _lib.MlstChunkRule(long_len, scale10, scale100, threshold, 0)


def test_contig_typing_argument_errors_without_gpu():
    from xspect2_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint32)  # stands in for every non-null pointer: never dereferenced
    p = buf.ctypes.data
    offs = np.zeros(2, dtype=np.uint64)
    o = offs.ctypes.data
    width = np.full(1, 450, dtype=np.uint64)
    w = width.ctypes.data
    loci = (ctypes.c_void_p * 1)(None)
    bad_scale = _rule(_lib, scale10=10, scale100=9)
    host = (lib.xs_mlst_type_contigs, lambda r, wd, ol=o: (wd, r, p, ol))
    dev = (lib.xs_mlst_type_contigs_device, lambda r, wd, nbytes=8: (wd, r, p, nbytes, o, None))
    for fn, reads in (host, dev):
        tail = (1, 1, 0, p, p, None, None)  # n, step, workspace_bytes, top, top_score, n_tied, num_kmers
        assert fn(loci, 1, *reads(None, None), *tail) == _lib.XS_ERR_ARG
        assert b"locus_width" in lib.xs_last_error()
        assert fn(loci, 1, *reads(ctypes.byref(bad_scale), w), *tail) == _lib.XS_ERR_ARG
        assert b"scale10_len" in lib.xs_last_error()
        assert fn(None, 1, *reads(None, w), *tail) == _lib.XS_ERR_ARG
        assert b"null argument" in lib.xs_last_error()
        assert fn(loci, 0, *reads(None, w), *tail) == _lib.XS_ERR_ARG
        assert b"n_loci" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), *tail) == _lib.XS_ERR_ARG  # a null handle
        assert b"null argument" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), 1, 0, 0, p, p, None, None) == _lib.XS_ERR_ARG
        assert b"step" in lib.xs_last_error()
        assert fn(loci, 1, *reads(None, w), 1, 1, 0, None, p, None, None) == _lib.XS_ERR_ARG  # no output
    # 2^32 - 64 sequence bytes and more: a summed score could leave uint32
    big = np.array([0, (1 << 32) - 64], dtype=np.uint64)
    assert lib.xs_mlst_type_contigs(loci, 1, w, None, p, big.ctypes.data, 1, 1, 0, p, p, None, None) == _lib.XS_ERR_ARG
    assert b"sequence bytes" in lib.xs_last_error()
    assert lib.xs_mlst_type_contigs_device(loci, 1, *dev[1](None, w, (1 << 32) - 64), 1, 1, 0, p, p, None,
                                           None) == _lib.XS_ERR_ARG
    assert b"sequence bytes" in lib.xs_last_error()
    assert lib.xs_mlst_type_contigs(loci, 1, w, None, p, None, 1, 1, 0, p, p, None, None) == _lib.XS_ERR_ARG  # no offsets
    assert lib.xs_mlst_type_contigs_device(loci, 1, w, None, None, 8, o, None, 1, 1, 0, p, p, None,
                                           None) == _lib.XS_ERR_ARG  # no reads


def test_split_and_chunk_top_argument_errors_without_gpu():
    """The splitter takes k as an argument, so a width or long_len below k is reported without a bank."""
    from xspect2_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    nc, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    short_long = _rule(_lib, long_len=20)
    bad_scale = _rule(_lib, scale10=10, scale100=9)
    for call in (lambda width, k, r: lib.xs_mlst_split_size(p, 1, width, k, r, ctypes.byref(nc), ctypes.byref(nb)),
                 lambda width, k, r: lib.xs_mlst_split_device(p, p, p, 1, width, k, r, p, p, p, None)):
        assert call(20, 21, None) == _lib.XS_ERR_ARG
        assert b"width" in lib.xs_last_error()
        assert call(450, 0, None) == _lib.XS_ERR_ARG
        assert call(450, 21, ctypes.byref(short_long)) == _lib.XS_ERR_ARG
        assert b"long_len" in lib.xs_last_error()
        assert call(450, 21, ctypes.byref(bad_scale)) == _lib.XS_ERR_ARG
        assert b"scale10_len" in lib.xs_last_error()
    assert lib.xs_mlst_split_size(None, 1, 450, 21, None, ctypes.byref(nc), ctypes.byref(nb)) == _lib.XS_ERR_ARG
    assert lib.xs_mlst_split_size(p, 1, 450, 21, None, None, ctypes.byref(nb)) == _lib.XS_ERR_ARG
    assert lib.xs_mlst_split_device(p, p, p, 1, 450, 21, None, None, p, p, None) == _lib.XS_ERR_ARG
    assert b"null argument" in lib.xs_last_error()
    assert lib.xs_mlst_split_device(None, p, p, 1, 450, 21, None, p, p, p, None) == _lib.XS_ERR_ARG
    top = lib.xs_mlst_chunk_top_device
    assert top(None, 1, 4, p, 1, 50, p, p, None, 1, None) == _lib.XS_ERR_ARG
    assert b"null argument" in lib.xs_last_error()
    assert top(p, 1, 4, None, 1, 50, p, p, None, 1, None) == _lib.XS_ERR_ARG
    assert top(p, 1, 4, p, 1, 50, None, p, None, 1, None) == _lib.XS_ERR_ARG
    assert top(p, 1, 4, p, 1, 50, p, None, None, 1, None) == _lib.XS_ERR_ARG
    assert top(p, 1, 0, p, 1, 50, p, p, None, 1, None) == _lib.XS_ERR_ARG
    assert b"num_docs" in lib.xs_last_error()
    assert top(p, 1, 4, p, 1, 50, p, p, None, 0, None) == _lib.XS_ERR_ARG
    assert b"out_stride" in lib.xs_last_error()


def test_split_size_matches_the_oracle_splitter(oracle_mod):
    """Chunks and chunk bytes of every length around the edges of the rule, for two k and widths,
    against the lists ``oracle.sequence_splitter`` returns (the reference's scale boundaries
    included: the oracle has them built in)."""
    from xspect2_amd.bank import mlst_split_size
    for k, w in ((21, 450), (31, 470), (5, 5), (1, 3)):
        s = w - k + 1
        lengths = sorted(set(list(range(k, 3 * w + 2 * k)) + [m * s + w + d for m in (7, 23) for d in (-1, 0, 1)]))
        for n in lengths:
            parts = oracle_mod.sequence_splitter("A" * n, w, k)
            assert mlst_split_size([n], w, k, (k, 1_000_000, 10_000_000, 50)) == (len(parts), sum(map(len, parts))), (k, w, n)
    for n in (999_999, 1_000_000, 9_999_999, 10_000_000):
        parts = oracle_mod.sequence_splitter("A" * n, 450, 21)
        assert mlst_split_size([n], 450, 21) == (len(parts), sum(map(len, parts))), n
    lens = [10_000, 10_110, 10_109, 10_111, 123_456]
    parts = [oracle_mod.sequence_splitter("A" * n, 450, 31) for n in lens]
    assert mlst_split_size(lens, 450, 31) == (sum(map(len, parts)), sum(len(p) for ps in parts for p in ps))
    assert [len(ps) for ps in parts[1:4]] == [24, 24, 25] and len(parts[1][-1]) == 480 and len(parts[2][-1]) == 449
