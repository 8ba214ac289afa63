#!/usr/bin/env python3
"""filter_genus / filter_species from file to filtered FASTA, timed.

Writes a seeded FASTQ (default 1 M reads of 150 bp, about 10 % of them drawn
from the genus' genomes, the rest random), builds a genus Bloom model and a
4-species COBS + SVM model over synthetic genomes in a temporary data
directory, and times ``filter_genus`` and ``filter_species`` at threshold 0.7
without a classification output: the median of ``--runs`` runs after one
warm-up, each a host clock around a call that ends with the output file on
disk.  Prints one JSON line.  It uses the package's public calls only, so the
same file runs on an older checkout for comparison.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

K = 21


def write_fastq(path: Path, genomes, n: int, length: int, member_frac: float, seed: int) -> int:
    """n fixed-width FASTQ records; returns how many were drawn from genomes[0:2]."""
    rng = np.random.default_rng(seed)
    member = rng.random(n) < member_frac
    seqs = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n, length))
    rows = np.flatnonzero(member)
    for g in (0, 1):
        sel = rows[g::2]
        start = rng.integers(0, len(genomes[g]) - length, sel.size)
        seqs[sel] = genomes[g][start[:, None] + np.arange(length)[None, :]]
    head = np.frombuffer("".join(f"@r{i:08d}\n" for i in range(n)).encode(), dtype=np.uint8).reshape(n, 11)
    rec = np.empty((n, 11 + length + 3 + length + 1), dtype=np.uint8)
    rec[:, :11] = head
    rec[:, 11:11 + length] = seqs
    rec[:, 11 + length:14 + length] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 14 + length:-1] = ord("I")
    rec[:, -1] = ord("\n")
    rec.tofile(path)
    return int(member.sum())


def build_models(tmp: Path, genomes) -> None:
    from xspect2_amd.classify import model_dir
    from xspect2_amd.file_io import Record, write_fasta
    from xspect2_amd.probabilistic_filter_svm_model import ProbabilisticFilterSVMModel
    from xspect2_amd.probabilistic_single_filter_model import ProbabilisticSingleFilterModel

    base = model_dir()
    text = [g.tobytes().decode() for g in genomes]
    gfa = tmp / "Acinetobacter.fasta"
    write_fasta([Record("g0", text[0]), Record("g1", text[1])], gfa)
    genus = ProbabilisticSingleFilterModel(K, "Acinetobacter", None, None, "Genus", base)
    genus.fit(gfa, "Acinetobacter")
    genus.save()
    genus.close()
    sdir, svm = tmp / "species", tmp / "svm"
    sdir.mkdir()
    for i, t in enumerate(text):
        write_fasta([Record(f"c{i}", t)], sdir / f"{470 + i}.fasta")
        for j in range(2):
            write_fasta([Record("x", t[j * 7000:j * 7000 + 9000])], svm / f"{470 + i}" / f"acc{i}{j}.fasta")
    species = ProbabilisticFilterSVMModel(K, "Acinetobacter", None, None, "Species", base, "rbf", 1.0)
    species.fit(sdir, svm, svm_step=1)
    species.save()
    species.close()


def timed(fn, out: Path, runs: int) -> dict:
    times, records = [], 0
    for i in range(runs + 1):  # the first run warms up (code objects, pinned buffers, page cache)
        out.unlink(missing_ok=True)
        t0 = time.perf_counter()
        fn(out)
        dt = time.perf_counter() - t0
        if i:
            times.append(dt)
        records = out.read_bytes().count(b">") if out.exists() else 0
    return {"median_s": round(statistics.median(times), 4), "min_s": round(min(times), 4),
            "max_s": round(max(times), 4), "runs": runs, "kept_records": records}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--members", type=float, default=0.10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--label", default="", help="recorded in the output line")
    args = ap.parse_args()

    with tempfile.TemporaryDirectory(prefix="xs_bench_filter_") as d:
        tmp = Path(d)
        os.environ["XSPECT_DATA"] = str(tmp / "xd")
        from xspect2_amd import _lib
        from xspect2_amd.filter_sequences import filter_genus, filter_species
        from xspect2_amd.synth import make_genomes

        if _lib.device_count() < 1:
            raise RuntimeError("no HIP device visible")
        genomes = make_genomes(4, 200_000, seed=args.seed)
        build_models(tmp, genomes)
        inp = tmp / "reads.fq"
        members = write_fastq(inp, genomes, args.reads, args.length, args.members, args.seed)
        quiet = open(os.devnull, "w")
        stdout, sys.stdout = sys.stdout, quiet  # the calls print one line per file
        try:
            genus = timed(lambda out: filter_genus("Acinetobacter", inp, out, 0.7), tmp / "genus.fasta", args.runs)
            species = timed(lambda out: filter_species("Acinetobacter", "470", inp, out, 0.7), tmp / "species.fasta",
                            args.runs)
        finally:
            sys.stdout = stdout
            quiet.close()
        print(json.dumps({"bench": "filter_onepass", "label": args.label, "build_id": _lib.build_id(),
                          "reads": args.reads, "read_len": args.length, "genus_members": members, "threshold": 0.7,
                          "input_bytes": inp.stat().st_size, "filter_genus": genus, "filter_species": species}))


if __name__ == "__main__":
    main()
