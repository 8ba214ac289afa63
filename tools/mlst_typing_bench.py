"""MLST typing over reads at BASELINE config-4 size, the existing path and the
new one in one run on one GPU:

    python tools/mlst_typing_bench.py [--reads 1000000] [--ranks N] [--out FILE] [--time-limit 900]

and the assembly leg, ``predict_columnar`` over a FASTA of contigs, on this
checkout and on another one (the parent commit, built beforehand) in one run:

    python tools/mlst_typing_bench.py --assembly --parent-root DIR [--genomes 20] [--out FILE]

Banks and reads follow tests/test_gpu_fullsize.py::test_config4_mlst_full_size:
7 loci x 1430 alleles of 400-600 bp (COBS compact, k = 31, one hash, fpr 0.001,
64-byte pages), error-free 150 bp windows of random alleles.  Three legs, each
after its own warm-up, each repeat timed by a host clock around a call that ends
synchronised:

  a  7 x Bank.mlst_query on the packed host reads: the per-locus path of
     ProbabilisticFilterMlstSchemeModel._locus_rows (reads uploaded per locus, the
     n x D uint32 rows copied back per locus)
  b  mlst_type on the same host reads (one upload, rows reduced on the device)
  c  mlst_type on the reads already in HBM

Beside them, for leg c's account: the device-resident probe step (7 x
query_device into an n x D device matrix), the reduction alone over that matrix
(7 x mlst_top_device between two device events), and leg c at other workspace
sizes.  Before timing, legs b and c must agree, and equal numpy's argmax / max /
count over leg a's rows on a sample of reads.  Prints one JSON line (and writes
it to --out).  The run ends itself after --time-limit seconds.

With ``--ranks N`` the same run also measures the N best alleles per read and
locus: ``mlst_type_ranked`` on the reads already in HBM (beside leg c), and the
ranked reduction alone (7 x mlst_ranks_device between two device events, beside
the top-1 reduction over the same matrix), with their ratio.  Before timing, the
ranked call's top / score / tied must equal leg c's, its rank 0 its top, and on
the sample its ranks the stable argsort of leg a's rows.

The assembly leg writes one synthetic FASTA (--genomes genomes of --genome-mbp
Mbp each, cut into contigs of 20-500 kbp, 80 columns per line, one allele of
every locus embedded per genome; the same 7 x 1430 alleles, k 31) and starts one
fresh child process per checkout.  Each child builds the same banks from the
same seed, wraps them in a ProbabilisticFilterMlstSchemeModel and times
``predict_columnar(path)`` (medians after warm-up, host clock around the call,
which returns synchronised); the children's columns must be identical.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import signal
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

K, LOCI, ALLELES, PAGE, READ_LEN = 31, 7, 1430, 64, 150


def make_alleles(rng):
    """Per locus its alleles (uint8 arrays), sorted by size as a COBS compact bank stores its docs."""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    loci = []
    for _ in range(LOCI):
        base = acgt[rng.integers(0, 4, 620)]
        alleles = []
        for _ in range(ALLELES):
            a = base[:int(rng.integers(400, 601))].copy()
            pos = rng.integers(0, a.size, int(rng.integers(0, 12)))
            a[pos] = acgt[(np.searchsorted(acgt, a[pos]) + 1) % 4]
            alleles.append(a)
        alleles.sort(key=lambda a: a.size)
        loci.append(alleles)
    return loci


def make_scheme(torch, dev, rng):
    """The loci banks, built on the device, and their alleles padded to one array."""
    from xspect2_amd.bank import Bank, cobs_signature_size
    s = torch.cuda.current_stream(dev).cuda_stream
    banks = []
    padded = np.zeros((LOCI, ALLELES, 620), dtype=np.uint8)
    sizes = np.zeros((LOCI, ALLELES), dtype=np.int64)
    for li, alleles in enumerate(make_alleles(rng)):
        per = 8 * PAGE
        sig = [cobs_signature_size(max(a.size for a in alleles[g:g + per]) - K + 1, 1, 0.001)
               for g in range(0, ALLELES, per)]
        bank = Bank.create_cobs(K, 1, sig, ALLELES, [f"Allele_ID_{i}" for i in range(ALLELES)], page_size=PAGE,
                                compact=True, device=dev.index)
        buf = np.concatenate(alleles)
        offs = np.zeros(ALLELES + 1, dtype=np.int64)
        offs[1:] = np.cumsum([a.size for a in alleles])
        bank.build_device(torch.from_numpy(buf).to(dev), buf.size, torch.from_numpy(offs).to(dev), ALLELES,
                          torch.arange(ALLELES, dtype=torch.int32, device=dev), stream=s)
        torch.cuda.synchronize(dev)
        for i, a in enumerate(alleles):
            padded[li, i, :a.size] = a
            sizes[li, i] = a.size
        banks.append(bank)
    return banks, padded, sizes


def make_reads(rng, padded, sizes, n):
    li = rng.integers(0, LOCI, n)
    ai = rng.integers(0, ALLELES, n)
    st = (rng.random(n) * (sizes[li, ai] - READ_LEN + 1)).astype(np.int64)
    return padded[li[:, None], ai[:, None], st[:, None] + np.arange(READ_LEN)[None, :]]


def timed(fn, warmup, repeats, sync):
    for _ in range(warmup):
        fn()
    sync()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "warmup": warmup, "repeats": repeats}


# ---------------------------------------------------------------- the assembly leg
def write_assembly(path: Path, rng, loci, genomes: int, genome_bp: int) -> dict:
    """A FASTA of `genomes` genomes cut into contigs of 20-500 kbp, one allele of every locus per genome."""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    n_contigs = total = 0
    with open(path, "wb") as f:
        for g in range(genomes):
            lens = []
            while sum(lens) < genome_bp:
                lens.append(int(rng.integers(20_000, 500_001)))
            contigs = [acgt[rng.integers(0, 4, n)] for n in lens]
            for alleles in loci:
                a = alleles[int(rng.integers(0, len(alleles)))]
                c = contigs[int(rng.integers(0, len(contigs)))]
                pos = int(rng.integers(0, c.size - a.size))
                c[pos:pos + a.size] = a
            for ci, c in enumerate(contigs):
                f.write(f">g{g}_c{ci}\n".encode())
                full = c.size // 80 * 80
                lines = np.full((full // 80, 81), ord("\n"), dtype=np.uint8)
                lines[:, :80] = c[:full].reshape(-1, 80)
                f.write(lines.tobytes())
                if c.size > full:
                    f.write(c[full:].tobytes() + b"\n")
                n_contigs += 1
                total += c.size
    return {"genomes": genomes, "contigs": n_contigs, "bases": total, "file_bytes": path.stat().st_size}


def assembly_child(a) -> int:
    """Time predict_columnar(a.fasta) with the package of checkout a.root; one JSON line."""
    sys.path.insert(0, str(a.root))
    import torch
    from xspect2_amd import _lib
    from xspect2_amd.probabilistic_filter_mlst_model import ProbabilisticFilterMlstSchemeModel

    assert Path(_lib.__file__).resolve().is_relative_to(Path(a.root).resolve()), _lib.__file__
    dev = torch.device("cuda", 0)
    banks, _, sizes = make_scheme(torch, dev, np.random.default_rng(4242))
    m = ProbabilisticFilterMlstSchemeModel(K, "MLST (bench)", Path(a.fasta).parent, "https://example/schemes/1", "bench")
    m.indices = banks
    m.loci = {f"locus{li}": ALLELES for li in range(LOCI)}
    m.avg_locus_bp_size = [int(sizes[li, 0]) for li in range(LOCI)]
    res = m.predict_columnar(Path(a.fasta))
    digest = hashlib.sha256()
    for col in (res.top_allele, res.top_score, res.n_tied):
        digest.update(np.ascontiguousarray(col).tobytes())
    t = timed(lambda: m.predict_columnar(Path(a.fasta)), a.warmup, a.repeats, lambda: torch.cuda.synchronize(dev))
    t.update({"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev),
              "records": int(res.top_allele.shape[0]), "records_with_a_call": int((res.n_tied > 0).any(axis=1).sum()),
              "columns_sha256": digest.hexdigest()})
    print(json.dumps(t))
    m.close()
    return 0


def assembly_leg(a) -> int:
    rng = np.random.default_rng(4242)
    loci = make_alleles(rng)
    with tempfile.TemporaryDirectory() as tmp:
        fasta = Path(tmp) / "assembly.fasta"
        info = write_assembly(fasta, rng, loci, a.genomes, int(a.genome_mbp * 1e6))
        runs = {}
        for name, root in (("parent", a.parent_root), ("this", ROOT)):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--assembly-child", "--root", str(root), "--fasta",
                   str(fasta), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.time_limit)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                return 1
            runs[name] = json.loads(out.stdout.strip().splitlines()[-1])
            print(f"{name}: median {runs[name]['median_ms']} ms", file=sys.stderr, flush=True)
    same = runs["parent"]["columns_sha256"] == runs["this"]["columns_sha256"]
    line = {"tool": "mlst_typing_bench --assembly", "input": info,
            "config": {"loci": LOCI, "alleles_per_locus": ALLELES, "k": K, "page_size": PAGE, "step": 1},
            "parent": runs["parent"], "this": runs["this"], "same_columns": same,
            "this_over_parent_speedup": round(runs["parent"]["median_ms"] / runs["this"]["median_ms"], 2),
            "clock": "host perf_counter around predict_columnar(path), which returns synchronised; one process per checkout"}
    text = json.dumps(line)
    print(text)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(text + "\n")
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assembly", action="store_true", help="the assembly leg instead of the read legs")
    ap.add_argument("--parent-root", type=Path, default=None, help="assembly leg: the other checkout (built)")
    ap.add_argument("--genomes", type=int, default=20)
    ap.add_argument("--genome-mbp", type=float, default=4.0)
    ap.add_argument("--assembly-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", type=Path, default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--fasta", type=Path, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--ranks", type=int, default=0, help="also measure the N best alleles per read and locus")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--existing-warmup", type=int, default=1, help="leg a (seconds per call at full size)")
    ap.add_argument("--existing-repeats", type=int, default=3)
    ap.add_argument("--sweep-mib", type=int, nargs="*", default=[256, 1024, 16384],
                    help="leg c again with these workspace sizes")
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the run ends itself")
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()

    def too_long(*_):
        raise SystemExit(f"mlst_typing_bench: time limit of {a.time_limit} s reached")

    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(a.time_limit)
    if a.assembly_child:
        return assembly_child(a)
    if a.assembly:
        if a.parent_root is None:
            raise SystemExit("mlst_typing_bench: --assembly needs --parent-root")
        return assembly_leg(a)

    import torch
    from xspect2_amd import _lib
    from xspect2_amd.bank import DeviceReads, mlst_ranks_device, mlst_top_device, mlst_type, mlst_type_ranked
    from xspect2_amd.packing import pack_fixed

    if not torch.cuda.is_available():
        raise SystemExit("mlst_typing_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream

    def sync():
        torch.cuda.synchronize(dev)

    rng = np.random.default_rng(4242)
    n = a.reads
    banks, padded, sizes = make_scheme(torch, dev, rng)
    reads = make_reads(rng, padded, sizes, n)
    packed = pack_fixed(reads)
    d_seqs = torch.from_numpy(reads.reshape(-1)).to(dev)
    d_offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN
    sync()
    dreads = DeviceReads(d_seqs, n * READ_LEN, d_offs, n, READ_LEN)

    # ---- results first: b == c, and both equal the reduction of leg a's rows on a sample
    sample = np.unique(np.concatenate([np.arange(min(n, 500)), np.arange(max(0, n - 500), n),
                                       rng.integers(0, n, 2000)]))
    got_b = mlst_type(banks, packed)
    got_c = mlst_type(banks, dreads)
    same_bc = all(np.array_equal(x, y) for x, y in zip(got_b, got_c))
    N = a.ranks
    widths = [int(sizes[li, 0]) for li in range(LOCI)]  # the model's "average" size; 150 bp reads are never chunked
    got_r = mlst_type_ranked(banks, dreads, widths, N) if N else None
    mismatches = rank_mismatches = 0
    for l, bank in enumerate(banks):
        rows = bank.mlst_query(packed, [], [], 0)[0][sample]
        m = rows.max(axis=1)
        mismatches += int((got_b[0][sample, l] != rows.argmax(axis=1)).sum() + (got_b[1][sample, l] != m).sum()
                          + (got_b[2][sample, l] != (rows == m[:, None]).sum(axis=1)).sum())
        if N:
            order = np.argsort(-rows.astype(np.int64), axis=1, kind="stable")[:, :N]
            rank_mismatches += int((got_r[4][sample, l] != order).sum()
                                   + (got_r[5][sample, l] != np.take_along_axis(rows, order, axis=1)).sum())
        del rows
    own = (got_b[1].max(axis=1) == READ_LEN - K + 1)  # an error-free window scores all its k-mers somewhere
    checks = {"b_equals_c": bool(same_bc), "sample_reads": int(sample.size), "sample_mismatches_vs_leg_a_rows": mismatches,
              "reads_with_a_full_score": int(own.sum()), "num_kmers_ok": bool((got_b[3] == READ_LEN - K + 1).all())}
    checks["ok"] = bool(same_bc and mismatches == 0 and own.all() and checks["num_kmers_ok"])
    if N:
        checks["ranked_equals_c"] = all(np.array_equal(x, y) for x, y in zip(got_c, got_r[:4]))
        checks["rank0_is_top"] = bool(np.array_equal(got_r[4][:, :, 0], got_r[0]) and np.array_equal(got_r[5][:, :, 0], got_r[1]))
        checks["sample_rank_mismatches_vs_leg_a_rows"] = rank_mismatches
        checks["ok"] = bool(checks["ok"] and checks["ranked_equals_c"] and checks["rank0_is_top"] and rank_mismatches == 0)
    del got_r

    # ---- the legs
    def leg_a():
        for bank in banks:
            bank.mlst_query(packed, [], [], 0)

    legs = {
        "a_mlst_query_per_locus": timed(leg_a, a.existing_warmup, a.existing_repeats, sync),
        "b_mlst_type_host_reads": timed(lambda: mlst_type(banks, packed), a.warmup, a.repeats, sync),
        "c_mlst_type_device_reads": timed(lambda: mlst_type(banks, dreads), a.warmup, a.repeats, sync),
    }
    if N:
        legs["c_mlst_type_ranked_device_reads"] = timed(lambda: mlst_type_ranked(banks, dreads, widths, N), a.warmup,
                                                        a.repeats, sync)
    sweep = {str(mib): timed(lambda mib=mib: mlst_type(banks, dreads, workspace_bytes=mib << 20), a.warmup,
                             a.repeats, sync) for mib in a.sweep_mib}

    # ---- leg c's parts: the probe step on device reads, and the reduction alone (device events)
    hits = torch.empty((n, ALLELES), dtype=torch.int32, device=dev)
    d_nk = torch.empty(n, dtype=torch.int64, device=dev)
    tot = torch.empty(ALLELES + 1, dtype=torch.int64, device=dev)

    def probe_step():
        for bank in banks:
            bank.query_device(d_seqs, n * READ_LEN, d_offs, n, 1, hits, d_nk, tot, stream=s)

    probe = timed(probe_step, a.warmup, a.repeats, sync)
    outs = [torch.empty(n * LOCI, dtype=torch.int32, device=dev) for _ in range(3)]  # n x LOCI, row-major

    def reduce_all():
        for l in range(LOCI):
            mlst_top_device(hits, n, ALLELES, outs[0][l:], outs[1][l:], outs[2][l:], LOCI, stream=s)

    def by_events(fn):
        for _ in range(a.warmup):
            fn()
        sync()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            sync()
            ms.append(e0.elapsed_time(e1))
        return ms

    ev_ms = by_events(reduce_all)
    reduce_ms = statistics.median(ev_ms)
    matrix_gb = LOCI * n * ALLELES * 4 / 1e9
    ranked = None
    if N:
        r_outs = [torch.empty(n * LOCI * N, dtype=torch.int32, device=dev) for _ in range(2)]  # n x LOCI x N

        def reduce_ranked():
            for l in range(LOCI):
                mlst_ranks_device(hits, n, ALLELES, N, r_outs[0][l * N:], r_outs[1][l * N:], LOCI * N, outs[0][l:],
                                  outs[1][l:], outs[2][l:], LOCI, stream=s)

        r_ms = by_events(reduce_ranked)
        ranked_ms = statistics.median(r_ms)
        ranked = {"ranks": N, "median_ms": round(ranked_ms, 3), "ms": [round(x, 3) for x in r_ms],
                  "matrix_gb_read": round(matrix_gb, 2), "rank_mb_written": round(LOCI * n * N * 8 / 1e6, 1),
                  "gb_per_s": round(matrix_gb / ranked_ms * 1e3, 1),
                  "over_top1_reduction": round(ranked_ms / reduce_ms, 2),
                  "clock": "device events around 7 x mlst_ranks_device (top, score, tied and the ranks) over the same matrix"}

    med = {k: v["median_ms"] for k, v in legs.items()}
    line = {
        "tool": "mlst_typing_bench", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev),
        "config": {"reads": n, "read_len": READ_LEN, "loci": LOCI, "alleles_per_locus": ALLELES, "k": K,
                   "page_size": PAGE, "step": 1, "default_workspace_mib": 4096},
        "checks": checks, "legs": legs,
        "b_over_a_speedup": round(med["a_mlst_query_per_locus"] / med["b_mlst_type_host_reads"], 2),
        "device_probe_step": probe,
        "reduction_alone": {"median_ms": round(reduce_ms, 3), "ms": [round(x, 3) for x in ev_ms],
                            "matrix_gb_read": round(matrix_gb, 2), "gb_per_s": round(matrix_gb / reduce_ms * 1e3, 1),
                            "clock": "device events around 7 x mlst_top_device over the n x D device matrix"},
        "c_over_probe_step": round(med["c_mlst_type_device_reads"] / probe["median_ms"], 2),
        **({"ranked_reduction_alone": ranked,
            "ranked_over_c": round(med["c_mlst_type_ranked_device_reads"] / med["c_mlst_type_device_reads"], 2)}
           if N else {}),
        "c_workspace_sweep_mib": sweep,
        "clock": "host perf_counter around calls that return synchronised (legs), a device synchronise (probe step)",
    }
    text = json.dumps(line)
    print(text)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(text + "\n")
    for bank in banks:
        bank.close()
    return 0 if checks["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
