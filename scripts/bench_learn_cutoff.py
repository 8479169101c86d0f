#!/usr/bin/env python3
"""learn-cutoff measurements (profiles/r07_learn_cutoff.json):

* the column reader (``rp_cutoff_read_host``) against ``pandas.read_csv(usecols=4 columns)`` on a
  ``report_all``-shaped TSV of ``--tsv-gb`` GB (synthetic rows with the export's columns and profile
  lengths; pandas is timed on the first ``--pandas-mb`` MB: its rate does not depend on the size);
* the bootstrap (``bootstrap_medians``, hip backend) at ``--n`` rows per group and ``--reps`` resamples:
  the first call of the process (it builds the jump polynomials) and the steady state, against numpy's
  own path (seed + choice + gather + median) on the same arrays, timed at ``--numpy-reps`` resamples and
  scaled linearly to ``--reps`` (the full numpy run needs ~16 GB of host memory per group);
* the bytes the emit and select passes move (rank matrices written once, read once per radix pass)
  against 8 TB/s.

Per-kernel times: run it under ``rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_learn_cutoff.py``.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HEADER = ("ORF_ID\tORF_type\tstatus\tphase_score\tread_count\tlength\tvalid_codons\tvalid_codons_ratio\tread_density\t"
          "transcript_id\ttranscript_type\tgene_id\tgene_name\tgene_type\tchrom\tstrand\tstart_codon\tprofile\n")


def make_tsv(path: str, gb: float, seed: int = 1) -> None:
    """Rows with the export's columns and profiles of 30-1 200 values; a block of 2 000 rows repeated to the size."""
    rng = np.random.default_rng(seed)
    block = []
    for i in range(2000):
        L = int(rng.integers(30, 1200))
        prof = "[" + ", ".join(map(str, rng.integers(0, 3, L))) + "]"
        block.append(f"tx{i}_{i}_{i + L}_{L}\t{('annotated', 'uORF', 'dORF', 'novel')[i % 4]}\tnontranslating\t{rng.random()!r}\t"
                     f"{L // 3}\t{L}\t{L // 9}\t0.3\t0.1\ttx{i}\t{('protein_coding', 'lncRNA')[i % 2]}\tg{i}\tG{i}\tprotein_coding\t"
                     f"chr1\t+\tATG\t{prof}\n")
    text = "".join(block)
    with open(path, "w") as fh:
        fh.write(HEADER)
        for _ in range(int(gb * 1e9) // len(text) + 1):
            fh.write(text)


def bench_reader(path: str, pandas_mb: float) -> dict:
    import pandas as pd

    from ribotricer_amd import learn_cutoff as lc

    size = os.path.getsize(path)
    lc.read_cutoff_columns(path)  # page cache warm
    t0 = time.perf_counter()
    cols = lc.read_cutoff_columns(path)
    t_native = time.perf_counter() - t0
    head = path + ".head"
    with open(path, "rb") as src, open(head, "wb") as dst:
        dst.write(src.read(int(pandas_mb * 1e6)))
        dst.write(src.readline())
    hsize = os.path.getsize(head)
    pd.read_csv(head, sep="\t", usecols=lc.USECOLS)
    t0 = time.perf_counter()
    pd.read_csv(head, sep="\t", usecols=lc.USECOLS)
    t_pandas = time.perf_counter() - t0
    os.remove(head)
    return {"tsv_bytes": size, "rows": len(cols), "native_s": t_native, "native_GBps": size / t_native / 1e9,
            "pandas_bytes": hsize, "pandas_s": t_pandas, "pandas_GBps": hsize / t_pandas / 1e9,
            "threads": __import__("ribotricer_amd._lib", fromlist=["usable_cores"]).usable_cores()}


def bench_bootstrap(n: int, reps: int, numpy_reps: int, steady: int) -> dict:
    from ribotricer_amd import learn_cutoff as lc

    rng = np.random.default_rng(3)
    ribo, rna = rng.random(n), rng.random(n)
    t0 = time.perf_counter()
    lc.bootstrap_medians(ribo, rna, 0.33, reps)
    first = time.perf_counter() - t0
    first_ms = list(lc.bootstrap_medians.last_ms)
    walls, parts = [], []
    for _ in range(steady):
        t0 = time.perf_counter()
        got = lc.bootstrap_medians(ribo, rna, 0.33, reps)
        walls.append(time.perf_counter() - t0)
        parts.append(list(lc.bootstrap_medians.last_ms))
    # numpy's path, as the reference runs it, at numpy_reps resamples
    t0 = time.perf_counter()
    np.random.seed(42)
    ri = np.random.choice(range(n), (int(0.33 * n), numpy_reps))
    ni = np.random.choice(range(n), (int(0.33 * n), numpy_reps))
    want = np.median(ribo[ri], axis=0), np.median(rna[ni], axis=0)
    t_np = time.perf_counter() - t0
    sub = lc.bootstrap_medians(ribo, rna, 0.33, numpy_reps)
    equal = bool(np.array_equal(sub[0], want[0]) and np.array_equal(sub[1], want[1]))
    k = int(0.33 * n)
    draws = 2 * k * reps
    width = 4 if n > 65536 else 2
    passes = -(-int(np.ceil(np.log2(n))) // 8)
    emit_bytes = draws * width
    select_bytes = passes * draws * width
    med = float(np.median(walls))
    mid = parts[int(np.argsort(walls)[len(walls) // 2])]
    return {"n": n, "k": k, "reps": reps, "draws": draws, "first_call_s": first, "first_call_parts_ms": first_ms,
            "steady_s_median": med, "steady_s_all": walls, "steady_parts_ms": mid,
            "parts_legend": ["poly tables (host, first call)", "jump tree", "count pass", "emit pass", "select", "whole call",
                             "chunks", "words per chunk"],
            "numpy_reps": numpy_reps, "numpy_s": t_np, "numpy_s_scaled_to_reps": t_np * reps / numpy_reps,
            "numpy_equal_at_numpy_reps": equal,
            "emit_bytes_written": emit_bytes, "select_bytes_read": select_bytes, "radix_passes": passes,
            "emit_hbm_floor_ms_at_8TBps": emit_bytes / 8e12 * 1e3, "select_hbm_floor_ms_at_8TBps": select_bytes / 8e12 * 1e3,
            "emit_achieved_TBps": emit_bytes / (mid[3] * 1e-3) / 1e12 if mid[3] else None,
            "select_achieved_TBps": select_bytes / (mid[4] * 1e-3) / 1e12 if mid[4] else None, "medians_sample": float(got[0][0])}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300_000)
    ap.add_argument("--reps", type=int, default=20_000)
    ap.add_argument("--numpy-reps", type=int, default=1_000)
    ap.add_argument("--steady", type=int, default=5)
    ap.add_argument("--tsv-gb", type=float, default=2.0)
    ap.add_argument("--pandas-mb", type=float, default=300.0)
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--skip-reader", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"bootstrap": bench_bootstrap(a.n, a.reps, a.numpy_reps, a.steady)}
    if not a.skip_reader:
        path = os.path.join(a.tmp, "bench_learn_cutoff_report_all.tsv")
        t0 = time.perf_counter()
        make_tsv(path, a.tsv_gb)
        res["reader"] = bench_reader(path, a.pandas_mb)
        res["reader"]["make_s"] = time.perf_counter() - t0
        os.remove(path)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
