#!/usr/bin/env python3
"""Generate the G13 fixtures (learn-cutoff) FROM THE REFERENCE ITSELF.

Run only where the reference is mounted read-only (as make_golden.py):

    python tests/golden/make_golden_cutoff.py     # writes tests/golden/g13_*

For every case it writes the input TSVs (``*_translating_ORFs.tsv``-shaped), then calls the reference's
``ribotricer.learn_cutoff.determine_cutoff_tsv`` (``pysam`` / ``quicksect`` stubbed: module-level imports of packages
not installed here) and records its stdout, the exception type it raised (if any), the two per-resample median arrays
(captured from its ``np.median(..., axis=0)`` calls) and ``np.random.get_state()`` after the call.  Only inputs and
outputs are written; tests read these files and never the reference.

  g13_cases.json        the cases: files, filter_by, sampling_ratio, reps, stdout, error
  g13_<case>_*.tsv.gz   inputs (gzip)
  g13_results.npz       <case>_ribo / <case>_rna medians, <case>_key / <case>_pos state
"""

from __future__ import annotations

import contextlib
import gzip
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("RIBOTRICER_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
for _m in ("pysam", "quicksect"):
    sys.modules.setdefault(_m, types.ModuleType(_m))
sys.modules["quicksect"].Interval = object
sys.modules["quicksect"].IntervalTree = dict
from ribotricer.learn_cutoff import determine_cutoff_tsv  # noqa: E402  (the reference)

HEADER = ["ORF_ID", "ORF_type", "status", "phase_score", "read_count", "length", "valid_codons", "transcript_id",
          "transcript_type", "gene_id", "chrom", "strand", "profile"]
ORF_TYPES = ["annotated", "annotated", "annotated", "uORF", "dORF", "novel"]
TX_TYPES = ["protein_coding", "protein_coding", "Protein_Coding", "PROTEIN_CODING", "lncRNA", "NA", "", "None"]


def phase_text(rng, style: str) -> str:
    v = float(rng.random())
    if style == "repr":
        return repr(v)
    if style == "small":  # [0.001, 0.01): leading zeros count toward pandas' 17 digits
        return repr(0.001 + 0.009 * v)
    if style == "long":  # 17+ significant digits
        return f"{v:.22f}"
    if style == "exp":
        return f"{v:.9e}" if rng.random() < 0.5 else f"{v * 1e-3:.17E}"
    return "0" if v < 0.5 else "1"


def rows(rng, n: int, layout, styles, nan_rows=()):
    out = []
    for i in range(n):
        ot, tt = layout[i]
        text = "nan" if i in nan_rows else phase_text(rng, styles[i % len(styles)])
        prof = "[" + ", ".join(str(int(x)) for x in rng.integers(0, 4, int(rng.integers(3, 9)))) + "]"
        out.append([f"tx{i}_{i * 3}_{i * 3 + 300}_300", ot, "translating", text, str(int(rng.integers(0, 90))), "300", "5",
                    f"ENST{i:07d}", tt, f"ENSG{i:07d}", "chr1", "+", prof])
    return out


def layout_for(rng, n: int, all_selected: bool = False):
    if all_selected:
        return [("annotated", "protein_coding")] * n
    return [(ORF_TYPES[rng.integers(len(ORF_TYPES))], TX_TYPES[rng.integers(len(TX_TYPES))]) for _ in range(n)]


def write(name: str, table, crlf: bool = False, quote_row: int | None = None) -> str:
    """One input TSV, gzip-compressed (pandas and the native reader both take `.gz`; mtime 0: reproducible bytes)."""
    name += ".gz"
    eol = "\r\n" if crlf else "\n"
    lines = ["\t".join(HEADER) + eol]
    for i, r in enumerate(table):
        if quote_row == i:
            r = list(r)
            r[9] = '"ENSG_quoted"'
        lines.append("\t".join(r) + eol)
    with open(os.path.join(HERE, name), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as fh:
        fh.write("".join(lines).encode("utf-8"))
    return name


def main() -> None:
    rng = np.random.default_rng(20261015)
    styles = ["repr", "repr", "small", "long", "exp"]
    cases = []

    # two files per group, mixed-case / NA transcript types, every phase-text style, a CRLF file, a file with a '"'
    lay = [layout_for(rng, 240), layout_for(rng, 180)]
    cases.append(dict(name="multi", ribo=[write("g13_multi_ribo_1.tsv", rows(rng, 240, lay[0], styles)),
                                          write("g13_multi_ribo_2.tsv", rows(rng, 180, lay[1], styles), crlf=True)],
                      rna=[write("g13_multi_rna_1.tsv", rows(rng, 240, lay[0], styles), quote_row=7),
                           write("g13_multi_rna_2.tsv", rows(rng, 180, lay[1], styles))],
                      filter_by=None, sampling_ratio=0.33, reps=7))
    lay = layout_for(rng, 150)
    cases.append(dict(name="filter", ribo=[write("g13_filter_ribo.tsv", rows(rng, 150, lay, styles))],
                      rna=[write("g13_filter_rna.tsv", rows(rng, 150, lay, styles))],
                      filter_by=["Protein_Coding", "LNCRNA"], sampling_ratio=0.5, reps=7))
    lay = layout_for(rng, 60, True)
    cases.append(dict(name="nanphase", ribo=[write("g13_nanphase_ribo.tsv", rows(rng, 60, lay, styles, nan_rows={17}))],
                      rna=[write("g13_nanphase_rna.tsv", rows(rng, 60, lay, styles))], filter_by=None, sampling_ratio=0.33, reps=7))
    # acceptance ~1 (n = 2^b) and ~1/2 (n = 2^b + 1); odd and even k
    for name, n, ratio in (("pow2", 1024, 0.33), ("pow2p1", 1025, 0.5)):
        lay = layout_for(rng, n, True)
        cases.append(dict(name=name, ribo=[write(f"g13_{name}_ribo.tsv", rows(rng, n, lay, ["repr"]))],
                          rna=[write(f"g13_{name}_rna.tsv", rows(rng, n, lay, ["repr", "int"]))],
                          filter_by=None, sampling_ratio=ratio, reps=7))
    # k = 0, k = 1, reps = 0 / 1, n = 1 with sampling_ratio 1.0 (no words), n = 1 against n = 40 (broadcasts)
    for name, nr, nn, ratio, reps in (("k0", 2, 2, 0.33, 7), ("k1", 4, 4, 0.25, 7), ("reps0", 50, 50, 0.33, 0),
                                       ("reps1", 50, 50, 0.33, 1), ("n1", 1, 1, 1.0, 7), ("n1vs40", 1, 40, 1.0, 7),
                                       ("mismatch", 10, 12, 0.33, 7), ("wide", 3000, 3000, 0.33, 2000)):
        cases.append(dict(name=name, ribo=[write(f"g13_{name}_ribo.tsv", rows(rng, nr, layout_for(rng, nr, True), styles))],
                          rna=[write(f"g13_{name}_rna.tsv", rows(rng, nn, layout_for(rng, nn, True), styles))],
                          filter_by=None, sampling_ratio=ratio, reps=reps))

    arrays = {}
    real_median = np.median
    for case in cases:
        captured = []

        def median(a, *args, **kwargs):
            out = real_median(a, *args, **kwargs)
            if kwargs.get("axis") == 0 or (args and args[0] == 0):
                captured.append(np.array(out, copy=True))
            return out

        buf = io.StringIO()
        error = None
        np.median = median
        cwd = os.getcwd()
        os.chdir(HERE)
        try:
            with contextlib.redirect_stdout(buf):
                determine_cutoff_tsv(case["ribo"], case["rna"], case["filter_by"], case["sampling_ratio"], case["reps"])
        except Exception as exc:  # noqa: BLE001  (recorded: the port must raise the same type)
            error = type(exc).__name__
        finally:
            np.median = real_median
            os.chdir(cwd)
        case["stdout"] = buf.getvalue()
        case["error"] = error
        state = np.random.get_state()
        arrays[f"{case['name']}_key"] = np.asarray(state[1], np.uint32)
        arrays[f"{case['name']}_pos"] = np.int64(state[2])
        if error is None:
            arrays[f"{case['name']}_ribo"], arrays[f"{case['name']}_rna"] = captured[0], captured[1]
        print(case["name"], error or case["stdout"].splitlines()[-1])
    np.savez_compressed(os.path.join(HERE, "g13_results.npz"), **arrays)
    with open(os.path.join(HERE, "g13_cases.json"), "w") as fh:
        fh.write('{"numpy": %s, "cases": [\n' % json.dumps(np.__version__))
        fh.write(",\n".join(json.dumps(c) for c in cases) + "\n]}\n")


if __name__ == "__main__":
    main()
