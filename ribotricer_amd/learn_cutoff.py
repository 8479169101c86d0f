"""``ribotricer learn-cutoff`` (the reference's learn_cutoff.py) on this package's native pieces.

``determine_cutoff_tsv`` prints the reference's fifteen lines, byte for byte, and leaves numpy's global random state
where the reference leaves it.  Its two costs move off the Python host loop:

* reading the ``*_translating_ORFs.tsv`` files back: ``read_cutoff_columns`` (``rp_cutoff_read_host``, multi-threaded
  C++) returns the category codes of ``ORF_type`` / ``transcript_type`` and the phase with pandas' default float
  converter.  ``str.lower()``, the NA tokens and ``isin`` are applied here, in Python, to the few distinct strings.  A
  file with a construct the reader does not model sends its whole group to ``pandas.read_csv`` exactly as the
  reference calls it (recorded in ``timings["pandas_fallback"]``).
* the bootstrap: ``bootstrap_medians`` -- on the ``hip`` backend ``rp_bootstrap_medians_dev`` (the legacy MT19937
  stream by jump-ahead, masked-rejection draws as value ranks, radix-selected medians: csrc/rp_bootstrap.hpp); on the
  ``cpu`` backend numpy's own legacy ``RandomState`` path, as the reference runs it.

Everything computed over the ``reps`` medians or the ``n`` values (means, medians, sds, ``diff_all``) is numpy on
the host, as in the reference.
"""

from __future__ import annotations

import ctypes
import gzip
import mmap
import operator
import os
import re
import sys
import time

import numpy as np

from . import _lib, backend
from .const import (
    CUTOFF,
    MINIMUM_DENSITY_OVER_ORF,
    MINIMUM_READS_PER_CODON,
    MINIMUM_VALID_CODONS,
    MINIMUM_VALID_CODONS_RATIO,
)

USECOLS = ["ORF_ID", "ORF_type", "phase_score", "transcript_type"]
SEED = 42  # np.random.seed(42) of learn_cutoff.py:94
# pandas' default NA tokens (pandas._libs.parsers.STR_NA_VALUES): such a field is NaN, and NaN matches nothing
NA_TOKENS = frozenset(["", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>",
                       "N/A", "NA", "NULL", "NaN", "None", "n/a", "nan", "null"])
# a transcript_type text pandas might read as a number or a bool rather than a string
_NOT_TEXT = re.compile(r"\s*[+-]?((\d+\.?\d*|\.\d+)([eEdD][+-]?\d+)?|inf|infinity)\s*|true|false", re.I)
_FALLBACK = {2: "a '\"' byte", 3: "a lone carriage return", 4: "a row whose field count differs from the header's",
             5: "a phase text outside [+-]digits[.digits][e[+-]digits]", 6: "a byte-order mark or a duplicated column"}


class CutoffColumns:
    """What learn-cutoff needs of one TSV: per row the ``ORF_type`` / ``transcript_type`` category codes (int32) and
    ``phase`` (float64), and the distinct raw strings the codes stand for (``orf_cats`` / ``tx_cats``)."""

    def __init__(self, orf_type, tx_type, phase, orf_cats, tx_cats):
        self.orf_type, self.tx_type, self.phase = orf_type, tx_type, phase
        self.orf_cats, self.tx_cats = orf_cats, tx_cats

    def __len__(self) -> int:
        return int(self.phase.size)

    def selected(self, filter_by) -> np.ndarray:
        """Phases of the rows ``ORF_type == "annotated"`` with ``transcript_type.str.lower().isin(filter_by)``
        (``filter_by`` already lower-cased), in row order."""
        keep_o = np.array([s == "annotated" for s in self.orf_cats] + [False], bool)
        keep_t = np.array([s not in NA_TOKENS and s.lower() in filter_by for s in self.tx_cats] + [False], bool)
        return self.phase[keep_o[self.orf_type] & keep_t[self.tx_type]]

    def text_transcript_types(self) -> bool:
        """False when pandas could read this file's transcript_type column as numbers / bools (or all NaN): the reference
        then behaves differently (``.str`` on a non-string column), and the group is read by pandas."""
        return any(s not in NA_TOKENS and not _NOT_TEXT.fullmatch(s) for s in self.tx_cats)


def _missing_columns_error(path: str):
    """The ValueError pandas raises for absent usecols, raised by pandas itself on the header line alone."""
    import io

    import pandas as pd

    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as fh:
        head = fh.readline()
    pd.read_csv(io.BytesIO(head), sep="\t", usecols=USECOLS)
    raise ValueError(f"Usecols do not match columns: {path}")  # (not reached: pandas raised)


def read_cutoff_columns(path: str, n_threads: int = 0, timings: dict | None = None):
    """``rp_cutoff_read_host`` on one TSV (``.gz`` is decompressed first).  Returns ``CutoffColumns``, or ``None`` when
    the file holds a construct the reader does not model (the reason is recorded in ``timings["pandas_fallback"]``).
    Missing columns raise pandas' own ``ValueError``."""
    t0 = time.perf_counter()
    lib = _lib.load()
    n_threads = n_threads or _lib.usable_cores()
    mm = None
    if path.endswith(".gz"):
        with gzip.open(path, "rb") as fh:
            data = np.frombuffer(fh.read(), np.uint8)
    else:
        with open(path, "rb") as fh:
            size = os.fstat(fh.fileno()).st_size
            if size:
                mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
                data = np.frombuffer(mm, np.uint8)
            else:
                data = np.zeros(0, np.uint8)
    try:
        status, missing, bad_line, handle = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_void_p()
        _lib.check(lib.rp_cutoff_read_host(data.ctypes.data if data.size else None, data.size, n_threads, ctypes.byref(status),
                                           ctypes.byref(missing), ctypes.byref(bad_line), ctypes.byref(handle)))
    finally:
        del data
        if mm is not None:
            mm.close()
    if timings is not None:
        timings["read_native"] = timings.get("read_native", 0.0) + time.perf_counter() - t0
    if status.value == 1:
        _missing_columns_error(path)
    if status.value != 0:
        if timings is not None:
            timings.setdefault("pandas_fallback", []).append(f"{path}: {_FALLBACK.get(status.value, status.value)} (line {bad_line.value})")
        return None
    try:
        view = _lib.CutoffView()
        _lib.check(lib.rp_cutoff_view_host(handle, ctypes.byref(view)))
        n = view.n_rows

        def arr(ptr, ctype, count, dtype):
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), (count,)).astype(dtype, copy=True) if count else np.zeros(0, dtype)

        def cats(blob, off, count):
            offs = arr(off, ctypes.c_int64, count + 1, np.int64)
            raw = ctypes.string_at(blob, int(offs[-1])) if offs[-1] else b""
            return [raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(count)]

        return CutoffColumns(arr(view.orf_type, ctypes.c_int32, n, np.int32), arr(view.tx_type, ctypes.c_int32, n, np.int32),
                             arr(view.phase, ctypes.c_double, n, np.float64), cats(view.orf_cats, view.orf_cat_off, view.n_orf_cats),
                             cats(view.tx_cats, view.tx_cat_off, view.n_tx_cats))
    finally:
        lib.rp_cutoff_free(handle)


def _group_values_pandas(tsvs, filter_by) -> np.ndarray:
    """learn_cutoff.py:60-92 itself, for a group the native reader hands over."""
    import pandas as pd

    df_all = pd.DataFrame()
    for tsv in tsvs:
        df = pd.read_csv(tsv, sep="\t", usecols=USECOLS)
        df_all = pd.concat([df_all, df])
    filtered = df_all.loc[df_all.ORF_type == "annotated"]
    filtered = filtered.loc[filtered.transcript_type.str.lower().isin(filter_by)]
    return np.array(filtered.phase_score.tolist())


def group_values(tsvs, filter_by, timings: dict | None = None) -> np.ndarray:
    """The selected phases of one group (files concatenated in the given order)."""
    parts = []
    for tsv in tsvs:
        cols = read_cutoff_columns(tsv, timings=timings)
        if cols is None or not cols.text_transcript_types():
            if cols is not None and timings is not None:
                timings.setdefault("pandas_fallback", []).append(f"{tsv}: transcript_type is not a text column")
            t0 = time.perf_counter()
            out = _group_values_pandas(tsvs, filter_by)
            if timings is not None:
                timings["read_pandas"] = timings.get("read_pandas", 0.0) + time.perf_counter() - t0
            return out
        parts.append(cols.selected(filter_by))
    return np.concatenate(parts) if parts else np.zeros(0, np.float64)


def _check_shape(n: int, k, reps) -> None:
    """Raise what ``np.random.choice(range(n), (k, reps))`` raises for an invalid shape (nothing is drawn)."""
    try:
        ok = operator.index(k) >= 0 and operator.index(reps) >= 0
    except TypeError:
        ok = False
    if not ok:
        np.random.RandomState(0).choice(range(n), (k, reps))


def bootstrap_medians(ribo_values, rna_values, sampling_ratio, reps, device=None):
    """``(ribo_medians, rna_medians)`` of learn_cutoff.py:94-103: ``np.random.seed(42)``, ``int(sampling_ratio * n)``
    draws with replacement per resample and group (RNA continuing the stream), ``np.median(..., axis=0)``.  Leaves
    numpy's global random state where the reference leaves it."""
    ribo_values = np.asarray(ribo_values)
    rna_values = np.asarray(rna_values)
    n_r, n_n = int(ribo_values.shape[0]), int(rna_values.shape[0])
    k_r = int(sampling_ratio * n_r)
    k_n = int(sampling_ratio * n_n)
    if backend.selected() == "cpu":
        np.random.seed(SEED)
        ribo_idx = np.random.choice(range(n_r), (k_r, reps))
        rna_idx = np.random.choice(range(n_n), (k_n, reps))
        return np.median(ribo_values[ribo_idx], axis=0), np.median(rna_values[rna_idx], axis=0)
    np.random.seed(SEED)
    _check_shape(n_r, k_r, reps)
    _check_shape(n_n, k_n, reps)
    reps = operator.index(reps)
    for n, k in ((n_r, k_r), (n_n, k_n)):
        if n == 0 and k * reps:
            np.random.choice(range(n), (k, reps))  # numpy's own error ("a cannot be empty ...")
    vr = np.ascontiguousarray(ribo_values, dtype=np.float64)
    vn = np.ascontiguousarray(rna_values, dtype=np.float64)
    med_r = np.median(np.zeros((k_r, reps)), axis=0) if not (k_r and reps) else np.empty(reps, np.float64)
    med_n = np.median(np.zeros((k_n, reps)), axis=0) if not (k_n and reps) else np.empty(reps, np.float64)
    key = np.empty(624, np.uint32)
    pos = ctypes.c_int32(0)
    ms = (ctypes.c_float * 8)()
    dev = _device_index(device)
    lib = _lib.load()
    _lib.check(lib.rp_bootstrap_medians_dev(dev, vr.ctypes.data if vr.size else None, n_r, k_r, vn.ctypes.data if vn.size else None,
                                            n_n, k_n, reps, SEED, med_r.ctypes.data if med_r.size else None,
                                            med_n.ctypes.data if med_n.size else None, key.ctypes.data, ctypes.byref(pos), ms))
    np.random.set_state(("MT19937", key, pos.value, 0, 0.0))
    bootstrap_medians.last_ms = list(ms)
    return med_r, med_n


bootstrap_medians.last_ms = None  # the timings of the last hip call (rp_bootstrap_medians_dev ms[8])


def _device_index(device) -> int:
    if device is None:
        return 0
    if isinstance(device, int):
        return device
    text = str(device)
    return int(text.split(":")[1]) if ":" in text else 0


def determine_cutoff_tsv(ribo_tsvs, rna_tsvs, filter_by=None, sampling_ratio: float = 0.33, reps: int = 10000,
                         timings: dict | None = None) -> None:
    """learn_cutoff.py:35-144: the same fifteen lines on stdout."""
    if filter_by is None:
        filter_by = ["protein_coding"]
    filter_by = [x.lower() for x in filter_by]
    ribo = group_values(ribo_tsvs, filter_by, timings)
    rna = group_values(rna_tsvs, filter_by, timings)
    int(sampling_ratio * ribo.shape[0]), int(sampling_ratio * rna.shape[0])  # (the reference's errors, in its order)
    if ribo.shape[0] != rna.shape[0] and 1 not in (ribo.shape[0], rna.shape[0]):
        np.random.seed(SEED)
        _check_shape(ribo.shape[0], int(sampling_ratio * ribo.shape[0]), reps)
        _check_shape(rna.shape[0], int(sampling_ratio * rna.shape[0]), reps)
        ribo - rna  # the reference's ValueError (learn_cutoff.py:118), raised before any draw and any output
    t0 = time.perf_counter()
    ribo_phase_median_samples, rna_phase_median_samples = bootstrap_medians(ribo, rna, sampling_ratio, reps)
    if timings is not None:
        timings["bootstrap"] = time.perf_counter() - t0
    diff_phase_median_samples = ribo_phase_median_samples - rna_phase_median_samples
    diff_all = ribo - rna
    # learn_cutoff.py:105-144: the same numpy reductions, printed in the same order
    print(f"sampling_ratio: {sampling_ratio}")
    print(f"n_samples: {reps}")
    for name, values in (("ribo_phase_score", ribo_phase_median_samples), ("rna_phase_score", rna_phase_median_samples),
                         ("diff_phase_score_sampled", diff_phase_median_samples), ("diff_phase_score_all", diff_all)):
        print(f"{name}_mean: {np.mean(values):.3f}")
        print(f"{name}_median: {np.median(values):.3f}")
        print(f"{name}_sd: {np.std(values):.3f}")
    print(f"recommended_cutoff: {np.median(diff_phase_median_samples):.3f}")


def determine_cutoff_bam(ribo_bams, rna_bams, ribotricer_index, prefix, ribo_stranded_protocols=None,
                         rna_stranded_protocols=None, filter_by=None, sampling_ratio: float = 0.33, reps: int = 10000,
                         phase_score_cutoff: float = CUTOFF, min_valid_codons: int = MINIMUM_VALID_CODONS,
                         report_all: bool = True) -> None:
    """learn_cutoff.py:147-265: ``detect_orfs`` at cutoff 0 on every BAM (``phase_score_cutoff`` and
    ``min_valid_codons`` are ignored, as in the reference), then ``determine_cutoff_tsv`` over the TSVs it wrote.

    This package's ``detect_orfs`` does not infer the protocol, so each group takes one protocol ('forward' /
    'reverse') per BAM; anything else exits with a message (INTEGRATION.md lists the deviation)."""
    from .detect_orfs import detect_orfs

    if filter_by is None:
        filter_by = ["protein_coding"]
    for name, bams, protocols in (("Ribo-seq", ribo_bams, ribo_stranded_protocols), ("RNA-seq", rna_bams, rna_stranded_protocols)):
        if protocols is None or len(protocols) != len(bams) or any(p not in ("forward", "reverse") for p in protocols):
            sys.exit(f"Error: ribotricer_amd.determine_cutoff_bam needs one protocol ('forward' or 'reverse') per {name} bam "
                     "(protocol inference is not part of this engine)")

    sample_str = "samples"
    if len(rna_bams) == 1:
        sample_str = "sample"
    print(f"Running ribotricer on {len(rna_bams)} Ribo-seq {sample_str} ..... \n")
    ribo_bams_renamed = dict(zip(ribo_bams, [f"ribo_bam_{i + 1}" for i in range(len(ribo_bams))]))
    rna_bams_renamed = dict(zip(rna_bams, [f"rna_bam_{i + 1}" for i in range(len(rna_bams))]))

    def run(bam, stranded, bam_prefix):
        parent = os.path.dirname(os.path.abspath(bam_prefix))
        os.makedirs(parent, exist_ok=True)
        detect_orfs(bam, ribotricer_index, bam_prefix, stranded, read_lengths=None, psite_offsets=None, phase_score_cutoff=0.0,
                    min_valid_codons=MINIMUM_VALID_CODONS, min_reads_per_codon=MINIMUM_READS_PER_CODON,
                    min_valid_codons_ratio=MINIMUM_VALID_CODONS_RATIO, min_density_over_orf=MINIMUM_DENSITY_OVER_ORF,
                    report_all=report_all)
        return f"{bam_prefix}_translating_ORFs.tsv"

    ribo_tsvs = [run(bam, p, f"{prefix}__{ribo_bams_renamed[bam]}") for bam, p in zip(ribo_bams, ribo_stranded_protocols)]
    print(f"Running ribotricer on {len(rna_bams)} RNA-seq {sample_str} ..... \n")
    rna_tsvs = [run(bam, p, f"{prefix}__{rna_bams_renamed[bam]}") for bam, p in zip(rna_bams, rna_stranded_protocols)]
    determine_cutoff_tsv(ribo_tsvs, rna_tsvs, filter_by, sampling_ratio, reps)
