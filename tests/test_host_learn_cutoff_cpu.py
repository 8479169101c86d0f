"""learn-cutoff on the host: the MT19937 jump, the native column reader against pandas, and the cpu backend's
determine_cutoff_tsv against the reference's own outputs (G13, tests/golden/make_golden_cutoff.py)."""

import contextlib
import gzip
import io
import json
import os

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN
from ribotricer_amd import _lib
from ribotricer_amd import learn_cutoff as lc

CASES = json.load(open(os.path.join(GOLDEN, "g13_cases.json")))["cases"]
RESULTS = np.load(os.path.join(GOLDEN, "g13_results.npz"))
G13_FILES = sorted({f for c in CASES for f in c["ribo"] + c["rna"]})


def numpy_state_after(offset: int):
    bg = np.random.RandomState(42)._bit_generator
    left = offset
    while left:
        step = min(left, 1 << 24)
        bg.random_raw(step)
        left -= step
    st = bg.state["state"]
    return np.asarray(st["key"], np.uint32), int(st["pos"])


@pytest.mark.parametrize("offset", [0, 1, 623, 624, 625, 10**6 + 17, 2**30 + 5])
def test_host_jump_equals_numpy_mt19937(offset):
    key = np.empty(624, np.uint32)
    pos = _lib.load().rp_mt19937_state_host(42, offset, key.ctypes.data)
    want_key, want_pos = numpy_state_after(offset)
    assert pos == want_pos
    assert np.array_equal(key, want_key)


def assert_reader_equals_pandas(path):
    cols = lc.read_cutoff_columns(path)
    df = pd.read_csv(path, sep="\t", usecols=lc.USECOLS)
    if cols is None:  # a construct the reader hands to pandas: only the '"' fixture
        assert b'"' in (gzip.open(path) if path.endswith(".gz") else open(path, "rb")).read()
        return
    assert len(cols) == len(df)
    want = df.phase_score.to_numpy(np.float64)
    assert np.array_equal(cols.phase.view(np.uint64), want.view(np.uint64)), path
    for codes, cats, col in ((cols.orf_type, cols.orf_cats, df.ORF_type), (cols.tx_type, cols.tx_cats, df.transcript_type)):
        raw = np.array(cats, object)[codes]
        na = np.array([s in lc.NA_TOKENS for s in raw])
        assert np.array_equal(na, col.isna().to_numpy()), path
        assert list(raw[~na]) == [str(v) for v in col[~na]], path


@pytest.mark.parametrize("name", G13_FILES + ["g6_expected_report_all.tsv", "g10_expected_report_all.tsv", "g10_expected_default.tsv",
                                              "g10_expected_strict.tsv", "g12_expected_report_all.tsv.gz"])
def test_reader_equals_pandas_on_fixtures(name):
    assert_reader_equals_pandas(os.path.join(GOLDEN, name))


def corner_strings():
    return ["0.0012345678901234567", "0.00999999999999999999", "1.00000000000000000001", "123456789012345678.5", "-0.0", "+0.5",
            "4.9e-324", "2.5e-320", "1e-330", "2.2250738585072014e-308", "00000.000000001234567890123", "1E5", "1e+05", "1e-05",
            "7.0E-3", "0.000000000000000000000000000000001", "1.7976931348623157e308", "9e-310", "123456789012345",
            "0", "1", "0.5", "nan", "NA", "", "NaN", "null", "None", "-nan", "<NA>", "#N/A", "n/a"]


def test_reader_equals_pandas_on_random_reprs(tmp_path):
    """pandas' default float converter (not correctly rounded) on a million random reprs and the corners."""
    rng = np.random.default_rng(7)
    n = 1_000_000
    x = rng.random(n) * 10.0 ** rng.uniform(-12, 3, n)
    texts = [repr(float(v)) for v in x]
    texts += [f"{v:.20f}" for v in x[:20000]] + [f"{v:.12e}" for v in x[20000:40000]] + corner_strings()
    path = tmp_path / "random_translating_ORFs.tsv"
    with open(path, "w") as fh:
        fh.write("ORF_ID\tORF_type\tphase_score\ttranscript_type\tprofile\n")
        for i, t in enumerate(texts):
            fh.write(f"o{i}\tannotated\t{t}\tprotein_coding\t[{i % 7}, 1]\n")
    cols = lc.read_cutoff_columns(str(path))
    want = pd.read_csv(path, sep="\t", usecols=lc.USECOLS).phase_score.to_numpy(np.float64)
    assert cols is not None and cols.phase.size == want.size
    bad = np.flatnonzero(cols.phase.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, [texts[i] for i in bad[:10]]
    # a correctly rounded reader would not pass: pandas' default converter differs from float() on many of these
    assert sum(float(t).hex() != w.hex() for t, w in zip(texts[:100000], want[:100000])) > 1000


@pytest.mark.parametrize("text,reason", [("0.5\t\"x\"", 2), ("inf", 5), (" 0.5", 5), ("0x1p-3", 5), ("1234567890123456", 5), ("-0", 5)])
def test_reader_hands_unmodelled_files_to_pandas(tmp_path, text, reason):
    path = tmp_path / "t.tsv"
    path.write_text("ORF_ID\tORF_type\tphase_score\ttranscript_type\textra\n" + f"a\tannotated\t{text}\tprotein_coding\tz\n".replace("\tz\n", "\tz\n" if "\t" not in text else "\n"))
    timings = {}
    assert lc.read_cutoff_columns(str(path), timings=timings) is None
    assert timings["pandas_fallback"]


def test_reader_missing_column_raises_pandas_error(tmp_path):
    path = tmp_path / "t.tsv"
    path.write_text("ORF_ID\tORF_type\ttranscript_type\na\tannotated\tprotein_coding\n")
    with pytest.raises(ValueError) as mine:
        lc.read_cutoff_columns(str(path))
    with pytest.raises(ValueError) as theirs:
        pd.read_csv(path, sep="\t", usecols=lc.USECOLS)
    assert str(mine.value) == str(theirs.value)


def run_case(case):
    out = io.StringIO()
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    error = None
    try:
        with contextlib.redirect_stdout(out):
            lc.determine_cutoff_tsv(case["ribo"], case["rna"], case["filter_by"], case["sampling_ratio"], case["reps"])
    except Exception as exc:  # noqa: BLE001
        error = type(exc).__name__
    finally:
        os.chdir(cwd)
    return out.getvalue(), error


def assert_case(case, medians_of):
    np.random.seed(0)
    stdout, error = run_case(case)
    assert error == case["error"]
    assert stdout == case["stdout"]
    if error is not None:
        assert stdout == ""
        return
    name = case["name"]
    key = np.asarray(np.random.get_state()[1], np.uint32)
    assert np.array_equal(key, RESULTS[f"{name}_key"]) and np.random.get_state()[2] == int(RESULTS[f"{name}_pos"])
    ribo, rna = medians_of(case)
    assert np.array_equal(ribo.view(np.uint64), RESULTS[f"{name}_ribo"].view(np.uint64))
    assert np.array_equal(rna.view(np.uint64), RESULTS[f"{name}_rna"].view(np.uint64))


def medians_via_bootstrap(case):
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        f = [x.lower() for x in (case["filter_by"] or ["protein_coding"])]
        ribo, rna = lc.group_values(case["ribo"], f), lc.group_values(case["rna"], f)
    finally:
        os.chdir(cwd)
    return lc.bootstrap_medians(ribo, rna, case["sampling_ratio"], case["reps"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cpu_backend_equals_reference(case, monkeypatch):
    monkeypatch.setenv("RIBOTRICER_AMD_BACKEND", "cpu")
    assert_case(case, medians_via_bootstrap)


def test_invalid_arguments_raise_what_the_reference_raises(monkeypatch):
    monkeypatch.setenv("RIBOTRICER_AMD_BACKEND", "cpu")
    v = np.linspace(0, 1, 10)
    with pytest.raises(ValueError):
        lc.bootstrap_medians(v, v, -0.5, 5)
    with pytest.raises(ValueError):
        lc.bootstrap_medians(v, v, 0.5, -1)
    with pytest.raises(TypeError):
        lc.bootstrap_medians(v, v, 0.5, 2.5)
