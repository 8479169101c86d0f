"""learn-cutoff on the MI355X: rp_bootstrap_medians_dev (the MT19937 stream by jump-ahead, masked-rejection draws as
value ranks, radix-selected medians) against the reference's own outputs (G13) and against numpy's own path on the
same arrays; determine_cutoff_bam over two builder BAMs."""

import contextlib
import io
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from ribotricer_amd import learn_cutoff as lc
from test_host_learn_cutoff_cpu import CASES, assert_case, medians_via_bootstrap

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hip_backend_equals_reference(case):
    assert_case(case, medians_via_bootstrap)


def numpy_path(ribo, rna, ratio, reps):
    np.random.seed(42)
    ri = np.random.choice(range(ribo.size), (int(ratio * ribo.size), reps))
    ni = np.random.choice(range(rna.size), (int(ratio * rna.size), reps))
    out = np.median(ribo[ri], axis=0), np.median(rna[ni], axis=0)
    return out, np.random.get_state()


@pytest.mark.parametrize("n", [4, 2**17, 2**17 + 1, 300_000])
@pytest.mark.parametrize("reps", [1, 2000])
def test_grid_against_numpy(n, reps):
    rng = np.random.default_rng(n + reps)
    ribo = np.round(rng.random(n), 4)  # ties: many equal values
    rna = rng.random(n)
    ratio = 0.33 if n > 4 else 0.5
    (want_r, want_n), want_state = numpy_path(ribo, rna, ratio, reps)
    got_r, got_n = lc.bootstrap_medians(ribo, rna, ratio, reps)
    assert np.array_equal(got_r.view(np.uint64), want_r.view(np.uint64))
    assert np.array_equal(got_n.view(np.uint64), want_n.view(np.uint64))
    state = np.random.get_state()
    assert np.array_equal(state[1], want_state[1]) and state[2] == want_state[2]


def test_large_draw_count():
    """2e8 draws over many chunks; the Ribo / RNA hand-off falls inside a chunk (the chunk length is 624 * 2^s, and the
    Ribo draws end at no particular word)."""
    n, reps = 303_031, 1000
    ratio = 0.33
    rng = np.random.default_rng(5)
    ribo = rng.random(n)
    rna = rng.random(n)
    (want_r, want_n), want_state = numpy_path(ribo, rna, ratio, reps)
    got_r, got_n = lc.bootstrap_medians(ribo, rna, ratio, reps)
    ms = lc.bootstrap_medians.last_ms
    assert ms[6] > 1  # several chunks
    assert np.array_equal(got_r.view(np.uint64), want_r.view(np.uint64))
    assert np.array_equal(got_n.view(np.uint64), want_n.view(np.uint64))
    state = np.random.get_state()
    assert np.array_equal(state[1], want_state[1]) and state[2] == want_state[2]


def test_determine_cutoff_bam(tmp_path, capsys):
    from bamwriter import write_bam

    from ribotricer_amd.detect_orfs import detect_orfs

    index = os.path.join(GOLDEN, "g6_index.tsv")
    starts = []  # 1-based first nt of the single-interval '+' ORFs: reads in frame 0 give the metagene its period
    for line in open(index).read().splitlines()[1:]:
        f = line.split("\t")
        if f[8] == "+" and "," not in f[10]:
            lo, hi = (int(x) for x in f[10].split("-"))
            starts.append((f[7], lo, hi))
    chroms = sorted({c for c, _, _ in starts})
    refs = [(c, 400000) for c in chroms]
    bams = []
    for seed, in_frame in ((1, 0.9), (2, 0.5)):  # Ribo-like and RNA-like (weaker period); >= 100 000 reads of one length
        rng = np.random.default_rng(seed)
        reads = []
        for _ in range(110_000):
            chrom, lo, hi = starts[int(rng.integers(len(starts)))]
            pos = lo - 1 + 3 * int(rng.integers(0, max(1, (hi - lo) // 3))) - 12
            if rng.random() >= in_frame:
                pos += int(rng.integers(1, 3))
            reads.append(dict(name="r", chrom=chrom, pos=max(0, pos), flag=0, mapq=255, cigar=[("M", 28)]))
        reads.sort(key=lambda r: (chroms.index(r["chrom"]), r["pos"]))
        path = str(tmp_path / f"s{seed}.bam")
        write_bam(path, refs, reads)
        bams.append(path)
    prefix = str(tmp_path / "lc" / "run")
    lc.determine_cutoff_bam([bams[0]], [bams[1]], index, prefix, ["forward"], ["forward"], reps=50)
    out = capsys.readouterr().out
    assert out.startswith("Running ribotricer on 1 Ribo-seq sample ..... \n")
    assert "Running ribotricer on 1 RNA-seq sample ..... \n" in out
    tail = out.splitlines()[-15:]
    for name, bam in (("ribo_bam_1", bams[0]), ("rna_bam_1", bams[1])):
        own = str(tmp_path / "own" / name)
        detect_orfs(bam, index, own, "forward", None, None, phase_score_cutoff=0.0, report_all=True)
        assert open(f"{prefix}__{name}_translating_ORFs.tsv").read() == open(f"{own}_translating_ORFs.tsv").read()
    capsys.readouterr()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        lc.determine_cutoff_tsv([f"{prefix}__ribo_bam_1_translating_ORFs.tsv"], [f"{prefix}__rna_bam_1_translating_ORFs.tsv"], reps=50)
    assert buf.getvalue().splitlines() == tail


def test_bam_needs_one_protocol_per_bam(tmp_path):
    with pytest.raises(SystemExit):
        lc.determine_cutoff_bam(["a.bam", "b.bam"], ["c.bam"], "index.tsv", str(tmp_path / "p"), ["forward"], ["forward"])
