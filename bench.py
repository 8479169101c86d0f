#!/usr/bin/env python3
"""bench.py -- ORFs phase-scored per second on N MI355X (BASELINE.json metric).

Workload (BASELINE.json): ONE seeded synthetic candidate-ORF set of 11 M ORFs with the
GENCODE-like length law of ribotricer_amd/synth.py "cfg3" (3.97 G nt, 16 GB of int32
P-site counts, resident in HBM):
    N = 1   configs[2]  the whole set on one MI355X
    N > 1   configs[3]  the SAME set cut into N nt-balanced ORF-index slices
                        (ribotricer_amd/sharding.py), one slice per GPU, no collective on
                        the data path -> "scaling": "strong".  With --full, after the timed
                        steps rank 0 scores the whole set on its own GPU and checks that
                        the concatenation of the ranks' results equals it.
A "step" is one pass of the hot path over the rank's slice: libribophase
rp_phase_score_csr_plan_dev = scoring kernel (rp::k_tile_score) + per-ORF finish kernel.
The tile plan (tile index + offsets validation, rp_plan_create_dev) depends on the index
only and is built once before the steps, the way `detect-orfs` reuses one index for every
sample; its time is reported as `plan_build_ms`, and `value_single_sample` is the rate with
the plan rebuilt inside every step (an index used for ONE sample).

    python bench.py --gpus 1 --steps 50 --warmup 5
    python bench.py --gpus 1 --steps 50 --warmup 5 --full   (the headline, then everything else below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N --steps K --warmup W      (no launcher: bench.py starts its own N ranks)

Without a launcher (WORLD_SIZE unset) and N > 1 this process never touches the GPU: it starts the N ranks
as fresh child processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set), relays
rank 0's JSON line and exits with the ranks' status (`self_launch`).  When the node shows fewer GPUs than
ranks (the one-GPU test box), the ranks share GPUs round-robin, the control traffic runs over gloo, and the
line says so (`config.ranks_share_gpus`): a self-test of the N-rank control flow, not a scaling measurement.

Once per index and outside the timed region, like the plan build: `engine.tune_workspace` tries a few
placements of the ENGINE'S OWN record workspace and keeps the fastest (on MI355X a write stream costs a read stream
10 % or 23 % depending on the classes of physical memory the two buffers lie in);
`--no-tune-workspace` switches it off and `value_first_allocation` is the step before the search.  The COUNTS stay
where the caller's allocation put them for the headline: no product path moves a caller's array.  What moving them
as well would give (`engine.tune_source`: copies behind spacers until the kernel runs at the fast class's rate) is
timed AFTER the headline with the same K steps and reported as `value_source_placed` (`--no-tune-source`: skip).

A PLAIN run does what the headline needs and nothing more: it sets up (the set, the plan, the workspace search and
the first-allocation steps before it), warms up, times the K steps, writes --dump-outputs and prints rank 0's ONE JSON
line: the contract fields, `config`, `per_rank` and (search run) `value_first_allocation`.  `--dump-outputs DIR` writes the per-ORF
arrays the last timed step computed (every ORF, or a fixed seeded sample of a larger set) as DIR/<name>.npy, so that two
builds can be compared output for output on the same seeded inputs; `--detail FILE` writes the full record -- every
block with its explanations -- beside the line.  Everything else runs only with `--full`, after the timed steps.

With --full the line (under 8 KB) also carries `roofline`, `cpu_baseline`, `verify` and the numbers that matter as
top-level scalars (`kernel_ms`, `finish_ms`, `step_frac`, `fused_step_frac`, `fused_nested_step_frac`,
`projected_efficiency_g8`, `value_source_placed`, `value_pipelined`, ...).  `roofline` is for the dominant kernel (algorithmic bytes
B = 4*sum(L) + 8*(n+1) + 24*n per launch over its HIP-event duration, vs the 8 TB/s
HBM peak); `cpu_baseline` is the literal scipy restatement of the reference's phasescore
(oracle/phasescore_literal.py) on all host cores, on a bounded sample of the same set.
AFTER the timed region (N = 1, --full): `verify` -- head / middle / tail slices of 20 000 ORFs and the
ORFs around 2^31 / 2^32 nt of what the steps computed, against the C oracle on the same bytes
(integers bit-exact, phase <= 1e-6, exact frame ties bit for bit) -- and `fused` / `fused_nested` -- what
the drop-in export runs by default (gather + score fused, rp::k_tile_score<true>, with RP_FILTER_PRINTED_ONLY as
the export's default mode sets it; the all-resolved step beside it, the two compared over the whole set) on an
exon layout of the same length law / a nested-transcript index, each with its own `verify` -- and `roofline.stream_read` -- a plain
streaming read of the same counts buffer in the same process (csrc/stream_probe.hip), the yardstick
next to which `frac_of_stream_read` puts the kernel (the kernel's time depends on where its buffers
lie, by up to 15 % from process to process; the plain read does not; `record_write_penalty` there says
which case this run was: DESIGN.md section 4).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CFG_NAMES = {"cfg2": "BASELINE configs[1]", "cfg3": "BASELINE configs[2]", "cfg5": "BASELINE configs[4]",
             "gencode": "GENCODE-like candidate set (67 % of the ORFs 60-150 nt)",
             "gencode_short": "uORF/dORF-dominated candidate set (77 % of the ORFs 60-150 nt)"}
DEFAULT_ORFS = {"cfg2": 1_000_000, "cfg3": 11_000_000, "cfg5": 20_000_000, "gencode": 11_000_000, "gencode_short": 11_000_000}
VERIFY_SLICE = 20_000  # ORFs per slice of the after-the-fact oracle check
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cfg", default="cfg3", choices=list(CFG_NAMES))
    ap.add_argument("--orfs", type=int, default=0, help="ORFs of the whole set (default: the config's size)")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="strong: one set sharded over the GPUs (configs[3]); weak: --orfs ORFs on every GPU")
    ap.add_argument("--algo", default="auto", choices=["auto", "wave", "tile"])
    ap.add_argument("--no-plan", action="store_true", help="rebuild the tile index inside every step")
    ap.add_argument("--cpu-sample", type=int, default=12000, help="ORFs per process for the CPU baseline (--full; 0 = skip)")
    ap.add_argument("--cpu-cores", type=int, default=0, help="processes for the CPU baseline (default: the usable cores, at most 64)")
    ap.add_argument("--no-verify", action="store_true", help="with --full: skip the oracle check of head / middle / tail slices (N = 1) and the concat == whole check (N > 1)")
    ap.add_argument("--no-tune-workspace", action="store_true", help="keep the record workspace where the first allocation put it (engine.tune_workspace off)")
    ap.add_argument("--no-tune-source", action="store_true", help="with --full: keep the synthetic counts / coverage where the first allocation put them (engine.tune_source off)")
    ap.add_argument("--no-pipelined", action="store_true", help="with --full: skip the two-stream many-samples section (N = 1); "
                    "with or without --full, the headline's record workspace is then one workspace instead of a block of two")
    ap.add_argument("--no-slice-projection", action="store_true", help="with --full: skip timing rank 0's slice of the 2 / 4 / 8-GPU runs on this one GPU (N = 1)")
    ap.add_argument("--no-fused", action="store_true", help="with --full: skip the fused gather + score section (N = 1)")
    ap.add_argument("--no-fused-nested", action="store_true", help="with --full: skip the nested-index fused section (N = 1)")
    ap.add_argument("--no-fused-exons", action="store_true", help="with --full: skip the fused section on the run's own length law (N = 1; counter passes that want the nested launches alone)")
    ap.add_argument("--dense-coverage", action="store_true", help="fused sections over the dense coverage layout (default: the compact one the export builds)")
    ap.add_argument("--coverage-block", type=int, default=None, help="positions per block of the compact coverage (default: the export's, gather.COVERAGE_BLOCK)")
    ap.add_argument("--fused-steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=20260213)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else the bench measures and checks: per-kernel times and the roofline, the "
                         "slice projection, the single-sample, two-stream and source-placed rates, the oracle checks (N = 1) and the "
                         "concat == whole check (N > 1), the fused sections, the plain-read yardstick and the CPU baselines.  Without "
                         "it a run sets up, warms up, times the steps, writes --dump-outputs and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (phase, valid, read_count, min_codon_cov, "
                         "flags, status and the ORF index of each row) as DIR/<name>.npy in float64: every ORF, or a fixed seeded "
                         "sample of 2^20 ORFs when there are more (N > 1: rank 0's slice)")
    ap.add_argument("--detail", default=None, help="write the FULL record (every block with its explanations: placement searches, per-slice "
                    "verification, gather-plan statistics, ...) to this file; stdout carries the compact line (< 8 KB) either way")
    return ap.parse_args()


def vbios_versions():
    """The GPUs' VBIOS versions as the amdgpu driver reports them (sysfs; no GPU call).  Round 4 found the boxes on which
    no workspace placement helps (kernel 2.86-3.06 ms) on 113-M355-01-1K1-020F and the ones where it does (2.6-2.7 ms) on
    -030A (profiles/archive/r04_box_kinds.txt): the line carries the version so that a reader can tell which kind a run met."""
    import glob

    seen = []
    for path in sorted(glob.glob("/sys/class/drm/card*/device/vbios_version")):
        try:
            v = open(path).read().strip()
        except OSError:
            continue
        if v and v not in seen:
            seen.append(v)
    return seen


DUMP_MAX_ORFS = 1 << 20  # 7 float64 arrays of this length: 56 MiB, under the 64 MB a dump may take
DUMP_SAMPLE_SEED = 12345


def dump_outputs(out, n_orfs: int, path: str) -> None:
    """--dump-outputs: the per-ORF arrays the caller of the timed path receives, as float64 .npy files (exact for every
    integer column).  More ORFs than DUMP_MAX_ORFS: the same seeded sample of ORF indices in every run, sorted."""
    import numpy as np
    import torch

    if n_orfs <= DUMP_MAX_ORFS:
        rows = np.arange(n_orfs, dtype=np.int64)
    else:
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n_orfs, size=DUMP_MAX_ORFS, replace=False)).astype(np.int64)
    idx = torch.from_numpy(rows).to(out.phase.device)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "orf_index.npy"), rows.astype(np.float64))
    for name in ("phase", "valid", "read_count", "min_codon_cov", "flags", "status"):
        t = getattr(out, name)
        if t is not None:
            np.save(os.path.join(path, f"{name}.npy"), t.index_select(0, idx).cpu().numpy().astype(np.float64))


def usable_cores():
    """Cores this process may really use: the scheduler affinity, capped by the cgroup CPU quota
    (the GPU boxes show 256 CPUs with a 16-CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(pool, counts_host, offsets_host, per_core):
    """Reference-equivalent CPU path on a bounded sample: pure-Python triplet loop +
    scipy.signal.coherence per frame (oracle/phasescore_literal.py), all cores via a
    process pool and one core alone; plus the best-effort C closed form (OpenMP)."""
    import numpy as np

    from oracle import c_oracle
    from oracle.phasescore_literal import phasescore_literal

    n_done, wall, n_workers = pool.run(counts_host, offsets_host, per_core)
    base = {
        "value": n_done / wall,
        "unit": "ORFs/s",
        "cores": n_workers,
        "kind": "port",
        "sample": f"first {n_done} ORFs of the set ({int(offsets_host[n_done])} nt), {n_done // n_workers} per process, "
        f"oracle/phasescore_literal.py (python triplet loop + scipy.signal.coherence) on {n_workers} processes "
        f"of a host with {usable_cores()} usable cores ({os.cpu_count()} visible), {wall:.1f} s wall",
    }
    n1 = min(per_core, offsets_host.size - 1)
    profiles = [counts_host[offsets_host[i] : offsets_host[i + 1]].tolist() for i in range(n1)]
    t0 = time.perf_counter()
    for p in profiles:
        phasescore_literal(p)
    dt = time.perf_counter() - t0
    one = {"value": n1 / dt, "unit": "ORFs/s", "cores": 1, "kind": "port",
           "sample": f"first {n1} ORFs, same code on one core, {dt:.1f} s"}
    # best-effort CPU: C closed form on all host cores over a larger sample
    cores = usable_cores()
    n_c = min(200_000, offsets_host.size - 1)
    c_oracle.build()
    c = np.ascontiguousarray(counts_host[: offsets_host[n_c]])
    o = np.ascontiguousarray(offsets_host[: n_c + 1])
    c_oracle.phase_score_csr(c, o, n_threads=cores)  # (threads started, pages touched)
    reps = 10  # the sample takes ~15 ms on 16 cores: time several passes
    t0 = time.perf_counter()
    for _ in range(reps):
        c_oracle.phase_score_csr(c, o, n_threads=cores)
    dt_c = (time.perf_counter() - t0) / reps
    extra = {"value": n_c / dt_c, "unit": "ORFs/s", "cores": cores, "kind": "port",
             "sample": f"first {n_c} ORFs, oracle/phase_oracle.c closed form + OpenMP, mean of {reps} passes of {dt_c * 1e3:.1f} ms"}
    # the reference's own float64 arithmetic (every scipy / numpy operation restated, libm pow included) in C++ on
    # all cores: libribophase's rp_phase_score_csr_host -- bit-exact with the reference, and what "the reference
    # without the Python interpreter" would cost
    from ribotricer_amd import _lib

    _lib.phase_score_csr_host(c[: int(o[2000])], o[:2001], n_threads=cores)
    t0 = time.perf_counter()
    _lib.phase_score_csr_host(c, o, n_threads=cores)
    dt_x = time.perf_counter() - t0
    exact = {"value": n_c / dt_x, "unit": "ORFs/s", "cores": cores, "kind": "port",
             "sample": f"first {n_c} ORFs, rp_phase_score_csr_host (the reference's float64 operation sequence in C++, bit-exact), one pass of {dt_x * 1e3:.0f} ms"}
    return base, one, extra, exact


def measured_traffic(cfg, n_orfs, algo, seed, kernel="rp::k_tile_score<false>"):
    """HBM bytes per launch of the dominant kernel, REPLAYED from the committed rocprofv3 PMC passes of this very command
    (profiles/traffic.json: FETCH_SIZE and WRITE_SIZE in KiB from separate --pmc runs), each counter times its CALIBRATED
    factor for the kernel's access pattern (`fetch_factor` / `write_factor` of the record; profiles/r06_fetch_calibration.txt:
    FETCH_SIZE x 2.0000 for 16-byte-per-lane loads AND for the fused kernel's dword LDS-DMA chunks, WRITE_SIZE x 1.0000 for the
    nt record stores).  Counters cannot be read from inside the run, so this is None unless a profile of exactly this
    workload is on file.  Returns (bytes, source, fetch_factor)."""
    path = os.path.join(REPO, "profiles", "traffic.json")
    if not os.path.exists(path):
        return None, None, None
    with open(path) as fh:
        for rec in json.load(fh):
            if (rec["cfg"] == cfg and rec["orfs_per_gpu"] == n_orfs and rec["algo"] == algo and rec["seed"] == seed
                    and rec.get("kernel", "rp::k_tile_score<false>") == kernel):
                ff, wf = float(rec.get("fetch_factor", 2.0)), float(rec.get("write_factor", 1.0))
                return int((ff * rec["fetch_size_kib"] + wf * rec["write_size_kib"]) * 1024), rec.get("source", "profiles/traffic.json"), ff
    return None, None, None


def verify_slices(out, counts, offsets, n_orfs, profiles_of=None):
    """AFTER the timed region: head / middle / tail slices (and the ORFs around 2^31 / 2^32 nt) of
    what the steps computed, against the C oracle on the same bytes (oracle/verify.py: integers
    bit-exact, phase <= 1e-6, exact frame ties bit for bit).  The oracle is the checker here, never
    the thing measured.  ``profiles_of(lo, hi)``: host CSR of ORFs lo..hi when ``counts`` is not a
    CSR array (the fused section)."""
    import numpy as np

    from oracle import verify
    from ribotricer_amd.engine import csr_profiles_of, resolve_big_ties

    off = offsets.cpu().numpy()
    n = n_orfs
    k = min(VERIFY_SLICE, n)
    ranges = {"head": (0, k), "middle": (max(0, n // 2 - k // 2), min(n, n // 2 - k // 2 + k)), "tail": (n - k, n)}
    for label, b in (("at_2^31_nt", 1 << 31), ("at_2^32_nt", 1 << 32)):
        if int(off[-1]) > b:
            i = int(np.searchsorted(off, b))
            ranges[label] = (max(0, i - k // 4), min(n, i + k // 4))
    rep = {"ok": True, "orfs_checked": 0, "max_abs_dphase": 0.0, "ties_bit_exact": 0, "slices": {}}
    keys = ("phase", "valid", "read_count", "min_codon_cov", "flags", "status")
    for label, (lo, hi) in ranges.items():
        part = {kk: getattr(out, kk)[lo:hi].cpu().numpy() for kk in keys}
        if profiles_of is None:
            a, b = int(off[lo]), int(off[hi])
            c_host, o_host = counts[a:b].cpu().numpy(), off[lo : hi + 1] - off[lo]
        else:
            c_host, o_host = profiles_of(lo, hi)
        resolve_big_ties(part, csr_profiles_of(c_host, o_host))
        try:
            st = verify.check_slice(part, c_host, o_host)
        except AssertionError as e:
            rep["ok"] = False
            rep["slices"][label] = {"orfs": [lo, hi], "error": str(e)}
            continue
        rep["orfs_checked"] += hi - lo
        rep["max_abs_dphase"] = max(rep["max_abs_dphase"], st["max_abs_dphase"])
        rep["ties_bit_exact"] += st["ties"]
        rep["slices"][label] = {"orfs": [lo, hi], "first_nt": int(off[lo]), "max_abs_dphase": st["max_abs_dphase"], "ties": st["ties"]}
    return rep


def fused_section(args, eng, dev, thresholds, n_set, layout="exons"):
    """What `export_orf_coverages` runs by default: gather + score FUSED (rp_phase_score_coverage_dev,
    k_tile_score<true>) over a candidate index laid out as exons over a dense coverage array.
    layout "exons":  the run's own length law (synth_exon_layout: 1-4 exons per ORF, introns < 300 nt, half of the
                     ORFs on '-', ORFs one after the other);
    layout "nested": the law of scripts/gen_big_index.cpp (synth_nested_layout: transcripts with nested candidate ORFs
                     that share coverage, 65 % of them 60-150 nt, ~2 exons per ORF, consecutive transcripts on
                     different chromosomes -- the pieces of one tile lie gigabytes apart)."""
    import statistics
    import time

    import numpy as np
    import torch

    from ribotricer_amd.gather import GatherPlan, IntervalTable, gather_profiles_device, select_orfs
    from ribotricer_amd.synth import orf_lengths, profiles_from_coverage, synth_coverage_device, synth_exon_layout, synth_nested_layout

    if layout == "nested":
        iv_start, iv_len, orf_iv, reverse, offsets, coverage_len = synth_nested_layout(n_set, args.seed)
        law = "nested candidate ORFs of the gen_big_index law (65 % 60-150 nt, transcripts on 48 chromosome / strand groups)"
    else:
        lengths = orf_lengths(n_set, args.seed, args.cfg)
        iv_start, iv_len, orf_iv, reverse, offsets, coverage_len = synth_exon_layout(lengths, args.seed)
        law = f"the {args.cfg} length law (introns < 300 nt, half of the ORFs on the '-' strand)"
    table = IntervalTable(iv_start, iv_len, orf_iv, reverse, offsets)
    dense_len = coverage_len
    map_ms = block = None
    if not args.dense_coverage:
        # what the export does since round 4: a COMPACT coverage -- only the positions (blocks of --coverage-block) under an
        # exon keep a slot (gather.CoverageMap); the synthetic counts are drawn straight into the compact array
        from ribotricer_amd.gather import CoverageMap

        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        cmap = CoverageMap(table, dense_len, dev, block_positions=args.coverage_block)
        block = cmap.block_positions
        torch.cuda.synchronize(dev)
        map_ms = 1e3 * (time.perf_counter() - t0)
        table, coverage_len = cmap.table, cmap.compact_len
        iv_start = table.iv_start
        cmap.release_device_intervals()
    cov = synth_coverage_device(coverage_len, args.seed, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    gplan = GatherPlan(table, coverage_len, dev)
    torch.cuda.synchronize(dev)
    gplan_ms = 1e3 * (time.perf_counter() - t0)
    placement = None
    if not args.no_tune_workspace and int(offsets[-1]) >= (64 << 20):  # (as for the CSR path: once per index, not timed)
        placement = eng.tune_workspace(cov, thresholds=thresholds, gather_plan=gplan)
        # (the coverage itself stays where the first allocation put it: the export never moves it)
        if placement.get("spacers"):
            time.sleep(min(3.0, 0.5 * placement.get("spacers", 0)))
    # The export's default mode prints translating rows only and says so to the library (RP_FILTER_PRINTED_ONLY: a
    # too-close-to-call ORF that no resolution could make translating is not re-walked, detect_orfs.export_orf_coverages):
    # THAT is the step of this section.  The same launches with every ORF resolved (what report_all and the CSR headline
    # run) are timed beside it, and checked against each other over the whole set below.
    from ribotricer_amd import _lib
    from ribotricer_amd.engine import make_filter

    printed = make_filter(thresholds.phase_score_cutoff, thresholds.min_valid_codons, thresholds.min_reads_per_codon,
                          thresholds.min_valid_codons_ratio, thresholds.min_density_over_orf, printed_only=True)
    for _ in range(5):
        full = eng.score_coverage(cov, gplan, thresholds=thresholds, reuse_outputs=False)
    tm_full: list = []
    for _ in range(max(3, args.fused_steps)):
        full = eng.score_coverage(cov, gplan, thresholds=thresholds, reuse_outputs=False, timings=tm_full)
    for _ in range(5):
        out = eng.score_coverage(cov, gplan, thresholds=printed, reuse_outputs=True)
    tm: list = []
    for _ in range(max(3, args.fused_steps)):
        out = eng.score_coverage(cov, gplan, thresholds=printed, reuse_outputs=True, timings=tm)
    k_main = statistics.median(t[1] for t in tm)  # (medians: this section's clocks follow whatever ran before it)
    k_fin = statistics.median(t[2] for t in tm)
    k_all = statistics.median(t[3] for t in tm)
    k_fin_full = statistics.median(t[2] for t in tm_full)
    k_all_full = statistics.median(t[3] for t in tm_full)
    torch.cuda.synchronize(dev)
    left_open = (out.flags & _lib.FLAG_UNRESOLVED).ne(0)
    rewalked = (full.flags & _lib.FLAG_RECHECK64).ne(0)
    same = bool(torch.equal(out.status, full.status)) and not bool(out.status[left_open].any())
    for key in ("phase", "valid", "read_count", "min_codon_cov", "flags"):
        same = same and bool(torch.equal(getattr(out, key)[~left_open], getattr(full, key)[~left_open]))
    same = same and not bool((left_open & ~rewalked).any())
    printed_check = {"ok": same, "orfs_checked": int(left_open.numel()), "left_open": int(left_open.sum()), "rewalked_when_all_resolved": int(rewalked.sum())}
    out = full  # (the oracle check below is of the fully resolved results; the printed-only ones were just compared with them)
    n = offsets.size - 1
    total_nt = int(offsets[-1])
    algo_bytes = 4 * total_nt + 8 * (n + 1) + 24 * n
    rep = {
        "workload": f"{n} ORFs / {iv_len.size} exons over a " + (f"dense coverage of {coverage_len} positions" if args.dense_coverage else
                    f"compact coverage of {coverage_len} positions (the {block}-position blocks under an exon; the dense layout spans {dense_len})")
                    + f" ({total_nt} nt of profiles): {law}",
        "coverage_positions": coverage_len, "dense_layout_positions": dense_len, "coverage_block": block, "coverage_map_build_ms": map_ms,
        "kernel": "rp::k_tile_score<true> (tile staged from the coverage through the gather plan)",
        "kernel_ms": k_main, "finish_ms": k_fin, "step_device_ms": k_all,
        "achieved": algo_bytes / (k_main * 1e-3) / 1e9, "frac": algo_bytes / (k_main * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "step_frac": algo_bytes / (k_all * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "value": n / (k_all * 1e-3), "unit": "ORFs/s",
        "mode": "default mode of the export: RP_FILTER_PRINTED_ONLY",
        "all_resolved": {"finish_ms": k_fin_full, "step_device_ms": k_all_full, "step_frac": algo_bytes / (k_all_full * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "value": n / (k_all_full * 1e-3)},
        "printed_only_check": printed_check,
        "gather_plan_build_ms": gplan_ms, "gather_plan": gplan.stats(),
        "workspace_placement": placement if placement is not None else "first allocation (engine.tune_workspace not run)",
        "algorithmic_bytes_per_launch": algo_bytes,
        "translating": int(out.status.sum()),
    }
    rep["traffic"], rep["traffic_source"], rep["fetch_factor"] = measured_traffic(args.cfg if layout == "exons" else "nested", n, "tile", args.seed,
                                                                                  kernel="rp::k_tile_score<true>")
    if not args.no_verify:
        if layout == "nested":  # neighbouring ORFs lie gigabytes apart: fetch the slices with the per-ORF gather kernel (a code path of its own)
            def profiles_of(lo, hi):
                c_dev, o_dev = gather_profiles_device(cov, select_orfs(table, np.arange(lo, hi, dtype=np.int64)), dev)
                return c_dev.cpu().numpy(), o_dev.cpu().numpy()
        else:
            def profiles_of(lo, hi):
                k0, k1 = int(orf_iv[lo]), int(orf_iv[hi])
                w_lo = int(iv_start[k0:k1].min())
                w_hi = int((iv_start[k0:k1] + iv_len[k0:k1]).max())
                return profiles_from_coverage(cov[w_lo:w_hi].cpu().numpy(), w_lo, iv_start, iv_len, orf_iv, reverse, lo, hi)

        rep["verify"] = verify_slices(out, None, gplan.offsets, n, profiles_of)
        rep["verify"]["ok"] = rep["verify"]["ok"] and printed_check["ok"]
    del cov, gplan, full
    torch.cuda.empty_cache()
    return rep


def self_launch(args) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks as FRESH child processes
    -- this parent has not imported torch and never touches the GPU (a process that has initialised the GPU must not
    exec another program on this pool; children started before any HIP call are fine) -- one rank per GPU, rendezvous
    on 127.0.0.1.  Rank 0's stdout (the one JSON line) is relayed to ours, the other ranks' output goes to stderr;
    returns rank 0's exit status, or the first non-zero status of another rank.  A rank that dies takes the others
    down (exact PIDs, after a grace period) instead of leaving them at a barrier for ever."""
    import socket
    import subprocess
    import threading

    import tempfile

    n = args.gpus
    # The ranks meet through a FILE store in a directory of this launch's own (torch.distributed's file:// rendezvous):
    # no port is picked here and handed on, so two bench runs on one box -- or anybody else's listener -- cannot take
    # it in between.  (MASTER_ADDR / MASTER_PORT are still exported for libraries that read them; the port is a free
    # one at this moment, nothing of ours depends on it staying free.)
    rdzv_dir = tempfile.mkdtemp(prefix="rp_bench_rdzv_")
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    base_env = dict(os.environ)
    base_env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this host driver (RCCL needs it)
    base_env.update(WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                    RP_BENCH_SELF_LAUNCHED="1", RP_BENCH_RDZV_FILE=os.path.join(rdzv_dir, "store"))
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    procs = []
    for r in range(n):
        env = dict(base_env, RANK=str(r), LOCAL_RANK=str(r), GROUP_RANK="0")
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True, cwd=os.getcwd()))

    def relay(proc, rank):
        for line in proc.stdout:
            if rank == 0:
                sys.stdout.write(line)
                sys.stdout.flush()
            else:
                sys.stderr.write(f"[rank {rank}] {line}")

    import signal

    def stop_ranks(signum=None, frame=None):  # the parent is being stopped (a driver's timeout): do not leave ranks on the GPUs
        for p in procs:
            if p.poll() is None:
                p.terminate()
        if signum is not None:
            sys.exit(128 + signum)

    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, stop_ranks)
    threads = [threading.Thread(target=relay, args=(p, r), daemon=True) for r, p in enumerate(procs)]
    for t in threads:
        t.start()
    status = [None] * n
    failed_at = None
    while any(s is None for s in status):
        for r, p in enumerate(procs):
            if status[r] is None:
                status[r] = p.poll()
                if status[r] not in (None, 0) and failed_at is None:
                    failed_at = time.monotonic()
        if failed_at is not None and time.monotonic() - failed_at > 20.0:
            for r, p in enumerate(procs):  # the others are parked at a barrier the dead rank will never reach
                if status[r] is None:
                    p.kill()
        time.sleep(0.05)
    for t in threads:
        t.join(timeout=5.0)
    import shutil

    shutil.rmtree(rdzv_dir, ignore_errors=True)
    if status[0] != 0:
        return status[0] if status[0] > 0 else 1
    bad = [s for s in status if s != 0]
    return (bad[0] if bad[0] > 0 else 1) if bad else 0


def init_gloo(dist, rank: int, world: int):
    """The process group proper (gloo).  Self-launched ranks (and a one-rank RP_BENCH_FORCE_DIST run) meet through a file
    store -- no port to lose to somebody else --, ranks under a launcher through the launcher's env:// rendezvous.  A
    rendezvous that cannot complete fails after 5 minutes, not 30."""
    import datetime

    timeout = datetime.timedelta(minutes=5)
    path = os.environ.get("RP_BENCH_RDZV_FILE")
    if path:
        dist.init_process_group(backend="gloo", init_method="file://" + path, rank=rank, world_size=world, timeout=timeout)
    else:
        dist.init_process_group(backend="gloo", timeout=timeout)


def launch_only(rank: int, world: int) -> None:
    """RP_BENCH_LAUNCH_ONLY=1 (tests/test_sharding_cpu.py, no GPU): the rendezvous, the barrier, the max-over-ranks
    and the per-rank gather of the real run over gloo, with the slices of the real index -- everything of the N-rank
    control flow except the device work."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from ribotricer_amd.sharding import slice_bounds
    from ribotricer_amd.synth import offsets_from_lengths, orf_lengths

    args = parse_args()
    if os.environ.get("RP_BENCH_LAUNCH_ONLY_SLEEP"):  # (the launcher's clean-up, under test: ranks that are still busy when the parent is stopped)
        time.sleep(float(os.environ["RP_BENCH_LAUNCH_ONLY_SLEEP"]))
    init_gloo(dist, rank, world)
    n_set = args.orfs if args.orfs > 0 else DEFAULT_ORFS[args.cfg]
    offsets_set = offsets_from_lengths(orf_lengths(n_set, args.seed, args.cfg))
    bounds = slice_bounds(offsets_set, world)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])
    dist.barrier()
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ranks = [None] * world
    dist.all_gather_object(ranks, {"rank": rank, "orfs": hi - lo, "nt": int(offsets_set[hi] - offsets_set[lo]),
                                   "local_rank": int(os.environ.get("LOCAL_RANK", "-1")), "pid": os.getpid()})
    if rank == 0:
        emit_line(json.dumps({"launch_only": True, "n_gpus": world, "max_over_ranks": float(t.item()), "per_rank": ranks,
                          "orfs_total": n_set, "nt_total": int(offsets_set[-1]),
                          "self_launched": os.environ.get("RP_BENCH_SELF_LAUNCHED") == "1"}))
    dist.barrier()
    dist.destroy_process_group()
    if os.environ.get("RP_BENCH_LAUNCH_ONLY_FAIL_RANK") == str(rank):  # (the launcher's status relay, under test)
        sys.exit(7)


def ctypes_stream(torch, dev):
    import ctypes

    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_json_out = None


def claim_stdout() -> None:
    """The process's stdout is for the ONE JSON line.  Libraries write there too -- RCCL prints its version banner
    through C stdio, which on a pipe is flushed at exit, i.e. BEHIND the JSON line -- so file descriptor 1 is pointed at
    stderr for everybody else (C level: every library; Python's own `print` included) and the line goes out through a
    private duplicate of the original."""
    global _json_out
    if _json_out is None:
        sys.stdout.flush()
        _json_out = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def emit_line(text: str) -> None:
    out = _json_out if _json_out is not None else sys.stdout
    out.write(text + "\n")
    out.flush()


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(full: dict) -> dict:
    """The ONE JSON line: the contract fields and the config, and (--full) the roofline and cpu_baseline blocks and every
    number a reader of the driver's record needs as a top-level scalar -- under 8 KB (tests/test_gpu_bench_contract.py).  The explanations
    (`what` texts), the placement searches' step lists, per-slice verification records, gather-plan statistics and
    per-process baselines live in the full record (`--detail FILE`; DESIGN.md section 6 explains every field)."""
    line = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                        "dtype", "data"))
    cfg = full["config"]
    line["config"] = _pick(cfg, ("workload", "orfs_total", "nt_total", "orfs_rank0", "nt_rank0", "algo", "plan_build_ms", "physical_gpus",
                                 "ranks_share_gpus", "launcher", "control_backend"))
    wp = cfg.get("workspace_placement")
    if isinstance(wp, dict):
        line["config"]["workspace_placement"] = {"searched": True, "chosen": wp.get("chosen"), "candidates": len(wp.get("step_ms", [])),
                                                 "step_ms_first": (wp.get("step_ms") or [None])[0],
                                                 "step_ms_chosen": wp["step_ms"][wp["chosen"]] if wp.get("step_ms") and wp.get("chosen") is not None else None,
                                                 "settled": wp.get("settled")}
    else:
        line["config"]["workspace_placement"] = {"searched": False}
    roof = full.get("roofline")  # (--full only)
    if roof is not None:
        line["roofline"] = _pick(roof, ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "fetch_factor", "kernel", "rank",
                                        "node_achieved", "node_peak", "kernel_ms", "algorithmic_bytes_per_launch", "step_device_ms", "step_achieved",
                                        "step_frac", "frac_of_stream_read"))
        line["roofline"]["finish_ms"] = roof["aux_kernels_ms"]["orf_finish"]
        line["roofline"]["tile_index_ms"] = roof["aux_kernels_ms"]["tile_index"]
        if roof.get("stream_read"):
            line["roofline"]["stream_read_GBps"] = roof["stream_read"]["GBps"]
            pen = roof["stream_read"].get("record_write_penalty")
            if pen:
                line["roofline"]["record_write_penalty"] = [round(x, 4) for x in pen["penalty"]]
        # the scalars (they survive a flattening reader)
        line["kernel_ms"] = roof["kernel_ms"]
        line["finish_ms"] = roof["aux_kernels_ms"]["orf_finish"]
        line["step_frac"] = roof["step_frac"]
    for key in ("value_first_allocation", "value_source_placed", "value_pipelined", "value_one_stream_repeat", "value_single_sample"):
        if key in full:
            line[key] = full[key]
    for tag in ("fused", "fused_nested"):
        f = full.get(tag)
        if f is None:
            continue
        line[f"{tag}_step_frac"] = f["step_frac"]
        line[f"{tag}_finish_ms"] = f["finish_ms"]
        line[f"{tag}_step_frac_all_resolved"] = f["all_resolved"]["step_frac"]
        block = _pick(f, ("kernel_ms", "finish_ms", "step_device_ms", "achieved", "frac", "step_frac", "value", "unit", "mode", "traffic",
                          "traffic_source", "fetch_factor", "algorithmic_bytes_per_launch", "translating", "coverage_positions",
                          "dense_layout_positions", "gather_plan_build_ms"))
        block["all_resolved"] = _pick(f["all_resolved"], ("finish_ms", "step_device_ms", "step_frac"))
        block["left_open"] = f["printed_only_check"]["left_open"]
        block["rewalked_when_all_resolved"] = f["printed_only_check"]["rewalked_when_all_resolved"]
        block["printed_only_check_ok"] = f["printed_only_check"]["ok"]
        if "verify" in f:
            block["verify"] = _pick(f["verify"], ("ok", "orfs_checked", "max_abs_dphase", "ties_bit_exact"))
        wpf = f.get("workspace_placement")
        block["workspace_searched"] = isinstance(wpf, dict)
        line[tag] = block
    proj = full.get("slice_projection")
    if proj is not None:
        for row in proj["slices"]:
            line[f"projected_efficiency_g{row['gpus']}"] = row["projected_efficiency"]
        line["slice_projection"] = [_pick(r, ("gpus", "orfs", "step_ms", "kernel_ms", "finish_ms", "step_frac", "projected_value", "projected_efficiency",
                                              "integers_equal_headline")) for r in proj["slices"]]
    if "pipelined" in full:
        line["pipelined"] = _pick(full["pipelined"], ("two_streams_ms_per_step", "one_stream_ms_per_step", "steps", "results_equal_headline"))
    if "source_placed" in full:
        sp = full["source_placed"]
        line["source_placed"] = {"ms_per_step": sp["ms_per_step"], "steps": sp["steps"], "chosen": sp["search"].get("chosen"),
                                 "kernel_gbps": [round(x) for x in sp["search"].get("kernel_gbps", [])]}
    if "first_allocation" in full:
        line["first_allocation_ms_per_step"] = full["first_allocation"]["ms_per_step"]
    if "single_sample" in full:
        line["single_sample_ms_per_step"] = full["single_sample"]["ms_per_step"]
    line["per_rank"] = [_pick(r, ("rank", "device", "orfs", "nt", "kernel_ms", "finish_ms", "step_device_ms", "frac")) for r in full["per_rank"]]
    if "quality" in full:
        line["quality"] = full["quality"]
    if "verify" in full:
        v = full["verify"]
        line["verify"] = _pick(v, ("ok", "orfs_checked", "max_abs_dphase", "ties_bit_exact", "read_count_checksum_ok", "read_count_checksum"))
        if isinstance(v.get("slices"), dict):
            line["verify"]["slices"] = sorted(v["slices"])
        if "concat_equals_whole" in v:
            line["verify"]["concat_equals_whole"] = _pick(v["concat_equals_whole"], ("ok", "orfs_checked", "max_abs_dphase"))
    for key in ("cpu_baseline", "cpu_baseline_1core", "cpu_closed_form_c", "cpu_reference_arithmetic_cpp"):
        if key in full:
            line[key] = full[key] if key == "cpu_baseline" else _pick(full[key], ("value", "unit", "cores", "kind"))
    return line


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))
    claim_stdout()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:  # the launcher's world size is what runs
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; running {world} ranks", file=sys.stderr)
    if os.environ.get("RP_BENCH_LAUNCH_ONLY") == "1":
        return launch_only(rank, world)

    # CPU-baseline workers first (--full): they must exist before this process initialises the GPU
    pool = None
    if args.full and rank == 0 and world == 1 and args.cpu_sample > 0:
        from oracle.cpu_pool import CpuPool

        pool = CpuPool(args.cpu_cores if args.cpu_cores > 0 else min(usable_cores(), 64))

    import numpy as np
    import torch

    n_dev = torch.cuda.device_count()
    if n_dev == 0:
        sys.exit("bench.py measures the hip backend: it needs a HIP device")
    local_dev = local_rank % n_dev  # one rank per GPU on the driver's node; wraps only in 1-GPU self-tests
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    dist = None
    backend = None
    forced_dir = None
    rccl = None  # the RCCL group (barriers around the timed region, max over ranks) when it came up
    side = None  # (objects and result hand-over use the default group: gloo)
    if world > 1 or os.environ.get("RP_BENCH_FORCE_DIST") == "1":
        import datetime

        import torch.distributed as dist

        # There is no collective on the data path.  The process group proper is gloo (host tensors: per-rank reports, the
        # results handed to rank 0 for the concat == whole check after the timed region); RCCL ("nccl") -- one rank per
        # GPU over xGMI -- is a second group that carries the barriers around the timed region and the max-over-ranks of
        # the elapsed time.  It is PROBED first (one all_reduce + barrier, the ranks then agree over gloo whether it
        # worked): a node whose RCCL cannot come up still gets its scaling line, with config.control_backend saying so.
        # Fewer GPUs than ranks (the one-GPU test box): ranks share GPUs round-robin, two ranks on one device cannot form
        # an RCCL communicator -> gloo only (config.ranks_share_gpus); RP_BENCH_BACKEND overrides.
        want = os.environ.get("RP_BENCH_BACKEND", "nccl" if n_dev >= world else "gloo")
        if world == 1 and "RP_BENCH_RDZV_FILE" not in os.environ and "MASTER_PORT" not in os.environ:
            # RP_BENCH_FORCE_DIST: the N-rank control flow with one rank (RCCL init / barrier / all_reduce on one GPU);
            # a file store of its own instead of a guessed port
            import tempfile

            forced_dir = tempfile.mkdtemp(prefix="rp_bench_rdzv_")
            os.environ["RP_BENCH_RDZV_FILE"] = os.path.join(forced_dir, "store")
        init_gloo(dist, rank, world)
        backend = "gloo"
        if want == "nccl":
            ok, why = 1, ""
            # (a collective that hangs must end in an exception on the waiting thread, not in the watchdog tearing the
            # process down: blocking waits raise on their timeout)
            os.environ.setdefault("TORCH_NCCL_BLOCKING_WAIT", "1")
            try:
                rccl = dist.new_group(backend="nccl", timeout=datetime.timedelta(minutes=3))
                probe = torch.ones(1, dtype=torch.float64, device=dev)
                dist.all_reduce(probe, group=rccl)
                torch.cuda.synchronize(dev)
                if int(probe.item()) != world:
                    raise RuntimeError(f"RCCL all_reduce gave {probe.item()} for {world} ranks")
                dist.barrier(group=rccl)
            except Exception as e:  # noqa: BLE001 -- whatever RCCL raises, the run goes on over gloo
                ok, why = 0, f"{type(e).__name__}: {e}"[:300]
            agreed = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(agreed, op=dist.ReduceOp.MIN)
            if int(agreed.item()) == 1:
                backend = "nccl"
            else:
                rccl = None
                backend = "gloo (RCCL probe failed" + (f" on this rank: {why}" if why else " on another rank") + ")"
                if rank == 0:
                    print("bench.py: " + backend, file=sys.stderr)

    from ribotricer_amd import _lib
    from ribotricer_amd.engine import PhaseScoreEngine, make_filter
    from ribotricer_amd.sharding import slice_bounds
    from ribotricer_amd.synth import offsets_from_lengths, orf_lengths, synth_csr_device

    n_set = args.orfs if args.orfs > 0 else DEFAULT_ORFS[args.cfg]
    strong = args.scaling == "strong"
    if strong:
        # every rank derives the same index (lengths come from numpy: identical everywhere) and
        # materialises only its own nt-balanced slice of the one seeded set
        offsets_set = offsets_from_lengths(orf_lengths(n_set, args.seed, args.cfg))
        bounds = slice_bounds(offsets_set, world)
        lo, hi = int(bounds[rank]), int(bounds[rank + 1])
        counts, offsets = synth_csr_device(n_set, seed=args.seed, cfg=args.cfg, device=dev, orf_range=(lo, hi))
        n_job = n_set
    else:
        lo, hi = 0, n_set
        counts, offsets = synth_csr_device(n_set, seed=args.seed + 1000 * rank, cfg=args.cfg, device=dev)
        n_job = n_set * world
    n_orfs = offsets.numel() - 1
    total_nt = counts.numel()
    eng = PhaseScoreEngine(dev)
    if world == 1 and not args.no_pipelined:
        # (a stream's workspace is a block of two: the second serves the other stream of the two-stream trial -- with or
        # without --full, so that the headline's steps write into the same kind of block either way)
        eng.workspace_copies = 2
    thresholds = make_filter()
    algo = args.algo
    resolved = ("tile" if total_nt >= (2 << 20) else "wave") if algo == "auto" else algo
    plan = None
    plan_ms = 0.0
    if resolved == "tile" and not args.no_plan and n_orfs > 0:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        plan = eng.plan_for(offsets, total_nt, (counts.data_ptr() // 4) % 4)  # validates the offsets, syncs
        plan_ms = 1e3 * (time.perf_counter() - t0)

    def step():
        return eng.score(counts, offsets, thresholds=thresholds, algo=algo, reuse_outputs=True, plan=plan)

    placement = None
    first_alloc_ms = None
    shared_gpu = world > max(1, torch.cuda.device_count())  # (the one-GPU self-test of the N-rank flow: no searches that allocate tens of GiB per rank)
    if plan is not None and not args.no_tune_workspace and total_nt >= (64 << 20) and not shared_gpu:
        # once per index, like the plan and outside the timed region: where the record workspace lies relative to the
        # counts decides between 2.6 and 3.0 ms per launch on this part; the engine tries a few
        # placements, keeps the fastest and frees the rest -- exactly what the drop-in export does once per cached index
        # (detect_orfs.score_index).  Reported in config.workspace_placement; --no-tune-workspace switches it off.
        # Before it: the same step on the workspace as FIRST allocated (what a process gets without the search),
        # reported as value_first_allocation.  These steps run without --full too: they bring the clocks up before the
        # search times its first candidate, so that the search keeps the same workspace with and without --full.
        lib_tag = _lib.load()
        was_tag = lib_tag.rp_measurement_tag(1)  # (these launches and the search's run under the second kernel name: a profiler's
        n_first = max(3, min(args.steps, 20))    #  statistics of rp::k_tile_score hold the headline's launches only)
        for _ in range(3):
            step()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_first):
            step()
        e1.record()
        torch.cuda.synchronize(dev)
        first_alloc_ms = e0.elapsed_time(e1) / n_first
        # (copies=2: every candidate is a block of TWO workspaces side by side -- the second one serves the other stream
        # of the two-stream section below, so both samples in flight write where this search found the writes cheapest)
        two_streams = world == 1 and not args.no_pipelined
        placement = eng.tune_workspace(counts, offsets, thresholds=thresholds, copies=2 if two_streams else 1)
        # (the COUNTS stay where they are for the headline: they are the caller's array at the C ABI, and no product path
        # moves them.  What moving them too would give is timed AFTER the headline: value_source_placed below.)
        lib_tag.rp_measurement_tag(was_tag)
        if placement.get("spacers"):
            # the driver wipes the memory handed back in the background, which takes 1-4 % off the kernels meanwhile (and
            # an idle wait would let the clocks drop): run untimed steps until two batches of ten in a row run at the
            # speed the search itself measured on the workspace it kept (+0.5 %; five fresh processes of round 5 read
            # 2.948 ms per step in the timed region against 2.914 on the same, unmoved workspace before the search, with
            # the old rule "two batches within 0.5 % of the best seen, at most 4 s" ending after 0.36 s) -- at most 6 s;
            # then the W warm-up steps and the K timed ones as always
            t_settle, calm = time.perf_counter(), 0
            best_seen = placement["step_ms"][placement["chosen"]] if placement.get("step_ms") else None
            target = 10.0 * (1.005 * best_seen + 0.01) if best_seen else float("inf")
            lib_tag.rp_measurement_tag(1)
            while time.perf_counter() - t_settle < 6.0 and calm < 2:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    step()
                e1.record()
                torch.cuda.synchronize(dev)
                calm = calm + 1 if e0.elapsed_time(e1) <= target else 0
            lib_tag.rp_measurement_tag(was_tag)
            placement["settled_after_s"] = round(time.perf_counter() - t_settle, 3)
            placement["settled"] = calm >= 2

    def barrier():
        if dist is not None:
            dist.barrier(group=rccl)  # (rccl None: the default group, gloo)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)
    barrier()
    torch.cuda.synchronize(dev)
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()  # torch's current stream IS the stream the library launches on
    for _ in range(args.steps):
        out = step()
    ev1.record()
    torch.cuda.synchronize(dev)
    barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    dev_ms_per_step = ev0.elapsed_time(ev1) / max(1, args.steps)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if rccl is not None else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=rccl)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(out, n_orfs, args.dump_outputs)  # (before anything after the timed region reuses the output buffers)

    # ---- --full: everything below that is not the headline -------------------------------------
    # per-kernel HIP-event timing (events recorded inside the library, on the same stream)
    k_index = k_main = k_fin = None
    if args.full:
        timings: list = []
        for _ in range(max(5, min(args.steps, 20))):
            eng.score(counts, offsets, thresholds=thresholds, algo=algo, reuse_outputs=True, plan=plan, timings=timings)
        k_index = sum(t[0] for t in timings) / len(timings)
        k_main = sum(t[1] for t in timings) / len(timings)
        k_fin = sum(t[2] for t in timings) / len(timings)
    # The 1 -> 8 GPU curve (BASELINE configs[3]) PROJECTED from the one GPU at hand: for G in {2, 4, 8}, rank 0's
    # nt-balanced slice of the SAME set (sharding.slice_bounds -- exactly what `--gpus G` gives rank 0: views of the
    # resident counts / offsets, a tile plan of its own) timed with the headline protocol.  There is no collective and
    # no shared state on the data path (detect_orfs.py:274-324: independent iterations), so G GPUs run G such steps
    # side by side: projected_value = n_set / step_ms(G), projected_efficiency = step_ms(1) / (G * step_ms(G)).  What
    # the projection cannot see is anything the ranks share on a real node (host launch threads, power); the driver's
    # --gpus N runs measure that.
    projection = None
    if args.full and world == 1 and strong and plan is not None and not args.no_slice_projection and n_orfs >= 64:
        from ribotricer_amd.engine import TilePlan

        step1_ms = 1e3 * elapsed / max(1, args.steps)
        rows = []
        n_proj = max(5, min(args.steps, 50))
        proj_tag = _lib.load().rp_measurement_tag(1)  # (under the second kernel name: a profiler's rp::k_tile_score statistics stay the headline's launches)
        for g in (2, 4, 8):
            b = slice_bounds(offsets_set, g)
            hi_g = int(b[1])
            nt_g = int(offsets_set[hi_g])
            c_g, o_g = counts[:nt_g], offsets[: hi_g + 1]
            resolved_g = ("tile" if nt_g >= (2 << 20) else "wave") if algo == "auto" else algo
            plan_g = None
            if resolved_g == "tile":
                plan_g = TilePlan(dev, o_g, nt_g, (c_g.data_ptr() // 4) % 4, ctypes_stream(torch, dev))

            def step_g():
                return eng.score(c_g, o_g, thresholds=thresholds, algo=algo, reuse_outputs=True, plan=plan_g if plan_g is not None else "auto")

            for _ in range(max(3, min(args.warmup, 10))):
                out_g = step_g()
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_proj):
                out_g = step_g()
            e1.record()
            torch.cuda.synchronize(dev)
            ms_g = e0.elapsed_time(e1) / n_proj
            tm_g: list = []
            for _ in range(5):
                eng.score(c_g, o_g, thresholds=thresholds, algo=algo, plan=plan_g if plan_g is not None else "auto", timings=tm_g)
            km, kf = sum(t[1] for t in tm_g) / len(tm_g), sum(t[2] for t in tm_g) / len(tm_g)
            bytes_g = 4 * nt_g + 8 * (hi_g + 1) + 24 * hi_g
            same = all(bool(torch.equal(getattr(out_g, k_), getattr(out, k_)[:hi_g])) for k_ in ("valid", "read_count", "min_codon_cov", "status"))
            dphase = float((out_g.phase - out.phase[:hi_g]).abs().max()) if hi_g else 0.0
            rows.append({"gpus": g, "orfs": hi_g, "nt": nt_g, "step_ms": ms_g, "kernel_ms": km, "finish_ms": kf, "steps": n_proj,
                         "kernel_frac": bytes_g / (km * 1e-3) / 1e9 / HBM_PEAK_GBS if km > 0 else None,
                         "step_frac": bytes_g / (ms_g * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "projected_value": n_job / (ms_g * 1e-3),
                         "projected_efficiency": step1_ms / (g * ms_g),
                         "integers_equal_headline": same, "max_abs_dphase_vs_headline": dphase})
            del plan_g, out_g
        _lib.load().rp_measurement_tag(proj_tag)
        projection = {"step_ms_1gpu": step1_ms, "slices": rows,
                      "what": "rank 0's nt-balanced slice of the same set for G = 2, 4, 8 (what `--gpus G` hands rank 0), timed on this one GPU "
                              "with the headline protocol; projected_value = ORFs of the whole set / step_ms(G); projected_efficiency = "
                              "step_ms(1) / (G x step_ms(G)); a projection (the ranks share nothing on the data path), not a measurement of G GPUs"}
    # A single-sample `detect-orfs` run uses its index ONCE: the plan is then part of the job.
    # Timed separately (same K-step protocol, fewer steps): the tile index, descriptors and head
    # rows rebuilt inside every step (rp_phase_score_csr_dev without a plan).
    single_ms = None
    if args.full and plan is not None:
        n_single = max(3, min(args.steps, 10))
        for _ in range(2):
            eng.score(counts, offsets, thresholds=thresholds, algo="tile", reuse_outputs=True, plan=None)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_single):
            eng.score(counts, offsets, thresholds=thresholds, algo="tile", reuse_outputs=True, plan=None)
        e1.record()
        torch.cuda.synchronize(dev)
        single_ms = e0.elapsed_time(e1) / n_single
        out = step()  # (the outputs checked below come from the planned path the headline times)
        torch.cuda.synchronize(dev)
    # Many samples against one index: the engine's MANY-SAMPLES MODE -- sample k on stream k % 2, each stream with a record
    # workspace and outputs of its own, so that the per-ORF finish pass of one sample (latency-bound, 9 % of a step) runs
    # beside the scoring kernel of the next -- WHERE THAT WINS.  Two memory-bound kernels side by side share one HBM: on
    # some boxes the overlap gains 2-5 %, on others it loses (round 4's driver box: -9 %).  So the mode times both ways on
    # the batch at hand, same K-step protocol, and runs the faster one; `value_pipelined` is what it then delivers, and the
    # block says which way it went.  Both streams' workspaces come from the ONE block the headline's placement search chose
    # (engine.tune_workspace(copies=2) / share_placed_workspace), not from searches of their own.  Same work per step as the
    # headline (every sample is scored and finished); reported BESIDE `value`, never instead of it.
    pipelined = None
    if args.full and world == 1 and plan is not None and not args.no_pipelined and total_nt >= (64 << 20):
        lanes = [torch.cuda.Stream(device=dev) for _ in range(2)]
        tag_lib = _lib.load()
        tag_was = tag_lib.rp_measurement_tag(1)  # (overlapped launches last longer: kept out of a profiler's rp::k_tile_score statistics)
        shared = eng.share_placed_workspace(lanes)  # (0 when the search did not run: the streams then allocate their own)
        for st in lanes:
            st.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(st):
                for _ in range(3):
                    step()
        torch.cuda.synchronize(dev)
        n_pipe = max(4, args.steps // 2 * 2)
        for k in range(4):
            with torch.cuda.stream(lanes[k % 2]):
                step()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0p = time.perf_counter()
        e0.record(lanes[0])
        lanes[1].wait_event(e0)
        for k in range(n_pipe):
            with torch.cuda.stream(lanes[k % 2]):
                out_p = step()
        lanes[0].wait_stream(lanes[1])
        e1.record(lanes[0])
        torch.cuda.synchronize(dev)
        wall_p = time.perf_counter() - t0p
        ms_two = e0.elapsed_time(e1) / n_pipe
        same = all(bool(torch.equal(getattr(out_p, k_), getattr(out, k_))) for k_ in ("phase", "valid", "read_count", "min_codon_cov", "status"))
        # ... and one stream, the same protocol, right after it (the box in the same state): the mode keeps the faster
        for _ in range(3):
            step()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_pipe):
            step()
        e1.record()
        torch.cuda.synchronize(dev)
        ms_one = e0.elapsed_time(e1) / n_pipe
        pipelined = {"two_streams_ms_per_step": ms_two, "one_stream_ms_per_step": ms_one, "faster": 2 if ms_two < ms_one else 1,
                     "wall_ms_per_step_two_streams": 1e3 * wall_p / n_pipe, "steps": n_pipe, "results_equal_headline": same,
                     "workspaces_from_the_headline_placement": shared,
                     "what": "many-samples mode: sample k on stream k % 2 (a record workspace and outputs per stream: finish(k) beside "
                             "score(k + 1)), and all on one stream right after it with the same protocol; both reported, neither chosen"}
        tag_lib.rp_measurement_tag(tag_was)
        for st in lanes:
            eng.release_stream(st)
        del lanes, out_p
    # SECONDARY, after the headline: the other half of the placement relation is where the COUNTS lie (a step is slow
    # whenever counts and records share a class of physical memory, profiles/archive/r05_source_placement.txt).  engine.tune_source
    # copies this program's own synthetic array behind spacers until the kernel runs at the fast class's rate (same bytes)
    # and the same K steps are timed again: value_source_placed.  No product path moves a caller's array -- which is why
    # this is not `value` -- but a caller who owns his allocation can.
    source_placed = None
    if args.full and placement is not None and not args.no_tune_source and world == 1:
        tag_lib = _lib.load()
        tag_was = tag_lib.rp_measurement_tag(1)  # (kept out of a profiler's rp::k_tile_score statistics)
        counts_first = counts
        counts, source_placement = eng.tune_source(counts, offsets, thresholds=thresholds)
        if source_placement.get("chosen"):
            for _ in range(max(3, args.warmup)):
                step()
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize(dev)
            source_placed = {"ms_per_step": e0.elapsed_time(e1) / max(1, args.steps), "steps": args.steps, "search": source_placement}
        else:
            source_placed = {"ms_per_step": None, "steps": 0, "search": source_placement}  # (the first place was already the fast one)
        del counts_first
        tag_lib.rp_measurement_tag(tag_was)
    rank_bytes = 4 * total_nt + 8 * (n_orfs + 1) + 24 * n_orfs  # SURVEY 8(d), this rank's slice
    per_rank = {"rank": rank, "device": local_dev, "orfs": n_orfs, "nt": total_nt, "step_device_ms": dev_ms_per_step,
                "algorithmic_bytes_per_launch": rank_bytes}
    if k_main is not None:
        per_rank.update(kernel_ms=k_main, finish_ms=k_fin, achieved=rank_bytes / (k_main * 1e-3) / 1e9 if k_main > 0 else 0.0,
                        frac=rank_bytes / (k_main * 1e-3) / 1e9 / HBM_PEAK_GBS if k_main > 0 else 0.0)
    ranks = [per_rank]
    if dist is not None:
        ranks = [None] * world
        dist.all_gather_object(ranks, per_rank, group=side)

    # ---- N > 1: the concatenation of the ranks' results must equal the one-GPU result ----------
    verify = None
    if args.full and dist is not None and strong and not args.no_verify:
        keys = ("phase", "valid", "read_count", "min_codon_cov", "flags", "status")
        mine = {k: getattr(out, k) for k in keys}
        if rank == 0:
            counts_all, offsets_all = synth_csr_device(n_set, seed=args.seed, cfg=args.cfg, device=dev)
            whole = eng.score(counts_all, offsets_all, thresholds=thresholds, algo=algo, plan=None)
            torch.cuda.synchronize(dev)
            verify = {"ok": True, "max_abs_dphase": 0.0, "orfs_checked": 0,
                      "read_count_checksum": int(whole.read_count.sum())}
            for r in range(world):
                a, b = int(bounds[r]), int(bounds[r + 1])
                for k in keys:
                    ref = getattr(whole, k)[a:b]
                    if r == 0:
                        got = mine[k]
                    else:
                        got = torch.empty(b - a, dtype=ref.dtype, device="cpu")
                        dist.recv(got, src=r, group=side)
                        got = got.to(dev)
                    if k == "phase":
                        d = float((got - ref).abs().max()) if b > a else 0.0
                        verify["max_abs_dphase"] = max(verify["max_abs_dphase"], d)
                        verify["ok"] &= d <= 1e-6
                    elif k == "flags":  # the split / recheck bits depend on where the tiles fall
                        verify["ok"] &= bool(torch.equal(got & 1, ref & 1))
                    else:
                        verify["ok"] &= bool(torch.equal(got, ref))
                verify["orfs_checked"] += b - a
            del counts_all, offsets_all, whole
        else:
            for k in keys:
                dist.send(mine[k].contiguous().cpu(), dst=0, group=side)
        barrier()
        if rank == 0 and not verify["ok"]:
            emit_line(json.dumps({"error": "sharded results differ from the one-GPU result", "verify": verify}))
            sys.exit(2)

    quality = None
    if args.full and rank == 0:  # (now: the fused sections below reuse the engine's output buffers)
        hf = out.flags
        quality = {
            "tie_flag_rate": float((hf & _lib.FLAG_TIE).ne(0).double().mean()) if n_orfs else 0.0,
            "recheck64_rate": float((hf & _lib.FLAG_RECHECK64).ne(0).double().mean()) if n_orfs else 0.0,
            "replay_rate": float((hf & _lib.FLAG_REPLAY).ne(0).double().mean()) if n_orfs else 0.0,
            "translating": int(out.status.sum()),
            # (the headline resolves EVERY ORF -- no RP_FILTER_PRINTED_ONLY; what the export's default mode leaves open
            # is in fused.left_open / fused_nested.left_open)
            "left_open": int((hf & _lib.FLAG_UNRESOLVED).ne(0).sum()) if n_orfs else 0,
        }
    fused = fused_nested = None
    if args.full and rank == 0 and world == 1:
        if not args.no_verify and n_orfs > 0:
            concat_check = verify  # (RP_BENCH_FORCE_DIST: the N-rank check ran with one rank)
            verify = verify_slices(out, counts, offsets, n_orfs)
            if concat_check is not None:
                verify["concat_equals_whole"] = concat_check
            verify["read_count_checksum_ok"] = bool(int(out.read_count.sum()) == int(counts.sum(dtype=torch.int64)))
            verify["ok"] = verify["ok"] and verify["read_count_checksum_ok"]
        if not args.no_fused and resolved == "tile" and n_orfs > 0:
            if not args.no_fused_exons:
                fused = fused_section(args, eng, dev, thresholds, n_set)
            if not args.no_fused_nested:
                fused_nested = fused_section(args, eng, dev, thresholds, n_set, layout="nested")
        bad = (verify is not None and not verify["ok"]) or any(f is not None and "verify" in f and not f["verify"]["ok"] for f in (fused, fused_nested))
        if bad:
            emit_line(json.dumps({"error": "results differ from the oracle", "verify": verify, "fused": fused, "fused_nested": fused_nested}))
            sys.exit(2)

    stream_read = None
    if args.full and rank == 0 and world == 1 and total_nt >= (1 << 22):
        # After the timed region: what does a plain read of the SAME counts buffer reach in this process, on this
        # box, right now?  (csrc/stream_probe.hip: 32 KiB pieces DMA'd into LDS by one loader wave, four workgroups
        # per CU -- the scoring kernel's skeleton and nothing else.)  The scoring kernel was seen between 2.6 and
        # 3.1 ms on the same bytes depending on where its buffers lie (profiles/archive/r03_clock_trace.txt); the plain
        # read is the yardstick that does not move.
        try:
            from ribotricer_amd._probe import stream_read_GBps

            gbps, ms = stream_read_GBps(counts, launches=10, flavour="lds_dma")
            stream_read = {"GBps": gbps, "ms": ms, "bytes": int(counts.numel()) * 4 // 32768 * 32768,
                           "what": "csrc/stream_probe.hip k_stream_read_lds over the counts buffer of this run, after the timed region"}
            # ... and where do this run's record workspace and counts lie relative to each other?  (the write stream
            # costs a read stream ~10 % or ~23 % depending on whether the two share a class of the physical address
            # space: profiles/archive/r03_probe_rw_regions.txt; the records are dead after the steps, the probe overwrites them)
            from ribotricer_amd._probe import write_penalty

            ws_t = next(iter(eng._workspace.values()), None)
            wps = [write_penalty(counts, ws_t, where=w) for w in (0.0, 0.5, 1.0)] if ws_t is not None else []
            if wps and all(w is not None for w in wps):
                stream_read["record_write_penalty"] = {"penalty": [w[0] for w in wps], "read_only_ms": [w[1] for w in wps],
                                                       "read_plus_writes_ms": [w[2] for w in wps],
                                                       "what": "2 GiB of the counts read (head / middle / tail of the array), 1 152 B per 32 KiB written into the head of "
                                                               "the engine's record workspace (csrc/stream_probe.hip k_stream_rw): ~0.10 = different classes of "
                                                               "physical memory, ~0.2 = the same; a 16 GB array can span two classes"}
        except ImportError:
            stream_read = None

    if rank == 0:
        nt_set = int(offsets_set[-1]) if strong else total_nt * world
        result = {
            "metric": "ORFs phase-scored/sec (whole node)",
            "value": n_job * args.steps / elapsed,
            "unit": "ORFs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(1, args.steps),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32 codon math, f64 reduction/score (int32 counts)",
            "data": "synthetic",
            "config": {
                "workload": (
                    f"{CFG_NAMES[args.cfg]}{' sharded over ' + str(world) + ' GPUs (configs[3])' if world > 1 and strong and args.cfg == 'cfg3' else ''}: "
                    f"one synthetic set of {n_job} ORFs, mean {nt_set / max(1, n_job):.0f} nt, Poisson P-site counts "
                    f"({args.cfg} length law), resident in HBM"
                ),
                "orfs_total": n_job,
                "nt_total": nt_set,
                "orfs_rank0": n_orfs,
                "nt_rank0": total_nt,
                "algo": algo,
                "plan": "tile plan built once per index, outside the steps" if plan is not None else "tile index rebuilt in every step",
                "plan_build_ms": plan_ms,
                "workspace_placement": placement if placement is not None else "first allocation (engine.tune_workspace not run)",
                "sharding": "nt-balanced contiguous ORF-index slices of one set, host-side concat, no collective on the data path"
                if strong else "independent per-GPU sets (weak scaling)",
                "physical_gpus": n_dev,
                "vbios": vbios_versions(),
                "ranks_share_gpus": world > n_dev,
                "launcher": "bench.py self_launch" if os.environ.get("RP_BENCH_SELF_LAUNCHED") == "1" else
                            ("external (torch.distributed.run)" if world > 1 else "none"),
                "control_backend": backend,
            },
            "per_rank": ranks,
        }
        if args.full:
            # N > 1: the roofline block is the SLOWEST rank's kernel (the one the max-over-ranks time follows), per launch
            # and per GPU like at N = 1; `node_achieved` = all ranks' bytes over that slowest kernel's time
            slow = max(ranks, key=lambda r: r["kernel_ms"])
            algo_bytes = slow["algorithmic_bytes_per_launch"]
            k_main, k_fin, dev_ms_per_step = slow["kernel_ms"], slow["finish_ms"], slow["step_device_ms"]
            achieved = algo_bytes / (k_main * 1e-3) / 1e9
            node_bytes = sum(r["algorithmic_bytes_per_launch"] for r in ranks)
            traffic, traffic_src, fetch_factor = (measured_traffic(args.cfg, n_orfs, resolved, args.seed) if world == 1 else (None, None, None))
            result["roofline"] = {
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic,
                "traffic_source": traffic_src,
                "fetch_factor": fetch_factor,
                "kernel": "rp::k_tile_score" if resolved == "tile" else "rp::k_wave_score",
                "rank": slow["rank"],
                "node_achieved": node_bytes / (k_main * 1e-3) / 1e9,
                "node_peak": HBM_PEAK_GBS * min(world, n_dev),
                "kernel_ms": k_main,
                "algorithmic_bytes_per_launch": algo_bytes,
                "step_device_ms": dev_ms_per_step,
                "aux_kernels_ms": {"tile_index": k_index, "orf_finish": k_fin},
                "step_achieved": algo_bytes / (dev_ms_per_step * 1e-3) / 1e9,
                "step_frac": algo_bytes / (dev_ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "stream_read": stream_read,
                "frac_of_stream_read": (achieved / stream_read["GBps"]) if stream_read else None,
            }
            result["quality"] = quality
        if first_alloc_ms is not None:
            result["value_first_allocation"] = (n_job / (first_alloc_ms * 1e-3)) if world == 1 else None
            result["first_allocation"] = {"ms_per_step": first_alloc_ms, "steps": max(3, min(args.steps, 20)),
                                          "what": "the same step before engine.tune_workspace: the record workspace where the first allocation put it (rank 0's slice)"}
        if projection is not None:
            result["slice_projection"] = projection
        if pipelined is not None:
            result["value_pipelined"] = n_job / (pipelined["two_streams_ms_per_step"] * 1e-3)  # (two streams; NOT a best-of)
            result["value_one_stream_repeat"] = n_job / (pipelined["one_stream_ms_per_step"] * 1e-3)
            result["pipelined"] = pipelined
        if source_placed is not None:
            result["value_source_placed"] = n_job / (source_placed["ms_per_step"] * 1e-3) if source_placed["ms_per_step"] else None
            result["source_placed"] = source_placed
        if single_ms is not None:
            result["value_single_sample"] = n_job / (single_ms * 1e-3) if world == 1 else None
            result["single_sample"] = {"ms_per_step": single_ms, "what": "tile index + segment descriptors + head rows rebuilt inside every step "
                                       "(an index used for ONE sample); rank 0's slice", "steps": max(3, min(args.steps, 10))}
        if verify is not None:
            result["verify"] = verify
        if fused is not None:
            result["fused"] = fused
        if fused_nested is not None:
            result["fused_nested"] = fused_nested
        if pool is not None:
            per_core = args.cpu_sample
            n_s = min(max(per_core * pool.n, 200_000), n_orfs)
            o_host = offsets[: n_s + 1].cpu().numpy()
            c_host = counts[: int(o_host[-1])].cpu().numpy()
            base, one, extra, exact = cpu_baseline(pool, c_host, o_host, per_core)
            pool.close()
            result["cpu_baseline"] = base
            result["cpu_baseline_1core"] = one
            result["cpu_closed_form_c"] = extra
            result["cpu_reference_arithmetic_cpp"] = exact
        if args.detail:
            os.makedirs(os.path.dirname(os.path.abspath(args.detail)), exist_ok=True)
            with open(args.detail, "w") as fh:
                json.dump(result, fh, indent=1)
        emit_line(json.dumps(compact_line(result)))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
        if forced_dir is not None:
            import shutil

            shutil.rmtree(forced_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
