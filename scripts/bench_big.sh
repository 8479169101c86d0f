#!/bin/bash
# Full-size cfg3 / cfg5 bench lines (run on the GPU box) -> <out dir>/bench_<cfg>.json.  usage: bash scripts/bench_big.sh [out dir]
cd ${GRAFT_REPO_ROOT:-.}
OUT=${1:-${TMPDIR:-/tmp}/bench_big}
mkdir -p $OUT
timeout 900 python bench.py --full --cfg cfg3 --orfs 11000000 --steps 10 --warmup 2 --cpu-sample 0 > $OUT/bench_cfg3.json 2>$OUT/bench_cfg3.err
timeout 900 python bench.py --full --cfg cfg5 --orfs 20000000 --steps 5 --warmup 1 --cpu-sample 0 > $OUT/bench_cfg5.json 2>$OUT/bench_cfg5.err
python - "$OUT" <<'PY'
import json, sys
out = sys.argv[1]
for c in ("cfg3","cfg5"):
    try:
        d=json.load(open(f"{out}/bench_{c}.json")); r=d["roofline"]
        print(c, "step_ms=%.4f kernel_ms=%.4f frac=%.3f value=%.3e"%(d["ms_per_step"], r["kernel_ms"], r["frac"], d["value"]), r["aux_kernels_ms"])
    except Exception as e:
        print(c, "failed", e, open(f"{out}/bench_{c}.err").read()[-500:])
PY
