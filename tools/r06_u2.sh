#!/bin/bash
# usage (GPU box): bash tools/r06_u2.sh OUTDIR — the whole -m gpu suite and the default bench line with the current library (a mid-session check)
R=$GRAFT_REPO_ROOT
OUT=$(realpath -m "${1:?usage: bash tools/r06_u2.sh OUTDIR}")
cd $R
mkdir -p "$OUT"
timeout 2400 python -m pytest tests -m gpu -q -n 2 -p no:cacheprovider 2>&1 | tail -8 > "$OUT/pytest_gpu.log"; tail -3 "$OUT/pytest_gpu.log"
timeout 900 python bench.py --full > "$OUT/bench_default_N1.json.log" 2> "$OUT/bench_default_N1.err"; tail -c 300 "$OUT/bench_default_N1.err"
python - "$OUT" <<'P'
import json, sys
d=json.loads(open(sys.argv[1] + '/bench_default_N1.json.log').read().strip().splitlines()[-1])
print({k:d[k] for k in ('value','ms_per_step')}, 'gang p50', d['gang_admit_latency_ms_p50'], 'seq', d['drain']['sequential_on_device']['total_ms_device'], d['drain']['sequential_on_device']['gang_admit_latency_ms_p50'], d['drain']['sequential_on_device']['bit_identical_to_cpu_pass'])
P
