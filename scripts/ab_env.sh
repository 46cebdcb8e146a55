#!/bin/bash
# ab_env.sh ROUNDS "ENV_A" "ENV_B" ... -- interleaved A/B of run-time switches on one box: each
# round runs one bench per setting ("-" = no extra environment), printing ms/step and the
# profiled pass's top kernels. Every bench under its own time limit; a failure ends the script.
# Results go under $OUT (default out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R=$1; shift
OUT=${OUT:-out}
mkdir -p "$OUT"
for r in $(seq 1 "$R"); do
  for E in "$@"; do
    [ "$E" = - ] && E=""
    env $E timeout -k 10 200 python bench.py --full --steps ${STEPS:-30} --warmup 5 --sustain-seconds 0 --no-cpu-baseline ${BENCH_ARGS:-} > "$OUT/abe.json" 2>"$OUT/abe.err" || { tail -5 "$OUT/abe.err"; exit 1; }
    AB_JSON="$OUT/abe.json" python3 -c "
import json, os; d=json.load(open(os.environ['AB_JSON'])); k=d['kernel_ms_per_step']; p=d['phase_ms']; sel=os.environ.get('AB_KERNELS')
print('r$r', '${E:-default}', round(d['ms_per_step'],3), 'bwd', round(p['backward'],3), {x: k[x] for x in (sel.split(',') if sel else list(k)[:8]) if x in k})"
  done
done
