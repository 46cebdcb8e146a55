#!/bin/bash
# ab_libs.sh LIB... -- one short bench per library ("" = the product library), top kernels
# (results under $OUT, default out/)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}
mkdir -p "$OUT"
for L in "$@"; do
  [ "$L" = prod ] && L=""
  FI_LIB_OVERRIDE=$L timeout -k 10 200 python bench.py --full --steps 8 --warmup 3 --sustain-seconds 0 --no-cpu-baseline ${BENCH_ARGS:-} > "$OUT/ab.json" 2>"$OUT/ab.err" || exit 1
  AB_JSON="$OUT/ab.json" python3 -c "
import json, os; d=json.load(open(os.environ['AB_JSON'])); k=d['kernel_ms_per_step']; sel=os.environ.get('AB_KERNELS'); print('${L:-prod}', round(d['ms_per_step'],3), {x: k[x] for x in (sel.split(',') if sel else list(k)[:7]) if x in k})"
done
