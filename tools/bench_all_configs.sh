#!/bin/bash
# One JSON line per BASELINE config on one MI355X -> OUT_DIR/r02_bench_all_configs.jsonl (copy into profiles/).
# usage: tools/bench_all_configs.sh OUT_DIR
OUT=${1:?usage: tools/bench_all_configs.sh OUT_DIR}
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
mkdir -p "$OUT"
: > "$OUT/r02_bench_all_configs.jsonl"
for c in fom pod_galerkin pod_lspg quadratic ann decoder_bf16; do
  python bench.py --config $c --full 2>"$OUT/bench_$c.err" | tail -1 >> "$OUT/r02_bench_all_configs.jsonl" || exit 1
done
python - "$OUT/r02_bench_all_configs.jsonl" <<'PY'
import json, sys
for l in open(sys.argv[1]):
    d = json.loads(l)
    print("%-14s %.4g %s  frac %.3f  parity %.2e" % (d["config"]["workload"][:14], d["value"], d["unit"], d["roofline"]["frac"], d.get("rel_l2_vs_cpu_ref", float("nan"))))
PY
