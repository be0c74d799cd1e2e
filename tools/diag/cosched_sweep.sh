#!/bin/bash
# bench (C2 + 64 MiB) per co-scheduling split of the decode over sample/select/resolve/compact
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
export OUT=${OUT:-bench_out}  # where this script writes its logs and results
mkdir -p $OUT
for sh in ${SHARES:-0.2,0.3,0.35,0.15}; do
  DPZ_COSCHED=$sh timeout -k 10 200 python bench.py --full --no-cpu ${BENCH_ARGS} > $OUT/cs.log 2>&1 || { tail -3 $OUT/cs.log; exit 1; }
  python3 - "$sh" <<'PY'
import json, os, sys
d = json.loads([x for x in open(os.environ["OUT"] + "/cs.log") if x.startswith("{")][-1])
e, s = d.get("secondary") or {}, d["stages"]
print(sys.argv[1], "C2", d["value"], d["ms_per_step"], "serial", s["one_node_serial_ms_per_step"], "host", s["host_enqueue_ms_per_step"],
      "| 64MiB", e.get("value"), e.get("ms_per_step"), "serial", e.get("one_node_serial_ms_per_step"), e.get("fell_back"))
print("   ", {k: round(v["avg_us"], 1) for k, v in s["kernels"].items()})
PY
done
