#!/bin/bash
# default bench (C2, eager) per library build: value, ms/step and the per-kernel breakdown
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
export OUT=${OUT:-bench_out}  # where this script writes its logs and results
mkdir -p $OUT
for v in ${VARIANTS}; do
  DPZ_CODEC_LIB=$PWD/decentralizepy_amd/libdpz_v_$v.so timeout -k 10 200 python bench.py --full --no-cpu ${BENCH_ARGS} > $OUT/bv_$v.log 2>&1 || { tail -3 $OUT/bv_$v.log; exit 1; }
  python3 - "$v" <<'PY'
import json, os, sys
l = [x for x in open(os.environ["OUT"] + f"/bv_{sys.argv[1]}.log") if x.startswith("{")][-1]
d = json.loads(l)
sec = d.get("secondary") or {}
print(sys.argv[1], d["value"], d["ms_per_step"], sec.get("value"), {k: v["avg_us"] for k, v in d["stages"]["kernels"].items()})
PY
done
