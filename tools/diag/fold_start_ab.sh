#!/bin/bash
# DPZ_WALK_GUESS was removed after the A/B (profiles/r05_fold_start_ab.txt): build lib_guess from
# commit ff7398b (tools/diag/build_variant.sh guess "-DDPZ_WALK_GUESS=1" ff7398b) to re-run it.
# DPZ_WALK4_LOCKSTEP / DPZ_WALK4_L_FIRST (and the groups kernel's DPZ_WALKG_* twins) were removed
# after their A/B too (profiles/r04_c4_round_ab.jsonl): build lib_ls / lib_lf / lib_lslf from commit
# 1ca54c3 (tools/diag/build_variant.sh ls "-DDPZ_WALK4_LOCKSTEP=1" 1ca54c3, ...).
# The lone walk fold's start-up switches (DPZ_WALK4_LOCKSTEP / DPZ_WALK4_L_FIRST / DPZ_WALK_GUESS,
# build_variant.sh libraries base / ls / lf / lslf / guess): the fold parity tests on the guess
# library, then the bench's product-path stage (64 MiB, 1 and 3 payloads), alternating on one box.
# Outputs in $OUT/.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
OUT=${OUT:-bench_out}  # where this script writes its logs and results
mkdir -p $OUT
DPZ_CODEC_LIB=$PWD/tools/diag/variants/lib_guess.so timeout -k 10 400 python -u -m pytest -x -q --timeout 120 --timeout-method thread -p no:cacheprovider -m gpu \
  tests/test_gpu_codec.py tests/test_gpu_fold_batch.py tests/test_gpu_foldbase.py tests/test_gpu_gossip.py tests/test_gpu_batch.py \
  > $OUT/fsab_tests.log 2>&1 || { echo "guess tests failed"; tail -30 $OUT/fsab_tests.log; exit 1; }
tail -1 $OUT/fsab_tests.log
for r in 1 2; do for v in base guess ls lf lslf; do
  DPZ_CODEC_LIB=$PWD/tools/diag/variants/lib_$v.so timeout -k 10 300 python bench.py --full --no-cpu --no-extra > $OUT/fsab_${v}_$r.json 2> $OUT/fsab.err || { echo "$v rc=$?"; tail -3 $OUT/fsab.err; exit 1; }
  python -c "
import json; d=json.load(open('$OUT/fsab_${v}_$r.json')); p=d['stages']['product_one_node']
print('$v $r', {k: (p[k]['step_us'], p[k]['fold_us']) for k in p if isinstance(p[k], dict) and 'fold_us' in p[k]})"
done; done
