#!/bin/bash
# A/B of GEMM configuration overrides inside the bench step: tools/ab_override.sh "label:M,N,K,al,bl,cfg,split[ ...]" ...
# ("label:" alone = the built-in table); two interleaved rounds.  The log goes to $ERGM_OUT (default bench_out).
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${ERGM_OUT:-bench_out}; mkdir -p $OUT
for rep in $(seq 1 ${ROUNDS:-2}); do
  for v in "$@"; do
    l=${v%%:*}; o=${v#*:}
    if [ -z "$o" ]; then
      timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-gpu-only > $OUT/ov.log 2>&1 || { tail -5 $OUT/ov.log; exit 1; }
    else
      timeout -k 10 300 python tools/bench_override.py $o -- --full --no-cpu-baseline --no-gpu-only > $OUT/ov.log 2>&1 || { tail -5 $OUT/ov.log; exit 1; }
    fi
    python -c "import json,sys; r=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[2], r['value'], r['ms_per_step'])" $OUT/ov.log $l
  done
done
