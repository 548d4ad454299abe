#!/bin/bash
# A/B of the line search's record order and load width (profiles/linesearch_record_order_ab.txt): builds of the library made with scripts/build_variant.sh,
# selected with CVO_HIP_LIB, alternated on one device (first, second, ..., first, second, ...), profiler off.
# usage: gpu_linesearch_order_ab.sh REPS lib.so lib.so ...      (the first is the parent's build)
# Per repetition and build: `python bench.py` and `python bench.py --steps 20 --warmup 5`; then once per build the config-5 shape and the phase timers
# (CVO_BENCH_PHASES: us per iteration of workgroup 0 of every pair of the last launch).  Stops at the first run that does not end with a result line.
REPS=$1; shift
LIBS=("$@")
value() { python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(round(d['value'],1))"; }
run() {   # run <lib> <label> <bench arguments...>
  local lib=$1 label=$2; shift 2
  local v; v=$(CVO_HIP_LIB=$PWD/$lib timeout -k 10 300 python bench.py "$@" 2>/dev/null | value) || { echo "$label $(basename $lib): FAILED (rc $?)"; exit 1; }
  echo "$label $(basename $lib): $v"
}
for rep in $(seq 1 $REPS); do
  for lib in "${LIBS[@]}"; do run $lib "rep $rep default (256 steps, 32 warm-up)"; done
  for lib in "${LIBS[@]}"; do run $lib "rep $rep --steps 20 --warmup 5" --steps 20 --warmup 5; done
done
for lib in "${LIBS[@]}"; do run $lib "--shape eth3d" --shape eth3d; done
for lib in "${LIBS[@]}"; do
  out=$(CVO_BENCH_PHASES=1 CVO_HIP_LIB=$PWD/$lib timeout -k 10 300 python bench.py 2>&1 >/dev/null | grep -o "phase us.*" | cut -c1-330) || { echo "phases $(basename $lib): FAILED"; exit 1; }
  echo "phases $(basename $lib): $out"
done
