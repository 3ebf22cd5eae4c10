#!/bin/bash
# Measurements behind StTuning::side_start (profiles/side_schedule.json; reduced by tools/side_schedule_report.py). Run from the repository root on a
# machine with an MI355X, with the library built and — for `ab` and `control` — the parent's library in ab_base/base.so (tools/ab_build_base.sh).
#   bash tools/gpu_side_schedule.sh timelines        kernel trace (no counters) of a short bench run per start point and scene -> tools/timeline.py
#   bash tools/gpu_side_schedule.sh choose           this library's headline per start point (ST_SIDE_START), interleaved twice, both scenes
#   bash tools/gpu_side_schedule.sh ab STEPS NAME    parent head parent head, both scenes, the whole bench line -> $OUT_ROOT/side_ab_NAME
#   bash tools/gpu_side_schedule.sh control          parent, head at side_start 0 (the parent's schedule) and head at its default, Cornell, 300 steps, twice
# OUT_ROOT names the directory the results go to (it must be set; keep it out of git). Every GPU step has its own time limit and the script ends at the first step that fails.
set -o pipefail
WHAT=$1
R=${OUT_ROOT:?set OUT_ROOT to the directory the results go to}
line() {   # line FILE LABEL: the figures of one bench result
  python -c "
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[2], d.get('build_stamp'), {k: d[k] for k in ('ms_per_step', 'ms_per_step_moving', 'ms_per_step_geometry_moving', 'ms_per_step_with_present', 'gpu_kernel_ms_per_frame') if k in d})" "$1" "$2"
}
case "$WHAT" in
timelines)
  for scene in cornell dungeon; do for v in 0 1 2 3; do
    OUT=$R/side_timeline/${scene}_${v}; rm -rf $OUT; mkdir -p $OUT
    ST_SIDE_START=$v timeout -k 10 150 rocprofv3 --kernel-trace --output-format csv -d $OUT/trace -- python bench.py --no-cpu-baseline --no-extras --no-profile --steps 12 --warmup 6 --scene $scene > $OUT/run.log 2>&1 || { echo "FAILED $scene $v"; tail -20 $OUT/run.log; exit 1; }
    python tools/timeline.py $(find $OUT/trace -name "*_kernel_trace.csv" | head -1) --frames 6 > $OUT/timeline.txt || exit 1
    rm -rf $OUT/trace; echo "$scene side_start=$v"; tail -5 $OUT/timeline.txt
  done; done ;;
choose)
  mkdir -p $R/side_choose
  for round in 1 2; do for scene in cornell dungeon; do for v in 0 1 2 3; do
    F=$R/side_choose/${scene}_${v}_r${round}.json
    ST_SIDE_START=$v timeout -k 10 120 python bench.py --gpus 1 --no-cpu-baseline --no-extras --no-profile --steps 120 --scene $scene > $F 2> $F.err || { echo "FAILED $scene $v"; tail -20 $F.err; exit 1; }
    line $F "$scene side_start=$v round $round"
  done; done; done ;;
ab)
  STEPS=$2; D=$R/side_ab_$3; mkdir -p $D
  for round in 1 2; do for lib in parent head; do for scene in cornell dungeon; do
    F=$D/${scene}_${lib}_r${round}.json
    if [ $lib = parent ]; then export STROLLE_HIP_LIB=$PWD/ab_base/base.so; else unset STROLLE_HIP_LIB; fi
    timeout -k 10 240 python bench.py --gpus 1 --no-cpu-baseline --steps $STEPS --scene $scene > $F 2> $F.err || { echo "FAILED $scene $lib"; tail -20 $F.err; exit 1; }
    line $F "$scene $lib round $round"
  done; done; done ;;
control)
  D=$R/side_control; mkdir -p $D
  for round in 1 2; do for lib in parent head0 head; do
    F=$D/cornell_${lib}_r${round}.json
    unset STROLLE_HIP_LIB ST_SIDE_START
    if [ $lib = parent ]; then export STROLLE_HIP_LIB=$PWD/ab_base/base.so; fi
    if [ $lib = head0 ]; then export ST_SIDE_START=0; fi
    timeout -k 10 240 python bench.py --gpus 1 --no-cpu-baseline --steps 300 > $F 2> $F.err || { echo "FAILED $lib"; tail -20 $F.err; exit 1; }
    line $F "$lib round $round"
  done; done ;;
*) echo "usage: $0 timelines | choose | ab STEPS NAME | control"; exit 2 ;;
esac
