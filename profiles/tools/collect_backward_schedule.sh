#!/bin/bash
# What DESIGN.md section 6.BS quotes, in one GPU-box call (run from the repo root of the built change):
#   bash profiles/tools/collect_backward_schedule.sh PARENT_TREE [OUTDIR] [PART]
# PARENT_TREE: a built checkout of the parent commit (its own cbf-ssm_amd/lib/libcbfssm_hip.so).  PART: bench | prof | all.
#   bench: five alternating `bench.py --gpus 1 --steps 200 --warmup 20` lines per tree, then --dump-outputs of the first step
#          and after 25 updates in both trees and their comparison (output_differences.txt)
#   prof:  rocprofv3 --kernel-trace --stats per tree with CBFSSM_NO_SPLIT=1 (kernel times on one stream) and with the
#          default split (step timeline: when each queue goes idle before the reductions)
# Every GPU step has its own time limit and the first failure ends the script.
set -o pipefail
P=$(cd "${1:?parent tree}" && pwd); R=$(pwd); O=$R/${2:-bench_out/backward_schedule}; PART=${3:-all}
mkdir -p $O
run() { # tree tag bench-args...
  local tree=$1 tag=$2; shift 2
  (cd $tree && timeout -k 10 240 python3 bench.py "$@" > $O/$tag.json 2> $O/$tag.err) || { echo FAILED $tag; tail -5 $O/$tag.err; exit 1; }
  echo "$tag $(grep -o '"ms_per_step": *[0-9.]*' $O/$tag.json | head -1)"
}
prof() { # tree tag env...
  local tree=$1 tag=$2; shift 2
  (cd $tree && env CBFSSM_HIP_GRAPH=0 "$@" timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_$tag -o c3 -- python3 bench.py --gpus 1 --steps 8 --warmup 2 > $O/bench_under_rocprof_$tag.json 2> $O/kt_$tag.log) || { echo FAILED $tag; tail -5 $O/kt_$tag.log; exit 1; }
  cp $(find $O/kt_$tag -name "*kernel_stats.csv" | head -1) $O/train_C3_kernel_stats_$tag.csv
  grep -E "rev_kernel|pass_kernel" $O/train_C3_kernel_stats_$tag.csv | cut -c1-200 | head -8
}
if [ "$PART" != "prof" ]; then
  for i in 1 2 3 4 5; do
    run $P bench_train_C3_parent_$i --gpus 1 --steps 200 --warmup 20
    run $R bench_train_C3_change_$i --gpus 1 --steps 200 --warmup 20
  done
  run $P first_step_parent --gpus 1 --steps 1 --warmup 0 --dump-outputs $O/dump_parent
  run $R first_step_change --gpus 1 --steps 1 --warmup 0 --dump-outputs $O/dump_change
  run $P steps25_parent --gpus 1 --steps 20 --warmup 5 --dump-outputs $O/dump25_parent
  run $R steps25_change --gpus 1 --steps 20 --warmup 5 --dump-outputs $O/dump25_change
  python3 - $O > $O/output_differences.txt <<'PY'
import glob, os, sys
import numpy as np
O = sys.argv[1]
for a, b, title in (('dump_parent', 'dump_change', 'first step (--steps 1 --warmup 0)'),
                    ('dump25_parent', 'dump25_change', 'after 25 updates (--steps 20 --warmup 5)')):
    print(title + ', parent against change')
    for f in sorted(glob.glob(os.path.join(O, a, '*.npy'))):
        n = os.path.basename(f)
        x, y = np.load(f), np.load(os.path.join(O, b, n))
        same = x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
        d = float(np.abs(x - y).max()) if x.shape == y.shape and x.size else float('nan')
        print('  %-28s %-14s %s  max|diff| %.3e  max|parent| %.3e' % (n, x.shape, 'bitwise equal' if same else 'differs', d,
                                                                     float(np.abs(x).max()) if x.size else 0.0))
PY
  cat $O/output_differences.txt
fi
if [ "$PART" != "bench" ]; then
  export TMPDIR=/tmp
  prof $P nosplit_parent CBFSSM_NO_SPLIT=1
  prof $R nosplit_change CBFSSM_NO_SPLIT=1
  prof $P split_parent
  prof $R split_change
  for t in parent change; do
    python3 $R/profiles/tools/step_timeline.py $(find $O/kt_split_$t -name "*kernel_trace.csv" | head -1) 4 > $O/train_C3_step_timeline_$t.txt
  done
  find $O -name "*kernel_trace.csv" -delete
fi
ls $O
