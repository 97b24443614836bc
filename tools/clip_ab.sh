#!/bin/bash
# usage (on a machine with the GPU): tools/clip_ab.sh PARENT_TREE [reps] [optimizer] > ab_clip_<optimizer>.txt: the config-2 training step
# (tools/bench_clip.py step) under three arms, alternating fresh processes on one box: the parent commit's checkout PARENT_TREE (built, with
# its own library), this tree with --clip_grad_norm off, this tree with it on (1e30: measures and guards, never clips). The spread of the
# parent arm's runs is the noise the other two are read against. Then the norm pass alone (bench_clip.py norm). Stops at the first failing
# run. The record goes to standard output: keep it under profiles/rNN/.
REPO=$(cd "$(dirname "$0")/.." && pwd)
PARENT=$1; REPS=${2:-4}; OPT=${3:-momentum}
for rep in $(seq 1 $REPS); do
  timeout -k 10 120 python3 $REPO/tools/bench_clip.py step --tree $PARENT --clip 0 --optimizer $OPT || exit 1
  timeout -k 10 120 python3 $REPO/tools/bench_clip.py step --clip 0 --optimizer $OPT || exit 1
  timeout -k 10 120 python3 $REPO/tools/bench_clip.py step --clip 1e30 --optimizer $OPT || exit 1
done
timeout -k 10 120 python3 $REPO/tools/bench_clip.py norm --optimizer $OPT || exit 1
