#!/bin/bash
# usage (GPU box, repo root): bash tools/prof_step.sh <tag> <marker kernel> [bench args...]
#   -> profile_out/<tag>_kernel_stats.csv, <tag>_kstats.txt (top kernels), <tag>_timeline.txt (one step: every kernel between two
#      occurrences of the marker kernel, e.g. rng_forward), <tag>.json (the bench line)
# rocprofv3 --kernel-trace --stats of one bench.py command, the program itself after `--`.
tag=$1; marker=$2; shift; shift
R=${GRAFT_REPO_ROOT:-$PWD}
O=$R/profile_out; mkdir -p $O/prof
cd /tmp && export TMPDIR=/tmp
timeout -k 10 ${PROF_TIMEOUT:-900} rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o $tag -- \
  python3 $R/bench.py --steps 10 "$@" > $O/$tag.json 2> $O/$tag.err || { rc=$?; echo "profiled run failed: exit $rc, see $O/$tag.err"; exit $rc; }
cd $R
cp $O/prof/${tag}_kernel_stats.csv $O/${tag}_kernel_stats.csv
python3 tools/timeline.py $O/prof/${tag}_kernel_trace.csv "$marker" > $O/${tag}_timeline.txt
python3 tools/kstats.py $O/${tag}_kernel_stats.csv 20 > $O/${tag}_kstats.txt
