#!/bin/bash
# usage (on the GPU box, from the repo root): bash tools/prof_train.sh <tag> [bench args...]
tag=$1; shift
R=${GRAFT_REPO_ROOT:-$PWD}
O=$R/profile_out/c
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o $tag -- python3 $R/bench.py --full --no-cpu-baseline --no-frame --steps 10 "$@" > $O/$tag.json 2> $O/$tag.err
cd $R
cut -c1-260 $O/$tag.json
python3 tools/kstats.py $O/prof/${tag}_kernel_stats.csv 12
