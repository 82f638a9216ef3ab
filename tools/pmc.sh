#!/bin/bash
# usage (GPU box, repo root): bash tools/pmc.sh <tag> [bench args...]   -> profile_out/c/<tag>_pmc.json
# Separate passes per counter group (FETCH_SIZE and WRITE_SIZE do not fit one pass); --pmc only with --kernel-trace.
tag=$1; shift
R=${GRAFT_REPO_ROOT:-$PWD}
O=$R/profile_out/c
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/pmc -o ${tag}_$c -- python3 $R/bench.py --full --no-cpu-baseline --no-frame --steps 5 --warmup 2 "$@" > /dev/null 2>&1
done
cd $R
python3 tools/pmc_summary.py $O/${tag}_pmc.json "rocprofv3 --kernel-trace --pmc <counter>, one counter per pass; bench.py --full --steps 5 --warmup 2 $*; FETCH_SIZE/WRITE_SIZE in KiB as reported" $O/pmc/${tag}_FETCH_SIZE_counter_collection.csv $O/pmc/${tag}_WRITE_SIZE_counter_collection.csv
