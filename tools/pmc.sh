#!/bin/bash
# usage (GPU box, repo root): bash tools/pmc.sh <tag> [bench args...]   -> profile_out/pmc_<tag>.json
# rocprofv3 --pmc passes of one bench.py command, collapsed into the stamped JSON that `bench.py --full` reads.  bench.py looks the file up
# as profiles/<round>/pmc_<tag>.json with <tag> = <workload>_f<fine>_<forward|train_<backward>>[_p<precision>] (copy it there).
# One pass per counter group (FETCH_SIZE and WRITE_SIZE do not fit one pass), each with --kernel-trace and nothing else traced; the
# program itself after `--`.  A failed pass ends the script: nothing more is started on the GPU.
tag=$1; shift
R=${GRAFT_REPO_ROOT:-$PWD}
O=$R/profile_out; mkdir -p $O/pmc
GROUPS_=("FETCH_SIZE" "WRITE_SIZE"
         "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU_MFMA_MOPS_F16"
         "GRBM_GUI_ACTIVE GRBM_COUNT")
ARGS=(--steps 5 --warmup 2 "$@")
cd /tmp && export TMPDIR=/tmp
rm -f $O/pmc/${tag}_g*
i=0
for grp in "${GROUPS_[@]}"; do
  i=$((i+1))
  timeout -k 10 ${PMC_PASS_TIMEOUT:-900} rocprofv3 --kernel-trace --pmc $grp --output-format csv -d $O/pmc -o ${tag}_g$i -- \
    python3 $R/bench.py "${ARGS[@]}" > $O/pmc/${tag}_g$i.log 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "pass $i ($grp) failed: exit $rc, see $O/pmc/${tag}_g$i.log"; exit $rc; fi
done
cd $R
python3 tools/pmc_json.py $O/pmc_${tag}.json "$tag: bench.py ${ARGS[*]}" $O/pmc/${tag}_g*_counter_collection.csv $O/pmc/${tag}_g*_kernel_trace.csv
