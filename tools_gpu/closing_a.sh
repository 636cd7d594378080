#!/bin/bash
# Closing evidence A on the final build: the GPU suite with the forward-error log (PT_KAPPA_LOG), the chain counters
# of C4 / C3 / C5's longest universes (pmc_chain.sh), the driver's command and a rocprofv3 kernel-trace summary of it,
# then C2's PMC passes (pmc.sh). TAG names the outputs under $RESULTS/.
set -u
export RESULTS=${RESULTS:-results}   # where this script leaves its logs and summaries
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $RESULTS
T=${TAG:-closing}
PT_KAPPA_LOG=$PWD/$RESULTS/${T}_kappa.jsonl timeout -k 10 600 python -u -m pytest -q --timeout 200 \
  --timeout-method thread tests -m gpu > $RESULTS/${T}_gpu_tests.txt 2>&1
rc=$?
echo "pytest rc=$rc" >> $RESULTS/${T}_gpu_tests.txt
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
python3 tools_gpu/kappa_summary.py $RESULTS/${T}_kappa.jsonl $RESULTS/${T}_parity_bound_summary.json \
  "PT_KAPPA_LOG of pytest -m gpu, final build" > $RESULTS/${T}_kappa_print.txt || exit $?
for w in c4 c3 c5; do W=$w TW=1 bash tools_gpu/pmc_chain.sh || exit $?; done
timeout -k 10 300 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $RESULTS/${T}_default.log 2>&1 || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $RESULTS/${T}_prof -o run --output-format csv -- python3 \
  bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline > $RESULTS/${T}_prof.log 2>&1 || exit $?
bash tools_gpu/pmc.sh || exit $?
