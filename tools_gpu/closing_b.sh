#!/bin/bash
# Closing evidence B on the final build (after closing_a.sh's pmc_c2.json and pmc_c*_chain.json are committed under
# profiles/): the driver's command with counted traffic, the C4 / C3 / C5 lines with 8-way shares and drop-in legs
# and their kernel stats, the reference experiment's scale, the N = 2 gloo rehearsal and smoke().
set -u
export RESULTS=${RESULTS:-results}   # where this script leaves its logs and summaries
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $RESULTS
T=${TAG:-closingb}
timeout -k 10 300 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $RESULTS/${T}_default.log 2>&1 || exit $?
for w in c4 c3 c5; do
  timeout -k 10 400 python3 bench.py --full --workload $w --steps 2 --warmup 1 --place-world 8 --no-cpu-baseline \
    > $RESULTS/${T}_$w.log 2>&1 || exit $?
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $RESULTS/${T}_${w}_prof -o run --output-format csv -- \
    python3 bench.py --full --workload $w --steps 2 --warmup 1 --no-cpu-baseline --no-dropin --deterministic-timing 0 \
    > $RESULTS/${T}_${w}_prof.log 2>&1 || exit $?
done
timeout -k 10 400 python3 bench.py --full --workload c3 --universes 6000 --dim 20 --valid-steps 100 --link-prediction \
  --steps 2 --warmup 1 --no-cpu-baseline --deterministic-timing 0 > $RESULTS/${T}_ref6000.log 2>&1 || exit $?
PT_BENCH_BACKEND=gloo timeout -k 10 600 python bench.py --full --gpus 2 --steps 20 --warmup 5 --no-cpu-baseline \
  > $RESULTS/${T}_dist2.log 2>&1 || exit $?
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $RESULTS/${T}_smoke.log 2>&1 \
  || exit $?
