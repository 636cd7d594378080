#!/bin/bash
# default bench line + rocprofv3 kernel stats of the same kind of run
set -u
export RESULTS=${RESULTS:-results}   # where this script leaves its logs and summaries
mkdir -p $RESULTS
timeout -k 10 400 python bench.py --full --no-c3 --no-cpu-baseline > $RESULTS/bench.log 2>&1 || exit $?
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $RESULTS/prof -o run --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-c3 > $RESULTS/prof.log 2>&1 || exit $?
