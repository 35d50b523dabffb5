#!/bin/bash
# rocprofv3 kernel stats of the default bench command -> $RESULTS/$1/prof (summarise with scripts/rocpd_summary.py)
RESULTS=${RESULTS:-results}                    # where the outputs go (relative to the repository root)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
TAG=${1:-p}
cd $R
mkdir -p $RESULTS/$TAG
rocprofv3 --kernel-trace --stats -d $R/$RESULTS/$TAG/prof -o bench -- python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $RESULTS/$TAG/bench_prof.log 2>&1
python scripts/rocpd_summary.py $RESULTS/$TAG/prof/bench_results.db | head -24 | cut -c1-150
