#!/bin/bash
# Full GPU check: parity tests, smoke, bench line (+ full per-leg report), rocprofv3 kernel stats of the bench command, PMC traffic.
#   usage (through gpurun): bash scripts/round_check.sh <tag> [traffic]
RESULTS=${RESULTS:-results}                    # where the outputs go (relative to the repository root)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
TAG=${1:-x}
cd $R
mkdir -p $RESULTS/$TAG
(timeout 1500 python -m pytest tests -m gpu -q --timeout 900 2>&1 | tail -25) > $RESULTS/$TAG/pytest.log
(timeout 120 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3) > $RESULTS/$TAG/smoke.log
T0=$(date +%s)
(timeout 900 python bench.py --full --legs-file $RESULTS/$TAG/bench_legs.json 2> /dev/null | tail -1) > $RESULTS/$TAG/bench_line.json
echo "default bench.py wall seconds: $(( $(date +%s) - T0 ))" > $RESULTS/$TAG/bench_time.txt
PROF="--steps 10 --warmup 2 --no-cpu-baseline --trained-epochs 0 --neumf-trained-steps 0 --legs-file /tmp/legs_prof.json"
rocprofv3 --kernel-trace --stats -d $R/$RESULTS/$TAG/prof -o bench -- python bench.py --full $PROF > $RESULTS/$TAG/bench_prof.log 2>&1
python scripts/rocpd_summary.py $RESULTS/$TAG/prof/bench_results.db "rocprofv3 --kernel-trace --stats -- python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --trained-epochs 0 --neumf-trained-steps 0 ($TAG)" > $RESULTS/$TAG/bench_kernel_stats.md 2>&1
rm -rf $RESULTS/$TAG/prof
# the headline leg alone (10M x 1M x 128): the other legs launch the same kernels on other shapes, which would blur the per-kernel averages above
rocprofv3 --kernel-trace --stats -d $R/$RESULTS/$TAG/prof -o bench -- python bench.py --full $PROF --legs bpr,metrics > $RESULTS/$TAG/bench_prof_bpr.log 2>&1
python scripts/rocpd_summary.py $RESULTS/$TAG/prof/bench_results.db "rocprofv3 --kernel-trace --stats -- python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --trained-epochs 0 --neumf-trained-steps 0 --legs bpr,metrics ($TAG; headline leg only: 10M x 1M x 128 training step + top-k block + metrics)" > $RESULTS/$TAG/bench_kernel_stats_bpr.md 2>&1
rm -rf $RESULTS/$TAG/prof
if [ "$2" = "traffic" ]; then bash scripts/collect_traffic.sh > $RESULTS/$TAG/traffic.log 2>&1; fi
tail -4 $RESULTS/$TAG/pytest.log; tail -1 $RESULTS/$TAG/smoke.log; cat $RESULTS/$TAG/bench_time.txt; wc -c $RESULTS/$TAG/bench_line.json; cut -c1-1800 $RESULTS/$TAG/bench_line.json; tail -30 $RESULTS/$TAG/traffic.log
