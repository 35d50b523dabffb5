RESULTS=${RESULTS:-results}                    # where the outputs go (relative to the repository root)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p $R/$RESULTS/prof
cd $R
(timeout 300 python -m pytest tests -m gpu -q --timeout 300 2>&1 | tail -15) > $RESULTS/pytest2.log
rocprofv3 --kernel-trace --stats -d $R/$RESULTS/prof/stats -o bench -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $RESULTS/bench_prof.log 2>&1
rocprofv3 -L > $RESULTS/prof/counters_list.txt 2>&1
ls -R $RESULTS/prof | head -30
tail -3 $RESULTS/pytest2.log
