# Check on an MI355X: parity suite, smoke, one bench line with every leg (each step
# time-limited, chained with && so a failing step stops the run).  Logs go to $OUT_DIR.
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${1:-r02}
O=${OUT_DIR:-$TMPDIR/pathfeas_check}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > $O/gpu_tests_$TAG.log 2>&1 && \
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 && \
timeout -k 10 400 python bench.py --full --steps 5 --warmup 2 --cpu-sample-s 10 > $O/bench_$TAG.log 2>&1
RC=$?
echo "CHAIN EXIT $RC"
tail -3 $O/gpu_tests_$TAG.log; tail -2 $O/smoke_$TAG.log; tail -c 3000 $O/bench_$TAG.log
exit $RC
