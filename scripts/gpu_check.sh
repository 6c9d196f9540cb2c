#!/bin/bash
# The one parameterised GPU-box runner (run from the repo root on a machine with an MI355X):
#   bash scripts/gpu_check.sh [tests|parity|bench|prof]...      (default: tests bench; outputs under $MN_OUT_DIR, default out/)
#   tests  : pytest -m gpu (whole suite)            -> out/pytest_gpu.log
#   parity : only tests/test_gpu_parity_full.py      -> out/pytest_parity.log (the test writes its own parity record)
#   bench  : smoke + bench.py --full (default workloads) -> out/bench.json, out/bench_detail.json
#   prof   : rocprofv3 --kernel-trace --stats of bench.py per workload -> out/prof_<w>/
#   (PMC traffic / MFMA-busy: bench.py --full collects them itself -- roofline.traffic, out/bench_detail.json)
cd ${GRAFT_REPO_ROOT:-$(pwd)}
export TMPDIR=/tmp PYTHONDONTWRITEBYTECODE=1
OUT=$(pwd)/${MN_OUT_DIR:-out}
mkdir -p $OUT
WL=${MN_WORKLOADS:-"c2 c1_w2a2"}
[ $# -eq 0 ] && set -- tests bench
for what in "$@"; do
  case $what in
    tests)
      timeout 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider -x > $OUT/pytest_gpu.log 2>&1
      grep -E "^E  |FAILED|ERROR|passed|failed" $OUT/pytest_gpu.log | cut -c1-400 | head -12 ;;
    parity)
      timeout 900 python -m pytest tests/test_gpu_parity_full.py -m gpu -q --tb=short -p no:cacheprovider -s > $OUT/pytest_parity.log 2>&1
      grep -E "^E  |FAILED|ERROR|passed|failed|worst" $OUT/pytest_parity.log | cut -c1-1500 | head -20 ;;
    bench)
      timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
      timeout 600 python bench.py --full --detail $OUT/bench_detail.json > $OUT/bench.json 2> $OUT/bench.err; tail -c 1500 $OUT/bench.json ;;
    prof)
      for w in $WL; do
        (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$w -o p -- python $OLDPWD/bench.py --only $w --steps 20 --warmup 5 --repeats 1 --no-pmc --no-cpu-baseline --no-kernel-timing --detail /tmp/prof_detail_$w.json > $OUT/prof_$w.log 2>&1)
        f=$(find $OUT/prof_$w -name "*kernel_stats.csv" | head -1)
        [ -n "$f" ] && python scripts/prof_summary.py $f $OUT/prof_${w}_summary.md "rocprofv3 --kernel-trace --stats: bench.py --only $w --steps 20 --warmup 5 --repeats 1 --no-pmc --no-cpu-baseline --no-kernel-timing" && head -25 $OUT/prof_${w}_summary.md
      done ;;
  esac
done
