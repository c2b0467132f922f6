#!/bin/bash
# full GPU suite, the default bench (C2 with host path and index load), C4 and
# C3 benches, the C4 kernel stats, experiment libs' C2 kernel stats ($@)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
D=${CLY_OUT:?set CLY_OUT to the output directory}/r4e
mkdir -p $D
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -q -x --timeout 300 --timeout-method thread -m gpu > $D/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -5 $D/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full > $D/bench_c2.json 2> $D/bench_c2.err || exit $?
CFG=c2 bash tools/gpu/gpu_xp.sh libclyscan.so "$@" || exit $?
timeout -k 10 400 python -u bench.py --full --config c4 --no-host-path --no-cpu-baseline > $D/bench_c4.json 2> $D/bench_c4.err || exit $?
timeout -s KILL 400 rocprofv3 --kernel-trace --stats --output-format csv -d $D/c4_stats -o run -- python3 bench.py --full --config c4 --steps 3 --warmup 1 --no-host-path --no-cpu-baseline > $D/c4_stats.log 2>&1 || exit $?
timeout -k 10 400 python -u bench.py --full --config c3 --no-host-path --no-cpu-baseline > $D/bench_c3.json 2> $D/bench_c3.err || exit $?
echo done
CFG=c3 bash tools/gpu/gpu_xp.sh libclyscan.so libclyscan_head.so || exit $?
echo done2
