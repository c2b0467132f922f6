#!/bin/bash
# same-box C2 kernel stats of the round-3 library and this build, then the default bench line
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
D=${CLY_OUT:?set CLY_OUT to the output directory}/cmp
mkdir -p $D
i=0
for lib in libclyscan_r3.so libclyscan.so libclyscan_r3.so libclyscan.so; do
  i=$((i + 1))
  timeout -s KILL 200 rocprofv3 --kernel-trace --stats --output-format csv -d $D/${i}_$lib -o run -- \
    python3 tools/scan_once.py c2 10 $lib > $D/${i}_$lib.log 2>&1 || exit $?
  tail -1 $D/${i}_$lib.log
done
timeout -k 10 400 python -u bench.py --full > $D/bench_c2.json 2> $D/bench_c2.err || exit $?
echo done
