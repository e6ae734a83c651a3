#!/bin/bash
# One GPU-box visit: parity tests, smoke, bench (--full), rocprof kernel trace.  Logs under $LOGDIR (default: logs/).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
O=$(realpath -m "${LOGDIR:-logs}")
mkdir -p "$O"
export TMPDIR=/tmp
echo "== build" && python -c "import __graft_entry__ as g; g.build()" 2>&1 | tail -3
echo "== pytest -m gpu"
timeout -k 10 900 python -m pytest tests -m gpu -q ${XFLAG--x} --timeout=600 -p no:cacheprovider ${PYTEST_ARGS:-} > "$O/pytest_gpu.log" 2>&1
rc=$?; tail -n ${TAILN:-40} "$O/pytest_gpu.log"; echo "pytest rc=$rc"
[ $rc -ne 0 ] && [ -z "$KEEP_GOING" ] && exit $rc
echo "== smoke"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1; rc=$?; tail -5 "$O/smoke.log"
[ $rc -ne 0 ] && [ -z "$KEEP_GOING" ] && exit $rc
echo "== bench"
timeout -k 10 600 python bench.py --full --steps ${STEPS:-20} --warmup 6 > "$O/bench.json" 2> "$O/bench.log"; rc=$?
tail -25 "$O/bench.log"; cat "$O/bench.json"
[ $rc -ne 0 ] && exit $rc
if [ -n "$PROFILE" ]; then
  echo "== rocprofv3"
  cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -- python3 "$R/bench.py" --full --prime 0 --steps 10 --warmup 6 --no-cpu-baseline > "$O/prof_bench.json" 2> "$O/prof_bench.log"
  echo "rocprof rc=$?"; cd "$R"; find "$O/prof" -name "*stats*" | head
fi
