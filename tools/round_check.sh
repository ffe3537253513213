#!/bin/bash
# Round-end rehearsal on one GPU box: the full -m gpu suite, smoke(), and the default bench line with everything
# bench.py measures (--full: the CPU baseline too). OUT: where the logs go (default ./out).
set -euo pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-out}
mkdir -p "$OUT"
timeout -k 10 900 python3 -u -m pytest tests/ -m gpu -x -v --timeout 300 --timeout-method thread --durations=15 > "$OUT/rc_tests.log" 2>&1
echo "tests ok"
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/rc_smoke.log" 2>&1
echo "smoke ok"
timeout -k 10 400 python3 bench.py --full > "$OUT/rc_bench.json" 2> "$OUT/rc_bench.err"
cat "$OUT/rc_bench.json"
