# Full GPU check: build (no-op when fresh), every -m gpu test, smoke(), the bench line with every sub-line.
# Logs and the line go to $OUT (default bench_out/).
set -e
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.build()"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > "$OUT/tests.log" 2>&1 || { tail -40 "$OUT/tests.log"; exit 1; }
tail -2 "$OUT/tests.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tail -2
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
cat "$OUT/bench.json"
