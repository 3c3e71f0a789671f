#!/bin/bash
# bench_two_trees.sh OUT.jsonl ROUNDS NAME_A TREE_A NAME_B TREE_B [bench.py args...]
# The default bench line of two built checkouts of this repository (e.g. the parent commit and a
# change), alternating A, B, A, B, ... so that clock and thermal drift hit both alike.  Each run is
# `python bench.py --gpus 1 --steps 20 --warmup 5 ARGS` inside its tree, under its own time limit;
# one line {"tree": NAME, "line": <bench JSON>} per run is appended to OUT.jsonl, and the means are
# printed at the end.  Stops at the first run that fails.
set -u
out=$1; rounds=$2; na=$3; a=$(cd "$4" && pwd); nb=$5; b=$(cd "$6" && pwd); shift 6
mkdir -p "$(dirname "$out")"; out=$(cd "$(dirname "$out")" && pwd)/$(basename "$out"); : > "$out"
for i in $(seq "$rounds"); do
  for k in a b; do
    if [ $k = a ]; then t=$a; name=$na; else t=$b; name=$nb; fi
    line=$(cd "$t" && timeout -k 10 180 python bench.py --gpus 1 --steps 20 --warmup 5 "$@" 2>/dev/null | tail -1)
    rc=$?
    if [ $rc -ne 0 ] || [ -z "$line" ]; then echo "bench.py failed in $t (exit $rc)" >&2; exit 1; fi
    echo "{\"tree\": \"$name\", \"line\": $line}" >> "$out"
  done
done
python - "$out" <<'PY'
import json, statistics, sys
v = {}
for l in open(sys.argv[1]):
    j = json.loads(l)
    v.setdefault(j["tree"], []).append(j["line"]["value"])
for t, x in v.items():
    print(t, x, "mean", round(statistics.mean(x), 2), "min", min(x), "max", max(x))
PY
