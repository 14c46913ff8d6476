#!/bin/bash
# the round's closing measurements on one box: default bench, 2- and 4-rank rehearsals (through gpurun)
out=${OUT_DIR:-$(mktemp -d)}  # where the bench lines are kept
mkdir -p "$out"
python bench.py --full > "$out/r03_bench_c2.json" 2> "$out/r03_bench_c2.err"; echo "rc=$?"
timeout -k 10 300 python bench.py --full --rehearse-ranks 2 --steps 5 --warmup 1 > "$out/r03_bench_2rank_rehearsal.json" 2> "$out/r03_bench_2rank_rehearsal.err"; echo "rc=$?"
timeout -k 10 500 python bench.py --full --rehearse-ranks 4 --steps 5 --warmup 1 > "$out/r03_bench_4rank_rehearsal.json" 2> "$out/r03_bench_4rank_rehearsal.err"; echo "rc=$?"
python3 - "$out" <<'PY'
import json, os, sys
for f in ("c2", "2rank_rehearsal", "4rank_rehearsal"):
    r = json.load(open(os.path.join(sys.argv[1], "r03_bench_%s.json" % f))); rd = r["reference_default"]
    print(f, r["ms_per_step"], rd["f64"]["ms_per_step"], rd["f64"]["to_1e-7"]["iterations"], rd["f64"]["to_1e-7"]["time_ms"], rd["f32"]["to_1e-7"]["iterations"], r["cpu_baseline"]["cores"], r["cpu_baseline"]["value"])
PY
