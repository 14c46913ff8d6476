#!/bin/bash
# Run on the GPU box: hardware counters of ONE double three-array gather stiffness instance at config C2, every counter
# group in a rocprofv3 --pmc run of its own (three launches each).
# usage: tools/stiffness_lines_counters.sh <out dir> old|new|parent|lean [pass names: lds valu waits fetch write]
# old / new: the slab and the streamed line instance (tools/stiffness_lines_ab.py); parent / lean: the shared line instance
# and its lean form on one repeated factor block (tools/lean_line_ab.py).
# FETCH_SIZE and WRITE_SIZE do not fit into one pass on gfx950 (rocprofv3 refuses the pair), so each has its own.
# Any pass that does not end with status 0 ends the script: nothing more starts on the GPU after a failure.  Leave a pass
# whose counters this rocprofv3 refuses out of the next call by naming the others.
out=$1; which=$2; shift 2
passes=${*:-lds valu waits fetch write}
want() { case " $passes " in *" $1 "*) return 0;; esac; return 1; }
root=$(pwd)
tool=stiffness_lines_ab.py
case "$which" in parent|lean) tool=lean_line_ab.py;; esac
mkdir -p "$out"
pass() {
    name=$1; shift
    dir=$(mktemp -d /tmp/pmc_XXXXXX)
    (cd /tmp && TMPDIR=/tmp timeout -k 10 240 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d "$dir" -o run -- python3 "$root/tools/$tool" --counters "$which") > "$out/${which}_$name.run.log" 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then echo "pass $name ($*) ended with status $rc: stopping" | tee -a "$out/${which}_counters.txt"; rm -rf "$dir"; exit $rc; fi
    python3 - "$dir" "$name" "$*" >> "$out/${which}_counters.txt" <<'PY'
import collections, csv, glob, sys
d, name, counters = sys.argv[1:4]
agg = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.Counter()
for path in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(path)):
        k = row["Kernel_Name"]
        if "stiffness" not in k: continue
        k = k.replace("void (anonymous namespace)::", "").split("(")[0][:90]
        agg[k][row["Counter_Name"]] += float(row["Counter_Value"]); cnt[(k, row["Counter_Name"])] += 1
print("## pass %s (%s)" % (name, counters))
for k in agg:
    print(k)
    for c, v in agg[k].items():
        print("   %-26s %.6g per launch (%d launches)" % (c, v / cnt[(k, c)], cnt[(k, c)]))
PY
    rm -rf "$dir"
}
want lds && pass lds SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT
want valu && pass valu SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES
want waits && pass waits SQ_WAIT_INST_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VMEM SQ_INSTS_VMEM SQ_WAVE_CYCLES
want fetch && pass fetch FETCH_SIZE
want write && pass write WRITE_SIZE
cat "$out/${which}_counters.txt"
