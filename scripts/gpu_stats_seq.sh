#!/bin/bash
# rocprofv3 kernel stats of the headline workload with every launch sequential on one stream (NNN_SCHED=seq, no one-frame calls):
# the per-launch durations bench.py's roofline pass measures with HIP events (its launches are sequential too), for comparison
# with the pipelined run's stats, where overlapping kernels share the machine and each takes longer.
set -u
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/out}
mkdir -p $OUT; rm -rf $OUT/prof_seq
cd /tmp && export TMPDIR=/tmp
NNN_SCHED=seq timeout 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_seq" -- python "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline --no-also --no-tick > "$OUT/prof_seq.log" 2>&1; echo "rocprof rc=$?"
cd "$R"
DB=$(find $OUT/prof_seq -name '*_results.db' | head -1)
python scripts/rocpd_kernel_stats.py "$DB" > $OUT/kernel_stats_seq.md; head -8 $OUT/kernel_stats_seq.md
grep -o '"avg_kernel_us": [0-9.]*' $OUT/prof_seq.log | head -2
find $OUT/prof_seq -name '*.db' -delete
