#!/bin/bash
# Copy what scripts/profile_round.sh left in $OUT (default out/) into profiles/<round>_* (run locally afterwards).
R=${1:-r02}
cd "$(dirname "$0")/.."
OUT="${OUT:-out}"
python3 scripts/pmc_summary.py "$OUT" $R > /dev/null
cp "$OUT"/bench_line.json profiles/${R}_bench_line.json
cp "$OUT"/bench_line_under_rocprof.json profiles/${R}_bench_line_under_rocprof.json
cp "$OUT"/prof_stats/bench_kernel_stats.csv profiles/${R}_bench_kernel_stats.csv
cp "$OUT"/phase_times.log profiles/${R}_phase_times.log
cp "$OUT"/kbench.log profiles/${R}_kbench.log
grep -v "amdgpu.ids" "$OUT"/all_configs.log > profiles/${R}_all_configs.log
for p in valu_probe rbody_probe xcd_chain_probe rollout_lab pipe_timeline; do cp "$OUT"/$p.log profiles/${R}_$p.log; done
ls -la profiles/${R}_*
