#!/bin/bash
# Everything profiles/<round>_* holds, in one GPU call: scripts/profile_bench.sh (bench line, rocprofv3 stats, PMC passes, phase
# times, kernel table) + every config + the probes.  Run on the GPU box from the repo root; outputs land in $OUT (default out/).
cd "$(dirname "$0")/.."
R="$(pwd)"
mkdir -p "${OUT:=$R/out}" && OUT="$(cd "$OUT" && pwd)" && export OUT
bash scripts/profile_bench.sh > "$OUT"/profile_bench.log 2>&1
( bash scripts/all_configs.sh; python scripts/env_batched_step.py --envs 1 32 64 ) > "$OUT"/all_configs.log 2>&1
for p in valu_probe rbody_probe xcd_chain_probe; do timeout 120 ./scripts/probe/$p > "$OUT"/$p.log 2>&1; done
LAB_STAGES=1 timeout 300 ./scripts/probe/rollout_lab 8192 32768 65536 131072 1048576 > "$OUT"/rollout_lab.log 2>&1
timeout 60 ./scripts/probe/pipe_timeline > "$OUT"/pipe_timeline.log 2>&1
tail -3 "$OUT"/all_configs.log; grep -c . "$OUT"/rollout_lab.log "$OUT"/valu_probe.log
