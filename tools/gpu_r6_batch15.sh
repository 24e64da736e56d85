#!/bin/bash
# Round 6, batch 15: the channel-major combine over 16-row blocks (256 blocks at CA1 shape S); the
# attention suite and shape-S tests, then the stress line with LDM_FLASH_SPLIT=0 / 1
# twice around and a kernel summary of the default.   bash tools/gpu_r6_batch15.sh <tag>
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
T=${1:-r6b15}; OUT=gpurun_out/$T; mkdir -p $OUT
export PYTHONUNBUFFERED=1
timeout -k 10 400 python -u -m pytest tests/test_gpu_attention_wide.py tests/test_gpu_shape_s.py -q -x \
    --timeout 300 --timeout-method thread > $OUT/tests.log 2>&1
rc=$?; tail -2 $OUT/tests.log
if [ $rc -ne 0 ]; then grep -E "^FAILED|^ERROR|Error|assert" $OUT/tests.log | head -20; echo "tests exited $rc: stopping"; exit $rc; fi
for r in 1 2; do
  for m in 0 1; do
    LDM_FLASH_SPLIT=$m timeout -k 10 240 python -u bench.py --full --workload stress --steps 3 --warmup 1 --no-cpu-baseline \
        > $OUT/stress_${r}_$m.json 2> $OUT/stress.err || { tail -20 $OUT/stress.err; exit 1; }
    python -c "import json; d=json.load(open('$OUT/stress_${r}_$m.json')); print('round $r flash_split=$m', d['us_per_denoise_iteration'], 'us/iter', d['roofline']['avg_launch_us'])"
  done
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/$OUT/prof_stress -o run -- \
    python3 $GRAFT_REPO_ROOT/bench.py --workload stress --steps 2 --warmup 1 --no-cpu-baseline > $GRAFT_REPO_ROOT/$OUT/prof_stress.log 2>&1 \
    || { echo "rocprof stress failed"; tail $GRAFT_REPO_ROOT/$OUT/prof_stress.log; exit 1; }
echo done
