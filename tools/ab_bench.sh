#!/bin/bash
# A/B of library variants in one gpurun call: tools/ab_bench.sh "B1 B2 .." lib1.so lib2.so ...
# REPS alternating rounds (default 2).  Per run: the headline rate, the one-lane rate and the single-scan latency (the two where host
# work per enqueue shows), the mean NN launch and the parity verdict.  A run that fails or outlives BENCH_TIMEOUT seconds ends the script.
set -o pipefail
L=slam_sensor_fusion_amd/lib/libslamfusion.so
BS="$1"; shift
cp $L /tmp/orig.so
for rep in $(seq 1 ${REPS:-2}); do
for lib in "$@"; do
  cp $lib $L
  for B in $BS; do
    timeout -k 10 ${BENCH_TIMEOUT:-300} python bench.py --full $BENCH_EXTRA --steps 8 --warmup 2 --batch $B --no-cpu-baseline 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); r=lambda k: None if d.get(k) is None else round(d[k],3); print(sys.argv[1], 'B', d['config']['scans_in_flight'], 'scans/s', round(d['value'],1), 'no_pipeline', r('value_no_pipeline'), 'single_scan_ms', r('single_scan_latency_ms'), 'nn_us', round(d['roofline']['avg_launch_ms']*1e3,1), d['parity']['ok'], flush=True)" $(basename $lib) || { cp /tmp/orig.so $L; exit 1; }
  done
done
done
cp /tmp/orig.so $L
