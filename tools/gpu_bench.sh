#!/bin/bash
# GPU bench (every leg: bench.py --full) + rocprofv3 kernel-trace summaries of its legs.
# Usage: bash tools/gpu_bench.sh TAG   (outputs under $M2DEC_AMD_OUT, default bench_out/)
set -o pipefail
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/${M2DEC_AMD_OUT:-bench_out}
mkdir -p $O
cd $R
timeout -k 10 600 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err
rc=$?; echo "bench rc=$rc"; cat $O/bench_$TAG.json; tail -5 $O/bench_$TAG.err
if [ $rc -ne 0 ]; then exit $rc; fi
cd /tmp && export TMPDIR=/tmp
# two profiles, one per roofline of the bench line, so each kernel's average is over exactly the launches
# its roofline is quoted on: the value leg (k_picture, one launch per 1080p picture) and the
# single-stream replay leg (k_batch, one launch per 60-picture pass)
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof_$TAG -o run --output-format csv -- python3 $R/bench.py > $O/prof_$TAG.log 2>&1
rc=$?; echo "rocprof rc=$rc"; tail -2 $O/prof_$TAG.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof_${TAG}_replay -o run --output-format csv -- python3 $R/bench.py --replay-only > $O/prof_${TAG}_replay.log 2>&1
rc=$?; echo "rocprof replay rc=$rc"; tail -2 $O/prof_${TAG}_replay.log
if [ $rc -ne 0 ]; then exit $rc; fi
# every leg of the full bench (decode path, replay, H.265 I and P / B, MPEG-2): one summary naming
# k_picture, k_batch, k_h265_mc / k_h265_ctu_rows / k_h265_deblock / k_h265_sao and k_m2v
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $O/prof_${TAG}_all -o run --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline > $O/prof_${TAG}_all.log 2>&1
rc=$?; echo "rocprof all rc=$rc"; tail -2 $O/prof_${TAG}_all.log
find $O/prof_$TAG $O/prof_${TAG}_replay $O/prof_${TAG}_all -name "*kernel_stats*"
exit $rc
