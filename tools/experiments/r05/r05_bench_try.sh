#!/bin/bash
cd "$(dirname "$0")/../../.."; export TMPDIR=/tmp; O=${OUT:-/tmp}
( time python bench.py --full --cpu-seconds 3 ) > $O/r05_bench_try.json 2> $O/r05_bench_try.err
tail -5 $O/r05_bench_try.err
timeout 1200 python -m pytest tests/test_gpu_random.py -x -q -m gpu -k "bench_size and natural" 2>&1 | tail -3
