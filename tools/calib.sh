#!/bin/bash
out=${AZ_OUT:-out}                  # where the results land
export TMPDIR=/tmp
mkdir -p $out/calib
rocprofv3 --kernel-trace --output-format csv -d $out/calib -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-episode --no-cpu > $out/calib/bench.json 2> $out/calib/err.log || exit 1
python3 tools/calib_from_trace.py $out/calib/run_kernel_trace.csv $out/calib/bench.json $out/calib/summary.json
rm -f $out/calib/run_kernel_trace.csv
