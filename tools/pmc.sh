#!/bin/bash
# usage (GPU box): tools/pmc.sh <tag> "<COUNTER ...>" [bench args...]   -- one PMC pass (with --kernel-trace only), per-kernel means printed
out=${AZ_OUT:-out}                  # where the results land
export TMPDIR=/tmp
tag=$1; ctrs=$2; shift; shift
mkdir -p $out/pmc
rocprofv3 --pmc $ctrs --kernel-trace --output-format csv -d $out/pmc -o $tag -- python3 bench.py --full --steps 1 --warmup 0 --no-episode --no-cpu --pmc-run --engines 1 "$@" > $out/pmc/${tag}_run.log 2>&1
python3 tools/pmc_summary.py $out/pmc/${tag}_counter_collection.csv
