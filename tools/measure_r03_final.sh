#!/bin/bash
# GPU box, end of round 3: everything under profiles/r03_* measured again on the final binary, in two calls
# (usage: tools/measure_r03_final.sh a|b).  Results land under $AZ_OUT (default out/); copy what is to be judged into profiles/.
out=${AZ_OUT:-out}                  # where the results land
export TMPDIR=/tmp
mkdir -p $out/prof $out/pmc
if [ "${1:-a}" = a ]; then
  python bench.py --full > $out/r03_bench.json 2> $out/r03_bench.err; echo "bench rc=$?"
  tools/measure_r03_evidence.sh benches
  python tools/latency.py $out/r03_latency.json 2>&1 | grep -v amdgpu.ids
  python tools/upgrades_gain.py > $out/r03_upgrades.json 2> $out/upg.err; tail -c 600 $out/r03_upgrades.json
else
  tools/measure_r03_evidence.sh profiles
  python tools/episode_trace.py 4 > $out/r03_episode_trace.txt 2>&1; tail -4 $out/r03_episode_trace.txt
fi
