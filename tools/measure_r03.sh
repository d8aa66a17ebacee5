#!/bin/bash
# GPU box, round 3: the -m gpu suite, the latency path under rocprofv3 (single search, 51-game arena), kernel stats with one
# lane (every kernel alone on the GPU) and the headline bench line.  usage: tools/measure_r03.sh [tag] [suite|nosuite]
out=${AZ_OUT:-out}                  # where the results land
export TMPDIR=/tmp
tag=${1:-r03}
mkdir -p $out/prof
if [ "${2:-suite}" = suite ]; then
  AZ_PARITY_REPORT=$(realpath $out)/${tag}_emulated_trunk_parity.json python -m pytest tests -m gpu -x -q > $out/${tag}_suite.log 2>&1; rc=$?
  tail -4 $out/${tag}_suite.log
  [ $rc -ne 0 ] && exit $rc
fi
python3 tools/latency_prof.py search > $out/${tag}_latency.txt 2>&1
python3 tools/latency_prof.py arena >> $out/${tag}_latency.txt 2>&1
cat $out/${tag}_latency.txt
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o ${tag}_lat_search -- python3 tools/latency_prof.py search > $out/prof/${tag}_lat_search.log 2>&1
python3 tools/kstats.py $out/prof/${tag}_lat_search_kernel_stats.csv 10
tools/prof.sh ${tag}_f32_engines1 --engines 1
python3 bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err; echo "bench rc=$?"
python3 - <<PY
import json
d = json.load(open("$out/${tag}_bench.json"))
print("exp/s", round(d["value"]), "ms/ply", round(d["ms_per_step"], 2), "frac", round(d["roofline"]["frac"], 4), "games/s", d["self_play_games_per_sec"], d["self_play_games_per_sec_steady_state"],
      [(r["kernel"][:6], round(r["avg_launch_ms"] * 1e3, 1)) for r in d["roofline"]["rest"]])
PY
