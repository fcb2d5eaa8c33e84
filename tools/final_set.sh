#!/bin/bash
# dev tool (GPU box): the evidence set of a round on the FINAL sources, one call: rocprofv3 kernel trace + PMC passes of the bench command
# (tools/profile_round.sh), per-kernel counters of five (view, path) workloads (tools/pass_counters.sh), then the bench line itself.
# usage: tools/final_set.sh <tag> <dir>   -> <dir>/<tag>_*.log, <dir>/<tag>_bench.json (the full line), and what the two tools write
# (then, in the container: tools/summarize_profile.py <tag>; tools/summarize_pass_counters.py <tag>)
tag=$1
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=$(pwd)
D=${2:?usage: tools/final_set.sh <tag> <dir>}; mkdir -p "$D"; D=$(cd "$D" && pwd)
bash $R/tools/profile_round.sh $tag > "$D/${tag}_profile_round.log" 2>&1 || exit 1
echo "profile_round done"
for vp in "default single" "key1 three_pass" "skimmer single" "skimmer single_ordered" "skimmer shard0of8"; do
  bash $R/tools/pass_counters.sh $vp > "$D/${tag}_passc_$(echo $vp | tr ' ' '_').log" 2>&1 || { echo "pass_counters $vp FAILED"; exit 1; }
  echo "pass_counters $vp done"
done
cd $R && timeout -k 10 500 python3 bench.py --full --steps 20 --warmup 5 > "$D/${tag}_bench.json" 2> "$D/${tag}_bench.err"
echo "bench done: $(cut -c1-120 "$D/${tag}_bench.json")"
