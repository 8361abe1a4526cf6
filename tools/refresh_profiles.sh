#!/bin/bash
# usage: bash tools/refresh_profiles.sh <round> <out dir>   (<out dir>: where tools/profile_round.sh writes its prof_<round>/)
# Profiles the bench workloads (tools/profile_round.sh), condenses the raw tables (they are too large to keep), and runs the
# full bench lines right after.  Everything lands in <out dir>/<round>_summary/: copy it into profiles/<round>/.
R=$(cd "$(dirname "$0")/.." && pwd); TAG=${1:-r2}; O=${2:?usage: bash tools/refresh_profiles.sh <round> <out dir>}
cd $R
bash tools/profile_round.sh $TAG sponza_teapots test_glb sponza_class > $O/profile_round.log 2>&1
python tools/profile_summary.py $O/prof_$TAG $O/${TAG}_summary
rm -rf $O/prof_$TAG
for w in sponza_teapots test_glb sponza_class; do
  python bench.py --full --workload $w > $O/${TAG}_summary/${w}_bench.json 2> $O/${TAG}_summary/${w}_bench.err || echo "bench $w failed"
  tail -1 $O/${TAG}_summary/${w}_bench.json | cut -c1-400
done
ls -la $O/${TAG}_summary
