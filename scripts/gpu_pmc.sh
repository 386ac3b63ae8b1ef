# PMC passes + summary + a bench line:  gpurun --timeout 1200 -- 'bash scripts/gpu_pmc.sh r04'
OUT=${OUT:-out}  # where the run's files go
pfx=${1:-r04}
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
mkdir -p $OUT/pmc
bash scripts/pmc_passes.sh $OUT/pmc | tail -12
python scripts/pmc_summary.py $OUT/pmc profiles/$pfx > $OUT/pmc_summary.log 2>&1; tail -2 $OUT/pmc_summary.log
cp profiles/${pfx}_pmc.json profiles/${pfx}_pmc_summary.md $OUT/
python bench.py --full --steps 50 --warmup 10 > $OUT/bench_${pfx}.json 2> $OUT/bench_${pfx}.err
grep '^{' $OUT/bench_${pfx}.json | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read()); r=d['roofline']
print(round(d['value']), d['ms_per_step'], d['long_run']['median_ms_per_step'], 'frac', round(r['frac'],4), 'in-step', r['avg_launch_ms_in_step'], 'traffic', r['traffic'], r.get('traffic_unavailable'))
print(d['cpu_baseline']['value'], d['gpu_over_cpu'])"
