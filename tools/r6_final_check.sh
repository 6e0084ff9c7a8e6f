# round 6, final tree: the whole -m gpu suite, the driver's bench command, the one-rank sharded lines (metric, hetero, DeepWalk + node2vec)
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p "$OUT"
T=${1:-r6_final6}
timeout 1500 python -m pytest tests -m gpu --maxfail=5 -q > $OUT/${T}_gpu_pytest.txt 2>&1
echo "pytest rc=$?"; grep -a "passed\|failed" $OUT/${T}_gpu_pytest.txt | tail -2
timeout 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err
echo "bench rc=$?"
for W in metric hetero; do
  timeout 600 python bench.py --full --force-sharded --workload $W > $OUT/${T}_sharded_1rank_$W.json 2> $OUT/${T}_sharded_1rank_$W.err
  echo "sharded $W rc=$?"
done
timeout 600 python bench.py --full --force-sharded --workload deepwalk --n2v > $OUT/${T}_sharded_1rank_deepwalk.json 2> $OUT/${T}_sharded_1rank_deepwalk.err
echo "sharded deepwalk rc=$?"
python - "$T" <<'P'
import json,os,sys
T=sys.argv[1]
def last(p):
    l=[x for x in open(p).read().splitlines() if x.startswith('{')]
    return json.loads(l[-1])
d=last(os.environ['OUT']+'/%s_bench.json'%T); print('bench', d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['avg_launch_ms'])
for W in ('metric','hetero','deepwalk'):
    d=last(os.environ['OUT']+'/%s_sharded_1rank_%s.json'%(T,W)); print('sharded', W, d['value'], d['ms_per_step'], d.get('roofline',{}).get('frac'))
print(json.dumps(d['config'].get('node2vec'))[:600])
P
