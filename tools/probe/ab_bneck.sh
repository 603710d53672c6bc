set -e
out=${OUT:-out}/bn
mkdir -p $out
export GLSDET_TUNE_CACHE=/tmp/tc_a.json
GLSDET_NO_BNECK_FUSION=1 timeout -k 10 300 python bench.py --full --no-secondary --no-cpu-baseline --steps 50 --warmup 10 --op-table $out/ops_off.tsv > $out/off.log 2>&1
export GLSDET_TUNE_CACHE=/tmp/tc_b.json
timeout -k 10 300 python bench.py --full --no-secondary --no-cpu-baseline --steps 50 --warmup 10 --op-table $out/ops_on.tsv > $out/on.log 2>&1
export GLSDET_TUNE_CACHE=/tmp/tc_c.json
GLSDET_FORCE_BNECK=1 timeout -k 10 300 python bench.py --full --no-secondary --no-cpu-baseline --steps 50 --warmup 10 --op-table $out/ops_force.tsv > $out/force.log 2>&1
export GLSDET_TUNE_CACHE=/tmp/tc_a.json
GLSDET_NO_BNECK_FUSION=1 timeout -k 10 300 python bench.py --full --no-secondary --no-cpu-baseline --steps 50 --warmup 10 > $out/off2.log 2>&1
export GLSDET_TUNE_CACHE=/tmp/tc_b.json
timeout -k 10 300 python bench.py --full --no-secondary --no-cpu-baseline --steps 50 --warmup 10 > $out/on2.log 2>&1
for f in off on force off2 on2; do tail -1 $out/$f.log | python -c "
import json,sys; d=json.loads(sys.stdin.read()); r=d['roofline']; print('$f', d['value'], d['ms_per_step'], r['conv_ms_per_step'], r['all_ops_ms_per_step_eager'], r['launches_per_step'], r['frac'])"; done
