set -e
out=${OUT:-out}/gn
mkdir -p $out
W=mp_det_res50_1344x800_bs8
export GLSDET_TUNE_CACHE=/tmp/tc_a.json
timeout -k 10 400 python bench.py --full --no-secondary --no-cpu-baseline --workload $W --steps 30 --warmup 8 --op-table $out/ops_off.tsv > $out/off.log 2>&1
export GLSDET_TUNE_CACHE=/tmp/tc_b.json
GLSDET_GN_FUSION=1 timeout -k 10 400 python bench.py --full --no-secondary --no-cpu-baseline --workload $W --steps 30 --warmup 8 --op-table $out/ops_on.tsv > $out/on.log 2>&1
export GLSDET_TUNE_CACHE=/tmp/tc_a.json
timeout -k 10 400 python bench.py --full --no-secondary --no-cpu-baseline --workload $W --steps 30 --warmup 8 > $out/off2.log 2>&1
export GLSDET_TUNE_CACHE=/tmp/tc_b.json
GLSDET_GN_FUSION=1 timeout -k 10 400 python bench.py --full --no-secondary --no-cpu-baseline --workload $W --steps 30 --warmup 8 > $out/on2.log 2>&1
for f in off on off2 on2; do tail -1 $out/$f.log | python -c "
import json,sys; d=json.loads(sys.stdin.read()); r=d['roofline']; print('$f', d['value'], d['ms_per_step'], r['conv_ms_per_step'], r['all_ops_ms_per_step_eager'], r['launches_per_step'], r['frac'])"; done
grep -i "groupnorm\|gn stats" $out/ops_on.tsv
