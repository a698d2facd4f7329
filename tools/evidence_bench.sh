# the full bench line, then the same with the NdtWithGicp CPU leg (numpy oracle, ~100 s) to record that baseline
# usage: tools/evidence_bench.sh <output dir>
set -u
out=${1:?usage: tools/evidence_bench.sh <output dir>}
export TMPDIR=/tmp
mkdir -p "$out"
t0=$(date +%s)
python bench.py --full > "$out/bench_line.json" 2> "$out/bench.err"; echo "bench rc=$? wall=$(( $(date +%s) - t0 )) s"
python - "$out" <<'PY'
import json, sys
d=json.load(open(sys.argv[1] + '/bench_line.json'))
print(d['value'], d['roofline']['frac'], d['figures']['identity_guess']['value'], d['figures']['early_exit']['value'])
print(d['single_pair'])
print({k:(v.get('value'), v.get('ms_per_alignment'), v.get('target_kept')) for k,v in d['other_workloads'].items()})
PY
SMHIP_BENCH_GICP_CPU=1 python bench.py --full --steps 2 --warmup 1 --no-figures > "$out/bench_line_gicp_cpu.json" 2> "$out/bench2.err"; echo "bench2 rc=$?"
python - "$out" <<'PY'
import json, sys
d=json.load(open(sys.argv[1] + '/bench_line_gicp_cpu.json'))
g=d['other_workloads']['ndt_gicp']
print(g.get('cpu_baseline'), g.get('parity'))
json.dump(g.get('cpu_baseline'), open(sys.argv[1] + '/r02_gicp_cpu_baseline.json','w'))
PY
