cd "${GRAFT_REPO_ROOT:-/root/repo}"
show() {  # label, bench line
  python -c "import json,sys; d=json.loads(sys.argv[2]); r=d['roofline']; print(sys.argv[1], d['value'], d['ms_per_step'], r['kernel'], r['frac'], r['iteration']['traffic_ratio'], d.get('cpu_baseline',{}).get('value'))" "$1" "$2"
}
for i in 1 2; do
  line=$(set -o pipefail; timeout -k 10 300 python bench.py --full | tail -1) || exit $?
  show default_$i "$line"
done
line=$(set -o pipefail; timeout -k 10 300 python bench.py --full --steps 200 --warmup 10 --no-cpu-baseline | tail -1) || exit $?
show steps_200 "$line"
