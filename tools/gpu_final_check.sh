#!/bin/bash
# round-end rehearsal: the -m gpu suite, smoke(), and the default bench line
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p gpurun_out
bash tools/gpu_tests.sh > gpurun_out/final_tests.txt 2>&1 || { tail -20 gpurun_out/final_tests.txt; exit 1; }
tail -1 gpurun_out/final_tests.txt
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > gpurun_out/final_smoke.log 2>&1 || { tail -5 gpurun_out/final_smoke.log; exit 1; }
tail -1 gpurun_out/final_smoke.log
line=$(set -o pipefail; timeout -k 10 300 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 | tail -1) || exit 1
python3 -c "import json,sys; d=json.loads(sys.argv[1]); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['cpu_baseline']['value'])" "$line"
