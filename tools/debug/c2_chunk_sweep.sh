#!/bin/bash
# C2 step time against the slice length of the small-batch mode, one box.
mkdir -p gpurun_out/c2sweep
for c in 512 256 192 128 96; do
  TPHIP_SITE_CHUNK=$c timeout -k 10 200 python bench.py --workload C2 --steps 30 --warmup 5 --cpu-seconds 0 --stage1-loci 0 > gpurun_out/c2sweep/c$c.json 2> gpurun_out/c2sweep/c$c.err || exit 1
  python - $c <<'PY'
import json, sys
d = json.loads(open("gpurun_out/c2sweep/c%s.json" % sys.argv[1]).read().strip().splitlines()[-1])
print("chunk", sys.argv[1], "ms/step %.4f site %.4f evals %d" % (d["ms_per_step"], d["stages_ms"]["site_rate_kernel"], d["fp64"]["evals_per_launch"]), flush=True)
PY
done
