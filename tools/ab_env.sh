#!/bin/bash
# A/B bench of environment settings on a GPU: tools/ab_env.sh "NAME=VALUE ..." "NAME=VALUE ..." ...  (one bench run per argument, --full without the side legs; "" = defaults)
T=$(mktemp -d)
i=0
for v in "$@"; do
  i=$((i+1))
  env $v timeout 300 python bench.py --full --cpu-frames 0 --host-frames 0 --pose-frames 0 --latency-calls 0 --pipelined-steps 0 ${BENCH_ARGS} 2>$T/abenv_$i.err | tail -1 > $T/abenv_$i.json
  python - "$v" $T/abenv_$i.json <<PY
import json, sys
d = json.load(open(sys.argv[2]))
s = d["stage_ms_per_step"]
print("[%s]" % sys.argv[1], d["value"], "fps (one stream %s)  sweep frac" % (d.get("one_stream") or {}).get("value"), d["roofline"]["frac"], " ".join("%s=%.3f" % (k, v) for k, v in s.items()))
PY
done
