#!/bin/bash
# three bench lines of the current build: default window (200 frames), the driver's window (20 frames from frame 5), 1024^3
# usage: tools/experiments/bench3.sh <outdir> [tag]   (the lines go to <outdir>/<tag>/)
out=${1:?usage: tools/experiments/bench3.sh <outdir> [tag]}/${2:-cur}
mkdir -p $out
python bench.py --full --no-cpu-baseline > $out/b512.json 2>$out/b512.err
python bench.py --full --no-cpu-baseline --steps 20 --warmup 5 > $out/b512_driver.json 2>/dev/null
python bench.py --full --no-cpu-baseline --volume 1024 --steps 60 > $out/b1024.json 2>/dev/null
python - "$out" <<'PY'
import json, sys
for f in ("b512", "b512_driver", "b1024"):
    try:
        j = json.loads(open(f"{sys.argv[1]}/{f}.json").read().strip().splitlines()[-1])
        r = j["roofline"]
        print(f, j["value"], "fps", j["stage_us"]["integrate"], "us integrate", r["frac"], "frac | icp", j["stage_us"]["icp"], "raycast", j["stage_us"]["raycast"])
    except Exception as e:
        print(f, "failed", e)
PY
