#!/bin/bash
# Per-kernel time vs batch size (fixed launch costs vs per-item costs).
#   usage: tools/batch_sweep.sh OUT_DIR
set -o pipefail
out=${1:?usage: tools/batch_sweep.sh OUT_DIR}
mkdir -p $out
for B in 128 256 512 1024; do
  timeout -k 10 200 python bench.py --full --no-cpu --steps 10 --batch $B > $out/b$B.log 2>&1 || { tail -5 $out/b$B.log; exit 1; }
  echo B=$B $(tail -1 $out/b$B.log | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); k=d["roofline"]["kernels_ms"]; print(round(d["value"]/1e9,2), "G", {a: round(v*1e3/d["config"]["batch_per_gpu"],3) for a,v in k.items()}, "us/utt")')
done
