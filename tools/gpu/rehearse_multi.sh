#!/bin/bash
# Rehearse bench.py's N > 1 path on a one-GPU box: 2 ranks share the card,
# gloo process group (RCCL refuses two ranks on one device). The driver runs the
# real N = 2/4/8 with nccl on a full node. --full: the rank-0 gather and its
# verification are not part of a plain run. The log goes to $OUT (default out/).
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}
cd "$R"; mkdir -p "$OUT"
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29533 bench.py --full --gpus 2 --steps 10 --warmup 3 --dist-backend gloo > "$OUT/multi.log" 2>&1; rc=$?
grep -v amdgpu.ids "$OUT/multi.log" | tail -3 | cut -c1-600
grep '"gather"' "$OUT/multi.log" | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('gather', d['gather'], 'value', d['value'], 'n_gpus', d['n_gpus'])"
exit $rc
