#!/bin/bash
# same-box A/B of the loop detector's candidate search: prs_place_query_batch of _abtmp/base (a built copy of the parent commit)
# against this tree's prs_place_bank_query_batch and prs_place_query_batch, alternating; the base runs three times for the spread.
# B sequences query M stored maps of 1500 random rows: the base and the "shared" rows share ONE database of M maps, the bank keeps M
# maps per sequence -- the same B * 1500 * M * 1500 pairs.
# usage (GPU box, repo root): bash tools/ab_place.sh [reps]
REPS=${1:-10}
cat > /tmp/ab_place.py <<PY
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
from srrg2_proslam_amd import configs, ops
which, reps, ROWS = sys.argv[1], $REPS, 1500
PADDED = (ROWS + 15) // 16 * 16
ctx = ops.Context(0)
rng = np.random.default_rng(0)
rows, qrows = (rng.integers(0, 256, (ROWS, 32), dtype=np.uint8) for _ in range(2))
P = ops.place_params(configs.get("kitti")["place"], max_candidates=8, minimum_age_difference_to_candidates=0)

def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps

for M in (16, 64):
    for B in (1, 64, 1024):
        if which == "bank":
            db = ops.PlaceBank(ctx, B, M, M * PADDED)
            q = ops.PlaceQueries(0, B, ROWS, 8, None, count_stride=M, key_stride=M * PADDED, corr_stride=ROWS)
            q.desc[:, :ROWS] = torch.from_numpy(rows).to(q.desc.device)
            q.n_query.fill_(ROWS)
            for m in range(M):
                q.graph_id.fill_(m)
                db.append(q)
            run = lambda: ops.place_bank_query_batch(ctx, db, P, q)
        else:
            db = ops.PlaceDatabase(ctx)
            db.reserve(M, M * PADDED)
            for m in range(M):
                db.add(m, rows)
            q = ops.PlaceQueries(0, B, ROWS, 8, db)
            run = lambda: ops.place_query_batch(ctx, db, P, q)
        q.desc[:, :ROWS] = torch.from_numpy(qrows).to(q.desc.device)
        q.n_query.fill_(ROWS)
        q.graph_id.fill_(10**6)
        ms = timed(run)
        print(json.dumps({"run": sys.argv[2], "entry": which, "maps": M, "batch": B, "ms": round(ms, 4),
                          "pairs_per_s": float(B) * ROWS * M * ROWS / (ms * 1e-3)}), flush=True)
        db.close()
        del q, db
        torch.cuda.empty_cache()
ctx.close()
PY
set -e -o pipefail
for i in 1 2 3; do
  (cd _abtmp/base && timeout -k 10 300 python /tmp/ab_place.py shared base$i 2>&1 | grep '^{')
  if [ $i -lt 3 ]; then
    timeout -k 10 300 python /tmp/ab_place.py bank new$i 2>&1 | grep '^{'
    timeout -k 10 300 python /tmp/ab_place.py shared new$i 2>&1 | grep '^{'
  fi
done
