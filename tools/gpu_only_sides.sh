#!/bin/bash
# Each side of the step alone (RELA_BENCH_ONLY), per precision, with its per-kernel table.
#   tools/gpu_only_sides.sh [OUT]      lines and detail records under OUT (default: a new temporary directory)
O=${1:-$(mktemp -d)}; mkdir -p $O; echo "output: $O"
for prec in f32 bf16x2; do for side in learner actor; do
RELA_BENCH_ONLY=$side python bench.py --full --precision $prec --steps 200 --repeats 3 --no-cpu-baseline --no-threaded > $O/only_${side}_$prec.json 2>/dev/null
python - <<PY
import json, shutil
line=json.loads(open("$O/only_${side}_$prec.json").read().strip().splitlines()[-1])
shutil.copy(line["detail"], "$O/detail_${side}_$prec.json")  # the record this run wrote, named by its own line
d=json.load(open("$O/detail_${side}_$prec.json"))
k=d["kernels_ms_per_step"]
print("$side $prec ms/step", round(d["ms_per_step"],4), "sum kernels", round(sum(k.values()),3))
print("  ", ", ".join("%s %.3f"%(n,v) for n,v in sorted(k.items(), key=lambda kv:-kv[1])[:22]))
PY
done; done
