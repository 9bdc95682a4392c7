#!/bin/bash
# Quick A/B helper for the GPU box: bench lines (no CPU baseline) of the C3 train and eval steps, kernel times printed.
# usage: profiles/tools/quick_bench.sh TAG [WORKLOAD [OUTDIR]]      -> OUTDIR/qb_TAG_{train,eval}.json (OUTDIR: bench_out)
tag=${1:-x}; wl=${2:-C3}; out=${3:-bench_out}
mkdir -p $out
for mode in train eval; do
  python bench.py --workload $wl --mode $mode --no-cpu-baseline --full > $out/qb_${tag}_${mode}.json 2> $out/qb_${tag}_${mode}.err || { tail -5 $out/qb_${tag}_${mode}.err; exit 1; }
done
python - "$tag" "$out" <<'PY'
import json, sys
tag, out = sys.argv[1], sys.argv[2]
for mode in ("train", "eval"):
    d = json.loads(open("%s/qb_%s_%s.json" % (out, tag, mode)).read().strip().splitlines()[-1])
    r = d["roofline"]
    print(tag, mode, "%.3f ms" % d["ms_per_step"], {k: round(v, 3) for k, v in r["kernel_ms"].items()}, "frac %.3f" % r["frac"],
          "main", {k: round(v.get("ms", 0), 3) if isinstance(v, dict) else v for k, v in (r.get("main_piece") or {}).items()})
PY
