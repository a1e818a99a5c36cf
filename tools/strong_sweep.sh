# Strong-scaling rehearsal of BASELINE config 4 on one GPU under different small-launch thresholds: [OUT=dir] bash tools/strong_sweep.sh <tag> t1 t2 ...
# (the rehearsal is the `strong_scaling` entry of the bench line, which only a --full run measures)
TAG=$1; shift
OUT=${OUT:-results}; mkdir -p $OUT
for t in "$@"; do
  for set in cjk_like dejavu; do
    MSDFHIP_SMALL_LAUNCH_TILES=$t python bench.py --full --strong --strong-set $set --steps 12 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_strong_${set}_$t.json 2> $OUT/${TAG}_strong_${set}_$t.err
  done
done
python - <<PY
import json,glob
for f in sorted(glob.glob("$OUT/${TAG}_strong_*.json")):
    try: d=json.loads(open(f).read().strip().splitlines()[-1])
    except Exception as e: print(f, "unreadable", e); continue
    for name,row in d.get("strong_scaling",{}).items():
        if not isinstance(row,dict): continue
        print(f.split("_strong_")[1][:-5], name, "whole %.3f ms" % row["ms_whole_set"], " ".join("%s: eff %.3f max %.3f" % (k, v["efficiency"], max(v["ms_per_shard"])) for k,v in row.items() if k.startswith("x")))
PY
