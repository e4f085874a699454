# parity tests, then the f32 / f64 bench lines with the phase breakdown; files under $OUT (default: a new temporary directory)
OUT=${OUT:-$(mktemp -d)}; echo "output: $OUT"
python -m pytest tests/test_gpu_parity.py -x -q -m gpu > $OUT/t.log 2>&1; tail -5 $OUT/t.log
python bench.py --full --dtype f32 --no-cpu-baseline > $OUT/b32.json 2> $OUT/b32.err
python bench.py --full --dtype f64 --no-cpu-baseline > $OUT/b64.json 2> $OUT/b64.err
ILQR_BACKWARD_NO_PIN=1 python bench.py --full --dtype f32 --no-cpu-baseline > $OUT/b32r.json 2> $OUT/b32r.err
python - "$OUT" <<'PY'
import json, sys
for f in [f"{sys.argv[1]}/{b}.json" for b in ("b32", "b64", "b32r")]:
    try:
        d=json.load(open(f)); print(f, d["dtype"], "%.3g it/s"%d["value"], "%.3f ms"%d["ms_per_step"], "bw %.0f GB/s %.3f"%(d["roofline"]["achieved"], d["roofline"]["frac"]), {k:round(v,1) for k,v in d["phases_us_per_step"].items()})
    except Exception as e: print(f, "ERR", e); print(open(f.replace(".json",".err")).read()[-1500:])
PY
