# tools/final_evidence.sh OUTDIR: the GPU suite and the benchmark's --full line, summarised
OUT="${1:?usage: tools/final_evidence.sh OUTDIR}"; mkdir -p "$OUT"
python -m pytest tests -m gpu -q -x 2>&1 | grep -v Warn | tail -4 > "$OUT/final_gpu_suite.txt"; cat "$OUT/final_gpu_suite.txt"
python bench.py --full > "$OUT/bench_line_final.json" 2> "$OUT/bench_line_final.err"
python -c "
import json, sys; d=json.load(open(sys.argv[1])); p=d['config']['paths']; print(d['value'], d['ms_per_step'], d['sustained_iters_per_s'], p['heavy_raster']['ms_per_step'], p['patched']['ms_per_step'], {k:v for k,v in d.items() if 'render' in k})" "$OUT/bench_line_final.json"
