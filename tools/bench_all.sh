set -u
# The benchmark records of a round on one GPU: every workload with its --full line (CPU baseline, 10-digit leg), the driver's plain
# 20-step run, the all-kernel table and the rank shares.  Records go to ${OUT:-bench_records}/${TAG:-r04}_bench/ (git-ignored).
out=${OUT:-bench_records}/${TAG:-r04}_bench
mkdir -p $out
python bench.py --full > $out/n1.json 2> $out/n1.err
python bench.py --steps 20 --warmup 3 > $out/n1_driver_style.json 2>> $out/n1.err
for w in laplace_sl_16k laplace_sldl stokeslet stokeslet_f32 helmholtz p2p_lists near_apply; do
  st=5; [ $w = laplace_sl_16k ] && st=200
  python bench.py --full --workload $w --steps $st --warmup 2 > $out/$w.json 2>> $out/n1.err
done
python bench.py --workload laplace_sl_f32 --steps 2 --warmup 1 --no-cpu-baseline > $out/laplace_sl_f32_1gpu.json 2>> $out/n1.err
python tools/time_all_digits.py > $out/all_kernels_full_vs_10digits.txt 2>&1
python tools/rank_share.py > $out/rank_share.txt 2>&1
for f in $out/*.json; do python - "$f" <<'PY'
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[1].split('/')[-1], "%.3f ms/step" % d['ms_per_step'], "frac %.4f" % d['roofline']['frac'], "value %.4g" % d['value'], (d.get('at_reference_callers_accuracy') or {}).get('ms_per_step'), (d.get('cpu_baseline') or {}).get('value'), (d.get('cpu_baseline') or {}).get('cores'), (d.get('cpu_baseline') or {}).get('threads'))
PY
done
cat $out/all_kernels_full_vs_10digits.txt $out/rank_share.txt
