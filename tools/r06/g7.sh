O=${CGCN_PROFILE_OUT:-profile_out}/r06
mkdir -p "$O"
python -m pytest tests/test_gpu_saliency.py -x -q -m gpu > $O/t_sal.log 2>&1; tail -8 $O/t_sal.log
python bench.py --full --steps 10 --warmup 3 > $O/bench_full.json 2> $O/bench_full.err; tail -3 $O/bench_full.err
python - "$O/bench_full.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['ms_per_step'], d['value'])
print(json.dumps(d['cpu_baseline'])[:700])
r=d['roofline']; print({k:r[k] for k in ('kernel','frac','achieved','gather_GBps','gather_reference_GBps','frac_of_gather_reference','avg_kernel_us')})
print(r['all_kernels_us'])
print(d.get('saliency_ms'), json.dumps(d.get('sddmm_roofline'))[:600])
PY
