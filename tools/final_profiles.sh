set -u
T=$1
# raw output of the run: $CGCN_PROFILE_OUT/<tag>/ (default profile_out/ in the repository root); tools/collect_profiles.py
# reads it from there
R=$(cd "$(dirname "$0")/.." && pwd)
O=${CGCN_PROFILE_OUT:-$R/profile_out}/$T
mkdir -p "$O" && O=$(cd "$O" && pwd)   # (absolute: the steps below run from /tmp)
python -c "from chromegcn_amd import _build; print(_build.source_hash([]))" > $O/src_hash.txt
if [ -z "${SKIP_TESTS:-}" ]; then python -m pytest tests -m gpu -q > $O/pytest.log 2>&1; echo "pytest rc=$?" >> $O/pytest.log; tail -3 $O/pytest.log; fi
( time python bench.py --full > $O/bench_genome.json 2> $O/bench_genome.err ) 2> $O/bench_genome.time
python bench.py --full --hic-like --no-cpu-baseline > $O/bench_genome_hic.json 2>/dev/null
for w in chr21 chr1 config1; do python bench.py --full --workload $w --no-cpu-baseline > $O/bench_$w.json 2>/dev/null; python bench.py --full --workload $w --hic-like --no-cpu-baseline > $O/bench_${w}_hic.json 2>/dev/null; done
python bench.py --full --generator hub --no-cpu-baseline > $O/bench_genome_hub.json 2>/dev/null
for a in both constant none; do python bench.py --full --adj-type $a --no-cpu-baseline --no-extras > $O/bench_genome_adj_$a.json 2>/dev/null; done
for w in chr21 chr1; do python bench.py --full --workload $w --generator hub --no-cpu-baseline > $O/bench_${w}_hub.json 2>/dev/null; done
python bench.py --full --workload chr21 --d 256 --layers 4 --no-cpu-baseline > $O/bench_chr21_d256L4.json 2>/dev/null
python bench.py --full --d 256 --layers 4 --no-cpu-baseline > $O/bench_genome_d256L4.json 2>/dev/null
python bench.py --full --gpus 2 --backend gloo --share-gpu --no-cpu-baseline --no-extras > $O/bench_genome_2ranks_one_gpu_gloo.json 2>/dev/null
python bench.py --full --workload e2e > $O/bench_e2e.json 2>/dev/null
python bench.py --full --workload e2e --e2e-windows 0 > $O/bench_e2e_chr21_full.json 2>/dev/null
( cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/sal_prof && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/sal_prof -- python3 $R/tools/saliency_bench.py > $O/saliency.log 2>&1; f=$(find /tmp/sal_prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && { echo "# rocprofv3 --kernel-trace --stats -- python3 tools/saliency_bench.py (adjacency saliency of a chr21-size and a chr1-size chromosome, 6 calls each)"; cat "$f"; } > $O/saliency_kernel_stats.csv )
bash tools/profile_round.sh $T genome
bash tools/profile_round.sh $T genome_hic --hic-like
bash tools/profile_round.sh $T chr21 --workload chr21
bash tools/profile_round.sh $T chr21_hic --workload chr21 --hic-like
bash tools/profile_round.sh $T chr1 --workload chr1
bash tools/profile_round.sh $T chr1_hic --workload chr1 --hic-like
bash tools/profile_round.sh $T chr21_d256L4 --workload chr21 --d 256 --layers 4
bash tools/profile_round.sh $T genome_hub --generator hub
bash tools/profile_round.sh $T genome_constant --adj-type constant
bash tools/profile_round.sh $T genome_both --adj-type both
for f in $O/bench_*.json; do python - "$f" <<'PY'
import json,sys
try:
    d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[1].split('/')[-1], round(d['ms_per_step'],4), 'ms', round(d['value']/1e6,2), 'M win/s')
except Exception as e: print(sys.argv[1], 'ERR', e)
PY
done
