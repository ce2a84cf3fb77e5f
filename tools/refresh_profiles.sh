# Regenerates what profiles/ holds for a round: bench line (--full), rocprofv3 kernel stats of the same command, the --pmc passes over
# tools/microbench.py (FETCH_SIZE / WRITE_SIZE / TCC hits in separate passes), microbench and config 3-5 checks -> <out dir>.
#   bash tools/refresh_profiles.sh <out dir>
set -x
cd "$(dirname "$0")/.."
R=$(pwd)
O=$(mkdir -p "${1:?usage: tools/refresh_profiles.sh <out dir>}" && cd "$1" && pwd)
python bench.py --full --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err
tail -c 600 $O/bench.json
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_b -o r -- python3 $R/bench.py --full --steps 20 --warmup 5 --cpu-baseline off > /tmp/b.log 2>&1
cp /tmp/prof_b/*kernel_stats.csv $O/bench_kernel_stats.csv
for c in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum"; do
  n=$(echo $c | tr ' ' '_')
  rocprofv3 --pmc $c --output-format csv -d /tmp/pmc_$n -o r -- python3 $R/tools/microbench.py --only spmm,spmm_dot,sddmm --iters 3 > /tmp/pmc_$n.log 2>&1
done
python3 $R/tools/pmc_summary.py /tmp/pmc_* > $O/pmc_microbench.csv
wc -l $O/pmc_microbench.csv
python3 $R/tools/microbench.py --iters 10 > $O/microbench.jsonl 2>/dev/null
python3 $R/tools/scale_check.py reddit proteins products 2>/dev/null | grep workload > $O/scale_check.jsonl
