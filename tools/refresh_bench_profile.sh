# Bench line (+ the stock-fp32-GEMM line beside it) and the rocprofv3 kernel stats of the same command -> <out dir>.
# Every run is a --full run, as the committed profiles are.  The trace run sets BOT_GEMM_TUNE=0 so that the candidate-timing launches
# of the first step are not in the statistics, and names --gemm halves so that the extra stock-fp32 loop of --full is not in them either.
#   bash tools/refresh_bench_profile.sh <out dir>
set -x
cd "$(dirname "$0")/.."
R=$(pwd)
O=$(mkdir -p "${1:?usage: tools/refresh_bench_profile.sh <out dir>}" && cd "$1" && pwd)
python bench.py --full --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err
tail -c 300 $O/bench.json
python bench.py --full --steps 20 --warmup 5 --gemm f32 --cpu-baseline off > $O/bench_gemm_f32.json 2>> $O/bench.err
cd /tmp; export TMPDIR=/tmp
BOT_GEMM_TUNE=0 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_b -o r -- python3 $R/bench.py --full --steps 20 --warmup 5 --cpu-baseline off --gemm halves > /tmp/b.log 2>&1
cp /tmp/prof_b/*kernel_stats.csv $O/bench_kernel_stats.csv || find /tmp/prof_b -name "*kernel_stats.csv" -exec cp {} $O/bench_kernel_stats.csv \;
tail -1 /tmp/b.log | cut -c1-200
