R=$(cd "$(dirname "$0")/.." && pwd); O=${1:?usage: prof_bench.sh OUTDIR}; mkdir -p $O; O=$(cd $O && pwd)
python -m pytest tests/test_gpu_units.py tests/test_gpu_ipm.py tests/test_gpu_sdpi.py -m gpu -q 2>&1 | grep -E "passed|failed|FAILED|Error" | head
cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats -d $O/prof_e -o e -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu > $O/bench_e.json 2>$O/bench_e.err; cut -c1-200 $O/bench_e.json
