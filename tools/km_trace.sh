set -e
R=$GRAFT_REPO_ROOT
cd /tmp && export TMPDIR=/tmp
O=${1:-$R/bench_out}; mkdir -p $O
timeout -s KILL 200 rocprofv3 --kernel-trace --stats -d $O/kmt -o p --output-format csv -- python3 $R/bench.py --full --dot 0 --cpu-baseline 0 --steps 2 > $O/kmt.log 2>&1
