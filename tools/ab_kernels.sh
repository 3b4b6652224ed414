# GPU box: per-kernel times (rocprofv3 --kernel-trace --stats) of a short bench run for several library builds.
# usage: tools/ab_kernels.sh [-k NAME,NAME,...] [-b "BENCH ARGS"] [-o DIR] lib1.so lib2.so ...   -> a table on stdout
#   -k  kernels to list: substrings of their names (default: the scatter, gather and bf16 MLP kernels)
#   -b  arguments of bench.py behind --steps 40 --warmup 5 --no-cpu-baseline --no-extras (default: --refresh 0)
#   -o  directory (absolute) that also gets abk_<n>_kernel_stats.csv of library n; the traces themselves stay under /tmp
set -u
NAMES="k_scatter,k_grid_forward,k_mlp_backward_bf16<,k_mlp_forward_bf16"
BENCH_ARGS="--refresh 0"
OUT=""
while getopts "k:b:o:" opt; do
  case $opt in
    k) NAMES=$OPTARG ;;
    b) BENCH_ARGS=$OPTARG ;;
    o) OUT=$OPTARG ;;
    *) exit 2 ;;
  esac
done
shift $((OPTIND - 1))
R=$GRAFT_REPO_ROOT
cd /tmp && export TMPDIR=/tmp
k=0
for lib in "$@"; do
  k=$((k+1))
  D=$(mktemp -d /tmp/abk_${k}_XXXXXX)
  LNERF_HIP_LIB=$R/$lib timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D -- python3 $R/bench.py --steps 40 --warmup 5 --no-cpu-baseline --no-extras $BENCH_ARGS > $D/bench.log 2>&1 || { tail -5 $D/bench.log; exit 1; }
  [ -z "$OUT" ] || cp $D/*/*kernel_stats.csv $OUT/abk_${k}_kernel_stats.csv
  echo "== $lib"
  python3 - $D/*/*kernel_stats.csv "$NAMES" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    n = r["Name"]
    if any(t in n for t in sys.argv[2].split(",")):
        print("  %-60s calls %5s avg_us %8.2f" % (n.split("(")[0][-60:], r["Calls"], float(r["AverageNs"]) / 1e3))
PY
done
