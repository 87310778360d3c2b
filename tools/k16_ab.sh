#!/bin/bash
# A/B of builds of libaesmc_hip.so on one MI355X in one session: for every named library, in turn and ROUNDS times over,
# one plain `bench.py` run (default arguments: ms_per_step of the replayed forward ELBO, workload c4); then one
# `rocprofv3 --kernel-trace --stats` pass each over the replayed workload for the item kernel's average (runs of their
# own, no counters).  With DUMP=1 each library also leaves loss.npy of `--dump-outputs` for c4, tiny and c4s, and their
# checksums are printed.
#   tools/k16_ab.sh OUTDIR ROUNDS NAME=path/to/lib.so [NAME=path ...]
# The library in the package is replaced by each candidate in turn and by the FIRST one named at the end; every step
# runs under a time limit of its own and the script stops at the first step that fails.
set -u
cd "$(dirname "$0")/.."
OUT=${1:?output directory}; ROUNDS=${2:?rounds}; shift 2
mkdir -p "$OUT"
LIB=aesmc_amd/libaesmc_hip.so
use() { cp "${1#*=}" $LIB; }
for round in $(seq 1 "$ROUNDS"); do
  for entry in "$@"; do
    name=${entry%%=*}
    use "$entry" || exit 1
    timeout -k 10 240 python3 bench.py > "$OUT/bench_${name}_${round}.json" 2> "$OUT/bench_${name}_${round}.err" || { echo "bench $name failed"; exit 1; }
    python3 -c "import json,sys; r=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('bench', sys.argv[2], sys.argv[3], r['ms_per_step'])" "$OUT/bench_${name}_${round}.json" "$name" "$round"
  done
done
for entry in "$@"; do
  name=${entry%%=*}
  use "$entry" || exit 1
  (export TMPDIR=/tmp; timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$name" -- \
      python3 bench.py --steps 10 --warmup 3 > "$OUT/prof_$name.json" 2> "$OUT/prof_$name.err") || { echo "rocprofv3 $name failed"; exit 1; }
  stats=$(ls "$OUT"/prof_$name/*/*kernel_stats.csv | head -1)
  python3 tools/summarize_rocprof.py "$stats" 6 > "$OUT/rocprof_$name.csv"
  rm -rf "$OUT/prof_$name"
  echo "rocprof $name $(grep affine_propagate_item_kernel "$OUT/rocprof_$name.csv" | head -1 | cut -d, -f2-4)"
  if [ "${DUMP:-0}" = 1 ]; then
    for workload in c4 tiny c4s; do
      timeout -k 10 240 python3 bench.py --workload $workload --steps 10 --warmup 3 --dump-outputs "$OUT/dump_${name}_$workload" \
          > /dev/null 2> "$OUT/dump_${name}_$workload.err" || { echo "dump $name $workload failed"; exit 1; }
      echo "loss $name $workload $(sha256sum < "$OUT/dump_${name}_$workload/loss.npy" | cut -c1-16)"
    done
  fi
done
use "$1"
