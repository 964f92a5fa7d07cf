#!/bin/bash
# tools/ab_libs.sh OUTFILE ROUNDS STEPS WARMUP "BENCH ARGS" NAME… — the A/B protocol of DESIGN §7.21: the named builds of the library
# (slr_amd/csrc/variants/libslrhip_NAME.so; "tree" is the working tree's) alternating in ONE job, ROUNDS times, each run a fresh
# `bench.py --gpus 1 --steps STEPS --warmup WARMUP BENCH ARGS --dump-outputs`; WARMUP_RUNS=1 puts one run of each library first.
# One line per run in $AB_OUT/OUTFILE (AB_OUT: the output directory, default bench_out; tools/ab_line.py): ms per frame, bench.py's HIP-event kernel times and launches per frame, the
# three counters, the SHA-256 of the frame.  Stops at the first run that fails.
dir=${AB_OUT:-bench_out}; out=$dir/$1; rounds=$2; steps=$3; warm=$4; bargs=$5; shift 5
mkdir -p $dir
dump=$(mktemp -d)
run() {   # NAME PREFIX
  if [ "$1" = tree ]; then unset SLRHIP_LIBRARY; else export SLRHIP_LIBRARY=$PWD/slr_amd/csrc/variants/libslrhip_$1.so; fi
  rm -rf $dump/frame
  timeout -k 10 280 python bench.py --gpus 1 --steps $steps --warmup $warm $bargs --dump-outputs $dump/frame > $dump/out.txt 2> $dump/err.txt
  rc=$?
  if [ $rc != 0 ]; then echo "$1 FAILED rc $rc" | tee -a $out; tail -5 $dump/err.txt | tee -a $out; exit $rc; fi
  echo -n "$2" >> $out
  python tools/ab_line.py $1 $dump/frame $steps < $dump/out.txt | tee -a $out
}
if [ "$WARMUP_RUNS" = 1 ]; then for v in "$@"; do run $v "warm-up  "; done; fi
for r in $(seq $rounds); do for v in "$@"; do run $v ""; done; done
rm -rf $dump
