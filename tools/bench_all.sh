#!/bin/bash
# tools/bench_all.sh TAG [DIR] — the un-profiled full bench lines (bench.py --full) of the four BASELINE workloads (+ the
# instanced grid) on one box: DIR/TAG_bench_{n1,boxes_spectral,ibl,grid10m,grid10m_instanced}.json (DIR defaults to bench_out)
tag=$1; out=${2:-bench_out}; mkdir -p $out
python3 bench.py --full > $out/${tag}_bench_n1.json 2> $out/${tag}_b1.err; echo "headline done" >&2
python3 bench.py --full --workload boxes_spectral --steps 1 --warmup 1 > $out/${tag}_bench_boxes_spectral.json 2> $out/${tag}_b2.err
python3 bench.py --full --workload ibl --steps 1 --warmup 1 > $out/${tag}_bench_ibl.json 2> $out/${tag}_b3.err; echo "configs 2,3 done" >&2
python3 bench.py --full --workload grid10m --steps 1 --warmup 0 > $out/${tag}_bench_grid10m.json 2> $out/${tag}_b4.err; echo "grid done" >&2
python3 bench.py --full --workload grid10m --instanced --steps 1 --warmup 0 > $out/${tag}_bench_grid10m_instanced.json 2> $out/${tag}_b5.err; echo "all done" >&2
