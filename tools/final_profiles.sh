#!/bin/bash
# regenerates the round's committed evidence under OUTDIR (copied to profiles/ afterwards): tools/final_profiles.sh OUTDIR
O=$(realpath -m "${1:?usage: tools/final_profiles.sh OUTDIR}")
set -x
mkdir -p $O
python bench.py --full > $O/bench.json 2> $O/bench.err
cat $O/bench.json
export TMPDIR=/tmp; R=$PWD; cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -- python $R/bench.py --steps 5 --warmup 2 --no-cpu-baseline > $O/stats.log 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmc_$c -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc_$c.log 2>&1
done
cd $R
python bench.py --algo plsnipals --p 2000 --q 1 --nlv 50 --steps 2 --warmup 1 --no-cpu-baseline > $O/bench_cfg4.json 2>/dev/null
python bench.py --dtype bf16 --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_bf16.json 2>/dev/null
python tools/host_rate.py > $O/host_rate.json 2>/dev/null
python tools/bench_lwplsr.py 2>/dev/null | tail -1 > $O/lwplsr_cfg5.json
python tools/bench_gridcv.py 2>/dev/null | tail -1 > $O/gridcv.json
python tools/bench_accessors.py 2>/dev/null | tail -1 > $O/accessors.json
python bench.py --algo plskern2 --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_plskern2.json 2>/dev/null
ls -la $O
for a in plssimp plsrosa plswold; do python bench.py --algo $a --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_$a.json 2>/dev/null; done
python tools/p2p_cost.py 2>/dev/null | tail -1 > $O/p2p_cost.json
python bench.py --rows 125000 --steps 20 --warmup 3 --no-cpu-baseline > $O/bench_rank_share_125k.json 2>/dev/null
ls -la $O
python bench.py --scal --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_scal.json 2>/dev/null
python tools/raw_mode_error.py > $O/raw_mode_error.log 2>/dev/null
python tools/small_fit_latency.py 2>/dev/null | tail -1 > $O/small_fit_latency.json
