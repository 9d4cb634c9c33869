#!/bin/bash
# regenerate the judged artifacts of a round under gpurun_out/refresh (then copied into profiles/<round>/ by hand).
#   tools/refresh_profiles.sh <round dir, e.g. r02>      -- run on the GPU box via gpurun
# Order matters: the PMC traffic passes first (bench.py reads profiles/<round>/traffic.json for roofline.traffic), then rocprofv3
# kernel stats / per-shape table of the graph replay (-> graph_calls.json, which bench.py reads too), then the bench line of the
# same build and the per-call event breakdown of that command.
# Second half: the bf16 dense-cloud configuration (BASELINE configs[3]).
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
RD=${1:-r06}
O=$R/gpurun_out/refresh
rm -rf $O; mkdir -p $O $R/profiles/$RD
# (bench.py --full --steps 4 --warmup 2 --no-graph issues 2 + 4 + 46 = 52 steps: the median is always taken over >= 50)
for c in FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/pmc_$c -- python $R/bench.py --full --steps 4 --warmup 2 --no-graph --no-cpu-baseline --no-u3 --no-side > $O/pmc_$c.log 2>&1
  cp $(find $O/pmc_$c -name '*counter_collection.csv' | head -1) $O/k_pmc_$c.csv
done
python $R/tools/pmc_traffic.py $O/k_pmc_FETCH_SIZE.csv $O/k_pmc_WRITE_SIZE.csv $O/traffic.json $O/k_pmc_SQ_INSTS_VALU.csv 52 16 step_f32_b16_n1028 > /dev/null
cp $O/traffic.json $R/profiles/$RD/traffic.json
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -- python $R/bench.py --full --no-cpu-baseline --no-u3 --no-side > $O/stats_bench.log 2>&1
cp $(find $O/stats -name '*kernel_stats.csv' | head -1) $O/k_graph_kernel_stats.csv
T=$(find $O/stats -name '*kernel_trace.csv' | head -1)
python $R/tools/trace_by_shape.py $T auto > $O/k_per_shape_kernel_us.txt
python $R/tools/graph_call_us.py $O/k_per_shape_kernel_us.txt > $R/profiles/$RD/graph_calls.json
# the bench line AFTER the trace: it prices its dominant call on profiles/$RD/graph_calls.json
python $R/bench.py --full > $O/k_bench.json 2> $O/bench.err
tail -1 $O/k_bench.json | cut -c1-300
python $R/bench.py --full --steps 20 --warmup 5 --breakdown --no-cpu-baseline --no-u3 --no-side > $O/k_breakdown_eager_events.txt 2>&1
# comparison figure: the BLAS library for the dense products (tools/library_gemm.py)
HSP_GEMM=library python $R/bench.py --full --no-cpu-baseline --no-u3 --no-side > $O/k_bench_gemm_library.json 2>/dev/null
# ---- bf16, B=64, N=4096
BF="--dtype bf16 --points 4096 --batch 64 --no-cpu-baseline"
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/bpmc_$c -- python $R/bench.py --full $BF --steps 2 --warmup 1 --no-graph > $O/bpmc_$c.log 2>&1
  cp $(find $O/bpmc_$c -name '*counter_collection.csv' | head -1) $O/b_pmc_$c.csv
done
python $R/tools/pmc_traffic.py $O/b_pmc_FETCH_SIZE.csv $O/b_pmc_WRITE_SIZE.csv $O/b_traffic.json "" 51 64 step_bf16_b64_n4096 > /dev/null
python - $O/traffic.json $O/b_traffic.json $R/profiles/$RD/traffic.json <<'PY'
import json, sys
a = json.load(open(sys.argv[1])); a.update(json.load(open(sys.argv[2]))); json.dump(a, open(sys.argv[3], "w"), indent=1, sort_keys=True)
PY
cp $R/profiles/$RD/traffic.json $O/traffic.json
python $R/bench.py --full $BF --steps 10 --warmup 3 > $O/b_bench_bf16.json 2>> $O/bench.err
tail -1 $O/b_bench_bf16.json | cut -c1-300
rocprofv3 --kernel-trace --stats --output-format csv -d $O/bstats -- python $R/bench.py --full $BF --steps 10 --warmup 3 > $O/bstats_bench.log 2>&1
cp $(find $O/bstats -name '*kernel_stats.csv' | head -1) $O/b_graph_kernel_stats_bf16.csv
T=$(find $O/bstats -name '*kernel_trace.csv' | head -1)
python $R/tools/trace_by_shape.py $T last3 > $O/b_per_shape_kernel_us_bf16.txt
python $R/bench.py --full $BF --steps 5 --warmup 2 --breakdown > $O/b_breakdown_eager_events_bf16.txt 2>&1
python $R/bench.py --full --points 4096 --batch 64 --steps 10 --warmup 3 --no-cpu-baseline --no-u3 > $O/b_bench_f32_same_shape.json 2>/dev/null
# ---- the full training step (unit U3): kernels of one step by launch shape (no BLAS / Cijk row is left in it)
bash $R/tools/prof_train_step.sh > $O/u3_prof.log 2>&1
head -120 $R/gpurun_out/prof_u3/u3_per_shape_kernel_us.txt > $R/profiles/$RD/u3_per_shape_kernel_us_top120.txt
# the judged copies (trimmed: the library tuning runs of the first steps fill the long tail of the bf16 tables)
for f in k_bench.json k_pmc_FETCH_SIZE.csv k_pmc_WRITE_SIZE.csv k_bench_gemm_library.json k_graph_kernel_stats.csv k_per_shape_kernel_us.txt k_breakdown_eager_events.txt b_bench_bf16.json b_bench_f32_same_shape.json b_breakdown_eager_events_bf16.txt; do cp $O/$f $R/profiles/$RD/$f; done
head -61 $O/b_per_shape_kernel_us_bf16.txt > $R/profiles/$RD/b_per_shape_kernel_us_bf16_top60.txt
head -81 $O/b_graph_kernel_stats_bf16.csv > $R/profiles/$RD/b_graph_kernel_stats_bf16_top80.csv
mkdir -p $R/gpurun_out/profiles_$RD && cp $R/profiles/$RD/* $R/gpurun_out/profiles_$RD/
rm -rf $O/stats $O/bstats $O/pmc_FETCH_SIZE $O/pmc_WRITE_SIZE $O/bpmc_FETCH_SIZE $O/bpmc_WRITE_SIZE $O/b_pmc_*.csv
ls -la $O
