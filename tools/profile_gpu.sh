#!/bin/bash
# Run on the GPU box (through gpurun): kernel trace + stats, then PMC passes (own runs, no tracing domains mixed in).
# usage: tools/profile_gpu.sh <tag>      outputs under gpurun_out/prof_<tag>/
set -e
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/prof_$TAG
mkdir -p $OUT
# build OUTSIDE the profiler: under rocprofv3 the tool library has initialised the GPU before Python starts, and bench.py must
# not spawn make from there (it gets --no-build and fails loudly on a missing or stale artefact instead)
# (only when the library is missing or older than its sources: a current one is not compiled again on the GPU box)
python3 -c "import sys; sys.path.insert(0, '$R/hybrid-ode-for-glp-1-and-glucose_amd'); from hode import _build; _build.ensure(jobs=8, quiet=False)" > $OUT/build.log 2>&1
make -C $R/oracle -s >> $OUT/build.log 2>&1
export TMPDIR=/tmp
cd /tmp
# --no-zscore: every launch of solve_fwd_kernel<float,4,0,2,false,false> is then the benchmark workload (physio cohort,
# 4 096 x 241), so the profile's average duration of that kernel IS bench.py's ms_per_step; the z-scored regime gets its own
# trace below (same kernel name, other workload: 3.7-3.9 ms)
ARGS="--full --steps 12 --warmup 3 --train-steps 12 --no-cpu-baseline --no-vi --no-generic --no-zscore --no-sobol --no-class-path --no-build"
# the kernel sources these counters belong to (bench.py reports PMC traffic only while this hash matches)
python3 -c "import sys; sys.path.insert(0, '$R'); import bench; print(bench.kernel_source_sha())" > $OUT/kernel_source_sha.txt
# the trace pass runs 40 + 5 forward launches and 20 training steps: the first launches of a process are slower (clocks, cold
# caches), with 11 adjoint launches they moved its average 5 % above the bench's figure
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 $R/bench.py --full --steps 40 --warmup 5 --train-steps 20 --no-cpu-baseline --no-vi --no-generic --no-zscore --no-sobol --no-class-path --no-build > $OUT/bench_trace.log 2>&1
echo "trace done"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_zscore -- python3 $R/tools/zscore_launches.py > $OUT/bench_trace_zscore.log 2>&1
echo "zscore trace done"
for C in FETCH_SIZE WRITE_SIZE "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU" "SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VMEM SQ_INSTS_SMEM GRBM_GUI_ACTIVE"; do
  N=$(echo $C | tr ' ' '_' | cut -c1-40)
  # (a pass that fails ends the run: nothing more is started on a card that may have faulted)
  timeout -k 10 300 rocprofv3 --pmc $C --output-format csv -d $OUT/pmc_$N -- python3 $R/bench.py $ARGS > $OUT/bench_pmc_$N.log 2>&1 || { echo "pmc $C failed"; exit 1; }
  echo "pmc $C done"
done
find $OUT -name "*.csv" | head -50
