#!/bin/bash
# Round-4 measurement pass on the GPU box (everything lands in gpurun_out/, copied to profiles/ afterwards): environment probe, full
# GPU test suite, smoke, separate --pmc passes (FETCH_SIZE / WRITE_SIZE: trunk convolutions at 256^2 and 224^2, stain kernels at the
# headline size, Vahadane statistics, HoVer-Net post-processing, canvas kernels), the default bench (+cpu_baseline), rocprofv3
# kernel trace of the bench, per-layer / per-kernel tables, the other bench configurations.
#   usage: final_profile_r04.sh TAG [skip_tests]
set -u
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$R/gpurun_out
TAG=${1:-r04p}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
cd $R
python scripts/probe_env.py > $OUT/${TAG}_env_probe.txt 2>&1
if [ "${2:-}" != "skip_tests" ]; then
  timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -5 > $OUT/${TAG}_pytest_gpu.log; cat $OUT/${TAG}_pytest_gpu.log
  timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/${TAG}_smoke.log 2>&1; echo "smoke rc=$?"
fi
pmc() {  # pmc STEM COMMAND...: one pass per counter, summaries named ${TAG}_${STEM}_pmc_${COUNTER}.txt
  local stem=$1; shift
  for c in FETCH_SIZE WRITE_SIZE; do
    rm -rf /tmp/rp_$stem$c; (cd /tmp && timeout 400 rocprofv3 --kernel-trace --pmc $c --output-format csv -d /tmp/rp_$stem$c -- "$@" > /dev/null 2>&1)
    python $R/scripts/prof_summarize.py /tmp/rp_$stem$c $OUT/${TAG}_${stem}_pmc_${c}.txt > /dev/null
  done
}
pmc trunk python $R/scripts/perf_trunk.py 1024 256
pmc trunk224 python $R/scripts/perf_trunk.py 1024 224
pmc stain python $R/scripts/perf_stain.py 4096 256
pmc vahadane python $R/scripts/pmc_workloads.py vahadane 2
pmc hover python $R/scripts/pmc_workloads.py hover 3
pmc canvas python $R/scripts/pmc_workloads.py canvas 3
grep -h "conv3x3\|conv_mfma\|stem7x7" $OUT/${TAG}_trunk_pmc_*.txt | cut -c1-120
# the benches read the traffic of their kernels from profiles/: make this pass visible to the runs below
cp $OUT/${TAG}_*_pmc_*.txt $R/profiles/ 2>/dev/null
cd $R
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?"; cut -c1-400 $OUT/${TAG}_bench.json
(cd /tmp && rm -rf /tmp/rp_bench; timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_bench -- \
    python $R/bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-extras > $OUT/${TAG}_bench_under_rocprof.json 2> /dev/null)
python $R/scripts/prof_summarize.py /tmp/rp_bench $OUT/${TAG}_bench_rocprofv3_summary.txt > /dev/null; head -14 $OUT/${TAG}_bench_rocprofv3_summary.txt | cut -c1-150
timeout 300 python scripts/perf_trunk.py 1024 256 2>&1 | grep -v "amdgpu\|No local" > $OUT/${TAG}_perf_trunk.txt
timeout 300 python scripts/perf_trunk.py 1024 224 2>&1 | grep -v "amdgpu\|No local" >> $OUT/${TAG}_perf_trunk.txt; cat $OUT/${TAG}_perf_trunk.txt
timeout 300 python scripts/perf_conv.py 1024 224 2>&1 | grep -v "amdgpu\|No local" > $OUT/${TAG}_perf_conv224.txt; tail -1 $OUT/${TAG}_perf_conv224.txt
timeout 400 python scripts/perf_stain.py 4096 256 2>&1 | grep -v amdgpu > $OUT/${TAG}_perf_stain.txt; grep "^stats\|^apply" $OUT/${TAG}_perf_stain.txt
timeout 300 python scripts/perf_vahadane.py 2048 256 2>&1 | grep vahadane > $OUT/${TAG}_perf_vahadane.txt; cat $OUT/${TAG}_perf_vahadane.txt
timeout 300 python scripts/perf_hovernet_layers.py hovernet 32 2>&1 | grep -v "amdgpu\|No local" > $OUT/${TAG}_hovernet_layers.txt; head -1 $OUT/${TAG}_hovernet_layers.txt
timeout 300 python scripts/perf_hovernet_layers.py unet 8 2>&1 | grep -v "amdgpu\|No local" > $OUT/${TAG}_unet_layers.txt; head -1 $OUT/${TAG}_unet_layers.txt
timeout 600 python bench.py --config hovernet --steps 5 --warmup 2 > $OUT/${TAG}_bench_hovernet.json 2> /dev/null; cut -c1-200 $OUT/${TAG}_bench_hovernet.json
timeout 600 python bench.py --config vahadane --steps 5 --warmup 2 > $OUT/${TAG}_bench_vahadane.json 2> /dev/null; cut -c1-200 $OUT/${TAG}_bench_vahadane.json
timeout 600 python bench.py --config semantic --steps 1 --warmup 1 > $OUT/${TAG}_bench_semantic.json 2> /dev/null; cut -c1-200 $OUT/${TAG}_bench_semantic.json
ls $OUT | grep $TAG | wc -l
