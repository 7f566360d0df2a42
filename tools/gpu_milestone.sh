#!/bin/bash
# Milestone evidence in one call: parity tests, full bench line (roofline + cpu baseline + fp32), synthesis bench, rocprofv3
# kernel traces (side stream on = what the bench runs; off = every kernel alone on the device), PMC HBM-traffic passes and
# two PMC passes for the MFMA / LDS picture of every kernel.
TAG=${1:-r05m}
OUT=${OUT:-milestone_out}                # logs, traces and counter passes of this run (profiles/ keeps what is committed)
set -eo pipefail                         # stop at the first failed step: nothing more is started on the GPU after it
trap 'echo "gpu_milestone.sh: stopped at line $LINENO (exit $?)" >&2' ERR
export TMPDIR=/tmp
mkdir -p $OUT
# (1) HBM traffic of the contraction kernels FIRST: bench.py refuses a PMC file that was measured on other kernel sources
# (fastspeech2_amd/_lib.kernel_source_sha) and tests/test_bench_contract_gpu.py wants roofline.traffic non-null - the file of THIS
# tree has to exist under profiles/ before the suite runs (it is copied there from $OUT and committed)
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_$c
  timeout -k 10 600 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_$c -- python bench.py --steps 3 --warmup 1 --windows 1 --side-stream 0 --no-cpu-baseline --no-roofline --no-fp32 --no-synth --no-graph-line > $OUT/pmc_$c.log 2>&1
done
python tools/pmc_traffic.py $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE 6 $OUT/${TAG}_pmc_traffic.json > $OUT/${TAG}_pmc_traffic.md 2>&1
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE
cp $OUT/${TAG}_pmc_traffic.json $OUT/${TAG}_pmc_traffic.md profiles/
( time timeout -k 10 1500 python -m pytest tests -m gpu -x -q -s ) > $OUT/${TAG}_pytest.log 2>&1; grep -E "rel-Frobenius|valid-frame|ratios|passed|failed|FAILED|eager-vs|SKIPPED" $OUT/${TAG}_pytest.log | tail -16 | cut -c1-900
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench_bf16.log 2>&1; tail -1 $OUT/${TAG}_bench_bf16.log | cut -c1-2500
timeout -k 10 300 python bench.py --mode synth --full > $OUT/${TAG}_bench_synth.log 2>&1; tail -1 $OUT/${TAG}_bench_synth.log | cut -c1-1500
timeout -k 10 300 python bench.py --workload libritts --full --no-cpu-baseline --no-fp32 --no-synth > $OUT/${TAG}_bench_libritts.log 2>&1; tail -1 $OUT/${TAG}_bench_libritts.log | cut -c1-700
for side in 1 0; do
  rm -rf $OUT/prof; mkdir -p $OUT/prof
  timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/prof -o bench -- python bench.py --steps 6 --warmup 2 --windows 1 --side-stream $side --no-cpu-baseline --no-roofline --no-fp32 --no-synth --no-graph-line > $OUT/prof.log 2>&1
  DB=$(find $OUT/prof -name '*.db' | head -1)
  python tools/rocpd_summary.py $DB 10 shapes > $OUT/${TAG}_kernel_trace_side${side}.md 2>&1
done
rm -rf $OUT/prof; mkdir -p $OUT/prof
timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/prof -o bench -- python bench.py --mode synth --steps 4 --warmup 2 --no-roofline > $OUT/prof.log 2>&1
DB=$(find $OUT/prof -name '*.db' | head -1)
python tools/rocpd_summary.py $DB 6 shapes > $OUT/${TAG}_kernel_trace_synth.md 2>&1
rm -rf $OUT/prof
rm -rf $OUT/pmc_m
timeout -k 10 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_m -- python bench.py --steps 3 --warmup 1 --windows 1 --side-stream 0 --no-cpu-baseline --no-roofline --no-fp32 --no-synth --no-graph-line > $OUT/pmc_m.log 2>&1
python tools/pmc_mfma.py $OUT/pmc_m 6 > $OUT/${TAG}_pmc_mfma.md 2>&1
rm -rf $OUT/pmc_l
timeout -k 10 600 rocprofv3 --pmc SQ_INSTS_LDS SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_LDS_ADDR_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU SQ_INSTS_MFMA SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_l -- python bench.py --steps 3 --warmup 1 --windows 1 --side-stream 0 --no-cpu-baseline --no-roofline --no-fp32 --no-synth --no-graph-line > $OUT/pmc_l.log 2>&1
python tools/pmc_lds.py $OUT/pmc_l 6 > $OUT/${TAG}_pmc_lds.md 2>&1
rm -rf $OUT/pmc_m $OUT/pmc_l
head -14 $OUT/${TAG}_pmc_traffic.md; head -12 $OUT/${TAG}_pmc_mfma.md; head -12 $OUT/${TAG}_pmc_lds.md
