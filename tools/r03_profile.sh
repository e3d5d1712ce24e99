#!/bin/bash
# Round-3 evidence run (on the GPU box, from the repo root), everything from the binary as committed: GPU parity tests,
# the default bench line, rocprofv3 kernel-trace statistics of the same command, PMC passes (one counter group per pass,
# kernel trace only), phase table. Output: gpurun_out/r03f/ -> copied to profiles/r03_final_* by tools/r03_collect.py.
set -u
export TMPDIR=/tmp
out=gpurun_out/r03f
mkdir -p $out
if [ "${SKIP_TESTS:-0}" != 1 ]; then
  timeout 1500 python -m pytest tests -m gpu -x -q > $out/pytest_gpu.log 2>&1
  tail -4 $out/pytest_gpu.log
fi
timeout 900 python bench.py --full > $out/bench.json 2> $out/bench.log
tail -1 $out/bench.json | cut -c1-300
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats.d -o stats -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-shard --no-peaky --no-extras > $out/stats.log 2>&1
find $out/stats.d -name '*kernel_stats.csv' -exec cp {} $out/kernel_stats_4096.csv \;
rm -rf $out/stats.d
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats.d -o stats -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-shard --no-peaky --no-extras --batch 512 > $out/stats512.log 2>&1
find $out/stats.d -name '*kernel_stats.csv' -exec cp {} $out/kernel_stats_512.csv \;
rm -rf $out/stats.d
timeout 600 bash tools/pmc_run.sh $out fetch_4096 "FETCH_SIZE" --no-shard --no-peaky --no-extras
timeout 600 bash tools/pmc_run.sh $out write_4096 "WRITE_SIZE" --no-shard --no-peaky --no-extras
timeout 600 bash tools/pmc_run.sh $out sq1_4096 "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR" --no-shard --no-peaky --no-extras
timeout 600 bash tools/pmc_run.sh $out sq2_4096 "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_VMEM SQ_LDS_BANK_CONFLICT SQ_INST_CYCLES_VMEM" --no-shard --no-peaky --no-extras
CTCDEC_BEAM_KERNEL=wave timeout 300 python bench.py --batch 512 --phases --no-shard --no-peaky --no-cpu-baseline --no-extras --steps 3 > $out/phases512.json 2> $out/phases512.log
grep "phase ticks" $out/phases512.log
ls -la $out
