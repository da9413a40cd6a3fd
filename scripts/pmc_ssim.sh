#!/bin/bash
# Counter passes + a kernel trace over vcf_ssim_u8 (scripts/bench_ssim.py --once: 8 pairs of 4K RGB frames):
#   scripts/pmc_ssim.sh -> $OUT/{summary.json,kernel_stats.csv} (OUT defaults to bench_out/pmc_ssim)
# Every pass is a run of its own; counters are never combined with tracing.
set -u
cd "$(dirname "$0")/.."
ROOT=$(pwd); OUT=${OUT:-$ROOT/bench_out/pmc_ssim}; RAW=/tmp/pmc_ssim
rm -rf "$OUT" "$RAW"; mkdir -p "$OUT" "$RAW"; export TMPDIR=/tmp; cd /tmp   # raw counters stay in /tmp
timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d "$RAW/trace" -o run \
    -- python3 "$ROOT/scripts/bench_ssim.py" --once 10 > "$OUT/trace.log" 2>&1
rc=$?; echo "trace rc=$rc"; case $rc in 0) ;; *) exit $rc;; esac
find "$RAW/trace" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats.csv" \;
i=0
for grp in "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE" \
           "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_SALU SQ_BUSY_CYCLES" \
           "SQ_INSTS_VMEM_RD SQ_WAVES SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_FMA_F64 GRBM_GUI_ACTIVE" \
           "FETCH_SIZE"; do
  i=$((i+1))
  timeout -k 10 -s KILL 90 rocprofv3 --pmc $grp --output-format csv -d "$RAW/p$i" -o pmc \
      -- python3 "$ROOT/scripts/bench_ssim.py" --once 2 > "$OUT/p$i.log" 2>&1
  rc=$?; echo "pass $i rc=$rc"
  case $rc in 0) ;; *) exit $rc;; esac
done
python3 "$ROOT/scripts/pmc_kernels.py" "$RAW" "ssim" > "$OUT/summary.json"
cat "$OUT/summary.json"
