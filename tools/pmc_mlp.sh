#!/bin/bash
# PMC of one fused-MLP launch (hidden = 4 C, LayerNorm prologue, residual):  tools/pmc_mlp.sh M C tag   -> $PMC_OUT/<tag>.txt (default pmc_out/mlp)
# VIP_LIB_PATH selects the build.  Counters in separate passes (no tracing flags beside --pmc); a failed pass ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
M=$1; C=$2; TAG=$3
OUT=${PMC_OUT:-pmc_out/mlp}
mkdir -p $OUT
timeout -k 10 120 python3 tools/bench_mlp_one.py $M $C 3 > $OUT/$TAG.txt 2>&1 || exit 1
i=0
for set in "SQ_BUSY_CYCLES SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY" "SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS" \
           "SQ_VALU_MFMA_BUSY_CYCLES SQ_VALU_MFMA_COEXEC_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA" "SQ_ACTIVE_INST_LDS SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INST_CYCLES_VMEM_RD"; do
  timeout -k 10 180 rocprofv3 --pmc $set --output-format csv -d $OUT/p_$i -- python3 tools/bench_mlp_one.py $M $C 3 > /dev/null 2> $OUT/p_$i.err || { tail -5 $OUT/p_$i.err; exit 1; }
  python3 tools/pmc_parse.py $OUT/p_$i mlp_ >> $OUT/$TAG.txt 2>&1
  rm -rf $OUT/p_$i
  i=$((i+1))
done
grep -v "^void\|^_ZN" $OUT/$TAG.txt
