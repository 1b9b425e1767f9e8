#!/bin/bash
# PMC of the fp16 swin attention kernel on one stack of the 200 pixel tiny member:  tools/pmc_swin_attn.sh MAP tag  -> $PMC_OUT/<tag>.txt
# (default pmc_out/swin).  Counters in separate passes (no tracing flags beside --pmc); a failed pass ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
MAP=$1; TAG=$2
OUT=${PMC_OUT:-pmc_out/swin}
mkdir -p $OUT
: > $OUT/$TAG.txt
i=0
for set in "SQ_BUSY_CYCLES SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VALU SQ_INSTS_LDS" \
           "SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT" "SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INST_CYCLES_VMEM_RD"; do
  timeout -k 10 180 rocprofv3 --pmc $set --output-format csv -d $OUT/p_$i -- python3 tools/bench_swin_attn.py --one $MAP > /dev/null 2> $OUT/p_$i.err || { tail -5 $OUT/p_$i.err; exit 1; }
  python3 tools/pmc_parse.py $OUT/p_$i swin_attn_kernel >> $OUT/$TAG.txt 2>&1
  rm -rf $OUT/p_$i
  i=$((i+1))
done
cat $OUT/$TAG.txt
