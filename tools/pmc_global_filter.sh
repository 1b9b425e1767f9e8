#!/bin/bash
# PMC of one shape of the global-local filter:  tools/pmc_global_filter.sh H W S kind tag   -> $PMC_OUT/<tag>.txt (default pmc_out/gf)
# Counters in separate passes (no tracing flags beside --pmc); a failed pass ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
H=$1; W=$2; S=$3; KIND=$4; TAG=$5
OUT=${PMC_OUT:-pmc_out/gf}
mkdir -p $OUT
timeout -k 10 120 python3 tools/global_filter_one.py $H $W $S $KIND 3 > $OUT/$TAG.txt 2>&1 || exit 1
i=0
for set in "SQ_BUSY_CYCLES SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VALU SQ_INSTS_LDS" \
           "SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT" "SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INST_CYCLES_VMEM_RD"; do
  timeout -k 10 180 rocprofv3 --pmc $set --output-format csv -d $OUT/p_$i -- python3 tools/global_filter_one.py $H $W $S $KIND 3 > /dev/null 2> $OUT/p_$i.err || { tail -5 $OUT/p_$i.err; exit 1; }
  python3 tools/pmc_parse.py $OUT/p_$i global_local_filter >> $OUT/$TAG.txt 2>&1
  rm -rf $OUT/p_$i
  i=$((i+1))
done
grep -v "^void\|^_ZN" $OUT/$TAG.txt
