"""usage: python tools/swin_fp64_worst.py <per-row log> [<out>]   (default out: profiles/swin_attn_fp64.log)

Reduces what tests/test_gpu_swin_attn.py appends to VIP_SWIN_FP64_LOG - one line per row and storage,
`<family> <storage>: max_abs_err <e> = <share> of its bound` - to the worst row of every (family, storage)."""
import collections
import re
import sys

src = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/swin_attn_fp64.log"
worst, count = collections.OrderedDict(), collections.Counter()
for line in open(src):
    m = re.match(r"(\S+) (\S+): max_abs_err (\S+) = (\S+) of its bound", line)
    if not m:
        continue
    key, val = (m.group(1), m.group(2)), (float(m.group(4)), float(m.group(3)))
    count[key] += 1
    if key not in worst or val > worst[key]:
        worst[key] = val
lines = ["tests/test_gpu_swin_attn.py on an MI355X with VIP_SWIN_FP64_LOG set, reduced by tools/swin_fp64_worst.py to the worst row of every",
         "(row family, storage): error against tests/_swin_v2_ref.py in float64.  Families and bounds: tests/_swin_cases.py (E1 - E5: scenario S3's",
         "0.5 ulp16 + N 2^-23 max|v|, torch.equal held besides on f16 / h2 where the top set has a power-of-two size; b10 / bsmallq / beps / member:",
         "TOL_F16 on f16, TOL_OP on h2 / s32; b100: (exp(2 tau 2^-10) - 1) max|v| + 1 ulp16 on f16, TOL_OP on h2 / s32)."]
for (fam, st), (share, err) in worst.items():
    lines.append(f"{fam:8s} {st:3s}: {count[(fam, st)]:3d} rows, worst max_abs_err {err:.3e} = {share:.3f} of its bound")
open(out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
