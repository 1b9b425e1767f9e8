"""One shape of ops.global_local_filter, launched n times (for counter collection):  python tools/global_filter_one.py H W S f16|h2|s32 [n] [B]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
import vipcup_amd  # noqa: E402,F401
from vipcup_amd import ops  # noqa: E402

H, W, S, kind = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
n = int(sys.argv[5]) if len(sys.argv) > 5 else 3
B = int(sys.argv[6]) if len(sys.argv) > 6 else 256
g = torch.Generator().manual_seed(0)
x = torch.randn(B, H, W, S, generator=g).cuda()
x = {"f16": lambda t: t.half(), "h2": ops.pack_h2, "s32": lambda t: t}[kind](x)
w3 = (torch.randn(3, 3, S // 2, generator=g) / 3).cuda()
gd = ops.make_global_filter_weight(torch.randn(2, H, W // 2 + 1, S // 2, generator=g), H, W)
for _ in range(n):
    y = ops.global_local_filter(x, w3, gd)
torch.cuda.synchronize()
print(f"global_local_filter [{B},{H},{W},{S}] {kind} x {n}: {ops.global_filter_plan(H, W, S)}")
