"""LayerNorm folded into its GEMM (ops.ln_dense -> vip_ln_gemm_bias_act_f16, pwx_ln_kernel) against the two launches it replaces
(layernorm_kernel + the GEMM ops.dense picks) on the ensemble's LayerNorm -> Dense call sites with M >= 16384 and K <= 384:

    ViT-S/16      norm1 -> qkv  50432 x 384 x 1152        norm2 -> fc1  50432 x 384 x 1536 gelu
    ConvNeXt-T    stage 2 norm -> fc1  147456 x 384 x 1536 gelu
    GCViT-T       level 1 norm2 -> fc1 200704 x 128 x 384 gelu      (mlp_ratio 3)
                  level 2 norm1 -> qkv 50176 x 256 x 768, with a global query 50176 x 256 x 512;  norm2 -> fc1 50176 x 256 x 768 gelu

Runs with VIP_LN_GEMM_ALL=1, so EVERY site goes through the fused kernel whatever vip_ln_gemm_supported's policy says (the column
'policy' shows what the library does without it).  Per site: one discarded and ROUNDS kept rounds of (layernorm, dense, fused), each the mean of 30 launches
timed with HIP events after 5 warm-up launches; a side's spread over the rounds is printed as min..max, and the fused launch counts
as a gain only when its slowest round beats the fastest round of the two launches."""
import os, sys, torch
os.environ["VIP_LN_GEMM_ALL"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vipcup_amd  # noqa
from vipcup_amd import _abi, ops
ROUNDS = 8          # after one discarded round (clocks and caches settle)
SITES = [("ViT-S qkv", 50432, 384, 1152, None), ("ViT-S fc1", 50432, 384, 1536, "gelu"), ("ConvNeXt-T s2 fc1", 147456, 384, 1536, "gelu"),
         ("GCViT-T l1 fc1", 200704, 128, 384, "gelu"), ("GCViT-T l2 qkv", 50176, 256, 768, None), ("GCViT-T l2 qkv gq", 50176, 256, 512, None),
         ("GCViT-T l2 fc1", 50176, 256, 768, "gelu")]


def timed(fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(30):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 30 * 1e3


for name, M, K, N, act in SITES:
    x = (torch.randn((M, K)) * 1.5 + 0.3).to(torch.float16).cuda()
    cw = ops.make_dense_weight(torch.randn(K, N) / K ** 0.5, torch.randn(N) * 0.1)
    ln = ((torch.randn(K) * 0.2 + 1).cuda(), (torch.randn(K) * 0.1).cuda(), 1e-6)
    assert ops.ln_gemm_fused(x, cw, act)
    del os.environ["VIP_LN_GEMM_ALL"]
    policy = "fused" if _abi.lib().vip_ln_gemm_supported(M, K, N, {None: 0, "gelu": 3}[act]) else "two"
    os.environ["VIP_LN_GEMM_ALL"] = "1"
    xn = ops.layernorm(x, ln[0], ln[1], ln[2])
    two, fus, lnt = [], [], []
    for r in range(ROUNDS + 1):
        a = timed(lambda: ops.layernorm(x, ln[0], ln[1], ln[2]))
        b = timed(lambda: ops.dense(xn, cw, act=act))
        c = timed(lambda: ops.ln_dense(x, ln, cw, act=act))
        if r:
            lnt.append(a); two.append(a + b); fus.append(c)
    verdict = "GAIN" if max(fus) < min(two) else ("LOSS" if min(fus) > max(two) else "inside the spread")
    print(f"{name:18s} M={M:6d} K={K} N={N:4d} act={str(act):4s} policy={policy:5s}: layernorm {min(lnt):5.1f}..{max(lnt):5.1f}, two launches "
          f"{min(two):6.1f}..{max(two):6.1f} us | fused {min(fus):6.1f}..{max(fus):6.1f} us -> {verdict}")
