"""A/B of the fused MLP kernels at the three production shapes of the flagship step (batch 256), LayerNorm prologue and residual on:
    python tools/bench_mlp_slices.py [--other OTHER_LIB.so]... [--rounds 8] [--launches 20] [--warm 100]
The library under test ("this") is the one vipcup_amd loads (VIP_LIB_PATH or the in-tree build); each --other names another build of
libvipcup_hip.so (the parent commit's, say; a side is called by its file name), loaded beside it.  All run in ONE process on the same
operands, round by round (other, this, other, this, ...), so clocks and cache state are shared; per round the mean of `launches`
back-to-back launches between two events.  Prints every round, then median / min / max per side, and for every other build whether
the outputs are bit-identical and whether the slowest round of this build beat its fastest round."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vipcup_amd  # noqa: E402,F401
from vipcup_amd import _abi, ops  # noqa: E402

# ConvNeXt-T stage 1, ConvNeXt-T stage 0, GCViT level 0
SHAPES = [(589824, 192, 768), (2359296, 96, 384), (802816, 64, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", action="append", default=[])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warm", type=int, default=100, help="untimed launches per side and shape (clocks settle over the first ~50 ms)")
    a = ap.parse_args()
    sides = [("this", _abi.lib().vip_mlp_fused_f16)]
    for path in reversed(a.other):
        other = C.CDLL(os.path.abspath(path)).vip_mlp_fused_f16
        other.restype, other.argtypes = _abi.SIGNATURES["vip_mlp_fused_f16"]
        sides.insert(0, (os.path.splitext(os.path.basename(path))[0], other))
    g = torch.Generator().manual_seed(7)
    for M, Cc, hid in SHAPES:
        x = (torch.rand((M, Cc), generator=g) * 4 - 2).to(torch.float16).cuda()
        fc1 = ops.make_dense_weight(torch.randn((Cc, hid), generator=g) / math.sqrt(Cc), torch.randn(hid, generator=g) * 0.5)
        fc2 = ops.make_dense_weight(torch.randn((hid, Cc), generator=g) / math.sqrt(hid), torch.randn(Cc, generator=g) * 0.5)
        lg, lb = (1 + 0.3 * torch.randn(Cc, generator=g)).cuda(), (0.2 * torch.randn(Cc, generator=g)).cuda()
        outs = {n: torch.empty_like(x) for n, _ in sides}
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def launch(name, fn):
            st = fn(p(x), p(lg), p(lb), 1e-6, p(fc1.w), p(fc1.bias), p(fc2.w), p(fc2.bias), p(x), p(outs[name]), M, Cc, hid, Cc,
                    fc1.ldw, fc2.ldw, Cc, Cc, ops._act("gelu"), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert st == 0, (name, st)

        for n, fn in sides:
            for _ in range(a.warm):
                launch(n, fn)
        torch.cuda.synchronize()
        t = {n: [] for n, _ in sides}
        for r in range(a.rounds):
            for n, fn in sides:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    launch(n, fn)
                e1.record()
                torch.cuda.synchronize()
                t[n].append(e0.elapsed_time(e1) / a.launches * 1e3)
            print(f"M={M} C={Cc} hidden={hid} round {r + 1}: " + "  ".join(f"{n} {t[n][-1]:8.1f} us" for n, _ in sides), flush=True)
        for n, _ in sides:
            v = t[n]
            print(f"M={M} C={Cc} hidden={hid} {n}: median {statistics.median(v):8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  "
                  f"({4.0 * M * Cc * hid / statistics.median(v) / 1e6:6.1f} TF)")
        for n, _ in sides[:-1]:
            same = torch.equal(outs["this"].view(torch.int16), outs[n].view(torch.int16))
            print(f"M={M} C={Cc} hidden={hid} this vs {n}: outputs bit-identical: {same}; slowest this {max(t['this']):.1f} us < fastest "
                  f"{n} {min(t[n]):.1f} us: {max(t['this']) < min(t[n])}")


if __name__ == "__main__":
    main()
