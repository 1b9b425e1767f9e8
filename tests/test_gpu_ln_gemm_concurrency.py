"""The LayerNorm-prologue GEMM (pwx_ln_kernel: 2 / 3 / 4 / 6 resident k chunks) next to a busy matrix pipe: every instantiation is launched
on one stream while a second stream saturates the MFMA pipes, and compared BIT FOR BIT with its solo result - the families and the
protocol of tests/test_gpu_concurrency.py (results must not depend on what else the chip is running)."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

N_CO = int(os.environ.get("VIP_CONCURRENCY_ITERS", "200"))


def _victims():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    g = torch.Generator().manual_seed(11)
    out = {}
    for K, N, act, res in [(128, 256, None, False), (192, 320, "gelu", False), (256, 768, None, False), (256, 768, "gelu", False),
                           (384, 1152, None, False), (384, 1536, "gelu", False), (384, 384, None, True)]:
        M = 50176 if K == 256 else 50432
        x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(torch.float16).cuda()
        cw = ops.make_dense_weight(torch.randn(K, N, generator=g) / K ** 0.5, torch.randn(N, generator=g) * 0.1)
        ln = ((torch.randn(K, generator=g) * 0.2 + 1).cuda(), (torch.randn(K, generator=g) * 0.1).cuda(), 1e-6)
        r = torch.randn(M, N, generator=g).to(torch.float16).cuda() if res else None
        assert ops.ln_gemm_fused(x, cw, act, None, r), (K, N, act, res)
        out[f"ln_gemm K{K} N{N} {act or ('res' if res else 'none')}"] = (lambda x=x, ln=ln, cw=cw, act=act, r=r:
                                                                         ops.ln_dense(x, ln, cw, act=act, residual=r))
    return out


def test_ln_gemm_is_bit_exact_next_to_a_busy_matrix_pipe(report, monkeypatch):
    monkeypatch.setenv("VIP_LN_GEMM_ALL", "1")      # every instantiation, whatever the measured dispatch policy takes by default
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    sink = torch.zeros((16,), dtype=torch.float32, device="cuda")
    flops = C.c_double(0.0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    bad = {}
    for name, fn in _victims().items():
        ref = fn().clone()
        torch.cuda.synchronize()
        n_bad, worst = 0, 0.0
        for _ in range(N_CO):
            with torch.cuda.stream(sb):      # 4 waves per SIMD of back-to-back v_mfma_f32_16x16x32_f16, nothing else
                _abi.check(lib.vip_microbench_mfma_f16(sink.data_ptr(), 300, C.byref(flops), sb.cuda_stream), "vip_microbench_mfma_f16")
            with torch.cuda.stream(sa):
                out = fn()
            torch.cuda.synchronize()
            if not torch.equal(out, ref):
                n_bad += 1
                worst = max(worst, float((out.float() - ref.float()).abs().max()))
        report(f"[concurrency] {name:30s} next to an MFMA-saturating kernel: {n_bad} of {N_CO} launches differ from the solo result"
               + (f" (max |d| {worst:.2e})" if n_bad else ""))
        if n_bad:
            bad[name] = (n_bad, worst)
    assert not bad, f"results depend on the co-running kernel: {bad}"
