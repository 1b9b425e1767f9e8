"""The host-side rules of conv2d_impl / launch_pw / launch_pw_k / launch_pwk_direct / launch_pwk / gemm8p_eligible (csrc/conv_igemm.hip,
csrc/gemm8p.hpp) that pick a kernel's template arguments and tile grid, restated once for both fp16 storages under DEFAULT dispatch (no
environment switch).  `halfs` is the number of fp16 values per logical input channel: 1 for the fp16 storage, 2 for the packed strict
storage (conv_h2.hip = conv_igemm.hip with VIP_GEMM_H2), where a.K, a.ldx and a.Cin_g count halfs and every K threshold therefore
applies to 2 K.

The dispatcher's dry run (ops.conv_kernel_name / conv_kernel_name_h2) names the KERNEL; the instantiation is finer than the name, and this
restatement is the oracle for it: tests/_h2_gemm_cases.py and tests/_f16_gemm_cases.py hold every row's `variant` string against these
functions, tests/test_h2_dispatch_cpu.py and tests/test_f16_dispatch_cpu.py hold the kernel name of the same row against the dry run.  A
change of the C rules fails those tests: re-derive the shapes then, never the expected kernel."""
import re


def cdiv(a, b):
    return (a + b - 1) // b


def pointwise_mode(act, post, has_res):
    """does a pointwise kernel carry this epilogue?  (activation alone) or (residual [+ ReLU]); anything else - an activation AND a
    residual, a post-activation other than ReLU - is left to conv_igemm_kernel"""
    if not has_res and not post:
        return True
    return bool(has_res and not act and post in (None, "relu"))


def conv_variant_of(M, k_taps, cin_g, cout_g, halfs=1, mode_ok=True, gated=False):
    """the k x k path of conv2d_impl: im2col staging of the pointwise tile kernel for stems and for maps of >= 32 K pixels, else the
    tile kernel, whose first argument follows short_k (a.K <= 256 halfs) and the second the group's channel count"""
    if (cin_g <= 16 or M >= 32768) and mode_ok and not gated:
        return f"im2col<{1 if cout_g <= 64 else 2}>"
    return f"conv_igemm<{64 if halfs * k_taps * cin_g <= 256 else 128},{64 if cout_g <= 64 else 128}>"


def dense_variant(M, K, N, has_res=False, halfs=1, gated=False, act=None, post=None, hilo=False):
    """the instantiation and tile grid a 1 x 1 stride-1 ungrouped launch [M, K] x [K, N] reaches, in logical K"""
    ka = halfs * K                                                # a.K
    mode_ok = pointwise_mode(act, post, has_res)
    if hilo or (mode_ok and ka <= 256 and M >= 65536 and not gated):     # launch_pw_k / launch_pw
        ks = 2 * cdiv(ka, 64) if halfs == 2 else cdiv(ka, 32)    # the k-step template: {1, 2, 3, 4, 6, 8}
        ks = ks if ks <= 4 else 6 if ks <= 6 else 8
        s16 = ks * 4 * (2 if hilo else 1)                         # LDS row stride in 16-byte chunks, 2 (mod 4)
        while s16 & 3 != 2:
            s16 += 1
        lds = (156 if halfs == 2 and M >= 1 << 19 else 72) * 1024
        max_rows = (lds // (s16 * 16 + 4)) & ~63
        cout64 = cdiv(N, 64) * 64
        chunks = cdiv(cout64, max_rows)
        return f"pw_gemm<KS={ks}{',hilo' if hilo else ''}> {chunks} x {cdiv(cout64 // 64, chunks) * 64}"
    if M <= 256 and not has_res and not gated and not post:
        return "rows_gemm"
    if not mode_ok:
        return conv_variant_of(M, 1, K, N, halfs, False, gated)
    mt = cdiv(M, 256)
    if not gated and ka >= 1024 and ka % 64 == 0 and N % 256 == 0 and mt * (N // 256) >= 128:
        return f"gemm8p<{'pipe' if ka % 128 == 0 else 'basic'}> {mt} x {N // 256}"
    if ka < 768 or gated:                                         # launch_pwk_direct
        ng = 1 if N <= 64 else 2
        return f"pwk_direct<{ng}{',gated' if gated else ''}> PT={1 if mt * cdiv(N, 64 * ng) < 256 else 4}"
    if N <= 64:
        return f"pwk_gemm<1,1> {mt} x 1"
    if N % 256 == 0 and ka >= 1024 and mt * (N // 256) >= 256:
        return f"pwk_gemm<2,2> {mt} x {N // 256}"
    return f"pwk_gemm<2,1> {mt} x {cdiv(N, 128)}"


def case_variant(case, halfs=1, gated=False):
    """the same for a CONV_CASES tuple (B, H, W, Cin, Cout, k, stride, pad(t,b,l,r), groups, act, residual): the pointwise rules for a
    1 x 1 stride-1 unpadded ungrouped one, the k x k rules for the rest"""
    B, H, W, Cin, Cout, k, s, pad, groups, act, use_res = case
    Ho, Wo = (H + pad[0] + pad[1] - k) // s + 1, (W + pad[2] + pad[3] - k) // s + 1
    if k == 1 and s == 1 and groups == 1 and tuple(pad) == (0, 0, 0, 0):
        return dense_variant(B * Ho * Wo, Cin, Cout, use_res, halfs, gated, act)
    return conv_variant_of(B * Ho * Wo, k * k, Cin // groups, Cout // groups, halfs, pointwise_mode(act, None, use_res), gated)


KERNEL_OF = {"rows_gemm": "rows_gemm_kernel", "pw_gemm": "pw_gemm_kernel", "gemm8p": "gemm8p_kernel", "pwk_direct": "pwk_direct_kernel",
             "pwk_gemm": "pwk_gemm_kernel", "im2col": "pwk_gemm_kernel(im2col)", "conv_igemm": "conv_igemm_kernel"}


def kernel_of(variant):
    """the dry run's name for a variant string"""
    return KERNEL_OF[variant.split("<")[0].split(" ")[0]]


def instantiation(variant):
    """a variant string without its tile grid: 'pwk_gemm<2,2> 65 x 4' -> 'pwk_gemm<2,2>'; 'pwk_direct<2> PT=4' stays (PT is a template
    argument)"""
    return re.sub(r" \d+ x \d+$", "", variant)
