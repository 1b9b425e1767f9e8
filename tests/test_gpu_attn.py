"""Every attention kernel against the fp64 reference under structured logits (tests/_attn_cases.py: S1 permutation spike, S2 common
offset +600, S3 uniform, S4 bias-dominated, S5 everything near -600, S6 other scales and non-square maps).

  vip_window_attn_fwd_f16   window_attn_kernel<7, ...> / <14, ...>, local and global query             S1 - S6
                            window_attn_pipe_kernel (VIP_ATTN_PIPE=1, experiments build)              S1, S2, S5, bit-identical to the plain kernel
  vip_gcvit_attn_block_f16  gcvit_attn_block_kernel C 64 / 2 heads, C 128 / 4 heads; the ws 14 form (experiments build); and the four
                            launches it replaces (LayerNorm + Dense, attention core, Dense + residual)  S1 (identity), S2, S3, S5, S6 maps
  vip_mhsa_fwd_f16          mhsa_kernel, N in {1, 16, 17, 33, 197, 224}                                S1, S2, S3, S5, S6 scales
  vip_window_attn_fwd_h2 / vip_mhsa_fwd_h2 (attn_h2_kernel; with VIP_ATTN_H2_MFMA=0 the fp32 VALU kernel of strict_ops.hip, in a child
  process: the switch is read once) and vip_window_attn_fwd_s32 / vip_mhsa_fwd_s32                     S1, S3, S2 / S5 at +-64

The expected-output rule of each case is `_attn_cases.judge` (the same function the CPU emulation test uses): finite; S1 on an fp16
attention core bit for bit v[pi(i)]; S3 per element 0.5 ulp16 + N 2^-23 max|v|; otherwise the tolerance of the kernel's own test (the
strict storages: 2e-5 of the output scale over every element).  One
`[attn]` line per case goes to the parity log."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _attn_cases as A  # noqa: E402

VALU = os.environ.get("VIP_ATTN_H2_MFMA") == "0"          # set for the child process of test_strict_valu_kernels_all_cases


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def _experiments():
    """the experimental kernels (VIP_BUILD_EXPERIMENTS=1 python vip-cup-2022_amd/build.py --force) are not in the default library"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    return bool(_abi.lib().vip_experiments_built())


def _no_experiments():
    return not torch.cuda.is_available() or not _experiments()


# (a string condition: evaluated in this module at set-up time, after conftest.py has skipped every gpu test on a box without a GPU)
needs_experiments = pytest.mark.skipif("_no_experiments()", reason="experimental kernel: build with VIP_BUILD_EXPERIMENTS=1")


def dev16(t):
    return None if t is None else t.to(torch.float16).cuda().contiguous()


def _verdict(report, tag, case, got, storage="f16"):
    torch.cuda.synchronize()
    got = got.float().cpu()
    assert torch.isfinite(got).all(), f"{tag} {case.name}: non-finite output"
    ok, line = A.judge(case, got, storage)
    report(f"[attn] {tag} {line}")
    assert ok, f"{tag} {line}"


def _window_f16(case, rep=1):
    i = case.inputs
    qkv, qg = i["qkv"].repeat(rep, 1, 1, 1), None if i["qg"] is None else i["qg"].repeat(rep, 1, 1)
    return _ops().window_attention(dev16(qkv), dev16(qg), i["table"].cuda(), case.heads, case.ws, case.scale)


@pytest.mark.parametrize("spec", A.WINDOW_F16, ids=A.spec_id)
def test_window_attention_cases(spec, report):
    case = A.build(spec)
    _verdict(report, "window_attn_f16", case, _window_f16(case))


@needs_experiments
@pytest.mark.parametrize("spec,rep", A.WINDOW_PIPE, ids=lambda v: A.spec_id(v) if isinstance(v, tuple) else f"x{v}")
def test_window_attention_pipelined_cases(spec, rep, report, monkeypatch):
    """window_attn_pipe_kernel: >= 1024 (window, head) items, every image block of the batch the same 4 images: each block must come out the
    same, pass the scenario's rule, and equal the one-item kernel bit for bit"""
    case = A.build(spec)
    B = case.inputs["qkv"].shape[0]
    assert B * rep * (case.q.shape[0] // B) * case.heads >= 1024 and case.ws == 14
    monkeypatch.setenv("VIP_ATTN_PIPE", "1")               # read per call by the C entry point
    got = _window_f16(case, rep)
    torch.cuda.synchronize()
    monkeypatch.setenv("VIP_ATTN_PIPE", "0")
    plain = _window_f16(case, rep)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, plain), "the pipelined kernel changes the schedule, not the arithmetic"
    blocks = got.reshape(rep, B, *got.shape[1:])
    assert torch.equal(blocks, blocks[:1].expand_as(blocks))
    _verdict(report, "window_attn_f16(pipe)", case, blocks[0])


@pytest.mark.parametrize("spec", A.MHSA_F16, ids=A.spec_id)
def test_mhsa_cases(spec, report):
    case = A.build(spec)
    _verdict(report, "mhsa_f16", case, _ops().mhsa(dev16(case.inputs["qkv"]), case.heads, case.scale))


@pytest.mark.parametrize("spec", [pytest.param(s, marks=needs_experiments) if dict(s[2])["heads"] == 8 else s for s in A.BLOCK], ids=A.spec_id)
def test_gcvit_attn_block_cases(spec, report, monkeypatch):
    """the fused block and the four launches it replaces, each against the fp64 restatement"""
    from vipcup_amd import _abi
    ops = _ops()
    case = A.build(spec)
    i, heads, ws = case.inputs, case.heads, case.ws
    C = i["x"].shape[-1]
    cq, cp = ops.make_dense_weight(i["wq"], i["bq"]), ops.make_dense_weight(i["wp"], i["bp"])
    ln = (i["gam"].cuda(), i["bet"].cuda(), 1e-5)
    args = (dev16(i["x"]), dev16(i["qg"]), ln, cq, cp, i["table"].cuda(), heads, ws, case.scale)
    assert _abi.lib().vip_gcvit_attn_block_supported(C, heads, ws) == 1
    monkeypatch.setattr(ops, "_GCVIT_BLOCK14", True)           # the ws 14 form is opt-in
    monkeypatch.setattr(ops, "_GCVIT_BLOCK_FUSED", True)
    _verdict(report, "gcvit_attn_block_f16(fused)", case, ops.gcvit_attn_block(*args))
    monkeypatch.setattr(ops, "_GCVIT_BLOCK_FUSED", False)
    _verdict(report, "gcvit_attn_block_f16(four launches)", case, ops.gcvit_attn_block(*args))


# ---- strict storages -----------------------------------------------------------------------------------------------------------
def _strict_in(t, mode):
    if t is None:
        return None
    d = t.to(torch.float32).cuda().contiguous()
    return _ops().pack_h2(d) if mode == "strict" else d


@pytest.mark.parametrize("mode", ["strict", "f32"])
@pytest.mark.parametrize("spec", A.STRICT + A.STRICT_OFFSET, ids=A.spec_id)
def test_strict_cases(spec, mode, report):
    """packed storage: attn_h2_kernel (VIP_ATTN_H2_MFMA=0: the VALU kernel); fp32 storage: the VALU kernel.  Tolerance of
    tests/test_gpu_strict.py (2e-5 of the output scale) over every designed element; whether S1 came out exact is reported"""
    ops = _ops()
    case = A.build(spec)
    i = case.inputs
    if case.kind == "window":
        got = ops.window_attention(_strict_in(i["qkv"], mode), _strict_in(i["qg"], mode), i["table"].cuda(), case.heads, case.ws, case.scale)
    else:
        got = ops.mhsa(_strict_in(i["qkv"], mode), case.heads, case.scale)
    if mode == "strict":
        got = ops.unpack_h2(got)
        ops.h2_check(case.name)
    tag = {"strict": "attn_h2(valu)" if VALU else "attn_h2(mfma)", "f32": "attn_s32"}[mode]
    _verdict(report, tag, case, got, "strict")


@pytest.mark.skipif(VALU, reason="this IS the child process")
def test_strict_valu_kernels_all_cases():
    """VIP_ATTN_H2_MFMA=0 routes the packed storage to the fp32 VALU kernels; the switch is read once per process, hence the child"""
    env = dict(os.environ, VIP_ATTN_H2_MFMA="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", "test_strict_cases and not f32",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ---- what the entry points refuse (nothing is launched: the argument checks come first) --------------------------------------------
def test_entry_points_refuse_what_they_do_not_implement():
    from vipcup_amd import _abi
    import ctypes as C
    lib = _abi.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    tab = torch.zeros(15 * 15 * 2, dtype=torch.float32, device="cuda")
    p, t, st = C.c_void_p(buf.data_ptr()), C.c_void_p(tab.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    UNSUPPORTED, BAD_ARG = -3, -1
    assert lib.vip_mhsa_fwd_f16(p, p, 1, 225, 64, 1, 0.125, st) == UNSUPPORTED           # N = 225 > 224 key rows
    assert lib.vip_mhsa_fwd_f16(p, p, 1, 16, 96, 1, 0.125, st) == UNSUPPORTED            # D != 64 * heads
    assert lib.vip_mhsa_fwd_f16(p, p, 1, 16, 128, 3, 0.125, st) == UNSUPPORTED
    assert lib.vip_window_attn_fwd_f16(p, None, t, p, 1, 8, 8, 64, 2, 8, 3, 0.2, st) == UNSUPPORTED      # ws = 8
    assert lib.vip_window_attn_fwd_f16(p, None, t, p, 1, 10, 7, 64, 2, 7, 3, 0.2, st) == BAD_ARG         # Hp % ws != 0
    assert lib.vip_window_attn_fwd_f16(p, None, t, p, 1, 14, 15, 64, 2, 14, 3, 0.2, st) == BAD_ARG       # Wp % ws != 0
    torch.cuda.synchronize()
    assert buf.abs().max().item() == 0.0
