"""The GEMM and k x k convolution kernels of the three storages against exact fp64 references (tests/_gemm_exact_cases.py): one launch
per row through ops.dense / ops.conv2d (the C entry point itself on the slice rows), torch.equal with the ONE documented rounding of
post(act(x . W + b) + r) - both planes on the packed storage -, the dispatcher picks the kernel the row names, inputs and residual are
unchanged, and on slice rows every element outside the slice still holds the sentinel.  No tolerance: a failing row is a finding about
the kernel.  tests/test_gemm_exact_cases_cpu.py holds the table (condition EXACT, dispatch, mutants) without a GPU."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _f16_gemm_cases as F16  # noqa: E402
from tests import _gemm_exact_cases as T  # noqa: E402

_times = {}


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def to_storage(ops, t, storage):
    """a host fp64 tensor -> the activation storage on the device"""
    if storage == "f16":
        return t.to(torch.float16).cuda().contiguous()
    d = t.to(torch.float32).cuda().contiguous()
    return ops.pack_h2(d) if storage == "h2" else d


def planes(ops, t, storage):
    """a device tensor of the storage -> the host fp64 value planes it holds: (v,) or (hi, lo)"""
    if storage == "h2":
        return T.planes_of_packed(t.cpu())
    return (t.cpu().double(),)


def first_and_worst(row, got, exp):
    """row, 256-row tile, channel, got and expected of the first and of the worst differing element, and their count"""
    g, e = got.reshape(-1, got.shape[-1]), exp.reshape(-1, exp.shape[-1])
    bad = (g != e) | torch.isnan(g)
    n = int(bad.sum())
    if not n:
        return None
    idx = bad.reshape(-1).nonzero()[:, 0]
    err = torch.where(bad, (g - e).abs().nan_to_num(float("inf"), float("inf"), float("inf")), torch.zeros_like(g)).reshape(-1)

    def at(i):
        r, c = divmod(int(i), g.shape[1])
        return f"row {r} (256-row tile {r // 256}) channel {c}: got {g[r, c].item()!r} expected {e[r, c].item()!r}"
    return f"{row.id}: {n} of {g.numel()} elements differ; first {at(idx[0])}; worst {at(err.argmax())}"


def launch_direct(ops, row, xd, cw, rd, out, d):
    """the C entry point of the storage with the descriptor as given (res_off is not reachable through ops.conv2d)"""
    tail = (ops._p(cw.bias), ops._p(rd), ops._p(out), C.byref(d))
    if row.storage == "f16":
        ops._launch("vip_conv2d_nhwc_f16", ops._p(xd), ops._p(cw.w), *tail)
    elif row.storage == "h2":
        ops._launch("vip_conv2d_nhwc_h2", ops._p(xd), ops._p(cw.w), *tail, 1.0 / cw.h2_scale, status=True)
    else:
        ops._launch("vip_conv2d_nhwc_s32x", ops._p(xd), ops._p(cw.w_bf3), cw.w_bf3.shape[2], *tail)


def kernel_of(ops, row, cw, d, has_res):
    if row.storage == "f16":
        return ops.conv_kernel_name(d, has_res, row.gated, cw.w_lo is not None)
    if row.storage == "h2":
        return ops.conv_kernel_name_h2(d, has_res)
    split = ops.STRICT_GEMM in ("bf16x3", "bf16x2") and cw.w_bf3 is not None          # ops._conv2d_s32's own rule
    return "sconv6_kernel" if split else "sconv_kernel"


@pytest.mark.parametrize("row", T.ROWS, ids=T.IDS)
def test_gemm_exact(row, report, monkeypatch):
    ops = _ops()
    t0 = time.perf_counter()
    if row.storage == "s32":
        monkeypatch.setattr(ops, "STRICT_GEMM", row.variant)
    B, H, W, Cin, Cout, k, s, pad, groups = row.case
    act, post, has_res = T.EPI[row.epi]
    op = T.operands(row)
    exp = T.expected(row, T.ref64(row, op))
    exp = tuple(e.double() for e in exp) if row.storage == "h2" else (exp.double(),)
    with ops.precision(T.MODE[row.storage]):
        cw = ops.make_conv_weight(op["w"].float(), op["b"].float(), groups=groups, hilo=row.hilo)
    assert cw.kind == row.storage and (cw.w_lo is not None) == row.hilo
    x, r = op["x"], (op["r"] if has_res else None)
    gd = None if op["gate"] is None else op["gate"].to(torch.float16).cuda().contiguous()
    d, _ = F16.conv_desc(row.case + (act, has_res), cw.ldw)
    d.act_post = ops._act(post)
    Ho, Wo = T.out_hw(row.case)
    if row.slice is None:
        assert kernel_of(ops, row, cw, d, has_res) == row.kernel, row.what
        xd, rd = to_storage(ops, x, row.storage), (None if r is None else to_storage(ops, r, row.storage))
        x0, r0 = xd.clone(), (None if rd is None else rd.clone())
        if T.is_dense(row):
            got = ops.dense(xd.reshape(B, Cin), cw, act=act, act_post=post, residual=None if rd is None else rd.reshape(B, Cout))
        else:
            got = ops.conv2d(xd, cw, stride=s, pad=pad, act=act, act_post=post, residual=rd, gate=gd)
        torch.cuda.synchronize()
        if row.storage == "h2":
            ops.h2_check(row.id)
        got = got.reshape(B, Ho, Wo, Cout)
        outside = None
    else:
        name, ld, off = row.slice
        wide_x = torch.full((B, H, W, ld if name == "ldx" else Cin), 1000.0, dtype=torch.float64)    # the neighbours would show in any sum
        wide_r = torch.full((B, Ho, Wo, ld if name == "ldr" else Cout), 1000.0, dtype=torch.float64)
        xo, ro, yo = (off if name == "ldx" else 0), (off if name == "ldr" else 0), (off if name == "ldy" else 0)
        wide_x[..., xo:xo + Cin] = x
        if r is not None:
            wide_r[..., ro:ro + Cout] = r
        xd, rd = to_storage(ops, wide_x, row.storage), (None if r is None else to_storage(ops, wide_r, row.storage))
        x0, r0 = xd.clone(), (None if rd is None else rd.clone())
        out = to_storage(ops, torch.full((B, Ho, Wo, ld if name == "ldy" else Cout), T.SENTINEL, dtype=torch.float64), row.storage)
        d.ldx, d.cin_off, d.ldy, d.cout_off = wide_x.shape[3], xo, out.shape[3], yo
        d.ldr, d.res_off = (wide_r.shape[3] if r is not None else 0), ro
        assert kernel_of(ops, row, cw, d, has_res) == row.kernel, row.what
        assert (name == "ldr") <= has_res
        launch_direct(ops, row, xd, cw, rd, out, d)
        torch.cuda.synchronize()
        if row.storage == "h2":
            ops.h2_check(row.id)
        got = out[..., yo:yo + Cout]
        outside = torch.cat([out[..., :yo], out[..., yo + Cout:]], 3)
    gp = planes(ops, got.contiguous(), row.storage)
    msgs = [first_and_worst(row, g, e) for g, e in zip(gp, exp)]
    bad = [f"{'hi lo'.split()[i] if len(gp) == 2 else 'value'} plane: {m}" for i, m in enumerate(msgs) if m]
    dt = time.perf_counter() - t0
    _times[row.id] = dt
    report(f"[gemm-exact] {row.id} {row.kernel} {row.variant}: {'EXACT' if not bad else 'DIFFERS'} ({got.numel()} elements, {dt:.2f} s)")
    for m in bad:
        report(f"[gemm-exact]   {m}")
    assert not bad, "\n".join(bad)
    assert all(torch.equal(g, e) for g, e in zip(gp, exp))
    assert torch.equal(xd, x0) and (rd is None or torch.equal(rd, r0)), "the launch wrote to its input or residual"
    if outside is not None:
        assert outside.numel() == (0 if row.slice[0] != "ldy" else B * Ho * Wo * (row.slice[1] - Cout))
        for p, want in zip(planes(ops, outside.contiguous(), row.storage) if outside.numel() else (), (T.SENTINEL, 0.0)):
            assert bool((p == want).all()), f"{row.id}: an element outside the output slice changed"


def test_gemm_exact_total(report):
    """the measured total and the slowest case of this file's rows (reference on the host included), for profiles/gemm_exact.log"""
    if not _times:          # (run on its own: nothing to report)
        return
    worst = max(_times, key=_times.get)
    report(f"[gemm-exact] {len(_times)} rows, total {sum(_times.values()):.1f} s, slowest {worst} {_times[worst]:.2f} s")
