"""ops.swin_window_attention (csrc/swin_attn.hip) on the three storages against tests/_swin_v2_ref.py in float64 - the layer as the
reference writes it (pad, two cats, partition, mask tensor, reverse, un-roll, crop), which shares no addressing with the kernel.
Rows and rules are those of tests/_swin_cases.py:
  * EXACT rows E1 .. E5 (spike, region means, padded keys with and without v_bias, table-dominated, epsilon) on every geometry of the
    table there: torch.equal on the fp16 and packed storages wherever the top set of the softmax has a power-of-two size (everywhere
    for E1 and E5), and the bound of scenario S3 of tests/_attn_cases.py - 0.5 ulp16(ref) + N 2^-23 max|v| per element - on every
    element of every storage, the fp32 storage included; a second launch agrees bit for bit;
  * BOUNDED rows, error relative to the output's absmax: tau around 10 (b10, bsmallq, beps - queries below the epsilon of the
    normalisation, where the clamp sets every logit - and one row per shape the registered members produce) under TOL_F16 on the fp16
    storage and TOL_OP on the packed and fp32 ones; tau = 100 (b100) under TOL_OP on packed / fp32 and, on the fp16 storage, under
    (exp(2 tau 2^-10) - 1) max|v| + one fp16 ulp: one fp16 rounding of the normalised q and k moves a logit by at most tau 2^-10 - no
    tolerance of the suite covers that, the bound is the arithmetic's own;
  * batch independence: each image of a three-image launch equals the image launched alone, bit for bit;
  * the argument checks refuse what the kernel does not serve before any launch.
With VIP_SWIN_FP64_LOG=<file> set every row appends its error per storage to that file (profiles/swin_attn_fp64.log is one such run
on an MI355X, reduced to the worst row of every family by tools/swin_fp64_worst.py)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _swin_cases as T  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402

STORAGES = ("f16", "h2", "s32")
assert (T.TOL_F16, T.TOL_OP) == (P.TOL_F16, P.TOL_OP)       # the case table's tolerances ARE the suite's
_ops = P._ops
_REF = {}


def _ref(row):
    """(operands, ref64, max|v|) of a row on the host, computed once and left unchanged"""
    if row.id not in _REF:
        o = T.operands(row)
        vmax = o[0][..., 2 * row.heads * T.HD:].abs().max().item()
        if o[1] is not None:
            vmax = max(vmax, o[1].abs().max().item())
        _REF[row.id] = (o, T.ref64(row, o), vmax)
    return _REF[row.id]


def _act(x, storage):
    return {"f16": P.dev16, "h2": P.packed, "s32": P.dev32}[storage](x)


def _host64(t, what):
    if t.dtype == torch.int32:
        t = _ops().unpack_h2(t)
        _ops().h2_check(what)
    return t.cpu().double()


def _run(row, o, storage):
    ops = _ops()
    qkv, v_bias, tau, table = o
    return ops.swin_window_attention(_act(qkv, storage), None if v_bias is None else P.dev32(v_bias), P.dev32(tau), P.dev32(table),
                                     row.heads, row.ws, row.shift)


def _note(family, storage, err, lim):
    path = os.environ.get("VIP_SWIN_FP64_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{family} {storage}: max_abs_err {err:.3e} = {err / lim if lim else 0.0:.3f} of its bound\n")


@pytest.mark.parametrize("row", T.EXACT, ids=lambda r: r.id)
def test_swin_attn_exact(row, report):
    o, ref, vmax = _ref(row)
    p2 = T.pow2_mask(row, o)
    if row.kind in ("E1", "E5"):
        assert p2.all()
    bound = T.s3_bound(ref, vmax, row.ws ** 2)
    for storage in STORAGES:
        dev = _run(row, o, storage)
        got = _host64(dev, row.id)
        assert torch.isfinite(got).all(), (row.id, storage)
        d = (got - ref).abs()
        worst = (d / bound).max().item()
        print(f"[swin_attn] {row.id} {storage}: max_abs_err {d.max().item():.3e}, {worst:.3f} of the S3 bound, "
              f"{p2.float().mean().item():.2f} of the outputs exact by design")
        _note(row.kind, storage, d.max().item(), bound[d == d.max()].max().item())
        assert (d <= bound).all(), (row.id, storage, worst)
        if storage != "s32":
            want = ref.to(torch.float16).double() if storage == "f16" else ref
            assert torch.equal(got[p2], want[p2]), (row.id, storage, (got - want)[p2].abs().max().item())
        P._first_diff(dev, _run(row, o, storage), f"{row.id} {storage}: two launches on the same operands")
    report(f"[swin_attn] {row.id}: {row.B}x{row.H}x{row.W}, {row.heads} head(s), ws {row.ws}, shift {row.shift}: exact rule holds on f16 / h2 / s32")


@pytest.mark.parametrize("row", T.BOUNDED, ids=lambda r: r.id)
def test_swin_attn_bounded(row, report):
    o, ref, vmax = _ref(row)
    line = []
    for storage in STORAGES:
        got = _host64(_run(row, o, storage), row.id)
        assert torch.isfinite(got).all(), (row.id, storage)
        err, tol = (got - ref).abs().max().item(), T.tolerance(row, storage, ref, vmax)
        print(f"[swin_attn] {row.id} {storage}: max_abs_err {err:.3e} (max|ref| {ref.abs().max().item():.3e}), bound {tol:.3e}")
        _note("member" if row.id.startswith("member") else row.kind, storage, err, tol)
        assert err <= tol, (row.id, storage, err, tol)
        line.append(f"{storage} {err / tol:.2f}")
    report(f"[swin_attn] {row.id}: share of the bound used: " + ", ".join(line))


@pytest.mark.parametrize("geom", [(5, 9, 4, 2, 2), (13, 13, 8, 4, 3), (10, 10, 3, 1, 1)], ids=lambda g: "x".join(map(str, g)))
def test_swin_attn_batch_independence(geom):
    H, W, ws, shift, heads = geom
    row = T.Row(f"batch-{H}x{W}-ws{ws}", "b10", 3, H, W, heads, ws, shift)
    o = T.operands(row)
    for storage in STORAGES:
        three = _run(row, o, storage)
        for i in range(3):
            alone = _run(row._replace(B=1), (o[0][i:i + 1].contiguous(),) + o[1:], storage)
            P._first_diff(three[i:i + 1].contiguous(), alone, f"{row.id} {storage}: image {i} of three against the image alone")


def test_swin_attn_refusals():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    ops = _ops()
    row = T.Row("refuse", "b10", 1, 8, 8, 1, 4, 0)
    qkv, v_bias, tau, table = T.operands(row)
    dev = lambda t: P.dev32(t)  # noqa: E731
    with pytest.raises(_abi.VipError, match="shift"):
        ops.swin_window_attention(P.dev16(qkv), dev(v_bias), dev(tau), dev(table), 1, 4, 1)
    with pytest.raises(_abi.VipError, match="head_dim"):
        ops.swin_window_attention(P.dev16(qkv[..., :48].contiguous()), dev(v_bias[:16]), dev(tau), dev(table), 1, 4, 0)
    big = torch.zeros(1, 9, 9, 96)
    with pytest.raises(_abi.VipError, match="ws"):
        ops.swin_window_attention(P.dev16(big), None, dev(tau), dev(torch.zeros(17 * 17, 1)), 1, 9, 0)
    with pytest.raises(_abi.VipError, match="bias_table"):
        ops.swin_window_attention(P.dev16(qkv), dev(v_bias), dev(tau), dev(table[:-1]), 1, 4, 0)
