"""Every depthwise kernel of the fp16, packed strict and fp32 storages against an fp64 reference WITHOUT A TOLERANCE (tests/_dw_cases.py:
operands on which fp32 arithmetic is exact in any summation order, results on the fp16 grid), at the TensorFlow SAME paddings of the
stride-2 MBConv layers, at VALID and shifted pads, at tile tails, partly filled channel blocks and uneven XCD bands.  Per row:
  * the kernel the row names is the one the dry runs send it to (tests/test_dw_cases_cpu.py holds that without a GPU; asserted again
    here before the launch, with the LDS switch as the test sets it);
  * the output equals ref64 under torch.equal; a failure names how many elements differ and the first (image, y, x, channel);
  * a second launch on the same operands agrees bit for bit.
A mismatch on these operands is a kernel bug, never rounding.  The silu / gelu epilogues of the same rows are held to ref64 with the
existing metric and tolerances (tests/test_gpu_passes.py)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops_ref as R  # noqa: E402
from tests import _dw_cases as T  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402
from tests.test_gpu_ops import _experiments, check, dev, h, needs_experiments, same_pad_tf  # noqa: E402,F401  (_experiments: the mark's condition)
from tests.test_gpu_strict import A  # noqa: E402

TOL = {"f16": P.TOL_F16, "h2": P.TOL_OP, "s32": P.TOL_OP}
MODE = {"h2": "strict", "s32": "f32"}

_ops = P._ops
_REF = {}


def _ref(row, act="row"):
    """(x, w, b, ref64) of a row on the host, computed once and left unchanged"""
    act = row.act if act == "row" else act
    key = (row.id, act)
    if key not in _REF:
        x, w, b = T.operands(row)
        _REF[key] = (x, w, b, T.ref64(x, w, b, row.stride, row.pad, act))
    return _REF[key]


def _device(row, x, w, b):
    """the row's operands in its storage: the activation fp16 / packed / fp32, filter and bias fp32"""
    ops = _ops()
    xd = dev(x) if row.storage == "f16" else A(x, MODE[row.storage])
    return xd, ops.make_dw_weight(w), b.cuda()


def _host64(t):
    """an activation of any storage -> fp64 on the host (packed: hi + lo through vip_unpack_h2, then the status word is checked)"""
    if t.dtype == torch.int32:
        t = _ops().unpack_h2(t)
        _ops().h2_check("depthwise exact rows")
    return t.cpu().double()


def _assert_equal(name, got, ref):
    """exact equality of two [B, H, W, C] maps; the message counts the differing elements and names the first"""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    i = int(bad.flatten().nonzero()[0])
    _, H, W, Cc = ref.shape
    b, rem = divmod(i, H * W * Cc)
    y, rem = divmod(rem, W * Cc)
    x, c = divmod(rem, Cc)
    raise AssertionError(f"{name}: {int(bad.sum())} of {ref.numel()} elements differ, the first at image {b} y {y} x {x} channel {c}: "
                         f"got {got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}")


def _select(row, monkeypatch):
    """set the LDS switch the row's kernel needs and hold the dispatch once more"""
    ops = _ops()
    assert ops._DW_H2_LDS == 3
    assert T.reaches(row, ops) is None, T.reaches(row, ops)
    if row.kernel == "dwconv_tile_h2_kernel":
        monkeypatch.setattr(ops, "_DW_H2_LDS", 0)           # VIP_DW_H2_LDS=0: the tile twin takes what the LDS kernel took
    return ops


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_dw_exact(row, report, monkeypatch):
    ops = _select(row, monkeypatch)
    x, w, b, ref = _ref(row)
    xd, wd, bd = _device(row, x, w, b)
    run = lambda: ops.dwconv2d(xd, wd, bd, row.k, row.stride, row.pad, act=row.act)  # noqa: E731
    got = run()
    _assert_equal(f"{row.id} ({row.kernel})", _host64(got), ref)
    P._first_diff(got, run(), f"{row.id}: two launches on the same operands")
    report(f"[dw] {row.id}: {row.kernel} {row.B}x{row.H}x{row.W}x{row.C} k{row.k} s{row.stride} pad{row.pad} {row.act}: bit-exact")


@pytest.mark.parametrize("row", T.NONLINEAR, ids=lambda r: r.id)
def test_dw_nonlinear(row, report, monkeypatch):
    """the silu / gelu epilogue of a row per kernel: no longer exact, so the existing metric and tolerance of its storage"""
    ops = _select(row, monkeypatch)
    x, w, b, ref = _ref(row, row.nonlinear)
    xd, wd, bd = _device(row, x, w, b)
    got = ops.dwconv2d(xd, wd, bd, row.k, row.stride, row.pad, act=row.nonlinear)
    P._check_map(report, f"dw {row.id} ({row.kernel}) {row.nonlinear}", _host64(got), ref, TOL[row.storage])


def _vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


@pytest.mark.parametrize("row", T.POOL, ids=lambda r: r.id)
def test_dw_pool_partials_exact(row, report):
    """the pooling forms through their own entry points: the map equals the plain launch and ref64 bit for bit, and the partial sums add
    up to the fp64 per-channel sum of the map exactly (quarter units below 2^24: every fp32 sum is exact in any order)"""
    ops = _select(row, None)
    lib = ops._abi.lib()
    B, H, W, Cc, k, pad = row.B, row.H, row.W, row.C, row.k, row.pad
    Ho, Wo = T.out_hw(row)
    x, w, b, ref = _ref(row)
    assert 4 * ref.abs().sum((1, 2)).max().item() < 2 ** 24
    xd, wd, bd = _device(row, x, w, b)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = torch.empty((B, Ho, Wo, Cc), dtype=xd.dtype, device="cuda")
    if row.storage == "f16":
        parts = lib.vip_dwconv2d_pool_parts(B, H, W, Cc, k, 1, Ho, Wo)
        assert parts > 0
        partials = torch.full((B, parts, Cc), float("nan"), dtype=torch.float32, device="cuda")
        st = lib.vip_dwconv2d_pool_nhwc_f16(_vp(xd), _vp(wd), _vp(bd), _vp(y), _vp(partials), parts, B, H, W, Cc, k, 1, pad[0], pad[2], Ho, Wo,
                                            ops._act(row.act), stream)
    else:
        parts = lib.vip_dwconv2d_s1_pool_parts_h2(B, H, W, Cc, k, Ho, Wo)
        assert parts > 0
        partials = torch.full((B, parts, Cc), float("nan"), dtype=torch.float32, device="cuda")
        st = lib.vip_dwconv2d_s1_pool_h2(_vp(xd), _vp(ops._dw_quad_major(wd, k)), _vp(bd), _vp(y), _vp(partials), parts, B, H, W, Cc, k,
                                         pad[0], pad[2], Ho, Wo, ops._act(row.act), _vp(ops.h2_status()), stream)
    assert st == 0, lib.vip_last_error()
    torch.cuda.synchronize()
    plain = ops.dwconv2d(xd, wd, bd, k, 1, pad, act=row.act)
    P._first_diff(y, plain, f"{row.id}: the map of the pooling form against the plain launch")
    _assert_equal(f"{row.id} ({row.kernel}) map", _host64(y), ref)
    sums = partials.sum(1).cpu().double()
    want = ref.sum((1, 2))
    assert torch.equal(sums, want), (f"{row.id}: {int((sums != want).sum())} of {want.numel()} pooled sums differ, the first at (image, channel) "
                                     f"{divmod(int(((sums != want) | torch.isnan(sums)).flatten().nonzero()[0]), Cc)}")
    report(f"[dw] {row.id}: {row.kernel} {B}x{H}x{W}x{Cc} k{k} pad{pad} {row.act}, {parts} partial rows per image: bit-exact, partials exact")


@pytest.mark.parametrize("k,s,Cin,Ce,H,W,B,hilo", [(3, 2, 24, 144, 20, 20, 2, True), (5, 2, 32, 192, 15, 15, 2, True), (3, 2, 56, 336, 7, 7, 3, False)])
def test_mbconv_two_launches_tf_same(k, s, Cin, Ce, H, W, B, hilo, report):
    """ops.mbconv_expand_dw as the default build runs it - conv2d then dwconv2d - at the stride-2 shapes of
    tests/test_gpu_ops.py::test_mbconv_expand_dw (TF SAME padding: asymmetric on the even map), against the same oracle expression"""
    import math
    ops = _ops()
    assert not ops.mbconv_fused()
    g = torch.Generator().manual_seed(k * 100 + s * 10 + Cin)
    x = h(torch.randn(B, H, W, Cin, generator=g))
    we = torch.randn(1, 1, Cin, Ce, generator=g) / math.sqrt(Cin)
    be = torch.randn(Ce, generator=g) * 0.2
    wd = torch.randn(k, k, Ce, 1, generator=g) / k
    bd = torch.randn(Ce, generator=g) * 0.1
    pad = (*same_pad_tf(H, k, s), *same_pad_tf(W, k, s))
    hid = h(R.act(R.conv2d(x, we, be), "silu"))                      # the expanded activations are fp16
    ref = R.act(R.dwconv2d(hid, wd, bd, s, pad), "silu")
    cw = ops.make_conv_weight(we, be, hilo=hilo)
    two, names = P._launched(lambda: ops.mbconv_expand_dw(dev(x), cw, wd[..., 0].contiguous().cuda(), bd.cuda(), k, s, pad, act="silu"))
    torch.cuda.synchronize()
    assert "mbconv_expand_dw_kernel" not in names, names
    assert two.shape == ref.shape
    check(report, f"mbconv two launches k{k} s{s} Cin{Cin} Ce{Ce} {H}x{W} pad{pad} hilo={hilo}", two, ref, tol=3e-3)


@needs_experiments
@pytest.mark.parametrize("row", T.MFMA, ids=lambda r: r.id)
def test_dw_exact_matrix_cores(row, report, monkeypatch):
    """the matrix-core experiment (VIP_DW_MFMA=1, read per call) on the exact rows it supports: its hi / lo fp16 filter holds these taps
    exactly and it accumulates in fp32"""
    ops = _ops()
    x, w, b, ref = _ref(row)
    xd, wd, bd = _device(row, x, w, b)
    monkeypatch.setenv("VIP_DW_MFMA", "1")
    got = ops.dwconv2d(xd, wd, bd, row.k, row.stride, row.pad, act=row.act)
    torch.cuda.synchronize()
    _assert_equal(f"{row.id} (matrix cores)", _host64(got), ref)
    report(f"[dw] {row.id}: dwconv_mfma {row.B}x{row.H}x{row.W}x{row.C} k{row.k} pad{row.pad} {row.act}: bit-exact")
