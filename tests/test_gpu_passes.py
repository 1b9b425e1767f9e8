"""The persistent kernels PAST THEIR FIRST GRID PASS (tests/_pass_cases.py): every row is sized so that the launch's grid sits at its cap
and workgroups walk several units of work, carrying device-side state (the weight ring of the streamed MLPs, the reused LDS reduction
area of the pooling depthwise kernel, the descriptor slots of the LDS-staged one) from unit to unit.  Per row:
  * the launcher's own dry run confirms the regime BEFORE anything is launched (ceil(units / workgroups) >= 2 or 3, a ragged last pass);
  * the whole output is compared with oracle/ops_ref.py in fp32 (computed in chunks), at the tolerance the kernel's single-pass sibling
    test in test_gpu_ops.py / test_gpu_strict.py uses; a failure names the row / tile / pass or the image / y / x / channel of the worst
    element;
  * a second launch on the same operands must agree bit for bit (a race in the cross-tile ring or the reused reduction area would not);
  * where the product has a second path with the same rounding points (ops.unfused(), the two plain launches of a pooling form) the whole
    tensor is held against it."""
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops_ref as R  # noqa: E402
from tests import _pass_cases as T  # noqa: E402

TOL_MLP_F16 = 4e-3     # test_gpu_ops.py::test_mlp_fused: one extra fp16 rounding inside each dot product
TOL_F16 = 2e-3         # test_gpu_ops.py::check: fp32 accumulation order and the fp16 rounding of the output
TOL_OP = 2e-5          # test_gpu_strict.py::TOL_OP: fp32 summation order on the packed storage
# fused vs unfused fp16 MLP: the same rounding points (normalised row and hidden activations in fp16, output in fp16) and fp32 sums in
# another order.  An fp32 difference of ~1e-6 can move an output across an fp16 rounding boundary - one ulp, at most 2^-10 of the
# output scale - and flip a hidden value by one ulp (2^-11 |h| |w2| ~ 1e-5 each, a handful per row): two ulps bound both
TOL_MLP_F16_UNFUSED = 2.0 ** -9


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def h(t):
    """fp16-rounded fp32 copy (CPU) of t"""
    return t.to(torch.float16).to(torch.float32)


def dev16(t):
    return t.to(torch.float16).cuda().contiguous()


def dev32(t):
    return t.to(torch.float32).cuda().contiguous()


def packed(t):
    return _ops().pack_h2(dev32(t))


def host(t):
    """an activation of either storage -> fp32 on the host"""
    if t.dtype == torch.int32:
        t = _ops().unpack_h2(t)
    return t.float().cpu()


class _Kernels:
    """ops.set_profiler() recorder: the kernel name of every launch that declares one"""

    def __init__(self):
        self.names = []

    def start(self, kernel, flops, nbytes, tag=None):
        self.names.append(kernel)
        return 0

    def stop(self, tok):
        pass


def _launched(fn):
    """(fn(), kernel names it launched)"""
    ops = _ops()
    rec, old = _Kernels(), ops._PROF
    ops.set_profiler(rec)
    try:
        out = fn()
    finally:
        ops.set_profiler(old)
    return out, rec.names


def _assert_regime(units, workgroups, min_passes):
    passes = -(-units // workgroups)
    assert passes >= min_passes and units % workgroups != 0, f"not a ragged {min_passes}-pass launch: {units} units, {workgroups} workgroups"
    return passes


def _worst(got, ref):
    """(max |got - ref|, its flat index, output scale)"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    d = (got - ref).abs().flatten()
    i = int(d.argmax())
    return d[i].item(), i, ref.abs().max().item() + 1e-6


def _check_rows(report, name, got, ref, tol, tile_rows, workgroups):
    """[M, C] against the oracle; on failure: the row, its tile, the workgroup and the pass that computed it"""
    err, i, scale = _worst(got, ref)
    r, c = divmod(i, ref.shape[1])
    tile = r // tile_rows
    where = f"row {r} channel {c}: tile {tile} (row {r % tile_rows} of it) = pass {tile // workgroups} of workgroup {tile % workgroups}"
    report(f"[passes] {name}: max_abs_err={err:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e} worst at {where}")
    assert err <= tol * scale, f"{name}: err {err:.3e} > {tol} * {scale:.3e} at {where}"
    return err / scale


def _check_map(report, name, got, ref, tol):
    """[B, H, W, C] against the oracle; on failure: image, y, x, channel of the worst element"""
    err, i, scale = _worst(got, ref)
    _, H, W, C = ref.shape
    b, rem = divmod(i, H * W * C)
    y, rem = divmod(rem, W * C)
    x, c = divmod(rem, C)
    where = f"image {b} y {y} x {x} channel {c}"
    report(f"[passes] {name}: max_abs_err={err:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e} worst at {where}")
    assert err <= tol * scale, f"{name}: err {err:.3e} > {tol} * {scale:.3e} at {where}"
    return err / scale


def _check_gate(report, name, got, ref, tol):
    err, i, scale = _worst(got, ref)
    b, c = divmod(i, ref.shape[1])
    report(f"[passes] {name}: max_abs_err={err:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e} worst at image {b} channel {c}")
    assert err <= tol * scale, f"{name}: err {err:.3e} > {tol} * {scale:.3e} at image {b} channel {c}"


def _first_diff(a, b, what):
    """bit equality of two device tensors; the message names the first element that differs"""
    if torch.equal(a, b):
        return
    i = int((a.flatten() != b.flatten()).nonzero()[0])
    raise AssertionError(f"{what}: {int((a != b).sum())} elements differ, the first at flat index {i} of shape {tuple(a.shape)}")


def _mlp_oracle(x, ln, w1, b1, w2, b2, res):
    """fp32, 32768 rows at a time (the hidden tensor of the whole input would be gigabytes)"""
    out = torch.empty_like(x)
    for m0 in range(0, x.shape[0], 32768):
        xs = x[m0:m0 + 32768]
        if ln is not None:
            xs = R.layernorm(xs, *ln)
        out[m0:m0 + 32768] = R.dense(R.act(R.dense(xs, w1, b1), "gelu"), w2, b2)
    return out if res is None else out + res


def _dw_oracle(x, w, b, pad, act):
    """fp32, 64 images at a time"""
    return torch.cat([R.act(R.dwconv2d(x[i:i + 64], w, b, 1, pad), act) for i in range(0, x.shape[0], 64)])


def _mlp_shape(ops, row, is_packed):
    """(M, units, workgroups, tile rows, passes) of a table row on this device, the regime asserted from the launcher's dry run"""
    cap = ops.mlp_plan(T.BIG_M, row.C, row.hidden, packed=is_packed)
    assert cap is not None, "the fused kernel does not take this width"
    _, G, tile = cap
    M = T.mlp_rows(row, tile, G)
    units, workgroups, tile_m = ops.mlp_plan(M, row.C, row.hidden, packed=is_packed)
    assert (workgroups, tile_m) == (G, tile) and units == row.full(G) + 1
    return M, units, workgroups, tile, _assert_regime(units, workgroups, row.min_passes)


@pytest.mark.parametrize("row", T.MLP_F16, ids=lambda r: r.id)
def test_mlp_f16_passes(row, report):
    """inputs as tests/test_gpu_ops.py::test_mlp_fused"""
    ops = _ops()
    t0 = time.time()
    C, hid = row.C, row.hidden
    M, units, workgroups, tile, passes = _mlp_shape(ops, row, False)
    g = torch.Generator().manual_seed(M + C + hid)
    x = h(torch.randn(M, C, generator=g) * 1.5 + 0.3)
    w1 = h(torch.randn(C, hid, generator=g) / math.sqrt(C))
    b1 = torch.randn(hid, generator=g) * 0.1
    w2 = h(torch.randn(hid, C, generator=g) / math.sqrt(hid))
    b2 = torch.randn(C, generator=g) * 0.1
    res = h(torch.randn(M, C, generator=g)) if row.res else None
    ln = ln_dev = None
    if row.ln:
        lg, lb = torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.1
        ln, ln_dev = (lg, lb, 1e-6), (lg.cuda(), lb.cuda(), 1e-6)
    t1 = time.time()
    ref = _mlp_oracle(x, ln, w1, b1, w2, b2, res)
    t_oracle = time.time() - t1
    xd, rd = dev16(x), (None if res is None else dev16(res))
    fc1, fc2 = ops.make_dense_weight(w1, b1), ops.make_dense_weight(w2, b2)
    run = lambda: ops.mlp(xd, fc1, fc2, act="gelu", residual=rd, ln=ln_dev)  # noqa: E731
    got, names = _launched(run)
    assert names == ["mlp_fused_kernel" if C <= 96 else "mlp_stream_kernel"], names
    name = f"mlp f16 {row.id} M{M} C{C} hid{hid}: {units} tiles / {workgroups} workgroups = {passes} passes"
    rel = _check_rows(report, name, host(got), ref, TOL_MLP_F16, tile, workgroups)
    _first_diff(got, run(), f"{name}: two launches on the same operands")
    with ops.unfused():
        two, names2 = _launched(run)
    assert not any(n.startswith("mlp_") for n in names2), names2
    _check_rows(report, f"{name} vs unfused", host(got), host(two), TOL_MLP_F16_UNFUSED, tile, workgroups)
    report(f"[passes] {name}: rel={rel:.3e} oracle {t_oracle:.1f} s, test {time.time() - t0:.1f} s")


@pytest.mark.parametrize("row", T.MLP_H2, ids=lambda r: r.id)
def test_mlp_h2_passes(row, report):
    """inputs as tests/test_gpu_strict.py::test_mlp_fused_h2"""
    ops = _ops()
    t0 = time.time()
    C, hid = row.C, row.hidden
    M, units, workgroups, tile, passes = _mlp_shape(ops, row, True)
    g = torch.Generator().manual_seed(C + hid)
    x = torch.randn(M, C, generator=g) * 1.5
    k1, b1 = torch.randn(C, hid, generator=g) / math.sqrt(C), torch.randn(hid, generator=g) * 0.1
    k2, b2 = torch.randn(hid, C, generator=g) / math.sqrt(hid), torch.randn(C, generator=g) * 0.1
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    with ops.precision("strict"):
        fc1, fc2 = ops.make_dense_weight(k1, b1), ops.make_dense_weight(k2, b2)
    t1 = time.time()
    ref = _mlp_oracle(x, (gam, bet, 1e-5) if row.ln else None, k1, b1, k2, b2, x if row.res else None)
    t_oracle = time.time() - t1
    xa = packed(x)
    ln_dev = (dev32(gam), dev32(bet), 1e-5) if row.ln else None
    run = lambda: ops.mlp(xa, fc1, fc2, act="gelu", residual=xa if row.res else None, ln=ln_dev)  # noqa: E731
    got, names = _launched(run)
    ops.h2_check(row.id)
    assert names == ["h2:mlp_h2_kernel"], names
    name = f"mlp h2 {row.id} M{M} C{C} hid{hid}: {units} tiles / {workgroups} workgroups = {passes} passes"
    rel = _check_rows(report, name, host(got), ref, TOL_OP, tile, workgroups)
    _first_diff(got, run(), f"{name}: two launches on the same operands")
    with ops.unfused():
        three, names3 = _launched(run)
    assert "h2:mlp_h2_kernel" not in names3, names3
    _check_rows(report, f"{name} vs three launches", host(got), host(three), TOL_OP, tile, workgroups)
    report(f"[passes] {name}: rel={rel:.3e} oracle {t_oracle:.1f} s, test {time.time() - t0:.1f} s")


def _se_weights(g, C, Cr):
    w1 = torch.randn(C, Cr, generator=g) / math.sqrt(C)
    b1 = torch.randn(Cr, generator=g) * 0.1
    w2 = torch.randn(Cr, C, generator=g) / math.sqrt(Cr)
    b2 = torch.randn(C, generator=g) * 0.1
    return w1, b1, w2, b2


@pytest.mark.parametrize("row", T.DW_TILE, ids=lambda r: r.id)
def test_dwconv_tile_passes(row, report):
    """inputs as tests/test_gpu_ops.py::test_dwconv, the pooled row as test_dwconv_se_pool"""
    ops = _ops()
    t0 = time.time()
    B, H, W, C, k, pad, act = row.B, row.H, row.W, row.C, row.k, row.pad, row.act
    groups, workgroups, geom = ops.dwconv_tile_plan(B, H, W, C, k, pad=pad, pooled=row.pooled)
    passes = _assert_regime(groups, workgroups, 2)
    assert workgroups == geom["cap"]
    g = torch.Generator().manual_seed(k * 100 + C + H)
    x = h(torch.randn(B, H, W, C, generator=g) + (0.2 if row.pooled else 0.0))
    w = torch.randn(k, k, C, 1, generator=g) / k            # depthwise filters are fp32 at the boundary
    b = torch.randn(C, generator=g) * 0.1
    t1 = time.time()
    ref = _dw_oracle(x, w, b, pad, act)
    t_oracle = time.time() - t1
    xd, wd, bd = dev16(x), w[..., 0].contiguous().cuda(), b.cuda()
    name = f"dwconv tile {row.id} B{B}: {groups} groups / {workgroups} workgroups = {passes} passes"
    if not row.pooled:
        got = ops.dwconv2d(xd, wd, bd, k, 1, pad, act=act)
        rel = _check_map(report, name, host(got), ref, TOL_F16)
        _first_diff(got, ops.dwconv2d(xd, wd, bd, k, 1, pad, act=act), f"{name}: two launches on the same operands")
    else:
        Ho, Wo = ref.shape[1:3]
        assert ops._abi.lib().vip_dwconv2d_pool_parts(B, H, W, C, k, 1, Ho, Wo) * B == groups       # it really is the pooling kernel
        w1, b1, w2, b2 = _se_weights(g, C, T.POOL_CR)
        w1, w2 = h(w1 * 3), h(w2 * 2)
        ref_gate = R.act(R.dense(R.act(R.dense(ref.mean(dim=(1, 2)), w1, b1), "silu"), w2, b2), "sigmoid")
        fc1, fc2 = ops.make_dense_weight(w1, b1), ops.make_dense_weight(w2, b2)
        run = lambda: ops.dwconv2d_se(xd, wd, bd, k, 1, pad, act, fc1, fc2, "silu", "sigmoid")  # noqa: E731
        got, gate = run()
        rel = _check_map(report, name, host(got), ref, TOL_F16)
        gsum = gate[:, 0].float().cpu() + gate[:, 1].float().cpu()
        _check_gate(report, f"{name} gate vs fp32", gsum, ref_gate, 2e-5)
        plain = ops.dwconv2d(xd, wd, bd, k, 1, pad, act=act)
        plain_gate = ops.se_gate(plain, fc1, fc2, "silu", "sigmoid")
        _first_diff(got, plain, f"{name}: the map of the pooling form against the plain launch")
        d = (gsum - (plain_gate[:, 0].float().cpu() + plain_gate[:, 1].float().cpu())).abs()
        report(f"[passes] {name}: max |gate - gate(two launches)| = {d.max().item():.2e}")
        assert d.max().item() <= 2e-4, f"gate against the two plain launches: {d.max().item():.3e} at image {int(d.argmax()) // C}"
        again, again_gate = run()
        _first_diff(got, again, f"{name}: two launches on the same operands (map)")
        _first_diff(gate, again_gate, f"{name}: two launches on the same operands (gate)")
    report(f"[passes] {name}: rel={rel:.3e} oracle {t_oracle:.1f} s, test {time.time() - t0:.1f} s")


@pytest.mark.parametrize("row", T.DW_LDS, ids=lambda r: r.id)
def test_dwconv_lds_passes(row, report):
    """inputs as tests/test_gpu_strict.py::test_dwconv_lds_h2, the pooled row as test_dwconv_se_pooled_h2"""
    ops = _ops()
    t0 = time.time()
    H, W, C, k, act = row.H, row.W, row.C, row.k, row.act
    B = T.lds_batch(row, ops.dwconv_lds_plan(row.base_B, H, W, C, k)[1])
    items, workgroups, geom = ops.dwconv_lds_plan(B, H, W, C, k)
    assert items / workgroups >= 2.5, (items, workgroups)
    passes = _assert_regime(items, workgroups, 3)
    assert {key: geom[key] for key in row.geom} == row.geom, geom
    p = k // 2
    pad = (p, p, p, p)
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + k)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(k, k, C, 1, generator=g) / k
    b = torch.randn(C, generator=g) * 0.1
    t1 = time.time()
    ref = _dw_oracle(x, w, b, pad, act)
    t_oracle = time.time() - t1
    xa, dw, bb = packed(x), ops.make_dw_weight(w), dev32(b)
    name = f"dwconv lds {row.id} B{B}: {items} items / {workgroups} workgroups = {passes} passes"
    if not row.pooled:
        got = ops.dwconv2d(xa, dw, bb, k, 1, pad, act=act)
        ops.h2_check(row.id)
        rel = _check_map(report, name, host(got), ref, TOL_OP)
        _first_diff(got, ops.dwconv2d(xa, dw, bb, k, 1, pad, act=act), f"{name}: two launches on the same operands")
    else:
        assert ops._abi.lib().vip_dwconv2d_s1_pool_parts_h2(B, H, W, C, k, H, W) > 0
        Cr = max(8, C // 4 // 8 * 8)
        k1, b1, k2, b2 = _se_weights(g, C, Cr)
        with ops.precision("strict"):
            fc1, fc2 = ops.make_dense_weight(k1, b1), ops.make_dense_weight(k2, b2)
        ref_gate = torch.sigmoid(R.dense(R.act(R.dense(ref.mean((1, 2)), k1, b1), "silu"), k2, b2))
        run = lambda: ops.dwconv2d_se(xa, dw, bb, k, 1, pad, act, fc1, fc2, "silu", "sigmoid")  # noqa: E731
        got, gate = run()
        ops.h2_check(row.id)
        rel = _check_map(report, name, host(got), ref, TOL_OP)
        _check_gate(report, f"{name} gate vs fp32", host(gate), ref_gate, TOL_OP)
        with ops.unfused():
            plain, plain_gate = run()
        _first_diff(got, plain, f"{name}: the map of the pooling form against the plain launch")
        d = (host(gate) - host(plain_gate)).abs()
        report(f"[passes] {name}: max |gate - gate(two launches)| = {d.max().item():.2e}")
        assert d.max().item() <= 2e-6, f"gate against the two plain launches: {d.max().item():.3e} at image {int(d.argmax()) // C}"
        again, again_gate = run()
        _first_diff(got, again, f"{name}: two launches on the same operands (map)")
        _first_diff(gate, again_gate, f"{name}: two launches on the same operands (gate)")
    report(f"[passes] {name}: rel={rel:.3e} oracle {t_oracle:.1f} s, test {time.time() - t0:.1f} s")


@pytest.mark.parametrize("storage", ["f16", "h2"])
def test_scale_add_act_passes(storage, report):
    """act(x * gate + residual) and its second output past the 8192-block cap of the elementwise grids (grid_for / sgrid); inputs as
    tests/test_gpu_ops.py::test_scale_add_act_and_head, the gate split into (hi, lo) planes on the fp16 storage"""
    ops = _ops()
    t0 = time.time()
    B, H, W, C = T.ELEMENTWISE
    per_item = 8 if storage == "f16" else 4
    items = B * H * W * C // per_item
    passes = _assert_regime(items, T.ELEMENTWISE_CAP, 2)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, H, W, C, generator=g)
    s = torch.rand(B, C, generator=g)
    r = torch.randn(B, H, W, C, generator=g)
    if storage == "f16":
        x, r = h(x), h(r)
        hi = h(s)
        lo = h(s - hi)
        s = hi + lo
        xd, rd, sd = dev16(x), dev16(r), torch.stack([hi, lo], 1).to(torch.float16).cuda().contiguous()
        tol = TOL_F16
    else:
        xd, rd, sd = packed(x), packed(r), packed(s)
        tol = TOL_OP
    ref = torch.relu(x * s[:, None, None, :] + r)
    ref2 = R.act(ref, "silu")
    y, y2 = ops.scale_add_act(xd, sd, rd, "relu", act2="silu")
    if storage == "h2":
        ops.h2_check("scale_add_act")
    name = f"scale_add_act {storage} {B}x{H}x{W}x{C}: {items} items / {T.ELEMENTWISE_CAP} per pass = {passes} passes"
    rel = _check_map(report, name, host(y), ref, tol)
    _check_map(report, f"{name} second output", host(y2), ref2, tol)
    ya, y2a = ops.scale_add_act(xd, sd, rd, "relu", act2="silu")
    _first_diff(y, ya, f"{name}: two launches on the same operands")
    _first_diff(y2, y2a, f"{name}: two launches on the same operands (second output)")
    report(f"[passes] {name}: rel={rel:.3e} test {time.time() - t0:.1f} s")
