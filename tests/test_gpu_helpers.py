"""The NHWC helper kernels of the fp16, packed strict and fp32 storages against fp64 references (tests/_helper_cases.py): pooling, global
average pool, scale_add_act, mul, radix_combine, LayerNorm, the classifier heads and the score kernels, at their own edge shapes.  Most
rows run on operands whose correct result is exact and are held WITHOUT A TOLERANCE (torch.equal against the reference, or against its
one fp16 rounding); a failure names how many elements differ and the first.  A mismatch there is a kernel bug, never rounding.  What
cannot be exact is held to the project's existing tolerances, per channel chunk (scale_add_act) or per row (LayerNorm), and its worst
error goes through the report fixture.  Rows with a leading dimension wider than C, or an output offset, call the entry point through
ops._launch_kind with the wrapper's own argument order; their outputs lie inside a sentinel-filled buffer of one allocation, and every
element outside the slice must still hold the sentinel bit for bit.  tests/test_helper_cases_cpu.py holds the table without a GPU."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _helper_cases as T  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402
from tests.test_gpu_ops import dev  # noqa: E402
from tests.test_gpu_strict import A  # noqa: E402

MODE = {"h2": "strict", "s32": "f32"}
SENTINEL = -777.0                      # finite, on the fp16 grid

_ops = P._ops


def rows_of(op, big=None):
    return [r for r in T.ROWS if r.op == op and (big is None or bool(r.p.get("big")) == big)]


def _act(t, storage):
    """a host fp32 tensor -> an activation in the storage"""
    return dev(t) if storage == "f16" else A(t, MODE[storage])


def _f32(t):
    return None if t is None else t.float().cuda().contiguous()


def _host64(t):
    """an activation of any storage, or an fp32 result -> fp64 on the host (packed: hi + lo, then the status word is checked)"""
    if t.dtype == torch.int32:
        t = _ops().unpack_h2(t.contiguous())
        _ops().h2_check("helper rows")
    return t.cpu().double()


def _bits(t):
    """the carrier of an activation as integers: what `bit for bit` compares"""
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _assert_equal(name, got, want):
    """numerical equality (-0.0 == +0.0); the message counts the differing elements and names the first"""
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    i = int(bad.flatten().nonzero()[0])
    at = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), want.shape))
    raise AssertionError(f"{name}: {int(bad.sum())} of {want.numel()} elements differ, the first at {at}: got {got.flatten()[i].item()!r}, "
                         f"reference {want.flatten()[i].item()!r}")


def _hold(report, row, got, ref, part=""):
    """a row's output (fp64 on the host) against its reference, as the row's `accept` says; tolerance rows report their worst error"""
    name = f"{row.id}{part} ({row.kernel})"
    if row.accept in ("exact", "round16"):
        _assert_equal(name, got, T.expected(row, ref))
        return
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), name
    tol = T.tolerance(row, P)
    rel, i = T.rel_error(row, got, ref)
    at = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    report(f"[helpers] {name}: worst rel err {rel:.3e} per {T.group_of(row)} scale at {at} (abs {abs(got.flatten()[i] - ref.flatten()[i]).item():.3e}), "
           f"{row.accept} = {tol:g}")
    assert rel <= tol, f"{name}: relative error {rel:.3e} > {row.accept} = {tol:g} at {at}"


def _sentinel_buffer(shape, storage):
    return _act(torch.full(shape, SENTINEL), storage)


def _assert_outside_untouched(name, after, before, lo, hi):
    """every element of the last axis outside [lo, hi) still holds the sentinel's bits"""
    a, b = _bits(after), _bits(before)
    for part in (slice(0, lo), slice(hi, None)):
        assert torch.equal(a[..., part], b[..., part]), f"{name}: the launch wrote outside its output slice"


# ---- pool2d ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows_of("pool2d", big=False), ids=lambda r: r.id)
def test_pool2d(row, report):
    ops = _ops()
    p = row.p
    o = T.operands(row)
    ref = T.reference(row, o)
    Ho, Wo = T.pool_out_hw(p)
    if p["ldx"] is None:
        got = ops.pool2d(_act(o["x"], row.storage), p["k"], p["stride"], p["pad"], p["mode"], out_hw=p["out_hw"])
        _hold(report, row, _host64(got), ref)
        return
    B, H, W, Cc = o["x"].shape
    wide = torch.full((B, H, W, p["ldx"]), 1000.0)                      # the channels next to the slice would show in any sum
    wide[..., 8:8 + Cc] = o["x"]
    xd = _act(wide, row.storage)
    buf = _sentinel_buffer((B, Ho, Wo, p["ldy"]), row.storage)
    before = buf.clone()
    ops._launch_kind("pool2d_nhwc", row.storage, ops._p(xd[..., 8:]), ops._p(buf[..., 8:]), B, H, W, Cc, p["ldx"], p["ldy"], p["k"], p["stride"],
                     p["pad"][0], p["pad"][2], Ho, Wo, p["mode"])
    torch.cuda.synchronize()
    _hold(report, row, _host64(buf[..., 8:8 + Cc]), ref)
    _assert_outside_untouched(row.id, buf, before, 8, 8 + Cc)


@pytest.mark.parametrize("row", rows_of("pool2d", big=True), ids=lambda r: r.id)
def test_pool2d_second_pass(row):
    """the k = 1 copy past the grid cap; the reference is the input itself (fp32 on the host)"""
    ops = _ops()
    x = T.operands(row)["x"]
    got = ops.pool2d(_act(x, row.storage), 1, 1, (0, 0, 0, 0), 0)
    _assert_equal(row.id, _host64(got).float(), x)


# ---- global average pool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows_of("gap"), ids=lambda r: r.id)
def test_global_avgpool(row, report):
    ops = _ops()
    p = row.p
    o = T.operands(row)
    ref = T.reference(row, o)
    B, HW, Cc = o["x"].shape
    if p["ldx"] is None:
        xd = _act(o["x"], row.storage)
        run = lambda split: ops.global_avgpool(xd, split=split)  # noqa: E731
    else:
        wide = torch.full((B, HW, p["ldx"]), 1000.0)
        wide[..., 8:8 + Cc] = o["x"]
        xd = _act(wide, row.storage)

        def run(split):
            out = torch.empty((B, 2, Cc) if split else (B, Cc), dtype=xd.dtype, device="cuda")
            if split:
                ops._launch("vip_global_avgpool_split_f16", ops._p(xd[..., 8:]), ops._p(out), B, HW, Cc, p["ldx"])
            else:
                ops._launch_kind("global_avgpool", row.storage, ops._p(xd[..., 8:]), ops._p(out), B, HW, Cc, p["ldx"])
            return out
    if not p["split"]:
        _hold(report, row, _host64(run(False)), ref)
        return
    # the split form: hi is the plain output bit for bit, |lo| <= 2^-11 |hi|, hi + lo within the existing 1e-6 of the reference
    both, plain = run(True), run(False)
    hi, lo = both[:, 0], both[:, 1]
    assert torch.equal(_bits(hi.contiguous()), _bits(plain)), f"{row.id}: the hi plane is not the plain output"
    _assert_equal(f"{row.id} hi plane", hi.cpu().double(), T.round16(ref))
    assert (lo.double().abs() <= 2.0 ** -11 * hi.double().abs()).all(), f"{row.id}: |lo| > 2^-11 |hi|"
    _hold(report, row, hi.cpu().double() + lo.cpu().double(), ref)


# ---- scale_add_act ------------------------------------------------------------------------------------------------------------------------
def _saa_device(row, o):
    st = row.storage
    scale = None
    if o["hi"] is not None:
        scale = _act(o["hi"], st) if o["lo"] is None else dev(torch.stack([o["hi"], o["lo"]], 1))
    return _act(o["x"], st), scale, None if o["r"] is None else _act(o["r"], st)


@pytest.mark.parametrize("row", rows_of("scale_add_act", big=False), ids=lambda r: r.id)
def test_scale_add_act(row, report):
    ops = _ops()
    o = T.operands(row)
    ref = T.reference(row, o)
    xd, sd, rd = _saa_device(row, o)
    got = ops.scale_add_act(xd, sd, rd, row.p["act"], act2=row.p["act2"])
    if row.p["act2"]:
        _hold(report, row, _host64(got[0]), ref[0], " y")
        _hold(report, row, _host64(got[1]), ref[1], " y2")
    else:
        _hold(report, row, _host64(got), ref)


@pytest.mark.parametrize("row", rows_of("scale_add_act", big=True), ids=lambda r: r.id)
def test_scale_add_act_second_pass(row):
    """relu(x * gate + residual) past the grid cap; the reference in fp32 on the host (exact on these operands)"""
    ops = _ops()
    o = T.operands(row)
    ref = torch.relu(o["x"] * o["hi"][:, None, :] + o["r"])
    got = ops.scale_add_act(*_saa_device(row, o), "relu")
    _assert_equal(row.id, _host64(got).float(), ref)


# ---- mul ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows_of("mul"), ids=lambda r: r.id)
def test_mul(row, report):
    ops = _ops()
    p = row.p
    o = T.operands(row)
    st = row.storage
    if p["big"]:
        ref = o["a"][:, p["a_off"]:p["a_off"] + p["C"]] * o["b"][:, p["b_off"]:p["b_off"] + p["C"]]      # fp32: an exact product
    else:
        ref = T.reference(row, o)
    ad, bd = _act(o["a"], st), _act(o["b"], st)
    buf = _sentinel_buffer((p["rows"], p["ldy"]), st)
    before = buf.clone()
    ops._launch_kind("mul", st, ops._p(ad), ops._p(bd), ops._p(buf), p["rows"], p["C"], p["lda"], p["a_off"], p["ldb"], p["b_off"], p["ldy"], p["y_off"])
    torch.cuda.synchronize()
    got = _host64(buf[:, p["y_off"]:p["y_off"] + p["C"]])
    _assert_equal(f"{row.id} ({row.kernel})", got.float() if p["big"] else got, ref)
    _assert_outside_untouched(row.id, buf, before, p["y_off"], p["y_off"] + p["C"])
    if p["big"]:
        return
    # the wrapper's own call on the same slices: a contiguous output
    _assert_equal(f"{row.id} through ops.mul", _host64(ops.mul(ad, bd, p["C"], p["a_off"], p["b_off"])), got)


# ---- radix_combine ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows_of("radix_combine"), ids=lambda r: r.id)
def test_radix_combine(row, report):
    ops = _ops()
    p = row.p
    o = T.operands(row)
    st = row.storage
    B, HW, Cc, radix = p["B"], p["HW"], p["C"], p["radix"]
    xd = _act(o["x"].reshape(B, HW, 1, radix * Cc), st)
    sd = _act(o["hi"], st) if o["lo"] is None else dev(torch.stack([o["hi"], o["lo"]], 1))
    got = _host64(ops.radix_combine(xd, sd, radix)).reshape(B, HW, Cc)
    if p["big"]:                                                          # fp32 on the host: exact on these operands
        ref = (o["x"].reshape(B, HW, radix, Cc) * o["hi"].reshape(B, 1, radix, Cc)).sum(2)
        _assert_equal(row.id, got.float(), ref)
    else:
        _hold(report, row, got, T.reference(row, o))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows_of("layernorm"), ids=lambda r: r.id)
def test_layernorm(row, report):
    ops = _ops()
    o = T.operands(row)
    ref = T.reference(row, o)
    gd, bd = _f32(o["gamma"]), _f32(o["beta"])
    xd = _act(o["x"], row.storage)
    if row.storage == "h2":                                               # the kernel is handed exactly the packed values the reference saw
        assert torch.equal(_host64(xd), o["x"].double())
    got = ops.layernorm(xd, gd, bd, T.LN_EPS)
    _hold(report, row, _host64(got), ref)
    if row.p["kind"] != "structured":
        return
    # a row's result may not depend on where in the block it sits: the butterfly reductions leave every lane the same sum
    perm = torch.randperm(row.p["rows"], generator=torch.Generator().manual_seed(row.p["C"]))
    moved = ops.layernorm(xd[perm.cuda()].contiguous(), gd, bd, T.LN_EPS)
    P._first_diff(moved, got[perm.cuda()].contiguous(), f"{row.id}: the row-permuted input against the row-permuted output")


def test_layernorm_rejects_2056_channels_on_fp16():
    """five chunks per lane: the project's unsupported error, and nothing is launched - the output keeps its sentinel"""
    ops = _ops()
    from vipcup_amd import _abi
    x = dev(torch.ones(5, 2056))
    out = _sentinel_buffer((5, 2056), "f16")
    before = out.clone()
    par = torch.ones(2056, device="cuda")
    with pytest.raises(_abi.VipError, match=r"vip_status -3.*C=2056 too large"):
        ops._launch_kind("layernorm", "f16", ops._p(x), ops._p(par), ops._p(par), ops._p(out), 5, 2056, T.LN_EPS)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(before))


# ---- classifier heads ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows_of("head"), ids=lambda r: r.id)
def test_heads(row, report):
    ops = _ops()
    p = row.p
    o = T.operands(row)
    ref = T.reference(row, o)
    st = row.storage
    wd, bias = _f32(o["w"]), _f32(o["bias"])
    if p["kind"] == "cls_dense":
        got = ops.cls_dense_f32(_act(o["x"], st), wd, bias)
    elif p["kind"] == "gap_dense":
        got = ops.gap_dense_f32(_act(o["x"], st), wd, bias)
    elif p["ldx"] is None:
        got = ops.gap_ln_dense_f32(_act(o["x"], st), _f32(o["gamma"]), _f32(o["beta"]), T.HEAD_EPS, wd, bias)
    else:
        B, HW, Cc = o["x"].shape
        wide = torch.full((B, HW, p["ldx"]), 1000.0)
        wide[..., :Cc] = o["x"]
        xd = _act(wide, st)
        got = torch.empty((B, p["N"]), dtype=torch.float32, device="cuda")
        gd, bd = _f32(o["gamma"]), _f32(o["beta"])                        # held: a pointer does not keep its tensor alive
        head = (ops._p(xd), ops._p(gd), ops._p(bd), T.HEAD_EPS, ops._p(wd), ops._p(bias), ops._p(got), B, HW, Cc, p["ldx"])
        if st == "f16":
            ops._launch("vip_gap_ln_dense_f32", *head, p["N"])
        else:
            ops._launch_kind("gap_ln_dense", st, *head, HW * p["ldx"], p["N"])
    _hold(report, row, _host64(got), ref)


@pytest.mark.parametrize("storage", T.STORAGES)
def test_heads_reject_4104_channels(storage):
    """beyond the 4096 floats of the pooled vector in LDS: unsupported, nothing launched"""
    ops = _ops()
    from vipcup_amd import _abi
    Cc, N = 4104, 2
    xd = _act(torch.ones(3, 4, Cc), storage)
    w, par = torch.ones(N, Cc, device="cuda"), torch.ones(Cc, device="cuda")
    for ln in (False, True):
        out = torch.full((3, N), SENTINEL, device="cuda")
        with pytest.raises(_abi.VipError, match=r"vip_status -3.*C=4104 > 4096"):
            if storage != "f16":
                ops._launch_kind("gap_ln_dense", storage, ops._p(xd), ops._p(par if ln else None), ops._p(par if ln else None), T.HEAD_EPS, ops._p(w),
                                 None, ops._p(out), 3, 4, Cc, Cc, 4 * Cc, N)
            elif ln:
                ops._launch("vip_gap_ln_dense_f32", ops._p(xd), ops._p(par), ops._p(par), T.HEAD_EPS, ops._p(w), None, ops._p(out), 3, 4, Cc, Cc, N)
            else:
                ops._launch("vip_gap_dense_f32", ops._p(xd), ops._p(w), None, ops._p(out), 3, 4, Cc, Cc, N)
        torch.cuda.synchronize()
        assert (out == SENTINEL).all()


# ---- score kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows_of("score"), ids=lambda r: r.id)
def test_score_kernels(row, report):
    ops = _ops()
    p = row.p
    o = T.operands(row)
    ref = T.reference(row, o)
    if p["kind"] == "ensemble_mean":
        buf = torch.full((p["M"], p["ld"]), 1000.0, device="cuda")
        buf[:, :p["n"]] = o["s"].cuda()
        got = ops.ensemble_mean(buf[:, :p["n"]])
    elif p["kind"] == "binary_score":
        got = ops.binary_score(o["z"].cuda())
    else:
        got = ops.head_prob(o["z"].cuda(), act=p["act"])
    _hold(report, row, _host64(got), ref)
