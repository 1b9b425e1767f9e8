"""ops.nat_attention (csrc/nat_attn.hip) on the three storages against tests/_nat_ref.py in float64 - the layer as the reference writes
it (zero-pad, K x K patches of the VALID positions, replicate-pad, the bias gathered through the concatenated ramps and the reversal,
crop), which shares no addressing with the kernel.  Rows and rules are those of tests/_nat_cases.py:
  * EXACT rows N1 .. N5 (spike, self, table, uniform, padded maps with and without kv_pad) on every geometry of the table there:
    torch.equal on the fp16 and packed storages (both planes of the packed one) wherever the winner set of the softmax has a
    power-of-two size, and the bound of scenario S3 of tests/_attn_cases.py - 0.5 ulp16(ref) + N 2^-23 max|v| per element - on every
    element of every storage, the fp32 storage included; a second launch agrees bit for bit;
  * BOUNDED rows, error relative to the output's absmax, under TOL_F16 on the fp16 storage and TOL_OP on the packed and fp32 ones,
    among them one row per shape the registered members produce;
  * every element of a sentinel-filled output is written;
  * batch independence: each image of a three-image launch equals the image launched alone, bit for bit;
  * the argument checks refuse what the kernel does not serve before any launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _nat_cases as T  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402

STORAGES = ("f16", "h2", "s32")
assert (T.TOL_F16, T.TOL_OP) == (P.TOL_F16, P.TOL_OP)       # the case table's tolerances ARE the suite's
_ops = P._ops
_REF = {}


def _ref(row):
    """(operands, ref64, max|v|) of a row on the host, computed once and left unchanged"""
    if row.id not in _REF:
        o = T.operands(row)
        _REF[row.id] = (o, T.ref64(row, o), T.v_absmax(row, o))
    return _REF[row.id]


def _act(x, storage):
    return {"f16": P.dev16, "h2": P.packed, "s32": P.dev32}[storage](x)


def _host64(t, what):
    if t.dtype == torch.int32:
        t = _ops().unpack_h2(t)
        _ops().h2_check(what)
    return t.cpu().double()


def _run(row, o, storage):
    qkv, kv_pad, table = o
    return _ops().nat_attention(_act(qkv, storage), None if kv_pad is None else P.dev32(kv_pad), P.dev32(table), row.heads, row.K)


@pytest.mark.parametrize("row", T.EXACT, ids=lambda r: r.id)
def test_nat_attn_exact(row, report):
    o, ref, vmax = _ref(row)
    p2 = T.pow2_mask(row, o)
    if row.kind == "N2":
        assert p2.all()
    bound = T.s3_bound(ref, vmax, row.K ** 2)
    for storage in STORAGES:
        dev = _run(row, o, storage)
        got = _host64(dev, row.id)
        assert torch.isfinite(got).all(), (row.id, storage)
        d = (got - ref).abs()
        worst = (d / bound).max().item()
        print(f"[nat_attn] {row.id} {storage}: max_abs_err {d.max().item():.3e}, {worst:.3f} of the S3 bound, "
              f"{p2.float().mean().item():.2f} of the outputs exact by design")
        assert (d <= bound).all(), (row.id, storage, worst)
        if storage != "s32":
            # packed: the joined value hi + lo against the float64 reference itself, so both planes are held
            want = ref.to(torch.float16).double() if storage == "f16" else ref
            assert torch.equal(got[p2], want[p2]), (row.id, storage, (got - want)[p2].abs().max().item())
        P._first_diff(dev, _run(row, o, storage), f"{row.id} {storage}: two launches on the same operands")
    report(f"[nat_attn] {row.id}: {row.B}x{row.H}x{row.W}, {row.heads} head(s), K {row.K}: exact rule holds on f16 / h2 / s32")


@pytest.mark.parametrize("row", T.BOUNDED, ids=lambda r: r.id)
def test_nat_attn_bounded(row, report):
    o, ref, _ = _ref(row)
    line = []
    for storage in STORAGES:
        got = _host64(_run(row, o, storage), row.id)
        assert torch.isfinite(got).all(), (row.id, storage)
        err, tol = (got - ref).abs().max().item(), T.tolerance(row, storage, ref)
        print(f"[nat_attn] {row.id} {storage}: max_abs_err {err:.3e} (max|ref| {ref.abs().max().item():.3e}), bound {tol:.3e}")
        assert err <= tol, (row.id, storage, err, tol)
        line.append(f"{storage} {err / tol:.2f}")
    report(f"[nat_attn] {row.id}: share of the bound used: " + ", ".join(line))


@pytest.mark.parametrize("geom", [(9, 12, 7, 3), (5, 7, 7, 1), (6, 11, 5, 2), (13, 13, 7, 2)], ids=lambda g: "x".join(map(str, g)))
def test_nat_attn_every_element_is_written(geom, monkeypatch):
    """the operator's output buffer pre-filled with a sentinel (NaN; on the packed carrier the bit pattern of a NaN pair): nothing of it
    is left after the launch"""
    H, W, K, heads = geom
    row = T.Row(f"fill-{H}x{W}-k{K}", "b", 3, H, W, heads, K)
    o = T.operands(row)
    real_empty = torch.empty

    def poisoned(*a, **kw):
        t = real_empty(*a, **kw)
        if t.is_cuda:
            t.view(torch.int16).fill_(0x7E00)            # an fp16 NaN in every half; as fp32 0x7E007E00 is finite but huge (1e38)
        return t

    for storage in STORAGES:
        clean = _host64(_run(row, o, storage), row.id)
        qkv, kv_pad, table = _act(o[0], storage), P.dev32(o[1]), P.dev32(o[2])
        monkeypatch.setattr(torch, "empty", poisoned)
        try:
            dev = _ops().nat_attention(qkv, kv_pad, table, heads, K)
        finally:
            monkeypatch.setattr(torch, "empty", real_empty)
        raw = dev.cpu().view(torch.int16)
        if storage != "s32":
            assert not bool((raw == 0x7E00).any()), (row.id, storage)
        got = _host64(dev, row.id) if storage != "h2" else _ops().unpack_h2(dev).cpu().double()
        assert torch.equal(got, clean), (row.id, storage)


@pytest.mark.parametrize("geom", [(9, 12, 7, 2), (3, 10, 7, 3), (16, 9, 7, 1)], ids=lambda g: "x".join(map(str, g)))
def test_nat_attn_batch_independence(geom):
    H, W, K, heads = geom
    row = T.Row(f"batch-{H}x{W}-k{K}", "b", 3, H, W, heads, K)
    o = T.operands(row)
    for storage in STORAGES:
        three = _run(row, o, storage)
        for i in range(3):
            alone = _run(row._replace(B=1), (o[0][i:i + 1].contiguous(),) + o[1:], storage)
            P._first_diff(three[i:i + 1].contiguous(), alone, f"{row.id} {storage}: image {i} of three against the image alone")


def test_nat_attn_refusals():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    ops = _ops()
    row = T.Row("refuse", "b", 1, 8, 8, 1, 7)
    qkv, kv_pad, table = T.operands(row)
    with pytest.raises(_abi.VipError, match="kernel_size 3, 5 or 7"):
        ops.nat_attention(P.dev16(qkv), P.dev32(kv_pad), P.dev32(torch.zeros(1, 289)), 1, 9)
    with pytest.raises(_abi.VipError, match="head_dim"):
        ops.nat_attention(P.dev16(qkv[..., :48].contiguous()), None, P.dev32(table), 1, 7)
    with pytest.raises(_abi.VipError, match="table"):
        ops.nat_attention(P.dev16(qkv), P.dev32(kv_pad), P.dev32(table[:, :-1].contiguous()), 1, 7)
    with pytest.raises(_abi.VipError, match="kv_pad"):
        ops.nat_attention(P.dev16(qkv), P.dev32(kv_pad[:-1].contiguous()), P.dev32(table), 1, 7)
