"""tests/_gemm_exact_cases.py without a GPU: condition EXACT per output element of every row, operand planes free of fp16 subnormals, the
weights untouched by the weight constructors, the carrier channels really leave accumulators that are no fp16 values, every row is sent
to the kernel and the instantiation it names (the dispatcher's dry run), the table covers what it says it covers, and the operands tell
a wrong geometry, a premature rounding and a dropped term apart from the reference - on a CPU emulation of the kernels' rounding points
(fp32 sums, the epilogue order of epilogue<> / pw_epilogue<> / h2_store8<> in csrc/conv_igemm.hip).

The rounding mutants M1 - M4 also PASS tests/test_gpu_ops.py's check() on that file's randn operands: the gap the exact rows close.
The bound of the largest shapes is computed here as well: nothing is left to the GPU test's setup."""
import math

import pytest
import torch

import vipcup_amd  # noqa: F401
from vipcup_amd import ops

from tests import _f16_gemm_cases as F16
from tests import _gemm_exact_cases as T
from tests import _h2_gemm_cases as H2
from tests import test_gpu_ops as G
from tests import test_gpu_strict as S

SWITCHES = ("VIP_PW", "VIP_PWX", "VIP_PWK_XLK", "VIP_PWK_WN2K", "VIP_PWK_CONV", "VIP_PWK_FILL", "VIP_G8P_MINK", "VIP_PW_H2_LDS_KB", "VIP_HILO")


@pytest.fixture(autouse=True)
def default_dispatch(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def weight(row, w, b):
    """the ConvWeight of the row's storage, on the host"""
    with ops.precision(T.MODE[row.storage]):
        return ops.make_conv_weight(w.float(), None if b is None else b.float(), groups=row.case[8], device="cpu", hilo=row.hilo)


def rows_of(w, case):
    """HWIO -> the kernels' [Cout, k k Cin_g]"""
    return w.permute(3, 0, 1, 2).reshape(case[4], -1)


def subnormal(p):
    return bool(((p != 0) & (p.abs() < 2.0 ** -14)).any())


def is_multiple(t, g):
    q = t / g
    return bool((q == q.round()).all())


_keys = []
for _r in T.ROWS:
    if (_r.storage, _r.kind, _r.case) not in [k for k, _ in _keys]:
        _keys.append(((_r.storage, _r.kind, _r.case), [q for q in T.ROWS if (q.storage, q.kind, q.case) == (_r.storage, _r.kind, _r.case)]))


def test_geometry_lists_are_those_of_the_gpu_tests():
    assert T.CONV_GEOMS == [(c[:9], bool(c[9]), c[10]) for c in G.CONV_CASES]
    assert [c[:9] for c in S.CONV_CASES[:12]] == [g for g, _, _ in T.CONV_GEOMS]


@pytest.mark.parametrize("key,rows", _keys, ids=[f"{k[0]}-{k[1]}-" + "x".join(str(v) for v in k[2][:7]) for k, _ in _keys])
def test_exact_per_element(key, rows):
    """EXACT for every row of the shape (the bound per output element in fp64), operand planes, the stored weights, the carriers, and
    every expected result representable after its one rounding"""
    row = rows[0]
    op = T.operands(row)
    g = T.granule(row)
    gx = {"gated": 2.0 ** -7, "b": 2.0 ** -13}.get(row.kind, 1.0)
    assert is_multiple(op["xe"], gx) and is_multiple(op["w"], g / gx) and is_multiple(op["b"], g) and is_multiple(op["r"], g)
    for r in rows:
        bd = T.bound(r, op)
        assert float(bd.max()) <= 2.0 ** 24 * g, (r.id, float(bd.max()), 2.0 ** 24 * g)
    # ---- operand planes and stored weights
    cw = weight(row, op["w"], op["b"])
    Kt = row.case[5] ** 2 * row.case[3] // row.case[8]
    if row.storage == "f16":
        stored = cw.w[:, :Kt].double() + (cw.w_lo[:, :Kt].double() if row.hilo else 0.0)
        assert torch.equal(stored, rows_of(op["w"], row.case)), "make_conv_weight must leave these weights alone"
        assert not cw.w[:, Kt:].any()
        planes = [op["x"], cw.w.double(), op["r"]] + ([cw.w_lo.double()] if row.hilo else []) + ([op["gate"]] if row.gated else [])
        if row.hilo:
            assert (cw.w_lo != 0).float().mean() > 0.1 and torch.equal(cw.w[:, :Kt].double(), T.rn16(rows_of(op["w"], row.case)))
        if row.gated:
            gt = op["gate"]
            assert torch.equal(T.rn16(op["x"] * gt[:, 1, None, None, :]), op["x"] * gt[:, 1, None, None, :])
            assert torch.equal(T.rn16(op["xe"]), op["xe"]), "fma(x, hi, x * lo) must stay an fp16 value"
            assert ((gt[:, 0] == 0) & (gt[:, 1] != 0)).any() and ((gt[:, 0] != 0) & (gt[:, 1] != 0)).any()
            assert not (gt[1:] == gt[:-1]).all(dim=(1, 2)).any(), "neighbouring images never share a gate"
    elif row.storage == "h2":
        assert cw.h2_scale == 4096.0
        wh, wl = T.split16(rows_of(op["w"], row.case) * 4096.0)
        st = cw.w.double().reshape(row.case[4], Kt // 8, 2, 8)
        assert torch.equal(st[:, :, 0].reshape(-1, Kt), wh) and torch.equal(st[:, :, 1].reshape(-1, Kt), wl)
        assert torch.equal(wh + wl, rows_of(op["w"], row.case) * 4096.0)
        xh, xl = T.split16(op["x"])
        assert torch.equal(xh + xl, op["x"])
        assert bool(xl.any()) == (row.kind == "b") and bool(wl.any()) == (row.kind == "c")
        planes = [xh, xl, wh, wl, op["r"]]
    else:
        assert torch.equal(cw.w.double(), rows_of(op["w"], row.case))
        p3 = cw.w_bf3[:, :, :Kt].double()
        assert torch.equal(p3.sum(0), rows_of(op["w"], row.case))
        assert [bool(p.any()) for p in p3] == ([True, True, False] if row.kind == "p2" else [True, False, False])
        planes = []
    for p in planes:
        assert not subnormal(p)
    # ---- the results
    for r in rows:
        v = T.ref64(r, op)
        e = T.expected(r, v)
        if r.storage == "f16":
            assert torch.isfinite(e).all()
            if T.has_carriers(r):
                a = T.R.act(op["y"], T.EPI[r.epi][0])
                off = (T.rn16(a) != a).reshape(-1, a.shape[-1]).double().mean(0)
                assert float((off > 0.5).double().mean()) >= 0.2, (r.id, "the accumulators of the carrier channels are fp16 values")
                if T.EPI[r.epi][2] and r.kind == "a":           # (gated rows: g = 2^-9, the result takes a real rounding)
                    assert torch.equal(e.double(), v), "a residual epilogue's result is the small exact value"
        elif r.storage == "h2":
            assert torch.equal(e[0] + e[1], v) and float(v.abs().max()) < 65504 and not subnormal(e[0]) and not subnormal(e[1])
            if r.kind in "bc":
                assert (e[1] != 0).double().mean() > 0.1
        else:
            assert torch.equal(e.double(), v)


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------------------
_ldw = {}


def desc_of(row):
    B, H, W, Cin, Cout, k, s, pad, groups = row.case
    key = (row.storage, k, Cin // groups, Cout, groups, row.hilo)
    if key not in _ldw:
        cw = weight(row, torch.zeros(k, k, Cin // groups, Cout), None)
        _ldw[key] = (cw.ldw, cw.w_lo is not None)
    ldw, lo = _ldw[key]
    act, post, res = T.EPI[row.epi]
    d, _ = F16.conv_desc(row.case + (act, res), ldw)
    d.act_post = ops._act(post)
    if row.slice:
        name, ld, off = row.slice
        if name == "ldx":
            d.ldx, d.cin_off = ld, off
        elif name == "ldy":
            d.ldy, d.cout_off = ld, off
        else:
            d.ldr, d.res_off = ld, off
    return d, res, lo


@pytest.mark.parametrize("row", [r for r in T.ROWS if r.storage != "s32"], ids=lambda r: r.id)
def test_row_selects_its_kernel(row):
    d, res, lo = desc_of(row)
    assert lo == row.hilo
    if row.storage == "f16":
        name, variant = ops.conv_kernel_name(d, res, row.gated, lo), ops.conv_kernel_variant(d, res, row.gated, lo)
    else:
        name, variant = ops.conv_kernel_name_h2(d, res), ops.conv_kernel_variant_h2(d, res)
    assert (name, variant) == (row.kernel, row.variant), (row.id, row.what)


def test_fp32_rows_name_the_arithmetic_ops_selects():
    assert {(r.kernel, r.variant) for r in T.ROWS if r.storage == "s32"} == {("sconv6_kernel", "bf16x3"), ("sconv_kernel", "f32")}
    assert all(r.kernel == "sconv6_kernel" for r in T.ROWS if r.kind == "p2")


def test_table_covers_what_it_names():
    f16 = {F16.instantiation(r.variant) for r in T.ROWS if r.storage == "f16"}
    assert f16 >= F16.INSTANTIATIONS, F16.INSTANTIATIONS - f16
    h2 = {F16.instantiation(r.variant) for r in T.ROWS if r.storage == "h2"}
    assert h2 >= T.H2_INSTANTIATIONS, T.H2_INSTANTIATIONS - h2
    # every pointwise instantiation of the tables with its four epilogue families, conv_igemm_kernel with an activation and a residual
    for st, table in (("f16", F16._DENSE_ROWS), ("h2", H2._DENSE_ROWS)):
        for inst in {F16.instantiation(r[5]) for r in table}:
            assert {r.epi for r in T.ROWS if r.storage == st and F16.instantiation(r.variant) == inst} >= set(T.POINTWISE), (st, inst)
    for inst in ("conv_igemm<64,64>", "conv_igemm<128,64>", "conv_igemm<64,128>", "conv_igemm<128,128>"):
        assert any(r.epi == "relu_res" and r.variant == inst for r in T.ROWS if r.storage == "f16"), inst
    # packed: the three operand kinds on every instantiation of its table
    for inst in {F16.instantiation(r[5]) for r in H2._DENSE_ROWS}:
        assert {r.kind for r in T.ROWS if r.storage == "h2" and F16.instantiation(r.variant) == inst} == {"a", "b", "c"}, inst
    assert {r.case[0] for r in T.ROWS if r.kernel == "rows_gemm_kernel" and T.is_dense(r)} >= {1, 37, 256}

    def geo(c):
        return c[5], c[6], c[7], c[8]
    have = {st: {geo(r.case) for r in T.GEO_ROWS if r.storage == st} for st in ("f16", "h2", "s32")}
    assert have["f16"] >= {geo(c) for c in G.CONV_CASES} | {geo(c[0]) for c in F16.CONV_F16_CASES}
    assert have["h2"] >= {geo(c) for c in G.CONV_CASES} | {geo(c[0]) for c in H2.CONV_H2_CASES}
    assert have["s32"] >= {geo(c) for c in G.CONV_CASES}
    for st in have:
        assert have[st] >= {(3, 1, (0, 2, 2, 0), 1), (5, 1, (2, 2, 2, 2), 1), (3, 1, (1, 1, 1, 1), 2)}
        assert {r.slice[0] for r in T.ROWS if r.storage == st and r.slice} == {"ldx", "ldy", "ldr"}
    small = [r.case for r in T.GEO_ROWS if r.case[1] < r.case[5] and r.case[2] < r.case[5]]
    assert small and all(c[1:3] == (3, 4) and c[5] == 5 for c in small)
    assert any(r.case[8] == 2 and (r.case[4] // 2) % 64 for r in T.GEO_ROWS)


# ---- geometry mutants ---------------------------------------------------------------------------------------------------------------------------
_geo_keys = [(k, rows) for k, rows in _keys if rows[0] in T.GEO_ROWS]


@pytest.mark.parametrize("key,rows", _geo_keys, ids=[f"{k[0]}-{k[1]}-" + "x".join(str(v) for v in k[2][:7]) for k, _ in _geo_keys])
def test_geometry_mutants_change_every_row(key, rows):
    row = rows[0]
    op = T.operands(row)
    applied = 0
    for name, applies, mutant in T.GEOMETRY_MUTANTS:
        if not applies(row.case):
            continue
        y = mutant(op, row.case)
        assert y.shape == op["y"].shape, name
        for r in rows:
            e, m = T.expected(r, T.ref64(r, op)), T.expected(r, T.epilogue64(y, op["r"], r.epi))
            same = all(torch.equal(a, b) for a, b in zip(e, m)) if r.storage == "h2" else torch.equal(e, m)
            assert not same, (r.id, name)
        applied += 1
    assert applied >= 1


def test_every_geometry_mutant_applies_somewhere():
    for name, applies, _ in T.GEOMETRY_MUTANTS:
        assert sum(1 for r in T.GEO_ROWS if applies(r.case)) >= 3, name


# ---- numeric mutants ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in T.ROWS if r.storage == "f16"], ids=lambda r: r.id)
def test_f16_rounding_points_and_dropped_terms(row):
    """the emulation with the kernels' rounding points IS the reference; each mutant differs from it on every row it applies to"""
    op = T.operands(row)
    good = T.emulate_f16(row, op)
    n = good.shape[0]
    assert torch.equal(good, T.expected(row, T.ref64(row, op)).reshape(-1, good.shape[1])[:n])
    for m in ("M1", "M2", "M3", "M4", "M5", "M6"):
        if T.mutant_applies(row, m):
            assert not torch.equal(T.emulate_f16(row, op, m), good), (row.id, m)


@pytest.mark.parametrize("row", [r for r in T.ROWS if r.storage == "h2"], ids=lambda r: r.id)
def test_h2_dropped_terms_and_output_split(row):
    op = T.operands(row)
    hi, lo = T.emulate_h2(row, op)
    n = hi.shape[0]
    eh, el = T.expected(row, T.ref64(row, op))
    assert torch.equal(hi, eh.reshape(-1, hi.shape[1])[:n]) and torch.equal(lo, el.reshape(-1, hi.shape[1])[:n])
    for m in ("M7a", "M7b", "M7c", "M8"):
        if T.h2_mutant_applies(row, m):
            mh, ml = T.emulate_h2(row, op, m)
            assert not (torch.equal(mh, hi) and torch.equal(ml, lo)), (row.id, m)


def test_mutant_names_apply_to_rows():
    for m in ("M1", "M2", "M3", "M4", "M5", "M6"):
        assert sum(1 for r in T.ROWS if r.storage == "f16" and T.mutant_applies(r, m)) >= 6, m
    for m in ("M7a", "M7b", "M7c", "M8"):
        assert sum(1 for r in T.ROWS if r.storage == "h2" and T.h2_mutant_applies(r, m)) >= 20, m


# ---- the gap: M1 - M4 pass the old metric on the old operands ---------------------------------------------------------------------------------
def _rn(t):
    return t.to(torch.float16).to(torch.float32)


def test_rounding_mutants_pass_check_on_randn_operands(report):
    """test_gpu_ops.check() - 2e-3 of the absmax of the whole output - on dense_operands' randn inputs at the table shape (3000, 1240, 56)
    with a residual: an accumulator rounded to fp16 before the residual add (M1), the bias added in fp16 (M2) and fp16 partial sums
    between the 64-k chunks (M3) all pass it.  The measured relative errors go to the report."""
    M, K, N = 3000, 1240, 56
    assert any(r[:3] == (M, K, N) for r in F16._DENSE_ROWS)
    x, w, b, res, y = G.dense_operands(M, K, N)
    ref = y + res
    nob = x @ w
    m3 = torch.zeros(M, N)
    for c0 in range(0, K, 64):
        m3 = _rn(m3 + x[:, c0:c0 + 64] @ w[c0:c0 + 64])
    got = {"M1": _rn(_rn(y) + res), "M2": _rn(_rn(_rn(nob) + b) + res), "M3": _rn(m3 + b + res)}
    for m, t in got.items():
        assert not torch.equal(t, _rn(ref))
        G.check(report, f"gemm-exact gap: mutant {m} on randn operands {M}x{K}x{N} res (passes the old metric)", t, ref)


def test_dropped_gate_plane_passes_check_on_randn_operands(report):
    """test_f16_gated_conv_kernels' operands at its (1333, 72, 40) row with a residual: the gate's lo plane dropped (M4) passes check()"""
    B, K, N = 1333, 72, 40
    assert any(r[:3] == (B, K, N) for r in F16._GATED_ROWS)
    H, W = F16.GATE_HW
    g = torch.Generator().manual_seed(B + K + N)
    x = G.h(torch.randn(B, H, W, K, generator=g))
    gate = torch.rand(B, K, generator=g)
    w = G.h(torch.randn(1, 1, K, N, generator=g) / math.sqrt(K))
    bias = torch.randn(N, generator=g) * 0.1
    res = G.h(torch.randn(B, H, W, N, generator=g))
    hi = _rn(gate)
    lo = _rn(gate - hi)
    ref = G.R.conv2d(G.h(x * (hi + lo)[:, None, None, :]), w, bias, 1, (0, 0, 0, 0), 1) + res
    bad = G.R.conv2d(G.h(x * hi[:, None, None, :]), w, bias, 1, (0, 0, 0, 0), 1) + res
    assert bool(lo.any()) and not torch.equal(_rn(bad), _rn(ref))
    G.check(report, f"gemm-exact gap: mutant M4 (gate lo plane dropped) on randn operands {B}x7x7x{K}->{N} res (passes the old metric)",
            _rn(bad), ref)
