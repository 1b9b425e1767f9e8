"""The LayerNorm-site case table (tests/_ln_site_cases.py) checks itself, without a GPU.

emulate() is the table's forward() in float32 with the kernels' documented rounding points: for the fp16 storage the normalised row, the
hidden activations and the output are rounded to fp16; for the packed storage those three and the weights go through h2_quantise.  For
every case it must stay within A QUARTER of the case's tolerance per row, on every row kind: the inputs, not the kernel, fit the
tolerance.  Every wrong variant, put through the same emulation, must pass the FULL tolerance on some row kind of every case it applies
to (on the first WRONG_ROWS rows - a prefix of what the GPU test holds, so what bites here bites there).  And the reason the table
exists: on the inputs and the whole-tensor metric of tests/test_gpu_ops.py::test_mlp_fused three of the variants are invisible."""
import inspect
import math

import pytest
import torch

from oracle import ops_ref as R
from tests import _ln_site_cases as T
from tests import test_gpu_ln_gemm as G
from tests import test_gpu_passes as P
from tests._helper_cases import h2_quantise

WRONG_ROWS = 7 * 64          # 64 rows of every kind, 28 MFMA tiles


def _h(t):
    return t.half().float()


def emulate(case, o, wrong=None):
    if case.storage == "f16":
        return T.forward(case, o, wrong, torch.float32, q=_h)
    return T.forward(case, o, wrong, torch.float32, q=h2_quantise, qw=h2_quantise)


def _head(o, n):
    return {k: (v[:n] if k in ("x", "res") else v) for k, v in o.items()}


def _fmt(worst):
    return ", ".join(f"kind {k}: {e:.2e} (row {r} ch {c})" for k, (e, r, c) in enumerate(worst))


def test_table_is_well_formed():
    ids = [c.id for c in T.CASES]
    assert len(set(ids)) == len(ids)
    assert {(c.site, c.kernel) for c in T.CASES} == set(T.KERNELS)
    for c in T.CASES:
        assert c.what and c.eps in T.EPS and c.tol in T.TOLERANCES, c.id
        assert c.tol == ("TOL_MLP_F16" if c.storage == "f16" else "TOL_OP"), c.id
        assert c.M % 16 and c.M % c.tile, c.id                                       # ragged against the MFMA tile and the workgroup's
        assert (c.kernel is None) == (c.route != "fused"), c.id
        assert c.C % 8 == 0 and (c.site == "ln_dense" or c.C % 32 == 0), c.id
    for eps in T.EPS:
        for res in (False, True):
            mine = [c for c in T.MLP_CASES if c.eps == eps and c.res == res]
            assert {(c.C, c.N) for c in mine if c.storage == "f16" and c.route == "fused"} == {(64, 256), (96, 384), (192, 768), (192, 96)}
            assert {(c.C, c.N) for c in mine if c.storage == "h2" and c.route == "fused"} == {(64, 256), (96, 384), (128, 384)}
            assert {(c.C, c.M) for c in mine if c.route == "small"} == {(96, 37), (192, 37)}
            assert {c.C for c in mine if c.route == "unfused" and c.storage == "f16"} == {96, 192}
            assert all(c.M == 8192 + 37 for c in mine if c.route != "small")
        for mode in T.LN_MODES:
            mine = [c for c in T.LN_DENSE_CASES if c.eps == eps and c.mode == mode]
            assert [(c.C, c.N) for c in mine] == [(72, 256), (128, 256), (136, 256), (200, 1024), (256, 512), (320, 384), (384, 1152)]
            assert all(c.M == 16384 + 37 and c.res == (mode == "res") for c in mine)
    assert T.ln_chunks(72) == (2, 56) and T.ln_chunks(136) == (3, 56) and T.ln_chunks(200) == (4, 56) and T.ln_chunks(384) == (6, 0)
    assert T.MILDER == {}


def test_no_tolerance_is_new():
    assert T.TOLERANCES == {"TOL_MLP_F16": P.TOL_MLP_F16, "TOL_OP": P.TOL_OP} and P.TOL_MLP_F16 == 4e-3 and P.TOL_OP == 2e-5
    assert "tol=4e-3" in inspect.getsource(G.test_ln_dense_vs_oracle)


def test_shapes_are_what_the_library_takes():
    """the dry runs of the launchers (host arithmetic): the fused widths are supported, the small cases are not, M is ragged against
    the tile of the plan where the plan needs no device"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ops
    lib = _abi.lib()
    for c in T.MLP_CASES:
        sup = lib.vip_mlp_fused_supported_h2 if c.storage == "h2" else lib.vip_mlp_fused_supported
        assert bool(sup(c.M, c.C, c.N, 3)) == (c.route != "small"), c.id
        if c.route != "fused":
            continue
        try:
            plan = ops.mlp_plan(c.M, c.C, c.N, packed=c.storage == "h2")
        except Exception:                                                             # the plan asks the device for its CU count
            plan = None
        if plan is not None:
            tiles, _, tile = plan
            assert c.M % tile and T.MOVE_TILE % tile == 0 and tiles == -(-c.M // tile), (c.id, plan)
    for c in T.LN_DENSE_CASES:
        assert 64 < c.C <= 384 and c.N >= 256 and c.M >= 16384, c.id                  # vip_ln_gemm_supported's capability terms
        assert c.M % 128, c.id                                                        # pwx_ln_kernel: 128 rows per workgroup


def test_rows_are_what_the_table_says():
    g = torch.Generator().manual_seed(1)
    for storage in ("f16", "h2"):
        x = T.structured_rows(g, 70, 96, storage).double()
        for r in range(70):
            row, k = x[r], r % 7
            if k == 2:
                assert row.sum() == 8.0 and row[(7 * r) % 96] == 8.0
            elif k == 4:
                assert (row == (5 * r) % 9 - 4).all()
            else:
                mean, std = {0: (96, 64), 1: (-1.5, 1), 3: (100 if storage == "f16" else 16, 0.25), 5: (0, 2 ** -6), 6: (0, 2 ** -10)}[k]
                assert abs(row.mean() - mean) < 0.5 * std and 0.7 * std < row.std() < 1.4 * std, (storage, r)
            on16 = torch.equal(row.half().double(), row)
            assert on16 if (storage == "f16" or k in (2, 3, 4)) else not on16, (storage, r)
        assert torch.equal(h2_quantise(x.float()).double(), x)
    o = T.operands(T.BY_ID["mlp-f16-c96-h384-eps1e-6-res"])
    assert torch.equal(o["gamma"] * 4, (o["gamma"] * 4).round()) and 0.5 <= o["gamma"].min() and o["gamma"].max() <= 2
    assert torch.equal(o["beta"] * 4, (o["beta"] * 4).round()) and -2 <= o["beta"].min() and o["beta"].max() <= 2
    assert torch.equal(_h(o["w1"]), o["w1"]) and torch.equal(_h(o["res"]), o["res"]) and not torch.equal(o["res"], o["x"])
    assert o is T.operands(T.BY_ID["mlp-f16-c96-h384-eps1e-5-nores"])                # one shape, one set of operands
    # variance 0: the reference of a constant row is the MLP of beta, whatever the constant
    c = T.BY_ID["ln_dense-f16-k72-n256-none-eps1e-6"]
    o = T.operands(c)
    ref = T.reference(c, o)
    assert (ref[4::7] - R.dense(o["beta"].double(), o["w1"].double(), o["b1"].double())).abs().max() < 1e-12


@pytest.mark.parametrize("M,tile", [(T.M_SMALL, 16), (T.M_MLP, T.MOVE_TILE), (T.M_LN, T.MOVE_TILE)])
def test_move_rows_changes_every_tile(M, tile):
    p = T.move_rows(M, tile)
    assert torch.equal(p.sort().values, torch.arange(M))
    assert (p // tile != torch.arange(M) // tile).all()
    assert (p // 16 != torch.arange(M) // 16).all()
    assert torch.equal(p, T.move_rows(M, tile))                                      # fixed
    assert ((p[1:] - p[:-1]).abs() == 1).float().mean() < 0.3                        # and the neighbours change


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_emulation_fits_and_every_wrong_variant_bites(case):
    o = T.operands(case)
    ref = T.reference(case, o)
    assert torch.isfinite(ref).all()
    tol = T.tolerance(case)
    worst = T.worst_by_kind(emulate(case, o), ref)
    assert max(e for e, _, _ in worst) <= tol / 4, f"{case.id}: the emulation leaves a quarter of {tol}: {_fmt(worst)}"
    n = min(WRONG_ROWS, case.M)
    oh, refh = _head(o, n), ref[:n]
    for wrong in T.WRONG:
        if not T.applies(case, wrong):
            continue
        bad = T.worst_by_kind(emulate(case, oh, wrong), refh)
        caught = [k for k, (e, _, _) in enumerate(bad) if e > tol]
        assert caught, f"{case.id}: no row kind tells apart '{wrong}': {_fmt(bad)}"
        # and the reference function's own wrong= form moves by more than the tolerance too
        moved = T.worst_by_kind(T.reference(case, oh, wrong), refh)
        assert any(e > tol for e, _, _ in moved), f"{case.id}: reference(wrong='{wrong}') stays within {tol}: caught by kinds {caught}"


def test_padding_variants_apply_where_padding_exists():
    for c in T.CASES:
        pad = T.padded(c) != c.C
        assert pad == (c.site == "ln_dense" and c.C in (72, 136, 200)), c.id
        assert T.applies(c, T.PAD_DIV) == T.applies(c, T.PAD_SQ) == pad
        assert all(T.applies(c, w) for w in T.WRONG if w not in (T.PAD_DIV, T.PAD_SQ))


@pytest.mark.parametrize("M,C,hid", [(8192, 96, 384), (9001, 192, 768)])
def test_existing_inputs_and_metric_do_not_see_them(M, C, hid):
    """the witness: the inputs of tests/test_gpu_ops.py::test_mlp_fused (use_ln, use_res), its fp32 oracle and its metric max|err| /
    max|ref| over the whole tensor at 4e-3 - a one-pass variance, a dropped eps and an eps of 1e-5 for 1e-6 all pass"""
    g = torch.Generator().manual_seed(M + C + hid)
    x = _h(torch.randn(M, C, generator=g) * 1.5 + 0.3)
    w1 = _h(torch.randn(C, hid, generator=g) / math.sqrt(C))
    b1 = torch.randn(hid, generator=g) * 0.1
    w2 = _h(torch.randn(hid, C, generator=g) / math.sqrt(hid))
    b2 = torch.randn(C, generator=g) * 0.1
    res = _h(torch.randn(M, C, generator=g))
    lg, lb = torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.1
    ref = R.dense(R.act(R.dense(R.layernorm(x, lg, lb, 1e-6), w1, b1), "gelu"), w2, b2) + res
    case = T.Case("existing", "mlp", "f16", "fused", "", C, hid, M, 1e-6, True, "gelu", 512, "TOL_MLP_F16", "")
    o = dict(x=x, gamma=lg, beta=lb, w1=w1, b1=b1, w2=w2, b2=b2, res=res)
    scale = ref.abs().max().item() + 1e-6
    right = (emulate(case, o) - ref).abs().max().item() / scale
    assert right < 4e-3
    for wrong in (T.ONE_PASS, T.NO_EPS, T.OTHER_EPS):
        err = (emulate(case, o, wrong) - ref).abs().max().item() / scale
        assert err < 4e-3 and err < 1.5 * right, (wrong, err, right)
