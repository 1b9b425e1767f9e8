"""The helper case table (tests/_helper_cases.py) checks itself, without a GPU: the operands sit on the exact grid and make the reference
representable in the row's storage, every quotient a pooling kernel can form rounds to the same fp16 however the fp32 kernel divides,
every row names a kernel of the two files and every helper kernel of the two files is named, the second-pass rows pass the grid cap, no
tolerance is new, the LayerNorm rows reach the lanes-per-row / chunks-per-lane cases they claim, and each classic mistake moves some row's
reference by more than the row accepts."""
import ast
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from tests import _helper_cases as T
from tests import test_gpu_passes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vip-cup-2022_amd", "csrc")
SMALL = [r for r in T.ROWS if not r.p.get("big")]
BIG = [r for r in T.ROWS if r.p.get("big")]
EXACT = [r for r in SMALL if r.accept in ("exact", "round16")]

_CASE = {}


def _case(row):
    """(operands, reference) of a row, computed once"""
    if row.id not in _CASE:
        o = T.operands(row)
        _CASE[row.id] = (o, T.reference(row, o))
    return _CASE[row.id]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_table_is_well_formed():
    ids = [r.id for r in T.ROWS]
    assert len(set(ids)) == len(ids)
    for r in T.ROWS:
        assert r.what and r.op and isinstance(r.p, dict), r.id
        assert r.storage in T.STORAGES + ("f32",), r.id
        assert (r.storage, r.kernel) in T.KERNELS, r.id
        assert r.accept in ("exact", "round16") or r.accept in T.TOLERANCES, r.id
        assert r.accept != "round16" or r.storage == "f16", r.id


def test_every_helper_kernel_is_named():
    """the literal T.KERNELS against the __global__ functions of the two files, and against the rows"""
    found = {}
    for f in ("pointwise.hip", "strict_ops.hip"):
        found[f] = set(re.findall(r"__global__\s+__launch_bounds__\(\d+\)\s+void\s+(\w+)\(", _src(f)))
    assert len(found["pointwise.hip"]) == 14 and len(found["strict_ops.hip"]) == 13, found        # a new kernel changes the count
    mine = {k for _, k in T.KERNELS}
    assert (found["pointwise.hip"] | found["strict_ops.hip"]) - T.ELSEWHERE == mine
    assert not mine & T.ELSEWHERE
    named = {(r.storage, r.kernel) for r in T.ROWS}
    assert named == set(T.KERNELS), set(T.KERNELS) ^ named
    strict = found["strict_ops.hip"] - T.ELSEWHERE - {"h2_layernorm_kernel"}                      # the storage templates: both storages
    for k in strict:
        assert ("h2", k) in named and ("s32", k) in named, k


def _tolerance_key(row):
    if row.op == "gap":
        return "gap_split"
    if row.op == "head":
        return row.p["kind"]
    return row.p["kind"]


def test_no_tolerance_is_new():
    assert P.TOL_F16 == 2e-3 and P.TOL_OP == 2e-5
    with open(os.path.join(ROOT, "tests", "test_gpu_ops.py")) as f:
        text = f.read()
    funcs = {n.name: ast.get_source_segment(text, n) for n in ast.walk(ast.parse(text)) if isinstance(n, ast.FunctionDef)}
    needle = {"gap_dense": "gap_dense_f32", "gap_ln_dense": "gap_ln_dense_f32", "gap_split": "global_avgpool split", "ensemble_mean": "ensemble_mean",
              "head_prob": "head_prob", "head_act": "head_prob"}        # head_act: the issue's 2e-6 of head_prob (no GPU test called it before)
    for name, (module, users) in T.TOLERANCES.items():
        if module == "test_gpu_passes":
            assert isinstance(getattr(P, name), float)
            continue
        for op, fn in users.items():
            assert f"tol={name}" in funcs[fn] and needle[op] in funcs[fn], (name, op, fn)
    for r in T.ROWS:
        if r.accept in ("exact", "round16"):
            continue
        module, users = T.TOLERANCES[r.accept]
        if module == "test_gpu_passes":
            assert r.accept == T.TOL_OF[r.storage], r.id                 # the storage's own tolerance
        else:
            assert _tolerance_key(r) in users, r.id
        assert T.tolerance(r, P) in (2e-3, 2e-5, 1e-5, 1e-6, 2e-6), r.id


def test_second_pass_rows_pass_the_grid_cap():
    """grid_for (pointwise.hip) and sgrid (strict_ops.hip) cap the grid at 256 * 32 = 8192 workgroups of 256 threads"""
    for f, fn in (("pointwise.hip", "grid_for"), ("strict_ops.hip", "sgrid")):
        body = re.search(r"inline unsigned " + fn + r"\(long total\) \{(.*?)\n\}", _src(f), re.S).group(1)
        assert "(total + 255) / 256" in body and "if (g > 256L * 32) g = 256L * 32;" in body, fn
    assert T.GRID_CAP == 256 * 32 * 256 == 2097152
    assert {(r.op, r.storage) for r in BIG} == {(op, st) for op in ("pool2d", "scale_add_act", "mul", "radix_combine") for st in T.STORAGES}
    for r in BIG:
        p = r.p
        if r.op == "pool2d":
            Ho, Wo = T.pool_out_hw(p)
            n = p["B"] * Ho * Wo * p["C"]
            assert p["k"] == 1 and p["stride"] == 1
        elif r.op == "scale_add_act":
            n = math.prod(p["shape"])
        elif r.op == "mul":
            n = p["rows"] * p["C"]
        else:
            n = p["B"] * p["HW"] * p["C"]
        chunks = n // T.CHUNK[r.storage]
        assert T.GRID_CAP < chunks < 2 * T.GRID_CAP, (r.id, chunks)        # a ragged second pass
        assert str(chunks) in r.what, r.id


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------
def _on_grid(t, unit, lo, hi):
    return torch.equal(t / unit, (t / unit).round()) and lo <= t.min().item() and t.max().item() <= hi


def _fits(row, ref):
    """the reference is representable in the storage the row's output has"""
    if row.op in ("head", "score") or row.storage == "s32":
        return torch.equal(ref.float().double(), ref)
    return torch.equal(T.round16(ref), ref)                               # fp16; packed: hi = the value, the lo plane is 0


@pytest.mark.parametrize("row", EXACT, ids=lambda r: r.id)
def test_reference_is_exact(row):
    o, ref = _case(row)
    p = row.p
    refs = ref if isinstance(ref, tuple) else (ref,)
    if row.accept == "exact":
        for t in refs:
            assert _fits(row, t), "the reference leaves the storage's grid"
    if row.op in ("pool2d", "gap"):
        assert _on_grid(o["x"], 1, -4, 4)
        # integer sums of at most 143 (9) terms: exact in any order; the quotient: test_quotients_round_alike
        return
    if row.op == "scale_add_act":
        assert _on_grid(o["x"], 1, -4, 4)
        assert o["r"] is None or _on_grid(o["r"], 1, -4, 4)
        assert o["hi"] is None or _on_grid(o["hi"], 0.25, 0, 2)
        assert o["lo"] is None or _on_grid(o["lo"], T.LO_UNIT, -4 * T.LO_UNIT, 4 * T.LO_UNIT)
        lin = T.saa_ref(o, dict(p, act=None, act2=None))[0]
        assert _on_grid(lin, T.LO_UNIT, -16, 16)                          # < 2^18 units of 2^-14: one exact fp32 value, no rounding before the store
        if o["lo"] is not None:                                            # x * lo alone where hi = 0 and the residual is 0: representable in fp16
            quiet = lin[..., ::3]
            assert torch.equal(quiet, (o["x"].double() * o["lo"].double()[:, None, :])[..., ::3]) and (quiet != 0).any()
            assert torch.equal(T.round16(quiet), quiet)
        if row.accept == "exact" and o["hi"] is not None:
            assert len({tuple(s.tolist()) for s in o["hi"]}) == p["shape"][0], "two images share a gate"
        return
    if row.op == "mul":
        assert _on_grid(o["a"], 1, -4, 4) and _on_grid(o["b"], 0.25, 0, 2)
        assert len({p["lda"], p["ldb"], p["ldy"]}) == 3 and p["a_off"] and p["b_off"] and p["y_off"]
        return
    if row.op == "radix_combine":
        assert _on_grid(o["x"], 1, -4, 4) and _on_grid(o["hi"], 0.25, 0, 2)
        worst = T.radix_ref(dict(x=o["x"].abs(), hi=o["hi"], lo=None if o["lo"] is None else o["lo"].abs()), p)
        assert worst.max().item() / T.LO_UNIT < 2 ** 24                    # every partial sum: exact in fp32 in any order
        if o["lo"] is not None:
            B, HW, Cc, radix = p["B"], p["HW"], p["C"], p["radix"]
            quiet = ref[..., ::3]
            assert (o["hi"].reshape(B, radix, Cc)[..., ::3] == 0).all() and (quiet != 0).any() and torch.equal(T.round16(quiet), quiet)
        return
    if row.op == "layernorm":
        assert p["kind"] == "const" and _on_grid(o["x"], 1, -4, 4) and _on_grid(o["gamma"], 0.25, 0.5, 2) and _on_grid(o["beta"], 0.25, -2, 2)
        assert all(len(set(r.tolist())) == 1 for r in o["x"])
        assert torch.equal(ref, o["beta"].double().expand_as(ref))        # the centred values are 0: the output is beta
        # fp32: the row sum c * C <= 4 * 4096 is exact in any order and c * C / C = c is an exact quotient
        assert torch.equal((o["x"].sum(-1) / p["C"]), o["x"][:, 0])
        return
    if row.op == "head":
        assert _on_grid(o["x"], 1, -4, 4) and _on_grid(o["w"], 0.25, -2, 2) and (o["bias"] is None or _on_grid(o["bias"], 0.25, -2, 2))
        assert p["HW"] in (1, 4) and p["kind"] in ("gap_dense", "cls_dense")
        x = o["x"][:, :1] if p["kind"] == "cls_dense" else o["x"]
        worst = (x.abs().double().sum(1) / p["HW"]) @ o["w"].abs().double().t() + 2
        assert worst.max().item() * 16 < 2 ** 24                           # units of 1/16: every partial sum is exact in fp32 in any order
        return
    if row.op == "score":
        k = p["kind"]
        if k == "ensemble_mean":
            assert _on_grid(o["s"], 2.0 ** -10, 0, 1) and p["M"] in (1, 8)   # sums of 8 below 2^14 units, / 8 exact
        elif k == "head_act" and p["act"] == "softmax":
            assert p["N"] == 1 and torch.equal(ref, torch.ones_like(ref))
        return
    raise AssertionError(row.op)


def _alike(sums, d):
    """every integer sum over divisor d rounds to the same fp16 from: the exact quotient, fp32 division, multiplication by the rounded fp32
    reciprocal, and anything within 2 ulp32 of the fp32 quotient"""
    s = np.asarray(sums, dtype=np.float64)
    want = (s / d).astype(np.float16)
    q = s.astype(np.float32) / np.float32(d)
    forms = [q, s.astype(np.float32) * (np.float32(1) / np.float32(d))]
    up, dn = q, q
    for _ in range(2):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        forms += [up, dn]
    return all(np.array_equal(f.astype(np.float16), want) for f in forms)


def test_quotients_round_alike():
    """the "round16" claim, for exactly the divisors and pixel counts the table uses"""
    divisors = set().union(*(T.pool_divisors(r.p) for r in SMALL if r.op == "pool2d"))
    assert divisors == {1, 2, 4, 6, 9}, divisors
    for d in sorted(divisors):
        assert _alike(range(-4 * d, 4 * d + 1), d), d                      # |sum| <= 4 * taps
    counts = {r.p["HW"] for r in SMALL if r.op == "gap"}
    assert counts == set(T.GAP_HW) == {1, 5, 31, 32, 33, 49, 65, 143}
    for n in sorted(counts):
        assert _alike(range(-4 * n, 4 * n + 1), n), n
    # the rows that ARE held without a tolerance in the 22 / 24 bit storages divide by a power of two only
    for r in SMALL:
        if r.storage != "f16" and r.accept == "exact":
            if r.op == "pool2d":
                assert all(T._dyadic(d) for d in T.pool_divisors(r.p)), r.id
            if r.op == "gap":
                assert T._dyadic(r.p["HW"]), r.id
    for r in SMALL:                                                          # and nothing dyadic hides behind a tolerance
        if r.op == "pool2d" and r.accept == "TOL_OP":
            assert not all(T._dyadic(d) for d in T.pool_divisors(r.p)), r.id


def test_pool_reference_is_the_oracle():
    """pool_ref (explicit Ho, Wo, pt, pl, as the entry points take them) against oracle/ops_ref.py where that has the operator"""
    for rid, fn in (("pool-f16-k2s2-odd-m1", lambda x, p: R.avgpool_same(x, 2, 2)),
                    ("pool-f16-k3s2-odd-m0", lambda x, p: R.maxpool_valid(x, p["k"], p["stride"], p["pad"])),
                    ("pool-f16-max-negative-m0", lambda x, p: R.maxpool_valid(x, p["k"], p["stride"], p["pad"])),
                    ("pool-f16-k3s2-even-m2", lambda x, p: R.avgpool_valid(x, p["k"], p["stride"], p["pad"])),
                    ("pool-f16-k1-pad-m0", lambda x, p: R.zero_pad(x, p["pad"])),
                    ("pool-f16-k1-crop-m0", lambda x, p: x[:, :4, :3])):
        row = T.BY_ID[rid]
        o, ref = _case(row)
        want = fn(o["x"].double(), row.p)
        assert ref.shape == want.shape and (ref - want).abs().max().item() < 1e-14, rid
    neg = _case(T.BY_ID["pool-f16-max-negative-m0"])[1]
    assert (neg[:, 0] == 0).all() and (neg[:, :, 0] == 0).all() and (neg < 0).any()       # the border is the padded zero, the interior is not
    assert (_case(T.BY_ID["pool-f16-max-positive-m0"])[1] > 0).all()
    _, cnt = T.pool_ref(torch.zeros(1, 2, 2, 1), T.BY_ID["pool-f16-avg-small-m1"].p)
    assert (cnt == 4).all()


def test_rows_hold_the_values_the_issue_lists():
    for st in T.STORAGES:
        pool = [r for r in T.ROWS if r.op == "pool2d" and r.storage == st]
        assert {r.p["C"] for r in pool if not r.p["big"]} == {8, 24, 136} and all(r.p["B"] == 3 for r in pool)
        assert {(r.p["k"], r.p["stride"], r.p["mode"]) for r in pool} >= {(3, 2, m) for m in (0, 1, 2)} | {(2, 2, 1), (3, 1, 1), (1, 1, 0)}
        assert any(r.p["ldx"] == r.p["C"] + 8 and r.p["ldy"] == r.p["C"] + 16 for r in pool)
        assert any(r.p["out_hw"] for r in pool)
        saa = [r for r in SMALL if r.op == "scale_add_act" and r.storage == st]
        assert {(bool(r.p["scale"]), r.p["res"], r.p["act"]) for r in saa} >= {(s, x, a) for s in (False, True) for x in (False, True)
                                                                                   for a in (None, "relu", "silu", "gelu", "sigmoid")}
        assert any(r.p["act2"] == "relu" for r in saa)
        assert any(r.p["scale"] == "split" for r in saa) == (st == "f16")
        rad = [r for r in SMALL if r.op == "radix_combine" and r.storage == st]
        assert {(r.p["radix"], r.p["C"]) for r in rad} == {(x, c) for x in (1, 2, 4) for c in (8, 40)}
        assert any(r.p["planes"] == 2 for r in rad) == (st == "f16")
        ln = [r for r in T.ROWS if r.op == "layernorm" and r.storage == st]
        assert {r.p["C"] for r in ln} >= {8, 24, 96, 136, 520, 1032, 1536, 2040, 2048} and {r.p["rows"] for r in ln} == {1, 37}
        heads = [r for r in T.ROWS if r.op == "head" and r.storage == st]
        for kind in ("gap_dense", "gap_ln_dense"):
            mine = [r.p for r in heads if r.p["kind"] == kind]
            assert {p["C"] for p in mine} == {8, 264, 2056, 4096} and {p["HW"] for p in mine} == {1, 4, 49}
            for Cc in T.HEAD_C:
                assert {p["N"] for p in mine if p["C"] == Cc} == {1, 5} and {p["bias"] for p in mine if p["C"] == Cc} == {True, False}
        assert any(r.p["ldx"] for r in heads) and any(r.p["kind"] == "cls_dense" for r in heads)
    gap = [r for r in T.ROWS if r.op == "gap"]
    assert {(r.storage, r.p["split"]) for r in gap} == {("f16", False), ("f16", True), ("h2", False), ("s32", False)}
    assert {(r.p["HW"], r.p["C"]) for r in gap if not r.p["ldx"]} == {(n, c) for n in T.GAP_HW for c in T.GAP_C}
    sc = [r.p for r in T.ROWS if r.op == "score"]
    assert {(p["B"], p["N"]) for p in sc if p["kind"] == "head_prob"} == {(b, n) for b in (1, 257) for n in (1, 2, 5)}
    assert {p["M"] for p in sc if p["kind"] == "ensemble_mean"} == {1, 7, 8}
    z = T.logits(torch.Generator().manual_seed(0), 257, 5)
    assert torch.isfinite(z).all() and {88.0, -88.0, 100.0, -100.0} <= set(z[:5].flatten().tolist())


def test_layernorm_rows_reach_what_they_claim():
    """lanes per row and chunks per lane, recomputed from the formula of vip_layernorm_f16 / layernorm_impl"""
    for f in ("pointwise.hip", "strict_ops.hip"):
        assert "while (lpr < 64 && lpr < C8) lpr <<= 1;" in _src(f)
    assert "VIP_REQUIRE(cpl <= 4, VIP_ERR_UNSUPPORTED" in _src("pointwise.hip") and "if (cpl8 <= 4) {" in _src("strict_ops.hip")
    seen = {"f16": set(), "h2": set(), "s32": set()}
    for r in T.ROWS:
        if r.op != "layernorm":
            continue
        C8 = r.p["C"] // 8
        lpr = min(64, max(8, 1 << (C8 - 1).bit_length()))
        cpl = -(-C8 // lpr)
        if r.storage == "s32" or cpl > 4:
            t = -(-(r.p["C"] // 4) // 64)
            t = 1 << (t - 1).bit_length()
            assert r.kernel == "slayernorm_kernel" and f"slayernorm_kernel<{t}>" in r.what, r.id
            seen[r.storage].add(("s", t))
        else:
            part = "partial" if C8 % lpr else "full"
            assert f"lpr {lpr} CPL {cpl}, last chunk turn {part}" in r.what, r.id
            assert r.kernel == ("layernorm_kernel" if r.storage == "f16" else "h2_layernorm_kernel"), r.id
            seen[r.storage].add((lpr, cpl, part))
    every = {(64, c, part) for c in (2, 3, 4) for part in ("partial", "full")} | {(8, 1, "partial"), (8, 1, "full"), (16, 1, "partial"), (32, 1, "partial")}
    assert seen["f16"] == every and seen["h2"] == every | {("s", 16)}, seen
    assert seen["s32"] == {("s", t) for t in (1, 2, 4, 8, 16)}, seen["s32"]
    assert T.ln_geometry(2056)[1] == 5 and T.ln_geometry(2048)[1] == 4          # the fp16 entry point rejects 2056


# ---- every classic mistake moves some row -----------------------------------------------------------------------------------------------------
def _bites(row, wrong):
    o, ref = _case(row)
    bad = T.reference(row, o, wrong)
    refs, bads = (ref, bad) if isinstance(ref, tuple) else ((ref,), (bad,))
    for r, b in zip(refs, bads):
        if r.shape != b.shape:
            return True
        if row.accept in ("exact", "round16"):
            if not torch.equal(T.expected(row, b), T.expected(row, r)):
                return True
        elif not torch.isfinite(b).all() or T.rel_error(row, b, r)[0] > T.tolerance(row, P):
            return True
    return False


@pytest.mark.parametrize("wrong", sorted(T.MUTANTS), ids=lambda w: w.replace(" ", "-"))
def test_rows_bite(wrong):
    hit = {}
    for row in SMALL:
        if row.op in T.MUTANTS[wrong] and _bites(row, wrong):
            hit.setdefault((row.op, row.storage), []).append(row.id)
    for op in T.MUTANTS[wrong]:
        for st in T.STORAGES:
            if wrong == "lo plane dropped" and st != "f16":
                continue                                                    # the strict storages have no split form
            assert hit.get((op, st)), f"no {st} {op} row tells apart: {wrong}"
