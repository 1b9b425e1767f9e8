"""The LayerNorm prologues of mlp_fused_kernel, mlp_stream_kernel, mlp_h2_kernel and pwx_ln_kernel - and the launches ops.mlp makes
without them - on the structured rows of tests/_ln_site_cases.py.  Per case:
  * the kernel the table names ran (ops.set_profiler recorder), and on the packed storage ops.h2_check passes;
  * the output is finite and within the case's tolerance of the fp64 reference PER ROW, for every row kind; the worst value per kind goes
    to the report (profiles/ln_sites_fp64.log is such a run);
  * a second launch on the same operands gives the same bits; x and the residual come back untouched;
  * the rows of x (and of the residual) moved by a fixed permutation that takes every row to another tile give the same permutation of
    the first output, bit for bit: a row is an independent chain of dot products with a fixed k order, its statistics come from its own
    four lanes, so its bits may depend neither on its position nor on its neighbours."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _ln_site_cases as T  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402


def _put(t, storage):
    return P.dev16(t) if storage == "f16" else P.packed(t)


def _where(case, r, ch, plan):
    s = f"row {r} (kind {r % T.KINDS}: {T.KIND_NAMES[r % T.KINDS]}) channel {ch}: 16-token tile {r // 16} (lane {r % 16} of it)"
    if plan is not None:
        _, workgroups, tile = plan
        t = r // tile
        s += f", tile {t} (row {r % tile} of it) = pass {t // workgroups} of workgroup {t % workgroups}"
    return s


def _hold(report, case, kernel, got, ref, plan):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = T.tolerance(case)
    worst = T.worst_by_kind(got.double(), ref)
    for k, (err, r, ch) in enumerate(worst):
        report(f"[ln_sites] {case.id} ({kernel}) kind {k}: worst per-row err {err:.3e} at row {r} channel {ch}, {case.tol} = {tol:g}")
    assert torch.isfinite(got).all(), f"{case.id}: the output is not finite"
    for err, r, ch in worst:
        assert err <= tol, f"{case.id}: per-row err {err:.3e} > {case.tol} = {tol:g} at {_where(case, r, ch, plan)}"


def _run_case(case, report, launch, expect, plan):
    """launch(x, residual or None) -> output; expect(names): asserts on the kernel names of one launch"""
    t0 = time.time()
    o = T.operands(case)
    ref = T.reference(case, o)
    xd = _put(o["x"], case.storage)
    rd = _put(o["res"], case.storage) if case.res else None
    x0, r0 = xd.clone(), None if rd is None else rd.clone()
    got, names = P._launched(lambda: launch(xd, rd))
    if case.storage == "h2":
        P._ops().h2_check(case.id)
    expect(names)
    kernel = case.kernel or "+".join(names) or "several launches"
    _hold(report, case, kernel, P.host(got), ref, plan)
    P._first_diff(got, launch(xd, rd), f"{case.id}: two launches on the same operands")
    P._first_diff(xd, x0, f"{case.id}: x after the launches")
    if rd is not None:
        P._first_diff(rd, r0, f"{case.id}: the residual after the launches")
    p = T.move_rows(case.M, case.tile).cuda()
    moved = launch(xd[p].contiguous(), None if rd is None else rd[p].contiguous())
    P._first_diff(moved, got[p].contiguous(), f"{case.id}: the row-permuted input against the row-permuted output")
    report(f"[ln_sites] {case.id}: test {time.time() - t0:.1f} s")


@pytest.mark.parametrize("case", T.MLP_CASES, ids=lambda c: c.id)
def test_mlp_ln_site(case, report):
    ops = P._ops()
    o = T.operands(case)
    is_packed = case.storage == "h2"
    if is_packed:
        with ops.precision("strict"):
            fc1, fc2 = ops.make_dense_weight(o["w1"], o["b1"]), ops.make_dense_weight(o["w2"], o["b2"])
    else:
        fc1, fc2 = ops.make_dense_weight(o["w1"], o["b1"]), ops.make_dense_weight(o["w2"], o["b2"])
    ln = (P.dev32(o["gamma"]), P.dev32(o["beta"]), case.eps)
    plan = ops.mlp_plan(case.M, case.C, case.N, packed=is_packed)
    fused_names = ("mlp_fused_kernel", "mlp_stream_kernel", "h2:mlp_h2_kernel")
    if case.route == "small":
        assert plan is None, "37 rows must be below what the fused kernels take"
    else:
        assert plan is not None, "the fused kernel does not take this width"
        assert case.M % plan[2] and T.MOVE_TILE % plan[2] == 0, plan

    def launch(x, r):
        if case.route == "unfused":
            with ops.unfused():
                return ops.mlp(x, fc1, fc2, act="gelu", residual=r, ln=ln)
        return ops.mlp(x, fc1, fc2, act="gelu", residual=r, ln=ln)

    def expect(names):
        if case.route == "fused":
            assert names == [case.kernel], names
        else:
            assert not any(n in fused_names for n in names), names

    _run_case(case, report, launch, expect, plan if case.route == "fused" else None)


@pytest.mark.parametrize("case", T.LN_DENSE_CASES, ids=lambda c: c.id)
def test_ln_dense_site(case, report, monkeypatch):
    monkeypatch.setenv("VIP_LN_GEMM_ALL", "1")            # read per call: every shape the kernel can run, whatever the measured policy
    ops = P._ops()
    o = T.operands(case)
    cw = ops.make_dense_weight(o["w1"], o["b1"])
    ln = (P.dev32(o["gamma"]), P.dev32(o["beta"]), case.eps)
    act = "gelu" if case.mode == "gelu" else None

    def launch(x, r):
        assert ops.ln_gemm_fused(x, cw, act, None, r), "ops.ln_dense would fall back to layernorm + dense"
        return ops.ln_dense(x, ln, cw, act=act, residual=r)

    def expect(names):
        assert names == [case.kernel], names

    _run_case(case, report, launch, expect, None)
