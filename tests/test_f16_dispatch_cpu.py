"""The shape table of tests/_f16_gemm_cases.py against the C dispatcher's dry run (vip_conv2d_kernel_name / vip_conv2d_kernel_variant:
the plan of the launch without the launch, the library loads without a device - tests/test_abi.py): every row selects the kernel and
the instantiation it is in the table for, under default dispatch, each switch of the fp16 build sits where the table says, the
existing operator cases of tests/test_gpu_ops.py select what they were written for, and every GEMM-like launch of the ensemble step (profiles/r04_fast_shapes_with_floors.log) runs on an instantiation that some
operator test compares with the oracle."""
import os
import re

import pytest
import torch

import vipcup_amd  # noqa: F401
from vipcup_amd import ops

from tests import _f16_gemm_cases as T
from tests import test_gpu_ops as G

# the dispatch switches that are read once per process or per call: the table is for the default of each
SWITCHES = ("VIP_PW", "VIP_PWX", "VIP_PWK_XLK", "VIP_PWK_WN2K", "VIP_PWK_CONV", "VIP_PWK_FILL", "VIP_G8P_MINK")


@pytest.fixture(autouse=True)
def default_dispatch(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def _ldw(kh, kw, cin_g, cout_g, groups):
    """ldw as ops.make_conv_weight derives it in the fast precision - the constructor itself, on the host"""
    with ops.precision("fast"):
        cw = ops.make_conv_weight(torch.zeros(kh, kw, cin_g, cout_g * groups), None, groups=groups, device="cpu")
    assert cw.kind == "f16"
    return cw.ldw


def dense_desc(M, K, N, epi):
    return T.dense_desc(M, K, N, epi, _ldw(1, 1, K, N, 1))


def conv_desc(case):
    B, H, W, Cin, Cout, k, s, pad, groups, act, use_res = case
    return T.conv_desc(case, _ldw(k, k, Cin // groups, Cout // groups, groups))


def dense_variant(M, K, N, epi="none"):
    """the instantiation and tile grid the dispatcher plans for an fp16 Dense [M, K] x [K, N] with that epilogue family"""
    d, res = dense_desc(M, K, N, epi)
    return ops.conv_kernel_variant(d, res)


def conv_variant(case, gated=False):
    """the same for a CONV_CASES tuple"""
    d, res = conv_desc(case)
    return ops.conv_kernel_variant(d, res, has_gate=gated)


def pointwise_epilogue(act, use_res):
    """an epilogue the pointwise kernels carry: an activation or a residual, not both (that one is conv_igemm_kernel's)"""
    return not (act and use_res)


@pytest.mark.parametrize("M,K,N,epi,kernel,variant,what", T.DENSE_CASES, ids=T.DENSE_IDS)
def test_dense_row_selects_its_kernel(M, K, N, epi, kernel, variant, what):
    d, res = dense_desc(M, K, N, epi)
    assert d.ldw == K
    assert ops.conv_kernel_name(d, res) == kernel, what
    assert ops.conv_kernel_variant(d, res) == variant, what
    assert T.same_kernel(ops.conv_kernel_name(d, res), ops.conv_kernel_variant(d, res))


@pytest.mark.parametrize("B,K,N,res,kernel,variant,what", T.GATED_CASES, ids=T.GATED_IDS)
def test_gated_row_selects_its_kernel(B, K, N, res, kernel, variant, what):
    case = T.gated_case(B, K, N, res)
    d, _ = conv_desc(case)
    assert d.Ho * d.Wo == 49 and 256 // 49 >= 5          # a 256-pixel tile spans six images
    assert ops.conv_kernel_name(d, res, has_gate=True) == kernel, what
    assert ops.conv_kernel_variant(d, res, has_gate=True) == variant, what
    assert T.same_kernel(ops.conv_kernel_name(d, res, has_gate=True), ops.conv_kernel_variant(d, res, has_gate=True))
    if K >= 768:                                         # the deep-K loop is the gate's alone: without one the shape leaves this kernel
        assert ops.conv_kernel_name(d, res) != kernel


@pytest.mark.parametrize("case,kernel,variant,what", T.CONV_F16_CASES, ids=T.CONV_F16_IDS)
def test_conv_row_selects_its_kernel(case, kernel, variant, what):
    d, res = conv_desc(case)
    assert ops.conv_kernel_name(d, res) == kernel, what
    assert ops.conv_kernel_variant(d, res) == variant, what
    assert T.same_kernel(ops.conv_kernel_name(d, res), ops.conv_kernel_variant(d, res))


def test_grouped_strided_row_is_selected_by_row_count():
    """the last conv row: grouped, stride 2, asymmetric padding, and im2col by M >= 32 768 alone (cin_g > 16)"""
    case = T.CONV_F16_CASES[-1][0]
    B, H, W, Cin, Cout, k, s, pad, groups, act, use_res = case
    d, _ = conv_desc(case)
    assert groups > 1 and s == 2 and pad[0] != pad[1] and pad[2] != pad[3] and Cin // groups > 16 and B * d.Ho * d.Wo >= 32768
    half = (1,) + case[1:]
    dh, _ = conv_desc(half)
    assert dh.B * dh.Ho * dh.Wo < 32768 and ops.conv_kernel_name(dh, False) == "conv_igemm_kernel"


@pytest.mark.parametrize("below,above", T.DENSE_BOUNDARIES, ids=lambda p: "x".join(str(v) for v in p[:3]))
def test_dense_boundaries(below, above):
    for M, K, N, kernel in (below, above):
        d, _ = dense_desc(M, K, N, "none")
        assert ops.conv_kernel_name(d, False) == kernel, (M, K, N)
        assert T.same_kernel(kernel, ops.conv_kernel_variant(d, False)), (M, K, N)
    assert below[3] != above[3] and sum(a != b for a, b in zip(below[:3], above[:3])) == 1     # one switch, one step


def test_conv_im2col_boundary():
    (below, kb, _, _), (above, ka, _, _) = T.CONV_BOUNDARY
    assert below[0] * below[1] * below[2] == 32512 and above[0] * above[1] * above[2] == 33020 and below[3:] == above[3:]
    assert (kb, ka) == ("conv_igemm_kernel", "pwk_gemm_kernel(im2col)")
    for case, kernel in ((below, kb), (above, ka)):
        d, res = conv_desc(case)
        assert ops.conv_kernel_name(d, res) == kernel


@pytest.mark.parametrize("case,variant,source", T.IGEMM_ROWS, ids=[r[1] for r in T.IGEMM_ROWS])
def test_conv_igemm_tile_shapes_are_reached_by_existing_cases(case, variant, source):
    """the four tile shapes of conv_igemm_kernel, each by a case test_conv2d / test_dense already runs against the oracle"""
    if source == "CONV_CASES":
        assert case in G.CONV_CASES
    else:
        assert (case[0], case[3], case[4]) in G.DENSE_SHAPES and case[9:] == ("gelu", True)      # test_dense's epilogue
    d, res = conv_desc(case)
    assert ops.conv_kernel_name(d, res) == "conv_igemm_kernel"
    assert ops.conv_kernel_variant(d, res) == variant


# ---- the intent of the existing operator cases, pinned here because test_conv2d is re-run under VIP_PWK_CONV=1 ----

def _pw_case(case):
    (B, H, W), Cin, Cout, act, use_res = case
    return (B, H, W, Cin, Cout, 1, 1, (0, 0, 0, 0), 1, act, use_res)


def test_pointwise_stream_cases_select_pw_gemm_and_reach_every_k_step():
    """every PW_CASES shape with an epilogue the pointwise kernels carry streams through pw_gemm_kernel, and between them they reach
    every k-step template.  The two shapes with an activation AND a residual never did: that epilogue is conv_igemm_kernel's (at
    65 792 rows, its largest operator-level launches) - they stay, and each has a residual-only twin that is a pw_gemm launch."""
    seen, other = set(), []
    for case in G.PW_CASES:
        c = _pw_case(case)
        d, res = conv_desc(c)
        if pointwise_epilogue(c[9], c[10]):
            assert ops.conv_kernel_name(d, res) == "pw_gemm_kernel", case
            seen.add((T.instantiation(ops.conv_kernel_variant(d, res)), res))
        else:
            assert ops.conv_kernel_name(d, res) == "conv_igemm_kernel" and ops.conv_kernel_variant(d, res) == "conv_igemm<64,128>", case
            other.append(case)
    assert {v for v, _ in seen} == {f"pw_gemm<KS={ks}>" for ks in (1, 2, 3, 4, 6, 8)}
    assert {v for v, res in seen if res} >= {"pw_gemm<KS=2>", "pw_gemm<KS=4>", "pw_gemm<KS=8>"}       # the residual epilogue, PRE and not
    assert other == [((1, 257, 256), 64, 256, "relu", True), ((1, 256, 257), 256, 768, "gelu", True)]


def test_few_rows_cases_select_rows_gemm():
    for M, K, N in G.FEW_ROWS_SHAPES:
        for act in G.FEW_ROWS_ACTS:
            d = T.dense_desc(M, K, N, "none", _ldw(1, 1, K, N, 1))[0]
            d.act_pre = ops._act(act)
            assert ops.conv_kernel_name(d, False) == "rows_gemm_kernel", (M, K, N, act)
            assert ops.conv_kernel_variant(d, False) == "rows_gemm"


def _gated_existing(c):
    B, H, W, Cin, Cout, use_res = c
    return (B, H, W, Cin, Cout, 1, 1, (0, 0, 0, 0), 1, None, use_res)


def test_gated_cases_select_pwk_direct():
    for c in G.GATED_CASES:
        case = _gated_existing(c)
        d, res = conv_desc(case)
        assert ops.conv_kernel_name(d, res, has_gate=True) == "pwk_direct_kernel", c
        assert ops.conv_kernel_variant(d, res, has_gate=True).endswith("gated> PT=1"), c      # all four: fewer than 256 workgroups


# ---- coverage ----

def covered():
    """the instantiations some operator test compares with the oracle under default dispatch: the rows of the table and the existing case
    lists whose intent the tests above pin"""
    seen = {T.instantiation(v) for *_, v, _ in T.DENSE_CASES} | {v for *_, v, _ in T.GATED_CASES} | {v for _, _, v, _ in T.CONV_F16_CASES}
    seen |= {v for _, v, _ in T.IGEMM_ROWS}
    seen |= {T.instantiation(conv_variant(_pw_case(c))) for c in G.PW_CASES if pointwise_epilogue(c[3], c[4])}
    seen |= {dense_variant(M, K, N) for M, K, N in G.FEW_ROWS_SHAPES}
    seen |= {conv_variant(_gated_existing(c), gated=True) for c in G.GATED_CASES}
    return seen


def test_table_covers_every_instantiation_it_names():
    assert covered() >= T.INSTANTIATIONS
    own = {T.instantiation(v) for *_, v, _ in T.DENSE_CASES} | {v for *_, v, _ in T.GATED_CASES} | {v for _, _, v, _ in T.CONV_F16_CASES}
    # what had no operator-level oracle test before this table
    assert own >= {"pwk_direct<1> PT=4", "pwk_direct<2> PT=4", "pwk_direct<1,gated> PT=4", "pwk_direct<2,gated> PT=4", "pwk_gemm<2,2>",
                   "gemm8p<basic>", "gemm8p<pipe>", "im2col<1>", "im2col<2>", "conv_igemm<128,128>", "conv_igemm<64,128>"}


LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r04_fast_shapes_with_floors.log")
LAUNCH = re.compile(r"\s(rows_gemm_kernel|pw_gemm_kernel|gemm8p_kernel|pwk_direct_kernel|pwk_gemm_kernel(?:\(im2col\))?|conv_igemm_kernel)\s+"
                    r"M=(\d+) N=(\d+) K=(\d+) (dense|k(\d+) s(\d+) g(\d+))( gate)?( res)? act=(\w+)")


def log_launches():
    """(kernel, M, N, K, k, s, g, gated, res, act) of every GEMM-like line of the profile; K is per group (k k cin_g), N the whole Cout"""
    out = []
    with open(LOG) as f:
        for line in f:
            m = LAUNCH.search(line)
            if not m:
                assert not re.search(r"\s(pw|pwk|gemm8p|conv_igemm|rows_gemm)\w*_kernel\S*\s+M=", line), f"unparsed GEMM line: {line}"
                continue
            kernel, M, N, K = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
            k, s, g = (1, 1, 1) if m.group(5) == "dense" else (int(m.group(6)), int(m.group(7)), int(m.group(8)))
            act = None if m.group(11) == "None" else m.group(11)
            # (the gated deep-K launches: only a gate keeps K >= 768 on pwk_direct_kernel, whatever the line says)
            gated = bool(m.group(9)) or (kernel == "pwk_direct_kernel" and K >= 768)
            out.append((kernel, M, N, K, k, s, g, gated, bool(m.group(10)), act))
    return out


def test_every_launch_of_the_ensemble_step_runs_a_tested_instantiation():
    """The profile lists the launches of one ensemble step at batch 256 with their kernel and shape.  Each must map, by the dry run of a
    descriptor built from the line (a k x k line: M images of k x k pixels with one output pixel each, the line's stride and groups), to
    the kernel the profile names and to an instantiation `covered()` holds.  Grid sizes are exempt: the tile counts of the ensemble's maps
    (up to 3 211 264 rows) are not reproduced - the table takes the smallest grid that selects each instantiation and exercises its
    edges (a last tile with one row, ragged channel tiles, a grid that is no multiple of the 8 XCDs) - so variants are compared without
    their `m x n` suffix."""
    launches = log_launches()
    assert len(launches) >= 120 and {l[0] for l in launches} >= {"pw_gemm_kernel", "gemm8p_kernel", "pwk_direct_kernel", "pwk_gemm_kernel",
                                                                 "pwk_gemm_kernel(im2col)", "conv_igemm_kernel"}
    assert sum(1 for l in launches if l[7]) >= 20
    seen, missing = covered(), []
    for kernel, M, N, K, k, s, g, gated, res, act in launches:
        assert K % (k * k) == 0 and N % g == 0
        d, _ = conv_desc((M, k, k, K // (k * k) * g, N, k, s, (0, 0, 0, 0), g, act, res))
        assert d.B * d.Ho * d.Wo == M and d.kh * d.kw * d.Cin // d.groups == K
        v = ops.conv_kernel_variant(d, res, has_gate=gated)
        assert ops.conv_kernel_name(d, res, has_gate=gated) == kernel and T.same_kernel(kernel, v), (kernel, M, N, K, k, s, g, gated, res, act, v)
        if T.instantiation(v) not in seen:
            missing.append((T.instantiation(v), M, N, K, k, s, g))
    assert not missing, missing
