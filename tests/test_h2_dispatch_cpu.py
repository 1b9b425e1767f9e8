"""The shape table of tests/_h2_gemm_cases.py against the C dispatcher's dry run (vip_conv2d_kernel_name_h2 / _variant_h2: the plan of the
launch without the launch, the library loads without a device - tests/test_abi.py): every row selects the kernel and the instantiation
it is in the table for, under default dispatch, and each switch of the packed build (thresholds on 2 K) sits where the table says."""
import pytest
import torch

import vipcup_amd  # noqa: F401
from vipcup_amd import ops

from tests import _h2_gemm_cases as T

# the dispatch switches that are read once per process or per call: the table is for the default of each
SWITCHES = ("VIP_PW", "VIP_PWX", "VIP_PWK_XLK", "VIP_PWK_WN2K", "VIP_PWK_CONV", "VIP_PWK_FILL", "VIP_PW_H2_LDS_KB", "VIP_G8P_MINK")

@pytest.fixture(autouse=True)
def default_dispatch(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def _ldw(kh, kw, cin_g, cout_g, groups):
    """ldw as ops.make_conv_weight derives it under precision("strict") - the constructor itself, on the host"""
    with ops.precision("strict"):
        cw = ops.make_conv_weight(torch.zeros(kh, kw, cin_g, cout_g * groups), None, groups=groups, device="cpu")
    assert cw.kind == "h2"
    return cw.ldw


def dense_desc(M, K, N, epi):
    return T.dense_desc(M, K, N, epi, _ldw(1, 1, K, N, 1))


def conv_desc(case):
    B, H, W, Cin, Cout, k, s, pad, groups, act, use_res = case
    return T.conv_desc(case, _ldw(k, k, Cin // groups, Cout // groups, groups))


@pytest.mark.parametrize("M,K,N,epi,kernel,variant,what", T.DENSE_CASES, ids=T.DENSE_IDS)
def test_dense_row_selects_its_kernel(M, K, N, epi, kernel, variant, what):
    d, res = dense_desc(M, K, N, epi)
    assert d.ldw == 2 * K
    assert ops.conv_kernel_name_h2(d, res) == kernel, what
    assert ops.conv_kernel_variant_h2(d, res) == variant, what


@pytest.mark.parametrize("case,kernel,variant,what", T.CONV_H2_CASES, ids=T.CONV_H2_IDS)
def test_conv_row_selects_its_kernel(case, kernel, variant, what):
    d, res = conv_desc(case)
    assert ops.conv_kernel_name_h2(d, res) == kernel, what
    assert ops.conv_kernel_variant_h2(d, res) == variant, what


@pytest.mark.parametrize("below,above", T.DENSE_BOUNDARIES, ids=lambda p: "x".join(str(v) for v in p[:3]))
def test_dense_boundaries(below, above):
    for M, K, N, kernel in (below, above):
        d, _ = dense_desc(M, K, N, "none")
        assert ops.conv_kernel_name_h2(d, False) == kernel, (M, K, N)
        assert ops.conv_kernel_variant_h2(d, False).startswith(kernel.replace("_kernel", "")), (M, K, N)


def test_conv_im2col_boundary():
    (below, kb, _, _), (above, ka, _, _) = T.CONV_BOUNDARY
    assert below[0] * below[1] * below[2] == 32512 and above[0] * above[1] * above[2] == 33020 and below[3:] == above[3:]
    assert (kb, ka) == ("conv_igemm_kernel", "pwk_gemm_kernel(im2col)")
    for case, kernel in ((below, kb), (above, ka)):
        d, res = conv_desc(case)
        assert ops.conv_kernel_name_h2(d, res) == kernel


def test_table_covers_every_instantiation_it_names():
    """the rows between them reach each tile shape / K-chunk count / slice budget the issue lists, each at least once"""
    seen = {v.split(" ")[0] for *_, v, _ in T.DENSE_CASES} | {v for _, _, v, _ in T.CONV_H2_CASES}
    assert seen >= {"gemm8p<pipe>", "gemm8p<basic>", "pwk_gemm<2,2>", "pwk_gemm<2,1>", "pwk_gemm<1,1>", "pwk_direct<2>", "pwk_direct<1>",
                    "pw_gemm<KS=2>", "pw_gemm<KS=4>", "pw_gemm<KS=6>", "pw_gemm<KS=8>", "im2col<1>", "im2col<2>", "conv_igemm<64,128>",
                    "conv_igemm<128,128>"}
    big = [(M, v) for M, K, N, e, k, v, w in T.DENSE_CASES if M >= 1 << 19]
    assert len(big) == 1 and big[0][1] == "pw_gemm<KS=8> 2 x 192"           # the one large case: the 156 KB slice
    d, _ = dense_desc(big[0][0] - (1 << 19) + 65536, 128, 384, "none")
    assert ops.conv_kernel_variant_h2(d, False) == "pw_gemm<KS=8> 3 x 128"                          # what 72 KB would give
