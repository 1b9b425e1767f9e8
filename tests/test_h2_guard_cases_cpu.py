"""tests/_h2_guard_cases.py without a GPU: the table covers exactly the entry points of include/vipcup_hip.h that take the status word,
every (row, kind, position) meets the conditions of its trigger in fp64 (operands in range, nothing in the band where the guard forms
disagree, exactly the named elements out of range), and the dry runs that work without a device send each row to the kernel it names."""
import os
import re

import pytest

import vipcup_amd  # noqa: F401
from vipcup_amd import ops

from tests import _h2_guard_cases as T
from tests.test_h2_dispatch_cpu import SWITCHES

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vipcup_hip.h")


@pytest.fixture(autouse=True)
def default_dispatch(monkeypatch):
    for s in SWITCHES + ("VIP_ATTN_H2_MFMA",):
        monkeypatch.delenv(s, raising=False)


def status_entry_points():
    """names of the prototypes `int vip_...(...)` of the header with an `int* status` parameter"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(vip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return {name for name, args in protos if re.search(r"\bint\s*\*\s*status\b", args)}


def test_table_covers_every_entry_point_with_a_status_word():
    found = status_entry_points()
    assert len(found) == 21, sorted(found)          # today's count: a new packed producer changes it, and needs a row
    assert T.ENTRY_POINTS == found, (sorted(found - T.ENTRY_POINTS), sorted(T.ENTRY_POINTS - found))


def test_table_names_every_kernel_of_the_issue():
    kernels = {r.kernel for r in T.ROWS}
    assert kernels >= {"conv_igemm_kernel", "pw_gemm_kernel", "pwk_direct_kernel", "pwk_gemm_kernel", "pwk_gemm_kernel(im2col)", "gemm8p_kernel",
                       "rows_gemm_kernel", "mlp_h2_kernel", "sdwconv_kernel", "dwconv_tile_h2_kernel", "dwconv_lds_h2_kernel",
                       "dwconv_lds_h2_kernel/pool", "se_gate_kernel", "se_gate_kernel(pooled)", "h2_layernorm_kernel", "slayernorm_kernel",
                       "spool2d_kernel", "sgap_kernel", "sscale_add_act_kernel", "sradix_combine_kernel", "smul_kernel", "svit_tokens_kernel",
                       "pack_h2_kernel", "attn_h2_kernel", "sattn_kernel", "global_local_filter_kernel", "swin_attn_kernel", "nat_attn_kernel"}
    assert len({r.id for r in T.ROWS}) == len(T.ROWS)
    for r in T.ROWS:
        assert "clean" in r.kinds and "nan" in r.kinds, r.id
        if "over+" not in r.kinds:
            assert r.why.startswith(tuple(T.NO_OVER.values())), r.id        # a row without over states why
        elif "over-" not in r.kinds:
            assert "no over-" in r.why, r.id
        assert ("hidden" in r.kinds) == (r.kernel == "mlp_h2_kernel"), r.id
    for entry, n in (("vip_window_attn_fwd_h2", 2), ("vip_mhsa_fwd_h2", 2), ("vip_layernorm_h2", 2), ("vip_mlp_fused_h2", 2),
                     ("vip_dwconv2d_nhwc_h2", 2), ("vip_conv2d_nhwc_h2", 7)):
        assert len({r.kernel for r in T.ROWS if r.entry == entry}) == (n if entry != "vip_mlp_fused_h2" else 1), entry
        assert sum(r.entry == entry for r in T.ROWS) == n, entry


@pytest.mark.parametrize("rid,kind,pos", T.params(), ids=lambda v: str(v))
def test_trigger_conditions(rid, kind, pos):
    ref, skip = T.check(T.BY_ID[rid], kind, pos)
    assert ref.shape == skip.shape and (kind == "clean") == (not skip.any())


def test_rounding_at_the_band():
    """what the module's docstring says of the two guard forms: the converted-half form raises from 65520, the fp32 form above 65504"""
    import torch
    assert torch.tensor(65519.99).half().item() == 65504.0 and torch.isinf(torch.tensor(65520.0).half())
    assert T.BAND[0] < 65504.0 < 65520.0 < T.BAND[1] == 2.0 ** 16


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_row_reaches_its_kernel(row):
    """the dry runs that work without a device (conv / GEMM dispatch as tests/test_h2_dispatch_cpu.py, the depthwise plans, the swin and
    nat plans), the LayerNorm geometry and the MFMA / VALU rule of the window and ViT attention restated from the C sources; rows of
    single-kernel entry points (T.single_kernel) have nothing to choose"""
    assert T.case_of(row).confirm(ops) is None


def test_attention_rows_follow_the_process_switch(monkeypatch):
    """VIP_ATTN_H2_MFMA=0 sends every packed attention call to sattn_kernel: the MFMA rows must then refuse to run as such"""
    mfma = [r for r in T.ROWS if r.kernel == "attn_h2_kernel"]
    valu = [r for r in T.ROWS if r.kernel == "sattn_kernel"]
    assert len(mfma) == 2 and len(valu) == 2
    monkeypatch.setenv("VIP_ATTN_H2_MFMA", "0")
    assert all(T.case_of(r).confirm(ops) is not None for r in mfma) and all(T.case_of(r).confirm(ops) is None for r in valu)
    monkeypatch.setenv("VIP_ATTN_H2_MFMA", "1")
    assert all(T.case_of(r).confirm(ops) is None for r in mfma + valu)
    many = [r for r in T.ROWS if T.case_of(r).confirm is T.single_kernel]
    assert {r.entry for r in many} == {"vip_pool2d_nhwc_h2", "vip_global_avgpool_h2", "vip_scale_add_act_h2", "vip_radix_combine_h2",
                                       "vip_mul_h2", "vip_vit_tokens_h2", "vip_pack_h2"}
