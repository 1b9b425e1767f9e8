"""The fp16 depthwise rows of tests/_pass_cases.py against the launcher's own dry run (vip_dwconv2d_tile_plan: host arithmetic, nothing
is launched, no GPU needed): every row really is in the multi-pass regime it claims, with the launch geometry its description names.  The
rows of the other families need the device's CU count; tests/test_gpu_passes.py asserts their regime before it launches anything."""
import pytest

from tests import _pass_cases as T


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


@pytest.mark.parametrize("row", T.DW_TILE, ids=lambda r: r.id)
def test_dw_tile_rows_are_multi_pass(row):
    ops = _ops()
    plan = ops.dwconv_tile_plan(row.B, row.H, row.W, row.C, row.k, pad=row.pad, pooled=row.pooled)
    assert plan is not None, "the tile kernel does not take this shape"
    groups, workgroups, geom = plan
    assert geom == row.geom, (geom, row.geom)
    assert workgroups == geom["cap"], "the grid must sit at its cap"
    ratio = groups / workgroups
    assert 1.2 < ratio <= 3 and groups % workgroups != 0, (groups, workgroups)
    Ho, Wo = row.H + row.pad[0] + row.pad[1] - row.k + 1, row.W + row.pad[2] + row.pad[3] - row.k + 1
    parts = ops._abi.lib().vip_dwconv2d_pool_parts(row.B, row.H, row.W, row.C, row.k, 1, Ho, Wo)
    if row.pooled:
        assert parts > 0, "ops.dwconv2d_se would fall back to two plain launches"
        assert groups == row.B * parts                       # image-aligned groups: the rows of partial sums the kernel writes
        assert row.C * T.POOL_CR * 2 <= ops.SE_FUSED_MAX_WEIGHTS


def test_plan_rejects_what_the_tile_kernel_does_not_take():
    lib = _ops()._abi.lib()
    assert lib.vip_dwconv2d_tile_plan(2, 14, 15, 64, 3, 2, 7, 8, 0, None, None) == 0          # stride 2
    assert lib.vip_dwconv2d_tile_plan(2, 14, 15, 64, 4, 1, 14, 15, 0, None, None) == 0        # k = 4
    assert lib.vip_dwconv2d_tile_plan(2, 14, 15, 60, 3, 1, 14, 15, 0, None, None) == 0        # C % 8
    assert lib.vip_dwconv2d_tile_plan(5, 7, 7, 144, 3, 1, 7, 7, 1, None, None) == 0           # pooling form declined: 8 tiles in 16 slots
    assert lib.vip_dwconv2d_tile_plan(5, 7, 7, 144, 3, 1, 7, 7, 0, None, None) > 0


@pytest.mark.parametrize("B,H,W,C,k", T.DW_SINGLE_PASS)
def test_existing_dwconv_shapes_are_single_pass(B, H, W, C, k):
    """what tests/test_gpu_ops.py::test_dwconv launches: fewer groups than workgroups could be, so every workgroup runs its loop once -
    the gap tests/test_gpu_passes.py closes"""
    groups, workgroups, geom = _ops().dwconv_tile_plan(B, H, W, C, k)
    assert groups == workgroups < geom["cap"]
