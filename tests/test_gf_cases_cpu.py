"""CPU: the case table of the global-local filter (tests/_gf_cases.py) is what it claims to be - the spatial reference IS the FFT
definition, the EXACT rows are exact in every storage, the structured rows do what their names say, every wrong reading of the operator
moves at least one row, and the channel blocks the table assumes are the kernel's.  Nothing runs on a GPU."""
import pytest
import torch

from tests import _gf_cases as T


@pytest.mark.parametrize("hw", T.CHECK_MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_spatial_reference_is_the_fft_definition(hw):
    """irfft2(rfft2(x) * Wc, s) == circular convolution with irfft2(Wc, s), on complex weights that are NOT Hermitian"""
    H, W = hw
    row = T.Row(f"check-{H}x{W}", 2, H, W, 16, "bounded")
    x, w3, cw = T.bounded_operands(row)
    a, b = T.ref64(x, w3, T.filter64(cw, H, W)), T.fft64(x, w3, cw)
    err = (a - b).abs().max().item()
    print(f"{H}x{W}: |spatial - fft| = {err:.2e} at absmax {b.abs().max().item():.2f}")
    assert err <= 1e-12


def test_product_filter_builder_matches_and_refuses_other_sizes():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    for H, W in T.CHECK_MAPS:
        cw = T.bounded_operands(T.Row(f"w-{H}x{W}", 1, H, W, 16, "bounded"))[2]
        g = ops.make_global_filter_weight(cw, H, W, device="cpu")
        assert g.dtype == torch.float32 and tuple(g.shape) == (H, W, 8)
        assert torch.equal(g, T.filter64(cw, H, W).float())
    cw = torch.zeros(2, 7, 4, 8)
    with pytest.raises(ValueError, match=r"stack3_x/complex_weight.*\(7, 4\).*14 x 14"):
        ops.make_global_filter_weight(cw, 14, 14, device="cpu", name="stack3_x/complex_weight")


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_exact_rows_are_exact(row):
    x, w3, g = T.operands(row)
    for t, lim in ((x, 2), (w3, 1), (g, 1)):
        assert t.abs().max() <= lim and torch.equal(t * 4, (t * 4).round())
    ref = T.ref64(x, w3, g)
    assert ref.shape == x.shape
    assert ref.abs().max().item() <= 2 * row.H * row.W and torch.equal(ref * 4, (ref * 4).round())
    assert torch.equal(ref.to(torch.float16).double(), ref)            # the fp16 storage holds it; hi + lo and fp32 then do too
    assert ref.abs().max() > 0
    half = row.S // 2
    glob, loc = ref[..., 1::2], ref[..., 0::2]
    if row.kind == "identity":
        assert torch.equal(glob, x[..., half:].double())
    if row.kind == "wrap-last":
        assert torch.equal(glob, torch.roll(x[..., half:].double(), (-1, -1), (1, 2)))
    if row.kind == "wrap-10":
        assert torch.equal(glob, torch.roll(x[..., half:].double(), (1, 0), (1, 2)))
    if row.kind == "corner-pixel":                                       # the global half IS the filter, shifted to the pixel
        want = torch.roll(g.double(), (0, row.W - 1), (0, 1)) * x[:, 0, row.W - 1, half:].double()[:, None, None, :]
        assert torch.equal(glob, want)
    if row.kind == "w3-corner":                                          # local[h, w] = tap * x[h - 1, w - 1]: row 0 and column 0 are zero
        assert not loc[:, 0].any() and not loc[:, :, 0].any() and loc[:, 1:, 1:].any()


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_every_mutant_moves_a_row(mutant):
    """EXACT rows accept equality alone: a mutant is caught when its output differs anywhere on any row"""
    moved = [r.id for r in T.ROWS if r.S <= 48 and not torch.equal(T.ref64(*T.operands(r), mutant=mutant), T.ref64(*T.operands(r)))]
    assert moved, mutant
    structured = [i for i in moved if i.split("-", 1)[1] in T.STRUCTURED]
    print(f"{mutant}: moves {len(moved)} rows, {len(structured)} of them structured")


def test_mutants_the_structured_rows_are_there_for():
    """a wrapping local half on the w3-corner rows, a zero-padded global half on the pure wraps"""
    by = {r.id: r for r in T.ROWS}
    for hw in ("14x14", "13x14"):
        r = by[f"{hw}-w3-corner"]
        assert not torch.equal(T.ref64(*T.operands(r), mutant="circular-local"), T.ref64(*T.operands(r)))
        for kind in ("wrap-last", "wrap-10"):
            r = by[f"{hw}-{kind}"]
            assert not torch.equal(T.ref64(*T.operands(r), mutant="zero-padded-global"), T.ref64(*T.operands(r)))
            assert not torch.equal(T.ref64(*T.operands(r), mutant="shift-sign"), T.ref64(*T.operands(r)))


def test_bounded_rows_mutants_exceed_the_tolerance():
    """on the BOUNDED rows a mutant must miss by more than the fp16 tolerance (2e-3 of the absmax), or the rows could not tell"""
    for row in T.BOUNDED[:3]:
        x, w3, cw = T.bounded_operands(row)
        ref = T.fft64(x, w3, cw)
        g = T.filter64(cw, row.H, row.W)
        for mutant in T.MUTANTS:
            err = (T.ref64(x, w3, g, mutant=mutant) - ref).abs().max().item()
            assert err > 2e-3 * ref.abs().max().item(), (row.id, mutant)


def test_channel_blocks_are_the_kernels():
    import ctypes as C
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ops
    lib = _abi.lib()
    for H, W in T.MAPS:
        bc, lds = C.c_int(0), C.c_int(0)
        S3 = T.three_blocks(H)
        assert lib.vip_global_local_filter_plan(H, W, S3, C.byref(bc), C.byref(lds)) == 3
        assert bc.value == T.block_channels(H) and 0 < lds.value <= 64 * 1024
        assert lib.vip_global_local_filter_plan(H, W, S3 - 16, None, None) == 2
        assert ops.global_filter_plan(H, W, 16)[0] == 1 and ops.global_filter_plan(H, W, 48)[0] == (1 if bc.value >= 48 else 2)
    assert ops.global_filter_plan(17, 14, 16) is None
