"""CPU: the case table of tests/_nat_cases.py is sound before a GPU sees it.
  * the folded form (block origin by a clamp, table index by the key-minus-query offset, everything outside the block masked: what
    csrc/nat_attn.hip computes) without a mutant meets every row's acceptance against the layer as the reference writes it
    (tests/_nat_ref.py, float64) - plain fp32, and with the fp16 kernel's roundings; bounded rows at a quarter of their tolerance;
  * every EXACT row's preconditions hold: operands are fp16 values, none of them subnormal, every query's winner set is >= 40 nats
    above the rest;
  * each mutant of tests/_nat_cases.MUTANTS moves some row by more than that row accepts;
  * every (heads, H) the two registered members hand the operator is written out in the table and has a row."""
import pytest
import torch

from tests import _nat_cases as T

_CACHE = {}


def _row(row):
    if row.id not in _CACHE:
        o = T.operands(row)
        _CACHE[row.id] = (o, T.ref64(row, o), T.v_absmax(row, o))
    return _CACHE[row.id]


def _accepts(row, got, storage, share=1.0):
    """does the row's rule accept `got` (an emulation's output) on `storage`?"""
    o, ref, vmax = _row(row)
    d = (got.double() - ref).abs()
    if row.kind in T.EXACT_KINDS:
        if not bool((d <= T.s3_bound(ref, vmax, row.K ** 2)).all()):
            return False
        if storage == "s32":
            return True
        p2 = T.pow2_mask(row, o)
        return torch.equal(got.to(torch.float16)[p2], ref.to(torch.float16)[p2])
    return d.max().item() <= share * T.tolerance(row, storage, ref)


def test_folded_form_is_the_layer():
    for row in T.ROWS:
        o, ref, _ = _row(row)
        f = T.folded(*o, row.heads, row.K, dtype=T.F64)
        assert (f - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), row.id


def test_exact_rows_preconditions():
    for row in T.EXACT:
        o, _, _ = _row(row)
        assert torch.equal(T.h(o[0]), o[0]), row.id
        nz = o[0][o[0] != 0].abs()
        assert float(nz.min()) >= 2.0 ** -14, row.id                       # no fp16 subnormal
        if o[1] is not None:
            assert torch.equal(T.h(o[1]), o[1]) and float(o[1][o[1] != 0].abs().min()) >= 2.0 ** -14, row.id
        gap, cnt = T.top_sets(row, o)
        assert gap.min().item() >= T.GAP, (row.id, gap.min().item())
        if row.kind == "N2" or (row.kind == "N1" and not T.padded(row.H, row.W, row.K)):
            assert int(cnt.max()) == 1, row.id
        if row.kind in ("N4", "N5u", "N5un"):
            assert int(cnt.min()) == int(cnt.max()) == row.K ** 2, row.id
    # N1 reaches every relative position of a block as a target, and N5s some padded slot
    row = next(r for r in T.EXACT if r.kind == "N1" and (r.H, r.W) == (13, 13))
    o = _row(row)[0]
    logits = T.folded(*o, row.heads, row.K, dtype=T.F64, want_logits=True)     # [B, heads, HW, HpWp]
    win = logits.argmax(-1)
    y, x = torch.arange(13)[:, None].expand(13, 13).reshape(-1), torch.arange(13)[None, :].expand(13, 13).reshape(-1)
    rel = {(int(w) // 13 - min(max(int(a) - 3, 0), 6), int(w) % 13 - min(max(int(b) - 3, 0), 6)) for w, a, b in zip(win[0, 0], y, x)}
    assert len(rel) == 49
    row = next(r for r in T.EXACT if r.kind == "N5s" and (r.H, r.W) == (5, 7))
    _, cnt = T.top_sets(row, _row(row)[0])
    assert int(cnt.max()) > 1                                                  # a padded target: every padded slot of the block wins


def test_fp32_emulation_passes_every_row():
    for row in T.ROWS:
        o, _, _ = _row(row)
        assert _accepts(row, T.emulate(row, o), "s32", 0.25), (row.id, "fp32")
        assert _accepts(row, T.emulate(row, o, round16=True), "f16", 0.25), (row.id, "fp16 roundings")


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = []
    for row in T.ROWS:
        if row.H * row.W > 700:                       # the small geometries carry every property
            continue
        o, _, _ = _row(row)
        if not _accepts(row, T.emulate(row, o, mutant=mutant), "s32"):
            caught.append(row.id)
    assert caught, mutant
    print(f"{mutant}: caught by {len(caught)} rows, e.g. {caught[:4]}")


def test_member_shapes_have_rows():
    assert T.member_shapes() == T.MEMBER_SHAPES
    have = {(r.heads, r.H) for r in T.ROWS if r.H == r.W and r.K == 7}
    assert set(T.MEMBER_SHAPES) <= have
