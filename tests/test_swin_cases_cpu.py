"""CPU: the case table of tests/_swin_cases.py is sound before a GPU sees it.
  * the folded form (rolled coordinate -> map position, regions, table index by formula: what csrc/swin_attn.hip computes) equals the
    layer as the reference writes it (tests/_swin_v2_ref.py) in float64 on every row;
  * every EXACT row's preconditions hold: operands are fp16 values, every real query's top set is >= 40 nats above the rest;
  * an fp32 emulation of the folded form - plain, and with the fp16 kernel's roundings - passes every row under the row's own rule;
  * each mutant of tests/_swin_cases.MUTANTS moves some row by more than that row accepts - among them three wrong epsilons of the
    normalisation (1e-12, 1e-7, a clamp of the norm instead of the squared norm), which only the beps rows can see;
  * every (heads, ws, shift, H) the two registered members hand the operator has a row."""
import pytest
import torch

from tests import _swin_cases as T

_CACHE = {}


def _row(row):
    if row.id not in _CACHE:
        o = T.operands(row)
        vmax = o[0][..., 2 * row.heads * T.HD:].abs().max().item()
        if o[1] is not None:
            vmax = max(vmax, o[1].abs().max().item())
        _CACHE[row.id] = (o, T.ref64(row, o), vmax)
    return _CACHE[row.id]


def _accepts(row, got, storage):
    """does the row's rule accept `got` (an emulation's output) on `storage`?"""
    o, ref, vmax = _row(row)
    d = (got.double() - ref).abs()
    if row.kind in T.EXACT_KINDS:
        if not bool((d <= T.s3_bound(ref, vmax, row.ws ** 2)).all()):
            return False
        if storage == "s32":
            return True
        p2 = T.pow2_mask(row, o)
        return torch.equal(got.to(torch.float16)[p2], ref.to(torch.float16)[p2])
    return d.max().item() <= T.tolerance(row, storage, ref, vmax)


def test_folded_form_is_the_layer():
    for row in T.ROWS:
        o, ref, _ = _row(row)
        f = T.folded(*o, row.heads, row.ws, row.shift, dtype=T.F64)
        assert (f - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), row.id


def test_exact_rows_preconditions():
    for row in T.EXACT:
        o, _, _ = _row(row)
        assert torch.equal(T.h(o[0]), o[0]), row.id
        gap, cnt = T.top_sets(row, o)
        assert gap.min().item() >= T.GAP, (row.id, gap.min().item())
        if row.kind in ("E1", "E5"):
            assert int(cnt.max()) == 1, row.id
    # E5 is what its name says: sum q^2 below the epsilon, so the normalised query is 1000 q and not a unit vector
    row = next(r for r in T.EXACT if r.kind == "E5")
    q = _row(row)[0][0][..., :row.heads * T.HD].reshape(-1, T.HD)
    assert float((q * q).sum(-1).max()) == 2.0 ** -21 < 1e-6
    # the beps rows are where the clamp's EFFECT is held: every query is an fp16 normal vector below the epsilon
    for row in (r for r in T.BOUNDED if r.kind == "beps"):
        q = _row(row)[0][0][..., :row.heads * T.HD].reshape(-1, T.HD)
        assert float((q * q).sum(-1).max()) < 1e-6 and float(q.abs()[q != 0].min()) >= 2.0 ** -13, row.id


def test_fp32_emulation_passes_every_row():
    for row in T.ROWS:
        o, _, _ = _row(row)
        assert _accepts(row, T.emulate(row, o), "s32"), (row.id, "fp32")
        assert _accepts(row, T.emulate(row, o, round16=True), "f16"), (row.id, "fp16 roundings")


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = []
    for row in T.ROWS:
        if row.H * row.W > 400:                       # the small geometries carry every property
            continue
        o, _, _ = _row(row)
        if not _accepts(row, T.emulate(row, o, mutant=mutant), "s32"):
            caught.append(row.id)
    assert caught, mutant
    print(f"{mutant}: caught by {len(caught)} rows, e.g. {caught[:4]}")


def test_member_shapes_have_rows():
    assert T.member_shapes() == T.MEMBER_SHAPES
    have = {(r.heads, r.ws, r.shift, r.H) for r in T.ROWS if r.H == r.W}
    assert set(T.MEMBER_SHAPES) <= have
