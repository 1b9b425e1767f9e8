"""Every packed-storage producer against its range guard (tests/_h2_guard_cases.py has the table, the operands and the fp64 reference;
tests/test_h2_guard_cases_cpu.py proves the triggers without a GPU).  One case per (row, trigger kind, position):
  * the status word reads 0 before the launch;
  * clean: it stays 0 and the whole output is within the operation's packed tolerance (tests/test_gpu_passes.py::TOL_OP, the tolerance of
    every packed operator test) of the fp64 reference;
  * over+ / over- / hidden / nan: it reads VIP_H2_OVERFLOW after the launch; every output element whose reference is in range and which
    does not depend on the poisoned value is still within that tolerance (one overflow corrupts no neighbour); a following clean launch
    leaves the word raised (it is sticky: no producer writes 0); ops.h2_check raises once and then passes.
The kernel a row names is confirmed before the launch by the project's dry runs, and for the GEMM / convolution / MLP rows also read off
the profiler hook while the launch runs.  Then the main scoring paths: ensemble.score_files and model.predict(dataset) read the word."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _h2_guard_cases as T  # noqa: E402
from tests import _pass_cases  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

import os  # noqa: E402
import re  # noqa: E402

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vipcup_hip.h")
VIP_H2_OVERFLOW = int(re.search(r"#define\s+VIP_H2_OVERFLOW\s+(\d+)", open(_HEADER).read()).group(1))     # the project's own value
_DEV = {}
_SEEN = {}


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def _args(ops, row):
    """the fused-MLP plan's workgroup cap G sizes the persistent row: (2 G + 1) tiles - 37 rows.  The plan of the row's own M is held to
    that: 2 G + 1 tiles of 256 tokens over G workgroups, so tile G + 3 (pass2) is a second pass and the ragged tile 2 G a third."""
    if row.id != "mlp_passes":
        return ()
    _, G, tile = ops.mlp_plan(_pass_cases.BIG_M, T.MLP_C, T.MLP_HID, packed=True)
    assert tile == T.MLP_TILE
    M = T.case_of(row, G).operands["x"].shape[0]
    assert ops.mlp_plan(M, T.MLP_C, T.MLP_HID, packed=True) == (2 * G + 1, G, T.MLP_TILE)
    assert P._assert_regime(2 * G + 1, G, 3) == 3
    return (G,)


def _clean(ops, row, args):
    """the clean operands of a row on the device, uploaded once per module"""
    key = (row.id,) + args
    if key not in _DEV:
        if len(_DEV) >= 2:                                  # rows run in table order: keep the device copies of the current row only
            _DEV.clear()
        case = T.case_of(row, *args)
        _DEV[key] = T.upload(ops, case, case.operands)
    return _DEV[key]


def _word(ops):
    return int(ops.h2_status().item())


def _compare(ops, got, ref, skip):
    """worst error over the compared elements, each relative to the scale of ITS channel (the largest compared |ref| of that index of the
    last axis, + 1e-6): a deliberate +-30000 bias or 8192 gamma entry sets the scale of its own channel only, so a neighbour of magnitude
    100 is held to 2e-3 absolute, not to 0.6.  Never looser than the whole-output scale of tests/test_gpu_strict.py::check."""
    out = ops.unpack_h2(got).double().cpu() if got.dtype == ops.PACKED else got.double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    keep = ~skip
    assert torch.isfinite(out[keep]).all(), "a compared element is not finite"
    C = ref.shape[-1]
    mag = torch.where(keep, ref.abs(), torch.zeros_like(ref)).reshape(-1, C)
    scale = mag.amax(0) + 1e-6                                                   # [C]
    err = torch.where(keep, (out - ref).abs(), torch.zeros_like(ref)).reshape(-1, C)
    return (err / scale).max().item(), int(keep.sum())


@pytest.mark.parametrize("rid,kind,pos", T.params(), ids=lambda v: str(v))
def test_guard(rid, kind, pos, report):
    ops = _ops()
    row = T.BY_ID[rid]
    args = _args(ops, row)
    case = T.case_of(row, *args)
    ref, skip = T.check(row, kind, pos, *args)
    assert case.confirm(ops) is None
    clean = _clean(ops, row, args)
    o, trig = T.triggered(case, kind, pos)
    dev = clean
    if trig is not None:
        only = case._replace(storage={trig.name: case.storage[trig.name]})       # the one operand the trigger touches
        dev = dict(clean, **T.upload(ops, only, o, trig))
    assert _word(ops) == 0, "the status word must read 0 before the launch"
    got, names = P._launched(lambda: case.run(ops, dev))
    word = _word(ops)
    if row.entry in ("vip_conv2d_nhwc_h2", "vip_conv2d_gated_nhwc_h2", "vip_mlp_fused_h2"):
        assert names == ["h2:" + row.kernel], names
    # the label says how the kernel is known: read off the profiler hook, by a dry run / the restated dispatch rule, or the only one there is
    ran = names[0] if names else row.kernel + ("" if case.confirm is T.single_kernel else " (dry run)")
    try:
        rel, n = _compare(ops, got, ref, skip)
        report(f"[h2-guard] {rid:16s} {ran:28s} {kind:6s} {pos:8s} word={word} compared {n} of {ref.numel()} rel={rel:.3e}")
        if kind == "clean":
            assert word == 0, "a clean launch raised the status word"
        else:
            assert word == VIP_H2_OVERFLOW, f"{row.kernel} did not raise the status word ({kind} at {pos})"
        assert rel <= P.TOL_OP, f"{rid}/{kind}/{pos}: rel {rel} > {P.TOL_OP}"
        if kind != "clean":
            case.run(ops, clean)                             # sticky: a clean launch on the same stream does not clear the word
            assert _word(ops) == VIP_H2_OVERFLOW, "a clean launch cleared the status word"
            with pytest.raises(ops._abi.VipError):
                ops.h2_check(f"{rid} {kind}")
            ops.h2_check(f"{rid} {kind}, second read")       # the failed check reset the word
    finally:
        ops.h2_status().zero_()                              # a failing case must not fail the next one
    _SEEN.setdefault(rid, []).append((kind, pos, word))


def test_every_row_ran_every_kind(report):
    """the summary line per row: the kernel and the word after each kind.  Rows of which only some cases were selected (-k, --lf) are
    reported and not judged: that every (row, kind, position) is a case is T.params()'s doing, not this test's."""
    for row in T.ROWS:
        seen = _SEEN.get(row.id, [])
        if not seen:
            continue
        report(f"[h2-guard] {row.id:16s} {row.entry:32s} {row.kernel:28s} " + " ".join(f"{k}@{p}={w}" for k, p, w in seen))
        if len(seen) == len(T.params([row])):
            assert {k for k, _, _ in seen} == set(row.kinds), row.id


# ---- the word is read on the main scoring paths --------------------------------------------------------------------------------------------
class _Stub:
    """a member of one packed global_avgpool and one packed Dense to a single logit (output channel 0 of 8)"""
    precision = "strict"

    def __init__(self, gain):
        ops = _ops()
        g = torch.Generator().manual_seed(7)
        w = torch.zeros(8, 8)
        w[:3, 0] = (torch.randint(1, 9, (3,), generator=g).float() / 4) * gain
        with ops.precision("strict"):
            self.fc = ops.make_dense_weight(w, torch.zeros(8))

    def logits(self, x):
        ops = _ops()
        return ops.unpack_h2(ops.dense(ops.global_avgpool(x), self.fc))[:, :1].contiguous()

    def predict(self, x):
        return torch.sigmoid(self.logits(x))


def _members(gain):
    return [(types.SimpleNamespace(name=f"stub{gain}", input_hw=64), _Stub(gain))]


def test_score_files_reads_the_status_word():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ensemble
    ops = _ops()
    raws = [synth_jpeg(i) for i in range(4)]
    assert _word(ops) == 0
    scores = ensemble.score_files(lambda lo, hi: raws[lo:hi], 4, _members(1.0), batch_size=2)
    assert scores.shape == (1, 4) and np.isfinite(scores).all() and 0.5 < scores.min() and scores.max() < 1.0
    with pytest.raises(_abi.VipError, match="precision f32"):
        ensemble.score_files(lambda lo, hi: raws[lo:hi], 4, _members(2.0 ** 20), batch_size=2)
    assert _word(ops) == 0                                   # the failed check reset the word


def test_predict_dataset_reads_the_status_word():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    ops = _ops()
    x = pipeline.decode_jpegs([synth_jpeg(i) for i in range(4)]).resized(64, 64, dtype=ops.PACKED)
    ops.h2_check("resize")

    @pipeline.keras_predict
    class Model(_Stub):
        pass

    out = Model(1.0).predict([x[:2], x[2:]])
    assert out.shape == (4, 1) and np.isfinite(out).all()
    with pytest.raises(_abi.VipError, match="precision f32"):
        Model(2.0 ** 20).predict([x[:2], x[2:]])
    assert _word(ops) == 0
    # the tensor-in / tensor-out form returns a device tensor and leaves the check to its caller
    y = Model(2.0 ** 20).predict(x)
    assert isinstance(y, torch.Tensor) and _word(ops) == VIP_H2_OVERFLOW
    ops.h2_status().zero_()
