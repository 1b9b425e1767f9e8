"""The global-local filter (ops.global_local_filter, csrc/global_filter.hip) on the three storages, and the HorNet-GF graph on it.
  * EXACT rows of tests/_gf_cases.py under torch.equal against the fp64 reference - the specialised widths (6, 7, 12, 14) and the generic
    form, one / a partly filled / three channel blocks, one and three images, the structured rows (identity, pure wraps, a single live
    pixel, a corner tap of the local filter); a second launch agrees bit for bit;
  * BOUNDED rows: a random complex weight through ops.make_global_filter_weight and randn activations against torch.fft in float64,
    error relative to the output's absmax under the suite's tolerances (TOL_F16 on the fp16 storage, TOL_OP on the packed and fp32 ones);
  * batch independence: image 1 of a three-image launch equals the same image launched alone, bit for bit;
  * member parity: hornet_tiny_gf at depths (1,1,2,1), two images, at 224 and at 200 pixels, against tests/_hornet_gf_ref.py - fast mode
    under the acceptance of tests/test_gpu_kecam.py::test_hornet_reduced_depth, strict and f32 within TOL_NORTH_STAR on the logit; the
    worst errors go to the suite's parity report and, with VIP_GF_PARITY_LOG=<file> set, are appended to that file
    (profiles/hornet_gf_parity.log is one such run).
Measured on an MI355X: see profiles/hornet_gf_parity.log."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _gf_cases as T  # noqa: E402
from tests import _hornet_gf_ref as gf_ref  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402
from tests._parity import TOL_NORTH_STAR  # noqa: E402
from tests.test_gpu_dw import _assert_equal  # noqa: E402
from tests.test_gpu_kecam import _compare  # noqa: E402
from tests.test_gpu_resnet_rs import _images  # noqa: E402

STORAGES = ("f16", "h2", "s32")
TOL = {"f16": P.TOL_F16, "h2": P.TOL_OP, "s32": P.TOL_OP}
_ops = P._ops
_REF = {}


def _ref(row):
    """(x, w3, g, ref64) of an EXACT row on the host, computed once and left unchanged"""
    if row.id not in _REF:
        x, w3, g = T.operands(row)
        _REF[row.id] = (x, w3, g, T.ref64(x, w3, g))
    return _REF[row.id]


def _act(x, storage):
    return {"f16": P.dev16, "h2": P.packed, "s32": P.dev32}[storage](x)


def _host64(t, what):
    if t.dtype == torch.int32:
        t = _ops().unpack_h2(t)
        _ops().h2_check(what)
    return t.cpu().double()


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_gf_exact(row, report):
    ops = _ops()
    x, w3, g, ref = _ref(row)
    blocks, bc, _ = ops.global_filter_plan(row.H, row.W, row.S)
    assert bc == T.block_channels(row.H) and blocks == -(-row.S // bc)
    w3d, gd = P.dev32(w3), P.dev32(g)
    for storage in STORAGES:
        xd = _act(x, storage)
        got = ops.global_local_filter(xd, w3d, gd)
        _assert_equal(f"{row.id} {storage}", _host64(got, row.id), ref)
        P._first_diff(got, ops.global_local_filter(xd, w3d, gd), f"{row.id} {storage}: two launches on the same operands")
    report(f"[gf] {row.id}: {row.B}x{row.H}x{row.W}x{row.S}, {blocks} channel block(s) of {bc}: bit-exact on f16 / h2 / s32")


@pytest.mark.parametrize("row", T.BOUNDED, ids=lambda r: r.id)
def test_gf_bounded(row, report):
    ops = _ops()
    x, w3, cw = T.bounded_operands(row)
    gd = ops.make_global_filter_weight(cw, row.H, row.W)
    w3d = P.dev32(w3)
    for storage in STORAGES:
        xs = P.h(x) if storage == "f16" else x                           # the reference sees what the storage holds
        ref = T.fft64(xs, w3, cw)
        got = ops.global_local_filter(_act(xs, storage), w3d, gd)
        P._check_map(report, f"gf {row.id} {storage}", _host64(got, row.id), ref, TOL[storage])


@pytest.mark.parametrize("hw", [(14, 14), (7, 7), (13, 14)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_gf_batch_independence(hw):
    ops = _ops()
    row = T.Row(f"batch-{hw[0]}x{hw[1]}", 3, hw[0], hw[1], 80, "bounded")
    x, w3, cw = T.bounded_operands(row)
    gd, w3d = ops.make_global_filter_weight(cw, *hw), P.dev32(w3)
    for storage in STORAGES:
        three = ops.global_local_filter(_act(x, storage), w3d, gd)
        alone = ops.global_local_filter(_act(x[1:2], storage), w3d, gd)
        P._first_diff(three[1:2].contiguous(), alone, f"{row.id} {storage}: image 1 of three against the image alone")


def _log(msg):
    path = os.environ.get("VIP_GF_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(msg + "\n")


@pytest.mark.parametrize("size", [224, 200])
@pytest.mark.parametrize("mode", ["fast", "strict", "f32"])
def test_hornet_gf_reduced_depth(mode, size, report):
    """HorNetTinyGF at depths (1,1,2,1): 14 x 14 and 7 x 7 filters at 224 pixels, 12 x 12 and 6 x 6 at 200"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet, ops
    cfg = dict(hornet.CONFIGS["hornet_tiny_gf"], num_blocks=(1, 1, 2, 1))
    p = hornet.synth_params(cfg, 1035, input_hw=size)
    x = _images(2, size).to(torch.float16).to(torch.float32)
    ca, cb = [], []
    with torch.no_grad():
        gf_ref.forward_features(p, x, cfg, collect=ca)
        z_ref = gf_ref.forward_logits(p, x, cfg)
    with ops.precision(mode):
        m = hornet.HorNet(p, **cfg, input_hw=size)
        xd = ops.to_device_nhwc8(x, dtype=ops.act_dtype(mode))
    m.features(xd, collect=cb)
    z = m.logits(xd).float().cpu()
    if mode == "strict":
        ops.h2_check("hornet_tiny_gf strict")
        cb = [ops.unpack_h2(t) for t in cb]
    worst = max(((a - b.float().cpu()) ** 2).mean().sqrt().item() / a.pow(2).mean().sqrt().item() for a, b in zip(ca, cb))
    ze = (z - z_ref).abs().max().item()
    line = (f"[hornet_tiny_gf d1121 @{size} {mode}] worst stage rel_rms_err {worst:.3e} | logit max_abs_err {ze:.3e} "
            f"(logits {[round(v, 3) for v in z_ref.flatten().tolist()]})")
    report(line)
    _log(line)
    if mode == "fast":
        _compare(report, f"HorNetTinyGF d1121 @{size}", ca, cb, z, z_ref)
    else:
        assert ze <= TOL_NORTH_STAR, line
