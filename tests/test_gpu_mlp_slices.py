"""The fused fp16 MLP kernels (csrc/mlp_fused.hip: mlp_fused_kernel, LDS-resident weights, C = 64 / 96; mlp_stream_kernel, streamed
weights, C = 192) held BIT FOR BIT to what they computed before their hidden-slice loops were rescheduled (biases staged in LDS, the
next slice's weights prefetched in registers): that change moves loads and waits, never arithmetic, so every output byte must stay.

tests/golden/mlp_slices_parent.json holds sha256 digests of the outputs of ops.mlp on seeded operands, recorded by THIS module in its
record mode on the commit named in the file, on an MI355X:
    VIP_MLP_SLICES_RECORD=<path of the json to write> python -m pytest -m gpu tests/test_gpu_mlp_slices.py
Without that variable the module compares.  Operands come from a CPU generator (the same on every machine): fp16 x and residual
uniform in [-2, 2], weights normal / sqrt(K), fp32 biases, LayerNorm gamma / beta where the row has them.

Rows: per (C, hidden) the token counts 1, one tile - 1, one tile + 1 (below the dispatcher's M >= 8192 threshold ops.mlp answers
them with its two-launch path: held to the same digests, they pin that the threshold did not move), 8192 + 1 (the smallest fused
launch, a one-token last tile) and (2 G + 1) tiles - 37 (G = workgroups of the launch: every workgroup runs a second pass, one a
ragged third, with the bias image and the weight ring carried from tile to tile), crossed with LayerNorm on / off and residual
on / off, plus one row each with fc1's and fc2's bias absent (NULL b1 / b2: zeros).  hidden = 96 at C = 192 is three slices (the ring
parity flips per tile), hidden = 32 one slice (every prefetch wraps onto slice 0 of the next tile).
Every row launches twice and wants equal bits, and x and the residual must come back untouched."""
import hashlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_slices_parent.json")
RECORD = os.environ.get("VIP_MLP_SLICES_RECORD")

# (C, hidden)
CONFIGS = [(192, 768), (192, 96), (192, 32), (128, 512), (96, 384), (64, 256), (64, 32)]


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def _digest(t):
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _record(entries):
    doc = {"recorded_by": "tests/test_gpu_mlp_slices.py in record mode (VIP_MLP_SLICES_RECORD), on one MI355X",
           "commit": os.environ.get("VIP_MLP_SLICES_COMMIT", "unknown"), "digests": {}}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            doc = json.load(f)
    doc["digests"].update(entries)
    os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("C,hidden", CONFIGS, ids=[f"C{c}-h{h}" for c, h in CONFIGS])
def test_mlp_bits_match_parent(C, hidden):
    ops = _ops()
    from vipcup_amd import _abi
    if not _abi.lib().vip_mlp_fused_supported(1 << 20, C, hidden, ops._act("gelu")):
        pytest.skip(f"vip_mlp_fused_supported refuses C = {C} in fast mode (measured slower than two GEMMs): no fused kernel to hold")
    n, G, tile = ops.mlp_plan(1 << 20, C, hidden)
    Ms = [1, tile - 1, tile + 1, 8192 + 1, (2 * G + 1) * tile - 37]
    assert ops.mlp_plan(Ms[-1], C, hidden) == (2 * G + 1, G, tile)         # a ragged third pass
    assert ops.mlp_plan(Ms[-2], C, hidden) is not None                        # fused

    g = torch.Generator().manual_seed(1000 * C + hidden)
    Mx = max(Ms)
    x_all = (torch.rand((Mx, C), generator=g) * 4 - 2).to(torch.float16).cuda()
    r_all = (torch.rand((Mx, C), generator=g) * 4 - 2).to(torch.float16).cuda()
    k1 = torch.randn((C, hidden), generator=g) / math.sqrt(C)
    k2 = torch.randn((hidden, C), generator=g) / math.sqrt(hidden)
    b1 = torch.randn(hidden, generator=g) * 0.5
    b2 = torch.randn(C, generator=g) * 0.5
    ln = ((1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.2 * torch.randn(C, generator=g)).cuda(), 1e-6)
    fc1, fc2 = ops.make_dense_weight(k1, b1), ops.make_dense_weight(k2, b2)
    fc1_nob, fc2_nob = ops.make_dense_weight(k1, None), ops.make_dense_weight(k2, None)
    assert fc1_nob.bias is None and fc2_nob.bias is None

    rows = [(M, use_ln, use_res, fc1, fc2, "") for M in Ms for use_ln in (False, True) for use_res in (False, True)]
    rows += [(Ms[-1], True, True, fc1_nob, fc2, ",b1=NULL"), (Ms[-1], True, True, fc1, fc2_nob, ",b2=NULL"),
             (Ms[-2], False, False, fc1_nob, fc2_nob, ",b1=NULL,b2=NULL")]
    got = {}
    for M, use_ln, use_res, f1, f2, tag in rows:
        x, r = x_all[:M], (r_all[:M] if use_res else None)
        assert x.is_contiguous()
        x0, r0 = x.clone(), (r.clone() if use_res else None)
        y1 = ops.mlp(x, f1, f2, act="gelu", residual=r, ln=ln if use_ln else None)
        y2 = ops.mlp(x, f1, f2, act="gelu", residual=r, ln=ln if use_ln else None)
        torch.cuda.synchronize()
        key = f"C={C},hidden={hidden},M={M},ln={int(use_ln)},res={int(use_res)}{tag}"
        assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), f"{key}: two launches on the same operands differ"
        assert torch.equal(x.view(torch.int16), x0.view(torch.int16)), f"{key}: x was written"
        if use_res:
            assert torch.equal(r.view(torch.int16), r0.view(torch.int16)), f"{key}: the residual was written"
        assert torch.isfinite(y1).all(), key
        got[key] = _digest(y1)
    if RECORD:
        _record(got)
        return
    want = _golden()["digests"]
    missing = [k for k in got if k not in want]
    assert not missing, f"no recorded digest (another workgroup count than the recording device's?): {missing[:3]}"
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(got)} outputs differ from the parent's bits, first: {bad[:4]}"
