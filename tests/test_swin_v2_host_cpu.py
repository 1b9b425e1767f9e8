"""CPU: the HOST LOGIC of the Swin V2 graph - the clamped window and shift of every block, query / value bias folded into the qkv Dense,
the bias table and the temperature built in float64, patch merging as a 2x2 convolution with regrouped rows, the post-norm block -
executed through tests/emul_ops.py with ops.swin_window_attention replaced here by the fp32 emulation of the operator's folded form
(tests/_swin_cases.folded), against tests/_swin_v2_ref.py, which writes the layer as the reference does."""
import math

import pytest
import torch

from tests import _swin_cases as T
from tests import _swin_v2_ref as ref
from tests import emul_ops
from tests.test_host_graphs_cpu import _check, _x

CFG = "swin_transformer_v2_tiny_window8"


def _emul_attention(qkv, v_bias, tau, table, heads, ws, shift):
    return T.folded(qkv.float(), v_bias, tau, table, heads, ws, shift)


def _cfg(**kw):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    return dict(swin_v2.CONFIGS[CFG], num_blocks=(1, 1, 2, 1), **kw)


def _run(p, cfg, size, x, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops, swin_v2
    with torch.no_grad(), emul_ops.patched(round_act=False):
        monkeypatch.setattr(ops, "swin_window_attention", _emul_attention)
        model = swin_v2.SwinV2(p, **cfg, input_hw=size, device="cpu")
        return model, model.logits(emul_ops.to_device_nhwc8(x)).float()


@pytest.mark.parametrize("size,maps,plans", [
    (64, (16, 8, 4, 2), [[(8, 0)], [(8, 0)], [(4, 0), (4, 0)], [(2, 0)]]),
    # 100 pixels: 25 -> 13 -> 7 -> 4: odd patch merging twice, padded windows (25 -> 32, 13 -> 16), the clamped windows 7 and 4
    (100, (25, 13, 7, 4), [[(8, 0)], [(8, 0)], [(7, 0), (7, 0)], [(4, 0)]])])
def test_swin_v2_host_graph(size, maps, plans, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    cfg = _cfg()
    assert tuple(m[0] for m in swin_v2.stack_maps(size)) == maps
    p = swin_v2.synth_params(cfg, 21, input_hw=size)
    x = _x(2, size)
    with torch.no_grad():
        z_ref = ref.forward_logits(p, x, cfg)
    model, z = _run(p, cfg, size, x, monkeypatch)
    _check(z, z_ref, f"swin_v2 tiny d1121 @{size}")
    assert [[(b["ws"], b["shift"]) for b in blocks] for _, blocks in model.stages] == plans


def test_shifted_blocks_reach_the_host_graph(monkeypatch):
    """depths (2,2,2,1) at 100 pixels: the odd blocks of stacks 1 and 2 shift by 4 on padded maps; stack 3's window is its whole map"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    cfg = dict(_cfg(), num_blocks=(2, 2, 2, 1))
    p = swin_v2.synth_params(cfg, 22)
    x = _x(1, 100)
    with torch.no_grad():
        z_ref = ref.forward_logits(p, x, cfg)
    model, z = _run(p, cfg, 100, x, monkeypatch)
    _check(z, z_ref, "swin_v2 tiny d2221 @100")
    assert [[(b["ws"], b["shift"]) for b in blocks] for _, blocks in model.stages] == [[(8, 0), (8, 4)], [(8, 0), (8, 4)], [(7, 0), (7, 0)], [(4, 0)]]


def test_bias_table_and_tau_are_the_float64_values():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    g = torch.Generator().manual_seed(5)
    heads = 3
    k1, b1, k2 = torch.randn(2, 512, generator=g), torch.randn(512, generator=g) * 0.1, torch.randn(512, heads, generator=g) * 0.1
    for ws, pos_scale in ((8, -1), (7, -1), (4, 12), (8, 6), (3, -1)):
        got = ops.make_swin_bias_table(k1, b1, k2, ws, pos_scale, device="cpu")
        assert got.dtype == torch.float32 and tuple(got.shape) == ((2 * ws - 1) ** 2, heads)
        want = ref.position_bias(k1.double(), b1.double(), k2.double(), ws, ws, pos_scale)          # [heads, N, N], the layer's gather
        assert torch.allclose(ref.gathered(got.double(), ws, ws), want, rtol=2e-7, atol=0), (ws, pos_scale)
        # hand-written float64: the entry of offset (dr, dc) = (1, -2)
        if ws >= 3:
            ps = ws if pos_scale == -1 else pos_scale
            c = [math.copysign(math.log2(1 + abs(8 * o / (ps - 1))) / 3, o) for o in (1, -2)]
            t = (torch.relu(torch.tensor(c, dtype=torch.float64) @ k1.double() + b1.double()) @ k2.double())
            row = (1 + ws - 1) * (2 * ws - 1) + (-2 + ws - 1)
            assert torch.allclose(got[row].double(), 16 * torch.sigmoid(t), rtol=1e-6, atol=0)
    w = torch.tensor([math.log(10.0), 5.0, math.log(100.0) + 1e-3, -1.0]).reshape(1, 4, 1, 1)       # one above ln 100: clamped to 100
    tau = ops.swin_tau(w, device="cpu")
    assert tau.dtype == torch.float32 and tau.tolist() == [pytest.approx(10.0, rel=1e-6), 100.0, 100.0, pytest.approx(math.exp(-1.0), rel=1e-6)]
    assert torch.allclose(tau.double(), ref.tau_of(w.double()), rtol=2e-7, atol=0)


def test_patch_merging_regroups_rows_by_dx_then_dy():
    """a map with distinct rows and columns: out = sum over the 2x2 patch of x[2i + dy, 2j + dx, c] * dense[(2 dx + dy) C + c]"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    C = 8
    g = torch.Generator().manual_seed(6)
    dense = torch.randn(4 * C, 2 * C, generator=g).double()
    x = (torch.arange(5)[:, None, None] * 100.0 + torch.arange(7)[None, :, None] * 10.0 + torch.arange(C)[None, None, :]).double()[None]
    p = {"d_dense/kernel": dense, "d_ln/gamma": torch.ones(2 * C).double(), "d_ln/beta": torch.zeros(2 * C).double()}
    k = swin_v2.merge_conv_kernel(dense)                                   # [dy, dx, c, out]
    assert tuple(k.shape) == (2, 2, C, 2 * C)
    for dy in range(2):
        for dx in range(2):
            assert torch.equal(k[dy, dx], dense[(2 * dx + dy) * C:(2 * dx + dy + 1) * C])
    xp = torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 1))                    # the odd 5 x 7 map padded at the bottom / right
    conv = torch.einsum("bijyxc,yxco->bijo", xp.reshape(1, 3, 2, 4, 2, C).permute(0, 1, 3, 2, 4, 5), k)
    want = ref.patch_merging(p, "d_", x)                                    # the reference's reshape / transpose / reshape + Dense + LN
    got = torch.nn.functional.layer_norm(conv, (2 * C,), eps=ref.LN_EPS)
    assert torch.allclose(got, want, rtol=1e-10, atol=1e-10)
    wrong = torch.einsum("bijyxc,xyco->bijo", xp.reshape(1, 3, 2, 4, 2, C).permute(0, 1, 3, 2, 4, 5), k)   # dy and dx exchanged
    assert not torch.allclose(torch.nn.functional.layer_norm(wrong, (2 * C,), eps=ref.LN_EPS), want, rtol=1e-3, atol=1e-3)


def test_blocks_are_alive():
    """the synthetic post-norm gammas are non-zero: zeroing one block's attn_ln gamma (and beta) moves the logit"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    cfg = _cfg()
    p = swin_v2.synth_params(cfg, 23)
    x = _x(2, 64)
    with torch.no_grad():
        z = ref.forward_logits(p, x, cfg)
        q = {k: (torch.zeros_like(v) if k.startswith("stack3_block1_attn_ln/") else v) for k, v in p.items()}
        z0 = ref.forward_logits(q, x, cfg)
    assert (z - z0).abs().max().item() > 1e-3 * max(1.0, z.abs().max().item())


def test_large_windows_are_refused():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    cfg = dict(swin_v2.CONFIGS["swin_transformer_v2_tiny_window16"], num_blocks=(1, 1, 1, 1))
    p = swin_v2.synth_params(cfg, 24)
    with pytest.raises(ValueError, match=r"stack1 runs 16 x 16 windows on its 64 x 64 map.*up to 8 x 8"):
        swin_v2.SwinV2(p, **cfg, input_hw=256, device="cpu")
    with pytest.raises(ValueError, match=r"stack1 runs 12 x 12 windows"):   # the window is clamped to the map before it is judged
        swin_v2.SwinV2(p, **cfg, input_hw=48, device="cpu")
