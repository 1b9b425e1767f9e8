"""CPU: the HOST LOGIC of the NAT graph - the two-convolution stem and the downsampling convolutions with their padding, attn_ln folded
into the qkv Dense, kv_pad taken from the qkv bias where a stack's map is below the kernel, the layer scales folded into the output Dense
and the second MLP Dense, the pre-norm block - executed through tests/emul_ops.py with ops.nat_attention replaced here by the fp32
emulation of the operator's formula (tests/_nat_cases.folded), against tests/_nat_ref.py, which writes the layer as the reference does."""
import pytest
import torch

from tests import _nat_cases as T
from tests import _nat_ref as ref
from tests import emul_ops
from tests.test_host_graphs_cpu import _check, _x


def _emul_attention(qkv, kv_pad, table, heads, kernel_size=7):
    return T.folded(qkv.float(), kv_pad, table, heads, kernel_size)


def _cfg(name, depths):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    return dict(nat.CONFIGS[name], num_blocks=depths)


def _run(p, cfg, size, x, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat, ops
    with torch.no_grad(), emul_ops.patched(round_act=False):
        monkeypatch.setattr(ops, "nat_attention", _emul_attention)
        model = nat.NAT(p, **cfg, input_hw=size, device="cpu")
        return model, model.logits(emul_ops.to_device_nhwc8(x)).float()


@pytest.mark.parametrize("name,depths,size,maps,pads", [
    # 64 pixels: 16 / 8 / 4 / 2 - the last two stacks are below the 7 x 7 kernel and pad
    ("nat_mini", (1, 1, 2, 1), 64, (16, 8, 4, 2), (False, False, True, True)),
    # 100 pixels: 25 / 13 / 7 / 4 - odd maps under the stride-2 convolutions, the 7 x 7 map is one block, the last stack pads
    ("nat_mini", (1, 1, 2, 1), 100, (25, 13, 7, 4), (False, False, False, True)),
    # layer scale and mlp_ratio 2
    ("nat_base", (1, 1, 1, 1), 64, (16, 8, 4, 2), (False, False, True, True))])
def test_nat_host_graph(name, depths, size, maps, pads, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    cfg = _cfg(name, depths)
    assert tuple(m[0] for m in nat.stack_maps(size)) == maps
    p = nat.synth_params(cfg, 31, input_hw=size)
    assert ("stack1_block1_1_gamma/weight" in p) == (name == "nat_base")
    x = _x(2, size)
    cfg_ref = {k: v for k, v in cfg.items() if k != "native_hw"}
    with torch.no_grad():
        z_ref = ref.forward_logits(p, x, cfg_ref)
    model, z = _run(p, cfg, size, x, monkeypatch)
    _check(z, z_ref, f"{name} d{''.join(map(str, depths))} @{size}")
    assert tuple(all(b["kv_pad"] is not None for b in blocks) for _, blocks in model.stages) == pads
    assert tuple(any(b["kv_pad"] is not None for b in blocks) for _, blocks in model.stages) == pads


def test_layer_scale_is_folded_not_dropped(monkeypatch):
    """doubling one block's 1_gamma moves the logit of the product and of the restatement alike"""
    cfg = _cfg("nat_base", (1, 1, 1, 1))
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    p = nat.synth_params(cfg, 32)
    q = dict(p)
    q["stack2_block1_1_gamma/weight"] = p["stack2_block1_1_gamma/weight"] * 2.0
    q["stack3_block1_2_gamma/weight"] = p["stack3_block1_2_gamma/weight"] * 2.0
    x = _x(2, 64)
    cfg_ref = {k: v for k, v in cfg.items() if k != "native_hw"}
    with torch.no_grad():
        z0, z1 = ref.forward_logits(p, x, cfg_ref), ref.forward_logits(q, x, cfg_ref)
    assert (z0 - z1).abs().max().item() > 1e-3 * max(1.0, z0.abs().max().item())
    _, z = _run(q, cfg, 64, x, monkeypatch)
    _check(z, z1, "nat_base d1111 @64, two layer scales doubled")


def test_rectangular_input_and_wrong_map(monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    cfg = _cfg("nat_mini", (1, 1, 1, 1))
    assert nat.stack_maps((64, 100)) == [(16, 25), (8, 13), (4, 7), (2, 4)]
    p = nat.synth_params(cfg, 33)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(1, 64, 100, 3, generator=g).to(torch.float16).to(torch.float32)
    cfg_ref = {k: v for k, v in cfg.items() if k != "native_hw"}
    with torch.no_grad(), emul_ops.patched(round_act=False):
        from vipcup_amd import ops
        monkeypatch.setattr(ops, "nat_attention", _emul_attention)
        model = nat.NAT(p, **cfg, input_hw=(64, 100), device="cpu")
        z = model.logits(emul_ops.to_device_nhwc8(x)).float()
        _check(z, ref.forward_logits(p, x, cfg_ref), "nat_mini d1111 @64x100")
        with pytest.raises(ValueError, match=r"built for a 16 x 25 map in this stack, got 16 x 16.*input_hw"):
            model.logits(emul_ops.to_device_nhwc8(_x(1, 64)))


def test_unsupported_configurations_are_refused():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    cfg = _cfg("nat_mini", (1, 1, 1, 1))
    p = nat.synth_params(cfg, 34)
    with pytest.raises(ValueError, match="attn_kernel_size 9"):
        nat.NAT(p, **dict(cfg, attn_kernel_size=9), input_hw=64, device="cpu")
    with pytest.raises(ValueError, match="stack1 has 64 channels on 4 heads.*head_dim 32"):
        nat.NAT(p, **dict(cfg, num_heads=(4, 4, 8, 16)), input_hw=64, device="cpu")
