"""CPU: the HOST LOGIC of the HorNet-GF graph - which stacks take the global-local filter, the complex weight turned into a circular
filter of the stack's map, `dw_list *= scale` folded into post_ln, the channel interleave - executed through tests/emul_ops.py with
ops.global_local_filter replaced here by an fp32 emulation of the operator's spatial sums, against tests/_hornet_gf_ref.py (torch.fft, as
the reference writes the layer).  The two sides share no arithmetic for the filter: one convolves with g, the other multiplies spectra."""
import pytest
import torch

from tests import _gf_cases as T
from tests import _hornet_gf_ref as ref
from tests import emul_ops
from tests.test_host_graphs_cpu import _check, _x


def _emul_global_local_filter(x, w3, g):
    return T.ref64(x.float(), w3.float(), g.float()).float()


def _run(ctor, x, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    with torch.no_grad(), emul_ops.patched(round_act=False):
        monkeypatch.setattr(ops, "global_local_filter", _emul_global_local_filter)
        model = ctor()
        return model, model.logits(emul_ops.to_device_nhwc8(x)).float()


@pytest.mark.parametrize("size,maps", [(112, ((7, 7), (3, 3))), (96, ((6, 6), (3, 3)))])
def test_hornet_gf_host_graph(size, maps, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet
    cfg = dict(hornet.CONFIGS["hornet_tiny_gf"], num_blocks=(1, 1, 2, 1))
    assert tuple(hornet.stack_maps(size)[2:]) == maps
    p = hornet.synth_params(cfg, 11, input_hw=size)
    x = _x(2, size)
    with torch.no_grad():
        z_ref = ref.forward_logits(p, x, cfg)
    model, z = _run(lambda: hornet.HorNet(p, **cfg, input_hw=size, device="cpu"), x, monkeypatch)
    _check(z, z_ref, f"hornet_tiny_gf@{size}")
    gf = [["gf_g" in b for b in blocks] for _, blocks in model.stages]
    assert gf == [[False], [False], [True, True], [True]]
    assert tuple(model.stages[2][1][0]["gf_g"].shape) == (*maps[0], 240) and tuple(model.stages[3][1][0]["gf_g"].shape) == (*maps[1], 496)


def test_gf_block_is_alive(monkeypatch):
    """the synthetic GF weights keep the block alive: zeroing the complex weights of stack 3 moves the logit"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet
    cfg = dict(hornet.CONFIGS["hornet_tiny_gf"], num_blocks=(1, 1, 2, 1))
    p = hornet.synth_params(cfg, 11, input_hw=96)
    x = _x(2, 96)
    with torch.no_grad():
        z = ref.forward_logits(p, x, cfg)
        q = {k: (torch.zeros_like(v) if k.startswith("stack3_") and k.endswith("complex_weight") else v) for k, v in p.items()}
        z0 = ref.forward_logits(q, x, cfg)
    assert (z - z0).abs().max().item() > 1e-2 * max(1.0, z.abs().max().item())


def test_wrong_filter_size_is_refused():
    """a checkpoint whose complex_weight was stored for another resolution: the constructor names the layer and both sizes"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet
    cfg = dict(hornet.CONFIGS["hornet_tiny_gf"], num_blocks=(1, 1, 1, 1))
    p = hornet.synth_params(cfg, 12, input_hw=112)                      # 7 x 7 and 3 x 3 filters
    with pytest.raises(ValueError, match=r"stack3_block1_gnconv_gf_complex_dense/complex_weight.*\(7, 4\).*6 x 6"):
        hornet.HorNet(p, **cfg, input_hw=96, device="cpu")
    m = hornet.HorNet(p, **cfg, input_hw=112, device="cpu")
    with torch.no_grad(), emul_ops.patched(round_act=False), pytest.raises(ValueError, match="7 x 7 map.*6 x 6"):
        m.logits(emul_ops.to_device_nhwc8(_x(1, 96)))


def test_plain_configs_build_the_graph_they_built_before():
    """the four plain entries: same keys and values, same synthetic checkpoint (no GF variable, no extra draw from the generator),
    same blocks; use_global_local_filter=False, as a scalar or per stack, is the plain graph"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet
    from oracle import hornet_ref
    for name in ("hornet_tiny", "hornet_small", "hornet_base", "hornet_large"):
        assert hornet.CONFIGS[name] == hornet_ref.CONFIGS[name]
        assert hornet.CONFIGS[name + "_gf"] == dict(hornet.CONFIGS[name], use_global_local_filter=(False, False, True, True))
    cfg = dict(hornet.CONFIGS["hornet_tiny"], num_blocks=(1, 1, 2, 1))
    p = hornet.synth_params(cfg, 10)
    assert not [k for k in p if "gf_" in k]
    assert torch.equal(p["predictions/kernel"], hornet.synth_params(dict(cfg, use_global_local_filter=False), 10, input_hw=96)["predictions/kernel"])
    x = _x(2, 64)
    with torch.no_grad():
        z_ref = hornet_ref.forward_logits(p, x, cfg)
        assert torch.equal(ref.forward_logits(p, x, cfg), z_ref)
    for flag in (False, (False,) * 4):
        with torch.no_grad(), emul_ops.patched(round_act=False):
            m = hornet.HorNet(p, **cfg, use_global_local_filter=flag, device="cpu")
            z = m.logits(emul_ops.to_device_nhwc8(x)).float()
        _check(z, z_ref, "hornet plain")
        assert all("dw" in b and "gf_g" not in b for _, blocks in m.stages for b in blocks)
