"""CPU: the four HorNet-GF entries against the reference's own literals (tests/golden/ref_hornet_gf.json, extracted with `ast` by
tools/extract_reference_hornet_gf.py), the variable names the synthetic checkpoint writes for the GF layers, and the registry."""
import json
import os

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_hornet_gf.json")))
CTORS = {"hornet_tiny_gf": "HorNetTinyGF", "hornet_small_gf": "HorNetSmallGF", "hornet_base_gf": "HorNetBaseGF",
         "hornet_large_gf": "HorNetLargeGF"}


def test_gf_configs_match_the_reference():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet
    assert set(GOLD["constructors"]) == set(CTORS.values())
    for key, fn in CTORS.items():
        cfg, want = hornet.CONFIGS[key], GOLD["constructors"][fn]
        assert list(cfg["use_global_local_filter"]) == want["use_global_local_filter"] == [False, False, True, True]
        assert cfg["embed_dim"] == want["embed_dim"]
        plain = hornet.CONFIGS[key[:-3]]
        assert {k: v for k, v in cfg.items() if k != "use_global_local_filter"} == plain


def test_gf_variable_names_are_the_references():
    """layer_norm(name) -> name + "ln", depthwise_conv2d_no_bias(name) -> name + "dw_conv" (common_layers.py), ComplexDense(name)"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet
    layer = {"layer_norm": ("ln", ("gamma", "beta")), "depthwise_conv2d_no_bias": ("dw_conv", ("depthwise_kernel",)),
             "ComplexDense": ("", tuple(GOLD["complex_dense_variables"]))}
    want = set()
    for ent in GOLD["global_local_filter_names"]:
        tail, variables = layer[ent["callee"]]
        want |= {f"{GOLD['gnconv_prefix']}{ent['suffix']}{tail}/{v}" for v in variables}
    assert len(want) == 6
    cfg = dict(hornet.CONFIGS["hornet_tiny_gf"], num_blocks=(1, 1, 1, 1))
    p = hornet.synth_params(cfg, 5, input_hw=96)
    for stack, on in ((1, False), (2, False), (3, True), (4, True)):
        pre = f"stack{stack}_block1_gnconv_"
        got = {k[len(pre):] for k in p if k.startswith(pre + "gf_")}
        assert got == (want if on else set()), (stack, sorted(got))
        assert (f"{pre}list_dw_conv/depthwise_kernel" in p) == (not on)
    assert f"{pre}gf_dw_conv/bias" not in p                               # use_bias=False
    assert tuple(p["stack3_block1_gnconv_gf_complex_dense/complex_weight"].shape) == (2, 6, 4, 240)
    assert tuple(p["stack4_block1_gnconv_gf_complex_dense/complex_weight"].shape) == (2, 3, 2, 496)
    assert p["stack3_block1_gnconv_gf_complex_dense/complex_weight"].std().item() > 0.3      # not the 0.02 init


def test_gf_members_are_registered():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet, zoo
    assert zoo.by_ckpt_name("HorNetBaseGF-200x200") == "hornet_base_gf"
    assert zoo.by_ckpt_name("HorNetTinyGF-224x224") == "hornet_tiny_gf"
    seeds = [s.seed for s in zoo.MEMBERS.values()]
    assert len(seeds) == len(set(seeds))
    for key, hw, maps in (("hornet_base_gf", 200, ((12, 12), (6, 6))), ("hornet_tiny_gf", 224, ((14, 14), (7, 7)))):
        spec = zoo.MEMBERS[key]
        assert spec.oracle == "hornet_ref" and spec.input_hw == hw and spec.head == "predictions"
        assert tuple(hornet.stack_maps(hw)[2:]) == maps
        assert spec.gmac_per_image > zoo.MEMBERS["hornet_base"].gmac_per_image * (1 if key == "hornet_base_gf" else 0.3)
    # the shipped ensembles and the manifest are what they were
    assert "hornet_base_gf" not in zoo.ENSEMBLE + zoo.ENSEMBLE4 + zoo.ENSEMBLE8
    assert zoo.variant_kwargs(zoo.MEMBERS["hornet_base_gf"], {"stem_strides": 2, "n_layers": 5}) == {"first_strides": 1}
