"""CPU: nat.CONFIGS, the variable names nat.synth_params writes and the two registry entries against what the reference's nat/nat.py
says, extracted as data by tools/extract_reference_nat.py into tests/golden/ref_nat.json."""
import json
import os

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nat.json")))
KEYS = ("num_blocks", "out_channels", "num_heads", "attn_kernel_size", "mlp_ratio", "layer_scale")


def _tup(v):
    return tuple(_tup(x) for x in v) if isinstance(v, (list, tuple)) else v


def test_configs_agree_with_the_reference():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    base = dict(GOLD["defaults"])
    want = {c["model_name"]: c for c in GOLD["constructors"].values()}
    want[base["model_name"]] = dict(base)                       # the generic constructor under its own defaults
    assert set(nat.CONFIGS) == set(want) and len(want) == 5
    for name, cfg in nat.CONFIGS.items():
        c = want[name]
        assert set(cfg) == set(KEYS) | {"native_hw"}, name
        for k in KEYS:
            assert _tup(cfg[k]) == _tup(c.get(k, base[k])), (name, k)
        assert [cfg["native_hw"]] * 2 + [3] == list(c["input_shape"]), name
        assert all(ch == 32 * h for ch, h in zip(cfg["out_channels"], cfg["num_heads"])), name               # head_dim 32 everywhere
    assert base["stem_width"] == -1                             # the stem is out_channels[0] // 2, then out_channels[0]
    a = GOLD["attention_defaults"]
    assert (a["kernel_size"], a["key_dim"], a["qkv_bias"], a["out_bias"], a["out_weight"]) == (7, 0, True, True, True)
    assert GOLD["layer_variables"]["MultiHeadRelativePositionalKernelBias"] == ["positional_embedding"]


def test_variable_names_agree_with_the_reference():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    n, nv = GOLD["names"], GOLD["name_variables"]
    sfx = lambda fn, callee: [s["suffix"] for s in n[fn] if s["callee"] == callee]       # noqa: E731
    stem1, stem2 = sfx("NAT", "conv2d_no_bias")[:2]
    ln_net = sfx("NAT", "layer_norm")                                                   # stem_, "" (ds_name), pre_output_
    attn = sfx("nat_block", "neighborhood_attention")[0]
    qkv, output = sfx("neighborhood_attention", "Dense")
    pos = sfx("neighborhood_attention", "MultiHeadRelativePositionalKernelBias")[0]
    gammas = sfx("nat_block", "ChannelAffine")
    for key in ("nat_mini", "nat_base"):
        cfg = nat.CONFIGS[key]
        got = set(nat.synth_params(cfg, 3, input_hw=64))
        want = {f"{s}conv/{v}" for s in (stem1, stem2) for v in ("kernel", "bias")}
        want |= {f"{ln_net[0]}ln/{v}" for v in ("gamma", "beta")} | {f"{ln_net[-1]}ln/{v}" for v in ("gamma", "beta")}
        want |= {"predictions/kernel", "predictions/bias"}
        for si, nb in enumerate(cfg["num_blocks"]):
            st = nv["stack_name"].format(si + 1)
            if si > 0:
                ds = st + nv["ds_name"]
                want |= {f"{ds}conv/kernel", f"{ds}ln/gamma", f"{ds}ln/beta"}           # conv2d_no_bias: no bias here
            for bi in range(nb):
                b = st + nv["block_name"].format(bi + 1)
                a = b + attn
                want |= {f"{a}{qkv}/kernel", f"{a}{qkv}/bias", f"{a}{output}/kernel", f"{a}{output}/bias",
                         f"{a}{pos}/{GOLD['layer_variables']['MultiHeadRelativePositionalKernelBias'][0]}"}
                for s in sfx("nat_block", "layer_norm"):
                    want |= {f"{b}{s}ln/gamma", f"{b}{s}ln/beta"}
                m = b + sfx("nat_block", "mlp_block")[0]
                want |= {f"{m}Dense_{i}/{v}" for i in (0, 1) for v in ("kernel", "bias")}
                if cfg["layer_scale"] >= 0:
                    want |= {f"{b}{g}/weight" for g in gammas}
        assert got == want, (key, sorted(got - want)[:6], sorted(want - got)[:6])
    p = nat.synth_params(nat.CONFIGS["nat_base"], 3)
    assert tuple(p["stack2_block1_attn_pos/positional_embedding"].shape) == (8, 169)
    assert tuple(p["stack1_block1_attn_qkv/bias"].shape) == (384,) and tuple(p["stack1_block1_mlp_Dense_0/kernel"].shape) == (128, 256)
    g1 = p["stack1_block1_1_gamma/weight"]
    assert float(g1.min()) >= 0.1 and float(g1.max()) <= 0.4                            # trained layer scales, not the 1e-5 initialiser


def test_registry_entries():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat, zoo
    seeds = [s.seed for s in zoo.MEMBERS.values()]
    assert len(seeds) == len(set(seeds))
    for key, ckpt, hw, seed in (("nat_mini", "NAT_Mini-200x200", 200, 1038), ("nat_base", "NAT_Base-224x224", 224, 1039)):
        spec = zoo.MEMBERS[key]
        assert zoo.by_ckpt_name(ckpt) == key and ckpt.split("-")[0] in GOLD["constructors"]
        assert GOLD["constructors"][ckpt.split("-")[0]]["model_name"] == key
        assert (spec.input_hw, spec.seed, spec.head, spec.family, spec.oracle) == (hw, seed, "predictions", "nat", "")
        assert spec.gmac_per_image == round(nat.gmac_per_image(nat.CONFIGS[key], hw), 3) > 1.0
        assert set(spec.synth(spec.seed)) == set(nat.synth_params(nat.CONFIGS[key], 0))
        # classes and the head activation come from a checkpoint's model_config; the fixed stem has no first_strides to identify
        assert zoo.variant_kwargs(spec, {"stem_strides": 2, "stem_layer": "stem_1_conv", "n_layers": 9, "classes": 2, "head_act": "softmax"}) == {"classes": 2}
        assert zoo.variant_kwargs(spec, {"n_layers": 9, "classes": 1, "head_act": "linear"}) == {"classifier_activation": "linear"}
    assert seeds.count(1038) == 1 and max(seeds) == 1039                              # the next two free seeds
    assert nat.stack_maps(200) == [(50, 50), (25, 25), (13, 13), (7, 7)] and nat.stack_maps(224) == [(56, 56), (28, 28), (14, 14), (7, 7)]
    # hand count of NAT_Mini at 200 pixels: stem 100^2 * 27 * 32 + 50^2 * 9 * 32 * 64; blocks (4 + 6) C^2 + 98 C per token
    mini = 100 * 100 * 27 * 32 + 2500 * 9 * 32 * 64
    for (h, c, nb, cin) in ((50, 64, 3, 0), (25, 128, 4, 64), (13, 256, 6, 128), (7, 512, 5, 256)):
        mini += h * h * 9 * cin * c + nb * h * h * (10 * c * c + 98 * c)
    assert abs(nat.gmac_per_image(nat.CONFIGS["nat_mini"], 200) - (mini + 512) / 1e9) < 1e-12
    for lst in (zoo.ENSEMBLE, zoo.ENSEMBLE8, zoo.ENSEMBLE4):
        assert not [m for m in lst if m.startswith("nat")]
