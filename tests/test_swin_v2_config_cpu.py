"""CPU: swin_v2.CONFIGS, the variable names swin_v2.synth_params writes and the two registry entries against what the reference's
swin_transformer_v2.py says, extracted as data by tools/extract_reference_swin_v2.py into tests/golden/ref_swin_v2.json."""
import json
import os

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_swin_v2.json")))


def _tup(v):
    return tuple(_tup(x) for x in v) if isinstance(v, (list, tuple)) else v


def _effective(ctor, base, key):
    """a constructor's value of `key` under its own default `pretrained`"""
    v = ctor.get(key, base[key])
    if isinstance(v, dict):
        v = v["then"] if ctor["pretrained"] == v["if_pretrained"] else v["else"]
    return v


def test_configs_agree_with_the_reference():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    base = dict(GOLD["defaults"])
    want = {c["model_name"]: c for c in GOLD["constructors"].values()}
    want[base["model_name"]] = dict(base)                       # the generic constructor under its own defaults
    assert set(swin_v2.CONFIGS) == set(want) and len(want) == 12
    for name, cfg in swin_v2.CONFIGS.items():
        c = want[name]
        for k in ("num_blocks", "num_heads", "embed_dim", "window_size", "pos_scale"):
            assert _tup(cfg[k]) == _tup(_effective(c, base, k)), (name, k)
        assert [cfg["native_hw"]] * 2 + [3] == list(c["input_shape"]), name
        assert all(cfg["embed_dim"] * 2 ** i == 32 * h for i, h in enumerate(cfg["num_heads"])), name      # head_dim 32 everywhere
    assert base["stem_patch_size"] == swin_v2.PATCH and base["use_stack_norm"] is False and base["extra_norm_period"] == 0
    assert GOLD["attention_defaults"]["meta_hidden_dim"] == swin_v2.META_HIDDEN and GOLD["attention_defaults"]["qv_bias"] is True
    assert GOLD["block_defaults"]["mlp_ratio"] == swin_v2.MLP_RATIO


def test_variable_names_agree_with_the_reference():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2
    cfg = swin_v2.CONFIGS["swin_transformer_v2_tiny_window8"]
    got = set(swin_v2.synth_params(cfg, 3, input_hw=64))
    n = GOLD["names"]
    sfx = lambda fn, callee: [s["suffix"] for s in n[fn] if s["callee"] == callee]       # noqa: E731
    stack_fmt, block_fmt = GOLD["stack_name_format"]
    attn = sfx("swin_transformer_block", "shifted_window_attention")[0]
    want = set()
    net = n["SwinTransformerV2"]
    want |= {net[0]["suffix"] + "/kernel", net[0]["suffix"] + "/bias"}                   # stem_conv
    want |= {f"{sfx('SwinTransformerV2', 'layer_norm')[0]}ln/{v}" for v in ("gamma", "beta")}
    want |= {f"{sfx('SwinTransformerV2', 'layer_norm')[-1]}ln/{v}" for v in ("gamma", "beta")}
    want |= {"predictions/kernel", "predictions/bias"}
    mh = "window_mhsa_with_pair_wise_positional_embedding"
    for si, nb in enumerate(cfg["num_blocks"]):
        st = stack_fmt.format(si + 1)
        if si > 0:
            down = st + sfx("SwinTransformerV2", "patch_merging")[0]
            want |= {down + sfx("patch_merging", "Dense")[0] + "/kernel"} | {f"{down}ln/{v}" for v in ("gamma", "beta")}
        for bi in range(nb):
            a = st + block_fmt.format(bi + 1) + attn
            dense = sfx(mh, "Dense")                                                    # qkv, meta_dense_1, meta_dense_2, output
            want |= {f"{a}{dense[0]}/kernel", f"{a}{dense[1]}/kernel", f"{a}{dense[1]}/bias", f"{a}{dense[2]}/kernel",
                     f"{a}{dense[3]}/kernel", f"{a}{dense[3]}/bias"}
            want |= {f"{a}{s}/bias" for s in sfx(mh, "BiasLayer")}
            want |= {f"{a}{sfx(mh, 'ExpLogitScale')[0]}/{GOLD['layer_variables']['ExpLogitScale'][0]}"}
            b = st + block_fmt.format(bi + 1)
            for s in sfx("swin_transformer_block", "layer_norm"):
                want |= {f"{b}{s}ln/gamma", f"{b}{s}ln/beta"}
            m = b + sfx("swin_transformer_block", "mlp_block")[0]
            want |= {f"{m}Dense_{i}/{v}" for i in (0, 1) for v in ("kernel", "bias")}
    assert got == want, (sorted(got - want)[:6], sorted(want - got)[:6])
    p = swin_v2.synth_params(cfg, 3)
    assert tuple(p["stack2_block1_attn_scale/weight"].shape) == (1, 6, 1, 1)            # ExpLogitScale(axis=1) on [b, heads, N, N]
    assert float(p["stack1_block1_attn_ln/gamma"].abs().min()) > 0 and float(p["stack1_block1_mlp_ln/gamma"].abs().min()) > 0


def test_registry_entries():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import swin_v2, zoo
    seeds = [s.seed for s in zoo.MEMBERS.values()]
    assert len(seeds) == len(set(seeds))
    for key, ckpt, hw, seed, cfg in (("swin_v2_tiny_window8", "SwinTransformerV2Tiny_window8-200x200", 200, 1036, "swin_transformer_v2_tiny_window8"),
                                     ("swin_v2_base_window8", "SwinTransformerV2Base_window8-224x224", 224, 1037, "swin_transformer_v2_base_window8")):
        spec = zoo.MEMBERS[key]
        assert zoo.by_ckpt_name(ckpt) == key and ckpt.split("-")[0] in GOLD["constructors"]
        assert (spec.input_hw, spec.seed, spec.head, spec.family, spec.oracle) == (hw, seed, "predictions", "swin_v2", "")
        assert spec.gmac_per_image == round(swin_v2.gmac_per_image(swin_v2.CONFIGS[cfg], hw), 3) > 1.0
        assert set(spec.synth(spec.seed)) == set(swin_v2.synth_params(swin_v2.CONFIGS[cfg], 0))
        # classes and the head activation come from a checkpoint's model_config; the patch stem has no first_strides to identify
        assert zoo.variant_kwargs(spec, {"stem_strides": 4, "stem_layer": "stem_conv", "n_layers": 9, "classes": 2, "head_act": "softmax"}) == {"classes": 2}
        assert zoo.variant_kwargs(spec, {"n_layers": 9, "classes": 1, "head_act": "linear"}) == {"classifier_activation": "linear"}
    assert swin_v2.stack_maps(200) == [(50, 50), (25, 25), (13, 13), (7, 7)] and swin_v2.stack_maps(224) == [(56, 56), (28, 28), (14, 14), (7, 7)]
    assert [swin_v2.window_plan(8, m, 1) for m in swin_v2.stack_maps(200)] == [(8, 4), (8, 4), (8, 4), (7, 0)]
    assert swin_v2.window_plan(7, (56, 56), 1) == (7, 3) and swin_v2.window_plan(8, (56, 56), 0) == (8, 0)
    for lst in (zoo.ENSEMBLE, zoo.ENSEMBLE8, zoo.ENSEMBLE4):
        assert not [m for m in lst if m.startswith("swin")]
