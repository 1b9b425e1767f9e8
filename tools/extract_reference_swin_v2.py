"""Extracts what the reference says about Swin Transformer V2 as DATA, without importing it: swin_transformer_v2/swin_transformer_v2.py
is parsed with `ast` and only literals are kept - the defaults of the generic `SwinTransformerV2`, per named constructor its assigned
`num_blocks` / `num_heads` / `embed_dim`, the defaults it pops for `window_size` and `pos_scale` (a conditional on `pretrained` is kept
as {"if_pretrained", "then", "else"} next to the constructor's default `pretrained`), its default input shape and `model_name`; the
name suffixes the attention, block, patch-merging and network functions hand their layers; the variable names of the custom layers.

    python tools/extract_reference_swin_v2.py <reference checkout> -> tests/golden/ref_swin_v2.json

tests/test_swin_v2_config_cpu.py compares swin_v2.CONFIGS and the names swin_v2.synth_params writes with this file."""
import ast
import json
import os
import sys

REF = sys.argv[1]
REL = "models/keras_cv_attention_models/swin_transformer_v2/swin_transformer_v2.py"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_swin_v2.json")
tree = ast.parse(open(os.path.join(REF, REL)).read())
funcs = {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def lit(node):
    try:
        return ast.literal_eval(node)
    except ValueError:
        return None


def defaults(fn):
    pos = fn.args.posonlyargs + fn.args.args
    return {a.arg: lit(d) for a, d in zip(pos[len(pos) - len(fn.args.defaults):], fn.args.defaults) if lit(d) is not None or
            (isinstance(d, ast.Constant) and d.value is None)}


def assigns_and_pops(fn):
    """`name = <literal>` and `name = kwargs.pop("name", <default>)` statements of a constructor"""
    out = {}
    for s in fn.body:
        if not (isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Name)):
            continue
        v = s.value
        if isinstance(v, ast.Call) and getattr(v.func, "attr", "") == "pop":
            d = v.args[1]
            if isinstance(d, ast.IfExp):             # [12, 12, 12, 6] if pretrained == "imagenet22k" else -1
                out[s.targets[0].id] = {"if_pretrained": lit(d.test.comparators[0]), "then": lit(d.body), "else": lit(d.orelse)}
            else:
                out[s.targets[0].id] = lit(d)
        elif lit(v) is not None:
            out[s.targets[0].id] = lit(v)
    return out


def name_suffixes(fn):
    """string literals added to `name` in keyword arguments `name=...`, in source order ("" for a bare `name`)"""
    out = []
    for call in sorted((c for c in ast.walk(fn) if isinstance(c, ast.Call)), key=lambda c: (c.lineno, c.col_offset)):
        for kw in call.keywords:
            if kw.arg != "name":
                continue
            lits = [n.value for n in ast.walk(kw.value) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
            callee = call.func.id if isinstance(call.func, ast.Name) else call.func.attr
            out.append({"callee": callee, "suffix": lits[0] if lits else ""})
    return out


ctors = {}
for name, fn in funcs.items():
    if not name.startswith("SwinTransformerV2") or name == "SwinTransformerV2":
        continue
    d = defaults(fn)
    call = next(c for c in ast.walk(fn) if isinstance(c, ast.Call) and getattr(c.func, "id", "") == "SwinTransformerV2")
    ctors[name] = dict(assigns_and_pops(fn), input_shape=d["input_shape"], pretrained=d["pretrained"],
                       model_name=next(lit(kw.value) for kw in call.keywords if kw.arg == "model_name"))
layers = {}
for cd in (n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)):
    layers[cd.name] = [kw.value.value for c in ast.walk(cd) if isinstance(c, ast.Call) and getattr(c.func, "attr", "") == "add_weight"
                       for kw in c.keywords if kw.arg == "name"]
out = {"_source": "awsaf49/vip-cup-2022 (reference checkout), " + REL + " parsed with ast by tools/extract_reference_swin_v2.py",
       "defaults": defaults(funcs["SwinTransformerV2"]), "constructors": ctors,
       "attention_defaults": defaults(funcs["window_mhsa_with_pair_wise_positional_embedding"]),
       "block_defaults": defaults(funcs["swin_transformer_block"]),
       "names": {fn: name_suffixes(funcs[fn]) for fn in ("window_mhsa_with_pair_wise_positional_embedding", "swin_transformer_block",
                                                         "patch_merging", "SwinTransformerV2")},
       "stack_name_format": [n.value for n in ast.walk(funcs["SwinTransformerV2"])
                             if isinstance(n, ast.Constant) and isinstance(n.value, str) and "{}" in n.value],
       "layer_variables": layers}
json.dump(out, open(OUT, "w"), indent=1, sort_keys=True)
print("wrote", OUT, os.path.getsize(OUT), "bytes")
