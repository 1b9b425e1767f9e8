"""Extracts what the reference says about NAT as DATA, without importing it: nat/nat.py is parsed with `ast` and only literals are kept -
the defaults of the generic `NAT`, per named constructor its assigned `num_blocks` / `num_heads` / `out_channels`, the defaults it pops
for `mlp_ratio` and `layer_scale`, its default input shape and `model_name`; the defaults of the attention and block functions; the name
suffixes the attention, block and network functions hand their layers, and the strings the network composes its stack, block and
downsampling names from; the variable names of the custom layer.

    python tools/extract_reference_nat.py <reference checkout> -> tests/golden/ref_nat.json

tests/test_nat_config_cpu.py compares nat.CONFIGS and the names nat.synth_params writes with this file."""
import ast
import json
import os
import sys

REF = sys.argv[1]
REL = "models/keras_cv_attention_models/nat/nat.py"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_nat.json")
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
            out[s.targets[0].id] = lit(v.args[1])
        elif lit(v) is not None:
            out[s.targets[0].id] = lit(v)
    return out


def strings(node):
    return [n.value for n in ast.walk(node) if isinstance(n, ast.Constant) and isinstance(n.value, str)]


def name_suffixes(fn):
    """string literals added to `name` in keyword arguments `name=...`, in source order ("" for a bare variable)"""
    out = []
    for call in sorted((c for c in ast.walk(fn) if isinstance(c, ast.Call)), key=lambda c: (c.lineno, c.col_offset)):
        for kw in call.keywords:
            if kw.arg != "name":
                continue
            lits = strings(kw.value)
            callee = call.func.id if isinstance(call.func, ast.Name) else call.func.attr
            var = next((n.id for n in ast.walk(kw.value) if isinstance(n, ast.Name) and n.id != "name"), None)
            out.append({"callee": callee, "suffix": lits[0] if lits else "", "variable": var})
    return out


ctors = {}
for name, fn in funcs.items():
    if not name.startswith("NAT_"):
        continue
    d = defaults(fn)
    call = next(c for c in ast.walk(fn) if isinstance(c, ast.Call) and getattr(c.func, "id", "") == "NAT")
    ctors[name] = dict(assigns_and_pops(fn), input_shape=d["input_shape"], pretrained=d["pretrained"],
                       model_name=next(lit(kw.value) for kw in call.keywords if kw.arg == "model_name"))
layers = {}
for cd in (n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)):
    layers[cd.name] = [kw.value.value for c in ast.walk(cd) if isinstance(c, ast.Call) and getattr(c.func, "attr", "") == "add_weight"
                       for kw in c.keywords if kw.arg == "name"]
# `stack_name = "stack{}_".format(...)`, `ds_name = stack_name + "downsample_"`, `block_name = stack_name + "block{}_".format(...)`
name_vars = {s.targets[0].id: strings(s.value)[0] for s in ast.walk(funcs["NAT"])
             if isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Name) and s.targets[0].id.endswith("_name") and strings(s.value)}
out = {"_source": "awsaf49/vip-cup-2022 (reference checkout), " + REL + " parsed with ast by tools/extract_reference_nat.py",
       "defaults": defaults(funcs["NAT"]), "constructors": ctors,
       "attention_defaults": defaults(funcs["neighborhood_attention"]),
       "block_defaults": defaults(funcs["nat_block"]),
       "names": {fn: name_suffixes(funcs[fn]) for fn in ("neighborhood_attention", "nat_block", "NAT")},
       "name_variables": name_vars,
       "layer_variables": layers}
json.dump(out, open(OUT, "w"), indent=1, sort_keys=True)
print("wrote", OUT, os.path.getsize(OUT), "bytes")
