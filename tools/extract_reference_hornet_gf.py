"""Extracts what the reference says about the HorNet global-filter variants as DATA, without importing it: hornet/hornet.py is parsed
with `ast` and only literals are kept - per GF constructor its `use_global_local_filter` list and `embed_dim` (the HorNet default where the
constructor assigns none), the name suffixes `global_local_filter` hands its layers, the prefix `gnconv` calls it with, and the variable
name of `ComplexDense`.

    python tools/extract_reference_hornet_gf.py <reference checkout> -> tests/golden/ref_hornet_gf.json

tests/test_hornet_gf_config_cpu.py compares hornet.CONFIGS and the names hornet.synth_params writes with this file."""
import ast
import json
import os
import sys

REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_hornet_gf.json")
tree = ast.parse(open(os.path.join(REF, "models/keras_cv_attention_models/hornet/hornet.py")).read())
funcs = {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def defaults(fn):
    pos = fn.args.posonlyargs + fn.args.args
    return {a.arg: ast.literal_eval(d) for a, d in zip(pos[len(pos) - len(fn.args.defaults):], fn.args.defaults)
            if isinstance(d, (ast.Constant, ast.List, ast.Tuple))}


def assigns(fn):
    out = {}
    for s in ast.walk(fn):
        if isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Name):
            try:
                out[s.targets[0].id] = ast.literal_eval(s.value)
            except ValueError:
                pass
    return out


def name_suffixes(fn):
    """string literals added to `name` in keyword arguments `name=name and name + "<suffix>"`, in source order ("" for a bare `name`)"""
    out = []
    for call in sorted((c for c in ast.walk(fn) if isinstance(c, ast.Call)), key=lambda c: (c.lineno, c.col_offset)):
        for kw in call.keywords:
            if kw.arg != "name":
                continue
            lits = [n.value for n in ast.walk(kw.value) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
            callee = call.func.id if isinstance(call.func, ast.Name) else call.func.attr
            out.append({"callee": callee, "suffix": lits[0] if lits else ""})
    return out


base = defaults(funcs["HorNet"])
ctors = {}
for fn in ("HorNetTinyGF", "HorNetSmallGF", "HorNetBaseGF", "HorNetLargeGF"):
    a = assigns(funcs[fn])
    ctors[fn] = {"use_global_local_filter": a["use_global_local_filter"], "embed_dim": a.get("embed_dim", base["embed_dim"])}
cd = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "ComplexDense")
weights = [kw.value.value for c in ast.walk(cd) if isinstance(c, ast.Call) and getattr(c.func, "attr", "") == "add_weight"
           for kw in c.keywords if kw.arg == "name"]
gn = [s for s in name_suffixes(funcs["gnconv"]) if s["callee"] == "global_local_filter"]
out = {"_source": "awsaf49/vip-cup-2022 (reference checkout), models/keras_cv_attention_models/hornet/hornet.py parsed with ast by "
                  "tools/extract_reference_hornet_gf.py",
       "constructors": ctors, "gnconv_prefix": gn[0]["suffix"], "global_local_filter_names": name_suffixes(funcs["global_local_filter"]),
       "complex_dense_variables": weights}
json.dump(out, open(OUT, "w"), indent=1, sort_keys=True)
print("wrote", OUT, os.path.getsize(OUT), "bytes")
