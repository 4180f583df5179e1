"""Records what the reference's point decoder uses from `torch_scatter` and `torch_geometric.utils`, as lists of names
(tests/golden/scatter_surface.json, read by tests/test_scatter_cpu.py).  Authoring only: it needs the reference tree, which
the tests never read.

    python tests/golden/make_scatter_surface.py REFERENCE_TREE

Per caller module, parsed with `ast`, nothing imported or executed:
  imports   {package: [names]}: `import torch_scatter` is recorded as the package itself ("*"), `from torch_geometric.utils
            import softmax as pyg_softmax` as "softmax"
  calls     {qualified function: {"keywords": the union of the keyword names its calls pass, "positional": the most
            positional arguments any call passes}}
"""
import ast
import json
import os
import sys

PACKAGES = ("torch_scatter", "torch_geometric.utils", "torch_geometric")
MODULES = ("lightning/point_decoder/autoencoder.py", "lightning/point_decoder/layers/normalization.py",
           "lightning/point_decoder/__init__.py")


def surface(path):
    tree = ast.parse(open(path).read())
    imports, alias, calls = {}, {}, {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                if a.name in PACKAGES:
                    imports.setdefault(a.name, []).append("*")
                    alias[a.asname or a.name] = a.name
        elif isinstance(node, ast.ImportFrom) and node.module in PACKAGES:
            for a in node.names:
                imports.setdefault(node.module, []).append(a.name)
                alias[a.asname or a.name] = f"{node.module}.{a.name}"
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and alias.get(f.value.id) in PACKAGES:
            name = f"{alias[f.value.id]}.{f.attr}"
        elif isinstance(f, ast.Name) and f.id in alias and alias[f.id] not in PACKAGES:
            name = alias[f.id]
        else:
            continue
        rec = calls.setdefault(name, {"keywords": [], "positional": 0})
        rec["keywords"] = sorted(set(rec["keywords"]) | {k.arg for k in node.keywords if k.arg})
        rec["positional"] = max(rec["positional"], len(node.args))
    return {"imports": {k: sorted(set(v)) for k, v in imports.items()}, "calls": dict(sorted(calls.items()))}


def main():
    ref = sys.argv[1]
    res = {m: surface(os.path.join(ref, m)) for m in MODULES}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scatter_surface.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
