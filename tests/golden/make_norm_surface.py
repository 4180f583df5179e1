"""Records the surface of the reference's AdaLayerNorm and positional_encoding that generativedensification_amd/norm.py
mirrors (tests/golden/norm_surface.json, read by tests/test_norm_cpu.py).  Authoring only: it needs the reference tree, which
the tests never read.

    python tests/golden/make_norm_surface.py REFERENCE_TREE

Parsed with `ast`, nothing imported or executed:
  AdaLayerNorm          bases, the parameter names of __init__ and forward, the default of eps, the child modules __init__
                        assigns (`self.NAME = nn.Something(...)`)
  positional_encoding   (lightning/point_decoder/autoencoder.py, the two-argument one UpscaleModule calls) its parameter names
                        and the functions whose results it concatenates, in order
"""
import ast
import json
import os
import sys

NORMALIZATION = "lightning/point_decoder/layers/normalization.py"
AUTOENCODER = "lightning/point_decoder/autoencoder.py"


def params(fn):
    return [a.arg for a in fn.args.args]


def defaults(fn):
    names = params(fn)[len(fn.args.args) - len(fn.args.defaults):]
    return {n: ast.literal_eval(d) for n, d in zip(names, fn.args.defaults)}


def ada_layer_norm(tree):
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "AdaLayerNorm")
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    children = []
    for node in ast.walk(fns["__init__"]):
        if (isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and isinstance(node.value.func, ast.Attribute)
                and isinstance(node.value.func.value, ast.Name) and node.value.func.value.id == "nn"):
            for t in node.targets:
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self":
                    children.append({"name": t.attr, "module": node.value.func.attr})
    return {"bases": [ast.unparse(b) for b in cls.bases], "init": params(fns["__init__"]), "init_defaults": defaults(fns["__init__"]),
            "forward": params(fns["forward"]), "children": children}


def positional_encoding(tree):
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "positional_encoding"
              and len(n.args.args) == 2 and n.args.args[0].arg == "f")
    ret = next(n for n in ast.walk(fn) if isinstance(n, ast.Return))
    parts = [e.func.attr for e in ret.value.args[0].elts]
    return {"params": params(fn), "concatenates": parts}


def main():
    ref = sys.argv[1]
    res = {"AdaLayerNorm": ada_layer_norm(ast.parse(open(os.path.join(ref, NORMALIZATION)).read())),
           "positional_encoding": positional_encoding(ast.parse(open(os.path.join(ref, AUTOENCODER)).read()))}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "norm_surface.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
