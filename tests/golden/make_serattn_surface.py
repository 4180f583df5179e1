"""Records the surface of the reference's SerializedAttention that generativedensification_amd/serattn.py binds onto
(tests/golden/serattn_surface.json, read by tests/test_serattn_cpu.py).  Authoring only: it needs the reference tree, which
the tests never read.

    python tests/golden/make_serattn_surface.py REFERENCE_TREE

Parsed with `ast`, nothing imported or executed:
  init        the parameter names of __init__
  forward     the parameter names of forward
  assigned    the attributes __init__ assigns (`self.NAME = ...`), in order
  methods     the methods of the class that forward calls on self (the bound forward replaces them with it)
  reads       the attributes of self that forward and those methods read, the methods themselves left out, sorted
  writes      the attributes of self that forward assigns, sorted
  point_reads / point_writes   the attributes of `point` that forward and those methods read / assign, sorted
  point_keys  the string keys under which those methods cache tensors in the point, sorted (an f-string is recorded by its
              constant head)
"""
import ast
import json
import os
import sys

AUTOENCODER = "lightning/point_decoder/autoencoder.py"
CLASS = "SerializedAttention"


def params(fn):
    return [a.arg for a in fn.args.args]


def attrs_of(fns, owner, ctx):
    return sorted({n.attr for fn in fns for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
                   and n.value.id == owner and isinstance(n.ctx, ctx)})


def key_of(value):
    if isinstance(value, ast.Constant) and isinstance(value.value, str):
        return value.value
    if isinstance(value, ast.JoinedStr) and value.values and isinstance(value.values[0], ast.Constant):
        return value.values[0].value
    return None


def surface(tree):
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == CLASS)
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    assigned = []
    for node in ast.walk(fns["__init__"]):
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self" and t.attr not in assigned:
                    assigned.append(t.attr)
    fwd = fns["forward"]
    methods = [m for m in attrs_of([fwd], "self", ast.Load) if m in fns]
    body = [fwd] + [fns[m] for m in methods]
    keys = sorted({k for m in methods for n in ast.walk(fns[m]) if isinstance(n, ast.Assign) and len(n.targets) == 1
                   and isinstance(n.targets[0], ast.Name) and n.targets[0].id.endswith("_key") for k in [key_of(n.value)] if k})
    return {"bases": [ast.unparse(b) for b in cls.bases], "init": params(fns["__init__"]), "forward": params(fwd),
            "assigned": assigned, "methods": methods,
            "reads": [a for a in attrs_of(body, "self", ast.Load) if a not in methods],
            "writes": attrs_of([fwd], "self", ast.Store),
            "point_reads": attrs_of(body, "point", ast.Load), "point_writes": attrs_of(body, "point", ast.Store),
            "point_keys": keys}


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], AUTOENCODER)).read())
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "serattn_surface.json")
    with open(dst, "w") as f:
        json.dump({CLASS: surface(tree)}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
