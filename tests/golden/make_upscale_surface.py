"""Records the surface of the reference's UpscaleModule and UpscaleResModule that generativedensification_amd/upscale.py binds
onto (tests/golden/upscale_surface.json, read by tests/test_upscale_cpu.py).  Authoring only: it needs the reference tree,
which the tests never read.

    python tests/golden/make_upscale_surface.py REFERENCE_TREE

Parsed with `ast`, nothing imported or executed.  Per class:
  init        the parameter names of __init__
  forward     the parameter names of forward
  assigned    the attributes __init__ assigns (`self.NAME = ...`) and the buffers it registers, in order
  reads       the attributes of self that forward reads, sorted
  point_reads / point_writes   the attributes of `point` that forward reads / assigns, sorted
"""
import ast
import json
import os
import sys

AUTOENCODER = "lightning/point_decoder/autoencoder.py"
CLASSES = ("UpscaleModule", "UpscaleResModule")


def params(fn):
    return [a.arg for a in fn.args.args]


def attrs_of(fn, owner, ctx):
    return sorted({n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
                   and n.value.id == owner and isinstance(n.ctx, ctx)})


def surface(tree, name):
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == name)
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    assigned = []
    for node in ast.walk(fns["__init__"]):
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self" and t.attr not in assigned:
                    assigned.append(t.attr)
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "register_buffer"
                and isinstance(node.args[0], ast.Constant)):
            assigned.append(node.args[0].value)
    fwd = fns["forward"]
    return {"bases": [ast.unparse(b) for b in cls.bases], "init": params(fns["__init__"]), "forward": params(fwd),
            "assigned": assigned, "reads": attrs_of(fwd, "self", ast.Load), "point_reads": attrs_of(fwd, "point", ast.Load),
            "point_writes": attrs_of(fwd, "point", ast.Store)}


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], AUTOENCODER)).read())
    res = {name: surface(tree, name) for name in CLASSES}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "upscale_surface.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
