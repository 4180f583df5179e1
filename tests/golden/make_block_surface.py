"""Records the surface of the reference's Block that generativedensification_amd/block.py binds onto, with the constructors of
the MLP it holds and of the DropPath it draws with (tests/golden/block_surface.json, read by tests/test_block_cpu.py).
Authoring only: it needs the reference tree, which the tests never read.

    python tests/golden/make_block_surface.py REFERENCE_TREE

Parsed with `ast`, nothing of the reference imported or executed.  Per class of autoencoder.py:
  init / defaults   the parameter names of __init__ and the source text of their defaults (None where there is none)
  forward           the parameter names of forward
  assigned          the attributes __init__ assigns (`self.NAME = ...`), in order
  reads / writes    the attributes of self that forward reads / assigns, sorted
  point_reads / point_writes   the attributes of `point` that forward reads / assigns, sorted (Block only)
DropPath is not the reference's own: autoencoder.py imports it (`import_from` records the module).  Its constructor
(drop_prob, scale_by_keep) and the attributes its forward reads are timm's public ones; they are taken from the installed timm
when there is one and written out here otherwise.
"""
import ast
import inspect
import json
import os
import sys

AUTOENCODER = "lightning/point_decoder/autoencoder.py"


def params(fn):
    return [a.arg for a in fn.args.args]


def defaults(fn):
    args, given = fn.args.args, fn.args.defaults
    texts = [None] * (len(args) - len(given)) + [ast.unparse(d) for d in given]
    return dict(zip((a.arg for a in args), texts))


def attrs_of(fn, owner, ctx):
    return sorted({n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
                   and n.value.id == owner and isinstance(n.ctx, ctx)})


def surface(tree, name, with_point):
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == name)
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    assigned = []
    for node in ast.walk(fns["__init__"]):
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self" and t.attr not in assigned:
                    assigned.append(t.attr)
    fwd = fns["forward"]
    out = {"bases": [ast.unparse(b) for b in cls.bases], "init": params(fns["__init__"]), "defaults": defaults(fns["__init__"]),
           "forward": params(fwd), "assigned": assigned, "reads": attrs_of(fwd, "self", ast.Load),
           "writes": attrs_of(fwd, "self", ast.Store)}
    if with_point:
        out["point_reads"], out["point_writes"] = attrs_of(fwd, "point", ast.Load), attrs_of(fwd, "point", ast.Store)
    return out


def drop_path(tree):
    origin = next(n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and any(a.name == "DropPath" for a in n.names))
    try:
        from timm.models.layers import DropPath

        sig = inspect.signature(DropPath.__init__)
        init = list(sig.parameters)
        dflt = {k: (None if p.default is inspect.Parameter.empty else repr(p.default)) for k, p in sig.parameters.items()}
    except ImportError:
        init, dflt = ["self", "drop_prob", "scale_by_keep"], {"self": None, "drop_prob": "0.0", "scale_by_keep": "True"}
    return {"import_from": origin, "init": init, "defaults": dflt, "reads": ["drop_prob", "scale_by_keep", "training"]}


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], AUTOENCODER)).read())
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "block_surface.json")
    with open(dst, "w") as f:
        json.dump({"Block": surface(tree, "Block", True), "MLP": surface(tree, "MLP", False), "DropPath": drop_path(tree)}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
