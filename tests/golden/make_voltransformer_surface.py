"""Records the surface of the reference's VolTransformer tail that generativedensification_amd/deconv3d.py serves
(tests/golden/voltransformer_surface.json, read by tests/deconv3d_ref.py and tests/test_deconv3d_cpu.py).  Authoring only: it
needs the reference tree, which the tests never read.

    python tests/golden/make_voltransformer_surface.py REFERENCE_TREE

Parsed with `ast`, nothing of the reference imported or executed; names and literal settings only:
  VolTransformer.__init__  its parameter names and literal defaults; the constructor calls of `norm` and `deconv` (an argument
                           is a literal, or the name of the parameter that is passed)
  VolTransformer.forward   its parameter names, the attributes of `self` it reads, and its einsum subscripts in source order
                           (the first builds a cond, the last three are the tail's)
"""
import ast
import json
import os
import sys

NETWORK = "lightning/network.py"
HERE = os.path.dirname(os.path.abspath(__file__))


def self_attr(node):
    return isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "self"


def setting(node):
    try:
        return ast.literal_eval(node)
    except ValueError:
        return ast.unparse(node)


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], NETWORK)).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "VolTransformer")
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    init, fwd = fns["__init__"], fns["forward"]
    params = [a.arg for a in init.args.args[1:]]
    defaults = dict(zip(params[len(params) - len(init.args.defaults):], (setting(d) for d in init.args.defaults)))
    modules = {}
    for node in init.body:
        if isinstance(node, ast.Assign) and self_attr(node.targets[0]) and node.targets[0].attr in ("norm", "deconv"):
            call = node.value
            args = [setting(a) for a in call.args]
            assert all(not isinstance(a, str) or a in params for a in args), args       # names of parameters only
            modules[node.targets[0].attr] = {"constructor": ast.unparse(call.func), "args": args,
                                             "keywords": {k.arg: setting(k.value) for k in call.keywords}}
    einsums = sorted((n for n in ast.walk(fwd) if isinstance(n, ast.Call) and ast.unparse(n.func).split(".")[-1] == "einsum"),
                     key=lambda n: (n.lineno, n.col_offset))
    res = {"init": {"params": params, "defaults": defaults}, "modules": modules,
           "forward": {"params": [a.arg for a in fwd.args.args], "reads": sorted({n.attr for n in ast.walk(fwd) if self_attr(n)}),
                       "einsum": [ast.literal_eval(c.args[0]) for c in einsums]}}
    with open(os.path.join(HERE, "voltransformer_surface.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
