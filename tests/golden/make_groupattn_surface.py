"""Records the surface of the reference's GroupAttBlock that generativedensification_amd/groupattn.py serves
(tests/golden/groupattn_surface.json, read by tests/groupattn_ref.py and tests/test_groupattn_cpu.py).  Authoring only: it
needs the reference tree, which the tests never read.

    python tests/golden/make_groupattn_surface.py REFERENCE_TREE

Parsed with `ast`, nothing of the reference imported or executed; names and literal settings only:
  GroupAttBlock.__init__   its parameter names and literal defaults; for every `self.X = ctor(...)` the constructor and its
                           arguments (a literal, or the name of the parameter that is passed); of the MLP the layer types
  GroupAttBlock.forward    its parameter names, the attributes of `self` it reads, the axes it unfolds and its einsum subscripts
  VolTransformer.forward   the axes unfolded and the einsum subscripts on the way to `volume_feats` (the cond of a block)
  parameters               the parameter names of a module built from that record (tests/groupattn_ref.py build_modules)
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


def calls(fn, name):
    return [n for n in ast.walk(fn) if isinstance(n, ast.Call) and ast.unparse(n.func).split(".")[-1] == name]


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], NETWORK)).read())
    classes = {n.name: n for n in tree.body if isinstance(n, ast.ClassDef)}
    fns = {n.name: n for n in classes["GroupAttBlock"].body if isinstance(n, ast.FunctionDef)}
    init, fwd = fns["__init__"], fns["forward"]
    params = [a.arg for a in init.args.args[1:]]
    defaults = dict(zip(params[len(params) - len(init.args.defaults):], (setting(d) for d in init.args.defaults)))
    modules = {}
    for node in init.body:
        if isinstance(node, ast.Assign) and self_attr(node.targets[0]):
            call = node.value
            if ast.unparse(call.func) == "nn.Sequential":
                modules[node.targets[0].attr] = {"constructor": "nn.Sequential", "types": [e.func.attr for e in call.args]}
            else:
                args = [setting(a) for a in call.args]
                assert all(not isinstance(a, str) or a in params for a in args), args       # names of parameters only
                modules[node.targets[0].attr] = {"constructor": ast.unparse(call.func), "args": args,
                                                 "keywords": {k.arg: setting(k.value) for k in call.keywords}}
    reads = sorted({n.attr for n in ast.walk(fwd) if self_attr(n)})
    vol_fwd = next(n for n in classes["VolTransformer"].body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    loop = next(n for n in vol_fwd.body if isinstance(n, ast.For) and any(calls(n, "unfold")))
    res = {"init": {"params": params, "defaults": defaults}, "modules": modules,
           "forward": {"params": [a.arg for a in fwd.args.args], "reads": reads,
                       "unfold_axes": sorted(ast.literal_eval(c.args[0]) for c in calls(fwd, "unfold")),
                       "einsum": [ast.literal_eval(c.args[0]) for c in calls(fwd, "einsum")]},
           "cond": {"unfold_axes": sorted(ast.literal_eval(c.args[0]) for c in calls(loop, "unfold")),
                    "einsum": ast.literal_eval(calls(loop, "einsum")[0].args[0])}}
    sys.path.insert(0, os.path.dirname(HERE))
    from groupattn_ref import build_modules
    from torch import nn

    stand = nn.ModuleDict(build_modules(res, 32, 24, 4))
    res["parameters"] = sorted(n for n, _ in stand.named_parameters())
    with open(os.path.join(HERE, "groupattn_surface.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
