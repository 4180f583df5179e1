"""Records the surface of the reference that generativedensification_amd/finehead.py serves (tests/golden/finehead_surface.json,
read by tests/finehead_ref.py and tests/test_finehead_cpu.py).  Authoring only: it needs the reference tree, which the tests
never read except to compare this record with it where it is present.

    python tests/golden/make_finehead_surface.py REFERENCE_TREE

Parsed with `ast`, nothing of the reference imported or executed; names, counts and literal settings only:
  GaussianModule, GaussianResModule   __init__'s parameter names and defaults (a literal, or the dotted name of a default
                          such as the activation), the layer list of `feat2attr` (per layer the constructor's name and, per
                          argument, the names it mentions and the sum of its integer literals), the `slice_*` attributes in the
                          order they are assigned, and for `forward` the attributes of `self` and of `point` it reads and the
                          objects it updates
  group_cat, Network._union_gaussians   their argument names; the names and sizes of the four-way split
  Network.forward         the five `torch.cat` assignments behind `_union_gaussians`: the name assigned and the names mentioned
"""
import ast
import json
import os
import sys

AUTOENCODER = "lightning/point_decoder/autoencoder.py"
NETWORK = "lightning/network.py"
HERE = os.path.dirname(os.path.abspath(__file__))


def dotted(node):
    """a.b.c of an attribute chain"""
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else None


def mentions(node):
    """the names an expression mentions, attribute chains as dotted names, in source order"""
    seen = []
    for n in ast.walk(node):
        name = dotted(n) if isinstance(n, (ast.Attribute, ast.Name)) else None
        if name and not any(s == name or s.startswith(name + ".") for s in seen):
            seen = [s for s in seen if not name.startswith(s + ".")] + [name]
    return sorted(seen)


def literal_sum(node):
    return sum(n.value for n in ast.walk(node) if isinstance(n, ast.Constant) and isinstance(n.value, int) and not isinstance(n.value, bool))


def module_surface(cls):
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    init, fwd = fns["__init__"], fns["forward"]
    params = [a.arg for a in init.args.args[1:]]
    defaults = {}
    for name, d in zip(params[len(params) - len(init.args.defaults):], init.args.defaults):
        defaults[name] = d.value if isinstance(d, ast.Constant) else dotted(d)
    layers, slices = None, []
    for node in init.body:
        if not isinstance(node, ast.Assign) or not isinstance(node.targets[0], ast.Attribute):
            continue
        attr, value = node.targets[0].attr, node.value
        if attr == "feat2attr":
            layers = {"constructor": dotted(value.func).split(".")[-1],
                      "layers": [{"type": dotted(e.func).split(".")[-1],
                                  "args": [{"names": [m.split(".")[-1] for m in mentions(a)], "plus": literal_sum(a)} for a in e.args]}
                                 for e in value.args]}
        elif attr.startswith("slice_"):
            slices.append(attr)
    chains = {dotted(n) for n in ast.walk(fwd) if isinstance(n, ast.Attribute) and dotted(n) and dotted(n).split(".")[0] in ("self", "point")}
    reads = sorted(c for c in chains if not c.endswith(".update") and not any(o.startswith(c + ".") for o in chains))      # the whole chains
    updates = sorted({dotted(n.func.value) for n in ast.walk(fwd) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "update"})
    keys = sorted({k.value for n in ast.walk(fwd) if isinstance(n, ast.Dict) for k in n.keys if isinstance(k, ast.Constant)})
    return {"init": {"params": params, "defaults": defaults}, "feat2attr": layers, "slices": slices,
            "forward": {"params": [a.arg for a in fwd.args.args], "reads": reads, "updates": updates, "update_keys": keys}}


def record(ref):
    """the surface record of the reference tree at `ref`"""
    auto = ast.parse(open(os.path.join(ref, AUTOENCODER)).read())
    net = ast.parse(open(os.path.join(ref, NETWORK)).read())
    res = {c.name: module_surface(c) for c in auto.body if isinstance(c, ast.ClassDef) and c.name in ("GaussianModule", "GaussianResModule")}
    group_cat = next(n for n in net.body if isinstance(n, ast.FunctionDef) and n.name == "group_cat")
    res["group_cat"] = {"params": [a.arg for a in group_cat.args.args]}
    network = next(n for n in net.body if isinstance(n, ast.ClassDef) and n.name == "Network")
    fns = {n.name: n for n in network.body if isinstance(n, ast.FunctionDef)}
    union = fns["_union_gaussians"]
    split = next(n for n in ast.walk(union) if isinstance(n, ast.Assign) and isinstance(n.value, ast.Call) and dotted(n.value.func) == "torch.split")
    ret = [n for n in ast.walk(union) if isinstance(n, ast.Return)][-1]
    res["_union_gaussians"] = {"params": [a.arg for a in union.args.args], "split": [e.id for e in split.targets[0].elts],
                               "split_sizes": [e.attr for e in split.value.args[1].elts], "returns": [e.id for e in ret.value.elts],
                               "level_reads": sorted({dotted(n) for n in ast.walk(union) if isinstance(n, ast.Attribute) and dotted(n)
                                                      and dotted(n).startswith("point.")})}
    cats = []
    for n in ast.walk(fns["forward"]):
        if (isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and isinstance(n.value, ast.Call) and dotted(n.value.func) == "torch.cat"
                and n.targets[0].id in ("_centers", "_shs", "_opacity", "_scaling", "_rotation") and isinstance(n.value.args[0], ast.List)
                and len(n.value.args[0].elts) == 2):
            first, second = n.value.args[0].elts
            cats.append({"name": n.targets[0].id, "fine": [m for m in mentions(first) if m != "torch"], "survivors": mentions(second)})
    res["concatenations"] = cats
    return res


def main():
    res = record(sys.argv[1])
    with open(os.path.join(HERE, "finehead_surface.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
