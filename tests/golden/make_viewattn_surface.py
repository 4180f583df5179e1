"""Records the surface of the reference's Decoder.forward_fine that generativedensification_amd/viewattn.py serves
(tests/golden/viewattn_surface.json, read by tests/viewattn_ref.py and tests/test_viewattn_cpu.py).  Authoring only: it needs
the reference tree, which the tests never read.

    python tests/golden/make_viewattn_surface.py REFERENCE_TREE

Parsed with `ast`, nothing imported or executed; names and literal settings only:
  Decoder.__init__       the constructor and the keywords of `self.cross_att` (a literal, or the name of the local / parameter
                         that is passed), the literal `cond_dim`, the layer types of `self.mlp_fine` by index
  Decoder.forward_fine   its parameter names and the attributes of `self` it reads
"""
import ast
import json
import os
import sys

NETWORK = "lightning/network.py"


def self_attr(node):
    return isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "self"


def assigned(fn, is_target):
    return next(n.value for n in ast.walk(fn) if isinstance(n, ast.Assign) and any(is_target(t) for t in n.targets))


def setting(node):
    try:
        return ast.literal_eval(node)
    except ValueError:
        return ast.unparse(node)


def layer_types(node):
    """the constructors of a list expression in order: [a(), b()] + [c()] * k is not expected here, only lists and their sums"""
    if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add):
        return layer_types(node.left) + layer_types(node.right)
    assert isinstance(node, ast.List), ast.dump(node)
    return [e.func.attr for e in node.elts]


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], NETWORK)).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Decoder")
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    init, fine = fns["__init__"], fns["forward_fine"]
    att = assigned(init, lambda t: self_attr(t) and t.attr == "cross_att")
    mlp = assigned(init, lambda t: self_attr(t) and t.attr == "mlp_fine")
    assert ast.unparse(mlp.func) == "nn.Sequential" and isinstance(mlp.args[0], ast.Starred)
    layers = assigned(init, lambda t: isinstance(t, ast.Name) and t.id == mlp.args[0].value.id)
    types = layer_types(layers)
    reads = []
    for node in ast.walk(fine):
        if self_attr(node) and node.attr not in reads:
            reads.append(node.attr)
    res = {"cross_att": {"constructor": ast.unparse(att.func), "keywords": {k.arg: setting(k.value) for k in att.keywords}},
           "cond_dim": ast.literal_eval(assigned(init, lambda t: isinstance(t, ast.Name) and t.id == "cond_dim")),
           "forward_fine": {"params": [a.arg for a in fine.args.args], "reads": sorted(reads)},
           "mlp_fine": {"types": types, "indices": {t: [i for i, u in enumerate(types) if u == t] for t in sorted(set(types))}}}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "viewattn_surface.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
