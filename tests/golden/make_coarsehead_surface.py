"""Records the surface of the reference's Decoder that generativedensification_amd/coarsehead.py serves
(tests/golden/coarsehead_surface.json, read by tests/coarsehead_ref.py, tests/test_coarsehead_cpu.py and
tests/test_gpu_coarsehead.py).  Authoring only: it needs the reference tree, which the tests never read.

    python tests/golden/make_coarsehead_surface.py REFERENCE_TREE

Parsed with `ast`, nothing of the reference imported or executed; names, counts and literal settings only:
  Decoder.__init__        its parameter names and literal defaults, the attributes of `self` it assigns from a parameter, and
                          the layer list of `mlp_coarse`: per layer the constructor's name and, per argument, the names it
                          mentions (list arithmetic with literal counts is carried out here)
  Decoder.forward_coarse  its parameter names, the attributes of `self` it reads, the names the five-way split assigns with the
                          literal or attribute name of each size, and the names it returns, in order
"""
import ast
import json
import os
import sys

NETWORK = "lightning/network.py"
HERE = os.path.dirname(os.path.abspath(__file__))


def self_attr(node):
    return isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "self"


def names_of(node):
    """the parameter / attribute names an argument mentions"""
    return sorted({n.attr if self_attr(n) else n.id for n in ast.walk(node)
                   if self_attr(n) or (isinstance(n, ast.Name) and n.id != "self")})


def layers_of(node, consts):
    """the layer list an expression of list literals, + and * builds; an int where it is a count"""
    if isinstance(node, ast.List):
        return [{"type": ast.unparse(e.func).split(".")[-1], "args": [names_of(a) for a in e.args]} for e in node.elts]
    if isinstance(node, ast.Constant) and isinstance(node.value, int):
        return node.value
    if isinstance(node, ast.Name):
        return consts[node.id]
    if isinstance(node, ast.BinOp):
        a, b = layers_of(node.left, consts), layers_of(node.right, consts)
        if isinstance(node.op, ast.Add):
            return a + b
        if isinstance(node.op, ast.Sub):
            return a - b
        if isinstance(node.op, ast.Mult):
            return a * b
    raise ValueError(ast.dump(node))


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], NETWORK)).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Decoder")
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    init, fwd = fns["__init__"], fns["forward_coarse"]
    params = [a.arg for a in init.args.args[1:]]
    defaults = dict(zip(params[len(params) - len(init.args.defaults):], (ast.literal_eval(d) for d in init.args.defaults)))
    consts, attributes, layer_lists, mlp = {}, {}, {}, None
    for node in init.body:
        if not isinstance(node, ast.Assign):
            continue
        target, value = node.targets[0], node.value
        if isinstance(target, ast.Name) and isinstance(value, ast.Constant) and isinstance(value.value, int):
            consts[target.id] = value.value
        elif self_attr(target) and isinstance(value, ast.Name) and value.id in params:
            attributes[target.attr] = value.id
        elif isinstance(target, ast.Name) and target.id == "layers_coarse":
            layer_lists[target.id] = layers_of(value, consts)
        elif self_attr(target) and target.attr == "mlp_coarse":
            mlp = {"constructor": ast.unparse(value.func).split(".")[-1], "layers": layer_lists[value.args[0].value.id]}
    split = next(n for n in ast.walk(fwd) if isinstance(n, ast.Assign) and isinstance(n.value, ast.Call)
                 and ast.unparse(n.value.func).split(".")[-1] == "split")
    sizes = [e.value if isinstance(e, ast.Constant) else e.attr for e in split.value.args[1].elts]
    ret = next(n for n in fwd.body if isinstance(n, ast.Return))
    res = {"init": {"params": params, "defaults": defaults, "attributes": attributes}, "mlp_coarse": mlp,
           "forward_coarse": {"params": [a.arg for a in fwd.args.args], "reads": sorted({n.attr for n in ast.walk(fwd) if self_attr(n)}),
                              "split": [e.id for e in split.targets[0].elts], "split_sizes": sizes,
                              "returns": [e.id for e in ret.value.elts]}}
    with open(os.path.join(HERE, "coarsehead_surface.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
