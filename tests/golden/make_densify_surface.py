"""Records the surface of the reference's top_k / top_p and MaskModule / MaskResModule that
generativedensification_amd/densify.py mirrors (tests/golden/densify_surface.json, read by tests/test_densify_cpu.py).  Authoring
only: it needs the reference tree, which the tests never read.

    python tests/golden/make_densify_surface.py REFERENCE_TREE

Parsed with `ast`, nothing imported or executed:
  top_k, top_p                  their parameter names
  MaskModule, MaskResModule     bases, the parameter names of __init__ and forward, the attributes __init__ assigns, the values
                                `mask_sampling_type` may take, the keyword names of the Point objects forward builds (outer and
                                `leaf_point`) and the keys of the dict forward passes to point.update
"""
import ast
import json
import os
import sys

AUTOENCODER = "lightning/point_decoder/autoencoder.py"


def params(fn):
    return [a.arg for a in fn.args.args]


def function(tree, name):
    return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)


def is_point_call(node):
    return isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "Point"


def mask_class(tree, name):
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    attributes = []
    for node in ast.walk(fns["__init__"]):
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self" and t.attr not in attributes:
                    attributes.append(t.attr)
    sampling = next(ast.literal_eval(n.test.comparators[0]) for n in ast.walk(fns["__init__"])
                    if isinstance(n, ast.Assert) and isinstance(n.test, ast.Compare) and isinstance(n.test.left, ast.Name)
                    and n.test.left.id == "mask_sampling_type")
    res = {"bases": [ast.unparse(b) for b in cls.bases], "init": params(fns["__init__"]), "forward": params(fns["forward"]),
           "attributes": attributes, "sampling_types": sampling}
    outer = [n for n in ast.walk(fns["forward"]) if is_point_call(n) and any(k.arg == "leaf_point" for k in n.keywords)]
    if outer:
        keys = {tuple(k.arg for k in n.keywords) for n in outer}
        leaf = {tuple(k.arg for k in next(v.value for v in n.keywords if v.arg == "leaf_point").keywords) for n in outer}
        assert len(keys) == 1 and len(leaf) == 1, "the branches of forward build different Points"
        res["point_keys"], res["leaf_point_keys"] = list(keys.pop()), list(leaf.pop())
    dicts = [n.value for n in ast.walk(fns["forward"]) if isinstance(n, ast.Assign) and isinstance(n.value, ast.Dict)
             and any(isinstance(t, ast.Name) and t.id == "dict_to_update" for t in n.targets)]
    if dicts:
        keys = {tuple(ast.literal_eval(k) for k in d.keys) for d in dicts}
        assert len(keys) == 1, "the branches of forward update different keys"
        res["update_keys"] = list(keys.pop())
    return res


def main():
    tree = ast.parse(open(os.path.join(sys.argv[1], AUTOENCODER)).read())
    res = {"top_k": {"params": params(function(tree, "top_k"))}, "top_p": {"params": params(function(tree, "top_p"))},
           "MaskModule": mask_class(tree, "MaskModule"), "MaskResModule": mask_class(tree, "MaskResModule")}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "densify_surface.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
