"""Records the call surface the reference's caller modules use from this repo's drop-in packages, as a list of names
(tests/golden/dropin_surface.json, read by tests/test_dropin_reference.py).  Authoring only: it needs the reference tree,
which the tests never read.

    python tests/golden/make_dropin_surface.py REFERENCE_TREE

Per caller module (lightning/renderer.py, lightning/renderer_2dgs.py, lightning/utils.py), parsed with `ast`, nothing
imported or executed:
  imports              {package: [names]} of its `from <package> import ...` of the drop-in packages
  settings_keywords    the keyword names of its GaussianRasterizationSettings(...) call
  rasterizer_keywords  the keyword names of its GaussianRasterizer(...) call
  call_keywords        the keyword names of its `rasterizer(...)` call (the forward of the rasterizer module)
  call_outputs         how many values it unpacks from that call
  signatures           {Class.method: [parameter names]} of the methods its callers use (Renderer, MiniCam)
"""
import ast
import json
import os
import sys

PACKAGES = ("diff_gaussian_rasterization", "diff_surfel_rasterization", "simple_knn._C")
MODULES = ("lightning/renderer.py", "lightning/renderer_2dgs.py", "lightning/utils.py")
METHODS = {"Renderer": ("__init__", "set_bg_color", "set_rasterizer", "render_img"), "MiniCam": ("__init__",)}


def _callee(node):
    f = node.func
    return f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None


def surface(path):
    tree = ast.parse(open(path).read())
    out = {"imports": {}, "settings_keywords": None, "rasterizer_keywords": None, "call_keywords": None,
           "call_outputs": None, "signatures": {}}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module in PACKAGES:
            out["imports"].setdefault(node.module, []).extend(a.name for a in node.names)
        elif isinstance(node, ast.Call) and _callee(node) == "GaussianRasterizationSettings":
            out["settings_keywords"] = [k.arg for k in node.keywords]
        elif isinstance(node, ast.Call) and _callee(node) == "GaussianRasterizer":
            out["rasterizer_keywords"] = [k.arg for k in node.keywords]
        elif (isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and _callee(node.value) == "rasterizer"
              and isinstance(node.targets[0], ast.Tuple)):
            out["call_keywords"] = [k.arg for k in node.value.keywords]
            out["call_outputs"] = len(node.targets[0].elts)
        elif isinstance(node, ast.ClassDef) and node.name in METHODS:
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name in METHODS[node.name]:
                    out["signatures"][f"{node.name}.{f.name}"] = [a.arg for a in f.args.args]
    return out


def main():
    ref = sys.argv[1]
    res = {m: surface(os.path.join(ref, m)) for m in MODULES}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_surface.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
