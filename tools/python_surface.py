#!/usr/bin/env python3
"""The Python surface of the package as data: the public names of `bonnie32_amd` and `bonnie32_amd.rasterizer`, and the signature of
every public function, class and public method among the latter.  tests/test_python_surface.py compares the tree with
tests/golden/python_surface.json; a refactor that moves code between modules must reproduce the file byte for byte.

    python tools/python_surface.py            # print the surface
    python tools/python_surface.py --write    # record it into tests/golden/python_surface.json (only when the surface is MEANT to change)

Needs no library and no device: nothing here is called, only looked at."""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "python_surface.json")


def _public(module):
    """The names a module exposes: __all__ where it states one, else what does not start with an underscore and is not a module."""
    names = getattr(module, "__all__", None)
    if names is None:
        names = [n for n, v in vars(module).items() if not n.startswith("_") and not inspect.ismodule(v)]
    return sorted(names)


def _signature(f):
    try:
        return str(inspect.signature(f))
    except (TypeError, ValueError):
        return None


def _members(cls):
    """Public methods (signature) and properties ("property") of a class, inherited ones included."""
    out = {}
    for name in dir(cls):
        if name.startswith("_"):
            continue
        m = inspect.getattr_static(cls, name)
        if isinstance(m, (staticmethod, classmethod)):
            out[name] = type(m).__name__ + _signature(m.__func__)
        elif isinstance(m, property):
            out[name] = "property"
        elif inspect.isfunction(m):
            out[name] = _signature(m)
    return out


def surface():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bonnie32_amd
    from bonnie32_amd import rasterizer
    package = _public(bonnie32_amd)
    missing = [n for n in package if not hasattr(bonnie32_amd, n)]
    if missing:
        raise AttributeError("bonnie32_amd.__all__ names what it does not have: %s" % missing)
    signatures = {}
    for name in _public(rasterizer):
        v = getattr(rasterizer, name)
        if inspect.isclass(v):
            signatures[name] = {"class": _signature(v), "members": _members(v)}
        elif inspect.isfunction(v):
            signatures[name] = _signature(v)
    return {"bonnie32_amd": package, "bonnie32_amd.rasterizer": _public(rasterizer), "signatures": signatures}


def dumps(s):
    return json.dumps(s, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    text = dumps(surface())
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
