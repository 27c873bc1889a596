"""The Python-visible surface of pycolmap_amd._pycolmap as one digest per top-level name: what a refactor of the
binding layer must leave as it is.  tests/golden/make_host_surface_golden.py freezes it, tests/test_host_surface_cpu.py
compares."""
import hashlib
import json

# the interpreter's own entries of a class dict, and the module attributes that name the file the module was loaded from
_SKIPPED_CLASS_ENTRIES = ("__dict__", "__weakref__", "__module__")
_SKIPPED_MODULE_ATTRS = ("__file__", "__loader__", "__spec__", "__builtins__", "__cached__", "__path__")
_SCALARS = (bool, int, float, str, bytes, type(None))


def _entry(value):
    """type name and docstring of one entry of a class dict; for a property also whether it can be set, and the
    getter's docstring"""
    rec = {"type": type(value).__name__, "doc": getattr(value, "__doc__", None)}
    if isinstance(value, property):
        rec["setter"] = value.fset is not None
        rec["getter_doc"] = getattr(value.fget, "__doc__", None)
    return rec


def _describe(value):
    if isinstance(value, type):
        return {"kind": "class", "doc": value.__doc__,
                "entries": {k: _entry(v) for k, v in sorted(vars(value).items()) if k not in _SKIPPED_CLASS_ENTRIES}}
    if isinstance(value, _SCALARS):
        return {"kind": "scalar", "type": type(value).__name__, "repr": repr(value)}
    if callable(value):
        return {"kind": "callable", "type": type(value).__name__, "doc": value.__doc__}
    return {"kind": type(value).__name__}  # a dict such as _last_stats: its content is the last call's, not surface


def host_surface():
    """{name: sha256 of the canonical JSON of what the name is} for every attribute of pycolmap_amd._pycolmap"""
    from pycolmap_amd import _pycolmap as P
    out = {}
    for name in sorted(vars(P)):
        if name in _SKIPPED_MODULE_ATTRS:
            continue
        text = json.dumps(_describe(getattr(P, name)), sort_keys=True, ensure_ascii=True, default=repr)
        out[name] = hashlib.sha256(text.encode()).hexdigest()
    return out
