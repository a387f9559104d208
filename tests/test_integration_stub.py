"""CPU checks of the reference-side binding (integration/deig_backend.py): it imports
nothing but ctypes, numpy and the standard library (a maintainer drops it next to the
reference's distributed.py), every libdeig symbol it binds is declared in
include/deig.h and exported by the built library, and its literal signatures agree
with the ones _lib derives from the header."""
import ast
import ctypes
import os
import re

import pytest

from distributed_eigenspaces_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "integration", "deig_backend.py")


def _tree():
    return ast.parse(open(STUB).read())


def test_stub_imports_only_ctypes_numpy():
    mods = set()
    for node in ast.walk(_tree()):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods <= {"ctypes", "numpy", "os", "warnings", "__future__"}, mods


def test_stub_binds_declared_exported_symbols():
    src = open(STUB).read()
    bound = sorted({n for n in _lib.header_symbols() if f"_L.{n}" in src})
    assert {"deig_syrk_shift", "deig_topk_sym_ex", "deig_projavg_topk_f32"} <= set(bound)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdeig.so not built")
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in bound:
        assert hasattr(L, name), name


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


def test_stub_signatures_match_the_header():
    """The stub keeps a literal table of its own (it may import only ctypes and numpy); what
    it binds must agree with the signatures derived from include/deig.h: the same restype,
    the same number of arguments, the same ctypes type at each non-pointer position and a
    pointer type wherever the header has a pointer."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdeig.so not built")
    import importlib.util
    spec = importlib.util.spec_from_file_location("deig_backend_under_test", STUB)
    stub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stub)
    stub._load()
    bound = sorted(set(re.findall(r"\bL\.(deig_\w+)", open(STUB).read())))
    assert len(bound) >= 9 and set(bound) <= set(_lib.SIGNATURES)
    for name in bound:
        res, args = _lib.SIGNATURES[name]
        fn = getattr(stub._L, name)
        assert fn.restype is res, (name, fn.restype, res)
        mine = list(fn.argtypes or [])
        assert len(mine) == len(args), (name, len(mine), len(args))
        for i, (a, b) in enumerate(zip(mine, args)):
            if _is_pointer(b):
                assert _is_pointer(a), (name, i, a, b)
            else:
                assert a is b, (name, i, a, b)
