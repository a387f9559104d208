"""The ctypes bindings are derived from include/deig.h (_lib.parse_header): the type rule
pinned on five prototypes that cover every case of it, the parser's refusals, the derived
constants, and the options struct's size against the library's own (CPU)."""
import ctypes

import pytest

from distributed_eigenspaces_amd import _lib

_int, _i64, _sz, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
_f32, _f64, _opts = ctypes.c_float, ctypes.c_double, ctypes.POINTER(_lib.SolverOpts)

PINNED = {
    "deig_last_error": (ctypes.c_char_p, []),
    "deig_shutdown": (None, []),
    "deig_syrk_u8_centered": (_int, [_vp, _i64, _i64, _i64, _int, _vp, _f64, _vp, _i64, _vp, _i64,
                                     _vp, _vp, _sz, _vp]),
    "deig_topk_sym_batch_ex": (_int, [_int, _vp, _int, _i64, _i64, _int, _int, _int, _f32, _vp,
                                      _i64, _vp, _vp, _vp, _vp, _opts, _vp, _sz, _vp]),
    "deig_topk_workspace_ex": (_sz, [_i64, _int, _int, _int, _opts]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_derived_signature(name):
    assert _lib.SIGNATURES[name] == PINNED[name]


def test_every_prototype_is_derived():
    assert sorted(_lib.SIGNATURES) == _lib.header_symbols()
    assert len(_lib.SIGNATURES) >= 52


def test_unknown_type_raises_naming_the_prototype():
    with pytest.raises(ValueError, match=r"'long n'.*deig_x"):
        _lib.parse_header("int deig_x(long n);")
    with pytest.raises(ValueError, match="deig_x"):
        _lib.parse_header("float* deig_x(int n);")  # only const char* may be returned
    with pytest.raises(ValueError, match="deig_x"):
        _lib.parse_header("int deig_x(unsigned int n);")


def test_counted_but_unparsed_prototype_raises():
    with pytest.raises(ValueError, match="deig_y"):
        _lib.parse_header("int deig_ok(int n);\nint deig_y(int (*cb)(int));")
    # a name inside a comment is not counted
    protos, _, _ = _lib.parse_header("/* see deig_y() */ int deig_ok(int n); // deig_z(")
    assert protos == {"deig_ok": (_int, [_int])}


def test_derived_constants():
    assert _lib.DEIG_SYRK_DEFAULT == _lib.DEIG_SYRK_AUTO
    assert _lib.DEIG_EINVAL == -1
    assert _lib.DEIG_SWEEP_HALF == 0x1000
    assert not hasattr(_lib, "DEIG_H")  # the include guard is no constant
    _, consts, _ = _lib.parse_header("#define DEIG_A (-3) /* c */\n#define DEIG_B DEIG_A\n"
                                     "#define DEIG_C 0x10\n#define DEIG_GUARD\n")
    assert consts == {"DEIG_A": -3, "DEIG_B": -3, "DEIG_C": 16}


def test_solver_opts_size_is_the_library_s():
    """The one check of the derived struct that is not circular: the size the library
    itself writes into a zeroed block."""
    o = _lib.SolverOpts()
    _lib.lib().deig_solver_opts_init(ctypes.byref(o))
    assert o.size == ctypes.sizeof(_lib.SolverOpts)
