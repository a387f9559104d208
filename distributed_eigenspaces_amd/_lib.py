"""ctypes binding of libdeig.so (the C ABI declared in include/deig.h).

ctypes releases the GIL for the duration of each call, so several
``my_threading.Slave`` worker threads can drive the GPU concurrently.
There is no CPU fallback: if the library is missing the import of an op raises.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import re
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
# DEIG_LIB_PATH: an A/B variant built by tools/ (_build.build_library(defines=...));
# the product default is the in-tree libdeig.so.
LIB_PATH = os.environ.get("DEIG_LIB_PATH") or os.path.join(HERE, "libdeig.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "deig.h")


class SolverOpts(ctypes.Structure):
    """``deig_solver_opts`` (include/deig.h); build with :func:`solver_opts`.  Its
    ``_fields_`` are the header's, set below once the header is parsed."""


_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}


def _ctype(decl: str, proto: str, ret: bool = False):
    """ctypes type of one C declaration (a return type, or a parameter with or without its
    name).  Pointers are c_void_p (device pointers are passed as integers, host ones with
    byref or as ctypes arrays) except the options struct; an unknown type raises."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        if ret:
            if words == ["char", "*"]:
                return ctypes.c_char_p
        else:
            return ctypes.POINTER(SolverOpts) if words[0] == "deig_solver_opts" else ctypes.c_void_p
    elif ret and words == ["void"]:
        return None
    elif words and words[0] in _SCALARS and len(words) <= (1 if ret else 2):
        return _SCALARS[words[0]]
    raise ValueError(f"include/deig.h: no ctypes type for {decl.strip()!r} in {proto!r}")


def parse_header(text: str):
    """``(prototypes, constants, fields)`` of a deig.h text: ``{name: (restype, [argtypes])}``
    of every ``deig_*`` function, ``{name: int}`` of every ``#define DEIG_<NAME>`` with an
    integer value (or another DEIG_ name's), and deig_solver_opts' ``[(field, ctype)]``."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for name, val in re.findall(r"^#define[ \t]+(DEIG_[A-Z0-9_]+)[ \t]+"
                                r"\(?(-?(?:0x[0-9a-fA-F]+|\d+)|DEIG_[A-Z0-9_]+)\)?[ \t]*$", text, re.M):
        consts[name] = consts[val] if val.startswith("DEIG_") else int(val, 0)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    fields = []
    struct = re.search(r"typedef struct deig_solver_opts \{(.*?)\} deig_solver_opts;", text, re.S)
    if struct:
        fields = [(f.split()[-1], _ctype(f, "deig_solver_opts"))
                  for f in struct.group(1).split(";") if f.strip()]
        text = text.replace(struct.group(0), " ")
    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s*]*?)\b(deig_[a-z0-9_]+)\s*\(([^()]*)\)\s*;",
                                      text):
        proto = f"{' '.join(ret.split())} {name}({' '.join(args.split())})"
        params = [] if args.strip() in ("", "void") else args.split(",")
        protos[name] = (_ctype(ret, proto, ret=True), [_ctype(a, proto) for a in params])
    lost = set(re.findall(r"\b(deig_[a-z0-9_]+)\s*\(", text)) - set(protos)
    if lost:
        raise ValueError(f"include/deig.h: cannot parse the prototype of {sorted(lost)}")
    return protos, consts, fields


# The header is the single source: entry-point signatures, DEIG_* constants (module
# attributes below) and the options struct are all read from it.
SIGNATURES, _consts, SolverOpts._fields_ = parse_header(open(HEADER).read())
globals().update(_consts)

# name -> code of the algorithm / mode arguments (the names are Python's)
SYRK_ALGOS = {"auto": DEIG_SYRK_AUTO, "split3": DEIG_SYRK_SPLIT3, "fp32": DEIG_SYRK_FP32}
SWEEP_ALGOS = {"auto": DEIG_SWEEP_AUTO, "bf16x6": DEIG_SWEEP_BF16X6, "fp32": DEIG_SWEEP_FP32}
U8_MODES = {"raw": DEIG_U8_RAW, "gray": DEIG_U8_GRAY3}
OJA_ALGOS = {"auto": DEIG_OJA_AUTO, "two_pass": DEIG_OJA_TWO_PASS, "resident": DEIG_OJA_RESIDENT}

_lock = threading.Lock()
_lib = None


class DeigError(RuntimeError):
    """A libdeig call failed (HIP error or workspace problem)."""


class DeigTimeoutError(DeigError):
    """A resident Oja run's hand-off waited past its bound (DEIG_ETIMEOUT): the basis
    it wrote is NaN (CUs held by other work kept its grid from being co-resident)."""


class NotConvergedWarning(RuntimeWarning):
    """The eigensolver stopped at max_sweeps above its residual tolerance."""


def header_symbols(path: str = HEADER):
    """Function names declared in include/deig.h."""
    txt = open(path).read()
    return sorted(set(re.findall(r"\b(deig_[a-z0-9_]+)\s*\(", txt)))


def lib() -> ctypes.CDLL:
    """Load libdeig.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
                    "(hipcc, gfx950).  There is no CPU fallback.")
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
            # free the library's pinned host blocks while the HIP runtime is alive:
            # Python's atexit runs before the C runtime's exit handlers (and the HIP
            # runtime's teardown), include/deig.h deig_shutdown
            atexit.register(_shutdown)
    return _lib


def _shutdown():
    if _lib is not None:
        try:
            _lib.deig_shutdown()
        except Exception:  # noqa: BLE001 - never raise from an exit handler
            pass


def solver_opts(**fields) -> SolverOpts:
    """Solver options: the library defaults (deig_solver_opts_init) with ``fields``
    overridden; DEIG_DEBUG=1 in the environment turns on the per-RR trace."""
    o = SolverOpts()
    lib().deig_solver_opts_init(ctypes.byref(o))
    if os.environ.get("DEIG_DEBUG", "") == "1":
        o.debug = 1
    for name, value in fields.items():
        if value is not None:
            setattr(o, name, value)
    return o


def last_error() -> str:
    msg = lib().deig_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str) -> int:
    """Map a libdeig return code to Python exceptions (0 and NOT_CONVERGED pass)."""
    if rc in (DEIG_OK, DEIG_NOT_CONVERGED):
        return rc
    msg = f"{what}: {last_error()} (code {rc})"
    if rc == DEIG_EINVAL:
        raise ValueError(msg)
    if rc == DEIG_ETIMEOUT:
        raise DeigTimeoutError(msg)
    raise DeigError(msg)
