"""The C signatures of include/flvis_hip.h as ctypes declarations: read from the header once, applied to the library once.

A new entry point needs no line here or at its call site: declare it in the header and the signature follows.  Every pointer
parameter is c_void_p, which takes what callers hand over (c_void_p, int, byref(...), ctypes arrays, POINTER(T) instances,
numpy's .ctypes.data_as(...), bytes, None); a scalar parameter takes a Python or numpy number, or the ctypes instance of its own type.
"""
import ctypes as C
import os
import re

from . import build as _build

HEADER = os.path.join(_build.HERE, "..", "include", "flvis_hip.h")

_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
            "double": C.c_double, "float": C.c_float}
_RETURNS = {"int": C.c_int, "void": None, "void*": C.c_void_p, "const char*": C.c_char_p}
_PROTO =re.compile(r"(const\s+)?(\w+)\s*(\*?)\s*(flvis_\w+)\s*\(([^()]*)\)")


class FlvisError(RuntimeError):
    pass


def _bad(name, ctype):
    return FlvisError("include/flvis_hip.h: %s has the type '%s', which the binding does not map to ctypes" % (name, ctype))


def parse(text):
    """{name: (restype, [argtypes])} for every `ret name(params);` of a header's text.  FlvisError for a type outside the header's
    vocabulary (int, int64_t, uint32_t, uint64_t, size_t, double, float, pointers; const char* / void* / void returns): no guess."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    table = {}
    for stmt in text.split(";"):
        stmt = stmt.strip()
        m = _PROTO.fullmatch(stmt)
        if not m:
            odd = re.search(r"(flvis_\w+)\s*\(", stmt)
            if odd:
                raise _bad(odd.group(1), " ".join(stmt[:odd.start()].split()))
            continue
        const, ret, star, name, params = m.groups()
        ret = ("const " if const else "") + ret + star
        if ret not in _RETURNS:
            raise _bad(name, ret)
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            if "*" in p:
                args.append(C.c_void_p)
                continue
            words = [w for w in p.split() if w != "const"]
            if not 1 <= len(words) <= 2 or words[0] not in _SCALARS:
                raise _bad(name, " ".join(words[:-1] if len(words) > 1 else words))
            args.append(_SCALARS[words[0]])
        table[name] = (_RETURNS[ret], args)
    return table


_TABLE = None


def signatures():
    """parse() of include/flvis_hip.h, read once per process"""
    global _TABLE
    if _TABLE is None:
        with open(HEADER) as f:
            _TABLE = parse(f.read())
    return _TABLE


def declare(lib):
    """Sets restype and argtypes of every declared function the library exports.  One it lacks (an older build behind FLVIS_LIB_PATH) is
    skipped: its call site fails with AttributeError."""
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
