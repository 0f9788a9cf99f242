"""The ctypes binding against the header, declaration by declaration: every SONIC_API function of include/sonic_hip.h has an entry in
sonicscribe_amd.engine.SIGNATURES with the same number of arguments, a pointer where the header has one, a scalar of the same width and float-ness where it
has not, and the same return type.  ctypes checks none of this at a call - one argument too few is silent stack corruption.  Needs no library."""
import ctypes as C
import os
import re

import abi_pins
from sonicscribe_amd.engine import SIGNATURES, EXPORTS

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sonic_hip.h")
SCALARS = {"int": ("i", 4), "int32_t": ("i", 4), "int64_t": ("i", 8), "uint64_t": ("i", 8), "float": ("f", 4)}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p, "void": None}


def declarations():
    """name -> (return type, [argument type]) as the header spells them, the argument names dropped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, args in re.findall(r"\bSONIC_API\s+([\w\s]+?\**)\s*(sonic_\w+)\s*\(([^)]*)\)\s*;", text):
        args = " ".join(args.split())
        types = []
        for a in ([] if args in ("", "void") else args.split(",")):
            a = a.strip()
            ptr = "*" in a or "[" in a
            base = re.sub(r"\bconst\b", "", a.replace("*", " ")).split()
            types.append("*" if ptr else " ".join(base[:-1]))          # the last word of a scalar argument is its name
        assert name not in out, name
        out[name] = (" ".join(ret.split()).replace(" *", "*"), types)
    return out


def kind(t):
    """a ctypes argument type -> '*' for anything passed as an address, else (integer or float, bytes)"""
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return "*"
    return ("f" if t in (C.c_float, C.c_double) else "i", C.sizeof(t))


def mismatches(table):
    decl = declarations()
    bad = []
    if set(decl) != set(table):
        bad.append(f"names: header only {sorted(set(decl) - set(table))}, binding only {sorted(set(table) - set(decl))}")
    for name in sorted(set(decl) & set(table)):
        ret, args = decl[name]
        restype, argtypes = table[name]
        if ret not in RETURNS or RETURNS[ret] is not restype:
            bad.append(f"{name}: returns {ret}, bound as {restype}")
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments, bound with {len(argtypes)}")
            continue
        for i, (a, t) in enumerate(zip(args, argtypes)):
            if (a if a == "*" else SCALARS[a]) != kind(t):
                bad.append(f"{name}: argument {i} is {a}, bound as {t.__name__}")
    return bad


def test_every_declaration_matches_its_binding():
    abi_pins.check_surface()
    assert len(declarations()) == len(EXPORTS) == abi_pins.N_EXPORTS
    assert mismatches(SIGNATURES) == []


def test_the_check_sees_a_missing_argument_and_a_wrong_width():
    short = dict(SIGNATURES)
    restype, argtypes = short["sonic_test_attention"]
    short["sonic_test_attention"] = (restype, argtypes[:-1])
    assert mismatches(short) == ["sonic_test_attention: 12 arguments, bound with 11"]
    wide = dict(SIGNATURES)
    wide["sonic_debug_read"] = (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int])       # n is int64_t
    assert mismatches(wide) == ["sonic_debug_read: argument 4 is int64_t, bound as c_int"]
