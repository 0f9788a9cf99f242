"""The C ABI's pins, once (imported like glue_ref.py; not collected): the version, the number of entry points, and the one check that holds the header, the
binding table, exports.map and the built library to each other.  A pull request that adds an export changes the two integers below; the host tests of the
features call check_surface() with the names, option keys and header strings they brought."""
import ctypes
import os
import re

from sonicscribe_amd import engine

ABI_VERSION = 13
N_EXPORTS = 101

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sonic_hip.h")
CSRC = os.path.join(ROOT, "sonicscribe_amd", "csrc")


def header():
    return open(HEADER).read()


def declared(hdr=None):
    """the names declared `SONIC_API ... sonic_x(`, in the header's order, comments dropped"""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", header() if hdr is None else hdr, flags=re.S))
    return re.findall(r"\bSONIC_API\b[^;]*?\b(sonic_\w+)\s*\(", text)


def check_surface(names=(), options=(), header_strings=(), engine_methods=()):
    hdr = header()
    m = re.search(r"#define\s+SONIC_ABI_VERSION\s+(\d+)\b", hdr)
    assert m and int(m.group(1)) == ABI_VERSION == engine.ABI_VERSION, (m and m.group(1), ABI_VERSION, engine.ABI_VERSION)
    decl = declared(hdr)
    assert len(decl) == len(set(decl)) == len(engine.EXPORTS) == N_EXPORTS, (len(decl), len(engine.EXPORTS), N_EXPORTS)
    assert set(decl) == set(engine.EXPORTS), sorted(set(decl) ^ set(engine.EXPORTS))
    assert engine.EXPORTS == list(engine.SIGNATURES)
    emap = open(os.path.join(CSRC, "exports.map")).read()
    assert "global: sonic_*" in emap
    pattern = re.search(r"global:\s*([^;]+);", emap).group(1).strip().replace("*", ".*")
    for n in names:
        assert re.search(r"SONIC_API int " + n + r"\(", hdr) and n in engine.EXPORTS and re.fullmatch(pattern, n), n
    src = open(os.path.join(CSRC, "engine_options.cpp")).read()
    for key in options:
        assert '{"%s", APPLY(opt_%s)}' % (key, key) in src and key in hdr, key
    for s in header_strings:
        assert s in hdr, s
    for meth in engine_methods:
        assert hasattr(engine.Engine, meth), meth
    if os.path.exists(engine.LIB_PATH):
        lib = ctypes.CDLL(engine.LIB_PATH)
        assert lib.sonic_abi_version() == ABI_VERSION
        for n in list(names) + engine.EXPORTS:
            assert hasattr(lib, n), n
