"""The C ABI of the HIP library is declared once, in csrc/hip/jb_hip_api.h,
and the ctypes table of ops/hip.py matches it by type: every argument and the
return type of every entry. The compiler holds the definitions and the native
callers to the same header, so an ABI slip is caught on the CPU instead of as
a garbage argument of a kernel launch."""
import ctypes
import glob
import os
import re

from jubatus_amd.ops import hip

CSRC = os.path.normpath(os.path.join(os.path.dirname(hip.__file__), "..", "csrc"))
HEADER = os.path.join(CSRC, "hip", "jb_hip_api.h")

_SCALARS = {
    "int": ctypes.c_int32, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
    "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
}
_NOT_A_TYPE = {"return", "else", "do", "throw", "case", "goto", "new", "delete", "sizeof"}


def _code(path):
    """the file without comments and with every string literal emptied
    (extern "C" reads extern "" from here on)"""
    text = open(path, encoding="utf-8").read()
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _ctype(decl, name, returns=False):
    """the ctypes type of one parameter declaration or return type"""
    decl = " ".join(decl.split())
    if "*" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split(" ") if w != "const"]
    if not returns:
        assert len(words) >= 2, f"{name}: parameter '{decl}' has no name"
        words = words[:-1]
    base = " ".join(words)
    if base == "hipStream_t":
        return ctypes.c_void_p
    if returns and base == "void":
        return None
    assert base in _SCALARS, f"{name}: no ctypes mapping for '{decl}'"
    return _SCALARS[base]


def _header():
    """{name: (restype, [argtypes])} of every declaration, and the names in
    the order they appear (a repeat shows as a repeat)"""
    text = _code(HEADER)
    blocks = re.findall(r'extern ""\s*\{(.*?)\n\}', text, flags=re.S)
    assert len(blocks) == 1, 'jb_hip_api.h must hold exactly one extern "C" block'
    assert len(re.findall(r'extern ""', text)) == 1
    decls, order = {}, []
    for stmt in blocks[0].split(";"):
        if not stmt.strip():
            continue
        m = re.fullmatch(r"\s*(.*?)\b(jb_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        assert m, f"not a jb_* prototype: {stmt.strip()!r}"
        ret, name, params = m.groups()
        args = [_ctype(p, name) for p in params.split(",") if p.strip()]
        decls[name] = (_ctype(ret, name, returns=True), args)
        order.append(name)
    return decls, order


def _prototype_only(path):
    """jb_* functions that `path` declares without defining, on an extern "C"
    line or inside a block alike: a type in front of the name, a ';' after
    the parameter list"""
    text = _code(path)
    found = []
    for m in re.finditer(r"\b(jb_\w+)\s*\(", text):
        before = re.search(r"(\w+)[\s\*]*$", text[max(0, m.start() - 200):m.start()])
        if not before or before.group(1) in _NOT_A_TYPE:
            continue   # a call: no type in front of the name
        depth, k = 0, m.end() - 1
        while True:
            depth += {"(": 1, ")": -1}.get(text[k], 0)
            if depth == 0:
                break
            k += 1
        if text[k + 1:k + 200].lstrip().startswith(";"):
            found.append(m.group(1))
    return found


def _definitions():
    """{name: [files]} of every extern "C" jb_* definition in csrc/hip/*.hip"""
    defs = {}
    for f in sorted(glob.glob(os.path.join(CSRC, "hip", "*.hip"))):
        text = _code(f)
        for m in re.finditer(r'extern ""\s+[\w\s\*]*?\b(jb_\w+)\s*\(', text):
            defs.setdefault(m.group(1), []).append(os.path.basename(f))
    return defs


def test_ctypes_signatures_match_header():
    decls, _ = _header()
    assert decls, "no prototypes found"
    for name, (restype, argtypes) in hip._SIGS.items():
        assert name in decls, f"{name} is not declared in jb_hip_api.h"
        want_ret, want_args = decls[name]
        assert restype is want_ret, (name, "return type", restype, want_ret)
        assert len(argtypes) == len(want_args), (name, len(argtypes), len(want_args))
        for i, (got, want) in enumerate(zip(argtypes, want_args)):
            assert got is want, (name, f"argument {i}", got, want)


def test_header_declares_every_definition_once():
    _, order = _header()
    defs = _definitions()
    assert len(defs) > 50, "no definitions found"
    for name, files in defs.items():
        assert len(files) == 1, (name, files)
        assert order.count(name) == 1, f"{name} ({files[0]}) is declared {order.count(name)} times"
    for name in order:
        assert name in defs, f"{name} is declared but no .hip file defines it"


def test_no_prototype_outside_the_header():
    files = [f for f in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True)
             if os.path.isfile(f) and f.endswith((".hip", ".hpp", ".h", ".cpp", ".c", ".cc"))
             and os.sep + "build" + os.sep not in f]
    assert len(files) > 50
    assert _prototype_only(HEADER), "the scan finds no prototype where there are some"
    for f in files:
        if os.path.samefile(f, HEADER):
            continue
        assert not _prototype_only(f), (os.path.relpath(f, CSRC), _prototype_only(f))
