"""The C-ABI of `libief_hip.so` as ctypes declarations, read from `include/ief_hip.h` itself.

The header is the single source of truth: `hip.py` binds what this module derives from it and declares nothing by
hand.  Pure Python (no torch), and the library is never loaded here.

    structs    name -> ctypes.Structure subclass, in header order
    functions  name -> (restype, argtypes)
    defines    name -> value of the integer #defines

The parser is STRICT: once comments, preprocessor lines, the `ief_half` typedefs and the `extern "C"` braces are
gone, every statement must be a `typedef struct X { ... } X;` of scalar / pointer fields or a prototype over the
types below.  Anything else (an array, a double, a struct by value, a function pointer, an unknown type name)
raises HeaderError quoting the statement: a declaration this module does not understand must never be bound.
"""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ief_hip.h")

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "long long": ctypes.c_longlong}
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p, "void": None}
# what a pointer may point at besides the header's own structs; callers pass data_ptr() integers and None
_POINTEES = set(_SCALARS) | {"void", "ief_half", "unsigned char"}

_TYPE = r"long long|unsigned char|\w+"
_STRUCT = re.compile(r"typedef struct (\w+) ?\{([^{}]*)\} ?(\w+) ?;")
_DECL = re.compile(rf"(const )?({_TYPE})( ?\* ?| )(\w+(?: ?, ?\w+)*)")
_PROTO = re.compile(rf"(const char ?\*|{_TYPE}) ?(\w+) ?\((.*)\)")


class HeaderError(ValueError):
    pass


def _declaration(stmt, structs, where):
    """`[const] T[*] a, b, ...` -> (ctype, [names])."""
    m = _DECL.fullmatch(stmt)
    const, base, sep, names = m.groups() if m else (None, None, "", "")
    names = re.split(r" ?, ?", names)
    if "*" in sep and len(names) == 1 and (base in _POINTEES or base in structs):
        return (ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p), names
    if m and "*" not in sep and not const and base in _SCALARS:
        return _SCALARS[base], names
    raise HeaderError(f"unsupported declaration `{stmt}` in `{where}`")


def parse(text):
    """(structs, functions, defines) of a header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {k: int(v, 0) for k, v in
               re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M)}
    text = " ".join(re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).split())
    text = re.sub(r"typedef \w+ ief_half ?;", "", text)
    text, braces = re.subn(r'extern "C" ?\{', "", text)
    text = text.strip()
    if braces:
        if braces > 1 or not text.endswith("}"):
            raise HeaderError('unbalanced extern "C" block')
        text = text[:-1]
    structs, functions, pos = {}, {}, 0
    while pos < len(text):
        if text[pos] == " ":
            pos += 1
            continue
        m = _STRUCT.match(text, pos)
        if m:
            name, body, alias = m.groups()
            if name != alias or name in structs:
                raise HeaderError(f"struct {name}: typedef'd as {alias}, or declared twice")
            fields = []
            for stmt in filter(None, (s.strip() for s in body.split(";"))):
                ctype, names = _declaration(stmt, structs, f"struct {name}")
                fields += [(n, ctype) for n in names]
            if not fields or len({n for n, _ in fields}) != len(fields):
                raise HeaderError(f"struct {name}: empty, or a field named twice")
            structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
            pos = m.end()
            continue
        end = text.find(";", pos)
        stmt = text[pos:end].strip() if end >= 0 else text[pos:].strip()
        m = _PROTO.fullmatch(stmt) if end >= 0 else None
        ret = m and re.sub(r" ?\*", "*", m.group(1))
        if not m or ret not in _RETURNS or m.group(2) in functions:
            raise HeaderError(f"neither a struct nor a prototype this binding supports (or declared twice): `{stmt}`")
        name, params = m.group(2), m.group(3).strip()
        functions[name] = (_RETURNS[ret], [_declaration(prm.strip(), structs, stmt)[0]
                                           for prm in ([] if params == "void" else params.split(","))])
        pos = end + 1
    return structs, functions, defines


with open(HEADER) as _f:
    structs, functions, defines = parse(_f.read())
