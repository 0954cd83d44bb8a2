"""CPU tests of `cabi.py`, which derives the ctypes binding from `include/ief_hip.h`: its struct layouts and function
signatures are compared with what a real compiler makes of the same header (an independent reader), and declaration forms
it does not support raise instead of being skipped."""
import ctypes
import os
import shlex
import shutil
import subprocess

import pytest

from ief_amd import cabi, hip

INCLUDE = os.path.dirname(cabi.HEADER)


def _compiler(env, names, lang):
    """the first of $CC / $CXX, the usual driver names, ROCm's clang and `hipcc -x c|c++` that exists"""
    for cand in (shlex.split(os.environ.get(env, "")), *([n] for n in names), ["/opt/rocm/llvm/bin/" + names[-1]]):
        if cand and shutil.which(cand[0]):
            return cand
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # where the library's Makefile takes it from
    assert os.path.exists(hipcc), "no host compiler and no hipcc: the library cannot have been built either"
    return [hipcc, "-x", lang]


def _compile_and_run(tmp_path, cc, suffix, source, flags=()):
    src, exe = tmp_path / ("probe" + suffix), tmp_path / "probe"
    src.write_text(source)
    subprocess.run([*cc, *flags, "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def test_struct_layouts_equal_the_compilers(tmp_path):
    """sizeof of all 10 structs and offsetof / sizeof of every field, as the C compiler lays the header out"""
    assert len(cabi.structs) == 10
    prints, want = [], []
    for name, cls in cabi.structs.items():
        prints.append(f'printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {ctypes.sizeof(cls)}")
        for field, _ in cls._fields_:
            prints.append(f'printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
            want.append(f"{name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    source = "#include <stddef.h>\n#include <stdio.h>\n#include \"ief_hip.h\"\nint main(void) {\n" + "\n".join(prints) + "\nreturn 0; }\n"
    got = _compile_and_run(tmp_path, _compiler("CC", ("cc", "gcc", "clang"), "c"), ".c", source)
    assert got == want


_KIND = {ctypes.c_int: "int", ctypes.c_uint: "unsigned", ctypes.c_float: "float", ctypes.c_longlong: "long long",
         ctypes.c_void_p: "ptr", ctypes.c_char_p: "cstr", None: "void"}
_CLASSIFY = """
#include <cstdio>
#include <string>
#include "ief_hip.h"
template <class T> struct Kind;      /* a type the binding has no mapping for does not compile */
template <> struct Kind<int> { static std::string s() { return "int"; } };
template <> struct Kind<unsigned> { static std::string s() { return "unsigned"; } };
template <> struct Kind<float> { static std::string s() { return "float"; } };
template <> struct Kind<long long> { static std::string s() { return "long long"; } };
template <class T> struct Kind<T*> { static std::string s() { return "ptr"; } };
template <class T> struct Ret : Kind<T> {};
template <> struct Ret<void> { static std::string s() { return "void"; } };
template <> struct Ret<const char*> { static std::string s() { return "cstr"; } };
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void print(const char* name) {
        std::string s = std::string(name) + " " + Ret<R>::s() + " (";
        ((s += Kind<A>::s() + ","), ...);
        std::puts((s + ")").c_str());
    }
};
"""


def _kind(t):
    return _KIND[t] if t in _KIND else "ptr:" + t._type_.__name__      # POINTER(<struct>)


def test_signatures_equal_the_compilers(tmp_path):
    """return type and every parameter of each declared function, classified by the C++ compiler from `&ief_xxx` itself
    (unevaluated: nothing is linked): a dropped, added, reordered or mistyped parameter shows here"""
    assert len(cabi.functions) >= 100
    source = _CLASSIFY
    for name in cabi.structs:       # pointers to the header's own structs are told apart from every other pointer
        for q in ("", "const "):
            source += f'template <> struct Kind<{q}{name}*> {{ static std::string s() {{ return "ptr:{name}"; }} }};\n'
    source += "int main() {\n" + "".join(f'Sig<decltype(&{n})>::print("{n}");\n' for n in cabi.functions) + "return 0; }\n"
    got = _compile_and_run(tmp_path, _compiler("CXX", ("c++", "g++", "clang++"), "c++"), ".cpp", source, ["-std=c++17"])
    want = [f"{n} {_kind(res)} ({''.join(_kind(a) + ',' for a in args)})" for n, (res, args) in cabi.functions.items()]
    assert got == want


def test_binding_uses_the_derived_classes():
    """one class object per struct in the process: what callers instantiate is what the POINTER(...) argtypes name"""
    for name, cls in cabi.structs.items():
        assert getattr(hip, name) is cls
    assert hip.load().ief_gemm_f16.argtypes[0]._type_ is hip.IefGemmParams
    assert hip.load().ief_gemm_x3_set_variant.restype is None
    assert (hip.ABI_VERSION, hip.REPEAT_MAX_JOBS) == (cabi.defines["IEF_ABI_VERSION"], cabi.defines["IEF_REPEAT_MAX_JOBS"]) == (4, 4)


def test_declaration_forms_of_the_header():
    structs, functions, defines = cabi.parse("""
        #define IEF_N 0x10
        typedef uint16_t ief_half;
        extern "C" {
        typedef struct S { const ief_half* a; float* b; int M, N,
                           K; unsigned u, v; long long s; const void* p; float f; } S;   /* several per line, wrapped */
        long long ief_f(const S* s, S* t,
                        const unsigned char* img, int n, void* stream);   // wrapped prototype
        void ief_g(void); const char* ief_h(unsigned u, float x, long long n);
        }
    """)
    S = structs["S"]
    assert [(n, t) for n, t in S._fields_] == [
        ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int),
        ("u", ctypes.c_uint), ("v", ctypes.c_uint), ("s", ctypes.c_longlong), ("p", ctypes.c_void_p), ("f", ctypes.c_float)]
    res, args = functions["ief_f"]
    assert res is ctypes.c_longlong and args[0] is args[1] and args[0]._type_ is S
    assert args[2:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert functions["ief_g"] == (None, []) and functions["ief_h"] == (ctypes.c_char_p, [ctypes.c_uint, ctypes.c_float, ctypes.c_longlong])
    assert list(functions) == ["ief_f", "ief_g", "ief_h"] and defines == {"IEF_N": 16}


_S = "typedef struct S { int a; } S;\n"


@pytest.mark.parametrize("text, quoted", [
    ("typedef struct T { int a; float v[4]; } T;", "float v[4]"),                   # array field
    ("typedef struct T { int a; double x; } T;", "double x"),                        # double
    ("int ief_f(double x, void* stream);", "double x"),
    (_S + "int ief_f(S s, void* stream);", "S s"),                                   # struct by value
    ("typedef struct T { int (*cb)(int); } T;", "int (*cb)(int)"),                   # function-pointer field
    ("int ief_f(size_t n, void* stream);", "size_t n"),                              # unknown type names
    ("int ief_f(const Unknown* p, void* stream);", "const Unknown* p"),
    ("typedef struct T { int8_t a; } T;", "int8_t a"),
    ("double ief_f(int n);", "double ief_f(int n)"),                                 # unsupported return type
    ("int ief_f(float** pp);", "float** pp"),
    ("int ief_f();", "int ief_f()"),                                                 # unprototyped parameter list
    ("int ief_f(int n); int ief_f(int n);", "int ief_f(int n)"),                     # declared twice
    ("extern int ief_counter;", "extern int ief_counter"),                           # not a struct, not a prototype
    (_S + "typedef struct T { S s; } T;", "S s"),                                    # nested struct by value
    ("typedef struct T { union { int a; float b; } u; } T;", "typedef struct T"),    # nested braces
])
def test_unsupported_declarations_raise_and_name_the_statement(text, quoted):
    with pytest.raises(cabi.HeaderError) as err:
        cabi.parse(text)
    assert quoted in str(err.value)
