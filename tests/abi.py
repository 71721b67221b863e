"""The one ABI mechanism (CPU only): include/wgsparkl_hip.h read into a table, the table compiled into ONE gcc probe per dimension, and
the same questions put to the three hand-written mirrors — the ctypes binding, the Rust -sys file (which nothing here compiles: its
repr(C) layout is computed), the C++ wrapper. tests/test_abi.py asserts; nothing here does, except for the parser's own completeness.

A `Layout` is what both the compiler and the Rust model answer: size[struct], fields[struct] = {field: (offset, size)} in declaration
order, const[name] = value."""
import collections
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER_PATH = os.path.join(INCLUDE, "wgsparkl_hip.h")
HPP_PATH = os.path.join(INCLUDE, "wgsparkl_hip.hpp")
RUST_PATH = os.path.join(ROOT, "rust", "wgsparkl-hip-sys", "src", "lib.rs")

Header = collections.namedtuple("Header", "structs constants functions")   # {struct: [fields]}, [names], {name: (return type, parameter list)}
Layout = collections.namedtuple("Layout", "size fields const")
_RET = r"(?:const char \*|int32_t |uint32_t |void |wgs_status )"


def read(path):
    with open(path) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ the header
def header(text=None):
    """Every struct (field names in order), integer constant and function declaration of the header (`text`: a copy to parse instead)."""
    raw = read(HEADER_PATH) if text is None else text
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef struct\s*\{(.*?)\}\s*(wgs_\w+)\s*;", text, re.S):
        assert name not in structs, f"{name} is defined twice"
        structs[name] = [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", d).group(1)          # `float lambda, mu;`, `float m[3][4];`, `void *p;`
                         for stmt in body.split(";") if stmt.strip() for d in stmt.split(",")]
    assert len(structs) == len(re.findall(r"typedef struct\s*\{", text)), "a struct definition this parser cannot read"
    found = [n for block in re.findall(r"\benum\s*\{(.*?)\}\s*;", text, re.S) for n in re.findall(r"\b(WGS_[A-Z0-9_]+)\s*=", block)]
    found += [n for n in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(WGS_[A-Z0-9_]+)[ \t]+\S", text, re.M) if n != "WGS_DIM"]
    raw_count = len(re.findall(r"\bWGS_[A-Z0-9_]+ =(?!=)", text)) + len(re.findall(r"^#define WGS_(?!DIM\b)\w+[ \t]+\S", text, re.M))
    assert len(found) == raw_count, f"{raw_count} constants in the text, {len(found)} parsed"
    constants = list(dict.fromkeys(found))                                               # (WGS_ANG_DIM has one #define per dimension)
    decls = re.findall(rf"^({_RET})(wgs_[a-z_]+)\(([^)]*)\)\s*;", text, re.M)
    functions = {name: (ret.strip(), params) for ret, name, params in decls}
    assert len(functions) == len(decls), "a function is declared twice"
    # a declaration the pattern above cannot read to its closing parenthesis would be missing here
    starts = set(re.findall(rf"^{_RET}(wgs_[a-z_]+)\(", text, re.M))
    assert starts == set(functions), sorted(starts ^ set(functions))
    return Header(structs, constants, functions)


@functools.lru_cache(maxsize=None)
def layout(dim):
    """sizeof of every struct, offsetof and sizeof of every field and the value of every constant of header(), as gcc sees them with
    -DWGS_DIM=dim: one program per dimension and process. A name the parser invented does not compile."""
    h = header()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "wgsparkl_hip.h"', "int main(void) {"]
    for s, fs in h.structs.items():
        lines.append(f'  printf("S {s} - %zu 0\\n", sizeof({s}));')
        lines += [f'  printf("F {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s} *)0)->{f}));' for f in fs]
    lines += [f'  printf("C {c} - %lld 0\\n", (long long)({c}));' for c in h.constants]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "abi.c"), os.path.join(tmp, "abi")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-DWGS_DIM={dim}", f"-I{INCLUDE}", src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lay = Layout({}, {s: {} for s in h.structs}, {})
    for kind, name, field, a, b in (l.split() for l in out.splitlines()):
        if kind == "S":
            lay.size[name] = int(a)
        elif kind == "F":
            lay.fields[name][field] = (int(a), int(b))
        else:
            lay.const[name] = int(a)
    return lay


# ------------------------------------------------------------------------------------------------ the Rust file
_RS_SCALARS = {"f32": 4, "u32": 4, "i32": 4, "u8": 1, "u64": 8, "i64": 8, "f64": 8, "usize": 8}


def _rs_value(expr, env):
    expr = re.sub(r"\s+as\s+\w+", "", expr.strip())
    assert re.fullmatch(r"[\w\s+*/()|-]+", expr), f"not a constant expression this model evaluates: {expr!r}"
    return int(eval(expr, {"__builtins__": {}}, dict(env)))


def _rs_structs(text):
    """{struct: [(field, type)]} of the #[repr(C)] pub structs, comments stripped."""
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, body in re.findall(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct (\w+)\s*\{([^{}]*)\}", text):
        out[name] = re.findall(r"pub\s+(\w+)\s*:\s*([^,]+?)\s*(?:,|$)", body)
    return out


def rust_layout(text, dim):
    """The Layout of lib.rs under the repr(C) rules: a scalar is aligned to its size, a raw pointer is 8 bytes, an array takes its
    element's alignment (its length an expression in DIM and the file's constants), a nested struct is looked up by name, a struct is
    aligned to its largest member and padded to a multiple of that. A trailing underscore of a field name (`type_`) is dropped."""
    env = {"DIM": dim}
    for name, expr in re.findall(r"^pub const (\w+)\s*:\s*\w+\s*=\s*([^;]+);", re.sub(r"//[^\n]*", "", text), re.M):
        if name != "DIM":
            env[name] = _rs_value(expr, env)
    structs = _rs_structs(text)
    lay = Layout({}, {}, {k: v for k, v in env.items() if k != "DIM"})
    aligns = {}

    def of(t):                                                   # (size, alignment) of a type
        t = t.strip()
        if t.startswith("*"):
            return 8, 8
        if t.startswith("["):
            elem, count = t[1:-1].rsplit(";", 1)
            size, align = of(elem)
            return size * _rs_value(count, env), align
        if t in _RS_SCALARS:
            return _RS_SCALARS[t], _RS_SCALARS[t]
        struct(t)
        return lay.size[t], aligns[t]

    def struct(name):
        if name in lay.size:
            return
        assert name in structs, f"{name}: neither a scalar nor a #[repr(C)] struct of the file"
        at, biggest, fields = 0, 1, {}
        for field, t in structs[name]:
            size, align = of(t)
            at = -(-at // align) * align
            fields[field[:-1] if field.endswith("_") else field] = (at, size)
            at, biggest = at + size, max(biggest, align)
        lay.size[name], lay.fields[name], aligns[name] = -(-at // biggest) * biggest, fields, biggest

    for name in structs:
        struct(name)
    return lay


def rust_functions(text):
    """{name: (return kind, [parameter kinds])} of the extern "C" block."""
    block = re.search(r'extern "C" \{(.*?)\n\}', re.sub(r"//[^\n]*", "", text), re.S).group(1)
    out = {}
    for name, params, ret in re.findall(r"pub fn (\w+)\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", block, re.S):
        assert name not in out, f"{name} is declared twice"
        out[name] = (_rs_kind(ret) if ret else "void", [_rs_kind(p.split(":", 1)[1]) for p in params.split(",") if p.strip()])
    return out


def _rs_kind(t):
    t = t.strip()
    if t.startswith("*"):
        return "ptr"
    return {"f32": "f32", "i32": "i32", "u32": "u32", "u64": "u64", "usize": "size", "wgs_status": "i32"}[t]


# ------------------------------------------------------------------------------------------------ parameter kinds
_C_KINDS = {"float": "f32", "int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "size_t": "size", "wgs_status": "i32"}


def param_kinds(decl):
    """A C parameter list as kinds: ptr, f32, i32, u32, u64, size. `(void)` is []; an array parameter is a pointer."""
    decl = re.sub(r"/\*.*?\*/", " ", decl, flags=re.S).strip()
    if decl == "void":
        return []
    assert decl, "an empty parameter list is not a C prototype"
    return ["ptr" if "*" in p or "[" in p else _C_KINDS[re.sub(r"\bconst\b", "", p).split()[0]] for p in decl.split(",")]


def return_kind(ret):
    return {"const char *": "ptr", "void": "void"}.get(ret) or _C_KINDS[ret]


def ctypes_kind(t):
    """The kind of a ctypes argtype / restype. c_size_t and c_uint64 are ONE class on an LP64 host, so a ctypes prototype cannot tell
    `size` from `u64`: both read `size` here and the comparison with the header reads them alike."""
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    return {C.c_float: "f32", C.c_int32: "i32", C.c_uint32: "u32", C.c_size_t: "size", C.c_uint64: "size"}[t]
