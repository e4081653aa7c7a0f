"""What every header's host test asks of its ctypes binding, stated once: the header's prototypes against a {name: (restype, argtypes)}
table, and gcc's layout of the header's structs against their ctypes mirrors.  ctypes converts silently, so a wrong width or a missing
argument would corrupt a call on the GPU instead of failing it.  Each function returns the disagreements as strings ([] = none); what
is specific to a header (its lists of names, its constants, which module owns the table) stays written out in that header's test."""
import ctypes
import os
import re
import subprocess

INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
C_SCALARS = {"int": ctypes.c_int, "uint8_t": ctypes.c_uint8, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
             "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


def _code(header_path):
    """The header's text without its comments"""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S))


def prototypes(header_path):
    """{name: (return type, [argument types])} of every function that the header declares, as C type strings without the argument
    names and without `const` (`const TexGSFrame* frame` -> `TexGSFrame*`)."""
    ctype = lambda decl: re.sub(r"\s+", "", re.sub(r"\bconst\b", "", decl))
    protos = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(texgs_\w+)\s*\(([^)]*)\)\s*;", _code(header_path), flags=re.M):
        args = [a.strip() for a in args.split(",")]
        args = [] if args == ["void"] else [ctype(re.sub(r"\w+$", "", a)) for a in args]       # drop the argument's name
        protos[name] = (ctype(ret), args)
    return protos


def same_scalar(a, b):
    """Two ctypes scalar types of the same width and kind (signed / unsigned integer, float)"""
    kind = lambda t: "int" if t._type_ in "bhilq" else "uint" if t._type_ in "BHILQ" else t._type_
    simple = lambda t: isinstance(t, type) and issubclass(t, ctypes._SimpleCData) and t._type_ in "bhilqBHILQfd"
    return simple(a) and simple(b) and ctypes.sizeof(a) == ctypes.sizeof(b) and kind(a) == kind(b)


def signature_mismatches(header_path, signatures, mirrors):
    """Every disagreement between a {name: (restype, argtypes)} table and the header's prototypes: the names (both ways), the return
    type, the argument count, and per argument a scalar of the same width and kind, exactly POINTER(mirror) for a pointer to a TexGS*
    struct (`mirrors`: {C struct name: ctypes.Structure}), c_void_p for any other pointer (or, for a pointer to a scalar, the ctypes
    pointer to that scalar)."""
    protos, bad = prototypes(header_path), []
    if sorted(signatures) != sorted(protos):
        bad.append(f"names differ: {sorted(set(signatures) ^ set(protos))}")
    for name, (restype, argtypes) in signatures.items():
        if name not in protos:
            continue
        ret, args = protos[name]
        if not (restype is ctypes.c_char_p if ret == "char*" else ret in C_SCALARS and same_scalar(restype, C_SCALARS[ret])):
            bad.append(f"{name}: returns {ret}, the table says {restype}")
        if len(argtypes) != len(args):
            bad.append(f"{name}: {len(args)} arguments, the table has {len(argtypes)}")
            continue
        for k, (c, t) in enumerate(zip(args, argtypes)):
            if c in C_SCALARS:
                ok = same_scalar(t, C_SCALARS[c])
            elif c.startswith("TexGS"):
                ok = c.endswith("*") and c[:-1] in mirrors and t is ctypes.POINTER(mirrors[c[:-1]])
            else:           # void* is c_void_p; a pointer to a scalar may also be stated as the ctypes pointer to that scalar
                typed = isinstance(t, type) and issubclass(t, ctypes._Pointer) and c[:-1] in C_SCALARS and same_scalar(t._type_, C_SCALARS[c[:-1]])
                ok = c.endswith("*") and (t is ctypes.c_void_p or typed)
            if not ok:
                bad.append(f"{name}: argument {k} is {c}, the table says {t}")
    return bad


def struct_fields(header_path, cname):
    """The field names of `typedef struct [cname] { ... } cname;` in the header's order (`float a, b;` declares two; `T row[N];` one)"""
    body = re.search(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*%s\s*;" % cname, _code(header_path))
    if body is None:
        return None
    decls = [re.sub(r"\[[^\]]*\]", "", d) for d in body.group(1).split(";") if d.strip()]
    return [re.findall(r"\w+", part)[-1] for d in decls for part in d.split(",")]


def layout_mismatches(header_name, mirrors, consts, tmp_path):
    """Every disagreement between the header as gcc (strict C99) lays it out and the host's statement of it: sizeof of each struct of
    `mirrors` ({C struct name: ctypes.Structure}), offsetof of each field, the field names in the header's order, and each constant of
    `consts` ({macro, enumerator or constant expression: the host's value}) as an int."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header_name}"', "int main(void) {"]
    for cname, cls in mirrors.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'printf("{k} %d\\n", (int)({k}));' for k in consts] + ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (l.rsplit(None, 1) for l in subprocess.check_output([str(exe)]).decode().splitlines() if l.strip())}
    bad = []
    for cname, cls in mirrors.items():
        names = [f for f, _ in cls._fields_]
        want = {cname: ctypes.sizeof(cls), **{f"{cname}.{f}": getattr(cls, f).offset for f in names}}
        bad += [f"{k}: the header has {got[k]}, the mirror {v}" for k, v in want.items() if got[k] != v]
        if struct_fields(os.path.join(INC, header_name), cname) != names:
            bad.append(f"{cname}: the header's fields are {struct_fields(os.path.join(INC, header_name), cname)}, the mirror's {names}")
    bad += [f"{k}: the header has {got[k]}, the host {v}" for k, v in consts.items() if got[k] != v]
    return bad


def build_script():
    """texture-gs_amd/build.py as a module, imported the way texgs/_lib.py tree_build_id() imports it"""
    import importlib.util
    path = os.path.join(os.path.dirname(INC), "texture-gs_amd", "build.py")
    spec = importlib.util.spec_from_file_location("texgs_build_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_knows_header(header_path):
    """The build script with `header_path` checked against what the build uses: the header is in the one list HEADERS, the rebuild rule
    (build) and build_id() both read that list, and build_id() depends on the header being in it."""
    build = build_script()
    header_path = os.path.abspath(header_path)
    assert header_path in build.HEADERS and build.HEADERS == sorted(set(build.HEADERS)), header_path
    assert "HEADERS" in build.build.__code__.co_names and "HEADERS" in build.build_id.__code__.co_names
    with_it = build.build_id()
    build.HEADERS = [h for h in build.HEADERS if h != header_path]
    assert build.build_id() != with_it, "build_id() does not read " + header_path
    return build_script()
