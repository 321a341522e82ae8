"""The Python statement of the C ABI (host/abi.py) against include/*.h: every prototype, every struct mirror and every
enum mirror, from the headers themselves.  No device; the struct and enum tests compile one small C probe."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADERS = ("kernelHandler.h", "ViT_opencl.h", "Network.h")

# C scalar types of the headers -> the ctypes type a table entry must hold for them
SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long": C.c_long, "size_t": C.c_size_t,
           "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double}
HANDLES = {"vh_stream_t", "vh_event_t"}     # typedef void *
# Struct types that a prototype takes by pointer and the table may declare as c_void_p, each with its reason.
NOT_MIRRORED = {
    "vit_hip_ctx": "opaque handle: declared, never defined, in ViT_opencl.h",
    "vit_hip_multi": "opaque handle: declared, never defined, in ViT_opencl.h",
    "vh_resize_desc": "vh_launch_resize_crop_u8 documents desc as n descriptors in device memory; the library's ingest "
                      "planner fills them and nothing on the Python side builds or reads one",
}


def _strip(text: str) -> str:
    """A header without comments, preprocessor lines (the VH_CHECK macro with its continued lines among them) and the
    extern "C" opening."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"\\\n", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    return text.replace('extern "C" {', " ")


def _header(name: str) -> str:
    return (ROOT / "include" / name).read_text()


def _split_top(s: str, sep: str) -> list:
    """s split at every sep outside parentheses, brackets and braces"""
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == sep and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return out + [cur]


def _param(text: str):
    """One parameter or return type -> (class, base type): class is "pointer", "void" or a key of SCALARS."""
    text = " ".join(text.split())
    if "(*" in text:
        return "pointer", "function"
    if text.count("*") > 1:                 # `float **rows`, `vit_hip_ctx **out`: a pointer to pointers
        return "pointer", "void"
    words = [w for w in re.sub(r"[*\[].*", "", text).split() if w != "const"]
    if "*" in text or "[" in text:
        # `float *x`, `const float box[4]`: the name follows the star or precedes the bracket
        base = words if "*" in text.split("[")[0] else words[:-1]
        return "pointer", " ".join(base)
    return None, words


def _classify(text: str, named: bool):
    kind, base = _param(text)
    if kind:
        return kind, base
    ty = " ".join(base[:-1] if named and len(base) > 1 else base)
    if ty == "void":
        return "void", ty
    if ty in HANDLES:
        return "pointer", "void"
    assert ty in SCALARS, f"a type the classes do not cover: {text!r}"
    return ty, ty


def parse_prototypes(name: str) -> list:
    """[(function, (return class, base), [(parameter class, base), ...])] of one header, in its order.  Every statement
    of the header is accounted for: a typedef, an enum, a prototype -- anything else fails."""
    text = _strip(_header(name))
    out = []
    for stmt in _split_top(text, ";"):
        stmt = " ".join(stmt.split())
        if not stmt or stmt == "}":         # the end of the file: extern "C"'s closing brace
            continue
        if stmt.startswith(("typedef ", "enum ", "enum{")):
            continue
        m = re.match(r"^(?P<ret>[\w\s\*]+?)\b(?P<fn>\w+)\s*\((?P<args>.*)\)$", stmt)
        assert m, f"{name}: neither a typedef, an enum nor a prototype: {stmt!r}"
        args = [a.strip() for a in _split_top(m["args"], ",")]
        params = [] if args in (["void"], [""]) else [_classify(a, named=True) for a in args]
        out.append((m["fn"], _classify(m["ret"], named=False), params))
    return out


def _is_pointer(t) -> bool:
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C._CFuncPtr)))


def _matches(abi, decl, t, where) -> str:
    """"" if the table's type t states the header's (class, base), else what is wrong"""
    kind, base = decl
    if kind == "void":
        return "" if t is None else f"{where}: void in the header, {t} in the table"
    if kind != "pointer":
        return "" if t is SCALARS[kind] else f"{where}: {kind} in the header, {getattr(t, '__name__', t)} in the table"
    if not _is_pointer(t):
        return f"{where}: a pointer in the header, {getattr(t, '__name__', t)} in the table"
    if base in abi.STRUCTS:
        mirror = abi.STRUCTS[base]
        return "" if t is C.POINTER(mirror) else \
            f"{where}: {base} * in the header wants POINTER({mirror.__name__}), the table has {t.__name__}"
    if base in SCALARS or base in NOT_MIRRORED or base in ("void", "char", "unsigned char", "function") or base in HANDLES:
        return ""
    return f"{where}: {base} * is neither a mirrored struct nor a listed exception"


def test_prototypes_agree_with_the_headers(pkg):
    """Test 1: every function the three headers declare has a table entry of the same arity, with the same type class
    per parameter and for the return, and struct pointers are declared as POINTER(their mirror)."""
    abi = pkg.host.abi
    assert tuple(abi.PROTOTYPES) == HEADERS
    declared, wrong = set(), []
    for header in HEADERS:
        parsed = parse_prototypes(header)
        table = {fn: (ret, args) for fn, ret, args in abi.PROTOTYPES[header]}
        assert len(table) == len(abi.PROTOTYPES[header]), f"{header}: a name twice in the table"
        for fn, ret, params in parsed:
            declared.add(fn)
            if fn not in table:
                wrong.append(f"{fn}: declared in {header}, not in its part of the table")
                continue
            t_ret, t_args = table[fn]
            if len(t_args) != len(params):
                wrong.append(f"{fn}: {len(params)} parameters in {header}, {len(t_args)} in the table")
                continue
            wrong += [w for w in [_matches(abi, ret, t_ret, f"{fn} return")] +
                      [_matches(abi, p, t, f"{fn} parameter {k}") for k, (p, t) in enumerate(zip(params, t_args))] if w]
        in_header = {p[0] for p in parsed}
        wrong += [f"{fn}: in the table under {header}, which does not declare it" for fn in table if fn not in in_header]
        # the headers' own order, so that a header and the table read side by side
        assert [fn for fn, _, _ in abi.PROTOTYPES[header] if fn in declared] == [p[0] for p in parsed if p[0] in table], header
    assert not wrong, "\n".join(wrong)
    # nothing skipped quietly: the names parsed are the names test_headers_declare_exactly_the_exports finds
    by_regex = set()
    for h in (ROOT / "include").glob("*.h"):
        text = re.sub(r"/\*.*?\*/", "", h.read_text(), flags=re.S)
        text = re.sub(r"#define VH_CHECK.*?while \(0\)", "", text, flags=re.S)
        by_regex |= set(re.findall(r"\b(vh_[a-z0-9_]+|vit_[a-z0-9_]+|ViT_opencl|load_image_data|load_weights)\s*\(", text))
    by_regex -= {"vh_check_err_"}
    assert declared == by_regex
    assert set(abi.EXPORTS) == declared and len(abi.EXPORTS) == len(declared)


def test_declare_covers_the_table(pkg):
    """Test 2: after declare() every table name of the built library carries its entry's argtypes and restype; a
    library that lacks a symbol is refused by that symbol's name."""
    abi = pkg.host.abi
    L = C.CDLL(str(pkg.binding.LIB_PATH))
    assert abi.declare(L) is L
    n = 0
    for header in HEADERS:
        for fn, ret, args in abi.PROTOTYPES[header]:
            f = getattr(L, fn)
            assert f.argtypes is not None and list(f.argtypes) == list(args), fn
            assert f.restype is ret, fn
            n += 1
    assert n == len(abi.EXPORTS)

    class Lacking:
        """every symbol but one"""
        def __getattr__(self, name):
            if name == "vh_launch_linear_p3_cols":
                raise AttributeError(name)
            f = type("F", (), {})()
            setattr(self, name, f)
            return f
    with pytest.raises(Exception, match="vh_launch_linear_p3_cols"):
        abi.declare(Lacking())


def _struct_bodies(name: str) -> dict:
    """{C type: [field names]} of every typedef struct with a body in one header"""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", _strip(_header(name)), flags=re.S):
        fields = []
        for decl in m[1].split(";"):
            if decl.strip():
                fields += [re.sub(r"\[.*", "", d).split()[-1].lstrip("*") for d in decl.split(",")]
        out[m[2]] = fields
    return out


def _constants(name: str) -> list:
    """every enumerator and every object-like #define of an integer in one header"""
    raw = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    out = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\d+[ \t]*$", raw, flags=re.M)
    for body in re.findall(r"\benum\s*\w*\s*\{(.*?)\}", _strip(raw), flags=re.S):
        out += [e.split("=")[0].strip() for e in body.split(",") if e.strip()]
    return out


@pytest.fixture(scope="module")
def probe(pkg, tmp_path_factory):
    """One C program generated from the registered pairs and the headers' constants: its output as
    {"sizeof T": n, "offsetof T.f": n, "value NAME": n}."""
    abi = pkg.host.abi
    lines = []
    for ctype, mirror in abi.STRUCTS.items():
        lines.append(f'    printf("sizeof {ctype} %zu\\n", sizeof({ctype}));')
        lines += [f'    printf("offsetof {ctype}.{f} %zu\\n", offsetof({ctype}, {f}));' for f, _ in mirror._fields_]
    for header in HEADERS:
        lines += [f'    printf("value {c} %lld\\n", (long long)({c}));' for c in _constants(header)]
    tmp = tmp_path_factory.mktemp("abi_probe")
    src = "#include <stdio.h>\n#include <stddef.h>\n" + "".join(f'#include "{h}"\n' for h in HEADERS) + \
        "int main(void)\n{\n" + "\n".join(lines) + "\n    return 0;\n}\n"
    (tmp / "probe.c").write_text(src)
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", str(tmp / "probe"), str(tmp / "probe.c")], check=True)
    out = subprocess.run([str(tmp / "probe")], check=True, capture_output=True, text=True).stdout
    return {line.rsplit(" ", 1)[0]: int(line.rsplit(" ", 1)[1]) for line in out.splitlines()}


def test_struct_mirrors_lay_out_as_the_headers_do(pkg, probe):
    """Test 3: sizeof and every field's offsetof of each registered C type, from the compiled headers, equal the
    mirror's; the field names are the header's; every struct the two public headers define is registered; the checker's
    own VitConfig and Network state the same fields."""
    abi = pkg.host.abi
    bodies = {}
    for header in HEADERS:
        bodies.update(_struct_bodies(header))
    for ctype, mirror in abi.STRUCTS.items():
        assert [f for f, _ in mirror._fields_] == bodies[ctype], f"{ctype}: field names"
        assert C.sizeof(mirror) == probe[f"sizeof {ctype}"], f"sizeof {ctype}"
        for f, _ in mirror._fields_:
            assert getattr(mirror, f).offset == probe[f"offsetof {ctype}.{f}"], f"offsetof {ctype}.{f}"
    public = set(_struct_bodies("ViT_opencl.h")) | set(_struct_bodies("Network.h"))
    assert len(public) >= 20 and public <= set(abi.STRUCTS), f"no mirror registered for {sorted(public - set(abi.STRUCTS))}"
    # kernelHandler.h's one struct is the exception NOT_MIRRORED gives the reason for
    assert set(bodies) - set(abi.STRUCTS) == {"vh_resize_desc"} and "vh_resize_desc" in NOT_MIRRORED
    from oracle import oracle
    assert oracle.VitConfig._fields_ == abi.VitConfig._fields_
    assert oracle.Network._fields_ == abi.Network._fields_


def test_enum_mirrors_hold_the_headers_constants(pkg, probe):
    """Test 4: under each registered prefix the dictionaries hold exactly the headers' constants, with their values."""
    abi = pkg.host.abi
    in_headers = [c for header in HEADERS for c in _constants(header)]
    assert len(in_headers) == len(set(in_headers))
    mirrored = {}
    for prefix, mapping, names in abi.ENUMS:
        for key, value in mapping.items():
            cname = (names or {}).get(key) or prefix + key.upper()
            assert cname.startswith(prefix), f"{cname} is not under {prefix}"
            assert cname in in_headers, f"{key!r} -> {cname}: no such constant in the headers"
            assert value == probe[f"value {cname}"], cname
            mirrored.setdefault(prefix, set()).add(cname)
    assert len(mirrored) >= 12
    for prefix, have in mirrored.items():
        want = {c for c in in_headers if c.startswith(prefix)}
        assert have == want, f"{prefix}: the headers also define {sorted(want - have)}"
