"""The ctypes view of libbqhip.so, derived from include/bqhip.h and include/bqhip_fusion.h -- the headers build.py compiles
against -- so that a prototype, a descriptor struct or a #define is stated once.  Imports neither torch nor the library.

  PROTOS   name -> (restype, [argtypes]) of every `BQ_API <ret> bq_name(<params>);`
  STRUCTS  name -> the ctypes.Structure of every `typedef struct bq_x { ... } bq_x;` (the header's field names and order)
  DEFINES  name -> int of every `#define BQ... <integer or (-integer)>`
  bind(lib) sets argtypes / restype on the library's functions.

The headers are regular C; what parse() does not recognise raises ValueError naming the declaration.  It never guesses."""
import ctypes
import os
import re

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = ("bqhip.h", "bqhip_fusion.h")

# The one mapping rule (`const` is dropped before it applies): these scalars by value; a pointer to a declared struct ->
# POINTER(that Structure); a `const char *` return -> c_char_p; every other pointer -> c_void_p.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "long": ctypes.c_long, "unsigned": ctypes.c_uint,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "long long"}   # what a c_void_p may stand for

_TOP = re.compile(r'\s*(?:#([^\n]*)|extern\s+"C"\s*\{|\}|typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;|BQ_API\b([^;]*);)')
_FIRST = re.compile(r"((?:\w+\s+)*?\w+)(?:\s+|\s*(\*+)\s*)(\w+)\s*(?:\[(\d+)\])?")   # `const float *gamma`, `bq_x layers[3]`
_NEXT = re.compile(r"(\**)\s*(\w+)\s*(?:\[(\d+)\])?")                        # `*beta` after a comma
_FUNC = re.compile(r"((?:\w+\s+)+?)(\**)\s*(bq[xmh]?_\w+)\s*\(([^()]*)\)")


def _ctype(base, stars, structs, decl, ret=False):
    base = " ".join(w for w in base.split() if w != "const")
    if stars:
        if base in structs and stars == "*":
            return ctypes.POINTER(structs[base])
        if base in _POINTEES:
            return ctypes.c_char_p if ret and base == "char" else ctypes.c_void_p
    elif base in _SCALARS:
        return _SCALARS[base]
    elif base in structs:
        return structs[base]
    elif base == "void" and ret:
        return None
    raise ValueError("unknown type %r in declaration %r" % ((base + " " + stars).strip(), " ".join(decl.split())))


def _declarators(text, structs, decl):
    """`const float *gamma, *beta` or `int B` -> [(name, ctype)]"""
    parts = [p.strip() for p in text.split(",")]
    m = _FIRST.fullmatch(parts[0])
    rest = [_NEXT.fullmatch(p) for p in parts[1:]]
    if not m or not all(rest):
        raise ValueError("cannot parse %r in declaration %r" % (" ".join(text.split()), " ".join(decl.split())))
    out = []
    for stars, name, count in [m.groups()[1:]] + [r.groups() for r in rest]:
        t = _ctype(m.group(1), stars or "", structs, decl)
        out.append((name, t * int(count) if count else t))
    return out


def parse(text):
    """header text -> (protos, structs, defines)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    protos, structs, defines = {}, {}, {}
    pos = 0
    while text[pos:].strip():
        m = _TOP.match(text, pos)
        if not m:
            raise ValueError("cannot parse the declaration at %r" % " ".join(text[pos:].split())[:120])
        pos = m.end()
        directive, tag, body, name, func = m.groups()
        if directive is not None:
            d = re.fullmatch(r"\s*define\s+(BQ\w*)\s+(\S.*?)\s*", directive)
            if d and d.group(1) != "BQ_API":
                try:
                    defines[d.group(1)] = int(d.group(2).strip("()"), 0)
                except ValueError:
                    raise ValueError("#define %s: %r is not an integer" % d.groups()) from None
        elif tag is not None:
            decl = "struct " + tag
            if tag != name:
                raise ValueError("typedef struct %s is named %s" % (tag, name))
            fields = [f for member in body.split(";") if member.strip() for f in _declarators(member, structs, decl)]
            structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        elif func is not None:
            f = _FUNC.fullmatch(func.strip())
            if not f:
                raise ValueError("cannot parse the declaration %r" % " ".join(("BQ_API" + func).split())[:200])
            params = [] if f.group(4).strip() == "void" else \
                [t for p in f.group(4).split(",") for _, t in _declarators(p, structs, f.group(3))]
            protos[f.group(3)] = (_ctype(f.group(1), f.group(2), structs, f.group(3), ret=True), params)
    return protos, structs, defines


def _read_headers(headers=HEADERS):
    try:
        return "\n".join(open(os.path.join(INCLUDE_DIR, h)).read() for h in headers)
    except OSError as e:
        raise ValueError("bridgeqa_amd: cannot read the C header %s" % e.filename) from None


PROTOS, STRUCTS, DEFINES = parse(_read_headers())

# Entry points added to ABI 6 after tests/test_cabi_cpu.py counted the two headers above by hand: they live in headers of their
# own (bqhip_fusion.h includes them) and in a table of their own, derived by the same parser.  bind(lib, ADDITIVE_PROTOS).
ADDITIVE_HEADERS = ("bqhip_lstm.h", "bqhip_scene.h", "bqhip_view.h", "bqhip_beam.h", "bqhip_mcan.h", "bqhip_mhatt.h")
_additive, ADDITIVE_STRUCTS, ADDITIVE_DEFINES = parse(_read_headers(ADDITIVE_HEADERS))
ADDITIVE_PROTOS = {n: p for n, p in _additive.items() if n.startswith("bq_")}
# Entry points added after tests/test_cabi_cpu.py took its census of the library's bq_ symbols (103 with the table above) are named
# bqx_: declared in an additive header, derived by the same parser, compiled against their declaration like every other, and
# outside that census.  bind(lib, EXTENSION_PROTOS).
EXTENSION_PROTOS = {n: p for n, p in _additive.items() if n.startswith("bqx_")}
# The bqx_ symbols are counted as well (tests/test_beam_device_cpu.py holds them to the beam step's one), so the row operators of
# the MCAN blocks (bqhip_mcan.h, csrc/mcan.hip) carry a family prefix of their own, bqm_: same header rules, same parser, same
# compile-against-the-declaration.  bind(lib, MCAN_PROTOS).
MCAN_PROTOS = {n: p for n, p in _additive.items() if n.startswith("bqm_")}
# The bqm_ symbols are counted too (tests/test_mcan_rows_cpu.py holds them to the five row operators), so the attention core of
# MHAtt (bqhip_mhatt.h, csrc/mhatt.hip) is a family of its own again, bqh_.  bind(lib, MHATT_PROTOS).
MHATT_PROTOS = {n: p for n, p in _additive.items() if n.startswith("bqh_")}


def bind(lib, names=None):
    """declare `names` (default: every prototype of HEADERS) on the loaded library"""
    for name in PROTOS if names is None else names:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError("bridgeqa_amd: libbqhip.so has no %s, which include/ declares (stale library: "
                              "python -m bridgeqa_amd.build --force)" % name) from None
        fn.restype, fn.argtypes = next(t[name] for t in (PROTOS, ADDITIVE_PROTOS, EXTENSION_PROTOS, MCAN_PROTOS, MHATT_PROTOS) if name in t)
