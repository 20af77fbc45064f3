"""bridgeqa_amd/_cabi.py derives the ctypes bindings, descriptor structs and constants of libbqhip.so from include/*.h.
The parser is held to truths it did not produce: a count of the headers' BQ_API declarations, struct layouts printed by the
host C compiler, and signatures / values written out by hand.  No GPU, no compute."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys
import types

import pytest

from conftest import ROOT
from bridgeqa_amd import _cabi

_vp, _i, _l, _f, _u = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_uint


def _declared():
    """names after every BQ_API token that starts a declaration (not the `#define BQ_API` lines), comments removed"""
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("bqhip.h", "bqhip_fusion.h"))
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    starts = re.findall(r"^[ \t]*BQ_API\b", hdr, flags=re.M)
    names = re.findall(r"^[ \t]*BQ_API\s[^;(]*?(bq_\w+)\s*\(", hdr, flags=re.M)
    assert len(names) == len(starts)
    return names


def test_every_declaration_is_parsed_and_bound():
    names = _declared()
    assert len(names) == len(set(names)) == len(_cabi.PROTOS) == 97
    assert set(names) == set(_cabi.PROTOS)
    # bind() sets both attributes on every name, also where the value equals ctypes' default
    fake = types.SimpleNamespace(**{n: types.SimpleNamespace() for n in names})
    _cabi.bind(fake)
    for n in names:
        assert set(vars(getattr(fake, n))) == {"argtypes", "restype"}, n
    from bridgeqa_amd import _ext
    for n in names:
        fn = getattr(_ext._lib, n)
        assert fn.argtypes is not None and list(fn.argtypes) == _cabi.PROTOS[n][1], n
        assert fn.restype is _cabi.PROTOS[n][0], n
    assert list(_ext._lib.bq_abi_version.argtypes) == [] and _cabi.PROTOS["bq_gemm_max_problems"] == (_i, [])


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof / offsetof as the host C compiler lays the headers' structs out, against the generated Structures"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bqhip_fusion.h"', 'int main(void) {']
    want = {}
    for name, cls in _cabi.STRUCTS.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want[name] = ctypes.sizeof(cls)
        for field in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field[0], name, field[0]))
            want["%s.%s" % (name, field[0])] = getattr(cls, field[0]).offset
    lines += ['  return 0;', '}']
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([exe]).decode().splitlines())}
    assert got == want
    # field counts read off the headers by hand: a member the parser dropped would not be printed above either
    assert {n: len(c._fields_) for n, c in _cabi.STRUCTS.items()} == {
        "bq_attn_side": 24, "bq_gemm_desc": 22, "bq_colsum_desc": 5, "bq_det_loss_desc": 55, "bq_det_loss_seg": 6,
        "bq_mlp_eval_layer": 10, "bq_mlp_eval_desc": 23}
    layers = dict((f[0], f[1]) for f in _cabi.STRUCTS["bq_mlp_eval_desc"]._fields_)["layers"]
    assert layers._type_ is _cabi.STRUCTS["bq_mlp_eval_layer"] and layers._length_ == 3


def test_hand_written_pins():
    P, S, D = _cabi.PROTOS, _cabi.STRUCTS, _cabi.DEFINES
    assert P["bq_attn_fwd"] == (_i, [_vp] * 6 + [_i] * 5 + [_l] * 9 + [_f] * 2 + [_u, _vp, _i, _vp])
    assert P["bq_drop_add_ln_fwd"] == (_i, [_vp] * 9 + [_i, _i, _f, _f, _f, _i, _u] + [_vp] * 2)
    assert P["bq_gemm_bf16"][1][0] is ctypes.POINTER(S["bq_gemm_desc"]) and P["bq_gemm_bf16"][1][1:] == [_i] * 4 + [_vp]
    assert P["bq_fps_workspace_bytes"] == (ctypes.c_size_t, [_i, _i])
    assert P["bq_drop_add_ln_bwd_det_slab_floats"] == (_l, [_i, _i, _i])
    assert P["bq_last_error"] == (ctypes.c_char_p, [])
    assert P["bq_ap_match"][1][5] is _vp        # const double *thresholds: a plain pointer like every other
    assert P["bq_nms"] == (_i, [_vp] * 5 + [_i, _i, _f, _i, _i, _vp])
    assert P["bq_nms_f64"] == (_i, [_vp] * 5 + [_i, _i, ctypes.c_double, _i, _i, _vp])      # the threshold by value, a double
    assert D["BQ_GEMM_DET"] == 16 and D["BQ_EINVAL"] == -1 and D["BQHIP_ABI_VERSION"] == 6


def test_ext_takes_its_structs_and_constants_from_the_headers():
    from bridgeqa_amd import _ext
    for alias, name in (("_AttnSide", "bq_attn_side"), ("_GemmDesc", "bq_gemm_desc"), ("_ColsumDesc", "bq_colsum_desc"),
                        ("_DetLossDesc", "bq_det_loss_desc"), ("_DetLossSeg", "bq_det_loss_seg"),
                        ("_MlpEvalLayer", "bq_mlp_eval_layer"), ("_MlpEvalDesc", "bq_mlp_eval_desc")):
        assert getattr(_ext, alias) is _cabi.STRUCTS[name]
    assert (_ext.GEMM_P_XC, _ext.GEMM_Q_XC, _ext.GEMM_OUT_F32, _ext.GEMM_BACKGROUND, _ext.GEMM_DET) == (1, 2, 4, 8, 16)
    assert (_ext.EPI_NONE, _ext.EPI_BIAS, _ext.EPI_BIAS_GELU, _ext.EPI_DGELU, _ext.EPI_BIAS_CE, _ext.EPI_ADD) == (0, 1, 2, 3, 4, 5)
    assert (_ext.ABI_VERSION, _ext.RANK_LMAX, _ext.RANK_QBLOCK) == (6, 32, 4)


@pytest.mark.parametrize("text, named", [
    ("BQ_API int bq_bad_word(uint64_t n, void *stream);", "bq_bad_word"),                # unknown type word
    ("BQ_API int bq_by_value(long long n);", "bq_by_value"),                             # known only behind a pointer
    ("BQ_API int bq_callback(int (*cb)(int), void *stream);", "bq_callback"),            # function-pointer parameter
    ("typedef struct bq_bits { int a : 3; int b; } bq_bits;", "bq_bits"),                # bit-field
    ("BQ_API int bq_open(int n)\nBQ_API int bq_next(int n);", "bq_open"),                # no terminating ';'
    ("BQ_API int bq_ok(int n);\nBQ_API int bq_open_at_end(int n)\n", "bq_open_at_end"),
    ("BQ_API int bq_unnamed(int, void *stream);", "bq_unnamed"),
    ("#define BQ_SHIFTED (1 << 4)\n", "BQ_SHIFTED"),                                     # not an integer literal
    ("int bq_no_api(int n);", "bq_no_api"),                                              # nothing is skipped silently
])
def test_parser_refuses_what_it_does_not_understand(text, named):
    with pytest.raises(ValueError, match=named):
        _cabi.parse(text)


def test_parser_reads_the_forms_the_headers_use():
    protos, structs, defines = _cabi.parse(
        "#ifndef BQ_T_H\n#define BQ_T_H\n#define BQ_NEG (-3) /* a\n comment */\n#define BQ_API\n"
        "typedef struct bq_in { const float *a, *b; int n; } bq_in;\n"
        "typedef struct bq_out { long r; bq_in two[2]; } bq_out; // tail\n"
        "BQ_API const char *bq_name(void);\nBQ_API size_t bq_f(const bq_out *d, const unsigned char *m,\n  double x, void *stream);\n"
        "#endif\n")
    assert defines == {"BQ_NEG": -3} and list(structs) == ["bq_in", "bq_out"]
    assert [(f[0], f[1]) for f in structs["bq_in"]._fields_] == [("a", _vp), ("b", _vp), ("n", _i)]
    assert protos == {"bq_name": (ctypes.c_char_p, []),
                      "bq_f": (ctypes.c_size_t, [ctypes.POINTER(structs["bq_out"]), _vp, ctypes.c_double, _vp])}


def test_missing_header_and_stale_library_are_named(tmp_path, monkeypatch):
    monkeypatch.setattr(_cabi, "INCLUDE_DIR", str(tmp_path))
    with pytest.raises(ValueError, match="bqhip.h"):
        _cabi._read_headers()
    from bridgeqa_amd import _ext
    monkeypatch.setitem(_cabi.PROTOS, "bq_declared_not_exported", (_i, [_vp]))
    with pytest.raises(ImportError, match=r"bq_declared_not_exported.*stale library: python -m bridgeqa_amd.build --force"):
        _cabi.bind(ctypes.CDLL(_ext.library_path()))


# ---- the other half: every definition is compiled against its declaration -------------------------------------------------
# The rule: an entry point is defined as `extern "C" <ret> bq_name(...)`, no visibility attribute, in a source
# that includes the header declaring it.  Then a definition that disagrees with the header does not compile.
CSRC = os.path.join(ROOT, "bridgeqa_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HAVE_HIPCC = os.path.exists(HIPCC)
ALL_HEADERS = _cabi.HEADERS + _cabi.ADDITIVE_HEADERS
UNDECLARED = {"bq_debug_clock_mhz"}       # exported for tools/clock.py, in no header: the one exception


def _all_declared():
    return set(_cabi.PROTOS) | set(_cabi.ADDITIVE_PROTOS)


def _definitions():
    """{bq_ name: [(source file, everything on its line in front of the name)]} of every function DEFINITION in csrc/*.hip"""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"^([^\n;{}]*?)\b(bq_\w+)\s*\(([^(){};]*)\)\s*\{", text, flags=re.M):
            found.setdefault(m.group(2), []).append((os.path.basename(path), m.group(1)))
    return found


def test_exported_symbols_are_the_declared_ones():
    from bridgeqa_amd import _ext
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ext.library_path()]).decode()
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[2].startswith("bq_")}
    assert len(_all_declared()) == 103
    assert exported == _all_declared() | UNDECLARED


def test_every_definition_is_extern_c_without_an_attribute():
    defs = _definitions()
    for name in sorted(_all_declared()):
        assert len(defs.get(name, ())) == 1, (name, defs.get(name))
        src, head = defs[name][0]
        assert re.fullmatch(r'extern "C" (?:const )?\w+(?: \w+)* ?\**', head), (name, src, head)
        assert "attribute" not in head and "visibility" not in head and "BQ_API" not in head, (name, src, head)
    # the exception carries its visibility itself, and nothing else does
    assert [h for s, h in defs["bq_debug_clock_mhz"]] == ['extern "C" __attribute__((visibility("default"))) int ']
    others = "".join(re.sub(r"[^\n]*bq_debug_clock_mhz[^\n]*", "", open(p).read()) for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert 'visibility("default")' not in others


def _declaring_header(name):
    hits = [h for h in ALL_HEADERS
            if re.search(r"\bBQ_API\s[^;(]*?\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S))]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def _first_mention(preprocessed, names):
    """{name: basename of the file whose text holds the first `name(` of a host-only preprocessed source}, by its line markers"""
    first, cur = {}, None
    want = re.compile(r"\b(%s)\s*\(" % "|".join(sorted(names)))
    for line in preprocessed.splitlines():
        m = re.match(r'# \d+ "([^"]*)"', line)
        if m:
            cur = os.path.basename(m.group(1))
            continue
        for n in want.findall(line):
            first.setdefault(n, cur)
    return first


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_every_definition_sees_its_declaration():
    """the host-only preprocessed text of the defining source meets the name in the declaring header first, before the definition"""
    from bridgeqa_amd import build
    by_src = {}
    for name, sites in _definitions().items():
        if name in _all_declared():
            by_src.setdefault(sites[0][0], set()).add(name)
    assert sum(len(v) for v in by_src.values()) == 103
    incl = [a for i, a in enumerate(build.FLAGS) if a == "-I" or (i and build.FLAGS[i - 1] == "-I")]
    procs = {src: subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-host-only", "-E"] + incl +
                                   [os.path.join(CSRC, src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
             for src in by_src}
    for src, p in procs.items():
        out, err = p.communicate()
        assert p.returncode == 0, (src, err.decode()[-2000:])
        first = _first_mention(out.decode(), by_src[src])
        for name in sorted(by_src[src]):
            assert first.get(name) == _declaring_header(name), (name, src, first.get(name))


def test_first_mention_tells_a_source_without_its_header():
    """the check above fails for a source that stops including the header: its first mention is then the definition itself"""
    with_hdr = '# 1 "x/bn.hip"\n# 1 "inc/bqhip_fusion.h" 1\nint bq_bn_chunks(long R);\n# 3 "x/bn.hip" 2\nextern "C" int bq_bn_chunks(long R) {\n'
    without = '# 1 "x/bn.hip"\nextern "C" int bq_bn_chunks(long R) {\n'
    assert _first_mention(with_hdr, {"bq_bn_chunks"}) == {"bq_bn_chunks": "bqhip_fusion.h"}
    assert _first_mention(without, {"bq_bn_chunks"}) == {"bq_bn_chunks": "bn.hip"}
    assert _declaring_header("bq_bn_chunks") == "bqhip_fusion.h" and _declaring_header("bq_view_prep") == "bqhip_view.h"


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
@pytest.mark.parametrize("first_param, conflict", [("int R", True), ("long R", False)])
def test_a_definition_that_disagrees_with_its_header_does_not_compile(tmp_path, first_param, conflict):
    """the mechanism itself: the header says `long R`"""
    src = str(tmp_path / "entry.hip")
    open(src, "w").write('#include "bqhip_fusion.h"\nextern "C" int bq_bn_chunks(%s, int S, int pool) { return 0; }\n' % first_param)
    r = subprocess.run([HIPCC, "--cuda-host-only", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    if conflict:
        assert r.returncode != 0 and "conflicting types" in r.stderr, r.stderr
    else:
        assert r.returncode == 0, r.stderr


def test_cabi_needs_neither_torch_nor_the_library():
    code = ("import importlib.util, sys\n"
            "spec = importlib.util.spec_from_file_location('_cabi', %r)\n"
            "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)\n"
            "assert len(m.PROTOS) > 90 and 'torch' not in sys.modules\n" % os.path.join(ROOT, "bridgeqa_amd", "_cabi.py"))
    subprocess.check_call([sys.executable, "-c", code])
