"""The ctypes binding is derived from include/micronet_hip.h: what the reader of micronet_amd._lib accepts, what it refuses, and that the
layouts and constants it derives are the compiler's.  Host only."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

from micronet_amd import _lib
from micronet_amd._lib import MicronetHipError, parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "micronet_hip.h")
P, I, L = C.c_void_p, C.c_int, C.c_int64

PROTOTYPE_CASES = [
    ("broken over lines", "int mn_a(const float* x, float* y,\n         int64_t n,\n         mn_stream_t stream);", {"mn_a": (I, [P, P, L, P])}),
    ("(void)", "int mn_version(void);", {"mn_version": (I, [])}),
    ("()", "int mn_version();", {"mn_version": (I, [])}),
    ("unnamed parameters", "int mn_b(const float*, int64_t, int, float, double, int32_t, mn_stream_t);",
     {"mn_b": (I, [P, L, I, C.c_float, C.c_double, C.c_int32, P])}),
    ("T* const*", "int mn_c(const float* const* w, float* const* qw, const int64_t* n, int32_t count);", {"mn_c": (I, [P, P, P, C.c_int32])}),
    ("struct pointers", "int mn_d(const mn_conv_geom* g, const mn_actq* aq, const mn_wq*, mn_prof_entry* out, const mn_adam_tensor* t, void* ws);",
     {"mn_d": (I, [C.POINTER(_lib.ConvGeom), C.POINTER(_lib.ActQ), C.POINTER(_lib.WQ), C.POINTER(_lib.ProfEntry), C.POINTER(_lib.AdamTensor), P])}),
    ("pointer to struct pointer", "int mn_e(const mn_adam_tensor* const* t);", {"mn_e": (I, [P])}),
    ("byte pointers", "int mn_f(const uint8_t* idx, int8_t* a, const double* stats, const int32_t* first);", {"mn_f": (I, [P, P, P, P])}),
    ("const char* return", "const char* mn_last_error(void);", {"mn_last_error": (C.c_char_p, [])}),
    ("void return", "void mn_profile_next(void* start_event, void* stop_event);", {"mn_profile_next": (None, [P, P])}),
    ("int64_t return", "int64_t mn_ws(int64_t rows, int64_t cols);", {"mn_ws": (L, [L, L])}),
    ("comments holding ; and (", "/* see f(x); g( */ int mn_g(int a); // h(y);\nint mn_h(int /* not; a( name */ b);", {"mn_g": (I, [I]), "mn_h": (I, [I])}),
    ("stream typedef", "typedef void* mn_stream_t;\nint mn_i(mn_stream_t stream);", {"mn_i": (I, [P])}),
    ("extern C and guards", '#ifndef H\n#define H\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\nint mn_j(void);\n#ifdef __cplusplus\n}\n#endif\n#endif',
     {"mn_j": (I, [])}),
]


@pytest.mark.parametrize("text,expected", [c[1:] for c in PROTOTYPE_CASES], ids=[c[0] for c in PROTOTYPE_CASES])
def test_reader_prototypes(text, expected):
    constants, structs, protos = parse_header("typedef void* mn_stream_t;\n" + text)
    assert constants == {} and structs == {}
    assert set(protos) == set(expected)
    for name, (res, args) in expected.items():
        assert protos[name][0] is res, name
        assert len(protos[name][1]) == len(args) and all(a is b for a, b in zip(protos[name][1], args)), (name, protos[name][1])


def test_reader_constants():
    text = "#define MN_OK 0\n#define MN_EINVAL (-22)\n#define MN_ALT 0x100 /* a flag; (hex) */\n  #  define MN_N 9 // rows\n#define OTHER_GUARD\n#define MN_MULTI 4 /* a comment\n that runs on */\n"
    assert parse_header(text) == ({"MN_OK": 0, "MN_EINVAL": -22, "MN_ALT": 256, "MN_N": 9, "MN_MULTI": 4}, {}, {})


def test_reader_struct_fields():
    text = """typedef struct mn_prof_entry {
        char name[96];     /* kernel; (name) */
        int32_t N, C, H, W;
        int64_t launches;
        double total_ms; float lr, weight_decay;
        const float* qp; void* codes;
        int flags;
    } mn_prof_entry;
    int mn_collect(mn_prof_entry* out, int cap);"""
    constants, structs, protos = parse_header(text)
    assert list(structs) == ["mn_prof_entry"]
    expected = [("name", C.c_char * 96), ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("launches", L), ("total_ms", C.c_double),
                ("lr", C.c_float), ("weight_decay", C.c_float), ("qp", P), ("codes", P), ("flags", I)]
    got = structs["mn_prof_entry"]
    assert [n for n, _ in got] == [n for n, _ in expected]
    assert all(a[1] is b[1] for a, b in zip(got, expected)), got
    assert protos["mn_collect"][1][0] is C.POINTER(_lib.ProfEntry)


REFUSALS = [
    ("size_t parameter", "int mn_a(const float* x, size_t n);", "mn_a"),
    ("unsigned parameter", "int mn_a(unsigned int n);", "mn_a"),
    ("struct by value", "int mn_a(mn_wq wq);", "mn_a"),
    ("array parameter", "int mn_a(float v[4]);", "mn_a"),
    ("function pointer parameter", "int mn_a(void (*cb)(int));", "mn_a"),
    ("pointer return", "float* mn_a(void);", "mn_a"),
    ("unknown return", "size_t mn_a(void);", "mn_a"),
    ("unknown field type", "typedef struct mn_wq { int32_t mode; uint16_t half; } mn_wq;", "mn_wq"),
    ("char field without extent", "typedef struct mn_wq { char c; } mn_wq;", "mn_wq"),
    ("array of scalars field", "typedef struct mn_wq { float v[4]; } mn_wq;", "mn_wq"),
    ("struct not in the map", "typedef struct mn_new { int32_t a; } mn_new;", "mn_new"),
    ("nested struct", "typedef struct mn_wq { struct { int a; } in; } mn_wq;", "mn_wq"),
    ("stray variable", "int mn_x;", "mn_x"),
    ("function with a body", "int mn_a(int a) { return a; }", "mn_a"),
    ("duplicate name", "int mn_a(int a);\nint64_t mn_b(void);\nint mn_a(int64_t a);", "mn_a"),
    ("other typedef", "typedef int mn_flag_t;", "mn_flag_t"),
    ("macro that is no integer", "#define MN_SHIFT (1 << 4)\n", "MN_SHIFT"),
    ("function-like macro", "#define MN_MAX(a, b) a\n", "MN_MAX"),
    ("extern C left open", 'extern "C" {\nint mn_a(void);\n', "extern"),
    ("extern C closed twice", 'extern "C" {\nint mn_a(void);\n}\n}\n', "extern"),
]


@pytest.mark.parametrize("text,named", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_reader_refuses(text, named):
    with pytest.raises(MicronetHipError, match=re.escape(named)):
        parse_header(text)


def _header_structs():
    """{C struct name: [field names]} by a reading of the header that shares nothing with the reader under test"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef struct \w+ \{(.*?)\} (\w+);", text, flags=re.S):
        out[name] = [w for stmt in body.split(";") for w in re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?:,|$)", stmt.strip())]
    return out


def test_struct_layouts_are_the_compilers(tmp_path):
    """sizeof and every offsetof of the five structs, as the host C++ compiler lays them out from the real header, against the derived ctypes classes"""
    cxx = shutil.which("g++")
    assert cxx, "the host C++ compiler (g++) that tests/emu/build_emu.sh needs is missing"
    structs = _header_structs()
    assert set(structs) == set(_lib.STRUCTS) and all(structs.values())
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "micronet_hip.h"', "int main() {"]
    for name, fields in structs.items():
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    measured = {(s, f): int(v) for s, f, v in (line.split() for line in out.splitlines())}
    derived = {}
    for name, cls in _lib.STRUCTS.items():
        derived[(name, "sizeof")] = C.sizeof(cls)
        for f, _ in cls._fields_:
            derived[(name, f)] = getattr(cls, f).offset
    assert derived == measured


def test_every_integer_define_is_a_module_attribute():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MN_[A-Z0-9_]+)[ \t]+\(?(-?[0-9][0-9a-fA-Fx]*)\)?[ \t]*$", text, flags=re.M)
    assert len(defines) == len(re.findall(r"#\s*define\s+MN_", text)) >= 23
    for name, value in defines:
        assert getattr(_lib, name) == int(value, 0), name
    assert _lib.MN_ENOTSUP == -95 and _lib.MN_BITCONV_ALT == 0x100 and _lib.MN_QA_NCH == 9


def test_the_real_header_gives_the_module_its_surface():
    constants, structs, protos = parse_header(open(HEADER).read())
    assert protos.keys() == _lib.PROTOTYPES.keys() and len(protos) >= 227
    assert set(structs) == set(_lib.STRUCTS)
    for name, cls in _lib.STRUCTS.items():
        assert cls._fields_ == structs[name]
    assert _lib.WQ.__doc__.startswith("mn_wq")
    g = _lib.ConvGeom(2, 3, 8, 8, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0)         # positional constructors in the header's field order
    assert (g.N, g.KH, g.groups, g.in_shuffle) == (2, 3, 1, 0)
    t = _lib.AdamTensor(1, 2, 3, 4, 5, 0.5, 0.25)
    assert (t.p, t.n, t.lr, t.weight_decay) == (1, 5, 0.5, 0.25)
    # host float arrays, as data.augment and optim.Adam pass them, convert to the void pointers a plain `const float*` now becomes
    assert _lib.PROTOTYPES["mn_adam_step_l1"][1][1].from_param((C.c_float * 2)(1.0, 2.0)) is not None


def test_import_names_a_header_it_cannot_read(tmp_path):
    """_lib placed where ../include/micronet_hip.h does not exist: the import fails and says which file it wanted"""
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    shutil.copy(_lib.__file__, pkg / "_lib.py")
    spec = importlib.util.spec_from_file_location("_lib_without_header", str(pkg / "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    with pytest.raises(RuntimeError, match=re.escape(os.path.join("include", "micronet_hip.h"))) as e:
        spec.loader.exec_module(mod)
    assert type(e.value).__name__ == "MicronetHipError" and str(tmp_path) in str(e.value)
