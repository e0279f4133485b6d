"""The C-ABI library loads and exports every symbol include/scorp_gs.h declares (no compute: runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from scorp_amd import build
    return build.build()


def header_functions():
    txt = open(os.path.join(ROOT, "include", "scorp_gs.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(scorp_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_expected_entry_points():
    fns = header_functions()
    for f in ("scorp_gs3d_preprocess", "scorp_gs3d_num_pairs", "scorp_gs3d_render", "scorp_gs3d_backward",
              "scorp_last_error", "scorp_version"):
        assert f in fns


def test_library_exports_every_declared_symbol(built_lib):
    lib = ctypes.CDLL(built_lib)
    for f in header_functions():
        assert hasattr(lib, f), f"{f} declared in include/scorp_gs.h but not exported by libscorp_gs.so"


def test_binding_lists_every_declared_symbol(built_lib):
    from scorp_amd import _C
    assert sorted(_C.EXPORTS) == header_functions()
    L = _C.lib()
    assert L.scorp_version() >= 100
    # workspace sizing is pure host arithmetic
    s = L.scorp_gs3d_state_bytes(1_000_000, 1600, 1200)
    assert 64 * 1_000_000 <= s < 128 * 1_000_000   # records + bin + tile masks + pixel state + block histograms
    assert L.scorp_gs3d_pairs_bytes(1_500_000) >= 12 * 1_500_000
    assert L.scorp_gs3d_backward_scratch_bytes(1000) >= 48 * 1000


def test_struct_layout_matches_header():
    from scorp_amd import _C
    assert ctypes.sizeof(_C.ScorpGs3dInputs) == 40 + 12 * 8 + 8   # 10 ints/floats, 12 pointers, raw_params + padding
    assert ctypes.sizeof(_C.ScorpGs3dGrads) == 9 * 8
    assert ctypes.sizeof(_C.ScorpGs3dTrainView) == 13 * 8 + 2 * 4 + 9 * 8   # see the struct in include/scorp_gs.h
    assert ctypes.sizeof(_C.ScorpFusedAdam) == 12 * 8 + 8 * 4 + 3 * 8 + 2 * 4 + 4 * 8


def header_prototypes():
    """{function: number of comma-separated parameters, 0 for (void)} by the crude expression of header_functions()."""
    txt = open(os.path.join(ROOT, "include", "scorp_gs.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: 0 if params.strip() == "void" else params.count(",") + 1
            for name, params in re.findall(r"\b(scorp_[a-z0-9_]+)\s*\(([^()]*)\)", txt)}


def test_reader_agrees_with_the_crude_witness():
    """The names the binding derives are the ones header_functions() finds, and every argtypes list is as long as the
    prototype's text has parameters: a dropped prototype or parameter shows without trusting the reader."""
    from scorp_amd import _C
    assert sorted(_C.FUNCTIONS) == header_functions()
    counts = header_prototypes()
    assert sorted(counts) == header_functions()
    for name, (_, argtypes) in _C.FUNCTIONS.items():
        assert len(argtypes) == counts[name], name


def test_header_is_plain_c(tmp_path):
    """include/scorp_gs.h must be consumable from C (the boundary is a C ABI), and every struct there must have, by the C
    compiler's own sizeof / offsetof, the size and the field offsets of the ctypes class derived from it."""
    import subprocess
    from scorp_amd import _C
    assert len(_C.STRUCTS) == 13
    c_name = {py: c for c, py in _C._FIELD_RENAMES.items()}
    want, prints = [], []
    for name, cls in _C.STRUCTS.items():
        want.append(ctypes.sizeof(cls))
        prints.append(f'printf("%zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            want.append(getattr(cls, field).offset)
            prints.append(f'printf("%zu\\n", offsetof({name}, {c_name.get(field, field)}));')
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "scorp_gs.h"\nint main(void) {\n' + "\n".join(prints) + "\nreturn 0; }\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


SYNTHETIC = """/* a comment with scorp_fake(int x); and a ; in it */
#ifndef SCORP_GS_H
#define SCORP_GS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void *scorp_stream_t;
#define SCORP_A 1u
#define SCORP_B (-4)   /* negative */
#define SCORP_C 0.3f
typedef struct ScorpT0 {
  uint64_t first, count;
} ScorpT0;
typedef struct ScorpT {
  const ScorpT0 *in;   /* a keyword in Python */
  float center[3];
  float *exp_avg[6];
  const float *x, *y, *z;
  double a, b, c;
  int32_t n, _pad;
} ScorpT;
int scorp_one(void);
const char *scorp_name(int k);
int32_t scorp_rows(int32_t a, int32_t b);
size_t scorp_bytes(uint64_t capacity);
int scorp_three(const ScorpT *t,
                const void *state, uint8_t *flags, int64_t n, double r,
                float s, uint32_t f, scorp_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_on_a_synthetic_header():
    from scorp_amd import _C
    vp, P = ctypes.c_void_p, ctypes.POINTER
    functions, structs, constants = _C.parse_header(SYNTHETIC)
    assert list(functions) == ["scorp_one", "scorp_name", "scorp_rows", "scorp_bytes", "scorp_three"]   # no scorp_fake
    assert functions["scorp_one"] == (ctypes.c_int, [])
    assert functions["scorp_name"] == (ctypes.c_char_p, [ctypes.c_int])
    assert functions["scorp_rows"] == (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32])
    assert functions["scorp_bytes"] == (ctypes.c_size_t, [ctypes.c_uint64])
    T = structs["ScorpT"]
    assert list(structs) == ["ScorpT0", "ScorpT"] and T.__name__ == "ScorpT"
    assert structs["ScorpT0"]._fields_ == [("first", ctypes.c_uint64), ("count", ctypes.c_uint64)]
    restype, argtypes = functions["scorp_three"]
    assert restype is ctypes.c_int and issubclass(argtypes[0], ctypes._Pointer) and argtypes[0]._type_ is T
    assert argtypes[1:] == [vp, vp, ctypes.c_int64, ctypes.c_double, ctypes.c_float, ctypes.c_uint32, vp]
    assert argtypes[0] is P(T)
    got = [(n, t) for n, t in T._fields_]
    assert got == [("inputs", vp), ("center", ctypes.c_float * 3), ("exp_avg", vp * 6), ("x", vp), ("y", vp), ("z", vp),
                   ("a", ctypes.c_double), ("b", ctypes.c_double), ("c", ctypes.c_double), ("n", ctypes.c_int32),
                   ("_pad", ctypes.c_int32)]
    assert constants == {"A": 1, "B": -4, "C": 0.3} and type(constants["A"]) is int and type(constants["C"]) is float


@pytest.mark.parametrize("bad, line, word", [
    ("int scorp_f(long foo);", 3, "long"),                                    # an unknown type
    ("int scorp_f(int32_t n,\n  int (*done)(int), void *p);", 4, "done"),     # a function-pointer parameter, on its line
    ("#define SCORP_D (1 << 3)", 3, "SCORP_D"),                               # a value that is no literal
    ("typedef struct ScorpU {\n  int32_t n;\n", 3, "ScorpU"),                # an unterminated struct
    ("typedef struct ScorpU {\n  int32_t n : 3;\n} ScorpU;", 4, "n : 3"),    # a bit-field
    ("typedef struct ScorpU {\n  ScorpU0 *p;\n} ScorpU;", 4, "ScorpU0"),     # a struct the header does not declare
    ("void scorp_f(int32_t n);", 3, "void"),                                  # a return type outside the table
    ("typedef struct ScorpU {\n  int32_t n;\n} ScorpU;\ntypedef struct ScorpV {\n  ScorpU u;\n} ScorpV;", 7, "ScorpU"),   # by value
    ("typedef struct ScorpU {\n  union { int32_t n; float f; } u;\n} ScorpU;", 4, "union"),
], ids=["unknown-type", "function-pointer", "define-expression", "unterminated-struct", "bit-field", "undeclared-struct",
        "void-return", "struct-by-value", "union"])
def test_reader_refuses_what_it_does_not_know(bad, line, word):
    """No fallback to int and no silent skip: the error names the header line."""
    from scorp_amd import _C
    with pytest.raises(_C.HeaderError, match=rf"line {line}: .*{re.escape(word)}"):
        _C.parse_header("/* two lines\n   of comment */\n" + bad + "\nint scorp_after(void);\n")


def test_constants_match_the_header():
    from scorp_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scorp_gs.h")).read(), flags=re.S)
    defines = re.findall(r"^#define SCORP_(\w+)[ \t]+(\S.*?)\s*$", txt, flags=re.M)
    assert len(defines) == 24 and len(_C.CONSTANTS) == 24
    for name, value in defines:
        written = value.strip("()").rstrip("uf")
        assert getattr(_C, name) == (float(written) if "." in written else int(written)), name
    assert _C.ERR_INVALID == -1 and _C.BACKWARD_DETERMINISTIC == 4 and _C.VOTE_BINARY == 2
    assert _C.DEPTH_SENSOR_MIN == 0.3 and _C.ADAM_MAX_TENSORS == 8
    assert not hasattr(_C, "GS_H")


def test_stale_library_is_named(built_lib, monkeypatch):
    """A library that lacks a function the header declares is refused when it is loaded, by the function's name."""
    from scorp_amd import _C

    class Stale:
        def __init__(self, path):
            pass

        def __getattr__(self, name):
            if name == "scorp_gs2d_render_score":
                raise AttributeError(name)
            return type("Function", (), {})()

    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", Stale)
    with pytest.raises(RuntimeError, match="scorp_gs2d_render_score.*rebuild"):
        _C.lib()
    assert _C._lib is None


def test_shim_packages_expose_reference_names(built_lib):
    import diff_gaussian_rasterization as dgr
    fields = dgr.GaussianRasterizationSettings._fields
    assert fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                      "projmatrix", "sh_degree", "campos", "prefiltered", "debug")
    r = dgr.GaussianRasterizer(raster_settings=None)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=None, means2D=None, opacities=None, shs=None, colors_precomp=None, scales=1, rotations=1)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=None, means2D=None, opacities=None, shs=1, colors_precomp=None, scales=1, rotations=1, cov3D_precomp=1)


@pytest.mark.parametrize("case, reason", [("wide", b"65535 tiles"), ("scales_only", b"scales+rotations")])
def test_gs2d_preprocess_applies_the_3dgs_input_checks(built_lib, case, reason):
    """2DGS validates its inputs as 3DGS does: an image wider than 65535 tiles (BinRec's tile rectangles are uint16) and
    scales without rotations beside a precomputed transform are refused.  Validation runs before any HIP call, so the
    dummy pointers are never dereferenced and no GPU is needed."""
    from scorp_amd import _C
    L = _C.lib()
    dummy = 0x10000   # non-zero, 256-byte aligned
    inp = _C.ScorpGs3dInputs(num_gaussians=1, sh_degree=0, sh_coeffs=1, image_width=64, image_height=64, tanfovx=1.0,
                             tanfovy=1.0, scale_modifier=1.0, bg=dummy, viewmatrix=dummy, projmatrix=dummy, campos=dummy,
                             means3D=dummy, shs=dummy, opacities=dummy, scales=dummy)
    if case == "wide":
        inp.image_width = 16 * 65535 + 1
        inp.rotations = dummy
    else:
        inp.cov3D_precomp = dummy
    rc = L.scorp_gs2d_preprocess(ctypes.byref(inp), dummy, dummy, 0, None)   # (state_bytes 0: never past the state check)
    assert rc == -1   # SCORP_ERR_INVALID
    assert reason in L.scorp_last_error()
