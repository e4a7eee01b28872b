"""
The whole boundary between include/pnyolo.h and its ctypes binding (pixel_nerf_yolo_amd/lib.py), generated from the two of
them, without a GPU: every declared symbol is bound and exported, every parameter and return type agrees in kind with its
argtypes / restype, every descriptor struct has a mirror with the compiler's layout, and every constant of the header has the
value lib.py gives it.  A new entry point needs its declaration, its row in lib.SIGNATURES and, for its constants, a row in
CONSTANTS below; nothing else here is written per entry.
"""
import ctypes as C
import inspect
import re

import pytest

from host_tools import built_lib, c99_program, header_code  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib

# header struct -> its mirror; every struct with a body and every ctypes.Structure of lib.py is here
STRUCTS = {
    "pny_model_desc": plib.ModelDesc, "pny_render_opts": plib.RenderOpts, "pny_render_out": plib.RenderOut,
    "pny_render_saved": plib.RenderSaved, "pny_render_grads": plib.RenderGrads, "pny_adam_hyper": plib.AdamHyper,
    "pny_train_batch_desc": plib.TrainBatchDesc, "pny_train_batch_draws": plib.TrainBatchDraws,
    "pny_yolo_batch_desc": plib.YoloBatchDesc, "pny_rgb_loss_desc": plib.RgbLossDesc, "pny_yolo_loss_desc": plib.YoloLossDesc,
    "pny_yolo_batches_desc": plib.YoloBatchesDesc, "pny_view_metrics_desc": plib.ViewMetricsDesc, "pny_lpips_desc": plib.LpipsDesc,
    "pny_color_jitter_desc": plib.ColorJitterDesc, "pny_ingest_desc": plib.IngestDesc,
    "pny_yolo_targets_desc": plib.YoloTargetsDesc, "pny_detect_views_desc": plib.DetectViewsDesc,
}


def _key_of(table, value):
    (key,) = [k for k, v in table.items() if v == value]
    return key


# header constant -> what lib.py calls it; a constant of the header that is neither here nor in NO_PYTHON_COUNTERPART fails
CONSTANTS = {
    "PNY_ABI_VERSION": plib.ABI_VERSION,
    "PNY_OK": plib.OK, "PNY_ERR_ARG": plib.ERR_ARG, "PNY_ERR_STATE": plib.ERR_STATE, "PNY_ERR_HIP": plib.ERR_HIP,
    "PNY_ERR_NOGPU": plib.ERR_NOGPU, "PNY_ERR_RANGE": plib.ERR_RANGE,
    "PNY_MAX_LATENT_LEVELS": plib.MAX_LATENT_LEVELS,
    "PNY_YOLO_BATCH_MAX_VIEWS": plib.YOLO_BATCH_MAX_VIEWS, "PNY_YOLO_BATCH_MAX_SCALES": plib.YOLO_BATCH_MAX_SCALES,
    "PNY_DETECT_MAX_CANDIDATES": plib.DETECT_MAX_CANDIDATES, "PNY_DETECT_CELLS": plib.DETECT_CELLS,
    "PNY_DETECT_BOXES": plib.DETECT_BOXES, "PNY_DETECT_TARGETS_OVERFLOW": plib.DETECT_TARGETS_OVERFLOW,
    "PNY_DETECT_PREDS_OVERFLOW": plib.DETECT_PREDS_OVERFLOW, "PNY_DETECT_BAD_SEGMENT": plib.DETECT_BAD_SEGMENT,
    "PNY_DETECT_RECORD": len(plib.DETECT_RECORD),
    "PNY_PROJECTION_OFF": plib.PROJECTION["off"], "PNY_PROJECTION_ON": plib.PROJECTION["on"],
    "PNY_PROJECTION_AUTO": plib.PROJECTION["auto"],
    "PNY_PROJECTION_ROUTE_TILED_F32": _key_of(plib.PROJECTION_ROUTE_TILED, "f32"),
    "PNY_PROJECTION_ROUTE_TILED_F16X2": _key_of(plib.PROJECTION_ROUTE_TILED, "f16x2"),
    "PNY_PRECISION_F32": plib.PRECISION["f32"], "PNY_PRECISION_F16X2": plib.PRECISION["f16x2"],
    "PNY_PRECISION_AUTO": plib.PRECISION["auto"], "PNY_PRECISION_F16": plib.PRECISION["f16"],
    "PNY_PRECISION_F16_TRAIN": plib.PRECISION["f16_train"],
    "PNY_RANGE_ACTIVATION": _key_of(plib.RANGE_BITS, "activation"), "PNY_RANGE_GRADIENT": _key_of(plib.RANGE_BITS, "gradient"),
    "PNY_RANGE_WEIGHT": _key_of(plib.RANGE_BITS, "weight"),
    "PNY_ACC_ADD": plib.ACC_ADD, "PNY_ACC_IMMEDIATE": plib.ACC_IMMEDIATE, "PNY_ACC_FINE_ONLY": plib.ACC_FINE_ONLY,
    "PNY_ACC_COARSE_ONLY": plib.ACC_COARSE_ONLY,
    "PNY_FLUSH_COARSE_ONLY": plib.FLUSH_COARSE_ONLY, "PNY_FLUSH_FINE_ONLY": plib.FLUSH_FINE_ONLY,
    "PNY_FINITE_NAN": plib.FINITE_NAN, "PNY_FINITE_INF": plib.FINITE_INF, "PNY_FINITE_MAX_IMMEDIATE": plib.FINITE_MAX_IMMEDIATE,
    "PNY_GT_NHWC_01": plib.GT_LAYOUT["nhwc01"], "PNY_GT_NCHW_PM1": plib.GT_LAYOUT["nchw_pm1"], "PNY_GT_FLAT": plib.GT_FLAT,
    "PNY_LPIPS_F32_NHWC_01": plib.LPIPS_KIND["nhwc01"], "PNY_LPIPS_F32_NCHW_PM1": plib.LPIPS_KIND["nchw_pm1"],
    "PNY_LPIPS_U8_NHWC": plib.LPIPS_KIND["u8"], "PNY_LPIPS_F32_NCHW_01": plib.LPIPS_KIND["nchw01"],
    "PNY_IMG_F32_NCHW_PM1": plib.IMG_F32_NCHW_PM1, "PNY_IMG_U8_NHWC": plib.IMG_U8_NHWC,
    "PNY_JITTER_MAX_OBJS": plib.JITTER_MAX_OBJS,
    "PNY_RESIZE_NONE": plib.RESIZE["none"], "PNY_RESIZE_BILINEAR_U8": plib.RESIZE["bilinear_u8"],
    "PNY_RESIZE_AREA": plib.RESIZE["area"],
    "PNY_YOLO_TARGETS_MAX_ANCHORS": plib.YOLO_TARGETS_MAX_ANCHORS,
}
# constants a Python caller never names (none today: lib.py binds them all)
NO_PYTHON_COUNTERPART = ()

# the scalar types a declaration may use, as ctypes spells them; any other C type fails the test that meets it
C_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
             "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
C_POINTER_TYPEDEFS = ("pny_stream",)


# --------------------------------------------------------------------------- the header, parsed
def declarations():
    """{name: (return type, [parameter, ...])} of every function the header declares, as C text: a parameter keeps its name
    ("const float* xyz_dev", "const float focal[2]")."""
    out = {}
    for ret, name, params in re.findall(r"(?m)^([A-Za-z_][\w \t\*]*?)\s*\b(pny_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_code()):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def struct_bodies():
    """{struct: [field name, ...]} of every `typedef struct pny_x { ... } pny_x;`, in declaration order."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(pny_\w+)\s*\{(.*?)\}\s*\1\s*;", header_code(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            # "double lr, beta1": each declarator's name is its last identifier outside [ ]
            fields += [re.findall(r"[A-Za-z_]\w*", re.sub(r"\[.*?\]", "", d))[-1] for d in decl.split(",")]
        out[name] = fields
    return out


def constant_names():
    """Every #define PNY_* with a numeric body and every enumerator, in header order."""
    code = header_code()
    numeric = r"\(?-?(?:0[xX])?[0-9a-fA-F]+[uUlL]*\)?"
    names = [(m.start(), [m.group(1)]) for m in re.finditer(r"(?m)^[ \t]*#[ \t]*define[ \t]+(PNY_\w+)[ \t]+%s[ \t]*$" % numeric, code)]
    names += [(m.start(), [e.split("=")[0].strip() for e in m.group(1).split(",") if e.strip()])
              for m in re.finditer(r"\benum\b[^{;]*\{(.*?)\}", code, flags=re.S)]
    return [n for _, group in sorted(names) for n in group]


def c_kind(ctype):
    """("pointer",) / ("int", size, signed) / ("float", size) / None (void) of a C type as the header writes it."""
    t = ctype.replace("const ", "").strip()
    if "*" in t or "[" in t or t in C_POINTER_TYPEDEFS:
        return ("pointer",)
    if t == "void":
        return None
    assert t in C_SCALARS, "a C type this test does not know: %r" % ctype
    return ctypes_kind(C_SCALARS[t])


def ctypes_kind(t):
    if t is None:
        return None
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return ("pointer",)
    assert issubclass(t, C._SimpleCData), "a ctypes type this test does not know: %r" % (t,)
    if t._type_ in "fd":
        return ("float", C.sizeof(t))
    return ("int", C.sizeof(t), t._type_.islower())


def without_name(param):
    """A parameter's type: "const float* xyz_dev" -> "const float*", "const float focal[2]" -> "const float[2]"."""
    return re.sub(r"\s*\b[A-Za-z_]\w*\s*(\[[^\]]*\])?$", r"\1", param)


# --------------------------------------------------------------------------- symbols
def test_every_declared_symbol_is_bound_and_exported(built_lib):
    declared = set(declarations())
    assert declared == set(re.findall(r"\b(pny_[a-z0-9_]+)\s*\(", header_code())), "a declaration the parser does not read"
    assert len(declared) >= 20
    bound = set(plib.SIGNATURES)
    assert declared == bound, "declared, not bound: %s; bound, not declared: %s" % (sorted(declared - bound), sorted(bound - declared))
    missing = [name for name in sorted(declared) if not hasattr(built_lib, name)]
    assert not missing, "not exported by the built library: %s" % missing
    assert built_lib.pny_version() == plib.ABI_VERSION == 11
    assert re.search(r"#define\s+PNY_ABI_VERSION\s+%d\b" % plib.ABI_VERSION, header_code())


# --------------------------------------------------------------------------- signatures
def test_every_signature_agrees_in_kind_with_its_binding():
    struct_of = {mirror: name for name, mirror in STRUCTS.items()}
    wrong = []
    for name, (ret, params) in sorted(declarations().items()):
        if name not in plib.SIGNATURES:
            wrong.append("%s: not in lib.SIGNATURES" % name)
            continue
        restype, argtypes = plib.SIGNATURES[name]
        if c_kind(ret) != ctypes_kind(restype):
            wrong.append("%s: returns %r, bound as %r" % (name, ret, restype))
        if len(params) != len(argtypes):
            wrong.append("%s: %d parameters declared, %d bound" % (name, len(params), len(argtypes)))
            continue
        for i, (param, argtype) in enumerate(zip(params, argtypes)):
            ctype = without_name(param)
            if c_kind(ctype) != ctypes_kind(argtype):
                wrong.append("%s: parameter %d %r is bound as %s" % (name, i, param, argtype.__name__))
            # a pointer to a mirror is declared as a pointer to that mirror's struct
            target = getattr(argtype, "_type_", None) if issubclass(argtype, C._Pointer) else None
            if target in struct_of and ctype.replace("const ", "").replace(" ", "") != struct_of[target] + "*":
                wrong.append("%s: parameter %d %r is bound as a pointer to %s" % (name, i, param, target.__name__))
    assert not wrong, "\n".join(wrong)


# --------------------------------------------------------------------------- structs
def test_every_struct_has_a_mirror_with_its_field_names():
    bodies = struct_bodies()
    assert set(bodies) == set(STRUCTS), "structs of the header without a row in STRUCTS, or rows without a struct: %s" % sorted(
        set(bodies) ^ set(STRUCTS))
    mirrors = {c for _, c in inspect.getmembers(plib, inspect.isclass) if issubclass(c, C.Structure) and c.__module__ == plib.__name__}
    assert mirrors == set(STRUCTS.values()), "ctypes.Structure classes of lib.py without a row in STRUCTS: %s" % sorted(
        c.__name__ for c in mirrors ^ set(STRUCTS.values()))
    for name, mirror in STRUCTS.items():
        mirrored = [f[0] for f in mirror._fields_]
        assert bodies[name] == mirrored, "%s has the fields %s, lib.%s has %s" % (name, bodies[name], mirror.__name__, mirrored)


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """One C program, generated from the mirrors: `S struct sizeof`, `F struct field offsetof sizeof` as the compiler has them.
    Its build is also the assertion that the header is strict C99 without a warning."""
    lines = []
    for name, mirror in STRUCTS.items():
        lines.append('    printf("S %s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name))
        lines += ['    printf("F %s %s %%lu %%lu\\n", (unsigned long)offsetof(%s, %s), (unsigned long)sizeof(((%s*)0)->%s));'
                  % (name, f[0], name, f[0], name, f[0]) for f in mirror._fields_]
    source = '#include <stddef.h>\n#include <stdio.h>\n#include "pnyolo.h"\nint main(void) {\n%s\n    return 0;\n}\n' % "\n".join(lines)
    run = c99_program(tmp_path_factory.mktemp("abi_layout"), source)()
    assert run.returncode == 0, (run.returncode, run.stderr)
    sizes, fields = {}, {}
    for row in (line.split() for line in run.stdout.splitlines()):
        if row[0] == "S":
            sizes[row[1]] = int(row[2])
        else:
            fields[row[1], row[2]] = (int(row[3]), int(row[4]))
    return sizes, fields


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_mirror_has_the_compilers_layout(compiled_layout, name):
    sizes, fields = compiled_layout
    mirror = STRUCTS[name]
    assert C.sizeof(mirror) == sizes[name], "sizeof(%s) = %d, lib.%s has %d" % (name, sizes[name], mirror.__name__, C.sizeof(mirror))
    for field, _ in mirror._fields_:
        got = (getattr(mirror, field).offset, getattr(mirror, field).size)
        assert got == fields[name, field], "%s.%s: (offset, size) %s in the header, %s in lib.%s" % (
            name, field, fields[name, field], got, mirror.__name__)


# --------------------------------------------------------------------------- constants
def test_every_constant_has_the_value_lib_gives_it(tmp_path):
    names = constant_names()
    assert "PNY_ABI_VERSION" in names and "PNY_ERR_RANGE" in names and "PNY_RESIZE_AREA" in names and len(names) == len(set(names))
    unknown = [n for n in names if n not in CONSTANTS and n not in NO_PYTHON_COUNTERPART]
    assert not unknown, "constants of the header without a row in CONSTANTS: %s" % unknown
    gone = [n for n in list(CONSTANTS) + list(NO_PYTHON_COUNTERPART) if n not in names]
    assert not gone, "rows of CONSTANTS the header does not define: %s" % gone
    source = '#include <stdio.h>\n#include "pnyolo.h"\nint main(void) {\n%s\n    return 0;\n}\n' % "\n".join(
        '    printf("%s %%ld\\n", (long)(%s));' % (n, n) for n in names)
    run = c99_program(tmp_path, source)()
    assert run.returncode == 0, (run.returncode, run.stderr)
    values = {n: int(v) for n, v in (line.split() for line in run.stdout.splitlines())}
    wrong = ["%s is %d, lib.py has %r" % (n, values[n], CONSTANTS[n]) for n in names if n in CONSTANTS and values[n] != CONSTANTS[n]]
    assert not wrong, "\n".join(wrong)


# --------------------------------------------------------------------------- a C host
def test_header_is_plain_c_and_links(built_lib, tmp_path):
    """include/pnyolo.h is the boundary a C / cgo / JNI host binds: it compiles as strict C99 (-pedantic, no warnings) without
    any HIP or torch header, and a C program linked against the shared library gets the ABI version it was compiled for."""
    run = c99_program(tmp_path, '#include "pnyolo.h"\n#include <stdio.h>\n'
                      "int main(void) { pny_render_opts o; pny_render_out r; pny_model_desc d; (void)o; (void)r; (void)d;\n"
                      '  printf("%d\\n", pny_version()); return pny_version() == PNY_ABI_VERSION ? 0 : 1; }\n', link=True)()
    assert run.returncode == 0 and run.stdout.strip() == str(plib.ABI_VERSION), (run.returncode, run.stdout, run.stderr)
