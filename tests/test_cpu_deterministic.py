"""The deterministic latent gradient (include/pnyolo.h pny_model_set_deterministic) at the levels that need no GPU: the two new
functions in the header, the Python mirror and the built library, the unchanged ABI version, PixelNeRFNet.set_deterministic's
argument check, and the default path's sources."""
import os
import re

import pytest

from host_tools import CSRC, header_text
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd.model import make_model

def test_header_declares_the_two_functions():
    src = header_text()
    assert re.search(r"^int pny_model_set_deterministic\(pny_model\* m, int enable\);", src, re.M)
    assert re.search(r"^int pny_scene_last_latent_grad_mode\(pny_scene\* s, int\* deterministic\);", src, re.M)


def test_abi_version_is_still_11():
    assert re.search(r"^#define PNY_ABI_VERSION 11\b", header_text(), re.M)   # the mode only adds functions
    assert plib.ABI_VERSION == 11


def test_lib_binds_them():
    assert plib.SIGNATURES["pny_model_set_deterministic"][1] == [plib.C.c_void_p, plib.C.c_int]
    assert plib.SIGNATURES["pny_scene_last_latent_grad_mode"][1][0] is plib.C.c_void_p


def test_built_library_exports_them():
    if not os.path.exists(plib.LIB_PATH):
        plib.build()
    lib = plib.load()
    assert hasattr(lib, "pny_model_set_deterministic") and hasattr(lib, "pny_scene_last_latent_grad_mode")
    assert lib.pny_version() == 11
    # null handles are argument errors, not crashes
    assert lib.pny_model_set_deterministic(None, 1) < 0
    assert lib.pny_scene_last_latent_grad_mode(None, None) < 0


@pytest.mark.parametrize("bad", ["on", "AUTO", 1, 0, None, "true", 1.0])
def test_set_deterministic_rejects_other_values(bad):
    net = make_model(pconf.default_mv()["model"])
    with pytest.raises(ValueError):
        net.set_deterministic(bad)
    assert net._deterministic == "auto"


def test_set_deterministic_accepts_the_three_modes():
    net = make_model(pconf.default_mv()["model"])
    assert net._deterministic == "auto"          # the default: torch.use_deterministic_algorithms decides
    for mode in (True, False, "auto"):
        assert net.set_deterministic(mode) is net
        assert net._deterministic is mode or net._deterministic == mode


def test_default_kernels_keep_their_float_atomics():
    """The fixed-point epilogue exists only in the PNY_LG_FIXED build: without it the macros expand to the default
    kernels' own names, output type and float atomic (the disassembly of the default kernels is unchanged)."""
    fx = open(os.path.join(CSRC, "latent_grad_fx.h")).read()
    default = fx.split("#else", 1)[1]
    assert "#define PNY_LG32_KERNEL latent_grad_kernel" in default
    assert "#define PNY_LG_OUT float" in default
    assert "#define PNY_LG_ADD(p, x) unsafeAtomicAdd((p), (x))" in default
    for f in ("latent_grad_det.hip", "latent_grad_h2_det.hip", "latent_grad_h1_det.hip"):
        assert "#define PNY_LG_FIXED" in open(os.path.join(CSRC, f)).read()
        assert f in open(os.path.join(CSRC, "Makefile")).read()
