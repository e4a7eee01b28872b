"""The single-plane f16 precision mode (include/pnyolo.h PNY_PRECISION_F16) at the levels that need no GPU: the ABI constant,
the Python mirror, and the argument check of PixelNeRFNet.set_matrix_precision before any scene exists."""
import re

import pytest

from host_tools import header_text
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd.model import make_model

def test_precision_constant_matches_the_header():
    assert plib.PRECISION["f16"] == 3
    src = header_text()
    assert re.search(r"^#define PNY_PRECISION_F16 3\b", src, re.M)
    for name, code in plib.PRECISION.items():
        assert re.search(r"^#define PNY_PRECISION_%s %d\b" % (name.upper(), code), src, re.M), name
    assert plib.LAST_PRECISION == {0: "f32", 1: "f16x2", 2: "f16"}


def test_set_matrix_precision_f16_before_any_scene():
    net = make_model(pconf.default_mv()["model"])
    assert net.set_matrix_precision("f16") is net
    assert net._precision == "f16"
    with pytest.raises(ValueError):
        net.set_matrix_precision("f8")
    assert net._precision == "f16"
