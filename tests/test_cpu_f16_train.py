"""The single-plane f16 training mode (include/pnyolo.h PNY_PRECISION_F16_TRAIN) at the levels that need no GPU: the ABI
constant and the new function, the Python mirror, and PixelNeRFNet.set_matrix_precision before any scene exists."""
import re

from host_tools import header_text
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd.model import make_model

def test_precision_constant_matches_the_header():
    assert re.search(r"^#define PNY_PRECISION_F16_TRAIN %d\b" % plib.PRECISION["f16_train"], header_text(), re.M)
    assert plib.LAST_PRECISION == {0: "f32", 1: "f16x2", 2: "f16"}
    assert len(set(plib.PRECISION.values())) == len(plib.PRECISION)


def test_last_backward_precision_declared_with_a_signature():
    src = header_text()
    assert re.search(r"^int pny_scene_last_backward_precision\(pny_scene\* s, int\* code\);", src, re.M)
    assert re.search(r"^int pny_model_last_flush_precision\(pny_model\* m, int\* code\);", src, re.M)


def test_set_matrix_precision_f16_train_before_any_scene():
    net = make_model(pconf.default_mv()["model"])
    assert net.set_matrix_precision("f16_train") is net
    assert net._precision == "f16_train"
    assert hasattr(net, "last_backward_precision") and hasattr(net, "last_flush_precision")
