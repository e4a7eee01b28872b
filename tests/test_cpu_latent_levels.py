"""
The list-of-feature-maps latent without a GPU (include/pnyolo.h pny_latent_levels, pny_latent_levels_backward,
pny_scene_set_latent_levels; PixelNeRFNet.encode(latent=[...]); tests/latent_levels_ref.py):

  * the recorded float32-restatement figures behind the sweep's bars, measured again, and the bars under their caps;
  * the committed golden (tools/make_golden.py fixture_latent_levels: the reference's SpatialEncoder.forward, backbone =
    "custom", over a stub backbone) against the restatement, bit for bit, and a level of the latent's own size as a copy;
  * the C ABI: declared, bound, exported, still version 11; every listed refusal, before any launch, naming its function;
  * PixelNeRFNet.encode's refusals of a bad list, by name.
"""
import ctypes as C
import os
import re

import pytest
import torch

import latent_levels_ref as lr
from host_tools import CSRC, built_lib, header_code, header_text  # noqa: F401
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd.model import check_latent_levels, make_model

ENTRIES = ("pny_latent_levels", "pny_latent_levels_backward", "pny_scene_set_latent_levels")


@pytest.fixture(scope="module")
def restatement_errors():
    """Per case (forward error, backward error) of the float32 restatement against float64."""
    out = {}
    for c in lr.all_cases():
        maps, g = lr.inputs(c)
        fwd = lr.rel_err(lr.latent_ref(maps, lr.F32), lr.latent_ref(maps), "act")
        bwd = max(lr.rel_err(a, b, "grad") for a, b in zip(lr.grads_ref(maps, g, lr.F32), lr.grads_ref(maps, g)))
        out[lr.case_id(c)] = (fwd, bwd)
    return out


def test_case_list_is_the_sweep():
    ids = [lr.case_id(c) for c in lr.all_cases()]
    assert len(ids) == len(set(ids)) == 6 * 8
    for c in lr.all_cases():
        assert len(c["sizes"]) == len(c["channels"]) and 1 <= len(c["sizes"]) <= lr.MAX_LEVELS == plib.MAX_LATENT_LEVELS
    tags = {c["tag"] for c in lr.all_cases()}
    assert tags == {"plain", "one_level", "eight_levels"}
    assert any(len(c["sizes"]) == 8 for c in lr.all_cases()) and any(len(c["sizes"]) == 1 for c in lr.all_cases())


def test_recorded_figures_are_what_the_restatement_measures(restatement_errors):
    fwd = max(v[0] for v in restatement_errors.values())
    bwd = max(v[1] for v in restatement_errors.values())
    print("float32 restatement vs float64: forward %.3e (recorded %.3e), backward %.3e (recorded %.3e)"
          % (fwd, lr.FWD_ERR32, bwd, lr.BWD_ERR32))
    assert 0.5 * lr.FWD_ERR32 <= fwd <= 1.1 * lr.FWD_ERR32
    assert 0.5 * lr.BWD_ERR32 <= bwd <= 1.1 * lr.BWD_ERR32


def test_bars_are_twice_the_figures_and_under_their_caps_on_every_case(restatement_errors):
    assert lr.FWD_BAR == 2 * lr.FWD_ERR32 and lr.BWD_BAR == 2 * lr.BWD_ERR32
    assert lr.FWD_BAR <= lr.CAP_ACT == 2e-4 and lr.BWD_BAR <= lr.CAP_GRAD == 1e-4
    for key, (fwd, bwd) in restatement_errors.items():
        assert 2 * fwd <= lr.CAP_ACT and 2 * bwd <= lr.CAP_GRAD, key      # (the bar this case alone would set)


def test_golden_latent_is_the_restatement_bit_for_bit(golden):
    g = golden("latent_levels")
    keys = sorted({k.split("/")[0] for k in g})
    by_id = {lr.case_id(c): c for c in lr.all_cases()}
    assert len(keys) == 12 and all(k in by_id for k in keys)
    assert {by_id[k]["name"] for k in keys} == set(lr.SIZES)
    for k in keys:
        maps, _ = lr.inputs(by_id[k])
        for i, m in enumerate(maps):
            assert torch.equal(torch.from_numpy(g["%s/map%d" % (k, i)]), m), (k, i)
        assert torch.equal(torch.from_numpy(g[k + "/latent"]), lr.latent_ref(maps, lr.F32)), k


def test_level_of_the_latents_size_is_a_copy():
    for c in lr.all_cases():
        maps, _ = lr.inputs(c)
        lat, off = lr.latent_ref(maps, lr.F32), 0
        seen = 0
        for m in maps:
            if m.shape[-2:] == maps[0].shape[-2:]:
                assert torch.equal(lat[:, off:off + m.shape[1]], m), lr.case_id(c)
                seen += 1
            off += m.shape[1]
        assert seen >= 1 + (c["name"] == "same_size" and c["tag"] == "plain")


# --------------------------------------------------------------------------- the C ABI
def test_entries_are_declared_bound_and_exported():
    assert plib.MAX_LATENT_LEVELS == 8 and "encoder.py:126-137" in header_text()      # (the header's 8: tests/test_cpu_abi.py)
    flat = re.sub(r"\s+", "", header_code())
    levels = ["const int* channels", "const int* h", "const int* w", "int n_levels"]
    decls = {
        "pny_latent_levels": ["const float* const* maps_dev"] + levels + ["int n", "float* latent_nhwc_dev", "pny_stream stream"],
        "pny_latent_levels_backward": ["const float* d_latent_nhwc_dev", "float* const* d_maps_dev"] + levels + ["int n", "pny_stream stream"],
        "pny_scene_set_latent_levels": ["pny_scene* s", "const float* const* maps_dev"] + levels + ["int ns", "pny_stream stream"],
    }
    assert tuple(decls) == ENTRIES
    ip, vpp = C.POINTER(C.c_int), C.POINTER(C.c_void_p)
    types = {
        "pny_latent_levels": [vpp, ip, ip, ip, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
        "pny_latent_levels_backward": [C.c_void_p, vpp, ip, ip, ip, C.c_int, C.c_int, C.c_void_p],
        "pny_scene_set_latent_levels": [C.c_void_p, vpp, ip, ip, ip, C.c_int, C.c_int, C.c_void_p],
    }
    for name, args in decls.items():
        assert "int" + name + "(" + ",".join(a.replace(" ", "") for a in args) + ");" in flat, name
        res, argtypes = plib.SIGNATURES[name]
        assert res is C.c_int and argtypes == types[name], name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " latent_levels.hip" in mk


def _arr(vals):
    return None if vals is None else (C.c_int * len(vals))(*vals)


def _ptrs(vals):
    return None if vals is None else (C.c_void_p * len(vals))(*vals)


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_bad_arguments_before_any_launch(built_lib, entry):
    """PNY_ERR_ARG (-1) and the function's name in the message, with or without a GPU: no pointer is followed to the device, and
    the scene entry looks at its scene only after the list has passed."""
    err = built_lib.pny_last_error
    good = dict(first=C.c_void_p(4096), maps=(8192, 12288, 16384), channels=(4, 8, 12), h=(9, 5, 3), w=(15, 8, 4), n_levels=3, n=2,
                lat=C.c_void_p(1 << 20))

    def rc(**kw):
        a = dict(good, **kw)
        lists = (_ptrs(a["maps"]), _arr(a["channels"]), _arr(a["h"]), _arr(a["w"]), a["n_levels"], a["n"])
        if entry == "pny_latent_levels":
            return built_lib.pny_latent_levels(*lists, a["lat"], None)
        if entry == "pny_latent_levels_backward":
            return built_lib.pny_latent_levels_backward(a["lat"], *lists, None)
        return built_lib.pny_scene_set_latent_levels(a["first"], *lists, None)

    def refused(what, **kw):
        assert rc(**kw) == -1, (entry, kw)
        msg = err().decode()
        assert msg.startswith(entry + ":") and what in msg, (entry, kw, msg)

    for kw in (dict(maps=None), dict(channels=None), dict(h=None), dict(w=None)):
        refused("null", **kw)
    if entry == "pny_scene_set_latent_levels":
        refused("null", first=None)
    else:
        refused("null", lat=None)
    if entry != "pny_latent_levels_backward":          # (the backward's NULL entries are levels to skip)
        for i in range(3):
            refused("null map", maps=tuple(None if j == i else 4096 * (j + 2) for j in range(3)))
    for n_levels in (0, -1, 9):
        refused("n_levels", n_levels=n_levels)
    for key in ("channels", "h", "w"):
        for i in range(3):
            for bad in (0, -4):
                refused("at least 1", **{key: tuple(bad if j == i else good[key][j] for j in range(3))})
    for n in (0, -1):
        refused("at least 1", n=n)
    refused("2^31", h=(9, 65536, 3), w=(15, 32768, 4))


# --------------------------------------------------------------------------- Python
def test_python_refuses_a_bad_list_by_name():
    maps = [torch.zeros(2, 24, 9, 15), torch.zeros(2, 40, 5, 8), torch.zeros(2, 64, 3, 4)]
    assert check_latent_levels(maps, 2, 128) == ((24, 9, 15), (40, 5, 8), (64, 3, 4))
    assert check_latent_levels(tuple(m.half() for m in maps), 2, 128) == ((24, 9, 15), (40, 5, 8), (64, 3, 4))
    with pytest.raises(ValueError, match="empty list"):
        check_latent_levels([], 2, 128)
    with pytest.raises(ValueError, match="more than 8 levels"):
        check_latent_levels([torch.zeros(2, 1, 3, 3)] * 9, 2, 9)
    with pytest.raises(ValueError, match="map 1 is not a 4-D"):
        check_latent_levels([maps[0], maps[1][0], maps[2]], 2, 128)
    with pytest.raises(ValueError, match="map 2 is not a 4-D"):
        check_latent_levels([maps[0], maps[1], "x"], 2, 128)
    with pytest.raises(ValueError, match="leading sizes differ: map 1"):
        check_latent_levels([maps[0], maps[1][:1], maps[2]], 2, 128)
    with pytest.raises(ValueError, match="leading sizes differ: map 0"):
        check_latent_levels(maps, 4, 128)
    with pytest.raises(ValueError, match="sum to 128, d_latent is 512"):
        check_latent_levels(maps, 2, 512)


def test_encode_refuses_a_bad_list_before_it_touches_the_device():
    net = make_model(pconf.default_mv()["model"]).eval()          # d_latent = 512; never moved to a device
    images, poses = torch.zeros(1, 2, 3, 64, 64), torch.eye(4).expand(1, 2, 4, 4)
    maps = [torch.zeros(2, 256, 8, 8), torch.zeros(2, 256, 4, 4)]
    for bad, what in (([], "empty list"), (maps[:1], "sum to 256, d_latent is 512"), ([maps[0], maps[1][:1]], "leading sizes differ"),
                      ([maps[0], maps[1][0]], "not a 4-D"), ([torch.zeros(2, 64, 2, 2)] * 9, "more than 8 levels")):
        with pytest.raises(ValueError, match=what):
            net.encode(images, poses, torch.tensor(60.0), latent=bad)
        with pytest.raises(ValueError, match=what):
            net.encode(images[0], poses[0], torch.tensor(60.0), latent=tuple(bad))
