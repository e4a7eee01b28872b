"""
LPIPS without a GPU: the fp64 restatement (tests/lpips_ref.py) has the properties the definition gives it; the weight loaders
of metrics.LPIPS map every accepted naming to the same 31 tensors and name what is wrong; the workspace sizing is the formula
written in csrc/pny_lpips.h and refuses what the forward refuses; lpips_views and LPIPS.__call__ refuse CPU tensors, wrong
shapes and unknown layouts before any device is looked at.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lpips_ref as lr
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import metrics as pmetrics
from pixel_nerf_yolo_amd import synth

F64 = torch.float64


@pytest.fixture(scope="module")
def state():
    return synth.vgg16_lpips_state(4711)


@pytest.fixture(scope="module")
def weights(state):
    return lr.weights_of(state)


def test_seeded_state_has_the_package_names_and_shapes(state):
    assert len(state) == 31
    for (cin, cout), f, s in zip(lr.CHANNELS, lr.FEATURES, lr.SLICE):
        assert state["net.slice%d.%d.weight" % (s, f)].shape == (cout, cin, 3, 3)
        assert state["net.slice%d.%d.bias" % (s, f)].shape == (cout,)
    for k, c in enumerate(lr.TAP_CH):
        w = state["lin%d.model.1.weight" % k]
        assert w.shape == (1, c, 1, 1) and (w >= 0).all() and w.dtype == np.float32
    again = synth.vgg16_lpips_state(4711)
    assert all(np.array_equal(state[k], again[k]) for k in state)


def test_identical_images_give_exactly_zero(weights):
    x, _ = lr.images(1, 2, 16, 16)
    val, _, _ = lr.lpips(x, x.clone(), *weights, dtype=F64)
    assert val.dtype == F64 and torch.equal(val, torch.zeros(2, dtype=F64))


def test_value_is_symmetric_and_positive(weights):
    p, g = lr.images(2, 2, 19, 21)
    a, _, _ = lr.lpips(p, g, *weights, dtype=F64)
    b, _, _ = lr.lpips(g, p, *weights, dtype=F64)
    assert torch.equal(a, b)          # (u - v)^2 == (v - u)^2 exactly, and the taps are summed in the same order
    assert bool((a > 0).all())


@pytest.mark.parametrize("hw, sizes", [((16, 16), [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]),
                                       ((19, 21), [(19, 21), (9, 10), (4, 5), (2, 2), (1, 1)])])
def test_tap_sizes(weights, hw, sizes):
    p, g = lr.images(3, 1, *hw)
    _, t0, t1 = lr.lpips(p, g, *weights, dtype=F64)
    assert [tuple(t.shape) for t in t0] == [(1, c) + s for c, s in zip(lr.TAP_CH, sizes)]
    assert [t.shape for t in t1] == [t.shape for t in t0]


def test_a_pixel_of_zero_features_contributes_zero():
    f0, f1 = torch.zeros(1, 64, 1, 2, dtype=F64), torch.zeros(1, 64, 1, 2, dtype=F64)
    f0[0, :, 0, 1], f1[0, :, 0, 1] = 1.0, 2.0           # the other pixel: the same direction, so zero as well
    d = lr.tap_distance(f0, f1, torch.ones(64))
    assert torch.isfinite(d).all() and float(d.abs().max()) < 1e-18


# ------------------------------------------------------------------------------------------------ weight loaders
def same_tensors(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_every_naming_maps_to_the_same_31_tensors(state, weights):
    convs, lins = weights
    by_package = pmetrics.LPIPS().load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}).tensors
    assert sorted(by_package) == sorted(pmetrics.lpips_tensor_names()) and len(by_package) == 31
    for i, (w, b) in enumerate(convs):
        assert torch.equal(by_package["conv%d.weight" % i], w) and torch.equal(by_package["conv%d.bias" % i], b)
    for k, w in enumerate(lins):
        assert by_package["lin%d.weight" % k].shape == (lr.TAP_CH[k],) and torch.equal(by_package["lin%d.weight" % k], w)
    assert same_tensors(by_package, pmetrics.LPIPS().load_state_dict(lr.torchvision_state(state)).tensors)
    assert same_tensors(by_package, pmetrics.LPIPS().load_tensors(convs, lins).tensors)
    # the package's full dict: the `lins` duplicates and the scaling layer's buffers beside the rest
    full = dict(state)
    for k in range(5):
        full["lins.%d.model.1.weight" % k] = full["lin%d.model.1.weight" % k]
    full["scaling_layer.shift"] = np.array(lr.SHIFT, np.float32).reshape(1, 3, 1, 1)
    full["scaling_layer.scale"] = np.array(lr.SCALE, np.float32).reshape(1, 3, 1, 1)
    assert same_tensors(by_package, pmetrics.LPIPS().load_state_dict(full).tensors)
    only_lins = {k: v for k, v in full.items() if not k.startswith("lin") or k.startswith("lins.")}
    assert same_tensors(by_package, pmetrics.LPIPS().load_state_dict(only_lins).tensors)


def test_loader_errors_name_the_key(state):
    sd = dict(state)
    del sd["net.slice3.12.bias"]
    with pytest.raises(KeyError, match=r"net\.slice3\.12\.bias"):
        pmetrics.LPIPS().load_state_dict(sd)
    tv = lr.torchvision_state(state)
    del tv["features.17.weight"]
    with pytest.raises(KeyError, match=r"features\.17\.weight"):
        pmetrics.LPIPS().load_state_dict(tv)
    sd = dict(state)
    sd["net.slice2.7.weight"] = sd["net.slice2.7.weight"][:, :64]
    with pytest.raises(ValueError, match=r"net\.slice2\.7\.weight.*\(128, 64, 3, 3\).*\(128, 128, 3, 3\)"):
        pmetrics.LPIPS().load_state_dict(sd)
    sd = dict(state)
    sd["lin4.model.1.weight"] = sd["lin4.model.1.weight"][:, :100]
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        pmetrics.LPIPS().load_state_dict(sd)
    sd = dict(state)
    sd["scaling_layer.shift"] = np.array([-.03, -.088, -.2], np.float32)
    with pytest.raises(ValueError, match=r"scaling_layer\.shift"):
        pmetrics.LPIPS().load_state_dict(sd)
    convs, lins = lr.weights_of(state)
    with pytest.raises(ValueError, match=r"convs\[5\]\[1\]"):
        pmetrics.LPIPS().load_tensors(convs[:5] + [(convs[5][0], convs[5][1][:7])] + convs[6:], lins)
    with pytest.raises(ValueError, match="13"):
        pmetrics.LPIPS().load_tensors(convs[:12], lins)


def test_other_nets_are_not_implemented():
    for net in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match=net):
            pmetrics.LPIPS(net=net)


def test_library_loader_names_the_tensor():
    L = plib.load()
    h = C.c_void_p()
    plib.check(L.pny_lpips_create(C.byref(h)))
    try:
        data = (C.c_float * 64)()
        shape = (C.c_int64 * 1)(64)
        assert L.pny_lpips_load_weights(h, b"conv0.bias", data, shape, 1) == 0
        assert L.pny_lpips_load_weights(h, b"lin0.weight", data, shape, 1) == 0
        for name in (b"conv13.weight", b"lin5.weight", b"lin0.bias", b"conv.weight", b"features.0.weight"):
            assert L.pny_lpips_load_weights(h, name, data, shape, 1) == -1
            assert name.decode() in L.pny_last_error().decode()
        assert L.pny_lpips_load_weights(h, b"conv2.bias", data, shape, 1) == -1      # 128 channels
        assert "conv2.bias" in L.pny_last_error().decode() and "(64)" in L.pny_last_error().decode()
        assert L.pny_lpips_finalize(h, None) == -2                                   # PNY_ERR_STATE before any device call
        assert "conv0.weight" in L.pny_last_error().decode()
    finally:
        L.pny_lpips_destroy(h)


# ------------------------------------------------------------------------------------------------ workspace sizing
def r64(count):
    return (count + 63) // 64 * 64


def formula(n, h, w):
    """csrc/pny_lpips.h: 4 (r64(2n H W 4) + 2 r64(2n H W 64)) bytes"""
    return 4 * (r64(2 * n * h * w * 4) + 2 * r64(2 * n * h * w * 64))


@pytest.mark.parametrize("n, h, w", [(1, 16, 16), (3, 19, 21), (32, 128, 128), (1, 400, 400), (5, 17, 33)])
def test_workspace_bytes_is_the_formula(n, h, w):
    assert pmetrics.lpips_workspace_bytes(n, h, w) == formula(n, h, w)


def test_workspace_bytes_refuses_small_images_and_32bit_overflow():
    for h, w in ((15, 16), (16, 15), (1, 400)):
        with pytest.raises(plib.PnyError, match="at least 16"):
            pmetrics.lpips_workspace_bytes(1, h, w)
    # 2 n H W 64 < 2^31: 128 x 128 allows 1023 pairs, not 1024
    assert pmetrics.lpips_workspace_bytes(1023, 128, 128) == formula(1023, 128, 128)
    with pytest.raises(plib.PnyError, match="32-bit"):
        pmetrics.lpips_workspace_bytes(1024, 128, 128)
    with pytest.raises(plib.PnyError, match="32-bit"):
        pmetrics.lpips_workspace_bytes(1, 4096, 4096)
    with pytest.raises(plib.PnyError, match="n_pairs"):
        pmetrics.lpips_workspace_bytes(0, 16, 16)


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture(scope="module")
def model(state):
    return pmetrics.LPIPS().load_state_dict(state)


def test_lpips_views_refuses_before_any_device_is_looked_at(model):
    rgb, gt = torch.rand(2, 16, 16, 3), torch.rand(2, 16, 16, 3)
    with pytest.raises(plib.PnyError, match="rgb is on cpu"):
        pmetrics.lpips_views(model, rgb, gt)
    with pytest.raises(plib.PnyError, match="rgb is on cpu"):
        pmetrics.lpips_views(model, (rgb * 255).to(torch.uint8), (gt * 255).to(torch.uint8))
    with pytest.raises(ValueError, match="gt_layout"):
        pmetrics.lpips_views(model, rgb, gt, gt_layout="nchw01")
    with pytest.raises(ValueError, match="gt has shape"):
        pmetrics.lpips_views(model, rgb, gt, gt_layout="nchw_pm1")
    with pytest.raises(ValueError, match="gt has shape"):
        pmetrics.lpips_views(model, rgb, torch.zeros(2, 3, 16, 16, dtype=torch.uint8), gt_layout="nchw_pm1")
    with pytest.raises(ValueError, match="rgb must be"):
        pmetrics.lpips_views(model, rgb[..., :2], gt)
    with pytest.raises(ValueError, match="is not"):
        pmetrics.lpips_views(model, torch.rand(2 * 16 * 16 + 1, 3), gt, H=16, W=16)
    with pytest.raises(ValueError, match="at least 16"):
        pmetrics.lpips_views(model, torch.rand(1, 15, 16, 3), torch.rand(1, 15, 16, 3))
    with pytest.raises(ValueError, match="batch_size"):
        pmetrics.lpips_views(model, rgb, gt, batch_size=0)
    with pytest.raises(plib.PnyError, match="rgb must be fp32 or uint8"):
        pmetrics.lpips_views(model, rgb.double(), gt)
    with pytest.raises(TypeError, match="gt must be a tensor"):
        pmetrics.lpips_views(model, rgb, gt.numpy())
    with pytest.raises(TypeError, match="model"):
        pmetrics.lpips_views(None, rgb, gt)


def test_lpips_call_refuses_before_any_device_is_looked_at(model):
    a, b = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    with pytest.raises(plib.PnyError, match="in0 is on cpu"):
        model(a, b)
    with pytest.raises(ValueError, match="in0 must be"):
        model(a.permute(0, 2, 3, 1), b)
    with pytest.raises(ValueError, match="in1 has shape"):
        model(a, b[:1])
    with pytest.raises(ValueError, match="at least 16"):
        model(a[..., :15], b[..., :15])
    with pytest.raises(plib.PnyError, match="in1 must be fp32"):
        model(a, b.double())
