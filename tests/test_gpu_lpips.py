"""
LPIPS (VGG-16) on the GPU (csrc/lpips.hip, include/pnyolo.h pny_lpips_*, metrics.LPIPS / metrics.lpips_views) against the plain
torch restatement of the published definition (tests/lpips_ref.py), with seeded stand-in weights (synth.vgg16_lpips_state):
  * prepare: bit-equal to the float32 torch expression for the three input kinds (and the [0, 1] NCHW form of LPIPS.__call__),
    with and without the clamp of a float prediction;
  * pool: bit-equal to torch.nn.functional.max_pool2d(x, 2, 2);
  * each of the 13 convolutions alone against float64, at pixel counts (198, 60) that are no multiple of a tile, K = 4608 among
    them, under the forward-convolution bar of tests/test_gpu_trunk_stages.py, restated here: max |got - ref| over
    max(1, max |ref|) at most 2 x 1.05e-6, twice the largest error of the float32 restatement of a convolution on the CPU;
  * the distance of one tap against float64 for every channel count and 1, 35 and 561 pixels, a pixel that is zero in both
    images, one that is zero in one image, two runs, and adding into a non-zero result;
  * end to end against the float64 restatement: the float32 restatement's own largest deviation over a case's pairs is that
    case's yardstick, the kernel may deviate by 4 yardsticks (the MFMA sums each dot product in another order than ATen: an
    error of the same kind and size, not the same values); exact zero for identical pairs; the same bits at batch sizes 2 and
    5, from bytes and from the bytes / 255, and from LPIPS.__call__ and lpips_views.
  * the tile size of a convolution changes no bit: the same images in a small and a large launch of one VGG layer run
    <1, 1, 1> and <1, 2, 2>, or <8, 1, 1> and <8, 2, 2> (K = 4608 included), and 5 pairs of 64 x 64 agree bit for bit at batch
    sizes 1, 2 and 5, between which the launches' own tile counts would also change the K split.
Each test prints one LPIPS line with its figures.

Distance bar: the kernel's arithmetic on the float32 features is float64 (u = 2^-53), like the restatement's.  A unit feature
a = f (1 / (sqrt(sum f^2) + 1e-10)) carries a relative error of at most 24 u: the sum of C <= 512 exact squares is at most 32
additions deep in a lane and 4 across the lanes (36 u on a sum of positive terms, halved by the root), then the root, the
added 1e-10, the reciprocal and the product.  So (a - b)^2 is off by at most 2 |a - b| 24 u (|a| + |b|) + 2 u (a - b)^2, and the
weighted sum of C positive terms adds at most 40 u of itself: below 96 u S per pixel, S = sum_c w[c] (|a| + |b|)^2.  The sum
over the pixels adds at most npix u, and the restatement's own sums over the channels and the pixels, in ATen's order, at most
(C + npix) u: the bar is (96 + C + 2 npix) u times the pixel mean of S.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import lpips_ref as lr
from helpers import DEV
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import metrics as pmetrics
from pixel_nerf_yolo_amd import synth

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
U64 = 2.0 ** -53
CONV_FWD_BAR = 2 * 1.05e-6          # tests/trunk_stage_ref.py CONV_FWD_BAR
E2E_FACTOR = 4.0
KIND = plib.LPIPS_KIND


def stream():
    return plib.stream_of(torch.device(DEV))


def desc_of(h, w, pred_kind, gt_kind, clamp=False, batch=0):
    return plib.LpipsDesc(height=h, width=w, pred_kind=KIND[pred_kind], gt_kind=KIND[gt_kind], clamp=1 if clamp else 0, batch_size=batch)


@pytest.fixture(scope="module")
def state():
    return synth.vgg16_lpips_state(4711)


@pytest.fixture(scope="module")
def weights(state):
    return lr.weights_of(state)


@pytest.fixture(scope="module")
def model(state):
    return pmetrics.LPIPS().load_state_dict(state)


# ------------------------------------------------------------------------------------------------ prepare
def hip_prepare(pred, gt, pred_kind, gt_kind, n, h, w, clamp=False):
    out = torch.full((2 * n, h, w, 4), float("nan"), device=DEV)
    d = desc_of(h, w, pred_kind, gt_kind, clamp)
    a, b = pred.to(DEV).contiguous(), gt.to(DEV).contiguous()
    plib.check(plib.load().pny_lpips_prepare(C.byref(d), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                             stream()))
    torch.cuda.synchronize()
    return out.cpu()


def stored_forms(seed, n, h, w):
    """kind -> (stored tensor, its float32 (n, 3, h, w) value in [-1, 1] by the torch expression)"""
    rs = np.random.RandomState(seed)
    f01 = torch.from_numpy(rs.uniform(-0.25, 1.25, size=(n, h, w, 3)).astype(np.float32))      # outside [0, 1] too
    pm1 = torch.from_numpy(rs.uniform(-1.0, 1.0, size=(n, 3, h, w)).astype(np.float32))
    u8 = torch.from_numpy(rs.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8))
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)                                   # every byte value
    return {"nhwc01": (f01, lr.pm1_from_01(f01).permute(0, 3, 1, 2)), "nchw_pm1": (pm1, pm1),
            "u8": (u8, lr.pm1_from_bytes(u8).permute(0, 3, 1, 2)),
            "nchw01": (f01.permute(0, 3, 1, 2).contiguous(), lr.pm1_from_01(f01).permute(0, 3, 1, 2))}


@pytest.mark.parametrize("n, h, w", [(1, 16, 16), (3, 19, 21)])
def test_prepare_is_bit_equal_to_the_torch_expression(n, h, w):
    forms, other = stored_forms(10 + n, n, h, w), stored_forms(20 + n, n, h, w)
    for pk in ("nhwc01", "u8", "nchw_pm1", "nchw01"):
        for gk in ("nhwc01", "nchw_pm1", "u8"):
            got = hip_prepare(forms[pk][0], other[gk][0], pk, gk, n, h, w)
            want = torch.cat([lr.prepare(forms[pk][1]), lr.prepare(other[gk][1])])
            assert torch.equal(got, want), (pk, gk, float((got - want).abs().max()))
    print("LPIPS prepare %d x %d x %d: 12 combinations of stored forms bit-equal" % (n, h, w))


def test_prepare_clamps_a_float_prediction_only_on_request():
    n, h, w = 2, 17, 16
    forms = stored_forms(31, n, h, w)
    f01, gt = forms["nhwc01"][0], forms["nhwc01"][0].flip(0).contiguous()
    assert float(f01.min()) < 0 and float(f01.max()) > 1
    got = hip_prepare(f01, gt, "nhwc01", "nhwc01", n, h, w, clamp=True)
    want_pred = lr.prepare(lr.pm1_from_01(f01.clamp(0, 1)).permute(0, 3, 1, 2))
    want_gt = lr.prepare(lr.pm1_from_01(gt).permute(0, 3, 1, 2))               # the ground truth is never clamped
    assert torch.equal(got, torch.cat([want_pred, want_gt]))
    off = hip_prepare(f01, gt, "nhwc01", "nhwc01", n, h, w, clamp=False)
    assert torch.equal(off[:n], lr.prepare(forms["nhwc01"][1])) and not torch.equal(off[:n], got[:n])
    # bytes are in range as they are: the flag changes nothing
    u8 = forms["u8"][0]
    assert torch.equal(hip_prepare(u8, gt, "u8", "nhwc01", n, h, w, clamp=True), hip_prepare(u8, gt, "u8", "nhwc01", n, h, w))


# ------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (1, 16, 16, 512)])
def test_maxpool2_is_bit_equal_to_torch(shape):
    n, h, w, c = shape
    x = torch.from_numpy(np.random.RandomState(h * w).standard_normal(shape).astype(np.float32))
    out = torch.full((n, h // 2, w // 2, c), float("nan"), device=DEV)
    xd = x.to(DEV)
    plib.check(plib.load().pny_lpips_maxpool2(plib.ptr(xd), n, h, w, c, plib.ptr(out), stream()))
    torch.cuda.synchronize()
    want = Fn.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(out.cpu(), want)


# ------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("layer", range(13))
def test_each_convolution_alone_against_fp64(model, weights, layer):
    n, (h, w) = 2, ((9, 11) if layer < 4 else (6, 5))
    cin, cout = lr.CHANNELS[layer]
    wt, b = weights[0][layer]
    x = torch.from_numpy(np.random.RandomState(900 + layer).standard_normal((n, cin, h, w)).astype(np.float32))
    xl = x.permute(0, 2, 3, 1)
    if cin % 4:
        xl = torch.cat([xl, torch.zeros(n, h, w, 4 - cin % 4)], -1)
    xd = xl.contiguous().to(DEV)
    out = torch.full((n, h, w, cout), float("nan"), device=DEV)
    variant = C.c_int(0)
    handle = model._ready(torch.device(DEV))
    plib.check(plib.load().pny_lpips_conv(handle, layer, plib.ptr(xd), n, h, w, plib.ptr(out), C.byref(variant), stream()))
    torch.cuda.synchronize()
    ref = Fn.relu(Fn.conv2d(x.to(F64), wt.to(F64), b.to(F64), 1, 1))
    got = out.cpu().permute(0, 3, 1, 2).to(F64)
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    v = variant.value
    print("LPIPS conv%d %d->%d, K = %d, %d px: error %.3e, bar %.3e (%.2f of the bar), conv_mfma_kernel<%d, %d, %d>"
          % (layer, cin, cout, 9 * cin, n * h * w, err, CONV_FWD_BAR, err / CONV_FWD_BAR, v // 100, v // 10 % 10, v % 10))
    assert v in (811, 822, 111, 122)
    assert err <= CONV_FWD_BAR, (layer, err, CONV_FWD_BAR)


# ------------------------------------------------------------------------------------------------ distance
def hip_distance(tap, w, n, h, wd, c, out, accumulate):
    plib.check(plib.load().pny_lpips_distance(plib.ptr(tap), plib.ptr(w), n, h, wd, c, 1 if accumulate else 0, C.c_void_p(out.data_ptr()),
                                              stream()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("c", [64, 128, 256, 512])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (17, 33)])
def test_distance_against_fp64(c, hw):
    n, (h, wd) = 4, hw
    rs = np.random.RandomState(c + 7 * h)
    feat = np.maximum(rs.standard_normal((2 * n, h, wd, c)), 0.0).astype(np.float32)          # behind a relu
    if h * wd > 1:
        feat[0, 0, 1] = 0.0
        feat[n, 0, 1] = 0.0              # pair 0, pixel 1: zero in both images
        feat[1, h - 1, wd - 1] = 0.0     # pair 1, last pixel: zero in the prediction only
    else:
        feat[0, 0, 0] = 0.0
        feat[n, 0, 0] = 0.0              # pair 0 is its one pixel: zero in both
        feat[1, 0, 0] = 0.0              # pair 1: zero in the prediction only
    feat[3] = 0.0
    feat[n + 3] = 0.0                    # pair 3: every pixel zero in both images, at every size
    w = rs.uniform(0.0, 2.0 / c, size=(c,)).astype(np.float32)
    ft, wt = torch.from_numpy(feat), torch.from_numpy(w)
    f64 = ft.to(F64).permute(0, 3, 1, 2)
    ref = lr.tap_distance(f64[:n], f64[n:], wt)
    a, b = lr.normalize_tensor(f64[:n]), lr.normalize_tensor(f64[n:])
    bar = (96 + c + 2 * h * wd) * U64 * ((a.abs() + b.abs()) ** 2 * wt.to(F64)[None, :, None, None]).sum(1).mean(dim=(1, 2))
    fd, wdv = ft.to(DEV), wt.to(DEV)
    got = hip_distance(fd, wdv, n, h, wd, c, torch.full((n,), float("nan"), device=DEV, dtype=F64), False)
    err = (got - ref).abs()
    print("LPIPS distance C = %d, %d px: worst error %.3e, bar %.3e (%.2f of the bar)"
          % (c, h * wd, float(err.max()), float(bar[err.argmax()]), float((err[bar > 0] / bar[bar > 0]).max())))
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bar).all()), (got, ref, bar)
    assert float(got[3]) == 0.0          # pixels of zero features in both images contribute exactly 0, not NaN
    if h * wd == 1:
        assert float(got[0]) == 0.0
    again = hip_distance(fd, wdv, n, h, wd, c, torch.full((n,), float("nan"), device=DEV, dtype=F64), False)
    assert torch.equal(got, again)
    base = torch.tensor([0.5, -1.25, 3.0, 7.0], dtype=F64)
    added = hip_distance(fd, wdv, n, h, wd, c, base.to(DEV), True)
    assert torch.equal(added, base + got)


# ------------------------------------------------------------------------------------------------ end to end
E2E_CASES = [(n, h, w) for n in (1, 3) for (h, w) in ((16, 16), (19, 21), (32, 24))]


def exact_01_images(seed, n, h, w):
    """[0, 1] images on the grid k / 256 (NHWC prediction, ground truth), for which 2 t - 1 and (g + 1) / 2 are exact in float32: the
    [0, 1] and the [-1, 1] forms then denote the same image to the bit."""
    rs = np.random.RandomState(seed)
    g = rs.randint(0, 257, size=(n, h, w, 3))
    p = np.clip(g + rs.randint(-40, 41, size=g.shape), 0, 256)
    return torch.from_numpy((p / 256.0).astype(np.float32)), torch.from_numpy((g / 256.0).astype(np.float32))


@pytest.mark.parametrize("n, h, w", E2E_CASES)
def test_end_to_end_against_fp64(model, weights, n, h, w):
    rs = np.random.RandomState(100 * n + h)
    g = torch.from_numpy(rs.uniform(-1.0, 1.0, size=(n, 3, h, w)).astype(np.float32))                  # the dataset's images
    p01 = ((g * 0.5 + 0.5).permute(0, 2, 3, 1) + torch.from_numpy(rs.standard_normal((n, h, w, 3)).astype(np.float32)) * 0.1).contiguous()
    x0 = lr.pm1_from_01(p01).permute(0, 3, 1, 2).contiguous()     # the prediction in [-1, 1] as the library forms it, float32
    ref, _, _ = lr.lpips(x0, g, *weights, dtype=F64)
    ref32, _, _ = lr.lpips(x0, g, *weights, dtype=F32)
    yard = float((ref32.to(F64) - ref).abs().max())
    views = pmetrics.lpips_views(model, p01.to(DEV), g.to(DEV), gt_layout="nchw_pm1")
    assert views.shape == (n,) and views.dtype == F64 and views.device.type == "cuda"
    got = views.cpu()
    err = float((got - ref).abs().max())
    print("LPIPS end to end %d x %d x %d: values %s, float32 restatement off by %.3e (the yardstick), kernel off by %.3e "
          "(%.2f yardsticks)" % (n, h, w, ["%.6f" % v for v in ref.tolist()], yard, err, err / yard if yard > 0 else float("inf")))
    assert bool(torch.isfinite(got).all()) and bool((got > 0).all())
    assert err <= E2E_FACTOR * yard, (err, yard)
    call = model(x0.to(DEV), g.to(DEV))                           # the same stored values in the package's form
    assert call.shape == (n, 1, 1, 1) and call.dtype == F32 and call.device.type == "cuda"
    assert torch.equal(call.cpu().reshape(n), got.to(F32))


def test_identical_pairs_give_exactly_zero(model):
    p, _ = exact_01_images(5, 3, 19, 21)
    pm1 = lr.pm1_from_01(p).permute(0, 3, 1, 2).contiguous()
    v = pmetrics.lpips_views(model, p.to(DEV), pm1.to(DEV), gt_layout="nchw_pm1").cpu()
    assert torch.equal(v, torch.zeros(3, dtype=F64))
    assert torch.equal(model(pm1.to(DEV), pm1.clone().to(DEV)).cpu(), torch.zeros(3, 1, 1, 1))


def test_batch_size_does_not_change_the_bits(model):
    p, g = exact_01_images(6, 5, 19, 21)
    a = pmetrics.lpips_views(model, p.to(DEV), g.to(DEV), batch_size=2).cpu()
    b = pmetrics.lpips_views(model, p.to(DEV), g.to(DEV), batch_size=5).cpu()
    c = pmetrics.lpips_views(model, p.to(DEV), g.to(DEV), batch_size=2).cpu()
    assert bool((a > 0).all()) and torch.equal(a, b) and torch.equal(a, c)
    # ... nor do the pairs that share the batch: each pair alone
    for i in range(5):
        assert torch.equal(pmetrics.lpips_views(model, p[i:i + 1].to(DEV), g[i:i + 1].to(DEV)).cpu(), a[i:i + 1])


# (layer, h, w, images of the small launch, of the large launch, the instantiations csrc/pny_lpips.h lpips_conv_variant gives them)
TILE_CASES = [(0, 64, 64, 2, 10, 111, 122),        # K = 36: never split; 128 tiles of 64 x 64 against 640
              (1, 64, 64, 2, 10, 811, 822),        # K = 576, a pair gives 512 tiles of 32 x 32: split at every batch
              (8, 16, 16, 2, 16, 811, 822),        # K = 4608 on 64 x 64 tiles
              (1, 128, 128, 1, 2, 111, 122)]       # K = 576, a pair gives 2048 tiles of 32 x 32: not split at any batch


@pytest.mark.parametrize("layer, h, w, n_small, n_large, v_small, v_large", TILE_CASES)
def test_tile_size_changes_no_bit_of_a_convolution(model, weights, layer, h, w, n_small, n_large, v_small, v_large):
    """The same images in a small and in a large launch of one VGG layer run 32 x 32 and 64 x 64 tiles (the tile size follows the
    configured batch), with the K split the layer and the image size alone decide: the results are bit-equal, and image 0 meets
    the forward-convolution bar against float64 under the 64 x 64 instantiations too."""
    cin, cout = lr.CHANNELS[layer]
    wt, b = weights[0][layer]
    x = torch.from_numpy(np.random.RandomState(1300 + layer + h).standard_normal((n_large, cin, h, w)).astype(np.float32))
    xl = x.permute(0, 2, 3, 1)
    if cin % 4:
        xl = torch.cat([xl, torch.zeros(n_large, h, w, 4 - cin % 4)], -1)
    xd = xl.contiguous().to(DEV)
    handle = model._ready(torch.device(DEV))
    outs, variants = [], []
    for n in (n_small, n_large):
        out = torch.full((n, h, w, cout), float("nan"), device=DEV)
        variant = C.c_int(0)
        plib.check(plib.load().pny_lpips_conv(handle, layer, plib.ptr(xd), n, h, w, plib.ptr(out), C.byref(variant), stream()))
        torch.cuda.synchronize()
        outs.append(out.cpu())
        variants.append(variant.value)
    assert variants == [v_small, v_large], variants
    assert torch.equal(outs[0], outs[1][:n_small])
    ref = Fn.relu(Fn.conv2d(x[:1].to(F64), wt.to(F64), b.to(F64), 1, 1))
    err = float((outs[1][:1].permute(0, 3, 1, 2).to(F64) - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    print("LPIPS conv%d at %d x %d: %d and %d images run instantiations %d and %d, bit-equal; error %.3e, bar %.3e"
          % (layer, h, w, n_small, n_large, variants[0], variants[1], err, CONV_FWD_BAR))
    assert err <= CONV_FWD_BAR, (err, CONV_FWD_BAR)


def test_batch_size_does_not_change_the_bits_where_the_tile_counts_differ(model, weights):
    """5 pairs of 64 x 64 at batch sizes 1, 2 and 5.  Chosen from the launch's own tile count, the instantiations would differ
    between these batches in the K split too (convolution 2, 128 channels at 32 x 32: 256 tiles of 32 x 32 for one pair, split;
    1280 for five, not split), and a split changes the order of every sum.  Here the split follows from one pair's tiles, and
    only the tile size differs (convolutions 0 and 1: 32 x 32 tiles at batch 1, 64 x 64 at batch 5).  The values must agree bit
    for bit, and meet the end-to-end bar against float64: 4 times the float32 restatement's largest deviation over the pairs."""
    rs = np.random.RandomState(64)
    g = torch.from_numpy(rs.uniform(0.0, 1.0, size=(5, 64, 64, 3)).astype(np.float32))
    p = (g + torch.from_numpy(rs.standard_normal((5, 64, 64, 3)).astype(np.float32)) * 0.1).contiguous()
    by_batch = {bs: pmetrics.lpips_views(model, p.to(DEV), g.to(DEV), batch_size=bs).cpu() for bs in (1, 2, 5)}
    assert torch.equal(by_batch[1], by_batch[5]) and torch.equal(by_batch[2], by_batch[5])
    x0, x1 = lr.pm1_from_01(p).permute(0, 3, 1, 2).contiguous(), lr.pm1_from_01(g).permute(0, 3, 1, 2).contiguous()
    ref, _, _ = lr.lpips(x0, x1, *weights, dtype=F64)
    ref32, _, _ = lr.lpips(x0, x1, *weights, dtype=F32)
    yard, err = float((ref32.to(F64) - ref).abs().max()), float((by_batch[5] - ref).abs().max())
    print("LPIPS 5 x 64 x 64 at batch sizes 1, 2, 5: bit-equal; float32 restatement off by %.3e (the yardstick), kernel off by %.3e "
          "(%.2f yardsticks)" % (yard, err, err / yard if yard > 0 else float("inf")))
    assert err <= E2E_FACTOR * yard, (err, yard)


def test_bytes_equal_the_bytes_over_255(model):
    rs = np.random.RandomState(8)
    p8 = torch.from_numpy(rs.randint(0, 256, size=(3, 32, 24, 3)).astype(np.uint8))
    g8 = torch.from_numpy(rs.randint(0, 256, size=(3, 32, 24, 3)).astype(np.uint8))
    from_bytes = pmetrics.lpips_views(model, p8.to(DEV), g8.to(DEV)).cpu()
    from_float = pmetrics.lpips_views(model, (p8.to(F32) / 255.0).to(DEV), (g8.to(F32) / 255.0).to(DEV)).cpu()
    assert bool((from_bytes > 0).all()) and torch.equal(from_bytes, from_float)
    mixed = pmetrics.lpips_views(model, (p8.to(F32) / 255.0).reshape(-1, 3).to(DEV), g8.to(DEV), H=32, W=24).cpu()
    assert torch.equal(from_bytes, mixed)


def test_call_equals_lpips_views(model):
    """On images of the grid k / 256 the [0, 1] form lpips_views takes and the [-1, 1] form __call__ takes are the same image
    to the bit, so the two entries must agree to the bit (up to __call__'s float32 result)."""
    p, g = exact_01_images(9, 3, 16, 16)
    p_pm1 = lr.pm1_from_01(p).permute(0, 3, 1, 2).contiguous()
    g_pm1 = lr.pm1_from_01(g).permute(0, 3, 1, 2).contiguous()
    views = pmetrics.lpips_views(model, p.to(DEV), g_pm1.to(DEV), gt_layout="nchw_pm1")
    call = model(p_pm1.to(DEV), g_pm1.to(DEV))
    assert torch.equal(call.reshape(3), views.to(F32))
    norm = model(p.permute(0, 3, 1, 2).contiguous().to(DEV), g.permute(0, 3, 1, 2).contiguous().to(DEV), normalize=True)
    assert torch.equal(norm, call)


def test_forward_refuses_what_it_cannot_run(model):
    handle = model._ready(torch.device(DEV))
    L = plib.load()
    x = torch.zeros(2, 16, 16, 3, device=DEV)
    work, out = torch.empty(1 << 20, device=DEV), torch.empty(2, device=DEV, dtype=F64)
    args = (C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()))
    d = desc_of(15, 16, "nhwc01", "nhwc01")
    assert L.pny_lpips_forward(handle, C.byref(d), *args, 2, plib.ptr(work), C.c_void_p(out.data_ptr()), stream()) == -1
    assert "at least 16" in L.pny_last_error().decode()
    d = desc_of(4096, 4096, "nhwc01", "nhwc01")
    assert L.pny_lpips_forward(handle, C.byref(d), *args, 1, plib.ptr(work), C.c_void_p(out.data_ptr()), stream()) == -1
    assert "32-bit" in L.pny_last_error().decode()
    d = desc_of(16, 16, "nhwc01", "nhwc01", batch=1)
    assert L.pny_lpips_forward(handle, C.byref(d), *args, 2, plib.ptr(work), C.c_void_p(out.data_ptr()), stream()) == -1
    assert "batch_size" in L.pny_last_error().decode()
