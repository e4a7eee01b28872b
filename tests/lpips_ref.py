"""
LPIPS v0.1 with net="vgg", normalize=False, spatial=False, restated from the published definition in plain torch; the
dtype is a parameter (float64: the yardstick; float32: the arithmetic the lpips package itself runs).  Every convolution is
torch.nn.functional.conv2d on the tensors as given, no shortcuts; the five taps are returned beside the value.

  scaling   (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
  features  torchvision's VGG-16 `features`: convolutions (3x3, pad 1, bias, relu) at 0, 2 | 5, 7 | 10, 12, 14 | 17, 19, 21 |
            24, 26, 28, max_pool2d(2, 2) in floor mode at 4, 9, 16, 23; taps behind relu 3, 8, 15, 22, 29
  per tap   f^ = f / (sqrt(sum_c f^2) + 1e-10);  sum_c w[c] (f^0[c] - f^1[c])^2;  mean over the tap's pixels
  value     the sum of the five taps
"""
import numpy as np
import torch
import torch.nn.functional as Fn

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # indices of the convolutions in vgg16().features
SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)                 # the lpips package's slice of each
POOL_BEFORE = (2, 4, 7, 10)                                     # convolutions (by position) that read a pooled tensor
TAP_AFTER = (1, 3, 6, 9, 12)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAP_CH = (64, 128, 256, 512, 512)
EPS = 1e-10


def weights_of(sd):
    """The lpips package's state dict (synth.vgg16_lpips_state) -> (convs [(w, b)] * 13, lins [w (C)] * 5) float32 tensors."""
    convs = [(torch.as_tensor(sd["net.slice%d.%d.weight" % (s, f)]), torch.as_tensor(sd["net.slice%d.%d.bias" % (s, f)]))
             for f, s in zip(FEATURES, SLICE)]
    lins = [torch.as_tensor(sd["lin%d.model.1.weight" % k]).reshape(-1) for k in range(5)]
    return convs, lins


def torchvision_state(sd):
    """The same weights under torchvision's names: features.{i}.weight / .bias, and the lin{k}.model.1.weight as they are."""
    out = {}
    for f, s in zip(FEATURES, SLICE):
        for p in ("weight", "bias"):
            out["features.%d.%s" % (f, p)] = sd["net.slice%d.%d.%s" % (s, f, p)]
    for k in range(5):
        out["lin%d.model.1.weight" % k] = sd["lin%d.model.1.weight" % k]
    return out


def scaling_layer(x, dtype):
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(x.device, dtype)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=torch.float32).to(x.device, dtype)[None, :, None, None]
    return (x.to(dtype) - shift) / scale


def vgg_taps(x, convs, dtype):
    """x (N, 3, H, W) behind the scaling layer -> the five taps (N, C_l, h_l, w_l)"""
    taps = []
    for i, (w, b) in enumerate(convs):
        if i in POOL_BEFORE:
            x = Fn.max_pool2d(x, 2, 2)
        x = Fn.relu(Fn.conv2d(x, w.to(dtype), b.to(dtype), stride=1, padding=1))
        if i in TAP_AFTER:
            taps.append(x)
    return taps


def normalize_tensor(f):
    return f / (torch.sqrt((f * f).sum(dim=1, keepdim=True)) + EPS)


def tap_distance(f0, f1, w):
    """(N, C, h, w) features of both images, w (C) -> (N): the weighted squared difference of the unit features, pixel mean"""
    d = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
    return (d * w.to(f0.dtype)[None, :, None, None]).sum(dim=1).mean(dim=(1, 2))


def lpips(x0, x1, convs, lins, dtype=torch.float64):
    """x0, x1 (N, 3, H, W) float32 in [-1, 1] -> (value (N), taps of x0, taps of x1), everything in `dtype`."""
    t0 = vgg_taps(scaling_layer(x0, dtype), convs, dtype)
    t1 = vgg_taps(scaling_layer(x1, dtype), convs, dtype)
    val = sum(tap_distance(a, b, w) for a, b, w in zip(t0, t1, lins))
    return val, t0, t1


def pm1_from_01(t):
    """float32 [0, 1] -> [-1, 1] as the library forms it: a separate multiply and subtract in float32"""
    return t.to(torch.float32) * 2.0 - 1.0


def pm1_from_bytes(b):
    return pm1_from_01(b.to(torch.float32) / 255.0)


def prepare(pm1_nchw):
    """float32 (n, 3, H, W) in [-1, 1] -> the library's prepared image (n, H, W, 4): scaling layer in float32, zero 4th channel"""
    y = scaling_layer(pm1_nchw, torch.float32).permute(0, 2, 3, 1)
    return torch.cat([y, torch.zeros_like(y[..., :1])], -1).contiguous()


def images(seed, n, h, w):
    """A pair of float32 (n, 3, h, w) image batches in [-1, 1]: uniform random ground truths and noisy copies of them."""
    rs = np.random.RandomState(seed)
    g = rs.uniform(-1.0, 1.0, size=(n, 3, h, w))
    p = np.clip(g + rs.standard_normal(g.shape) * 0.2, -1.0, 1.0)
    return torch.from_numpy(p.astype(np.float32)), torch.from_numpy(g.astype(np.float32))
