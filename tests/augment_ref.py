"""
The colour-jitter chain restated in float64 numpy, for tests/test_cpu_augment.py and tests/test_gpu_augment.py to compare the
kernel (csrc/augment.hip), its header (csrc/pny_augment.h) and the host chain (data.adjust_*) against.  Written from the
definitions (grey-level blends; the HSV hexcone model of Smith 1978 in its chroma form), not from data.py:

  t          (x + 1) / 2 of floats in [-1, 1], x / 255 of bytes
  grey       0.2989 r + 0.587 g + 0.114 b
  blend      clip(f a + (1 - f) b, 0, 1)
  chain      saturation: blend(t, grey, sat);  hue: h <- (h + hue) mod 1 in HSV;  contrast: blend(t, mean grey of the image,
             con);  brightness: blend(t, 0, bri);  out = 2 t - 1

Images are (..., 3, H, W) channel-first arrays; pixels for the per-pixel functions are (..., 3) with the channel last.
"""
import numpy as np

GREY = np.array([0.2989, 0.587, 0.114])


def from_pm1(x):
    return (np.asarray(x, np.float64) + 1.0) / 2.0


def from_bytes(x):
    """(..., H, W, 3) uint8 -> (..., 3, H, W) float64 in [0, 1]."""
    return np.moveaxis(np.asarray(x, np.float64) / 255.0, -1, -3)


def grey(px):
    return px[..., 0] * GREY[0] + px[..., 1] * GREY[1] + px[..., 2] * GREY[2]


def blend(a, b, f):
    return np.clip(f * a + (1.0 - f) * b, 0.0, 1.0)


def saturation(px, sat):
    return blend(px, grey(px)[..., None], sat)


def hue(px, shift):
    """Rotate the hue of (..., 3) pixels in [0, 1] by `shift` turns.  Hexcone model in its chroma form: value v = max and
    chroma c = max - min are kept, the hue -- sector offset 0 / 2 / 4 by the largest channel (r, g, b in that order on ties)
    plus a signed position d in [-1, 1] inside it, in sixths of a turn -- is moved by 6 shift, and the channels are
    v, v - c f, v - c (1 - f), v - c by the six-sector table (v s = c, so these are the p, q, t of the textbook form).  The
    sector and the fraction f are kept apart, so a shift of 0 returns the pixel to within a few units of 2^-53."""
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    v = px.max(-1)
    c = v - px.min(-1)
    cs = np.where(c == 0, 1.0, c)
    is_r, is_g = v == r, (v == g) & (v != r)
    off = np.where(is_r, 0, np.where(is_g, 2, 4))
    d = np.where(is_r, (g - b) / cs, np.where(is_g, (b - r) / cs, (r - g) / cs))
    y = d + 6.0 * shift
    k = np.floor(y)
    f = y - k
    sector = (off + k.astype(np.int64)) % 6
    p, q, t = (np.clip(x, 0.0, 1.0) for x in (v - c, v - c * f, v - c * (1.0 - f)))
    return np.stack([np.choose(sector, [v, q, p, p, t, v]), np.choose(sector, [t, v, v, q, p, p]),
                     np.choose(sector, [p, p, t, v, v, q])], -1)


def first(px, hue_f, sat):
    """Saturation then hue of (..., 3) pixels in [0, 1]."""
    return hue(saturation(px, sat), hue_f)


def second(px, mean, con, bri):
    """Contrast against `mean`, brightness, and the map to [-1, 1]."""
    return blend(blend(px, mean, con), 0.0, bri) * 2.0 - 1.0


def chain01(t, factors):
    """t (NV, 3, H, W) in [0, 1], one object's factors (hue, sat, bri, con) -> (NV, 3, H, W) in [-1, 1]; the contrast mean is
    per image."""
    hue_f, sat, bri, con = (float(v) for v in factors)
    px = first(np.moveaxis(np.asarray(t, np.float64), -3, -1), hue_f, sat)           # (NV, H, W, 3)
    mean = grey(px).mean(axis=(-2, -1))[..., None, None, None]
    return np.moveaxis(second(px, mean, con, bri), -1, -3)


def jitter(images, factors):
    """images (NV, 3, H, W) / (SB, NV, 3, H, W) floats in [-1, 1], or (NV, H, W, 3) / (SB, NV, H, W, 3) uint8; factors (4,) or
    (SB, 4) -> float64, channel-first, in [-1, 1]."""
    images = np.asarray(images)
    t = from_bytes(images) if images.dtype == np.uint8 else from_pm1(images)
    f = np.asarray(factors, np.float64)
    if t.ndim == 4:
        return chain01(t, f.reshape(4))
    assert f.shape == (t.shape[0], 4)
    return np.stack([chain01(t[o], f[o]) for o in range(t.shape[0])])


# ------------------------------------------------------------------ the error bar of the tests
FLOOR = 64 * 2.0 ** -24      # 32 rounded fp32 operations on values in [0, 1], doubled by the output map


def host_chain(images, factors):
    """The project's existing fp32 host chain (data.adjust_* in torch fp32 on the CPU, as ColorJitterDataset.apply_color_jitter
    runs it; bytes go through image_to_tensor_balanced first) on images / factors shaped as for `jitter` -> float32 numpy."""
    import torch
    from pixel_nerf_yolo_amd import data as pdata
    images = np.asarray(images)
    if images.dtype == np.uint8:
        flat = images.reshape((-1,) + images.shape[-3:])
        x = torch.stack([pdata.image_to_tensor_balanced(im) for im in flat]).reshape(images.shape[:-3] + (3,) + images.shape[-3:-1])
    else:
        x = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32))
    f = np.asarray(factors, np.float64)
    if x.dim() == 4:
        x, f = x[None], f.reshape(1, 4)
    out = torch.empty_like(x)
    for o in range(x.shape[0]):
        hue_f, sat, bri, con = (float(v) for v in f[o])
        for i in range(x.shape[1]):
            t = (x[o, i] + 1.0) * 0.5
            t = pdata.adjust_brightness(pdata.adjust_contrast(pdata.adjust_hue(pdata.adjust_saturation(t, sat), hue_f), con), bri)
            out[o, i] = t * 2.0 - 1.0
    return out.numpy()[0] if images.ndim == 4 else out.numpy()


def bar(images, factors, ref=None):
    """max(4 e_host, FLOOR) in output units, and e_host: the worst difference of the host chain from the restatement on
    these very inputs."""
    ref = jitter(images, factors) if ref is None else ref
    e_host = float(np.abs(host_chain(images, factors).astype(np.float64) - ref).max())
    return max(4.0 * e_host, FLOOR), e_host
