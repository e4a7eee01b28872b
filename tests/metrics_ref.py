"""
The reference's view metrics restated in fp64 (eval/eval.py:288-345: clamp, bytes, skimage's compare_ssim(multichannel=True,
data_range=1) and compare_psnr(data_range=1) per view).  skimage is not installed where the suite runs, so SSIM is written out
from its definition on the routine skimage itself calls, scipy.ndimage.uniform_filter: win_size 7, uniform window,
use_sample_covariance=True, K1 = 0.01, K2 = 0.03, the filtered map cropped by 3 pixels, channel by channel, then the mean
over the channels.  What the GPU tests compare the kernel against.
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7
NP = WIN * WIN
COV_NORM = NP / (NP - 1.0)
C1, C2 = 0.01 ** 2, 0.03 ** 2
PAD = (WIN - 1) // 2


def ssim_map(x, y, mode="reflect"):
    """S at every pixel of two 2-D fp64 images (skimage structural_similarity before its crop)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ux, uy = uniform_filter(x, size=WIN, mode=mode), uniform_filter(y, size=WIN, mode=mode)
    uxx, uyy, uxy = (uniform_filter(v, size=WIN, mode=mode) for v in (x * x, y * y, x * y))
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))


def ssim_channel(x, y, mode="reflect"):
    return float(ssim_map(x, y, mode)[PAD:-PAD, PAD:-PAD].mean(dtype=np.float64))


def ssim(x, y, mode="reflect"):
    """(H, W, 3) images -> the multichannel mean."""
    return float(np.mean([ssim_channel(x[..., ch], y[..., ch], mode) for ch in range(x.shape[-1])]))


def window_s(xw, yw):
    """S of one 7 x 7 window computed directly from its 49 pixel pairs (sums in fp64)."""
    xw, yw = np.asarray(xw, np.float64).reshape(-1), np.asarray(yw, np.float64).reshape(-1)
    assert xw.size == NP and yw.size == NP
    ux, uy = xw.sum() / NP, yw.sum() / NP
    vx, vy = COV_NORM * ((xw * xw).sum() / NP - ux * ux), COV_NORM * ((yw * yw).sum() / NP - uy * uy)
    vxy = COV_NORM * ((xw * yw).sum() / NP - ux * uy)
    return float(((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)))


def mse(x, y):
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return float(np.mean(d * d, dtype=np.float64))


def psnr_of_mse(m):
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(1.0 / np.float64(m)))


def clamp(rgb):
    """eval.py:288 on fp32."""
    return np.clip(np.asarray(rgb, np.float32), np.float32(0), np.float32(1))


def to_bytes(rgb):
    """eval.py:288-291: (clamp(rgb) * 255).astype(np.uint8) on fp32."""
    return (clamp(rgb) * np.float32(255)).astype(np.uint8)


def gt_from_pm1(images):
    """eval.py:315 on the dataset's (NV, 3, H, W) images in [-1, 1]: images * 0.5 + 0.5 in fp32, as (NV, H, W, 3)."""
    g = np.asarray(images, np.float32) * np.float32(0.5) + np.float32(0.5)
    return np.ascontiguousarray(g.transpose(0, 2, 3, 1))


def view_metrics(rgb, gt01):
    """(NV, H, W, 3) fp32 renders (unclamped) and ground truth in [0, 1] -> per view (mse, psnr, ssim) fp64 arrays."""
    x = clamp(rgb)
    m = np.array([mse(x[v], gt01[v]) for v in range(x.shape[0])])
    return m, np.array([psnr_of_mse(v) for v in m]), np.array([ssim(x[v], gt01[v]) for v in range(x.shape[0])])
