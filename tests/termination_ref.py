"""
csrc/pny_termination.h restated in numpy: the segment bounds, the transmittance in fp32 and the alive / kept sets of a pass.
The header multiplies a ray's factors one after the other and the kernel by a butterfly of shuffles; the restatement takes a
cumulative product.  The order of the multiplications is free, so the tests hold T to a bar (K * 2^-22) and the alive set exactly
only where T is clear of t_min.  The CPU tests hold the header to this, the GPU tests the kernels.
"""
import numpy as np

from occupancy_ref import slots  # noqa: F401  (the slot convention is the grid's: rank among the kept, ascending, or -1)

MAX_SEGMENTS = 16
EPS = np.float32(1e-10)


def bounds(K, S):
    """The S' + 1 first sample indices of the S' = min(S, K) segments of a pass with K samples per ray; the last is K."""
    sp = min(S, K)
    return [j * K // sp for j in range(sp + 1)]


def factors(rays, z, samp):
    """fp32 (n, K): 1 - alpha_k + 1e-10 with alpha_k = 1 - exp(-delta_k max(sigma_k, 0)), delta_k = z_{k+1} - z_k, the last
    delta reaching to the ray's far (rays column 7).  max is C's fmaxf: a NaN sigma counts as 0."""
    rays, z, samp = (np.asarray(v, dtype=np.float32) for v in (rays, z, samp))
    with np.errstate(invalid="ignore", over="ignore"):
        znext = np.concatenate([z[:, 1:], rays[:, 7:8]], axis=1)
        delta = (znext - z).astype(np.float32)
        sigma = np.fmax(samp[..., 3], np.float32(0.0))
        alpha = (np.float32(1.0) - np.exp((-delta * sigma).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return ((np.float32(1.0) - alpha).astype(np.float32) + EPS).astype(np.float32)


def transmittance(rays, z, samp):
    """fp32 (n, K + 1): T_b at every boundary b = 0 .. K, the product of the factors of the samples k < b; T_0 = 1."""
    f = factors(rays, z, samp)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([np.ones((f.shape[0], 1), dtype=np.float32), np.cumprod(f, axis=1, dtype=np.float32)], axis=1)


def alive_and_keep(rays, z, samp, t_min, S, grid_keep=None):
    """A pass of K samples per ray in S' = min(S, K) segments, `samp` (n, K, 4) being the MLP's output at every sample.
    -> alive bool (n, S'): the ray is alive in segment j; keep bool (n, K): the sample is evaluated; T fp32 (n, S' + 1): the
    transmittance of the MASKED samples at the segment bounds.  grid_keep bool (n, K) is the grid's verdict, None: no grid."""
    z = np.asarray(z, dtype=np.float32)
    samp = np.asarray(samp, dtype=np.float32)
    n, K = z.shape
    b = bounds(K, S)
    sp = len(b) - 1
    grid_keep = np.ones((n, K), dtype=bool) if grid_keep is None else np.asarray(grid_keep, dtype=bool)
    alive = np.zeros((n, sp), dtype=bool)
    keep = np.zeros((n, K), dtype=bool)
    T = np.ones((n, sp + 1), dtype=np.float32)
    now = np.ones(n, dtype=bool)
    f = factors(rays, z, samp)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(sp):
            alive[:, j] = now
            seg = slice(b[j], b[j + 1])
            keep[:, seg] = now[:, None] & grid_keep[:, seg]
            # a sample that is not kept has sigma = 0, alpha = 0 and a factor of 1 - 0 + 1e-10 = 1 in fp32
            fj = np.where(keep[:, seg], f[:, seg], np.float32(1.0))
            T[:, j + 1] = T[:, j] * np.prod(fj, axis=1, dtype=np.float32)
            now = now & ~(T[:, j + 1] < np.float32(t_min))
    return alive, keep, T


def clear_of_threshold(T, t_min, margin=1e-3):
    """bool (n): |T / t_min - 1| >= margin at every boundary BETWEEN two segments (where a ray's fate is decided); a NaN counts
    as clear (it keeps the ray alive whatever the rounding)."""
    inner = np.asarray(T, dtype=np.float64)[:, 1:-1]
    with np.errstate(invalid="ignore"):
        return ~(np.abs(inner / float(np.float32(t_min)) - 1.0) < margin).any(axis=1)
