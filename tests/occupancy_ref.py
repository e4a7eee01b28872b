"""
csrc/pny_occupancy.h restated in numpy, line by line in meaning and not in form: the cells are built raw first and dilated by a
box maximum (the header walks a window of grid points per cell), the fused multiply-add is an exact double product, an
error-free double sum and one rounding (the header calls fmaf), the ranks are a cumulative sum (the kernels rank by ballots
and tile sums).  The CPU tests hold the header to this bit for bit, the GPU tests the kernels.
"""
import numpy as np

TILE = 1024          # samples per scan tile (pny_occupancy.h OCC_TILE)
MAX_DILATE = 4


def n_cells(dims):
    return (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)


def n_words(dims):
    return (n_cells(dims) + 31) >> 5


def cells_occupied(sigma, sigma2, thresh, dilate):
    """bool (X - 1, Y - 1, Z - 1): a corner is occupied when not (sigma <= thresh), in either volume; a cell when any of its 8
    corners is (raw), then when any cell within Chebyshev distance `dilate` is raw-occupied."""
    s = np.asarray(sigma, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        corner = ~(s <= np.float32(thresh))
        if sigma2 is not None:
            corner |= ~(np.asarray(sigma2, dtype=np.float32) <= np.float32(thresh))
    raw = np.zeros(tuple(d - 1 for d in s.shape), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                raw |= corner[dx:dx + raw.shape[0], dy:dy + raw.shape[1], dz:dz + raw.shape[2]]
    occ = raw
    for axis in range(3):          # a box maximum is separable
        cur = occ.copy()
        for k in range(1, dilate + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(k, None), slice(None, -k)
            if occ.shape[axis] > k:
                cur[tuple(hi)] |= occ[tuple(lo)]
                cur[tuple(lo)] |= occ[tuple(hi)]
        occ = cur
    return occ


def pack_bits(occ):
    """uint32 words: flat cell f (x slowest, z fastest) is bit f & 31 of word f >> 5; the padding bits are 0."""
    flat = occ.reshape(-1)
    padded = np.zeros(((flat.size + 31) // 32) * 32, dtype=np.uint64)
    padded[:flat.size] = flat
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def build(sigma, sigma2, thresh, dilate):
    """(bits uint32[words], number of occupied cells)"""
    occ = cells_occupied(sigma, sigma2, thresh, dilate)
    return pack_bits(occ), int(occ.sum())


def fmaf(a, b, c):
    """round_fp32(a * b + c) of fp32 arrays, rounded once: the product of two fp32 is exact in double; the double sum is
    made exact by its rounding error (TwoSum) and rounded to odd, after which the rounding to fp32 is the correct one."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        r = p + c
        bb = r - p
        err = (p - (r - bb)) + (c - bb)
        fix = np.isfinite(r) & np.isfinite(err) & (err != 0.0) & ((r.view(np.int64) & 1) == 0)
        toward = np.where(err > 0.0, np.inf, -np.inf)
        r = np.where(fix, np.nextafter(r, toward), r)
        return r.astype(np.float32)


def grid_axes(dims, c1, c2):
    cells = np.asarray(dims, dtype=np.int64) - 1
    lo = np.asarray(c1, dtype=np.float64).astype(np.float32)
    inv = (cells.astype(np.float64) / (np.asarray(c2, dtype=np.float64) - np.asarray(c1, dtype=np.float64))).astype(np.float32)
    return cells, lo, inv, cells.astype(np.float32)


def sample_cells(dims, c1, c2, rays, z):
    """int64 (n, K): the flat cell of every depth sample, -1 outside the grid (a NaN is outside)."""
    cells, lo, inv, hi = grid_axes(dims, c1, c2)
    rays, z = np.asarray(rays, dtype=np.float32), np.asarray(z, dtype=np.float32)
    inside = np.ones(z.shape, dtype=bool)
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            p = fmaf(z, rays[:, 3 + a:4 + a], rays[:, a:a + 1])
            q = (p - lo[a]).astype(np.float32)
            t = (q * inv[a]).astype(np.float32)
            ok = (t >= np.float32(0.0)) & (t < hi[a])
            inside &= ok
            idx.append(np.where(ok, t, np.float32(0.0)).astype(np.int64))
    flat = (idx[0] * cells[1] + idx[1]) * cells[2] + idx[2]
    return np.where(inside, flat, -1)


def keep_mask(bits, dims, c1, c2, outside_empty, rays, z):
    """bool (n, K): the samples a culled pass evaluates."""
    f = sample_cells(dims, c1, c2, rays, z)
    g = np.where(f >= 0, f, 0)
    bit = ((np.asarray(bits, dtype=np.uint32)[g >> 5] >> (g & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
    return np.where(f >= 0, bit, not outside_empty)


def slots(keep):
    """(int32 (n, K): the rank of a kept sample among the kept ones in ascending sample order, -1 for a rejected one; count)"""
    flat = keep.reshape(-1)
    rank = np.cumsum(flat) - 1
    return np.where(flat, rank, -1).astype(np.int32).reshape(keep.shape), int(flat.sum())


# --------------------------------------------------------------------------- the cases the CPU and the GPU tests share
VOLUMES = ((9, 7, 34), (2, 2, 2), (5, 5, 66))     # 8 x 6 x 33 = 1584 cells: z rows straddle words, the last word is half used
BOX = ((-1.0, -1.5, -0.5), (1.0, 0.5, 1.5))


def case_volume(dims, seed, two=False):
    """A random field (or a pair) with NaN, +inf and -inf entries; about a fifth of the corners above 0.8."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2 if two else 1):
        v = rng.random(dims, dtype=np.float32)
        flat = v.reshape(-1)
        n = flat.size
        for value, count in ((np.nan, max(n // 97, 1)), (np.inf, max(n // 131, 1)), (-np.inf, max(n // 61, 1))):
            if n > 8:
                flat[rng.choice(n, size=count, replace=False)] = value
        out.append(v)
    return out if two else out[0]


def thresholds():
    """a middling cut, one below every finite sigma and every -inf (all occupied), +inf (only NaN corners occupied)"""
    return (0.8, -np.inf, np.inf)


def case_rays(n, k, seed, dims=VOLUMES[0], box=BOX):
    """(rays (n, 8), z (n, k)) fp32: rays that cross, graze and miss the box; the first rows are the edge cases -- samples
    exactly on c1, on cell faces and on c2 along each axis, rays inside a face of the box (parallel to it), a NaN depth."""
    rng = np.random.default_rng(seed)
    c1, c2 = np.asarray(box[0]), np.asarray(box[1])
    centre, half = (c1 + c2) / 2, (c2 - c1) / 2
    rays = np.zeros((n, 8), dtype=np.float32)
    z = np.zeros((n, k), dtype=np.float32)
    row = 0
    for a in range(3):                      # along axis a from c1: depth j * (cell size) lands on face j, the last on c2
        step = (c2[a] - c1[a]) / (dims[a] - 1)
        for o in (c1.copy(), np.where(np.arange(3) == a, c1, centre)):
            d = np.zeros(3)
            d[a] = 1.0
            rays[row, :3], rays[row, 3:6] = o, d
            z[row] = (np.arange(k) * (dims[a] - 1) // (k - 1) if k > 1 else np.zeros(1)) * step
            row += 1
    for a in range(3):                      # inside the upper and the lower face of axis a, parallel to it
        for face in (c1, c2):
            o = centre - half * 1.25
            o[a] = face[a]
            d = np.ones(3) / np.sqrt(2.0)
            d[a] = 0.0
            rays[row, :3], rays[row, 3:6] = o, d
            z[row] = np.linspace(0.0, 4.0, k)
            row += 1
    first_random = row
    while row < n:
        o = centre + rng.normal(size=3) * 3.0
        target = centre + rng.uniform(-1.0, 1.0, size=3) * half * (1.0, 1.6, 3.0)[row % 3]     # cross, graze, miss
        d = target - o
        d /= np.linalg.norm(d)
        dist = np.linalg.norm(centre - o)
        rays[row, :3], rays[row, 3:6] = o, d
        z[row] = np.sort(rng.uniform(max(dist - 2.5, 0.05), dist + 2.5, size=k))
        row += 1
    rays[:, 6], rays[:, 7] = z.min(axis=1), z.max(axis=1)
    z[first_random, k // 2] = np.nan
    z[min(first_random + 1, n - 1), 0] = np.inf
    return rays, z


def scan_levels(n_samples):
    """How many levels of tile sums a classification of n_samples uses: 1 up to TILE * TILE samples, 2 above."""
    n1 = (n_samples + TILE - 1) // TILE
    return 2 if n1 > TILE else 1
