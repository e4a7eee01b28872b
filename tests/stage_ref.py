"""
Inputs, bars and plain references of the stage-kernel and detection-tail sweeps (tests/test_cpu_stage_refs.py,
tests/test_gpu_stage_sweep.py).  The arbiter of every float result is oracle/pnyolo_oracle.py evaluated in float64 ON THE
FLOAT32 INPUTS; the arbiter of every index / integer result of the detection tail is the oracle's list restatement, exactly.

Bars.  Where an existing stage bar holds it is kept (tests/test_gpu_parity.py test_stage_kernels_vs_golden).  Everywhere else
the bar is TWICE the largest error of the oracle run in float32 on the CPU against its float64 run on the same inputs, with
the existing bar as the floor (the factor two: the kernels sum in another order than torch -- log-step scan, butterfly sums).
A stage without an existing bar (sample_coarse against float64, yolo_aggregate) has no floor: its bar is twice the float32
oracle's error and nothing else.  The float32-oracle error each constant came from is written beside it;
tests/test_cpu_stage_refs.py re-measures every one and asserts that it agrees with the recorded figure (at most 10 % above
it, not below half of it).  The kernels' own errors set nothing.
"""
import numpy as np
import torch

import pnyolo_oracle as orc

F32, F64 = torch.float32, torch.float64
N_LIST = (1, 3, 4, 5, 257)                      # 4 rays per workgroup: full groups, every tail, one ray
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))


def t32(x):
    return torch.as_tensor(np.asarray(x), dtype=F32).contiguous()


def as_dt(x, dtype):
    """The float32 VALUES of x in `dtype`: float64 arithmetic on float32 inputs."""
    return t32(x).to(dtype)


def err(a, b):
    """max |a - b| in float64 (both finite)."""
    a, b = torch.as_tensor(np.asarray(a), dtype=F64), torch.as_tensor(np.asarray(b), dtype=F64)
    return float((a - b).abs().max()) if a.numel() else 0.0


def make_rays(n, near, far, seed=0):
    rs = np.random.RandomState(1000 + seed)
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rs.randn(n, 3)
    d = rs.randn(n, 3)
    r[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 6], r[:, 7] = near, far
    return r


def near_far(lindisp):
    """lindisp: dyadic ends, so that 1 / (1 / near) is near itself and the range check is sharp at both ends."""
    return (0.5, 2.0) if lindisp else (0.8, 1.8)


def uniforms(rs, shape):
    return np.minimum(rs.rand(*shape).astype(np.float32), ONE_BELOW)      # rand() < 1 can round to 1.0f


# --------------------------------------------------------------------------- bars
# *_ERR32: the float32 oracle's largest error against the float64 oracle over every case of the sweep, measured on the CPU
# (tests/test_cpu_stage_refs.py measures it again: it must agree with the figure here to 10 % upwards -- torch's float32
# cumsum / sum may be vectorised otherwise on another build -- and must not fall below half of it).  The bars stay exactly
# twice the figures written here.
def _bar(floor, err32):
    return max(floor, 2.0 * err32)


COARSE_EXACT = (64, 0)                            # (kc, lindisp) of the existing `== 0.0` bar against the float32 reference
COARSE_ERR32 = 3.5e-7                             # kc to 1024, z in [0.5, 2]
COARSE_BAR = _bar(0.0, COARSE_ERR32)              # against float64 there is no earlier bar: twice the float32 oracle's error
COMPOSITE_ERR32_SMALL = 4.9e-7                     # K <= 96
COMPOSITE_BAR = _bar(2e-6, COMPOSITE_ERR32_SMALL)             # the existing bar (2e-6) at K <= 96
COMPOSITE_ERR32_LARGE = 6.1e-7                     # 96 < K <= 1000
COMPOSITE_BAR_LARGE = _bar(2e-6, COMPOSITE_ERR32_LARGE)
OPAQUE_ERR32 = 3.8e-7                              # weights behind an opaque sample TIMES 1e10 (order-one numbers again)
OPAQUE_SCALED_BAR = _bar(2e-6, OPAQUE_ERR32)      # the composite's bar on the rescaled weights
FINE_ERR32 = 6.3e-7                               # lindisp, all shapes to (1024, 512, 256), z in [0.5, 2] (lindisp off: 1.6e-7)
FINE_BAR = 1e-6                                   # the existing bar: lindisp off, every shape
FINE_BAR_LINDISP = _bar(1e-6, FINE_ERR32)         # 1 / (1 / near (1 - t) + 1 / far t): three more roundings, twice the error
AGG_ERR32 = 4.3e-7                                  # relative to max(1, max |ref|)
AGG_BAR = _bar(0.0, AGG_ERR32)                    # no earlier stage bar: twice the float32 oracle's error
BOX_ERR32 = 1.1e-7                                  # relative to max(1, max |finite ref|)
BOX_BAR = _bar(2e-6, BOX_ERR32)                   # the existing bar (2e-6)


def fine_bar(lindisp):
    return FINE_BAR_LINDISP if lindisp else FINE_BAR


def composite_bar(K):
    return COMPOSITE_BAR if K <= 96 else COMPOSITE_BAR_LARGE


# --------------------------------------------------------------------------- sample_coarse
COARSE_KC = (1, 2, 3, 63, 64, 65, 128, 1024)
COARSE_DRAWS = ("random", "zeros", "ones")


def coarse_case(n, kc, lindisp, draws, seed=0):
    near, far = near_far(lindisp)
    rays = make_rays(n, near, far, seed)
    if draws == "random":
        u = uniforms(np.random.RandomState(seed * 7 + kc), (n, kc))
    else:
        u = np.full((n, kc), 0.0 if draws == "zeros" else ONE_BELOW, np.float32)
    return rays, u


def coarse_ref(rays, kc, u, lindisp, dtype=F64):
    return orc.sample_coarse(as_dt(rays, dtype), kc, as_dt(u, dtype), bool(lindisp))


def rows_ascend_in_range(z, rays):
    z, rays = torch.as_tensor(z), torch.as_tensor(rays).to(z.dtype)
    up = bool((z[:, 1:] >= z[:, :-1]).all())
    return up and bool((z >= rays[:, 6:7]).all()) and bool((z <= rays[:, 7:8]).all())


# --------------------------------------------------------------------------- composite
COMPOSITE_K = (1, 2, 63, 64, 65, 96, 127, 128, 129, 192, 256, 1000)
NEAR, FAR = 0.8, 1.8


def opaque_positions(K):
    return sorted({i for i in (0, 62, 63, 64, 65, K - 2, K - 1) if 0 <= i < K})


def composite_families(K):
    return ["random", "zero_sigma", "neg_sigma", "z_last_far", "underflow"] + ["opaque@%d" % i for i in opaque_positions(K)]


def composite_case(family, n, K, seed=0):
    """rays (n, 8), z (n, K) ascending in (near, far) -- one jittered sample per stratum, every delta at least a quarter of a
    stratum, so that sigma = 1e6 is opaque whatever K -- and samp (n, K, 4) = [rgb in [0, 1], sigma]."""
    rs = np.random.RandomState(seed * 131 + K)
    rays = make_rays(n, NEAR, FAR, seed)
    t = (np.arange(K)[None, :] + 0.25 + 0.5 * rs.rand(n, K)) / K
    z = (NEAR + (FAR - NEAR) * t).astype(np.float32)
    samp = np.empty((n, K, 4), np.float32)
    samp[..., :3] = rs.rand(n, K, 3)
    sigma = rs.exponential(1.0, (n, K)) * K * 1.5 * rs.rand(n, 1)
    if family == "zero_sigma":
        sigma[:] = 0.0
    elif family == "neg_sigma":
        sigma = rs.randn(n, K) * K              # half of them negative: relu
    elif family == "z_last_far":
        z[:, -1] = FAR                          # last delta exactly 0
        sigma[:, -1] = 50.0 * K
    elif family == "underflow":
        sigma[:, 3:24:4] = 1e6                  # up to six opaque samples: T = 1e-60 -> 0 in float32 inside the first chunk
    elif family.startswith("opaque@"):
        i = int(family.split("@")[1])
        sigma[:] = K * (0.5 + rs.rand(n, K))    # alphas behind the opaque sample of order 1/2,
        sigma[:, :i] *= 0.002                   # in front of it of order 1e-3: it is reached with T of order one
        sigma[:, i] = 1e6
    else:
        assert family == "random", family
    samp[..., 3] = sigma
    return rays, z, samp


def composite_ref(rays, z, samp, white, dtype=F64):
    return orc.composite(as_dt(rays, dtype), as_dt(z, dtype), as_dt(samp, dtype), bool(white))


def behind(family, K):
    """Slice of the samples behind the opaque one (they see T = 1e-10 x ...), or None."""
    if not family.startswith("opaque@"):
        return None
    i = int(family.split("@")[1])
    return slice(i + 1, K) if i + 1 < K else None


# --------------------------------------------------------------------------- sample_fine
FINE_SHAPES = ((64, 32, 16), (64, 32, 0), (64, 32, 32), (1, 1, 0), (3, 5, 2), (63, 65, 1), (65, 63, 0), (128, 64, 32),
               (64, 0, 0), (1024, 512, 256))
FINE_REFUSED = (2048, 1024, 0)
FINE_PATTERNS = ("random", "zeros", "onehot", "bump")
DEPTH_STD = 0.01


def fine_weights(pattern, n, kc, rs):
    if pattern == "random":
        w = rs.rand(n, kc) ** 4
        w = 0.9 * w / w.sum(1, keepdims=True)
    elif pattern == "zeros":
        w = np.zeros((n, kc))
    elif pattern == "onehot":
        w = np.zeros((n, kc))
        w[np.arange(n), rs.randint(0, kc, n)] = 0.95
    else:
        assert pattern == "bump", pattern
        c, s = rs.rand(n, 1), 0.03 + 0.1 * rs.rand(n, 1)
        w = np.exp(-0.5 * (((np.arange(kc)[None, :] + 0.5) / kc - c) / s) ** 2)
        w = 0.8 * w / w.sum(1, keepdims=True)
    return w.astype(np.float32)


def cdf64(w):
    """The oracle's cdf (sample_fine) in float64 on float32 weights: (n, kc + 1), leading 0."""
    q = torch.as_tensor(np.asarray(w), dtype=F64) + 1e-5
    c = torch.cumsum(q / q.sum(-1, keepdim=True), -1)
    return torch.cat([torch.zeros_like(c[:, :1]), c], -1).numpy()


def cdf32_sequential(w):
    """The same cdf in float32, every sum in index order, one rounding per operation."""
    q = np.asarray(w, np.float32) + np.float32(1e-5)
    tot = np.zeros(q.shape[0], np.float32)
    for k in range(q.shape[1]):
        tot = tot + q[:, k]
    q = q / tot[:, None]
    c = np.zeros((q.shape[0], q.shape[1] + 1), np.float32)
    for k in range(q.shape[1]):
        c[:, k + 1] = c[:, k] + q[:, k]
    assert c.dtype == np.float32
    return c


def condition_draws(w, u):
    """Importance draws that no float32 evaluation can put into another bin than the float64 reference does: every draw within
    `margin` of an edge of the float64 cdf moves to the middle of its bin, or -- where that bin is narrower than 2.5 margins --
    to the middle of the ray's widest bin.  margin = 4 x max |sequential float32 cdf - float64 cdf| over the case.
    Returns (u', margin, number of draws moved)."""
    u = np.array(u, np.float32)
    if u.size == 0:
        return u, 0.0, 0
    c = cdf64(w)
    margin = 4.0 * float(np.abs(cdf32_sequential(w).astype(np.float64) - c).max())
    moved = 0
    for r in range(u.shape[0]):
        edges = c[r]
        width = np.diff(edges)
        wide = int(np.argmax(width))
        assert width[wide] > 2.5 * margin
        b = np.clip(np.searchsorted(edges, u[r].astype(np.float64), side="right") - 1, 0, len(width) - 1)
        dist = np.minimum(np.abs(u[r] - edges[b]), np.abs(edges[b + 1] - u[r]))
        dist = np.where(b == 0, np.abs(edges[1] - u[r]), dist)             # the edge at 0 cannot flip (u >= 0, clamp to bin 0)
        for i in np.nonzero(dist <= margin)[0]:
            bb = b[i] if width[b[i]] > 2.5 * margin else wide
            u[r, i] = np.float32(0.5 * (edges[bb] + edges[bb + 1]))
            moved += 1
    return u, margin, moved


def edge_distance(w, u):
    """Smallest distance of a draw to an interior or upper edge of the float64 cdf (the quantity condition_draws bounds)."""
    if np.asarray(u).size == 0:
        return np.inf
    c = cdf64(w)
    d = np.abs(np.asarray(u, np.float64)[:, :, None] - c[:, None, 1:])
    return float(d.min())


def fine_case(n, kc, kf, kfd, lindisp, pattern, seed=0):
    """Inputs of one pny_sample_fine call, importance draws conditioned.  dict of float32 arrays (+ margin, moved)."""
    near, far = near_far(lindisp)
    rs = np.random.RandomState(seed * 977 + kc * 7 + kf * 3 + kfd + 31 * lindisp + FINE_PATTERNS.index(pattern))
    rays = make_rays(n, near, far, seed)
    zc = coarse_ref(rays, kc, uniforms(rs, (n, kc)), lindisp, F32)
    zc = torch.sort(zc, -1)[0].numpy()                  # the kernel's precondition: ascending coarse depths
    w = fine_weights(pattern, n, kc, rs)
    kimp = kf - kfd
    u, margin, moved = condition_draws(w, uniforms(rs, (n, kimp)))
    u2 = uniforms(rs, (n, kimp))
    depth = (near + (far - near) * rs.rand(n)).astype(np.float32)
    g = rs.randn(n, kfd).astype(np.float32)
    return dict(rays=rays, zc=zc, w=w, depth=depth, u=u, u2=u2, g=g, margin=margin, moved=moved)


def fine_ref(c, kc, kf, kfd, lindisp, dtype=F64, depth_std=DEPTH_STD):
    """sort(cat(coarse, importance, depth samples)) as orc.render forms it."""
    rays = as_dt(c["rays"], dtype)
    parts = [as_dt(c["zc"], dtype)]
    if kf - kfd > 0:
        parts.append(orc.sample_fine(rays, as_dt(c["w"], dtype), as_dt(c["u"], dtype), as_dt(c["u2"], dtype), kc, bool(lindisp)))
    if kfd > 0:
        parts.append(orc.sample_fine_depth(rays, as_dt(c["depth"], dtype), as_dt(c["g"], dtype), depth_std))
    return torch.sort(torch.cat(parts, -1), -1)[0]


def hip_fine(c, kc, kf, kfd, lindisp, depth_std=DEPTH_STD, device="cuda:0", seed=0):
    """pny_sample_fine on a case of fine_case / dyadic_case / depth_tie_case (GPU; the one place that marshals its arguments,
    for the sweep and for its two-device child process).  An absent draw array is drawn from `seed`.  Returns the merged depths (n, kc + kf) on
    the CPU."""
    from pixel_nerf_yolo_amd import lib as plib
    t = {k: torch.as_tensor(c[k], dtype=F32, device=device).contiguous() for k in ("rays", "zc", "w", "depth", "u", "u2", "g")}
    opt = lambda v: plib.ptr(v) if v.numel() else None          # noqa: E731  (NULL for an absent draw array)
    n = t["rays"].shape[0]
    zo = torch.full((n, kc + kf), float("nan"), device=device)
    plib.check(plib.load().pny_sample_fine(plib.ptr(t["rays"]), plib.ptr(t["zc"]), plib.ptr(t["w"]), plib.ptr(t["depth"]), n, kc,
                                           kf, kfd, depth_std, lindisp, opt(t["u"]), opt(t["u2"]), opt(t["g"]), seed,
                                           plib.ptr(zo), plib.stream_of(torch.device(device))))
    torch.cuda.synchronize(device)
    return zo.cpu()


def contains_rows(out, zc):
    """Every coarse depth of a row appears in the row of merged depths, bit for bit."""
    out, zc = np.asarray(out), np.asarray(zc)
    return all(bool(np.isin(zc[r], out[r]).all()) for r in range(out.shape[0]))


def dyadic_weights(kind):
    """Weights whose cdf has the same bits under every summation order: w = fl32(2^-k - 1e-5f), so that fl32(w + 1e-5f) = 2^-k
    exactly, every partial sum is dyadic, and the total is 1.  Returns (weights (kc,), the bins' widths as exponents k)."""
    ks = {"eq4": [2] * 4, "eq16": [4] * 16, "eq64": [6] * 64, "mix": [1, 2, 3, 3]}[kind]
    e = np.float32(1e-5)
    w = np.array([np.float32(np.float32(2.0) ** -k) - e for k in ks], np.float32)
    return w, ks


def dyadic_case(kind, u2_value, lindisp, n=5, seed=0):
    """Draws exactly on the cdf's edges: 0, every interior edge, the largest float below 1; coarse draws 0, so that with
    u2 = 0 (and lindisp off) a new depth also TIES with a coarse depth.  expected_bin per draw: bin 0; the UPPER bin of an
    interior edge (right=True); the last bin."""
    w1, ks = dyadic_weights(kind)
    kc = len(ks)
    edges = np.concatenate([[0.0], np.cumsum([2.0 ** -k for k in ks])])
    u1 = np.array(list(edges[:-1]) + [ONE_BELOW], np.float32)
    assert np.array_equal(u1[:-1].astype(np.float64), edges[:-1])             # the edges are float32 numbers
    bins = np.array(list(range(kc)) + [kc - 1])
    near, far = near_far(lindisp)
    rays = make_rays(n, near, far, seed)
    zc = coarse_ref(rays, kc, np.zeros((n, kc), np.float32), lindisp, F32).numpy()
    assert bool((zc[:, 1:] >= zc[:, :-1]).all())
    c = dict(rays=rays, zc=zc, w=np.tile(w1, (n, 1)), depth=np.zeros(n, np.float32), u=np.tile(u1, (n, 1)),
             u2=np.full((n, len(u1)), u2_value, np.float32), g=np.zeros((n, 0), np.float32), margin=0.0, moved=0)
    return c, kc, len(u1), bins


def depth_tie_case(kind, n=5, kc=64, kf=32, kfd=16, seed=0):
    """Equal new depths / a new depth equal to a coarse depth: `std0` (depth_std = 0: all depth samples equal), `clamp`
    (|g| huge: all at near or far), `coarse_bits` (depth = a coarse depth's bits, g = 0).  Returns (case, depth_std)."""
    c = fine_case(n, kc, kf, kfd, 0, "random", seed + 5)
    std = DEPTH_STD
    if kind == "std0":
        std = 0.0
    elif kind == "clamp":
        sign = np.where(np.arange(n)[:, None] % 2 == 0, 1.0, -1.0)
        c["g"] = (sign * np.full((n, kfd), 1e30)).astype(np.float32)
    else:
        assert kind == "coarse_bits", kind
        c["depth"] = c["zc"][np.arange(n), (np.arange(n) * 13) % kc].copy()
        c["g"] = np.zeros((n, kfd), np.float32)
    return c, std


# --------------------------------------------------------------------------- yolo_aggregate
AGG_K = (1, 63, 64, 65, 128, 200)
AGG_ANCHORS = (1, 2, 3, 4, 5)


def agg_families(K):
    return ["random", "all_low", "all_high"] + ["peak@%d" % i for i in sorted({0, 63, 64, K - 1}) if 0 <= i < K]


def agg_case(family, n, K, na, seed=0):
    rs = np.random.RandomState(seed * 17 + K * 5 + na)
    raw = rs.randn(n, K, na, 7).astype(np.float32)
    if family == "all_low":
        raw[..., 0] = -100.0                    # sum p ~ 0: the 1e-5 dominates
    elif family == "all_high":
        raw[..., 0] = 100.0
    elif family.startswith("peak@"):
        raw[..., 0] = -20.0
        raw[:, int(family.split("@")[1]), :, 0] = 20.0
    else:
        assert family == "random", family
        raw[..., 0] *= 3.0
    return raw.reshape(n, K, na * 7)


def agg_ref(raw, na, dtype=F64):
    return orc.yolo_aggregate(as_dt(raw, dtype), na)


def agg_scale(ref):
    return max(1.0, float(torch.as_tensor(ref).abs().max()))


# --------------------------------------------------------------------------- detection tail: cells -> boxes
CELL_SHAPES = ((1, 1, 1), (7, 5, 4), (5, 7, 2), (64, 64, 2))
ANCHORS = np.array([[8.4, 3.52], [11.4, 7.68], [27.0, 12.48], [2.0, 30.0]], np.float32)


def cells_case(h, w, A, is_pred, family, seed=0, batch=2):
    rs = np.random.RandomState(seed * 19 + h * 64 + w * 8 + A + 2 * int(is_pred))
    c = rs.randn(batch, h, w, A, 7 if is_pred else 6).astype(np.float32)
    if not is_pred:
        c[..., 1:5] = rs.rand(batch, h, w, A, 4)
        c[..., 5] = rs.randint(0, 2, (batch, h, w, A))
    if family == "class_ties" and is_pred:
        c[..., 5:] = np.round(c[..., 5:])               # many equal class logits: the first maximum wins
        c[0, ..., 6] = c[0, ..., 5]                     # and a whole image of exact ties
    elif family == "extreme" and is_pred:
        sel = rs.rand(batch, h, w, A, 4)
        c[..., 1:5] = np.where(sel < 0.3, 90.0, np.where(sel < 0.6, -90.0, c[..., 1:5]))
        c.reshape(-1, 7)[0, 1:5] = (90.0, -90.0, 90.0, -90.0)
    return c


def cells_ref(cells, anchors, h, w, is_pred, dtype=F64):
    """reference src/util/util.py:633-689 for one image in `dtype` (orc.cells_to_bboxes is float32 only; the CPU test holds
    this to it bit for bit at float32)."""
    c = as_dt(cells, dtype)
    A = c.shape[2]
    box = c[..., 1:5].clone()
    if is_pred:
        box[..., 0:2] = torch.sigmoid(box[..., 0:2])
        box[..., 2:] = torch.exp(box[..., 2:]) * as_dt(anchors, dtype).reshape(1, 1, A, 2)
        cls = torch.argmax(c[..., 5:], dim=-1).unsqueeze(-1).to(dtype)
    else:
        cls = c[..., 5:6]
    cx = torch.arange(w, dtype=dtype).reshape(1, w, 1, 1).expand(h, w, A, 1)
    cy = torch.arange(h, dtype=dtype).reshape(h, 1, 1, 1).expand(h, w, A, 1)
    x = (1 / w) * (box[..., 0:1] + cx)
    y = (1 / h) * (box[..., 1:2] + cy)
    wh = 1 / torch.tensor([w, h], dtype=dtype) * box[..., 2:4]
    return torch.cat((cls, c[..., 0:1], x, y, wh), dim=-1).reshape(h * w * A, 6)


def check_boxes(got, ref64, ref32):
    """got against the float64 boxes where the float32 reference is finite (bar x max(1, max |finite|)); where the float32
    reference overflows (exp(90)) got must be non-finite with the same sign.  Returns the largest finite error / scale."""
    got, ref64, ref32 = (np.asarray(torch.as_tensor(v).cpu(), np.float64) for v in (got, ref64, ref32))
    fin = np.isfinite(ref32)
    assert np.array_equal(np.isfinite(got), fin), "non-finite boxes at other positions than the reference's"
    assert np.array_equal(np.sign(got[~fin]), np.sign(ref32[~fin])) and not np.isnan(got).any()
    scale = max(1.0, float(np.abs(ref64[fin]).max()))
    e = float(np.abs(got[fin] - ref64[fin]).max()) / scale
    return e


# --------------------------------------------------------------------------- detection tail: nms
def iou_rows(first, rows):
    """orc.iou_xywh(first, row) for every row at once: numpy float32, the same operations in the same order."""
    f = np.float32
    a = np.asarray(first, f)
    b = np.asarray(rows, f).reshape(-1, 4)
    two, zero = f(2.0), f(0.0)
    ax1, ay1, ax2, ay2 = a[0] - a[2] / two, a[1] - a[3] / two, a[0] + a[2] / two, a[1] + a[3] / two
    bx1, by1, bx2, by2 = b[:, 0] - b[:, 2] / two, b[:, 1] - b[:, 3] / two, b[:, 0] + b[:, 2] / two, b[:, 1] + b[:, 3] / two
    inter = np.maximum(np.minimum(ax2, bx2) - np.maximum(ax1, bx1), zero) * np.maximum(np.minimum(ay2, by2) - np.maximum(ay1, by1), zero)
    union = np.abs((ax2 - ax1) * (ay2 - ay1)) + np.abs((bx2 - bx1) * (by2 - by1)) - inter
    out = inter / (union + f(1e-6))
    assert out.dtype == np.float32
    return out


def _filter_sort(b, threshold):
    conf = b[:, 1].astype(np.float64)
    ok = conf > threshold
    above = int(ok.sum())
    bw, bh = b[:, 4].astype(np.float64), b[:, 5].astype(np.float64)
    ok &= (10e-4 < bw) & (bw < 10e4) & (10e-4 < bh) & (bh < 10e4)
    idx = np.nonzero(ok)[0]
    return idx[np.argsort(-b[idx, 1], kind="stable")], float(conf.max()), above


def nms_fast(boxes, iou_threshold, threshold, skip=True):
    """orc.nms restated with ONE vectorised float32 IoU per round followed by the same index walk: removing from the list under
    the iterator skips the element after a removed one, and `list.remove` deletes the FIRST equal row.
    skip=False: textbook NMS (every row above the IoU threshold goes) -- the control the clustered case is held against.
    Returns (kept rows (m, 6) float32, highest confidence, above-threshold count)."""
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 6))
    order, highest, above = _filter_sort(b, threshold)
    _, gid, cnt = np.unique(b, axis=0, return_inverse=True, return_counts=True)
    gid = gid.reshape(-1)
    twins = cnt[gid] > 1
    thr32 = np.float32(iou_threshold)
    lst = [int(i) for i in order]
    kept = []
    while lst:
        first = lst.pop(0)
        kept.append(first)
        if not lst:
            break
        sup = iou_rows(b[first, 2:], b[lst, 2:]) > thr32
        if not skip:
            lst = [r for r, s in zip(lst, sup) if not s]
            continue
        sup = dict(zip(lst, sup.tolist()))                 # row index -> above the threshold (rows are distinct indices)
        i = 0
        while i < len(lst):
            r = lst[i]
            if sup[r]:
                j = i
                if twins[r]:
                    j = next(k for k in range(i + 1) if gid[lst[k]] == gid[r])
                del lst[j]
            i += 1
    return b[kept].reshape(-1, 6), highest, above


def tp_fp_fn_fast(targets, preds, nms_iou, nms_t, match_iou):
    """orc.tp_fp_fn with nms_fast swapped in and the IoU maxima vectorised."""
    t, _, _ = nms_fast(targets, nms_iou, nms_t)
    p, _, _ = nms_fast(preds, nms_iou, nms_t)
    if len(t) == 0:
        return 0, len(p), 0
    if len(p) == 0:
        return 0, 0, len(t)
    m32 = np.float32(match_iou)
    best_p = np.array([iou_rows(pb[2:], t[:, 2:]).max() for pb in p], np.float32)
    best_t = np.array([iou_rows(tb[2:], p[:, 2:]).max() for tb in t], np.float32)
    tp = int((best_p > m32).sum())
    return tp, len(p) - tp, int((best_t < m32).sum())


def _boxes(rs, n, conf=None, size=(0.02, 0.2)):
    b = np.empty((n, 6), np.float32)
    b[:, 0] = rs.randint(0, 3, n)
    b[:, 1] = rs.rand(n) if conf is None else conf
    b[:, 2:4] = rs.rand(n, 2)
    b[:, 4:6] = size[0] + (size[1] - size[0]) * rs.rand(n, 2)
    return b


def clustered_boxes(n, n_clusters, seed=0, jitter=0.01):
    """n boxes around n_clusters centres on a grid (heavy suppression: the survivors stay a small multiple of the clusters)."""
    rs = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(n_clusters)))
    k = rs.randint(0, n_clusters, n)
    b = _boxes(rs, n)
    b[:, 2] = ((k % side) + 0.5) / side + jitter / side * rs.randn(n)
    b[:, 3] = ((k // side) + 0.5) / side + jitter / side * rs.randn(n)
    b[:, 4:6] = (0.5 / side) * (1.0 + 0.2 * rs.rand(n, 2))
    return b.astype(np.float32)


NMS_N = (1, 2, 255, 256, 257, 511, 512, 513, 4097, 8192)
NMS_MAX = 8192


def nms_cases():
    """name -> (boxes (n, 6) float32, iou threshold, confidence threshold).  Small enough for orc.nms except the sizes above
    1000 (nms_fast only, proven equal on the others)."""
    rs = np.random.RandomState(77)
    cases = {}
    for n in NMS_N:
        if n <= 513:
            cases["uniform%d" % n] = (_boxes(rs, n), 0.3, 0.2)
        cases["cluster%d" % n] = (clustered_boxes(n, max(1, min(100, n // 8)), seed=n), 0.5, 0.1)
    # uniform above 513 too: 3328 rows pass the filters and 904 DISTINCT rows survive, spread over the whole sorted list (rank
    # sort and compaction across many thread strides); nms_fast takes 0.4 s on it.  A generator of its own, so that the
    # cases below keep their draws.  At 8192 the survivor count is kept moderate by clustering alone.
    cases["uniform4097"] = (_boxes(np.random.RandomState(4097), 4097), 0.3, 0.2)
    cases["equal_conf600"] = (_boxes(rs, 600, conf=0.7, size=(0.05, 0.3)), 0.3, 0.5)
    d = clustered_boxes(120, 6, seed=3)
    rep = np.array([(2, 3, 5)[i % 3] for i in range(120)])
    d = np.repeat(d, rep, axis=0)                            # exact duplicate rows in runs of 2, 3 and 5
    d[:, 1] = np.repeat(np.round(rs.rand(120) * 8) / 8 * 0.5 + 0.3, rep)    # and equal confidences across different rows
    d = np.concatenate([d, d[::4]])                          # and twins apart, rows of the same confidence between them
    cases["duplicates"] = (d.astype(np.float32), 0.4, 0.2)
    c = np.repeat(clustered_boxes(60, 4, seed=4), 3, axis=0)
    c[:, 0] = np.tile([0, 1, 2], 60)                         # rows equal except for the class: NOT twins
    cases["class_only"] = (c.astype(np.float32), 0.4, 0.2)
    cases["below_conf"] = (_boxes(rs, 300, conf=0.1 * rs.rand(300)), 0.5, 0.5)
    s = _boxes(rs, 300)
    s[::2, 4] = 5e-4
    s[1::2, 5] = 2e5
    cases["size_filtered"] = (s, 0.5, 0.0)
    e = _boxes(rs, 64)
    e[:32, 1] = np.float32(0.3)          # 0.3f = 0.300000011920929 > 0.3: passes the double comparison
    e[32:, 1] = np.float32(0.25)         # below
    e[:16, 4] = np.float32(1e-3)         # fl32(1e-3) = 0.00100000004749745 > 10e-4: passes
    e[16:32, 5] = np.float32(1e-3)
    cases["threshold_edges"] = (e, 0.5, 0.3)
    return cases


def iou_pair_case():
    """Two boxes and their exact float32 IoU: with the threshold AT it the second survives (strict >), with the next float
    below it is suppressed."""
    b = np.array([[0, 0.9, 0.5, 0.5, 0.3, 0.2], [0, 0.8, 0.55, 0.52, 0.28, 0.22]], np.float32)
    v = np.float32(orc.iou_xywh(b[0, 2:], b[1, 2:]))
    return b, float(v), float(np.nextafter(v, np.float32(0)))


def match_cases():
    """name -> (targets, predictions, nms_iou, nms_t, match_iou) for tp / fp / fn."""
    rs = np.random.RandomState(99)
    low = lambda n: _boxes(rs, n, conf=0.05 * rs.rand(n))       # noqa: E731  (nothing survives a 0.5 threshold)
    cases = {
        "targets_empty": (low(50), _boxes(rs, 200), 0.5, 0.5, 0.2),
        "preds_empty": (_boxes(rs, 200), low(50), 0.5, 0.5, 0.2),
        "both_empty": (low(20), low(30), 0.5, 0.5, 0.2),
        "many_targets": (_boxes(rs, 900, size=(0.01, 0.03)), _boxes(rs, 120), 0.5, 0.1, 0.2),
        "many_preds": (_boxes(rs, 120), _boxes(rs, 900, size=(0.01, 0.03)), 0.5, 0.1, 0.2),
        "clustered": (clustered_boxes(300, 20, seed=8), clustered_boxes(400, 20, seed=9), 0.5, 0.1, 0.3),
    }
    b, v, _ = iou_pair_case()
    cases["iou_equals_match"] = (b[:1], b[1:], 0.5, 0.1, v)     # best IoU == match_iou: no true positive, no false negative
    return cases


# =========================================================================== backward stages (csrc/mlp_bwd.hip)
# The MLP-free reverses of the stages above, through their own entry points: pny_composite_backward,
# pny_yolo_aggregate_backward (float: the oracle under autograd in float64 on the float32 inputs), pny_depth_grad_gather and
# pny_locate_depth_samples (exact: a host restatement).
#
# Error measure of the two float stages, PER ROW -- a ray for the composite, a (ray, anchor) for the aggregation:
# max |got - ref| over the row / max |ref| over the row.  One row's error is not hidden behind another row's larger gradient,
# which the whole-tensor measure of test_composite_backward_vs_autograd allows.  A row whose reference maximum is below TINY
# (sigma == 0, all_low: gradients <= 5e-38, subnormal, which a GPU may flush) is checked absolutely: finite and <= TINY.
TINY = 1e-30


def row_err(got, ref, n):
    """Largest per-row relative error of got against ref, rows = the leading n entries (see above).  Asserts that got is
    finite, and that the rows whose reference stays below TINY stay below TINY."""
    g = torch.as_tensor(np.asarray(got), dtype=F64).reshape(n, -1)
    r = torch.as_tensor(np.asarray(ref), dtype=F64).reshape(n, -1)
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), "non-finite gradient"
    if g.shape[1] == 0:
        return 0.0
    top = r.abs().max(1)[0]
    small = top < TINY
    if bool(small.any()):
        assert float(g[small].abs().max()) <= TINY, "a row whose reference is below %g holds %.3e" % (TINY, float(g[small].abs().max()))
    if bool(small.all()):
        return 0.0
    return float(((g - r).abs().max(1)[0][~small] / top[~small]).max())


def _seed_of(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


# --------------------------------------------------------------------------- composite backward
# Inputs: composite_bwd_case = composite_case, every family, with sigma x delta either SMALL (at most X_CAP) or 1e6 (the planted
# opaque samples: alpha == 1 and A == 1e-10 in both precisions).  The opacities in between are EXCLUDED on purpose, and
# composite_case's exponential draws do reach them (sigma x delta to 28 at n = 257).  alpha = 1 - exp(-x) is rounded to float32
# with an absolute error of 6e-8, so A = 1 - alpha + 1e-10 = exp(-x) carries a RELATIVE error of 6e-8 exp(x): 3e-6 at x = 4,
# 2e-4 at x = 8, 1e-2 at x = 12, and from x = 15 to 25 A is one of 1e-10, 6e-8, 1.2e-7 whatever x is.  excl / A inherits that
# factor in every float32 evaluation, the oracle's included.  Under the whole-tensor measure a small T hides it; per ray it
# does not where such a sample comes FIRST on its ray (T = 1) and makes every gradient of the row tiny: the float32 oracle is
# then 1.7e-3 off the float64 one (x = 12.3 at sample 0, row maximum 1e-7; K = 64, n = 4).  No float32 implementation can be
# held to float64 there, so the sweep does not ask it.
X_CAP = 4.0


def composite_bwd_case(family, n, K, seed=0):
    """composite_case with every sigma x delta above X_CAP brought down to X_CAP, the planted 1e6 excepted."""
    rays, z, samp = composite_case(family, n, K, seed)
    delta = np.diff(np.concatenate([z, rays[:, 7:8]], 1).astype(np.float64), axis=1)
    sigma = samp[..., 3].astype(np.float64)
    high = (sigma < 1e5) & (sigma * delta > X_CAP)
    samp[..., 3] = np.where(high, X_CAP / np.where(high, delta, 1.0), sigma).astype(np.float32)
    return rays, z, samp


COMPOSITE_BWD_KMAX = 2048                                  # 4 rays x 2 arrays x K floats of LDS = 64 KB: the largest K accepted
COMPOSITE_BWD_K = COMPOSITE_K + (COMPOSITE_BWD_KMAX,)
COMPOSITE_BWD_FLOOR = 2e-5                                 # test_composite_backward_vs_autograd (there: of the whole tensor's max)
# float32 oracle under autograd against the float64 one, per ray, over every case of the sweep (n to 257, white 0 and 1, the
# gradient subsets included).  d_z of a ray with one or two samples is one or two numbers, each a difference of two terms
# (g_depth w_k - dL/ddelta_k [+ dL/ddelta_k-1]) that nearly cancel on a few of 257 rays: the float32 oracle itself is 3.7e-4
# off there, and those K get the bar that belongs to them instead of lending it to every K.
COMPOSITE_BWD_ERR32_DSAMPLE = 8.1e-6                       # every K (worst: K = 64, depth gradient only)
COMPOSITE_BWD_ERR32_DZ = {1: 3.7e-4, 2: 3.8e-5}            # K = 1, K = 2
COMPOSITE_BWD_ERR32_DZ_LONG = 1.6e-5                       # K >= 63 (worst: K = 256, underflow)
# the slice behind an opaque sample x 1e10 (d_sample's rgb columns, d_z).  Behind opaque@K-2 it is ONE sample: the same
# near-cancellation of a single d_z, on one of 257 rays (K = 1000; 5.1e-5 at K = 96)
COMPOSITE_BWD_ERR32_BEHIND = 7.2e-5
COMPOSITE_BWD_BAR_DSAMPLE = _bar(COMPOSITE_BWD_FLOOR, COMPOSITE_BWD_ERR32_DSAMPLE)      # = the floor
COMPOSITE_BWD_BAR_BEHIND = _bar(COMPOSITE_BWD_FLOOR, COMPOSITE_BWD_ERR32_BEHIND)


def composite_bwd_dz_err32(K):
    return COMPOSITE_BWD_ERR32_DZ.get(K, COMPOSITE_BWD_ERR32_DZ_LONG)


def composite_bwd_dz_bar(K):
    return _bar(COMPOSITE_BWD_FLOOR, composite_bwd_dz_err32(K))


GRAD_SUBSETS = ((0, 1, 0), (0, 0, 1), (0, 0, 0))           # (g_rgb, g_depth, g_weights) given: what the existing test does not run


def composite_bwd_n(K):
    return (1, 5) if K == COMPOSITE_BWD_KMAX else N_LIST


def subset_family(K):
    """The one family per K that also runs GRAD_SUBSETS and d_z_dev = NULL: an opaque sample next to the first chunk boundary
    where K reaches it, else `random`."""
    return "opaque@63" if K > 64 else "random"


def composite_grads(family, n, K):
    """Upstream gradients (g_rgb (n, 3), g_depth (n), g_weights (n, K)), standard normal, seeded from (K, family)."""
    rs = np.random.RandomState(_seed_of("composite_bwd", K, family))
    return tuple(rs.standard_normal(s).astype(np.float32) for s in ((n, 3), (n,), (n, K)))


def composite_bwd_ref(rays, z, samp, white, g_rgb, g_depth, g_w, dtype=F64):
    """(dL/d(sample) (n, K, 4), dL/dz (n, K)) of L = <g_rgb, rgb> + <g_depth, depth> + <g_w, weights> through orc.composite
    under autograd in `dtype` on the float32 inputs; a g that is None is absent (all None: zeros)."""
    zt, st = as_dt(z, dtype).requires_grad_(), as_dt(samp, dtype).requires_grad_()
    outs = orc.composite(as_dt(rays, dtype), zt, st, bool(white))                  # weights, rgb, depth
    terms = [(o * as_dt(g, dtype)).sum() for o, g in zip(outs, (g_w, g_rgb, g_depth)) if g is not None]
    if not terms:
        return torch.zeros_like(st), torch.zeros_like(zt)
    sum(terms).backward()
    return st.grad, zt.grad


def check_composite_bwd(fam, n, K, d_samp, d_z, ref, g_rgb_given=True):
    """One case against its reference ref = (d_sample, d_z) in float64.  d_z may be None (not asked for).
    Returns the per-row errors (d_sample, d_z, behind the opaque sample x 1e10); asserts the bars and the exact zeros."""
    e_s = row_err(d_samp, ref[0], n)
    assert e_s <= COMPOSITE_BWD_BAR_DSAMPLE, (fam, n, K, "d_sample", e_s)
    e_z = e_b = 0.0
    if d_z is not None:
        e_z = row_err(d_z, ref[1], n)
        assert e_z <= composite_bwd_dz_bar(K), (fam, n, K, "d_z", e_z)
    if fam == "zero_sigma":                                      # relu'(0) = 0, alpha = 0, w = 0: exact zeros
        assert float(torch.as_tensor(d_samp)[..., 3].abs().max()) == 0.0, (fam, n, K, "d_sigma not exactly 0")
        assert d_z is None or float(torch.as_tensor(d_z).abs().max()) == 0.0, (fam, n, K, "d_z not exactly 0")
    sl = behind(fam, K)
    if sl is not None:      # behind an opaque sample every gradient carries T = 1e-10 x ...: order-one numbers again after x 1e10
        e_b = row_err(torch.as_tensor(d_samp)[:, sl, :3].to(F64) * 1e10, ref[0][:, sl, :3] * 1e10, n)
        if d_z is not None:
            e_b = max(e_b, row_err(torch.as_tensor(d_z)[:, sl].to(F64) * 1e10, ref[1][:, sl] * 1e10, n))
        assert e_b <= COMPOSITE_BWD_BAR_BEHIND, (fam, n, K, "behind the opaque sample", e_b)
    return e_s, e_z, e_b


# --------------------------------------------------------------------------- yolo_aggregate backward
# float32 oracle under autograd against the float64 one, per (ray, anchor).  The figure comes from the maximum's own term
# g_0 p (1 - p) where the winning logit is 8 to 10: 1 - p = 2.5e-4 is formed from a float32 p, one ulp of which is 2.4e-4 of it
# (`random`, K = 200; 1.5e-5 at K = 128, below 1e-6 in every other family)
AGG_BWD_ERR32 = 3.2e-5
AGG_BWD_BAR = _bar(0.0, AGG_BWD_ERR32)                     # no earlier stage bar: twice the float32 oracle's error


def agg_bwd_families(K):
    return agg_families(K) + ["tie"]


def tie_pairs(K):
    """(first, second) positions of the exact maxima of the `tie` family: (K // 2, K - 1), and from K = 66 on (1, 65) -- the
    same lane in two successive `k += 64` iterations.  The first of ALL tied positions takes the maximum's gradient."""
    pairs = [(K // 2, K - 1)]
    if K >= 66:
        pairs.append((1, 65))
    return pairs


def agg_bwd_case(family, n, K, na, seed=0):
    """raw (n, K, na * 7) and the upstream gradient g (n, na, 7), standard normal."""
    if family == "tie":
        raw = agg_case("random", n, K, na, seed).reshape(n, K, na, 7)
        raw[..., 0] = np.minimum(raw[..., 0], 1.0)
        for pair in tie_pairs(K):
            raw[:, list(pair), :, 0] = 2.0
        raw = raw.reshape(n, K, na * 7)
    else:
        raw = agg_case(family, n, K, na, seed)
    g = np.random.RandomState(_seed_of("agg_bwd", K, na, family)).standard_normal((n, na, 7)).astype(np.float32)
    return raw, g


def agg_bwd_ref(raw, g, na, dtype=F64):
    """dL/d(raw) (n, K, na * 7) of L = <g, orc.yolo_aggregate(raw)> under autograd in `dtype` on the float32 inputs."""
    rt = as_dt(raw, dtype).requires_grad_()
    (orc.yolo_aggregate(rt, na) * as_dt(g, dtype)).sum().backward()
    return rt.grad


def agg_rows(d, na):
    """(n, K, na * 7) -> (n * na, K * 7): one row per (ray, anchor), as the kernel's wavefronts take them."""
    d = torch.as_tensor(np.asarray(d))
    n, K = d.shape[0], d.shape[1]
    return d.reshape(n, K, na, 7).permute(0, 2, 1, 3).reshape(n * na, K * 7)


def agg_row_err(got, ref, na):
    r = agg_rows(ref, na)
    return row_err(agg_rows(got, na), r, r.shape[0])


def max_term(raw, g, na):
    """The g_0 term of dL/d(raw[.., 0]) in float64 where it belongs: g_0 p (1 - p) at the FIRST index of the maximum, (n, K, na)."""
    o = as_dt(raw, F64).reshape(raw.shape[0], raw.shape[1], na, 7)[..., 0]
    p = torch.sigmoid(o)
    first = torch.zeros_like(p)
    first.scatter_(1, torch.argmax((o == o.max(1, keepdim=True)[0]).to(torch.int8), dim=1, keepdim=True), 1.0)   # first True
    return first * (as_dt(g, F64)[:, None, :, 0] * p * (1 - p))


def check_tie(got, ref, raw, g, K, na):
    """The semantics of the tie: the maximum's gradient reaches the first tied index and no other.  got, ref (n, K, na * 7);
    at each tied position got's column 0 is within the bar (x the row's maximum) of the reference -- which has the term at the
    first and not at the others -- and the term is at least 100 bars there, so that a kernel that puts it elsewhere, twice or
    nowhere fails.  Returns the number of (ray, anchor) rows on which the check discriminates."""
    n = raw.shape[0]
    G = torch.as_tensor(np.asarray(got), dtype=F64).reshape(n, K, na, 7)
    R = torch.as_tensor(np.asarray(ref), dtype=F64).reshape(n, K, na, 7)
    term = max_term(raw, g, na)
    tied = sorted({i for pair in tie_pairs(K) for i in pair})
    assert bool((term[:, tied[0]] != 0).any()) and float(term[:, tied[1:]].abs().max() if len(tied) > 1 else 0.0) == 0.0
    top = R.abs().amax(dim=(1, 3))                                          # (n, na): the row's maximum
    slack = AGG_BWD_BAR * top
    for i in tied:
        assert bool(((G[:, i, :, 0] - R[:, i, :, 0]).abs() <= slack).all()), ("tie", K, na, "position %d" % i)
    return int((term[:, tied[0]].abs() > 100 * slack).sum())


# --------------------------------------------------------------------------- depth-gradient gather (exact)
GATHER_KFD = (1, 4, 63, 64, 65, 130)
GATHER_PATTERNS = ("live", "dead", "alternating", "last_only", "random")


def gather_case(pattern, n, kfd, seed=0):
    """sel (n, kfd) int32: ray * kt + a random position of the ray's own row of dz, or -1; dz (n, kt); g_in (n)."""
    rs = np.random.RandomState(_seed_of("gather", pattern, n, kfd, seed) % (2 ** 31))
    kt = kfd + 7
    dz = rs.standard_normal((n, kt)).astype(np.float32)
    sel = (np.arange(n)[:, None] * kt + rs.randint(0, kt, (n, kfd))).astype(np.int32)
    if pattern == "dead":
        sel[:] = -1
    elif pattern == "alternating":
        sel[:, 1::2] = -1
    elif pattern == "last_only":
        sel[:, :-1] = -1
    elif pattern == "random":
        sel[rs.rand(n, kfd) < 0.3] = -1
    else:
        assert pattern == "live", pattern
    assert bool(((sel < 0) | (sel // kt == np.arange(n)[:, None])).all())
    return sel, dz, rs.standard_normal(n).astype(np.float32)


def gather_ref(sel, dz, g_in=None):
    """g_in[ray] (or 0) + the live samples' dz added one after the other in sample order, every sum rounded to float32: the
    order depth_grad_gather_kernel promises."""
    n, kfd = sel.shape
    flat = np.asarray(dz, np.float32).reshape(-1)
    s = np.zeros(n, np.float32) if g_in is None else np.array(g_in, np.float32)
    for j in range(kfd):
        live = sel[:, j] >= 0
        v = np.where(live, flat[np.where(live, sel[:, j], 0)], np.float32(0)).astype(np.float32)
        s = np.where(live, s + v, s).astype(np.float32)        # a dead sample adds nothing (not even + 0: -0 stays -0)
    assert s.dtype == np.float32
    return s


# --------------------------------------------------------------------------- locate depth samples (exact)
LOCATE_SHAPES = tuple(s for s in FINE_SHAPES if s[2] > 0)
LOCATE_N = (5, 257)
LOCATE_STD = (0.01, 0.05)
ROBUST = 1e-6
LOCATE_SEED = 0x5EED0000BEEF            # a non-zero high word


def locate_case(n, kc, kf, kfd, seed=0):
    """fine_case (lindisp off) with the coarse depth of a fifth of the rays exactly `near` and of a fifth exactly `far` -- about
    half of their draws clamp -- and g = 0 on ray 0, whose depth is `near`: zz == near exactly, which is NOT inside."""
    c = fine_case(n, kc, kf, kfd, 0, "random", seed)
    near, far = near_far(0)
    c["depth"] = c["depth"].copy()
    c["depth"][0::5] = near
    c["depth"][1::5] = far
    c["g"] = c["g"].copy()
    c["g"][0] = 0.0
    return c


def locate_expect(c, depth_std, g=None):
    """Float64 on the float32 inputs: zz = depth + g * std (n, kfd); inside = strictly within (near, far); checked = robust
    (further than ROBUST from both bounds) or exactly ON a bound through g == 0 (zz == depth == bound in every arithmetic)."""
    g = np.asarray(c["g"] if g is None else g, np.float32)
    depth = np.asarray(c["depth"], np.float32).astype(np.float64)[:, None]
    std = float(np.float32(depth_std))
    zz = depth + g.astype(np.float64) * std
    near = c["rays"][:, 6:7].astype(np.float64)
    far = c["rays"][:, 7:8].astype(np.float64)
    inside = (zz > near) & (zz < far)
    on_bound = (g == 0) & ((depth == near) | (depth == far))
    checked = (np.minimum(np.abs(zz - near), np.abs(zz - far)) > ROBUST) | on_bound
    return zz, inside, checked


def check_located(sel, z_fine, c, depth_std, kt, g=None):
    """sel (n, kfd) int32 and z_fine (n, kt) of one case against locate_expect.  Returns the number of samples left out."""
    sel, z_fine = np.asarray(sel), np.asarray(z_fine, np.float32)
    zz, inside, checked = locate_expect(c, depth_std, g)
    n, kfd = zz.shape
    assert sel.shape == (n, kfd) and 100 * int((~checked).sum()) < checked.size
    assert bool((sel[checked & ~inside] == -1).all()), "a clamped sample was located"
    ok = checked & inside
    assert bool((sel[ok] >= 0).all()), "%d samples strictly inside (near, far) were not located" % int((sel[ok] < 0).sum())
    ray = np.broadcast_to(np.arange(n)[:, None], (n, kfd))
    assert bool((sel[ok] // kt == ray[ok]).all()), "a sample was located on another ray"
    pos = sel[ok] % kt
    val = z_fine[ray[ok], pos]
    assert float(np.abs(val.astype(np.float64) - zz[ok]).max(initial=0.0)) <= ROBUST
    before = z_fine[ray[ok], np.maximum(pos - 1, 0)]
    assert bool(((pos == 0) | (before < val)).all()), "not the first position of its value"
    rest = sel[~checked]
    assert bool(((rest == -1) | ((rest >= 0) & (rest // kt == ray[~checked]))).all())      # left out, but never out of bounds
    return int((~checked).sum())
LOCATE_SEEDED_SHAPE = (64, 32, 16)
