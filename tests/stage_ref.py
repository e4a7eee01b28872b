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


def hip_fine(c, kc, kf, kfd, lindisp, depth_std=DEPTH_STD, device="cuda:0"):
    """pny_sample_fine on a case of fine_case / dyadic_case / depth_tie_case (GPU; the one place that marshals its arguments,
    for the sweep and for its two-device child process).  Returns the merged depths (n, kc + kf) on the CPU."""
    from pixel_nerf_yolo_amd import lib as plib
    t = {k: torch.as_tensor(c[k], dtype=F32, device=device).contiguous() for k in ("rays", "zc", "w", "depth", "u", "u2", "g")}
    opt = lambda v: plib.ptr(v) if v.numel() else None          # noqa: E731  (NULL for an absent draw array)
    n = t["rays"].shape[0]
    zo = torch.full((n, kc + kf), float("nan"), device=device)
    plib.check(plib.load().pny_sample_fine(plib.ptr(t["rays"]), plib.ptr(t["zc"]), plib.ptr(t["w"]), plib.ptr(t["depth"]), n, kc,
                                           kf, kfd, depth_std, lindisp, opt(t["u"]), opt(t["u2"]), opt(t["g"]), 0,
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
