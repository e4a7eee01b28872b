"""
Cases, plain references, bars and recorded figures of the trunk's stage sweep (tests/test_cpu_trunk_stage_refs.py,
tests/test_gpu_trunk_stages.py): the convolution in its forward and transposed form, the convolution's weight gradient, batch
norm forward and backward, the 3x3/2 max-pool and the bilinear pyramid, each through its own entry point (include/pnyolo.h
pny_trunk_*), on inputs the sweep chooses.

References.  Every float result is held to a float64 evaluation ON THE FLOAT32 INPUTS: F.conv2d, F.max_pool2d,
F.interpolate(bilinear, align_corners=True) and their autograd; batch norm forward and backward written out as formulae
(biased variance for normalising, unbiased for the running step, relu mask `out > 0`), which the CPU test shows equal to
F.batch_norm and its autograd in float64.

Errors are max |got - ref| over a tensor, divided by the float64 tensor's max |.| for gradients and by max(1, max |.|) for
activations and statistics -- the scales of the whole-trunk bounds the stages sit under (tests/test_gpu_trunk.py: 2e-4 x
max(1, max |.|) for activations, 1e-4 of the tensor's max for gradients, 2e-6 x max(1, max |.|) for running statistics).

Bars.  Each bar is TWICE the largest error of a float32 restatement against float64 over the sweep's cases (the factor and the
reasoning of tests/stage_ref.py: the kernels sum in another order than the restatement).  The restatement of a convolution is
F.conv2d (and its autograd) in float32 under the suite's pinned CPU arithmetic; of the bilinear pyramid F.interpolate in
float32; of batch norm's pixel sums a float32 accumulation IN PIXEL ORDER (np.cumsum(dtype=float32)) of the values the kernel
sums (shifted by pixel 0 in the forward) -- F.batch_norm and torch.sum accumulate in double or by cascade and would bound no
float32 kernel.  The figure behind every bar is recorded as *_ERR32; the CPU test measures each again (within 10 % above, not
below half) and shows every bar under its cap on every case.  The kernels' own errors set nothing.  Marker runs (below) are
cases like any other and count towards the figures.

Exact cases (torch.equal): max-pool forward; max-pool backward with an upstream gradient of small integers; the pyramid where
the level has the latent's size.

Marker pixels.  A pixel reduction (batch-norm statistics, batch-norm backward sums, the weight gradient) must not hide a dropped
or doubled pixel inside its bar, so every such case also runs with the pixels on both sides of every chunk / slice boundary, and
the last pixel, set to 100 x the input's standard deviation.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as Fn

F32, F64 = torch.float32, torch.float64
EPS = 1e-5
MARKER = 100.0

# ------------------------------------------------------------------------------------------------ caps, figures, bars
CAP_ACT, CAP_GRAD, CAP_RUN = 2e-4, 1e-4, 2e-6      # the whole-trunk bounds (see above); no stage bar may be looser

# *_ERR32: largest float32-restatement error over the sweep's cases, measured on the CPU (tests/test_cpu_trunk_stage_refs.py)
CONV_FWD_ERR32 = 1.05e-6
CONV_T_ERR32 = 7.7e-7
CONV_DW_ERR32 = 2.6e-6
BN_OUT_ERR32 = 1.8e-5
BN_STAT_ERR32 = 9.0e-6           # mean and invstd, as the backward takes them
BN_RUN_ERR32 = 9.6e-7            # stepped running_mean / running_var
BN_DY_ERR32 = 3.2e-6
BN_DPARAM_ERR32 = 6.7e-6         # d gamma, d beta
UP_FWD_ERR32 = 1.55e-6
UP_BWD_ERR32 = 1.8e-6

CONV_FWD_BAR, CONV_T_BAR, CONV_DW_BAR = 2 * CONV_FWD_ERR32, 2 * CONV_T_ERR32, 2 * CONV_DW_ERR32
BN_OUT_BAR, BN_STAT_BAR, BN_RUN_BAR = 2 * BN_OUT_ERR32, 2 * BN_STAT_ERR32, 2 * BN_RUN_ERR32
BN_DY_BAR, BN_DPARAM_BAR = 2 * BN_DY_ERR32, 2 * BN_DPARAM_ERR32
UP_FWD_BAR, UP_BWD_BAR = 2 * UP_FWD_ERR32, 2 * UP_BWD_ERR32

# bar -> (cap, kind of scale)
BARS = {
    "conv_fwd": (CONV_FWD_BAR, CAP_ACT, "act"), "conv_t": (CONV_T_BAR, CAP_GRAD, "grad"), "conv_dw": (CONV_DW_BAR, CAP_GRAD, "grad"),
    "bn_out": (BN_OUT_BAR, CAP_ACT, "act"), "bn_stat": (BN_STAT_BAR, CAP_ACT, "act"), "bn_run": (BN_RUN_BAR, CAP_RUN, "act"),
    "bn_dy": (BN_DY_BAR, CAP_GRAD, "grad"), "bn_dparam": (BN_DPARAM_BAR, CAP_GRAD, "grad"),
    "up_fwd": (UP_FWD_BAR, CAP_ACT, "act"), "up_bwd": (UP_BWD_BAR, CAP_GRAD, "grad"),
}


def t64(x):
    return torch.as_tensor(np.asarray(x)).to(F64)


def scale_of(ref, kind):
    m = float(t64(ref).abs().max()) if t64(ref).numel() else 0.0
    return max(1.0, m) if kind == "act" else m


def rel_err(got, ref, kind):
    """max |got - ref| over the float64 tensor's max (kind "grad") or over max(1, that) (kind "act")."""
    got, ref = t64(got), t64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite result"
    s = scale_of(ref, kind)
    e = float((got - ref).abs().max())
    return e / s if s > 0.0 else e


# ------------------------------------------------------------------------------------------------ geometries
# (k, stride, pad, cin, cout): the eight distinct convolutions of the trunk's table
GEOMS = ((7, 2, 3, 3, 64), (3, 1, 1, 64, 64), (3, 2, 1, 64, 128), (1, 2, 0, 64, 128), (3, 1, 1, 128, 128), (3, 2, 1, 128, 256),
         (1, 2, 0, 128, 256), (3, 1, 1, 256, 256))
STEM, L1 = 0, 1


def conv_out(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def table(lib):
    """The library's table of units as (k, stride, pad, cin, cout) rows (pny_trunk_unit; needs no GPU)."""
    rows, v = [], [C.c_int() for _ in range(5)]
    while lib.pny_trunk_unit(len(rows), *[C.byref(x) for x in v]) == 0:
        cin, cout, k, stride, pad = (x.value for x in v)
        rows.append((k, stride, pad, cin, cout))
        assert len(rows) < 1000
    return rows


def unit_of(lib):
    """GEOMS index -> the first unit of the table with that geometry."""
    rows = table(lib)
    return [rows.index(g) for g in GEOMS]


def in_size(g, out, parity):
    """An input size that convolution g maps to `out`: the only one at stride 1, the odd (parity 0) or even one at stride 2."""
    k, s, p = g[:3]
    i = out if s == 1 else 2 * out - 1 + parity
    assert conv_out(i, k, s, p) == out
    return i


def nhwc(x, pad4=False):
    """NCHW -> the kernels' channel-last layout (channels zero-padded to a multiple of 4: the stem's images)."""
    x = torch.as_tensor(x).permute(0, 2, 3, 1)
    if pad4 and x.shape[-1] % 4:
        x = torch.cat([x, torch.zeros(x.shape[:-1] + (4 - x.shape[-1] % 4,), dtype=x.dtype)], -1)
    return x.contiguous()


def nchw(x):
    return torch.as_tensor(x).permute(0, 3, 1, 2).contiguous()


def _randn(rs, *shape):
    return torch.from_numpy(rs.randn(*shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------ convolution
# output shapes (n, hout, wout) with 1, 30, 30, 33, 63, 64 and 65 pixels
CONV_OUT_SHAPES = ((1, 1, 1), (1, 5, 6), (2, 5, 3), (1, 3, 11), (1, 7, 9), (2, 4, 8), (1, 5, 13))
CONV_T_STRIDE2_INPUTS = ((4, 4), (5, 7), (8, 6), (9, 12))       # forward-input sizes of the stride-2 transposed cases
# (geometry, n, hin, win): the four conv_mfma_kernel instantiations on a 256-CU device.  The first four are whole 64-pixel tiles
# (2 x 128 x 131 = 524 x 64: every 2 x 128 x W is), so the others end in a ragged tile of 64 x 64: 64 -> 64 at 2 x 129 x 129
# (33 282 px: 2 left over, the tile's second half wholly outside) and 2 x 127 x 131 (33 274 px: 58 left over, the second half
# partly outside) for the split instantiation; the stem at 12 x 130 x 130 (50 700 px: 12 left over, 793 tiles) and 12 x 124 x 133
# (49 848 px: 56 left over, 779 tiles) for the plain one, whose workgroups of four tiles then end in idle waves.
CONV_LARGE = ((L1, 2, 128, 128), (L1, 2, 128, 131), (STEM, 12, 128, 128), (3, 1, 256, 256),
              (L1, 2, 129, 129), (L1, 2, 127, 131), (STEM, 12, 130, 130), (STEM, 12, 124, 133))
# ... and the 64 x 64 tiles under a transposed convolution: whole tiles, and 1 x 249 x 251 (62 499 px: 35 left over, 977 tiles)
CONV_T_LARGE = ((3, 1, 256, 256), (3, 1, 249, 251))


def large_tiles(case, transposed):
    """(output pixels, 64-channel tile columns) of a large case: what decides whether its last 64 x 64 tile is ragged."""
    k, s, p, cin, cout = GEOMS[case["gi"]]
    if transposed:
        return case["n"] * case["hin"] * case["win"], cin // 64
    return case["n"] * conv_out(case["hin"], k, s, p) * conv_out(case["win"], k, s, p), cout // 64


def conv_fwd_cases():
    """dicts gi, n, hin, win, resid, relu, affine (non-trivial scale / shift), tag"""
    out = []
    for gi, g in enumerate(GEOMS):
        for j, (n, ho, wo) in enumerate(CONV_OUT_SHAPES):
            out.append(dict(gi=gi, n=n, hin=in_size(g, ho, j & 1), win=in_size(g, wo, (j >> 1) & 1), resid=0, relu=0, affine=0, tag="edge"))
        for resid in (0, 1):
            for relu in (0, 1):
                out.append(dict(gi=gi, n=1, hin=in_size(g, 5, 0), win=in_size(g, 6, 1), resid=resid, relu=relu, affine=1, tag="epilogue"))
    out.append(dict(gi=STEM, n=1, hin=33, win=47, resid=0, relu=1, affine=0, tag="edge"))
    for gi, n, hin, win in CONV_LARGE:
        out.append(dict(gi=gi, n=n, hin=hin, win=win, resid=0, relu=0, affine=0, tag="large"))
    return out


def conv_t_cases():
    """The input gradient: (hin, win) is the FORWARD input's size, i.e. the size of the result."""
    out = []
    for gi, g in enumerate(GEOMS):
        if g[3] < 32:
            continue            # the stem: its input gradient (the images') is never computed, and 3 rows are no MFMA tile
        if g[1] == 1:
            for j, (n, ho, wo) in enumerate(CONV_OUT_SHAPES):
                out.append(dict(gi=gi, n=n, hin=ho, win=wo, resid=j & 1, tag="edge"))
        else:
            for n in (1, 2):
                for hin, win in CONV_T_STRIDE2_INPUTS:
                    out.append(dict(gi=gi, n=n, hin=hin, win=win, resid=n - 1, tag="stride2"))
    for gi, n, hin, win in CONV_T_LARGE:
        out.append(dict(gi=gi, n=n, hin=hin, win=win, resid=0, tag="large"))
    return out


def conv_inputs(case, transposed, seed=0):
    """float32 NCHW tensors: x (or dy when transposed), w, scale, shift, resid (or None)."""
    k, s, p, cin, cout = GEOMS[case["gi"]]
    n, hin, win = case["n"], case["hin"], case["win"]
    ho, wo = conv_out(hin, k, s, p), conv_out(win, k, s, p)
    rs = np.random.RandomState(7000 + 131 * case["gi"] + 17 * hin + win + 1000 * n + seed + (500 if transposed else 0))
    w = _randn(rs, cout, cin, k, k) / float(np.sqrt(cin * k * k))
    cres = cin if transposed else cout
    src = _randn(rs, n, cout, ho, wo) if transposed else _randn(rs, n, cin, hin, win)
    if case.get("affine"):
        scale, shift = 0.5 + torch.from_numpy(rs.rand(cres).astype(np.float32)), _randn(rs, cres)
    else:
        scale, shift = torch.ones(cres), torch.zeros(cres)
    rshape = (n, cin, hin, win) if transposed else (n, cout, ho, wo)
    resid = _randn(rs, *rshape) if case["resid"] else None
    return src, w, scale, shift, resid


def conv_fwd_ref(case, inputs, dtype):
    k, s, p = GEOMS[case["gi"]][:3]
    x, w, scale, shift, resid = [None if t is None else t.to(dtype) for t in inputs]
    y = Fn.conv2d(x, w, None, s, p) * scale[None, :, None, None] + shift[None, :, None, None]
    if resid is not None:
        y = y + resid
    return torch.relu(y) if case["relu"] else y


def conv_t_ref(case, inputs, dtype):
    k, s, p, cin, cout = GEOMS[case["gi"]]
    dy, w, _, _, resid = [None if t is None else t.to(dtype) for t in inputs]
    x0 = torch.zeros(case["n"], cin, case["hin"], case["win"], dtype=dtype, requires_grad=True)
    g, = torch.autograd.grad(Fn.conv2d(x0, w, None, s, p), x0, dy)
    return g if resid is None else g + resid


# ------------------------------------------------------------------------------------------------ weight gradient
# output shapes (n, hout, wout) with 1, 15, 33, 127, 128, 129, 255, 256 and 257 pixels; stride 2 takes the odd input size
DW_OUT_SHAPES = ((1, 1, 1), (1, 3, 5), (1, 3, 11), (1, 1, 127), (2, 8, 8), (1, 3, 43), (1, 15, 17), (1, 16, 16), (1, 1, 257))
# (geometry, n, hin, win): the stem and layer1.0.conv1 at the benchmark's 12 views of 128 x 128 (with and without the first pool)
DW_LARGE = ((STEM, 12, 128, 128), (L1, 12, 32, 32), (L1, 12, 64, 64))


def dw_cases():
    out = []
    for gi, g in enumerate(GEOMS):
        for n, ho, wo in DW_OUT_SHAPES:
            out.append(dict(gi=gi, n=n, hin=in_size(g, ho, 0), win=in_size(g, wo, 0), tag="edge"))
    for gi, n, hin, win in DW_LARGE:
        out.append(dict(gi=gi, n=n, hin=hin, win=win, tag="large"))
    return out


def boundary_pixels(npix, chunk, first=True):
    """Both sides of every chunk boundary, the last pixel and (first) pixel 0."""
    idx = {npix - 1}
    if first:
        idx.add(0)
    for b in range(chunk, npix, chunk):
        idx.update((b - 1, b))
    return sorted(idx)


def dw_chunk(case):
    """Pixels per slice of the weight gradient's split contraction, as the launcher cuts it today: about 1024 work items in
    all, slices of at least 128 pixels, rounded up to 4.  Only the CPU figure's marker runs place their markers by it; the GPU
    sweep takes the slice length the entry reports."""
    k, s, p, cin, cout = GEOMS[case["gi"]]
    npix = case["n"] * conv_out(case["hin"], k, s, p) * conv_out(case["win"], k, s, p)
    base = (cout // 64) * ((k * k * ((cin + 3) // 4 * 4) + 127) // 128)
    sp = max(1, min((1024 + base - 1) // base, max(1, npix // 128)))
    return ((npix + sp - 1) // sp + 3) // 4 * 4


def dw_inputs(case, chunk=None):
    """float32 NCHW x, dy; chunk: the slice length the entry reported -> dy carries marker pixels at the slice boundaries."""
    k, s, p, cin, cout = GEOMS[case["gi"]]
    n, hin, win = case["n"], case["hin"], case["win"]
    ho, wo = conv_out(hin, k, s, p), conv_out(win, k, s, p)
    rs = np.random.RandomState(9000 + 131 * case["gi"] + 17 * hin + win + 1000 * n)
    x, dy = _randn(rs, n, cin, hin, win), _randn(rs, n, cout, ho, wo)
    if chunk:
        flat = nhwc(dy).reshape(n * ho * wo, cout)
        flat[boundary_pixels(n * ho * wo, chunk)] = MARKER
        dy = nchw(flat.reshape(n, ho, wo, cout))
    return x, dy


def dw_ref(case, x, dy, dtype):
    k, s, p, cin, cout = GEOMS[case["gi"]]
    w = torch.zeros(cout, cin, k, k, dtype=dtype, requires_grad=True)
    g, = torch.autograd.grad(Fn.conv2d(x.to(dtype), w, None, s, p), w, dy.to(dtype))
    return g


# ------------------------------------------------------------------------------------------------ batch norm
BN_C = (64, 128, 256)
BN_P = (4, 6, 255, 256, 257, 1000, 16383, 16384, 16385, 20000, 49152)
BN_MAX_RATIO = 30.0                   # |mean| / std of the inputs
# The forward sums are shifted by pixel 0.  Summed in float32 in pixel order, an ordinary draw there (up to 3 sigma off the
# mean) makes the sum of the shifted values drift to 1e5 at 49 152 pixels, and twice the restatement's error of the stepped
# running statistics (7.5e-6) passes their 2e-6 cap.  From BN_PIN_FROM pixels on, pixel 0 therefore sits an eighth of a sigma
# off the channel's mean: the cases changed, the cap kept.  Below, pixel 0 is whatever was drawn.
BN_PIN_FROM, BN_PIN_OFFSET = 16383, 0.125
# The sum of 49 152 squares in float32 in pixel order is 1e-5 off, a tenth of which reaches the stepped running variance: twice
# that (2.6e-6) passes the cap as well, whatever pixel 0 holds.  The running step (a blend of the mean and variance the call
# also returns, which are held at every size) is therefore swept with momentum 0.1 up to BN_STEP_TO pixels and with
# BN_SMALL_MOMENTUM above, which still steps both statistics at the benchmark's 49 152 pixels; the marker runs, whose variance
# is 60 times the plain runs', leave it off (momentum 0).
BN_STEP_TO, BN_SMALL_MOMENTUM = 20000, 0.01


def bn_chunk(P):
    """Pixels per workgroup of the statistics kernels: at most 64 workgroups of at least 256 pixels (marker placement only)."""
    b = min(64, max(1, (P + 255) // 256))
    return (P + b - 1) // b


def bn_cases(C):
    """dicts P, dist ("n01" | "n30"), special (None | "const" | "markers"), resid, relu, momentum, use_running, run (running
    statistics passed), null (which optional backward output is left out: None, "g_out", "d_gamma", "d_beta"), mask
    (backward: "out" = a supplied mask with exact zeros, None = no relu behind the batch norm)."""
    out = []
    i = BN_C.index(C)
    for P in BN_P:
        for dist in ("n01", "n30"):
            out.append(dict(P=P, dist=dist, special=None, resid=i & 1, relu=(i >> 1) & 1, momentum=0.1 if (i >> 2) & 1 else 0.0,
                            use_running=1 if i % 5 == 4 else 0, run=0 if i % 7 == 3 else 1,
                            null=(None, "g_out", "d_gamma", "d_beta")[i % 4], mask="out" if i % 3 else None))
            if out[-1]["use_running"]:
                out[-1]["run"] = 1
            if P > BN_STEP_TO and out[-1]["momentum"] > 0:
                out[-1]["momentum"] = BN_SMALL_MOMENTUM
            i += 1
    for P in (257, 20000, 49152):
        out.append(dict(P=P, dist="n01", special="markers", resid=0, relu=1, momentum=0.0, use_running=0, run=1, null=None, mask="out"))
    out.append(dict(P=1000, dist="n30", special="const", resid=1, relu=1, momentum=0.1, use_running=0, run=1, null=None, mask="out"))
    return out


def bn_inputs(C, case):
    """float32 (P, C) y, d_out, resid-or-None, mask-or-None; (C,) gamma, beta, running_mean, running_var."""
    P = case["P"]
    rs = np.random.RandomState(11000 + C + 7 * P + (3 if case["dist"] == "n30" else 0) + (1 if case["special"] else 0))
    mu = 30.0 if case["dist"] == "n30" else 0.0
    y = _randn(rs, P, C) + mu
    d_out = _randn(rs, P, C)
    if P >= BN_PIN_FROM:
        y[0] = mu + BN_PIN_OFFSET
    if case["special"] == "const":
        y[:, 5] = y[0, 5]
    if case["special"] == "markers":
        y[boundary_pixels(P, bn_chunk(P), first=False)] = mu + MARKER     # (pixel 0 is the forward sums' shift: its term is zero)
        d_out[boundary_pixels(P, bn_chunk(P))] = MARKER
    gamma, beta = 0.5 + torch.from_numpy(rs.rand(C).astype(np.float32)), _randn(rs, C)
    rm, rv = _randn(rs, C) * 0.5 + mu, 0.5 + torch.from_numpy(rs.rand(C).astype(np.float32))
    resid = _randn(rs, P, C) if case["resid"] else None
    mask = None
    if case["mask"]:
        mask = torch.relu(_randn(rs, P, C))          # exact zeros and positives, as a relu leaves them
    return dict(y=y, d_out=d_out, resid=resid, mask=mask, gamma=gamma, beta=beta, rm=rm, rv=rv)


def bn_fwd_ref(case, inp, dtype=F64):
    """out, mean, invstd, running_mean', running_var' (the running pair as passed where it is not stepped)."""
    y, gamma, beta = inp["y"].to(dtype), inp["gamma"].to(dtype), inp["beta"].to(dtype)
    rm, rv = inp["rm"].to(dtype), inp["rv"].to(dtype)
    P = y.shape[0]
    mean = y.sum(0) / P
    var = ((y - mean) ** 2).sum(0) / P                   # biased: what normalises
    if case["use_running"]:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + EPS)
    out = (y - mean) * invstd * gamma + beta
    if inp["resid"] is not None:
        out = out + inp["resid"].to(dtype)
    if case["relu"]:
        out = torch.relu(out)
    m = float(np.float32(case["momentum"]))              # the float32 argument's value
    if not case["use_running"] and m > 0:
        rm = (1 - m) * rm + m * mean
        rv = (1 - m) * rv + m * var * (P / (P - 1.0) if P > 1 else 1.0)   # unbiased: what the running step takes
    return out, mean, invstd, rm, rv


def bn_fwd_f32(case, inp):
    """The float32 restatement: pixel sums accumulated in float32 in pixel order, on the values shifted by pixel 0."""
    f = np.float32
    y = inp["y"].numpy()
    P = y.shape[0]
    d = y - y[0]
    s1, s2 = np.cumsum(d, 0, dtype=f)[-1], np.cumsum(d * d, 0, dtype=f)[-1]
    m = s1 / f(P)
    mean, var = y[0] + m, np.maximum(s2 / f(P) - m * m, f(0))
    rm, rv = inp["rm"].numpy(), inp["rv"].numpy()
    if case["use_running"]:
        mean, var = rm, rv
    invstd = f(1) / np.sqrt(var + f(EPS))
    out = (y - mean) * (invstd * inp["gamma"].numpy()) + inp["beta"].numpy()
    if inp["resid"] is not None:
        out = out + inp["resid"].numpy()
    if case["relu"]:
        out = np.maximum(out, f(0))
    mo = f(case["momentum"])
    if not case["use_running"] and mo > 0:
        rm = (f(1) - mo) * rm + mo * mean
        rv = (f(1) - mo) * rv + mo * (var * (f(P) / f(P - 1)) if P > 1 else var)
    return [torch.from_numpy(np.asarray(a, f)) for a in (out, mean, invstd, rm, rv)]


def bn_bwd_ref(case, inp, mean, invstd, dtype=F64):
    """dy, g (the masked upstream gradient), d_gamma, d_beta; mean / invstd are INPUTS (float32, as the forward stored them)."""
    y, g, gamma = inp["y"].to(dtype), inp["d_out"].to(dtype), inp["gamma"].to(dtype)
    mean, invstd = mean.to(dtype), invstd.to(dtype)
    P = y.shape[0]
    if inp["mask"] is not None:
        g = g * (inp["mask"] > 0).to(dtype)
    xh = (y - mean) * invstd
    s1, s2 = g.sum(0), (g * xh).sum(0)
    dy = gamma * invstd * (g if case["use_running"] else g - s1 / P - xh * (s2 / P))
    return dy, g, s2, s1


def bn_bwd_f32(case, inp, mean, invstd):
    f = np.float32
    y, g, gamma = inp["y"].numpy(), inp["d_out"].numpy(), inp["gamma"].numpy()
    mean, invstd = mean.numpy(), invstd.numpy()
    P = y.shape[0]
    if inp["mask"] is not None:
        g = g * (inp["mask"].numpy() > 0).astype(f)
    xh = (y - mean) * invstd
    s1, s2 = np.cumsum(g, 0, dtype=f)[-1], np.cumsum(g * xh, 0, dtype=f)[-1]
    dy = gamma * invstd * (g if case["use_running"] else g - s1 / f(P) - xh * (s2 / f(P)))
    return [torch.from_numpy(np.asarray(a, f)) for a in (dy, g, s2, s1)]


# ------------------------------------------------------------------------------------------------ max-pool
POOL_SIZES = ((2, 2), (3, 3), (4, 5), (16, 16), (17, 24), (64, 64))
POOL_N = (1, 3)
POOL_KINDS = ("relu", "const", "distinct")
POOL_C = 64


def pool_inputs(n, h, w, kind):
    """float32 NCHW input, integer-valued upstream gradient and integer-valued `add`."""
    rs = np.random.RandomState(13000 + 100 * h + w + n)
    if kind == "relu":
        x = torch.relu(_randn(rs, n, POOL_C, h, w))               # about half the plane exact zeros: ties everywhere
    elif kind == "const":
        x = torch.full((n, POOL_C, h, w), 0.75)
    else:
        x = torch.from_numpy(rs.permutation(n * POOL_C * h * w).astype(np.float32).reshape(n, POOL_C, h, w)) * 0.25 - 7.0
    ho, wo = conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1)
    g = torch.from_numpy(rs.randint(-8, 9, (n, POOL_C, ho, wo)).astype(np.float32))
    add = torch.from_numpy(rs.randint(-8, 9, (n, POOL_C, h, w)).astype(np.float32))
    return x, g, add


def pool_fwd_ref(x):
    return Fn.max_pool2d(x.to(F64), 3, 2, 1)


def pool_bwd_ref(x, g, add=None):
    x0 = x.to(F64).requires_grad_(True)
    d, = torch.autograd.grad(Fn.max_pool2d(x0, 3, 2, 1), x0, g.to(F64))
    return d if add is None else d + add.to(F64)


def pool_bwd_first_max(x, g):
    """By hand: every window's gradient goes to its FIRST maximum in scan order (rows, then columns; `>` keeps the first)."""
    x, g = x.numpy(), g.numpy()
    n, c, h, w = x.shape
    d = np.zeros(x.shape, np.float64)
    for oy in range(g.shape[2]):
        for ox in range(g.shape[3]):
            best = np.full((n, c), -np.inf)
            arg = np.zeros((n, c), np.int64)
            for yy in range(max(0, 2 * oy - 1), min(h, 2 * oy + 2)):
                for xx in range(max(0, 2 * ox - 1), min(w, 2 * ox + 2)):
                    better = x[:, :, yy, xx] > best
                    best = np.where(better, x[:, :, yy, xx], best)
                    arg = np.where(better, yy * w + xx, arg)
            np.add.at(d.reshape(n, c, h * w), (np.arange(n)[:, None], np.arange(c)[None, :], arg), g[:, :, oy, ox])
    return torch.from_numpy(d)


# ------------------------------------------------------------------------------------------------ pyramid
UP_CH, UP_COFF, UP_LATENT = (64, 64, 128, 256), (0, 64, 128, 256), 512
UP_IMAGES = ((32, 32, True), (33, 47, True), (32, 40, True), (128, 128, True), (75, 100, False))   # (H, W, first pool)
UP_CASES = tuple(im + (1,) for im in UP_IMAGES) + ((33, 47, True, 2),)      # ... and n: one size with a second image behind the first


def pyramid(H, W, pool):
    hs, ws = [conv_out(H, 7, 2, 3)], [conv_out(W, 7, 2, 3)]
    hs.append(conv_out(hs[0], 3, 2, 1) if pool else hs[0])
    ws.append(conv_out(ws[0], 3, 2, 1) if pool else ws[0])
    for _ in range(2):
        hs.append(conv_out(hs[-1], 3, 2, 1))
        ws.append(conv_out(ws[-1], 3, 2, 1))
    return list(zip(hs, ws))


def up_inputs(H, W, pool, n=1):
    """Per level a float32 NCHW tensor; the upstream gradient of the latent (n, 512, h0, w0); per level an `add`."""
    rs = np.random.RandomState(15000 + 10 * H + W + 7 * (n - 1))
    sizes = pyramid(H, W, pool)
    levels = [_randn(rs, n, UP_CH[lv], *sizes[lv]) for lv in range(4)]
    g = _randn(rs, n, UP_LATENT, *sizes[0])
    adds = [_randn(rs, n, UP_CH[lv], *sizes[lv]) for lv in range(4)]
    return sizes, levels, g, adds


def up_fwd_ref(level, size0, dtype):
    return Fn.interpolate(level.to(dtype), size=tuple(size0), mode="bilinear", align_corners=True)


def up_bwd_ref(level, size0, g_slice, add, dtype):
    x0 = torch.zeros_like(level, dtype=dtype).requires_grad_(True)
    d, = torch.autograd.grad(Fn.interpolate(x0, size=tuple(size0), mode="bilinear", align_corners=True), x0, g_slice.to(dtype))
    return d if add is None else d + add.to(dtype)
