"""
Cases, plain references, bars and recorded figures of the latent projection's sweep (tests/test_cpu_projection_ref.py,
tests/test_gpu_projection.py): the pixel-wise GEMM that fills the projected maps, through its read-out (include/pnyolo.h
pny_scene_projection), on latents and lin_z weights the sweep chooses.

Reference.  out[p, 512 b + n] = sum_k lin_z[b].weight[n, k] latent[v, k, y, x] with p = (v hl + y) wl + x, in float64 ON THE
FLOAT32 INPUTS; no bias (the lin_z biases are folded into the MLP's own).  Every block, and the coarse and the fine MLP, has
weights of its own, so a block offset or an MLP mixed up shows.

Routes (csrc/encoder.hip run_pixel_linear): maps below 256 pixels run the 1x1-convolution path ("fallback"; its
conv_mfma_kernel instantiation is reported as 100 SPLIT + 10 NT + MT), larger ones the tiled GEMM in fp32 on scenes pinned to
F32 ("tiled_f32") and on split-f16 operands otherwise ("tiled_split").

Errors are max |got - ref| over a case's map divided by the float64 map's max |.|.

Bars.  Each bar is TWICE the largest error against float64 of a float32 restatement of the route's arithmetic over the cases
it is applied to (the factor of tests/stage_ref.py and tests/trunk_stage_ref.py: the kernels sum in another order than the
restatement), per K, since a sum's rounding grows with its length:
  fallback, tiled_f32   a float32 matmul, all cases of that K;
  tiled_split           the three-product split x1 w1 + x2 w1 + x1 w2 with x1 = f16(x), x2 = f16(x - x1) (numpy float16, round to
                        nearest even, denormals KEPT), each product a float32 matmul of the planes (a product of two f16 values
                        is exact in float32), summed in float32 -- over the ordinary-magnitude cases of that K on the tiled
                        routes (where the split kernel runs);
  envelope              the same split restatement on the ONE case per K whose latent has std 1e-3: there the second plane of
                        nearly every latent value has lost most of its bits to the f16 denormal spacing (2^-24), the split
                        arithmetic itself is far from float32, and the kernel is held to twice the emulation of THAT.
"A float32 matmul" is written out (mm32): every product rounded to float32 and added to the running float32 sum in k order, one
term at a time.  That is the order of the kernels (they walk k from 0 with one accumulator per output; the fallback's split-K
instantiation and the 16-wide f16 MFMA round LESS often), and it is the same on every CPU.  A BLAS matmul keeps a dozen
partial sums in vector lanes and blocks: its error does not grow with K (3e-7 .. 5e-7 at every K here) and would bound no
sequential float32 sum at K = 1792 -- the reasoning of tests/trunk_stage_ref.py for batch norm's pixel sums.
The figure behind every bar is recorded as *_ERR; the CPU test measures each again (within 10 % above, not below half).  The
kernels' own errors set nothing.

What a bar must see.  split_flushed() is the split restatement with f16 denormals flushed to zero in both planes -- what matrix
cores that did not honour denormals would compute.  The CPU test shows it at least 10 x above the split bar on every
ordinary-magnitude case: a bar that a flush would pass is not a bar.
"""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
HID = 512
TILE = 128                     # pixels per workgroup of the tiled GEMM
TILED_FROM = 2 * TILE          # first map size on the tiled routes
ROUTE_TILED_F32, ROUTE_TILED_SPLIT = 1, 2      # include/pnyolo.h PNY_PROJECTION_ROUTE_TILED_*; >= 111: a conv_mfma_kernel instantiation
F16_MIN_NORMAL = 2.0 ** -14

# ------------------------------------------------------------------------------------------------ cases
# (npix as ns, hl, wl) -> what it exercises
MAPS = {
    15: (1, 3, 5),         # fallback, below one 32-pixel tile
    255: (3, 5, 17),       # the fallback's upper edge
    256: (1, 16, 16),      # first tiled size, whole tiles
    257: (1, 1, 257),      # one live pixel in the last tile
    383: (1, 1, 383),      # 127 live pixels in the last tile
    270: (2, 9, 15),       # ragged tile at K = 1792
    5700: (3, 38, 50),     # DTU-like map, 68 live pixels in the last tile, at K = 512
}
KS = (128, 512, 1792)
STD_ORDINARY = (1.0, 0.05)     # at 0.05 almost every second plane is an f16 denormal
STD_ENVELOPE = 1e-3


def _case(npix, K, nvb, std):
    ns, hl, wl = MAPS[npix]
    assert ns * hl * wl == npix
    kind = "envelope" if std == STD_ENVELOPE else "ordinary"
    return dict(name="K%d_b%d_px%d_std%g" % (K, nvb, npix, std), K=K, nvb=nvb, ns=ns, hl=hl, wl=wl, npix=npix, std=std, kind=kind)


CASES = [_case(*c) for c in (
    # K = 128: every map size of the table but the two that belong to another K, view blocks 1 / 3 / 5, both magnitudes
    (15, 128, 1, 1.0), (15, 128, 3, 0.05),
    (255, 128, 3, 1.0), (255, 128, 1, 0.05),
    (256, 128, 1, 1.0), (256, 128, 5, 0.05),
    (257, 128, 3, 1.0), (257, 128, 1, 0.05),
    (383, 128, 5, 1.0), (383, 128, 3, 0.05),
    # K = 512: the fallback (its split-K instantiation), the first tiled size, the DTU-like map
    (15, 512, 3, 0.05), (255, 512, 1, 1.0),
    (256, 512, 3, 1.0), (256, 512, 1, 0.05),
    (5700, 512, 1, 0.05), (5700, 512, 3, 1.0),
    # K = 1792: the fallback, one live pixel in the last tile, the ragged two-view map
    (15, 1792, 1, 1.0), (257, 1792, 3, 0.05),
    (270, 1792, 1, 1.0), (270, 1792, 3, 0.05),
    # the envelope: one case per K, on a tiled map
    (257, 128, 3, STD_ENVELOPE), (256, 512, 1, STD_ENVELOPE), (270, 1792, 1, STD_ENVELOPE),
)]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def n_blocks_of(nvb):
    """The smallest model with nvb per-view blocks that a multi-view scene accepts (combine_layer < n_blocks)."""
    return nvb + 1


def expected_route(case, pinned_f32):
    """'fallback' below 256 pixels on either scene; else 'tiled_f32' on a scene pinned to F32 and 'tiled_split' on an AUTO one."""
    if case["npix"] < TILED_FROM:
        return "fallback"
    return "tiled_f32" if pinned_f32 else "tiled_split"


def route_name(code):
    return {ROUTE_TILED_F32: "tiled_f32", ROUTE_TILED_SPLIT: "tiled_split"}.get(code, "fallback" if code >= 111 else "unknown %d" % code)


# ------------------------------------------------------------------------------------------------ inputs
def weights(K, nvb, seed=0):
    """lin_z weights (2 MLPs [coarse, fine], nvb, 512, K) float32, std sqrt(2 / K), every matrix its own."""
    rs = np.random.RandomState(7100 + K + 17 * nvb + 1000 * seed)
    return (rs.standard_normal((2, nvb, HID, K)) * np.sqrt(2.0 / K)).astype(np.float32)


def latent(case, seed=0):
    """(ns, K, hl, wl) NCHW float32 of the case's magnitude."""
    rs = np.random.RandomState(7300 + sorted(BY_NAME).index(case["name"]) + 1000 * seed)
    return (rs.standard_normal((case["ns"], case["K"], case["hl"], case["wl"])) * case["std"]).astype(np.float32)


def rows_of(lat):
    """NCHW latent -> the GEMM's pixel rows (ns hl wl, K), p = (v hl + y) wl + x."""
    lat = np.asarray(lat)
    return np.ascontiguousarray(lat.transpose(0, 2, 3, 1).reshape(-1, lat.shape[1]))


def stacked(w):
    """(nvb, 512, K) -> (nvb 512, K): block b owns output columns [512 b, 512 b + 512)."""
    return np.ascontiguousarray(np.asarray(w).reshape(-1, w.shape[-1]))


# ------------------------------------------------------------------------------------------------ reference and restatements
def project64(x, w):
    """float64 on the float32 inputs: x (P, K), w (N, K) -> (P, N) numpy float64."""
    return (torch.from_numpy(np.array(x, dtype=np.float32)).to(F64) @ torch.from_numpy(np.array(w, dtype=np.float32)).to(F64).T).numpy()


def mm32(x, w, rows=128):
    """x (P, K) w (N, K)^T in float32, written out: every product rounded to float32 and added to the float32 sum IN k ORDER,
    one term at a time (no fused multiply-add, no partial sums) -- bit-reproducible on any CPU."""
    xt = torch.from_numpy(np.array(x, dtype=np.float32))
    wt = torch.from_numpy(np.array(w, dtype=np.float32)).T.contiguous()         # (K, N)
    P, K = xt.shape
    out = torch.empty(P, wt.shape[1], dtype=F32)
    for r0 in range(0, P, rows):                                                 # row blocks: the sums stay in cache
        xb = xt[r0:r0 + rows]
        acc = torch.zeros(xb.shape[0], wt.shape[1], dtype=F32)
        tmp = torch.empty_like(acc)
        for k in range(K):
            torch.mul(xb[:, k:k + 1], wt[k], out=tmp)
            acc.add_(tmp)
        out[r0:r0 + rows] = acc
    return out.numpy()


def project32(x, w):
    """The float32 restatement: a float32 matmul (mm32)."""
    return mm32(x, w)


def planes(a, flush=False):
    """a = a1 + a2 + (what two f16 planes cannot hold): a1 = f16(a), a2 = f16(a - a1), round to nearest even, as float32.
    flush: f16 denormals (|.| < 2^-14) become zero in both planes."""
    a = np.asarray(a, dtype=np.float32)
    a1 = a.astype(np.float16)
    if flush:
        a1 = np.where(np.abs(a1.astype(np.float32)) < F16_MIN_NORMAL, np.float16(0), a1)
    a1 = a1.astype(np.float32)
    a2 = (a - a1).astype(np.float16)          # a - a1 is exact in float32
    if flush:
        a2 = np.where(np.abs(a2.astype(np.float32)) < F16_MIN_NORMAL, np.float16(0), a2)
    return a1, a2.astype(np.float32)


def mm32_blas(x, w):
    return (torch.from_numpy(np.array(x, dtype=np.float32)) @ torch.from_numpy(np.array(w, dtype=np.float32)).T).numpy()


def project_split(x, w, flush=False, mm=mm32):
    """The split restatement: x1 w1 + x2 w1 + x1 w2 on f16 planes, float32 accumulation."""
    x1, x2 = planes(x, flush)
    w1, w2 = planes(w, flush)
    return (mm(x1, w1) + mm(x2, w1)) + mm(x1, w2)


def split_flushed(x, w):
    """... with f16 denormals flushed.  (Its error, 2e-4, is 100 x any summation order's: the products go through BLAS.)"""
    return project_split(x, w, flush=True, mm=mm32_blas)


def err(got, ref):
    """max |got - ref| over the float64 map's max |.|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "non-finite result"
    return float(np.abs(got - ref).max() / np.abs(ref).max())


_REF = {}


def reference(case, fine=0):
    """(pixel rows float32, stacked weights float32, float64 map) of a case, computed once and shared; read-only."""
    key = (case["name"], fine)
    if key not in _REF:
        x, w = rows_of(latent(case)), stacked(weights(case["K"], case["nvb"])[fine])
        r = project64(x, w)
        for a in (x, w, r):
            a.setflags(write=False)
        _REF[key] = (x, w, r)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ figures and bars
# *_ERR[K]: largest restatement error over the cases of that K the bar is applied to, measured on the CPU
# (tests/test_cpu_projection_ref.py prints them)
F32_ERR = {128: 5.69e-7, 512: 1.17e-6, 1792: 2.20e-6}
SPLIT_ERR = {128: 5.89e-7, 512: 1.09e-6, 1792: 2.13e-6}
ENVELOPE_ERR = {128: 1.63e-5, 512: 1.76e-5, 1792: 1.75e-5}       # latent std 1e-3: 15 .. 30 x the float32 figure
FLUSH_FACTOR = 10.0            # the flushed split restatement exceeds the split bar by at least this on every ordinary case


def bar(case, route):
    """The bar of a case's result on a route: twice the recorded figure of the route's restatement at the case's K."""
    K = case["K"]
    if route in ("fallback", "tiled_f32"):
        return 2.0 * F32_ERR[K]
    assert route == "tiled_split", route
    return 2.0 * (ENVELOPE_ERR if case["kind"] == "envelope" else SPLIT_ERR)[K]
