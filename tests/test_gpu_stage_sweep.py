"""
The renderer's stage kernels (csrc/render_kernels.hip: sample_coarse, composite, sample_fine, yolo_aggregate) through the C ABI
and the detection tail (csrc/detect.hip: cells_to_bboxes, nms, tp / fp / fn) through pixel_nerf_yolo_amd.util, swept over the
shapes, edges and ties where such kernels go wrong (-m gpu, real MI355X).

The MLP-free backward stages (csrc/mlp_bwd.hip: composite_bwd, yolo_aggregate_bwd, depth_grad_gather, locate_depth_samples)
follow, through their own entry points: the two float ones against the oracle under autograd, the two exact ones against a host
restatement, bit for bit.

Every float result is held to oracle/pnyolo_oracle.py evaluated in float64 on the float32 inputs, every index / integer result
of the detection tail to the oracle's list semantics (tests/stage_ref.py nms_fast, proven equal to orc.nms and to the
reference's captures in tests/test_cpu_stage_refs.py), exactly.  The inputs, the bars and where each bar comes from are in
tests/stage_ref.py; the CPU file shows that the float32 oracle itself meets every bar and no-flip condition on these inputs.
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
import stage_ref as sr
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import util as putil

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = sr.F32, sr.F64


def dev(x, device=DEV):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=device).contiguous()


def stream(device=DEV):
    return plib.stream_of(torch.device(device))


def bits(t):
    return np.ascontiguousarray(np.asarray(torch.as_tensor(t).cpu(), np.float32)).view(np.uint32)


def hip_coarse(rays, u, kc, lindisp):
    r, uu = dev(rays), dev(u)
    z = torch.full((r.shape[0], kc), float("nan"), device=DEV)
    plib.check(plib.load().pny_sample_coarse(plib.ptr(r), r.shape[0], kc, lindisp, plib.ptr(uu), 0, plib.ptr(z), stream()))
    torch.cuda.synchronize()
    return z.cpu()


def hip_composite(rays, z, samp, K, white, want=(True, True, True)):
    r, zz, s = dev(rays), dev(z), dev(samp)
    n = r.shape[0]
    w = torch.full((n, K), float("nan"), device=DEV) if want[0] else None
    rgb = torch.full((n, 3), float("nan"), device=DEV) if want[1] else None
    dep = torch.full((n,), float("nan"), device=DEV) if want[2] else None
    plib.check(plib.load().pny_composite(plib.ptr(r), plib.ptr(zz), plib.ptr(s), n, K, white, plib.ptr(w), plib.ptr(rgb),
                                         plib.ptr(dep), stream()))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (w, rgb, dep))


hip_fine = sr.hip_fine      # shared with the two-device child process


def hip_agg(raw, K, na):
    r = dev(raw)
    out = torch.full((r.shape[0], na, 7), float("nan"), device=DEV)
    plib.check(plib.load().pny_yolo_aggregate(plib.ptr(r), r.shape[0], K, na, plib.ptr(out), stream()))
    torch.cuda.synchronize()
    return out.cpu()


# --------------------------------------------------------------------------- sample_coarse
@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("kc", sr.COARSE_KC)
def test_sample_coarse_sweep(kc, lindisp):
    worst = 0.0
    for draws in sr.COARSE_DRAWS:
        for n in sr.N_LIST:
            rays, u = sr.coarse_case(n, kc, lindisp, draws)
            z = hip_coarse(rays, u, kc, lindisp)
            e = sr.err(z, sr.coarse_ref(rays, kc, u, lindisp, F64))
            worst = max(worst, e)
            assert e <= sr.COARSE_BAR, (draws, n, e)
            assert sr.rows_ascend_in_range(z, rays), (draws, n)             # sample_fine relies on ascending rows
            if (kc, lindisp) == sr.COARSE_EXACT:                              # the existing bar, where it holds today
                assert np.array_equal(bits(z), bits(sr.coarse_ref(rays, kc, u, lindisp, F32))), (draws, n)
    print("sample_coarse kc=%d lindisp=%d: max |err| vs float64 %.3e (bar %.1e)" % (kc, lindisp, worst, sr.COARSE_BAR))


# --------------------------------------------------------------------------- composite
def check_composite(fam, n, K, white, want=(True, True, True)):
    rays, z, samp = sr.composite_case(fam, n, K)
    got = hip_composite(rays, z, samp, K, white, want)
    ref = sr.composite_ref(rays, z, samp, white, F64)
    bar, worst = sr.composite_bar(K), 0.0
    for name, g, r in zip(("weights", "rgb", "depth"), got, ref):
        if g is None:
            continue
        e = sr.err(g, r)
        worst = max(worst, e)
        assert e <= bar, (fam, n, K, white, name, e)
    if got[0] is not None:
        assert float(got[0].sum(-1).max()) <= 1.0 + bar, (fam, n, K)
        if fam == "zero_sigma":
            assert float(got[0].abs().max()) == 0.0                           # weights exactly 0
        sl = sr.behind(fam, K)
        if sl is not None:      # behind an opaque sample T = 1e-10 x ..., as the reference's `+ 1e-10` gives it
            e = sr.err(got[0][:, sl] * 1e10, ref[0][:, sl] * 1e10)
            assert e <= sr.OPAQUE_SCALED_BAR, (fam, n, K, "behind the opaque sample", e)
    if fam == "zero_sigma" and got[1] is not None:
        assert bool((got[1] == float(white)).all())                           # rgb exactly 1 or 0
    return worst


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("K", sr.COMPOSITE_K)
def test_composite_sweep(K, white):
    worst = 0.0
    for fam in sr.composite_families(K):
        for n in sr.N_LIST + ((1025,) if fam == "random" and K == 129 else ()):
            worst = max(worst, check_composite(fam, n, K, white))
    print("composite K=%d white=%d: max |err| vs float64 %.3e (bar %.1e)" % (K, white, worst, sr.composite_bar(K)))


@pytest.mark.parametrize("white", [0, 1])
def test_composite_null_outputs(white):
    """Every combination of null and non-null weights / rgb / depth outputs (all null: the launch must simply succeed)."""
    for K in (65, 200):
        for mask in range(8):
            want = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
            check_composite("random", 5, K, white, want)
            check_composite("opaque@63", 3, K, white, want)


# --------------------------------------------------------------------------- sample_fine
def check_fine_rows(zo, c, kc):
    assert not bool(torch.isnan(zo).any())
    assert bool((zo[:, 1:] >= zo[:, :-1]).all()), "output not ascending"
    assert sr.contains_rows(zo.numpy(), c["zc"]), "a coarse depth is missing from the merged row"


@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("shape", sr.FINE_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_sample_fine_sweep(shape, lindisp):
    """No ray is left out: the importance draws are conditioned (stage_ref.condition_draws) so that the bin of every draw is
    beyond the reach of float32 rounding, and then EVERY row matches the float64 result within the bar."""
    kc, kf, kfd = shape
    worst = 0.0
    for pat in sr.FINE_PATTERNS:
        for n in sr.N_LIST:
            c = sr.fine_case(n, kc, kf, kfd, lindisp, pat)
            zo = hip_fine(c, kc, kf, kfd, lindisp)
            e = sr.err(zo, sr.fine_ref(c, kc, kf, kfd, lindisp, F64))
            worst = max(worst, e)
            assert e <= sr.fine_bar(lindisp), (pat, n, e, "margin %.2e, %d draws moved" % (c["margin"], c["moved"]))
            check_fine_rows(zo, c, kc)
    print("sample_fine %s lindisp=%d: max |err| vs float64 %.3e (bar %.1e)" % (shape, lindisp, worst, sr.fine_bar(lindisp)))


@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("kind", ["eq4", "eq16", "eq64", "mix"])
def test_sample_fine_draws_on_cdf_edges(kind, lindisp):
    """Dyadic cdf (the same bits under every summation order), draws exactly on its edges: u = 0 -> bin 0, an interior edge ->
    the upper bin (right=True), the largest float below 1 -> the last bin.  Bit for bit the float32 oracle; with u2 = 0 the
    new depths also tie with coarse depths."""
    for u2 in (0.0, 0.5):
        c, kc, kimp, bins = sr.dyadic_case(kind, u2, lindisp)
        zo = hip_fine(c, kc, kimp, 0, lindisp)
        ref = sr.fine_ref(c, kc, kimp, 0, lindisp, F32)
        assert np.array_equal(bits(zo), bits(ref)), (kind, u2, (zo - ref).abs().max())
        check_fine_rows(zo, c, kc)


@pytest.mark.parametrize("kind", ["std0", "clamp", "coarse_bits"])
def test_sample_fine_depth_ties(kind):
    """Equal depth samples (depth_std = 0; clamped to near / far) and a depth sample with a coarse depth's bits: the output is
    torch.sort of the concatenation bit for bit."""
    for n in (5, 257):
        c, std = sr.depth_tie_case(kind, n=n)
        zo = hip_fine(c, 64, 32, 16, 0, depth_std=std)
        rays = sr.t32(c["rays"])
        zf = orc.sample_fine(rays, sr.t32(c["w"]), sr.t32(c["u"]), sr.t32(c["u2"]), 64)
        zd = orc.sample_fine_depth(rays, sr.t32(c["depth"]), sr.t32(c["g"]), std)
        # the importance depths are the kernel's own if a bin differs in the last bit of a cdf: take them from the float64 check
        assert sr.err(zo, sr.fine_ref(c, 64, 32, 16, 0, F64, depth_std=std)) <= sr.FINE_BAR
        ref = torch.sort(torch.cat([sr.t32(c["zc"]), zf, zd], -1), -1)[0]
        assert np.array_equal(bits(zo), bits(ref)), (kind, n, float((zo - ref).abs().max()))
        check_fine_rows(zo, c, 64)


def test_sample_fine_refuses_what_does_not_fit():
    kc, kf, kfd = sr.FINE_REFUSED
    small = torch.zeros(8, device=DEV)
    rc = plib.load().pny_sample_fine(plib.ptr(small), plib.ptr(small), plib.ptr(small), plib.ptr(small), 1, kc, kf, kfd, 0.01, 0,
                                     plib.ptr(small), plib.ptr(small), None, 0, plib.ptr(small), stream())
    assert rc != 0 and b"too large" in plib.load().pny_last_error()
    with pytest.raises(plib.PnyError):
        plib.check(rc)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- yolo_aggregate
@pytest.mark.parametrize("na", sr.AGG_ANCHORS)
@pytest.mark.parametrize("K", sr.AGG_K)
def test_yolo_aggregate_sweep(K, na):
    worst = 0.0
    for fam in sr.agg_families(K):
        for n in sr.N_LIST + ((1000,) if fam == "random" and K == 65 else ()):
            raw = sr.agg_case(fam, n, K, na)
            out = hip_agg(raw, K, na)
            ref = sr.agg_ref(raw, na, F64)
            e = sr.err(out, ref) / sr.agg_scale(ref)
            worst = max(worst, e)
            assert e <= sr.AGG_BAR, (fam, n, e)
            if fam == "all_low":
                # sum p ~ 0 and the 1e-5 dominates: without it the quotient is 0 / 0
                assert not bool(torch.isnan(out).any()) and float(out[..., 1:].abs().max()) < 1e-20
    print("yolo_aggregate K=%d A=%d: max |err| / scale vs float64 %.3e (bar %.1e)" % (K, na, worst, sr.AGG_BAR))


# --------------------------------------------------------------------------- detection tail
@pytest.mark.parametrize("shape", sr.CELL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_cells_to_bboxes_sweep(shape):
    h, w, A = shape
    anchors = torch.from_numpy(sr.ANCHORS[:A])
    for is_pred in (True, False):
        for fam in ("random", "class_ties", "extreme"):
            cells = sr.cells_case(h, w, A, is_pred, fam)
            out = putil.convert_cells_to_bboxes(dev(cells), anchors, h, w, is_pred, as_tensor=True).cpu()
            assert out.shape == (2, h * w * A, 6)
            for b in range(2):
                r64 = sr.cells_ref(cells[b], sr.ANCHORS[:A], h, w, is_pred, F64)
                r32 = sr.cells_ref(cells[b], sr.ANCHORS[:A], h, w, is_pred, F32)
                e = sr.check_boxes(out[b], r64, r32)
                assert e <= sr.BOX_BAR, (is_pred, fam, b, e)
                assert np.array_equal(out[b][:, 0].numpy(), r64[:, 0].numpy().astype(np.float32))   # class: the first maximum
                assert np.array_equal(bits(out[b][:, 1]), bits(cells[b].reshape(-1, cells.shape[-1])[:, 0]))   # score: copied
    lst = putil.convert_cells_to_bboxes(dev(sr.cells_case(h, w, A, False, "random")), anchors, h, w, False)
    assert isinstance(lst, list) and len(lst) == 2 and len(lst[0]) == h * w * A and len(lst[0][0]) == 6


def test_cells_to_bboxes_refuses_bad_shapes():
    five = torch.ones(5, 2)
    with pytest.raises(plib.PnyError):
        putil.convert_cells_to_bboxes(torch.zeros(2, 3, 3, 5, 7, device=DEV), five, 3, 3, True, as_tensor=True)
    with pytest.raises(plib.PnyError):
        putil.convert_cells_to_bboxes(torch.zeros(2, 0, 3, 2, 7, device=DEV), five[:2], 0, 3, True, as_tensor=True)
    torch.cuda.synchronize()


def check_nms(boxes, iou_t, conf_t, name):
    ref_kept, ref_hi, ref_above = sr.nms_fast(boxes, iou_t, conf_t)
    kept, hi, above = putil.nms(dev(boxes), iou_t, conf_t, as_tensor=True)
    kept = kept.cpu().numpy()
    assert kept.shape[0] == ref_kept.shape[0] and above == ref_above, (name, kept.shape[0], ref_kept.shape[0], above, ref_above)
    assert np.float32(hi).view(np.uint32) == np.float32(ref_hi).view(np.uint32), name
    assert np.array_equal(kept, ref_kept), (name, "first difference at row %d" % int(np.nonzero((kept != ref_kept).any(1))[0][0]))
    return kept


@pytest.mark.parametrize("name", sorted(sr.nms_cases()))
def test_nms_sweep(name):
    boxes, iou_t, conf_t = sr.nms_cases()[name]
    kept = check_nms(boxes, iou_t, conf_t, name)
    if boxes.shape[0] <= 600:        # the reference's list form: list in, list out
        lst, hi, above = putil.nms(boxes.tolist(), iou_t, conf_t, device=DEV)
        assert isinstance(lst, list) and np.array_equal(np.array(lst, np.float32).reshape(-1, 6), kept)


def test_nms_iou_threshold_is_strict():
    b, v, below = sr.iou_pair_case()
    assert len(check_nms(b, v, 0.1, "iou == threshold")) == 2            # not suppressed: the test is a strict >
    assert len(check_nms(b, below, 0.1, "threshold one float below")) == 1


def test_nms_limit_and_time():
    """n = 8192 (76.8 KB of dynamic LDS) launches and matches; 8193 is refused without a launch.  Prints both times."""
    boxes, iou_t, conf_t = sr.nms_cases()["cluster%d" % sr.NMS_MAX]
    t0 = time.time()
    ref_kept = sr.nms_fast(boxes, iou_t, conf_t)[0]
    t_ref = time.time() - t0
    b = dev(boxes)
    n = b.shape[0]
    kept = torch.empty(n, 6, device=DEV)
    meta = torch.zeros(2, device=DEV, dtype=torch.int32)
    hc = torch.empty(1, device=DEV)
    L = plib.load()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(2):             # the second call is the timed one (the first loads the code object)
        ev[0].record()
        plib.check(L.pny_nms(plib.ptr(b), n, iou_t, conf_t, plib.ptr(kept), C.c_void_p(meta.data_ptr()), plib.ptr(hc), stream()))
        ev[1].record()
        torch.cuda.synchronize()
    m = int(meta[0])
    assert m == ref_kept.shape[0] and np.array_equal(kept[:m].cpu().numpy(), ref_kept)
    print("nms n=8192: %d survivors, kernel %.2f ms, numpy reference %.0f ms" % (m, ev[0].elapsed_time(ev[1]), 1e3 * t_ref))
    with pytest.raises(plib.PnyError):
        putil.nms(dev(np.concatenate([boxes, boxes[:1]])), iou_t, conf_t, as_tensor=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(sr.match_cases()))
def test_tp_fp_fn_sweep(name):
    t, p, nms_iou, nms_t, m = sr.match_cases()[name]
    ref = sr.tp_fp_fn_fast(t, p, nms_iou, nms_t, m)
    assert putil.calculate_tp_fp_fn(dev(t), dev(p), nms_iou, nms_t, m) == ref, name
    assert putil.calculate_tp_fp_fn(t.tolist(), p.tolist(), nms_iou, nms_t, m, device=DEV) == ref, name


# =========================================================================== backward stages (csrc/mlp_bwd.hip)
def opt_dev(x):
    return None if x is None else dev(x)


def hip_composite_bwd(rays, z, samp, K, white, g_rgb, g_depth, g_w, want_dz=True):
    r, zz, s = dev(rays), dev(z), dev(samp)
    n = r.shape[0]
    a, b, c = opt_dev(g_rgb), opt_dev(g_depth), opt_dev(g_w)
    d_samp = torch.full((n, K, 4), float("nan"), device=DEV)
    d_z = torch.full((n, K), float("nan"), device=DEV) if want_dz else None
    plib.check(plib.load().pny_composite_backward(plib.ptr(r), plib.ptr(zz), plib.ptr(s), n, K, white, plib.ptr(a), plib.ptr(b),
                                                  plib.ptr(c), plib.ptr(d_samp), plib.ptr(d_z), stream()))
    torch.cuda.synchronize()
    return d_samp.cpu(), None if d_z is None else d_z.cpu()


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("K", sr.COMPOSITE_BWD_K)
def test_composite_backward_sweep(K, white):
    """composite_bwd_kernel per ray against autograd through the oracle in float64: every family of the forward sweep, every n
    tail, K to the accepted maximum; for one family per K also each subset of upstream gradients that
    test_composite_backward_vs_autograd leaves out (all NULL: exactly zero) and d_z_dev = NULL."""
    worst = [0.0, 0.0, 0.0]
    for fam in sr.composite_families(K):
        for n in sr.composite_bwd_n(K):
            rays, z, samp = sr.composite_bwd_case(fam, n, K)
            grads = sr.composite_grads(fam, n, K)
            subsets = ((1, 1, 1),) + (sr.GRAD_SUBSETS if fam == sr.subset_family(K) else ())
            for sub in subsets:
                g = [v if on else None for v, on in zip(grads, sub)]
                ref = sr.composite_bwd_ref(rays, z, samp, white, *g, dtype=F64)
                d_samp, d_z = hip_composite_bwd(rays, z, samp, K, white, *g)
                e = sr.check_composite_bwd(fam, n, K, d_samp, d_z, ref)
                worst = [max(a, b) for a, b in zip(worst, e)]
                if sub == (0, 0, 0):
                    assert float(d_samp.abs().max()) == 0.0 and float(d_z.abs().max()) == 0.0, (fam, n, K)
                if sub == (1, 1, 1) and fam == sr.subset_family(K):          # d_z not asked for: d_sample is the same, bit for bit
                    only = hip_composite_bwd(rays, z, samp, K, white, *g, want_dz=False)[0]
                    assert np.array_equal(bits(only), bits(d_samp)), (fam, n, K, "d_z_dev = NULL")
    print("composite backward K=%d white=%d: worst per-ray error vs float64 d_sample %.3e (bar %.1e), d_z %.3e (bar %.1e), "
          "behind an opaque sample x 1e10 %.3e (bar %.1e)" % (K, white, worst[0], sr.COMPOSITE_BWD_BAR_DSAMPLE, worst[1],
                                                               sr.composite_bwd_dz_bar(K), worst[2], sr.COMPOSITE_BWD_BAR_BEHIND))


def hip_agg_bwd(raw, g, K, na):
    r, gg = dev(raw), dev(g)
    d = torch.full((r.shape[0], K, na * 7), float("nan"), device=DEV)
    plib.check(plib.load().pny_yolo_aggregate_backward(plib.ptr(r), plib.ptr(gg), r.shape[0], K, na, plib.ptr(d), stream()))
    torch.cuda.synchronize()
    return d.cpu()


@pytest.mark.parametrize("na", sr.AGG_ANCHORS)
@pytest.mark.parametrize("K", sr.AGG_K)
def test_yolo_aggregate_backward_sweep(K, na):
    """yolo_aggregate_bwd_kernel per (ray, anchor) against autograd through the oracle in float64; in the `tie` family the
    maximum's gradient reaches the first tied index and no other."""
    worst = 0.0
    for fam in sr.agg_bwd_families(K):
        for n in sr.N_LIST:
            raw, g = sr.agg_bwd_case(fam, n, K, na)
            ref = sr.agg_bwd_ref(raw, g, na, F64)
            got = hip_agg_bwd(raw, g, K, na)
            e = sr.agg_row_err(got, ref, na)
            worst = max(worst, e)
            assert e <= sr.AGG_BWD_BAR, (fam, n, K, na, e)
            if fam == "tie" and K > 1:
                rows = sr.check_tie(got, ref, raw, g, K, na)
                assert n < 257 or rows > n * na // 2, (K, na, n, rows)
    print("yolo_aggregate backward K=%d A=%d: worst per-(ray, anchor) error vs float64 %.3e (bar %.1e)" % (K, na, worst, sr.AGG_BWD_BAR))


def hip_gather(sel, dz, g_in):
    s = torch.as_tensor(sel, dtype=torch.int32, device=DEV).contiguous()
    d, gi = dev(dz), opt_dev(g_in)
    n, kfd = sel.shape
    out = torch.full((n,), float("nan"), device=DEV)
    plib.check(plib.load().pny_depth_grad_gather(C.c_void_p(s.data_ptr()), plib.ptr(d), plib.ptr(gi), n, kfd, plib.ptr(out), stream()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("kfd", sr.GATHER_KFD)
def test_depth_grad_gather_sweep(kfd):
    """depth_grad_gather_kernel: the sum over a ray's located depth samples in sample order, bit for bit the sequential float32
    sum -- across the `j0 += 64` chunks, with a partial last chunk, with wholly clamped rays, with and without g_in."""
    cases = 0
    for pat in sr.GATHER_PATTERNS:
        for n in sr.N_LIST:
            sel, dz, g_in = sr.gather_case(pat, n, kfd)
            for gi in (None, g_in):
                got = hip_gather(sel, dz, gi)
                ref = sr.gather_ref(sel, dz, gi)
                assert np.array_equal(bits(got), bits(ref)), (pat, n, kfd, gi is not None, float(np.abs(got.numpy() - ref).max()))
                cases += 1
    print("depth_grad_gather kfd=%d: %d cases bit-identical to the sequential float32 sum" % (kfd, cases))


def hip_locate(c, z_fine, kt, kfd, depth_std, g=None, seed=0):
    r, d, zf = dev(c["rays"]), dev(c["depth"]), dev(z_fine)
    gg = opt_dev(g)
    n = r.shape[0]
    sel = torch.full((n, kfd), -7, dtype=torch.int32, device=DEV)
    plib.check(plib.load().pny_locate_depth_samples(plib.ptr(r), plib.ptr(d), plib.ptr(gg), seed, plib.ptr(zf), n, kt, kfd, depth_std,
                                                    C.c_void_p(sel.data_ptr()), stream()))
    torch.cuda.synchronize()
    return sel.cpu().numpy()


@pytest.mark.parametrize("shape", sr.LOCATE_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_locate_depth_samples_sweep(shape):
    """locate_depth_samples_kernel on the real sorted output of pny_sample_fine: every robust sample strictly inside (near, far)
    is found on its own ray at the first position of its value, every clamped one -- zz == near exactly included -- gives -1."""
    kc, kf, kfd = shape
    left_out = total = 0
    for n in sr.LOCATE_N:
        c = sr.locate_case(n, kc, kf, kfd)
        for std in sr.LOCATE_STD:
            z_fine = hip_fine(c, kc, kf, kfd, 0, depth_std=std)
            sel = hip_locate(c, z_fine, kc + kf, kfd, std, g=c["g"])
            assert bool((sel[0] == -1).all()), "zz == near exactly was located"
            left_out += sr.check_located(sel, z_fine.numpy(), c, std, kc + kf)
            total += sel.size
    print("locate_depth_samples %s: %d samples exact, %d within %.0e of a bound left out" % (shape, total - left_out, left_out, sr.ROBUST))


def test_locate_depth_samples_seeded():
    """g_dev = NULL: the kernel re-creates the forward's seeded normals (normal_at is compiled into render_kernels.hip and into
    mlp_bwd.hip).  Every located position holds a depth strictly inside (near, far), and a ray has as many located samples as the
    oracle's generator puts strictly inside."""
    kc, kf, kfd = sr.LOCATE_SEEDED_SHAPE
    n, std, kt = 257, 0.05, kc + kf
    c = sr.locate_case(n, kc, kf, kfd)
    seeded = dict(c, g=np.zeros((n, 0), np.float32))                     # no explicit normals: pny_sample_fine draws them from the seed
    z_fine = sr.hip_fine(seeded, kc, kf, kfd, 0, depth_std=std, seed=sr.LOCATE_SEED)
    sel = hip_locate(c, z_fine, kt, kfd, std, g=None, seed=sr.LOCATE_SEED)
    g = orc.seeded_draws(sr.LOCATE_SEED, n, kc, kf, kfd)["g_depth"]
    sr.check_located(sel, z_fine.numpy(), c, std, kt, g=g)
    zz, inside, checked = sr.locate_expect(c, std, g)
    val = z_fine.numpy().reshape(-1)[sel[sel >= 0]]
    near, far = (np.float32(v) for v in sr.near_far(0))
    assert bool(((val > near) & (val < far)).all())
    rows = checked.all(1)
    assert int(rows.sum()) > 0.9 * n and np.array_equal((sel >= 0).sum(1)[rows], inside.sum(1)[rows])
    other = hip_locate(c, z_fine, kt, kfd, std, g=None, seed=sr.LOCATE_SEED + 1)        # another seed finds next to nothing
    assert int((other >= 0).sum()) < 0.02 * int((sel >= 0).sum())


def test_backward_stages_refuse_bad_arguments():
    L = plib.load()
    one = torch.zeros(64, device=DEV)
    p, st = plib.ptr(one), stream()
    isel = C.c_void_p(torch.zeros(64, dtype=torch.int32, device=DEV).data_ptr())
    K = sr.COMPOSITE_BWD_KMAX + 1
    assert L.pny_composite_backward(p, p, p, 1, K, 1, p, p, p, p, p, st) == -1 and b"too many samples" in L.pny_last_error()
    assert L.pny_composite_backward(p, p, p, -1, 4, 1, p, p, p, p, p, st) == -1
    assert L.pny_composite_backward(p, p, p, 1, 0, 1, p, p, p, p, p, st) == -1
    for miss in range(3):
        a = [p, p, p]
        a[miss] = None
        assert L.pny_composite_backward(a[0], a[1], a[2], 1, 4, 1, p, p, p, p, p, st) == -1
    assert L.pny_composite_backward(p, p, p, 1, 4, 1, p, p, p, None, p, st) == -1
    assert L.pny_composite_backward(None, None, None, 0, 4, 1, None, None, None, None, None, st) == 0          # n = 0: no launch
    for bad in ((p, p, -1, 4, 3, p), (p, p, 1, 0, 3, p), (p, p, 1, 4, 0, p), (None, p, 1, 4, 1, p), (p, None, 1, 4, 1, p), (p, p, 1, 4, 1, None)):
        assert L.pny_yolo_aggregate_backward(*bad, st) == -1 and b"pny_yolo_aggregate_backward" in L.pny_last_error(), bad
    assert L.pny_yolo_aggregate_backward(None, None, 0, 4, 3, None, st) == 0
    for bad in ((isel, p, p, -1, 4, p), (isel, p, p, 1, -1, p), (None, p, p, 1, 4, p), (isel, None, p, 1, 4, p), (isel, p, p, 1, 4, None)):
        assert L.pny_depth_grad_gather(*bad, st) == -1 and b"pny_depth_grad_gather" in L.pny_last_error(), bad
    assert L.pny_depth_grad_gather(None, None, None, 0, 4, None, st) == 0
    ok = [p, p, p, 0, p, 1, 8, 4, 0.01, isel]
    for i, v in ((5, -1), (6, 0), (7, -1), (7, 9), (0, None), (1, None), (4, None), (9, None), (5, 2 ** 31 // 8 + 1)):
        bad = list(ok)
        bad[i] = v
        assert L.pny_locate_depth_samples(*bad, st) == -1 and b"pny_locate_depth_samples" in L.pny_last_error(), (i, v)
    assert L.pny_locate_depth_samples(None, None, None, 0, None, 0, 8, 4, 0.01, None, st) == 0
    with pytest.raises(plib.PnyError):
        plib.check(L.pny_locate_depth_samples(*ok[:5], -1, *ok[6:], st))
    torch.cuda.synchronize()
    assert float(one.abs().max()) == 0.0                                  # nothing was launched on the refused calls


# --------------------------------------------------------------------------- a second device in the same process
def test_large_lds_launches_on_two_devices():
    """The kernels that raise their dynamic-LDS limit (nms at n = 8192, sample_fine at (1024, 512, 256)) on device 0 and then
    on device 1 of ONE fresh process: the raised limit is kept per device."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stage_two_devices_worker.py")
    res = subprocess.run([sys.executable, worker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "TWO_DEVICES_OK" in res.stdout, res.stdout[-4000:]
