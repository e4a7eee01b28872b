"""
CPU side of the stage-kernel and detection-tail sweeps (tests/stage_ref.py, tests/test_gpu_stage_sweep.py): what the GPU tests
take for granted is established here, without a GPU.
  * the bars: the float32 oracle's error against the float64 oracle on every case of the sweep is measured again and held to
    the figure each bar in stage_ref.py was derived from;
  * the chosen inputs: on them the float32 oracle itself ascends, stays in range, never flips an importance bin and meets
    the bars -- so a kernel that misses them is wrong, not unlucky;
  * the dyadic weights give the same cdf bits under every summation order, and the draws on its edges land where
    searchsorted(right=True) puts them;
  * stage_ref.nms_fast == orc.nms == the reference's captured outputs, and the clustered case exercises skip-after-remove.
"""
import os
import time

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
import stage_ref as sr

F32, F64 = sr.F32, sr.F64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


HELD_SLACK = 1.1    # torch's float32 sum / cumsum may be vectorised otherwise on another CPU or build: the last digit may move


def held(name, measured, recorded):
    """A measured float32-oracle error against the figure recorded in stage_ref.py (the bars are twice the RECORDED figure,
    whatever is measured here): within 10 % above it, not below half of it."""
    print("%s: float32 oracle vs float64 %.3e (recorded %.3e)" % (name, measured, recorded))
    assert measured <= HELD_SLACK * recorded, "%s: %.3e exceeds the recorded %.3e" % (name, measured, recorded)
    assert measured >= 0.5 * recorded, "%s: recorded %.3e is more than twice the measured %.3e" % (name, recorded, measured)


def test_coarse_fp32_oracle_error_and_order():
    worst = 0.0
    for lindisp in (0, 1):
        for kc in sr.COARSE_KC:
            for draws in sr.COARSE_DRAWS:
                for n in sr.N_LIST:
                    rays, u = sr.coarse_case(n, kc, lindisp, draws)
                    z32, z64 = sr.coarse_ref(rays, kc, u, lindisp, F32), sr.coarse_ref(rays, kc, u, lindisp, F64)
                    worst = max(worst, sr.err(z32, z64))
                    assert sr.rows_ascend_in_range(z64, rays), (kc, lindisp, draws, n)
                    assert sr.rows_ascend_in_range(z32, rays), (kc, lindisp, draws, n)
    held("sample_coarse", worst, sr.COARSE_ERR32)


def test_composite_fp32_oracle_error():
    small = large = opaque = 0.0
    for K in sr.COMPOSITE_K:
        for fam in sr.composite_families(K):
            for n in sr.N_LIST + ((1025,) if fam == "random" and K == 129 else ()):
                rays, z, samp = sr.composite_case(fam, n, K)
                for white in (0, 1):
                    r32, r64 = sr.composite_ref(rays, z, samp, white, F32), sr.composite_ref(rays, z, samp, white, F64)
                    e = max(sr.err(a, b) for a, b in zip(r32, r64))
                    if K <= 96:
                        small = max(small, e)
                    else:
                        large = max(large, e)
                    assert float(r32[0].sum(-1).max()) <= 1.0 + sr.composite_bar(K)
                    assert float(r64[0].sum(-1).max()) <= 1.0 + 1e-7           # the +1e-10 per sample lets the exact sum pass 1 by K x 1e-10
                    if fam == "zero_sigma":
                        assert float(r64[0].abs().max()) == 0.0 and bool((r64[1] == float(white)).all())
                    sl = sr.behind(fam, K)
                    if sl is not None:
                        opaque = max(opaque, sr.err(r32[0][:, sl] * 1e10, r64[0][:, sl] * 1e10))
                        assert 0.01 < float(r64[0][:, sl].max()) * 1e10 <= 1.0      # T = 1e-10 x ..., alphas of order one
    print("composite float32 oracle errors: K <= 96 %.3e, K > 96 %.3e, behind opaque x 1e10 %.3e" % (small, large, opaque))
    held("composite, K <= 96", small, sr.COMPOSITE_ERR32_SMALL)
    held("composite, K > 96", large, sr.COMPOSITE_ERR32_LARGE)
    held("composite, weights behind an opaque sample x 1e10", opaque, sr.OPAQUE_ERR32)
    # transmittance underflows within the first chunk of a multi-chunk ray (float32), not in float64
    rays, z, samp = sr.composite_case("underflow", 4, 192)
    w32, w64 = sr.composite_ref(rays, z, samp, 1, F32)[0], sr.composite_ref(rays, z, samp, 1, F64)[0]
    assert float(w32[:, 24:].abs().max()) == 0.0 and 0.0 < float(w64[:, 24:64].max()) < 1e-45


def test_fine_fp32_oracle_never_flips_on_the_conditioned_draws():
    worst, margins = 0.0, {}
    for kc, kf, kfd in sr.FINE_SHAPES:
        for lindisp in (0, 1):
            for pat in sr.FINE_PATTERNS:
                for n in sr.N_LIST:
                    c = sr.fine_case(n, kc, kf, kfd, lindisp, pat)
                    z32, z64 = sr.fine_ref(c, kc, kf, kfd, lindisp, F32), sr.fine_ref(c, kc, kf, kfd, lindisp, F64)
                    assert z64.shape == (n, kc + kf)
                    # NO ray is left out: every row of the float32 oracle is within the bar of the float64 one
                    e = sr.err(z32, z64)
                    assert e <= sr.fine_bar(lindisp), (kc, kf, kfd, lindisp, pat, n, e)
                    worst = max(worst, e)
                    if kf - kfd > 0:
                        assert sr.edge_distance(c["w"], c["u"]) > c["margin"] >= 0.0     # 0 only at kc = 1 (one bin, cdf exact)
                        margins[(kc, kf, kfd)] = max(margins.get((kc, kf, kfd), 0.0), c["margin"])
                    assert sr.contains_rows(z32.numpy(), c["zc"])
    held("sample_fine", worst, sr.FINE_ERR32)
    print("margins (4 x max |sequential float32 cdf - float64 cdf|):", {k: "%.2e" % v for k, v in margins.items()})
    # a sequential float32 sum of kc near-equal terms rounds the same way every time: up to 1.7e-5 off at kc = 1024.  Every ray
    # still has a bin wider than 2.5 margins to move a draw into (condition_draws asserts it)
    assert max(margins.values()) < 1e-4


@pytest.mark.parametrize("kind", ["eq4", "eq16", "eq64", "mix"])
def test_dyadic_cdf_is_exact_and_edges_land_right(kind):
    w, ks = sr.dyadic_weights(kind)
    q = w + np.float32(1e-5)
    assert q.dtype == np.float32 and np.array_equal(q.astype(np.float64), [2.0 ** -k for k in ks])
    exact = np.concatenate([[0.0], np.cumsum([2.0 ** -k for k in ks])])
    assert exact[-1] == 1.0
    assert np.array_equal(sr.cdf32_sequential(w[None])[0].astype(np.float64), exact)
    assert np.abs(sr.cdf64(w[None])[0] - exact).max() < 1e-8           # float64 adds the DOUBLE 1e-5 to fl32(2^-k - 1e-5f): not exact
    tw = torch.from_numpy(w)[None] + 1e-5                              # torch float32, its own (vectorised) summation order
    cdf = torch.cumsum(tw / tw.sum(-1, keepdim=True), -1)
    assert np.array_equal(cdf[0].numpy().astype(np.float64), exact[1:])
    for lindisp in (0, 1):
        for u2 in (0.0, 0.5):
            c, kc, kimp, bins = sr.dyadic_case(kind, u2, lindisp)
            near, far = (np.float32(v) for v in sr.near_far(lindisp))
            t = (bins.astype(np.float32) + np.float32(u2)) / np.float32(kc)
            one = np.float32(1)
            zn = near * (one - t) + far * t if not lindisp else one / (one / near * (one - t) + one / far * t)
            got = orc.sample_fine(sr.t32(c["rays"]), sr.t32(c["w"]), sr.t32(c["u"]), sr.t32(c["u2"]), kc, bool(lindisp))
            assert np.array_equal(got.numpy(), np.tile(zn, (got.shape[0], 1)))        # bin 0 / the upper bin / the last bin
            if u2 == 0.0 and not lindisp:
                assert np.isin(zn[:-1], c["zc"][0]).all()                             # and the new depths TIE with coarse depths


@pytest.mark.parametrize("kind", ["std0", "clamp", "coarse_bits"])
def test_depth_tie_cases_really_tie(kind):
    c, std = sr.depth_tie_case(kind)
    zd = orc.sample_fine_depth(sr.t32(c["rays"]), sr.t32(c["depth"]), sr.t32(c["g"]), std).numpy()
    assert np.array_equal(zd, np.repeat(zd[:, :1], zd.shape[1], 1))                  # all depth samples of a ray equal
    if kind == "clamp":
        assert set(np.unique(zd)) == {np.float32(0.8), np.float32(1.8)}
    if kind == "coarse_bits":
        assert all(zd[r, 0] in c["zc"][r] for r in range(zd.shape[0]))


def test_aggregate_fp32_oracle_error():
    worst = 0.0
    for K in sr.AGG_K:
        for na in sr.AGG_ANCHORS:
            for fam in sr.agg_families(K):
                for n in sr.N_LIST + ((1000,) if fam == "random" and K == 65 else ()):
                    raw = sr.agg_case(fam, n, K, na)
                    r32, r64 = sr.agg_ref(raw, na, F32), sr.agg_ref(raw, na, F64)
                    worst = max(worst, sr.err(r32, r64) / sr.agg_scale(r64))
                    if fam == "all_low":
                        assert float(r64[..., 1:].abs().max()) < 1e-30                # sum p ~ 0: the 1e-5 dominates
    held("yolo_aggregate", worst, sr.AGG_ERR32)


def test_cells_ref_is_the_oracle_and_its_fp32_error():
    worst = 0.0
    for h, w, A in sr.CELL_SHAPES:
        for is_pred in (True, False):
            for fam in ("random", "class_ties", "extreme"):
                cells = sr.cells_case(h, w, A, is_pred, fam)
                for b in range(cells.shape[0]):
                    r32 = sr.cells_ref(cells[b], sr.ANCHORS[:A], h, w, is_pred, F32)
                    o32 = orc.cells_to_bboxes(cells[b], sr.ANCHORS[:A], h, w, is_pred)
                    assert np.array_equal(r32.numpy(), o32.numpy(), equal_nan=True)   # the restatement IS the oracle at float32
                    r64 = sr.cells_ref(cells[b], sr.ANCHORS[:A], h, w, is_pred, F64)
                    worst = max(worst, sr.check_boxes(r32, r64, r32))
                    assert np.array_equal(r32[:, 0].numpy(), r64[:, 0].numpy())       # classes: the first maximum
                    if fam == "extreme" and is_pred:
                        assert bool(torch.isinf(r32).any()) and not bool(torch.isnan(r32).any())
                if fam == "class_ties" and is_pred and h * w * A > 10:
                    assert float(r32[:, 0].max()) == 1.0 and float(sr.cells_ref(cells[0], sr.ANCHORS[:A], h, w, True)[:, 0].max()) == 0.0
    held("cells_to_bboxes", worst, sr.BOX_ERR32)


def same_nms(a, b):
    return np.array_equal(np.asarray(a[0], np.float32).reshape(-1, 6), np.asarray(b[0], np.float32).reshape(-1, 6)) and \
        np.float32(a[1]) == np.float32(b[1]) and a[1] == b[1] and a[2] == b[2]


def test_nms_fast_is_the_oracle():
    t0 = time.time()
    n_checked = 0
    for name, (boxes, iou_t, conf_t) in sr.nms_cases().items():
        if boxes.shape[0] > 1000:
            continue
        assert same_nms(sr.nms_fast(boxes, iou_t, conf_t), orc.nms(torch.from_numpy(boxes), iou_t, conf_t)), name
        n_checked += 1
    b, v, below = sr.iou_pair_case()
    for thr in (v, below):
        assert same_nms(sr.nms_fast(b, thr, 0.1), orc.nms(torch.from_numpy(b), thr, 0.1))
    assert len(sr.nms_fast(b, v, 0.1)[0]) == 2 and len(sr.nms_fast(b, below, 0.1)[0]) == 1      # strict >
    for name, (t, p, nms_iou, nms_t, m) in sr.match_cases().items():
        assert sr.tp_fp_fn_fast(t, p, nms_iou, nms_t, m) == orc.tp_fp_fn(torch.from_numpy(t), torch.from_numpy(p), nms_iou, nms_t, m), name
    print("nms_fast == orc.nms on %d cases, %.1f s" % (n_checked, time.time() - t0))


def test_nms_fast_is_the_reference_on_its_captures():
    with np.load(os.path.join(GOLDEN, "yolo_tail.npz")) as f:
        g = {k: f[k] for k in f.files}
    for c in range(3):
        for k in range(2):
            iou_t, conf_t, hc, above = (float(v) for v in g["c%d_nms%d_meta" % (c, k)])
            kept, hi, ab = sr.nms_fast(g["c%d_p_boxes" % c], iou_t, conf_t)
            assert np.array_equal(kept, g["c%d_nms%d_kept" % (c, k)].astype(np.float32)) and ab == int(above) and hi == hc
            assert sr.tp_fp_fn_fast(g["c%d_t_boxes" % c], g["c%d_p_boxes" % c], iou_t, conf_t, 0.2) == \
                tuple(int(v) for v in g["c%d_tpfpfn%d" % (c, k)])
    for k in range(2):
        iou_t, conf_t, hc, above = (float(v) for v in g["dup_nms%d_meta" % k])
        kept, hi, ab = sr.nms_fast(g["dup_boxes"], iou_t, conf_t)
        assert ab == int(above) and np.array_equal(kept, g["dup_nms%d_kept" % k].astype(np.float32))


def test_nms_cases_exercise_what_they_claim():
    cases = sr.nms_cases()
    for n in sr.NMS_N:
        boxes, iou_t, conf_t = cases["cluster%d" % n]
        assert boxes.shape == (n, 6)
        t0 = time.time()
        kept = sr.nms_fast(boxes, iou_t, conf_t)[0]
        dt = time.time() - t0
        if n >= 255:
            # skip-after-remove matters: textbook NMS gives another list
            assert not np.array_equal(kept, sr.nms_fast(boxes, iou_t, conf_t, skip=False)[0]), n
        if n == sr.NMS_MAX:
            print("n = 8192: %d survivors, nms_fast %.2f s" % (len(kept), dt))
            assert 100 <= len(kept) <= 900
    for name in ("duplicates", "class_only"):
        boxes, iou_t, conf_t = cases[name]
        first_equal = sr.nms_fast(boxes, iou_t, conf_t)[0]
        assert 0 < len(first_equal) < len(boxes)
    d = cases["duplicates"][0]
    assert len(np.unique(d, axis=0)) < len(d) and len(np.unique(cases["class_only"][0], axis=0)) == 180
    kept, hi, ab = sr.nms_fast(*cases["below_conf"])
    assert len(kept) == 0 and ab == 0 and 0.0 < hi < 0.1
    kept, hi, ab = sr.nms_fast(*cases["size_filtered"])
    assert len(kept) == 0 and ab > 0
    kept, hi, ab = sr.nms_fast(*cases["threshold_edges"])
    assert ab == 32 and len(kept) > 0                    # 0.3f > 0.3 and fl32(1e-3) > 10e-4 as doubles
    assert any(r[4] == np.float32(1e-3) for r in kept) and any(r[5] == np.float32(1e-3) for r in kept)
    kept = sr.nms_fast(*cases["equal_conf600"])[0]
    assert 1 < len(kept) < 600
    boxes, iou_t, conf_t = cases["uniform4097"]          # uniform above 513: many distinct survivors, and the skip matters
    kept = sr.nms_fast(boxes, iou_t, conf_t)[0]
    assert boxes.shape == (4097, 6) and 513 < len(kept) < 1500 and len(np.unique(kept, axis=0)) == len(kept)
    assert not np.array_equal(kept, sr.nms_fast(boxes, iou_t, conf_t, skip=False)[0])
    m = sr.match_cases()
    assert len(sr.nms_fast(m["many_targets"][0], 0.5, 0.1)[0]) > 256 and len(sr.nms_fast(m["many_preds"][1], 0.5, 0.1)[0]) > 256
    assert sr.tp_fp_fn_fast(*m["iou_equals_match"]) == (0, 1, 0)
    assert sr.tp_fp_fn_fast(*m["both_empty"]) == (0, 0, 0)


def test_duplicates_case_needs_the_first_equal_rule():
    """Deleting the row at hand instead of the first equal one gives another list on the duplicates case."""
    boxes, iou_t, conf_t = sr.nms_cases()["duplicates"]
    ref = sr.nms_fast(boxes, iou_t, conf_t)[0]
    rows = [tuple(r) for r in ref]
    order, _, _ = sr._filter_sort(boxes, conf_t)
    lst, kept = [int(i) for i in order], []
    while lst:                                           # positional deletion, with the skip
        first = lst.pop(0)
        kept.append(first)
        if not lst:
            break
        sup = dict(zip(lst, (sr.iou_rows(boxes[first, 2:], boxes[lst, 2:]) > np.float32(iou_t)).tolist()))
        i = 0
        while i < len(lst):
            if sup[lst[i]]:
                del lst[i]
            i += 1
    assert [tuple(r) for r in boxes[kept]] != rows


# =========================================================================== backward stages
def composite_bwd_cases():
    """Every case of the composite backward sweep: (K, family, n, white, (g_rgb, g_depth, g_weights given))."""
    for K in sr.COMPOSITE_BWD_K:
        for fam in sr.composite_families(K):
            for n in sr.composite_bwd_n(K):
                for white in (0, 1):
                    yield K, fam, n, white, (1, 1, 1)
                    if fam == sr.subset_family(K):
                        for sub in sr.GRAD_SUBSETS:
                            yield K, fam, n, white, sub


def measure_composite_bwd():
    """The float32 oracle under autograd against the float64 one on every case, per row: d_sample, d_z by K, behind x 1e10.
    check_composite_bwd also asserts the bars and the exact zeros on the float32 oracle."""
    ds = beh = 0.0
    dz = {}
    for K, fam, n, white, sub in composite_bwd_cases():
        rays, z, samp = sr.composite_bwd_case(fam, n, K)
        g = [v if on else None for v, on in zip(sr.composite_grads(fam, n, K), sub)]
        r64 = sr.composite_bwd_ref(rays, z, samp, white, *g, dtype=F64)
        r32 = sr.composite_bwd_ref(rays, z, samp, white, *g, dtype=F32)
        e = sr.check_composite_bwd(fam, n, K, r32[0], r32[1], r64)
        ds, beh = max(ds, e[0]), max(beh, e[2])
        key = K if K in sr.COMPOSITE_BWD_ERR32_DZ else "long"
        dz[key] = max(dz.get(key, 0.0), e[1])
        if sub == (0, 0, 0):
            assert float(r64[0].abs().max()) == 0.0 and float(r64[1].abs().max()) == 0.0
    return ds, dz, beh


def test_composite_backward_fp32_oracle_error():
    ds, dz, beh = measure_composite_bwd()
    held("composite backward, d_sample per ray", ds, sr.COMPOSITE_BWD_ERR32_DSAMPLE)
    for K in sr.COMPOSITE_BWD_ERR32_DZ:
        held("composite backward, d_z per ray, K = %d" % K, dz[K], sr.composite_bwd_dz_err32(K))
    held("composite backward, d_z per ray, K >= 63", dz["long"], sr.COMPOSITE_BWD_ERR32_DZ_LONG)
    held("composite backward, behind an opaque sample x 1e10", beh, sr.COMPOSITE_BWD_ERR32_BEHIND)
    assert sr.COMPOSITE_BWD_BAR_DSAMPLE == 2e-5 and all(sr.composite_bwd_dz_bar(K) >= 2e-5 for K in sr.COMPOSITE_BWD_K)   # the floor


def test_composite_backward_inputs_avoid_the_intermediate_opacity_regime():
    """sigma x delta is at most X_CAP or is the planted 1e6 (stage_ref.py says why), and the cap leaves the families what they
    are: it moves a sample of the ordinary families only, and few of those."""
    moved = total = 0
    for K in sr.COMPOSITE_BWD_K:
        for fam in sr.composite_families(K):
            for n in sr.composite_bwd_n(K):
                rays, z, samp = sr.composite_bwd_case(fam, n, K)
                raw = sr.composite_case(fam, n, K)[2]
                zz = np.concatenate([z, rays[:, 7:8]], 1).astype(np.float64)
                x = np.diff(zz, axis=1) * np.maximum(samp[..., 3].astype(np.float64), 0.0)
                assert bool(((x <= sr.X_CAP * (1 + 1e-6)) | (samp[..., 3] == np.float32(1e6))).all()), (K, fam, n)
                assert np.array_equal(samp[..., :3], raw[..., :3]) and bool((samp[..., 3] <= raw[..., 3]).all())
                assert np.array_equal(samp[..., 3] == np.float32(1e6), raw[..., 3] == np.float32(1e6))
                moved += int((samp[..., 3] != raw[..., 3]).sum())
                total += x.size
                if fam == "z_last_far":
                    assert bool((x[:, -1] == 0).all()) and bool((samp[:, -1, 3] > 0).all())       # a zero last delta under a live sigma
    print("composite backward inputs: %d of %d samples brought down to sigma x delta = %g" % (moved, total, sr.X_CAP))
    assert 0 < moved < 0.05 * total


def aggregate_bwd_cases():
    for K in sr.AGG_K:
        for na in sr.AGG_ANCHORS:
            for fam in sr.agg_bwd_families(K):
                for n in sr.N_LIST:
                    yield K, na, fam, n


def measure_aggregate_bwd():
    worst, rows = 0.0, 0
    for K, na, fam, n in aggregate_bwd_cases():
        raw, g = sr.agg_bwd_case(fam, n, K, na)
        r32, r64 = sr.agg_bwd_ref(raw, g, na, F32), sr.agg_bwd_ref(raw, g, na, F64)
        worst = max(worst, sr.agg_row_err(r32, r64, na))
        if fam == "all_low":
            assert float(r64.abs().max()) < 1e-36 < sr.TINY             # at float32's smallest normal and below: the absolute check
        if fam == "tie" and K > 1:
            rows += sr.check_tie(r32, r64, raw, g, K, na)
    return worst, rows


def test_aggregate_backward_fp32_oracle_error():
    worst, rows = measure_aggregate_bwd()
    held("yolo_aggregate backward, per (ray, anchor)", worst, sr.AGG_BWD_ERR32)
    assert rows > 1000, rows          # the tie check discriminates (the maximum's term is 100 bars and more) on this many rows


@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_max_backward_sends_a_tie_to_the_first_index(dtype):
    """torch's max(dim) backward on the CPU, which the references of the `tie` family rest on: the gradient of out[..., 0]
    alone reaches raw[.., 0] at the FIRST tied position of each (ray, anchor) and nowhere else."""
    for K in sr.AGG_K:
        for na in (1, 3):
            raw, g = sr.agg_bwd_case("tie", 5, K, na)
            tied = sorted({i for pair in sr.tie_pairs(K) for i in pair})
            o = raw.reshape(5, K, na, 7)[..., 0]
            assert bool((o[:, tied] == 2.0).all()) and float(np.delete(o, tied, axis=1).max(initial=-9.0)) <= 1.0
            rt = sr.as_dt(raw, dtype).requires_grad_()
            orc.yolo_aggregate(rt, na)[..., 0].sum().backward()
            d = rt.grad.reshape(5, K, na, 7)
            assert float(d[..., 1:].abs().max()) == 0.0
            hit = d[..., 0] != 0
            assert bool(hit[:, tied[0]].all()) and int(hit.sum()) == 5 * na, (K, na, hit.sum(1))
            p = 1 / (1 + np.exp(-2.0))
            assert abs(float(d[0, tied[0], 0, 0]) - p * (1 - p)) < 1e-6
            assert sr.err(sr.max_term(raw, np.ones_like(g), na), d[..., 0]) < 1e-6      # the restatement check_tie uses


def test_gather_reference_is_a_sequential_float32_sum():
    for kfd in sr.GATHER_KFD:
        for pat in sr.GATHER_PATTERNS:
            for n in sr.N_LIST:
                sel, dz, g_in = sr.gather_case(pat, n, kfd)
                assert sel.dtype == np.int32 and sel.shape == (n, kfd) and int(sel.max()) < dz.size
                live = sel >= 0
                assert {"live": live.all(), "dead": not live.any(), "alternating": live[:, 0::2].all() and not live[:, 1::2].any(),
                        "last_only": live[:, -1].all() and not live[:, :-1].any(),
                        "random": kfd * n < 50 or 0.15 < 1 - live.mean() < 0.45}[pat], (pat, n, kfd)
                for gi in (None, g_in):
                    ref = sr.gather_ref(sel, dz, gi)
                    v = np.where(live, dz.reshape(-1)[np.maximum(sel, 0)].astype(np.float64), 0.0)
                    exact = v.sum(1) + (0.0 if gi is None else gi.astype(np.float64))
                    mag = np.abs(v).sum(1) + (0.0 if gi is None else np.abs(gi))
                    assert ref.dtype == np.float32 and bool((np.abs(ref - exact) <= (kfd + 1) * 2.0 ** -24 * mag).all())
                    if pat == "dead":
                        assert np.array_equal(ref, np.zeros(n, np.float32) if gi is None else gi)
    # the order matters at float32: summing the same samples backwards gives other bits somewhere
    sel, dz, _ = sr.gather_case("live", 257, 130)
    back = sr.gather_ref(sel[:, ::-1], dz)
    assert not np.array_equal(back, sr.gather_ref(sel, dz))


def host_locate(c, z_fine, depth_std, g=None):
    """locate_depth_samples_kernel restated in numpy float32 on a float32 z_fine: first position of clamp(zz), -1 if clamped."""
    g = np.asarray(c["g"] if g is None else g, np.float32)
    zz = (c["depth"][:, None] + g * np.float32(depth_std)).astype(np.float32)
    near, far = c["rays"][:, 6:7], c["rays"][:, 7:8]
    n, kt = z_fine.shape
    sel = np.full(zz.shape, -1, np.int32)
    for r in range(n):
        lo = np.searchsorted(z_fine[r], np.clip(zz[r], near[r], far[r]), side="left")
        found = (lo < kt) & (z_fine[r][np.minimum(lo, kt - 1)] == zz[r]) & (zz[r] > near[r]) & (zz[r] < far[r])
        sel[r] = np.where(found, r * kt + lo, -1)
    return sel


def test_locate_cases_are_robust_and_their_check_holds_on_the_float32_oracle():
    for kc, kf, kfd in sr.LOCATE_SHAPES:
        for n in sr.LOCATE_N:
            c = sr.locate_case(n, kc, kf, kfd)
            assert float(c["depth"][0]) == np.float32(0.8) and not c["g"][0].any()
            for std in sr.LOCATE_STD:
                zz, inside, checked = sr.locate_expect(c, std)
                assert 100 * int((~checked).sum()) < checked.size, (kc, kf, kfd, n, std)     # under 1 % left out
                assert not inside[0].any() and checked[0].all()                              # zz == near exactly: not inside, and checked
                if n * kfd >= 100:
                    assert 0.2 * inside.size < int(inside.sum()) < 0.95 * inside.size       # both kinds are present
                z32 = sr.fine_ref(c, kc, kf, kfd, 0, F32, depth_std=std).numpy()
                sel = host_locate(c, z32, std)
                sr.check_located(sel, z32, c, std, kc + kf)
                wrong = sel.copy()
                wrong[wrong >= 0] += 1                                                     # one position further: caught
                if (sel >= 0).any():
                    with pytest.raises(AssertionError):
                        sr.check_located(wrong, z32, c, std, kc + kf)
    # the seeded case: the draws of the renderer's generator instead of the explicit ones
    kc, kf, kfd = sr.LOCATE_SEEDED_SHAPE
    c = sr.locate_case(257, kc, kf, kfd)
    g = orc.seeded_draws(sr.LOCATE_SEED, 257, kc, kf, kfd)["g_depth"]
    zz, inside, checked = sr.locate_expect(c, 0.05, g)
    assert 100 * int((~checked).sum()) < checked.size and 0.2 * inside.size < int(inside.sum()) < 0.95 * inside.size


def test_backward_stage_entry_points_are_declared_and_refuse_on_the_host():
    """The three stage entry points: declared with the reference lines they restate (bound with the header's argument counts:
    tests/test_cpu_abi.py), and every bad argument refused before anything touches a device (so this runs without one)."""
    import re
    from host_tools import header_text
    from pixel_nerf_yolo_amd import lib as plib
    hdr = header_text()
    for name, cites in (("pny_yolo_aggregate_backward", "yolo.py:96-114"), ("pny_locate_depth_samples", "nerf.py:156-167"),
                        ("pny_depth_grad_gather", "nerf.py:156-167")):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and cites in hdr[hdr.rindex("/*", 0, decl.start()):decl.start()], name
    if not os.path.exists(plib.LIB_PATH):
        plib.build()
    L = plib.load()
    buf = np.zeros(64, np.float32)
    p = plib.C.c_void_p(buf.ctypes.data)          # never dereferenced: every call below is refused first
    assert L.pny_composite_backward(p, p, p, 1, sr.COMPOSITE_BWD_KMAX + 1, 1, p, p, p, p, p, None) == -1
    assert b"too many samples" in L.pny_last_error()
    for bad in ((p, p, -1, 4, 3, p), (p, p, 1, 0, 3, p), (p, p, 1, 4, 0, p), (None, p, 1, 4, 1, p), (p, None, 1, 4, 1, p), (p, p, 1, 4, 1, None)):
        assert L.pny_yolo_aggregate_backward(*bad, None) == -1 and b"pny_yolo_aggregate_backward" in L.pny_last_error(), bad
    for bad in ((p, p, p, -1, 4, p), (p, p, p, 1, -1, p), (None, p, p, 1, 4, p), (p, None, p, 1, 4, p), (p, p, p, 1, 4, None)):
        assert L.pny_depth_grad_gather(*bad, None) == -1 and b"pny_depth_grad_gather" in L.pny_last_error(), bad
    ok = [p, p, p, 0, p, 1, 8, 4, 0.01, p]
    for i, v in ((5, -1), (6, 0), (7, -1), (7, 9), (0, None), (1, None), (4, None), (9, None), (5, 2 ** 31 // 8 + 1)):
        bad = list(ok)
        bad[i] = v
        assert L.pny_locate_depth_samples(*bad, None) == -1 and b"pny_locate_depth_samples" in L.pny_last_error(), (i, v)
    assert not buf.any()
