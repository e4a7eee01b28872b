"""
What tests/test_gpu_trunk_stages.py rests on, checked without a GPU (tests/trunk_stage_ref.py): the recorded float32 figures
behind the bars still hold, every bar stays under the whole-trunk bound it sits under on every case, the written-out batch norm
is F.batch_norm (forward and autograd, float64), F.max_pool2d's backward sends a tied window's gradient to the first maximum in
scan order, and the case lists cover what the sweep promises.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import trunk_stage_ref as tr
from host_tools import built_lib  # noqa: F401

F32, F64 = tr.F32, tr.F64
HELD_SLACK = 1.1    # a float32 convolution may be blocked otherwise on another CPU or build: the last digit may move


def held(name, measured, recorded):
    """A measured float32 error against the figure recorded in trunk_stage_ref.py (the bars are twice the RECORDED figure,
    whatever is measured here): within 10 % above it, not below half of it."""
    print("%s: float32 restatement vs float64 %.3e (recorded %.3e)" % (name, measured, recorded))
    assert measured <= HELD_SLACK * recorded, "%s: %.3e exceeds the recorded %.3e" % (name, measured, recorded)
    assert measured >= 0.5 * recorded, "%s: recorded %.3e is more than twice the measured %.3e" % (name, recorded, measured)


def under_cap(bar_name, ref, where):
    """bar x scale <= cap x scale-of-the-cap for this case's float64 tensor."""
    bar, cap, kind = tr.BARS[bar_name]
    m = float(ref.abs().max())
    cap_abs = cap * (m if cap == tr.CAP_GRAD else max(1.0, m))
    assert bar * tr.scale_of(ref, kind) <= cap_abs, (bar_name, where, bar, m)


def test_bars_are_twice_the_recorded_figures_and_under_their_caps():
    figures = {"conv_fwd": tr.CONV_FWD_ERR32, "conv_t": tr.CONV_T_ERR32, "conv_dw": tr.CONV_DW_ERR32, "bn_out": tr.BN_OUT_ERR32,
               "bn_stat": tr.BN_STAT_ERR32, "bn_run": tr.BN_RUN_ERR32, "bn_dy": tr.BN_DY_ERR32, "bn_dparam": tr.BN_DPARAM_ERR32,
               "up_fwd": tr.UP_FWD_ERR32, "up_bwd": tr.UP_BWD_ERR32}
    assert set(figures) == set(tr.BARS)
    for name, (bar, cap, kind) in tr.BARS.items():
        assert bar == 2 * figures[name] and 0.0 < bar <= cap, (name, bar, cap)
        assert kind == ("grad" if cap == tr.CAP_GRAD else "act"), name
    assert (tr.CAP_ACT, tr.CAP_GRAD, tr.CAP_RUN) == (2e-4, 1e-4, 2e-6)


# ------------------------------------------------------------------------------------------------ convolution
def test_conv_forward_fp32_error():
    worst = 0.0
    for case in tr.conv_fwd_cases():
        inp = tr.conv_inputs(case, False)
        r64 = tr.conv_fwd_ref(case, inp, F64)
        worst = max(worst, tr.rel_err(tr.conv_fwd_ref(case, inp, F32), r64, "act"))
        under_cap("conv_fwd", r64, case)
    held("conv forward", worst, tr.CONV_FWD_ERR32)


def test_conv_transposed_fp32_error():
    worst = 0.0
    for case in tr.conv_t_cases():
        inp = tr.conv_inputs(case, True)
        r64 = tr.conv_t_ref(case, inp, F64)
        worst = max(worst, tr.rel_err(tr.conv_t_ref(case, inp, F32), r64, "grad"))
        under_cap("conv_t", r64, case)
    held("conv transposed", worst, tr.CONV_T_ERR32)


def test_conv_weight_gradient_fp32_error():
    worst = 0.0
    for case in tr.dw_cases():
        for chunk in (None, tr.dw_chunk(case)):     # plain, and with marker pixels at the slice boundaries
            x, dy = tr.dw_inputs(case, chunk)
            r64 = tr.dw_ref(case, x, dy, F64)
            worst = max(worst, tr.rel_err(tr.dw_ref(case, x, dy, F32), r64, "grad"))
            under_cap("conv_dw", r64, case)
    held("conv weight gradient", worst, tr.CONV_DW_ERR32)


# ------------------------------------------------------------------------------------------------ batch norm
def bn_stats32(inp, r64):
    """mean, invstd as float32 inputs of the backward: the float64 forward's, rounded."""
    return r64[1].to(F32), r64[2].to(F32)


def test_bn_fp32_errors():
    worst = dict(bn_out=0.0, bn_stat=0.0, bn_run=0.0, bn_dy=0.0, bn_dparam=0.0)
    for C in tr.BN_C:
        for case in tr.bn_cases(C):
            inp = tr.bn_inputs(C, case)
            std = float(inp["y"].to(F64).std(0).median())
            if case["P"] >= 1000 and not case["special"]:
                assert float(inp["y"].to(F64).mean(0).abs().max()) / std <= tr.BN_MAX_RATIO * 1.05, case
            r64, r32 = tr.bn_fwd_ref(case, inp), tr.bn_fwd_f32(case, inp)
            for name, idx in (("bn_out", (0,)), ("bn_stat", (1, 2)), ("bn_run", (3, 4))):
                for i in idx:
                    e = tr.rel_err(r32[i], r64[i], "act")
                    worst[name] = max(worst[name], e)
                    under_cap(name, r64[i], case)
            mean, invstd = bn_stats32(inp, r64)
            b64, b32 = tr.bn_bwd_ref(case, inp, mean, invstd), tr.bn_bwd_f32(case, inp, mean, invstd)
            for name, idx in (("bn_dy", (0, 1)), ("bn_dparam", (2, 3))):
                for i in idx:
                    e = tr.rel_err(b32[i], b64[i], "grad")
                    worst[name] = max(worst[name], e)
                    under_cap(name, b64[i], case)
    held("bn out", worst["bn_out"], tr.BN_OUT_ERR32)
    held("bn mean / invstd", worst["bn_stat"], tr.BN_STAT_ERR32)
    held("bn running statistics", worst["bn_run"], tr.BN_RUN_ERR32)
    held("bn dy / g", worst["bn_dy"], tr.BN_DY_ERR32)
    held("bn d gamma / d beta", worst["bn_dparam"], tr.BN_DPARAM_ERR32)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [0, 1])
def test_written_out_batch_norm_is_F_batch_norm_in_float64(training, relu):
    """Forward, the stepped running statistics and autograd, on an (N, C, H, W) tensor whose pixels are the (P, C) rows."""
    C, n, h, w = 64, 2, 5, 7
    case = dict(P=n * h * w, dist="n30", special=None, resid=1, relu=relu, momentum=0.1, use_running=0 if training else 1, run=1,
                null=None, mask="out" if relu else None)
    inp = tr.bn_inputs(C, case)
    out, mean, invstd, rm1, rv1 = tr.bn_fwd_ref(case, inp, F64)
    x = tr.nchw(inp["y"].reshape(n, h, w, C)).to(F64).requires_grad_(True)
    gamma, beta = inp["gamma"].to(F64).requires_grad_(True), inp["beta"].to(F64).requires_grad_(True)
    rm, rv = inp["rm"].to(F64).clone(), inp["rv"].to(F64).clone()
    o = Fn.batch_norm(x, rm, rv, gamma, beta, training, float(np.float32(0.1)), tr.EPS) + tr.nchw(inp["resid"].reshape(n, h, w, C)).to(F64)
    o = torch.relu(o) if relu else o
    flat = lambda t: tr.nhwc(t).reshape(-1, C)                                      # noqa: E731
    assert float((flat(o.detach()) - out).abs().max()) <= 1e-12
    assert float((rm - rm1).abs().max()) <= 1e-12 and float((rv - rv1).abs().max()) <= 1e-12
    g_up = tr.nchw(inp["d_out"].reshape(n, h, w, C)).to(F64)
    gx, gg, gb = torch.autograd.grad(o, (x, gamma, beta), g_up)
    # the backward takes the forward's result as its relu mask, and mean / invstd as inputs
    inp_b = dict(inp, mask=out.to(F32) if relu else None)
    dy, g, d_gamma, d_beta = tr.bn_bwd_ref(case, inp_b, mean, invstd, F64)
    for got, want in ((dy, flat(gx)), (d_gamma, gg), (d_beta, gb)):
        assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))
    assert torch.equal(g, flat(g_up) * (out > 0 if relu else torch.ones_like(out, dtype=torch.bool)))


# ------------------------------------------------------------------------------------------------ max-pool
def test_max_pool_backward_keeps_the_first_maximum():
    """On a constant plane every window is one tie, on a relu'd plane about half of them hold several zeros: F.max_pool2d's
    backward equals the hand restatement that keeps the first maximum in scan order, exactly."""
    for h, w in ((2, 2), (3, 3), (4, 5), (17, 24)):
        for kind in tr.POOL_KINDS:
            x, g, _ = tr.pool_inputs(1, h, w, kind)
            assert torch.equal(tr.pool_bwd_ref(x, g), tr.pool_bwd_first_max(x, g)), (h, w, kind)
    x, g, _ = tr.pool_inputs(1, 4, 5, "const")
    d = tr.pool_bwd_ref(x, g)[0, 0]
    # windows at rows {-1,0,1}, {1,2,3} and columns {-1,0,1}, {1,2,3}, {3,4,5}: first in-range element of each
    want = torch.zeros(4, 5, dtype=F64)
    for oy, yy in ((0, 0), (1, 1)):
        for ox, xx in ((0, 0), (1, 1), (2, 3)):
            want[yy, xx] += float(g[0, 0, oy, ox])
    assert torch.equal(d, want)
    xr, _, _ = tr.pool_inputs(3, 17, 24, "relu")
    assert float((xr == 0).float().mean()) > 0.3


def test_exact_cases_are_exact_in_float32_too():
    """The exact cases' references hold integers / copies: float32 evaluation gives the same bits as float64."""
    x, g, add = tr.pool_inputs(3, 17, 24, "relu")
    assert torch.equal(Fn.max_pool2d(x, 3, 2, 1).to(F64), tr.pool_fwd_ref(x))
    x0 = x.clone().requires_grad_(True)
    d, = torch.autograd.grad(Fn.max_pool2d(x0, 3, 2, 1), x0, g)
    assert torch.equal((d + add).to(F64), tr.pool_bwd_ref(x, g, add))
    lv = torch.from_numpy(np.random.RandomState(1).randn(1, 64, 9, 11).astype(np.float32))
    assert torch.equal(tr.up_fwd_ref(lv, (9, 11), F64), lv.to(F64))


# ------------------------------------------------------------------------------------------------ pyramid
def test_upsample_fp32_errors():
    wf = wb = 0.0
    for H, W, pool, n in tr.UP_CASES:
        sizes, levels, g, adds = tr.up_inputs(H, W, pool, n)
        for lv in range(4):
            r64 = tr.up_fwd_ref(levels[lv], sizes[0], F64)
            wf = max(wf, tr.rel_err(tr.up_fwd_ref(levels[lv], sizes[0], F32), r64, "act"))
            under_cap("up_fwd", r64, (H, W, lv))
            gs = g[:, tr.UP_COFF[lv]:tr.UP_COFF[lv] + tr.UP_CH[lv]]
            for add in (None, adds[lv]):
                b64 = tr.up_bwd_ref(levels[lv], sizes[0], gs, add, F64)
                wb = max(wb, tr.rel_err(tr.up_bwd_ref(levels[lv], sizes[0], gs, add, F32), b64, "grad"))
                under_cap("up_bwd", b64, (H, W, lv))
    held("pyramid upsample", wf, tr.UP_FWD_ERR32)
    held("pyramid upsample backward", wb, tr.UP_BWD_ERR32)


# ------------------------------------------------------------------------------------------------ coverage of the case lists
def test_case_lists_cover_the_sweep(built_lib):
    rows = tr.table(built_lib)
    assert sorted(set(rows)) == sorted(tr.GEOMS) and len(tr.GEOMS) == 8          # the table holds these eight and no other
    units = tr.unit_of(built_lib)
    assert all(rows[u] == g for u, g in zip(units, tr.GEOMS))
    co = tr.conv_out

    def out_px(c):
        k, s, p = tr.GEOMS[c["gi"]][:3]
        return c["n"] * co(c["hin"], k, s, p) * co(c["win"], k, s, p)

    fwd, tcs, dws = tr.conv_fwd_cases(), tr.conv_t_cases(), tr.dw_cases()
    for gi, g in enumerate(tr.GEOMS):
        mine = [c for c in fwd if c["gi"] == gi]
        assert {out_px(c) for c in mine if c["tag"] == "edge"} >= {1, 30, 33, 63, 64, 65}
        assert {c["n"] for c in mine} >= {1, 2}
        assert {(c["resid"], c["relu"]) for c in mine if c["affine"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        if g[1] == 2:
            assert {c["hin"] % 2 for c in mine} == {0, 1} and {c["win"] % 2 for c in mine} == {0, 1}
        mine = [c for c in dws if c["gi"] == gi]
        assert {out_px(c) for c in mine if c["tag"] == "edge"} == {1, 15, 33, 127, 128, 129, 255, 256, 257}
        if g[1] == 2:
            assert all(c["hin"] % 2 == 1 and c["win"] % 2 == 1 for c in mine if c["tag"] == "edge")
        mine = [c for c in tcs if c["gi"] == gi]
        if g[3] < 32:
            assert not mine
        elif g[1] == 1:
            assert {c["n"] * c["hin"] * c["win"] for c in mine} >= {1, 30, 33, 63, 64, 65} and {c["resid"] for c in mine} == {0, 1}
        else:
            assert {(c["hin"], c["win"]) for c in mine if c["tag"] == "stride2"} == {(4, 4), (5, 7), (8, 6), (9, 12)}
    assert dict(gi=tr.STEM, n=1, hin=33, win=47, resid=0, relu=1, affine=0, tag="edge") in fwd
    large = {(c["gi"], c["n"], c["hin"], c["win"]) for c in fwd if c["tag"] == "large"}
    assert large >= {(1, 2, 128, 128), (1, 2, 128, 131), (0, 12, 128, 128), (3, 1, 256, 256)}
    # ragged last tiles of 64 x 64, not just shapes: under the split instantiation (64 -> 64 3x3, 512 .. 1024 tiles) a remainder
    # below 32 pixels (the tile's second half wholly outside) and one above (partly outside); under the plain one (the stem,
    # J < 32) both again, with tile counts that are no multiple of the 4 tiles of a workgroup; and one under a transposed
    # convolution
    def ragged(cases, transposed, gi):
        out = []
        for c in cases:
            if c["tag"] == "large" and c["gi"] == gi:
                npix, cols = tr.large_tiles(c, transposed)
                tiles = -(-npix // 64) * cols
                assert tiles >= 512, c                               # 64 x 64 tiles on a 256-CU device
                out.append((npix % 64, tiles))
        return out
    split = ragged(fwd, False, tr.L1)
    assert all(512 <= t <= 1024 for _, t in split)
    assert any(0 < r < 32 for r, _ in split) and any(32 < r < 64 for r, _ in split) and any(r == 0 for r, _ in split)
    plain = ragged(fwd, False, tr.STEM)
    assert any(0 < r < 32 and t % 4 for r, t in plain) and any(32 < r < 64 and t % 4 for r, t in plain)
    assert any(r and t % 4 for r, t in ragged(tcs, True, 3))
    assert {(c["gi"], c["n"], c["hin"], c["win"]) for c in dws if c["tag"] == "large"} >= {(0, 12, 128, 128), (1, 12, 32, 32)}
    for C in tr.BN_C:
        cases = tr.bn_cases(C)
        plain = [c for c in cases if not c["special"]]
        assert {(c["P"], c["dist"]) for c in plain} == {(P, d) for P in tr.BN_P for d in ("n01", "n30")}
        assert tr.BN_P == (4, 6, 255, 256, 257, 1000, 16383, 16384, 16385, 20000, 49152)
        for key, vals in (("resid", {0, 1}), ("relu", {0, 1}), ("momentum", {0.0, 0.1, tr.BN_SMALL_MOMENTUM}), ("use_running", {0, 1}), ("run", {0, 1}),
                          ("null", {None, "g_out", "d_gamma", "d_beta"}), ("mask", {None, "out"})):
            assert {c[key] for c in plain} == vals, (C, key)
        assert {c["special"] for c in cases} == {None, "const", "markers"}
        inp = tr.bn_inputs(C, next(c for c in cases if c["mask"]))
        assert float((inp["mask"] == 0).float().mean()) > 0.3                   # exact zeros in the supplied mask
    assert tr.POOL_SIZES == ((2, 2), (3, 3), (4, 5), (16, 16), (17, 24), (64, 64)) and tr.POOL_N == (1, 3)
    assert [(H, W) for H, W, _ in tr.UP_IMAGES] == [(32, 32), (33, 47), (32, 40), (128, 128), (75, 100)]
    assert {c[:3] for c in tr.UP_CASES} == set(tr.UP_IMAGES) and {c[3] for c in tr.UP_CASES} == {1, 2}
    assert tr.pyramid(75, 100, False)[1] == tr.pyramid(75, 100, False)[0]       # without the first pool level 1 is exact too
    assert tr.boundary_pixels(10, 4) == [0, 3, 4, 7, 8, 9] and tr.boundary_pixels(8, 4, first=False) == [3, 4, 7]


def test_abi_declares_the_trunk_stage_entries(built_lib):
    """(Declared, bound and exported with the header's argument counts: tests/test_cpu_abi.py.)  pny_trunk_unit refuses an index
    outside the table."""
    assert built_lib.pny_trunk_unit(len(tr.table(built_lib)), None, None, None, None, None) == -1
    assert b"pny_trunk_unit" in built_lib.pny_last_error()
    assert built_lib.pny_trunk_unit(-1, None, None, None, None, None) == -1
