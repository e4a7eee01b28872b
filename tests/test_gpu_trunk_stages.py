"""
The ResNet-34 trunk's stage kernels (csrc/encoder.hip, csrc/encoder_train.hip), each through its own entry point
(include/pnyolo.h pny_trunk_*) on inputs this file chooses (-m gpu, real MI355X): the implicit-GEMM convolution forward and
transposed in its four instantiations, the split weight gradient, batch norm forward and backward, the max-pool and the
bilinear pyramid with their backwards.  The whole-trunk tests (tests/test_gpu_trunk.py) see these only through a 2e-4 / 1e-4
bound on the final result and need a unit-flipping reference to hold it; here the relu mask is an input, so nothing can flip.

Every float result is held to float64 on the float32 inputs; the cases, references, bars and where each bar comes from are in
tests/trunk_stage_ref.py, and tests/test_cpu_trunk_stage_refs.py shows without a GPU that the bars are what they claim to be.
Each test prints one TRUNKSTAGE line with its worst error / bar.
"""
import ctypes as C

import pytest
import torch

import trunk_stage_ref as tr
from pixel_nerf_yolo_amd import lib as plib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = tr.F32, tr.F64
NAN = float("nan")


def dev(t):
    return None if t is None else torch.as_tensor(t, dtype=F32).contiguous().to(DEV)


def stream():
    return plib.stream_of(torch.device(DEV))


def nans(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=F32)


def report(stage, worst, bar, extra=""):
    print("TRUNKSTAGE %s: worst error %.3e, bar %.3e (%.2f of the bar)%s" % (stage, worst, bar, worst / bar, extra))


@pytest.fixture(scope="module")
def units():
    return tr.unit_of(plib.load())


# ------------------------------------------------------------------------------------------------ entry-point wrappers
def hip_conv(unit, case, inputs, transposed):
    """-> (result NCHW on the host, the instantiation the entry reports as 100 SPLIT + 10 NT + MT)"""
    k, s, p, cin, cout = tr.GEOMS[case["gi"]]
    src, w, scale, shift, resid = inputs
    n, hin, win = case["n"], case["hin"], case["win"]
    ho, wo = tr.conv_out(hin, k, s, p), tr.conv_out(win, k, s, p)
    a_in, a_res = dev(tr.nhwc(src, pad4=True)), dev(None if resid is None else tr.nhwc(resid))
    a_w, a_sc, a_sh = dev(w), dev(scale), dev(shift)
    variant = C.c_int(0)
    if transposed:      # the gradient (n, ho, wo, cout) -> the forward input's size
        out = nans(n, hin, win, cin)
        dims = (n, ho, wo, hin, win)
    else:
        out = nans(n, ho, wo, cout)
        dims = (n, hin, win, ho, wo)
    plib.check(plib.load().pny_trunk_conv(unit, 1 if transposed else 0, plib.ptr(a_w), plib.ptr(a_in), *dims, plib.ptr(a_sc), plib.ptr(a_sh),
                                          plib.ptr(a_res), 0 if transposed else case["relu"], plib.ptr(out), C.byref(variant), stream()))
    torch.cuda.synchronize()
    return tr.nchw(out.cpu()), variant.value


def hip_dw(unit, case, x, dy):
    """-> (dw (cout, cin, k, k) on the host, splits, chunk)"""
    k, s, p, cin, cout = tr.GEOMS[case["gi"]]
    a_x, a_dy = dev(tr.nhwc(x, pad4=True)), dev(tr.nhwc(dy))
    dw = nans(cout, cin, k, k)
    splits, chunk = C.c_int(0), C.c_int64(0)
    plib.check(plib.load().pny_trunk_conv_dw(unit, plib.ptr(a_dy), plib.ptr(a_x), case["n"], case["hin"], case["win"], plib.ptr(dw),
                                             C.byref(splits), C.byref(chunk), stream()))
    torch.cuda.synchronize()
    return dw.cpu(), splits.value, chunk.value


# ------------------------------------------------------------------------------------------------ convolution
class ConvSweep:
    """The convolution sweep, a geometry at a time and each only once: errors per case and the instantiations reported."""

    def __init__(self, units):
        self.units, self.done = units, {}

    def run(self, transposed, key):
        """key: a GEOMS index (its edge and epilogue cases) or "large" -> [(case, error, variant)]"""
        if (transposed, key) not in self.done:
            cases = tr.conv_t_cases() if transposed else tr.conv_fwd_cases()
            cases = [c for c in cases if (c["tag"] == "large") == (key == "large") and key in ("large", c["gi"])]
            ref = tr.conv_t_ref if transposed else tr.conv_fwd_ref
            res = []
            for case in cases:
                inputs = tr.conv_inputs(case, transposed)
                got, variant = hip_conv(self.units[case["gi"]], case, inputs, transposed)
                res.append((case, tr.rel_err(got, ref(case, inputs, F64), "grad" if transposed else "act"), variant))
            self.done[(transposed, key)] = res
        return self.done[(transposed, key)]

    def variants(self):
        keys = list(range(len(tr.GEOMS))) + ["large"]
        return {v for t in (False, True) for key in keys for _, _, v in self.run(t, key)}


@pytest.fixture(scope="module")
def conv_sweep(units):
    return ConvSweep(units)


def check_conv(conv_sweep, transposed, key):
    res = conv_sweep.run(transposed, key)
    name, bar = ("conv_t", tr.CONV_T_BAR) if transposed else ("conv_fwd", tr.CONV_FWD_BAR)
    assert res or (transposed and key == tr.STEM)
    worst = 0.0
    for case, e, variant in res:
        print("  %s %s: error %.3e, conv_mfma_kernel<%d, %d, %d>" % (name, case, e, variant // 100, variant // 10 % 10, variant % 10))
        worst = max(worst, e)
    report("%s %s" % (name, key if key == "large" else "%dx%d/%d %d->%d" % ((tr.GEOMS[key][0],) * 2 + tr.GEOMS[key][1:2] + tr.GEOMS[key][3:])),
           worst, bar, ", instantiations %s" % sorted({v for _, _, v in res}))
    for case, e, _ in res:
        assert e <= bar, (case, e, bar)


@pytest.mark.parametrize("key", list(range(len(tr.GEOMS))) + ["large"])
def test_conv_forward_sweep(conv_sweep, key):
    """Every geometry at 1 .. 65 output pixels (odd and even input sizes under stride 2, n = 1 and 2), its epilogue with and
    without residual and relu under a non-trivial scale / shift, the stem at 33 x 47; "large": the shapes that aim at the
    four instantiations, whole tiles and ragged last tiles (the second half of a 64-pixel tile wholly and partly outside;
    tile counts that leave waves of the last workgroup idle)."""
    check_conv(conv_sweep, False, key)


@pytest.mark.parametrize("key", list(range(1, len(tr.GEOMS))) + ["large"])
def test_conv_transposed_sweep(conv_sweep, key):
    """The input gradient: stride 1 with and without the added residual, stride 2 (3x3 pad 1, 1x1 pad 0) read as a dilated
    input at forward-input sizes (4, 4), (5, 7), (8, 6), (9, 12); "large": 64 x 64 tiles under a transposed convolution.  The
    stem has no transposed form (3 output rows are no MFMA tile, and the trunk never asks for the images' gradient)."""
    check_conv(conv_sweep, True, key)


def test_conv_sweep_launched_every_instantiation(conv_sweep):
    """What the entry REPORTED over the whole sweep, not a restatement of the routing: all four conv_mfma_kernel
    instantiations ran (<8, 2, 2> is launched by no other test of the suite, <1, 2, 2> by two inference shapes only)."""
    seen = conv_sweep.variants()
    print("TRUNKSTAGE conv instantiations launched: %s" % sorted(seen))
    assert seen == {111, 122, 811, 822}, seen
    assert 122 in {v for _, _, v in conv_sweep.run(True, "large")}               # ... and <1, 2, 2> under a transposed convolution


# ------------------------------------------------------------------------------------------------ weight gradient
class DwSweep:
    def __init__(self, units):
        self.units, self.done = units, {}

    def run(self, key):
        """-> [(case, splits, chunk, npix, error, error with marker pixels)]"""
        if key not in self.done:
            res = []
            for case in tr.dw_cases():
                if (case["tag"] == "large") != (key == "large") or key not in ("large", case["gi"]):
                    continue
                k, s, p = tr.GEOMS[case["gi"]][:3]
                npix = case["n"] * tr.conv_out(case["hin"], k, s, p) * tr.conv_out(case["win"], k, s, p)
                x, dy = tr.dw_inputs(case)
                got, splits, chunk = hip_dw(self.units[case["gi"]], case, x, dy)
                e = tr.rel_err(got, tr.dw_ref(case, x, dy, F64), "grad")
                xm, dym = tr.dw_inputs(case, chunk)             # markers at the boundaries of the slices just reported
                gotm, splits_m, chunk_m = hip_dw(self.units[case["gi"]], case, xm, dym)
                assert (splits_m, chunk_m) == (splits, chunk)
                res.append((case, splits, chunk, npix, e, tr.rel_err(gotm, tr.dw_ref(case, xm, dym, F64), "grad")))
            self.done[key] = res
        return self.done[key]


@pytest.fixture(scope="module")
def dw_sweep(units):
    return DwSweep(units)


@pytest.mark.parametrize("key", list(range(len(tr.GEOMS))) + ["large"])
def test_conv_weight_gradient_sweep(dw_sweep, key):
    """Every geometry at 1 .. 257 output pixels (odd input sizes under stride 2); "large": the stem and layer1.0.conv1 at 12
    views of 128 x 128.  Each case plain and with marker pixels on both sides of every slice boundary the entry reported."""
    res = dw_sweep.run(key)
    assert res
    worst = 0.0
    for case, splits, chunk, npix, e, em in res:
        print("  conv_dw %s: %d pixels in %d slices of %d, error %.3e, with markers %.3e" % (case, npix, splits, chunk, e, em))
        worst = max(worst, e, em)
    report("conv_dw %s" % key, worst, tr.CONV_DW_BAR, ", (splits, chunk) %s" % sorted({(r[1], r[2]) for r in res}))
    for case, splits, chunk, npix, e, em in res:
        assert splits >= 1 and (splits - 1) * chunk < npix <= splits * chunk, (case, splits, chunk, npix)
        assert e <= tr.CONV_DW_BAR and em <= tr.CONV_DW_BAR, (case, e, em)


def test_conv_weight_gradient_sweep_saw_one_slice_and_a_short_last_slice(dw_sweep):
    res = [r for key in list(range(len(tr.GEOMS))) + ["large"] for r in dw_sweep.run(key)]
    print("TRUNKSTAGE conv_dw split counts seen: %s" % sorted({r[1] for r in res}))
    assert any(r[1] == 1 for r in res)
    assert any(r[1] > 1 and r[3] < r[1] * r[2] for r in res)                     # several slices, the last one short
    assert any(r[1] > 1 and r[3] == r[1] * r[2] for r in res)                    # ... and several full ones


# ------------------------------------------------------------------------------------------------ batch norm
def hip_bn_forward(C_, case, inp):
    P = case["P"]
    a = {k: dev(inp[k]) for k in ("y", "gamma", "beta", "resid")}
    rm, rv = (dev(inp["rm"]), dev(inp["rv"])) if case["run"] else (None, None)
    out, mean, invstd = nans(P, C_), nans(C_), nans(C_)
    plib.check(plib.load().pny_trunk_bn_forward(plib.ptr(a["y"]), P, C_, plib.ptr(a["gamma"]), plib.ptr(a["beta"]), plib.ptr(a["resid"]),
                                                case["relu"], plib.ptr(rm), plib.ptr(rv), case["momentum"], case["use_running"],
                                                plib.ptr(out), plib.ptr(mean), plib.ptr(invstd), stream()))
    torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in (out, mean, invstd, rm, rv)]


@pytest.mark.parametrize("C_", tr.BN_C)
def test_bn_forward_sweep(C_):
    """P from 4 to 49 152 around the one-workgroup, 64-workgroup and ragged-last-chunk edges, N(0, 1) and N(30, 1), residual /
    relu / momentum / eval-mode statistics on and off, no running statistics passed, a constant channel, marker pixels."""
    worst = dict(bn_out=0.0, bn_stat=0.0, bn_run=0.0)
    for case in tr.bn_cases(C_):
        inp = tr.bn_inputs(C_, case)
        ref = tr.bn_fwd_ref(case, inp)
        got = hip_bn_forward(C_, case, inp)
        errs = dict(bn_out=tr.rel_err(got[0], ref[0], "act"),
                    bn_stat=max(tr.rel_err(got[1], ref[1], "act"), tr.rel_err(got[2], ref[2], "act")), bn_run=0.0)
        if case["run"]:
            stepped = not case["use_running"] and case["momentum"] > 0
            if stepped:
                errs["bn_run"] = max(tr.rel_err(got[3], ref[3], "act"), tr.rel_err(got[4], ref[4], "act"))
            else:           # momentum 0, eval mode: left alone, to the bit
                assert torch.equal(got[3], inp["rm"]) and torch.equal(got[4], inp["rv"]), case
        if case["special"] == "const":
            assert float(got[1][5]) == float(inp["y"][0, 5]), case                    # the shifted sums of a constant channel are zero
        print("  bn_forward C=%d %s: %s" % (C_, case, {k: "%.3e" % v for k, v in errs.items()}))
        for k, e in errs.items():
            worst[k] = max(worst[k], e)
            assert e <= tr.BARS[k][0], (case, k, e, tr.BARS[k][0])
    for k in worst:
        report("bn_forward C=%d %s" % (C_, k), worst[k], tr.BARS[k][0])


@pytest.mark.parametrize("C_", tr.BN_C)
def test_bn_backward_sweep(C_):
    """The same cases; the relu mask is an input (half exact zeros) or null, mean / invstd are inputs, each optional output is
    left out in turn."""
    worst = dict(bn_dy=0.0, bn_dparam=0.0)
    L = plib.load()
    for case in tr.bn_cases(C_):
        inp = tr.bn_inputs(C_, case)
        fwd = tr.bn_fwd_ref(case, inp)
        mean, invstd = fwd[1].to(F32), fwd[2].to(F32)
        ref = tr.bn_bwd_ref(case, inp, mean, invstd)
        P = case["P"]
        a = {k: dev(inp[k]) for k in ("d_out", "mask", "y", "gamma")}
        a_mean, a_is = dev(mean), dev(invstd)
        outs = dict(dy=nans(P, C_), g_out=nans(P, C_), d_gamma=nans(C_), d_beta=nans(C_))
        if case["null"]:
            outs[case["null"]] = None
        plib.check(L.pny_trunk_bn_backward(plib.ptr(a["d_out"]), plib.ptr(a["mask"]), plib.ptr(a["y"]), plib.ptr(a_mean), plib.ptr(a_is),
                                           plib.ptr(a["gamma"]), P, C_, case["use_running"], plib.ptr(outs["dy"]), plib.ptr(outs["g_out"]),
                                           plib.ptr(outs["d_gamma"]), plib.ptr(outs["d_beta"]), stream()))
        torch.cuda.synchronize()
        errs = dict(bn_dy=tr.rel_err(outs["dy"].cpu(), ref[0], "grad"), bn_dparam=0.0)
        if outs["g_out"] is not None:
            assert torch.equal(outs["g_out"].cpu().to(F64), ref[1]), case               # the masked gradient: a copy or a zero
        for name, r in (("d_gamma", ref[2]), ("d_beta", ref[3])):
            if outs[name] is not None:
                errs["bn_dparam"] = max(errs["bn_dparam"], tr.rel_err(outs[name].cpu(), r, "grad"))
        print("  bn_backward C=%d %s: %s" % (C_, case, {k: "%.3e" % v for k, v in errs.items()}))
        for k, e in errs.items():
            worst[k] = max(worst[k], e)
            assert e <= tr.BARS[k][0], (case, k, e, tr.BARS[k][0])
    for k in worst:
        report("bn_backward C=%d %s" % (C_, k), worst[k], tr.BARS[k][0])


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("kind", tr.POOL_KINDS)
def test_maxpool_forward_and_backward_exact(kind):
    """relu'd noise (zeros tie in most windows), a constant plane (every window one tie), distinct values: the forward and,
    with an integer upstream gradient (and integer `add`), the backward are exact -- the first maximum in scan order takes a
    window's gradient (tests/test_cpu_trunk_stage_refs.py shows that this is what F.max_pool2d's backward does)."""
    L, Cc = plib.load(), tr.POOL_C
    for h, w in tr.POOL_SIZES:
        for n in tr.POOL_N:
            x, g, add = tr.pool_inputs(n, h, w, kind)
            ho, wo = tr.conv_out(h, 3, 2, 1), tr.conv_out(w, 3, 2, 1)
            a_x, a_g, a_add = dev(tr.nhwc(x)), dev(tr.nhwc(g)), dev(tr.nhwc(add))
            out = nans(n, ho, wo, Cc)
            plib.check(L.pny_trunk_maxpool(plib.ptr(a_x), n, h, w, Cc, plib.ptr(out), stream()))
            torch.cuda.synchronize()
            assert torch.equal(tr.nchw(out.cpu()).to(F64), tr.pool_fwd_ref(x)), (h, w, n)
            for use_add in (None, a_add):
                d_in = nans(n, h, w, Cc)
                plib.check(L.pny_trunk_maxpool_backward(plib.ptr(a_x), plib.ptr(a_g), plib.ptr(use_add), n, h, w, Cc, plib.ptr(d_in), stream()))
                torch.cuda.synchronize()
                ref = tr.pool_bwd_ref(x, g, None if use_add is None else add)
                assert torch.equal(tr.nchw(d_in.cpu()).to(F64), ref), (h, w, n, use_add is not None)
    print("TRUNKSTAGE maxpool %s: forward and backward exact at %d shapes" % (kind, len(tr.POOL_SIZES) * len(tr.POOL_N)))


# ------------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("H,W,pool,n", tr.UP_CASES)
def test_upsample_into_latent_and_backward(H, W, pool, n):
    """The four levels of an H x W image's pyramid written into ONE NaN-filled latent: every element is written, a level of the
    latent's own size is copied to the bit, the others meet the bar; then each level's backward, with and without `add`."""
    L = plib.load()
    sizes, levels, g, adds = tr.up_inputs(H, W, pool, n)
    h0, w0 = sizes[0]
    lat = nans(n, h0, w0, tr.UP_LATENT)
    for lv in range(4):
        a = dev(tr.nhwc(levels[lv]))
        plib.check(L.pny_trunk_upsample(plib.ptr(a), n, sizes[lv][0], sizes[lv][1], lv, h0, w0, plib.ptr(lat), stream()))
        torch.cuda.synchronize()
    got = tr.nchw(lat.cpu())
    assert not bool(torch.isnan(got).any())
    wf = wb = 0.0
    a_g = dev(tr.nhwc(g))
    for lv in range(4):
        sl = slice(tr.UP_COFF[lv], tr.UP_COFF[lv] + tr.UP_CH[lv])
        ref = tr.up_fwd_ref(levels[lv], sizes[0], F64)
        if sizes[lv] == sizes[0]:
            assert torch.equal(got[:, sl].to(F64), ref), lv
        else:
            e = tr.rel_err(got[:, sl], ref, "act")
            wf = max(wf, e)
            assert e <= tr.UP_FWD_BAR, (lv, e)
        for add in (None, adds[lv]):
            d_in = nans(n, sizes[lv][0], sizes[lv][1], tr.UP_CH[lv])
            a_add = dev(None if add is None else tr.nhwc(add))
            plib.check(L.pny_trunk_upsample_backward(plib.ptr(a_g), plib.ptr(a_add), n, sizes[lv][0], sizes[lv][1], lv, h0, w0, plib.ptr(d_in),
                                                     stream()))
            torch.cuda.synchronize()
            e = tr.rel_err(tr.nchw(d_in.cpu()), tr.up_bwd_ref(levels[lv], sizes[0], g[:, sl], add, F64), "grad")
            wb = max(wb, e)
            assert e <= tr.UP_BWD_BAR, (lv, add is not None, e)
    assert pool or sizes[1] == sizes[0]
    report("upsample %dx%dx%d" % (n, H, W), wf, tr.UP_FWD_BAR)
    report("upsample_backward %dx%dx%d" % (n, H, W), wb, tr.UP_BWD_BAR)


# ------------------------------------------------------------------------------------------------ refusals
def test_trunk_stages_refuse_bad_arguments(units):
    """PNY_ERR_ARG with the function's name in pny_last_error(), and nothing launched: a null pointer, C not 64 / 128 / 256, a
    count below 1, a unit or level out of range, sizes that are not the unit's."""
    L = plib.load()
    SENTINEL = 7.0            # no entry writes this from it: a launch on the refused arguments would change some element
    buf = torch.full((1 << 16,), SENTINEL, device=DEV)
    p, st = plib.ptr(buf), stream()
    n_units = len(tr.table(L))

    def refused(fn, name, ok, changes):
        for i, v in changes:
            bad = list(ok)
            bad[i] = v
            assert fn(*bad, st) == -1 and name in L.pny_last_error(), (name, i, v, L.pny_last_error())

    u = units[tr.L1]
    refused(L.pny_trunk_conv, b"pny_trunk_conv", [u, 0, p, p, 1, 5, 6, 5, 6, p, p, None, 0, p, None],
            [(0, -1), (0, n_units), (2, None), (3, None), (9, None), (10, None), (13, None), (4, 0), (5, 0), (6, -1), (7, 4), (8, 7)])
    refused(L.pny_trunk_conv, b"pny_trunk_conv", [units[tr.STEM], 1, p, p, 1, 3, 3, 5, 5, p, p, None, 0, p, None], [(0, units[tr.STEM])])
    refused(L.pny_trunk_conv, b"pny_trunk_conv", [units[2], 1, p, p, 1, 3, 3, 5, 5, p, p, None, 0, p, None], [(7, 7), (8, 4)])
    refused(L.pny_trunk_conv_dw, b"pny_trunk_conv_dw", [u, p, p, 1, 5, 6, p, None, None],
            [(0, -1), (0, n_units), (1, None), (2, None), (6, None), (3, 0), (4, 0), (5, -3)])
    refused(L.pny_trunk_bn_forward, b"pny_trunk_bn_forward", [p, 4, 64, p, p, None, 0, None, None, 0.1, 0, p, p, p],
            [(0, None), (1, 0), (2, 32), (2, 65), (2, 512), (3, None), (4, None), (11, None), (12, None), (13, None), (7, p), (8, p), (10, 1)])
    refused(L.pny_trunk_bn_backward, b"pny_trunk_bn_backward", [p, None, p, p, p, p, 4, 64, 0, p, None, None, None],
            [(0, None), (2, None), (3, None), (4, None), (5, None), (6, 0), (7, 100), (9, None)])
    refused(L.pny_trunk_maxpool, b"pny_trunk_maxpool", [p, 1, 2, 2, 64, p], [(0, None), (5, None), (1, 0), (2, 0), (3, 0), (4, 3)])
    refused(L.pny_trunk_maxpool_backward, b"pny_trunk_maxpool_backward", [p, p, None, 1, 2, 2, 64, p],
            [(0, None), (1, None), (7, None), (3, 0), (6, 7)])
    refused(L.pny_trunk_upsample, b"pny_trunk_upsample", [p, 1, 2, 2, 0, 2, 2, p], [(0, None), (7, None), (4, -1), (4, 4), (1, 0), (5, 0)])
    refused(L.pny_trunk_upsample_backward, b"pny_trunk_upsample_backward", [p, None, 1, 2, 2, 0, 2, 2, p],
            [(0, None), (8, None), (5, 4), (3, 0)])
    assert L.pny_trunk_unit(n_units, None, None, None, None, None) == -1 and b"pny_trunk_unit" in L.pny_last_error()
    with pytest.raises(plib.PnyError):
        plib.check(L.pny_trunk_maxpool(None, 1, 2, 2, 64, p, st))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                                          # nothing was launched on the refused calls
