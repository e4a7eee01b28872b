"""
The occupancy grid on the device (-m gpu; include/pnyolo.h "occupancy grid", csrc/occupancy.hip, csrc/pny_occupancy.h).

Build and classification equal the numpy restatement (tests/occupancy_ref.py) exactly.  A culled render is held to the MASKED
ORACLE at the project's parity bar of 1e-4: the oracle's public stages composed as the contract says -- the MLP's output at
every sample the grid rejects replaced by (0, 0, 0, 0) before the composite, in both passes, the fine samples following from the
masked coarse weights.  The mask is the restatement's, which the classification test pins to the device's.

Rays are chosen BEFORE a run, with the masked oracle alone (usable_rays): a ray is not used when a fine draw sits within 1e-5
of an edge of the masked coarse cdf (importance sampling is discontinuous there; the margin of helpers.clean_rays), or when
one of its samples sits within 2e-5 in depth of a change of the mask (the device's fine depths differ from the oracle's by
rounding).  At least 32 of the 37 rays must remain; nothing is excluded after a run.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import occupancy_ref as oref
import pnyolo_oracle as orc
from helpers import DEV, dt, maxabs, render_debug, scene_pair
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import recon, synth
from pixel_nerf_yolo_amd.render import NeRFRenderer, _MultiDeviceRenderWrapper

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # the project's parity bar
F16_TOL = 5e-3             # tests/test_gpu_f16.py RENDER_TOL: the bar that file holds the single-plane mode's renders to
N_RAYS, KC, KF, KFD = 37, 16, 8, 4
KT = KC + KF
H = W = 32
SLAB_DIMS = (9, 5, 5)      # 8 cells along x: the slab ix < t, t = 0 .. 8
SLAB_BOX = ((-0.5, -0.6, -0.6), (0.3, 0.6, 0.6))
MARGIN_CDF, MARGIN_Z = 1e-5, 2e-5


def report(name, value):
    print("OCCUPANCY-MEASURED %s %s" % (name, value))


# --------------------------------------------------------------------------- device calls
def dev_build(sigma, sigma2, thresh, dilate):
    L = plib.load()
    s1 = dt(sigma)
    s2 = None if sigma2 is None else dt(sigma2)
    dims = (C.c_int32 * 3)(*sigma.shape)
    bits = torch.full((oref.n_words(sigma.shape),), -1, device=DEV, dtype=torch.int32)
    count = torch.full((1,), -7, device=DEV, dtype=torch.int64)
    plib.check(L.pny_occupancy_build(C.c_void_p(s1.data_ptr()), None if s2 is None else C.c_void_p(s2.data_ptr()), dims, thresh, dilate,
                                     C.c_void_p(bits.data_ptr()), C.c_void_p(count.data_ptr()), plib.stream_of(torch.device(DEV))))
    return bits.cpu().numpy().view(np.uint32), int(count.item())


def dev_classify(bits, dims, box, outside_empty, rays, z):
    L = plib.load()
    n, k = z.shape
    need = C.c_int64(0)
    plib.check(L.pny_occupancy_classify_workspace_bytes(n * k, C.byref(need)))
    b = torch.from_numpy(bits.view(np.int32).copy()).to(DEV)
    r, zz = dt(rays), dt(z)
    slot = torch.full((n, k), -9, device=DEV, dtype=torch.int32)
    kept = torch.full((1,), -7, device=DEV, dtype=torch.int64)
    ws = torch.empty(need.value, device=DEV, dtype=torch.uint8)
    plib.check(L.pny_occupancy_classify(C.c_void_p(b.data_ptr()), (C.c_int32 * 3)(*dims), (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1]),
                                        int(outside_empty), C.c_void_p(r.data_ptr()), C.c_void_p(zz.data_ptr()), n, k,
                                        C.c_void_p(slot.data_ptr()), C.c_void_p(kept.data_ptr()), C.c_void_p(ws.data_ptr()), need.value,
                                        plib.stream_of(torch.device(DEV))))
    return slot.cpu().numpy(), int(kept.item())


# --------------------------------------------------------------------------- build
@pytest.mark.parametrize("dims", oref.VOLUMES)
def test_build_equals_the_restatement_and_itself(dims):
    cells = oref.n_cells(dims)
    for two in (False, True):
        vols = oref.case_volume(dims, seed=11 + sum(dims), two=two)
        s1, s2 = (vols[0], vols[1]) if two else (vols, None)
        for thresh in oref.thresholds():
            for dilate in (0, 1, 4):
                want, count = oref.build(s1, s2, thresh, dilate)
                got, n = dev_build(s1, s2, float(thresh), dilate)
                assert (got == want).all() and n == count, (dims, two, thresh, dilate, n, count)
                again, n2 = dev_build(s1, s2, float(thresh), dilate)
                assert (again == got).all() and n2 == n
                if cells % 32:
                    assert int(got[-1]) >> (cells % 32) == 0
                if thresh == -np.inf:
                    assert n == cells


# --------------------------------------------------------------------------- classify
# 70 x 16 = 1120 samples: two 1024-sample tiles, ONE level of tile sums (a single workgroup scans them).
# 65540 x 16 = 1048640 samples: 1025 tiles, more than one 1024-entry tile of sums: the SECOND level of sums and the add pass.
@pytest.mark.parametrize("n,levels", [(70, 1), (65540, 2)])
@pytest.mark.parametrize("outside_empty", (0, 1))
def test_classify_equals_the_restatement(n, levels, outside_empty):
    dims, k = oref.VOLUMES[0], 16
    assert oref.scan_levels(n * k) == levels
    bits, _ = oref.build(oref.case_volume(dims, seed=3), None, 0.8, 0)
    rays, z = oref.case_rays(70, k, seed=7)
    if n > 70:      # the 70 rays over and over, the depths shifted a little per copy so that the tiles differ
        reps = -(-n // 70)
        rays = np.tile(rays, (reps, 1))[:n]
        z = (np.tile(z, (reps, 1)) + (np.arange(reps * 70, dtype=np.float32)[:, None] % 97) * np.float32(0.003))[:n]
    keep = oref.keep_mask(bits, dims, oref.BOX[0], oref.BOX[1], outside_empty, rays, z)
    want, count = oref.slots(keep)
    got, kept = dev_classify(bits, dims, oref.BOX, outside_empty, rays, z)
    assert kept == count and 0 < count < n * k
    assert (got == want).all()
    order = got.reshape(-1)[got.reshape(-1) >= 0]
    assert (order == np.arange(count)).all(), "slot ascends over the kept samples"
    inside = oref.sample_cells(dims, oref.BOX[0], oref.BOX[1], rays, z) >= 0
    assert inside.any() and (~inside).any(), "rays cross and miss the box"


# --------------------------------------------------------------------------- the masked oracle
def draws_for(seed, n=N_RAYS):
    rs = np.random.RandomState(seed)
    return dict(u_coarse=rs.rand(n, KC).astype(np.float32), u_fine=rs.rand(n, KF - KFD).astype(np.float32),
                u_fine2=rs.rand(n, KF - KFD).astype(np.float32), g_depth=rs.randn(n, KFD).astype(np.float32))


def rays_for(seed, n=N_RAYS):
    _, tgt = synth.scene_cameras(1)
    rays = orc.gen_rays(tgt[None], W, H, 0.9 * W, 0.8, 1.8)[0].reshape(-1, 8)
    pick = np.random.RandomState(seed).choice(H * W, n, replace=False)
    return rays[torch.from_numpy(np.sort(pick))].contiguous()


def slab_sigma(t):
    """A synthetic volume whose occupied cells (threshold 0.5, no dilation) are exactly ix < t: corners 1 at x index < t."""
    v = np.zeros(SLAB_DIMS, dtype=np.float32)
    v[:t] = 1.0
    if t > 0:
        assert oref.cells_occupied(v, None, 0.5, 0)[:t].all() and not oref.cells_occupied(v, None, 0.5, 0)[t:].any()
    return v


@functools.lru_cache(maxsize=None)
def scene(ns, with_net):
    return scene_pair(ns, H, W, 512, 4, 5, 3, 8100 + ns, lat_hw=(H // 2, W // 2), with_net=with_net)


@functools.lru_cache(maxsize=None)
def coarse_oracle(ns):
    """The unmasked coarse pass of the oracle, shared by every mask: (rays, draws, z_coarse, per-sample output)."""
    _, sc = scene(ns, False) if not torch.cuda.is_available() else scene(ns, True)
    rays, draws = rays_for(21 + ns), draws_for(31 + ns)
    with torch.no_grad():
        zc = orc.sample_coarse(rays, KC, draws["u_coarse"])
        oc = orc._query_rays(sc, rays, zc, True, 50000).detach()
    return sc, rays, draws, zc, oc


def masked_oracle(ns, bits, dims, box, outside_empty, white):
    """The contract, from the oracle's stages: -> dict of both passes, the keep masks, and the usable rays."""
    sc, rays, draws, zc, oc = coarse_oracle(ns)
    rn = rays.numpy()
    mask = lambda z: oref.keep_mask(bits, dims, box[0], box[1], outside_empty, rn, z.numpy())
    with torch.no_grad():
        keep_c = mask(zc)
        wc, rgbc, dc = orc.composite(rays, zc, oc * torch.from_numpy(keep_c)[..., None].float(), white)
        samps = [zc, orc.sample_fine(rays, wc, draws["u_fine"], draws["u_fine2"], KC), orc.sample_fine_depth(rays, dc, draws["g_depth"], 0.01)]
        zf, _ = torch.sort(torch.cat(samps, dim=-1), dim=-1)
        keep_f = mask(zf)
        of = fine_oracle(ns, zf)
        wf, rgbf, df = orc.composite(rays, zf, of * torch.from_numpy(keep_f)[..., None].float(), white)
    # usable rays, before any run: fine draws clear of the masked cdf's edges; the mask stable under a nudge of every depth
    w = wc + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    ok = ((cdf[:, None, :] - torch.from_numpy(draws["u_fine"])[:, :, None]).abs().amin(dim=(1, 2)) >= MARGIN_CDF).numpy()
    for z, keep in ((zc, keep_c), (zf, keep_f)):
        for nudge in (-MARGIN_Z, MARGIN_Z):
            ok &= (mask(z + nudge) == keep).all(axis=1)
    return dict(rays=rays, draws=draws, ok=ok, keep=(keep_c, keep_f), z=(zc, zf),
                coarse=dict(weights=wc, rgb=rgbc, depth=dc), fine=dict(weights=wf, rgb=rgbf, depth=df))


_FINE_MEMO = {}


def fine_oracle(ns, zf):
    """The oracle's fine MLP at the fine depths; remembered per depth buffer (white and black background, both precisions and
    the slabs whose masked coarse weights coincide share it)."""
    key = (ns, zf.numpy().tobytes())
    if key not in _FINE_MEMO:
        sc, rays = coarse_oracle(ns)[:2]
        with torch.no_grad():
            _FINE_MEMO[key] = orc._query_rays(sc, rays, zf, False, 50000).detach()
    return _FINE_MEMO[key]


def grid_from(sigma, box, outside_empty, thresh=0.5, dilate=0):
    return recon.occupancy_grid(None, box[0], box[1], sigma_thresh=thresh, dilate=dilate, outside_empty=outside_empty,
                                sigma=torch.from_numpy(np.ascontiguousarray(sigma)).to(DEV))


def renderer(white):
    return NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=white).eval()


def culled_render(net, grid, ref, white):
    net.set_occupancy(grid)
    out, dbg = render_debug(renderer(white), net, ref["rays"], ref["draws"], KC, KT)
    return out, dbg, net.last_cull()


def check_against(ref, out, dbg, cull, grid_bits, dims, box, outside_empty, tol=TOL):
    """A culled render against the masked oracle on the rays chosen beforehand; last_cull() against the restatement's mask on
    the depths the device itself drew."""
    ok = ref["ok"]
    assert ok.sum() >= 32, "only %d of %d rays are unambiguous" % (ok.sum(), ok.size)
    sel = torch.from_numpy(ok)
    assert maxabs(dbg["z_coarse"][0], ref["z"][0]) == 0.0
    worst = 0.0
    for p in ("coarse", "fine"):
        for k in ("rgb", "depth", "weights"):
            d = maxabs(out[p][k][0].cpu()[sel], ref[p][k][sel])
            worst = max(worst, d)
            assert d < tol, (p, k, d)
    rn = ref["rays"].numpy()
    for i, (name, zkey) in enumerate((("coarse", "z_coarse"), ("fine", "z_fine"))):
        keep = oref.keep_mask(grid_bits, dims, box[0], box[1], outside_empty, rn, dbg[zkey][0].cpu().numpy())
        assert cull[name] == (int(keep.sum()), keep.size), (name, cull[name], int(keep.sum()))
        # a rejected sample's row of the per-sample buffer is exactly zero, a kept one's is the MLP's
        samp = dbg["sample_" + name][0].cpu().numpy()
        assert (samp[~keep] == 0.0).all()
    return worst


# --------------------------------------------------------------------------- render against the masked oracle
@pytest.mark.parametrize("precision", ["auto", "f32"])
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
@pytest.mark.parametrize("ns", [1, 3])
def test_culled_render_equals_the_masked_oracle(ns, white, precision):
    net, _ = scene(ns, True)
    net.set_matrix_precision(precision)
    counts, worst = [], 0.0
    cases = [(t, True) for t in range(SLAB_DIMS[0])] + [(SLAB_DIMS[0] - 1, False)]
    try:
        for t, outside_empty in cases:
            sigma = slab_sigma(t)
            bits, _ = oref.build(sigma, None, 0.5, 0)
            ref = masked_oracle(ns, bits, SLAB_DIMS, SLAB_BOX, outside_empty, white)
            grid = grid_from(sigma, SLAB_BOX, outside_empty)
            assert (grid.bits.cpu().numpy().view(np.uint32) == bits).all() and grid.n_occupied == t * 16 and grid.n_cells == 8 * 16
            out, dbg, cull = culled_render(net, grid, ref, white)
            worst = max(worst, check_against(ref, out, dbg, cull, bits, SLAB_DIMS, SLAB_BOX, outside_empty))
            counts += [cull["coarse"][0], cull["fine"][0]]
            print("OCCUPANCY-KEPT ns=%d t=%d outside_empty=%d coarse %d/%d fine %d/%d usable rays %d"
                  % (ns, t, outside_empty, *cull["coarse"], *cull["fine"], ref["ok"].sum()))
    finally:
        net.set_occupancy(None)
        net.set_matrix_precision("auto")
    report("masked_oracle_max_abs_diff[ns=%d,%s,%s]" % (ns, "white" if white else "black", precision), "%.3g" % worst)
    assert 0 in counts, counts
    assert any(0 < m < 32 for m in counts), counts
    assert any(m > 64 and m % 64 for m in counts), counts
    assert N_RAYS * KC in counts and N_RAYS * KT in counts, counts


# the issue's case (the volumes' median, dilate 1: on these seeded weights it keeps every cell) and a cut that bites
@pytest.mark.parametrize("quantile,dilate", [(0.5, 1), (0.97, 0)])
def test_grid_learnt_from_the_net_is_held_to_the_same_oracle(quantile, dilate):
    ns, white = 3, True
    net, _ = scene(ns, True)
    box = ((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6))
    try:
        vol = recon.sigma_grid(net, box[0], box[1], (17, 17, 17), coarse=True)
        vol_f = recon.sigma_grid(net, box[0], box[1], (17, 17, 17), coarse=False)
        thresh = float(torch.quantile(torch.cat([vol.reshape(-1), vol_f.reshape(-1)]), quantile, interpolation="lower"))
        grid = recon.occupancy_grid(net, box[0], box[1], (17, 17, 17), sigma_thresh=thresh, dilate=dilate)
        assert grid.dims == (17, 17, 17) and not grid.outside_empty and grid.n_cells == 16 ** 3
        bits = grid.bits.cpu().numpy().view(np.uint32)
        want, count = oref.build(vol.cpu().numpy(), vol_f.cpu().numpy(), thresh, dilate)
        assert (bits == want).all() and grid.n_occupied == count
        report("learnt_grid_occupied_fraction[q=%g,dilate=%d]" % (quantile, dilate), "%.3f (threshold %.4g)" % (count / grid.n_cells, thresh))
        ref = masked_oracle(ns, bits, grid.dims, box, False, white)
        out, dbg, cull = culled_render(net, grid, ref, white)
        worst = check_against(ref, out, dbg, cull, bits, grid.dims, box, False)
        report("learnt_grid_max_abs_diff[q=%g,dilate=%d]" % (quantile, dilate), "%.3g, kept %s" % (worst, cull))
    finally:
        net.set_occupancy(None)


# --------------------------------------------------------------------------- the two ends
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
def test_all_rejected_launches_no_mlp(white):
    ns = 3
    net, _ = scene(ns, True)
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    try:
        grid = grid_from(slab_sigma(0), SLAB_BOX, True)
        net.set_occupancy(grid)
        out, dbg = render_debug(renderer(white), net, rays, draws, KC, KT)
        stats = net.last_mlp_stats(full=True)
        assert stats["launches"] == 0 and stats["flops"] == 0.0
        assert net.last_cull() == {"coarse": (0, N_RAYS * KC), "fine": (0, N_RAYS * KT)}
    finally:
        net.set_occupancy(None)
    for p in ("coarse", "fine"):
        assert float(out[p]["weights"].abs().max()) == 0.0 and float(out[p]["depth"].abs().max()) == 0.0
        assert bool((out[p]["rgb"] == (1.0 if white else 0.0)).all())
        assert float(dbg["sample_" + p].abs().max()) == 0.0
    # the fine depths: the oracle's on zero weights (a flat cdf) and zero depth (the depth samples clamp to near)
    zero_w, zero_d = torch.zeros(N_RAYS, KC), torch.zeros(N_RAYS)
    edges = torch.arange(1, KC + 1, dtype=torch.float32) / KC
    assert float((edges[None, None, :] - torch.from_numpy(draws["u_fine"])[:, :, None]).abs().min()) >= MARGIN_CDF
    samps = [zc, orc.sample_fine(rays, zero_w, draws["u_fine"], draws["u_fine2"], KC), orc.sample_fine_depth(rays, zero_d, draws["g_depth"], 0.01)]
    zf, _ = torch.sort(torch.cat(samps, dim=-1), dim=-1)
    assert maxabs(dbg["z_fine"][0], zf) <= 1e-6


def test_all_kept_is_the_default_render():
    ns, white = 3, True
    net, _ = scene(ns, True)
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    plain, _ = render_debug(renderer(white), net, rays, draws, KC, KT)
    assert net.last_cull() == {"coarse": (0, 0), "fine": (0, 0)}
    try:
        net.set_occupancy(grid_from(slab_sigma(SLAB_DIMS[0]), SLAB_BOX, False))
        out, _ = render_debug(renderer(white), net, rays, draws, KC, KT)
        cull = net.last_cull()
    finally:
        net.set_occupancy(None)
    assert cull == {"coarse": (N_RAYS * KC, N_RAYS * KC), "fine": (N_RAYS * KT, N_RAYS * KT)}
    worst = max(maxabs(out[p][k], plain[p][k]) for p in ("coarse", "fine") for k in ("rgb", "depth", "weights"))
    report("all_kept_max_abs_diff_to_default", "%.3g" % worst)
    assert worst < TOL


# --------------------------------------------------------------------------- f16
def test_f16_mode_against_its_own_masked_samples():
    """Under set_matrix_precision('f16') a culled render against that mode's own UNCULLED per-sample output, masked by the
    restatement on the depths the device drew and composited by pny_composite; the bar is test_gpu_f16.py's RENDER_TOL.
    Measured on one MI355X: 0 (bit-equal)."""
    ns, white, t = 3, True, 5
    net, _ = scene(ns, True)
    L = plib.load()
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    bits, _ = oref.build(slab_sigma(t), None, 0.5, 0)
    rd = dt(rays)
    st = plib.stream_of(torch.device(DEV))

    def composite(z, samp, k):
        w, rgb, d = torch.empty(N_RAYS, k, device=DEV), torch.empty(N_RAYS, 3, device=DEV), torch.empty(N_RAYS, device=DEV)
        plib.check(L.pny_composite(plib.ptr(rd), plib.ptr(z), plib.ptr(samp), N_RAYS, k, int(white), plib.ptr(w), plib.ptr(rgb), plib.ptr(d), st))
        return dict(weights=w, rgb=rgb, depth=d)

    net.set_matrix_precision("f16")
    try:
        net.set_occupancy(grid_from(slab_sigma(t), SLAB_BOX, True))
        out, dbg = render_debug(renderer(white), net, rays, draws, KC, KT)
        cull = net.last_cull()
        net.set_occupancy(None)
        worst = 0.0
        for p, k, coarse in (("coarse", KC, True), ("fine", KT, False)):
            z = dbg["z_" + p][0].contiguous()
            keep = oref.keep_mask(bits, SLAB_DIMS, SLAB_BOX[0], SLAB_BOX[1], True, rays.numpy(), z.cpu().numpy())
            assert cull[p] == (int(keep.sum()), keep.size) and 0 < keep.sum() < keep.size
            xyz = (rd[:, None, :3] + z[..., None] * rd[:, None, 3:6]).reshape(1, -1, 3)
            vd = rd[:, None, 3:6].expand(-1, k, -1).reshape(1, -1, 3)
            with torch.no_grad():
                samp = net(xyz, coarse=coarse, viewdirs=vd)[0].reshape(N_RAYS, k, 4)
            assert net.last_launch_precision() == "f16"
            want = composite(z, (samp * torch.from_numpy(keep).to(DEV)[..., None]).contiguous(), k)
            for name in ("rgb", "depth", "weights"):
                d = maxabs(out[p][name][0], want[name])
                worst = max(worst, d)
                assert d < F16_TOL, (p, name, d)
        report("f16_culled_vs_own_masked_samples_max_abs_diff", "%.3g" % worst)
    finally:
        net.set_occupancy(None)
        net.set_matrix_precision("auto")


# --------------------------------------------------------------------------- state
def test_state_and_refusals():
    ns, white = 1, True
    net, _ = scene(ns, True)
    L = plib.load()
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    ren = renderer(white)
    keys = [(p, k) for p in ("coarse", "fine") for k in ("rgb", "depth", "weights")]
    same = lambda a, b: all(torch.equal(a[p][k], b[p][k]) for p, k in keys)
    grid = grid_from(slab_sigma(5), SLAB_BOX, True)
    try:
        before, _ = render_debug(ren, net, rays, draws, KC, KT)
        net.set_occupancy(grid)
        assert net.occupancy is grid
        one, _ = render_debug(ren, net, rays, draws, KC, KT)
        cull = net.last_cull()
        two, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert same(one, two) and net.last_cull() == cull and 0 < cull["coarse"][0] < cull["coarse"][1]
        assert not same(one, before)
        # the refusals, by name
        with pytest.raises(plib.PnyError, match="occupancy grid attached.*no-grad"):
            ren(net, dt(rays)[None])                                  # grad mode, a training net: _RenderFunction
        with pytest.raises(plib.PnyError, match="bind_parallel.*occupancy grid"):
            _MultiDeviceRenderWrapper(net, ren, [0, 1], False)(dt(rays)[None])
        h = net._scene(0)
        assert L.pny_model_defer_weight_grads(net._h_model, 1, ns, 64, 64) == 0      # (a stash to stash into)
        assert L.pny_scene_stash_next_render(h, 1) == 0
        o, r = plib.RenderOpts(n_coarse=KC), plib.RenderOut()
        assert L.pny_render(h, plib.ptr(dt(rays)), N_RAYS, C.byref(o), C.byref(r), None) == plib.ERR_STATE
        assert b"occupancy grid" in L.pny_last_error()
        assert L.pny_model_defer_weight_grads(net._h_model, 0, ns, 0, 0) == 0
        assert L.pny_scene_set_groups(h, 2) == 0 and L.pny_scene_set_occupancy(
            h, C.c_void_p(grid.bits.data_ptr()), (C.c_int32 * 3)(*grid.dims), (C.c_double * 3)(*grid.c1), (C.c_double * 3)(*grid.c2), 1,
            None) == plib.ERR_ARG and b"grouped" in L.pny_last_error()
        assert L.pny_scene_set_groups(h, 1) == 0
        # cleared again: the render from before the grid was ever set, bit for bit
        net.set_occupancy(None)
        assert net.occupancy is None
        after, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert same(after, before) and net.last_cull() == {"coarse": (0, 0), "fine": (0, 0)}
        # encode() drops the grid on both sides
        net.set_occupancy(grid)
        net.test_encode(net.test_latent)
        assert net.occupancy is None
        again, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert same(again, before) and net.last_cull() == {"coarse": (0, 0), "fine": (0, 0)}
        # ... the library's own copy too, without Python's help: attached through the ABI, dropped by the ABI's encode
        net.set_occupancy(grid)
        net._occupancy = None
        net.test_encode(net.test_latent)
        again, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert same(again, before) and net.last_cull() == {"coarse": (0, 0), "fine": (0, 0)}
        # more or fewer than ONE object
        with pytest.raises(TypeError):
            recon.occupancy_grid(net)                                   # sigma_thresh has no default
        net.num_objs = 2
        with pytest.raises(plib.PnyError, match="ONE encoded object"):
            net.set_occupancy(grid)
        net.num_objs = 1
        net.yolo = True
        with pytest.raises(plib.PnyError, match="YOLO"):
            net.set_occupancy(grid)
    finally:
        net.yolo, net.num_objs = False, 1
        net.set_occupancy(None)
