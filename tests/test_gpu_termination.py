"""
Early ray termination on the device (-m gpu; include/pnyolo.h "early ray termination", csrc/termination.hip, the segment kernels
of csrc/occupancy.hip, csrc/pny_termination.h).

The transmittance update is held to the numpy restatement (tests/termination_ref.py) within K * 2^-22 (pny_termination.h: under
four roundings of 2^-24 per factor, the factors at most 1, so the errors add), the segment classification to it exactly.  A
terminated render is held to the MASKED ORACLE at the project's parity bar of 1e-4, built as test_gpu_occupancy.masked_oracle
builds the grid's: the oracle's public stages, the MLP's output at every sample that is not kept replaced by (0, 0, 0, 0) before
the composite, in both passes, the mask being the restatement's alive_and_keep on the oracle's own per-sample output.

Rays are chosen BEFORE a run, with the oracle alone: a ray is not used when T / t_min lies within 1e-3 of 1 at a boundary
between two segments of either pass (a sigma error at the 1e-4 bar over a depth range of 1.0 moves T by at most 1e-4 relative;
the margin is ten times that), when a fine draw sits within 1e-5 of an edge of the masked coarse cdf or, with a grid, when one of
its samples sits within 2e-5 in depth of a change of the grid's verdict (the grid tests' rules).  At least 32 of the 37 rays must
remain; nothing is excluded after a run.

Measured on one MI355X: largest |diff| to the masked oracle 1.7e-6 under AUTO and 9.8e-7 pinned to F32 with 35 - 37 of 37 rays
usable and 186 / 592 ... 591 / 592 coarse, 317 / 888 ... 876 / 888 fine samples kept; 1.7e-6 with the slab grid as well; 0 to
the all-kept culled render when nothing terminates; 0 under f16 (bar 5e-3); T within 1.8e-7 (K = 16, bar 3.8e-6) and 3.3e-7
(K = 192, bar 4.6e-5) of the restatement's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import occupancy_ref as oref
import pnyolo_oracle as orc
import termination_ref as tref
from helpers import DEV, dt, maxabs, render_debug, scene_pair
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd.render import _MultiDeviceRenderWrapper
from test_gpu_occupancy import (F16_TOL, KC, KF, KFD, KT, MARGIN_CDF, MARGIN_Z, N_RAYS, SLAB_BOX, SLAB_DIMS, TOL, coarse_oracle, fine_oracle,
                                grid_from, renderer, scene, slab_sigma)

pytestmark = pytest.mark.gpu

MARGIN_T = 1e-3
SLAB_T = 4                 # the slab ix < 4 of test_gpu_occupancy


def report(name, value):
    print("TERMINATION-MEASURED %s %s" % (name, value))


def t_bar(K):
    return K * 2.0 ** -22


# --------------------------------------------------------------------------- device calls
def dev_update(rays, z, samp, kb, ke, t_min, T, alive):
    """One pny_termination_update on device tensors T (n) fp32 and alive (n) uint8, in place; -> the alive count."""
    L = plib.load()
    n, k = z.shape
    count = torch.full((1,), -7, device=DEV, dtype=torch.int64)
    plib.check(L.pny_termination_update(plib.ptr(rays), plib.ptr(z), plib.ptr(samp), n, k, kb, ke, t_min, plib.ptr(T),
                                        C.c_void_p(alive.data_ptr()), C.c_void_p(count.data_ptr()), plib.stream_of(torch.device(DEV))))
    return int(count.item())


def dev_classify_segment(bits, dims, box, outside_empty, rays, z, kb, ke, alive):
    L = plib.load()
    n, k = z.shape
    need = C.c_int64(0)
    plib.check(L.pny_occupancy_classify_workspace_bytes(n * (ke - kb), C.byref(need)))
    b = None if bits is None else torch.from_numpy(bits.view(np.int32).copy()).to(DEV)
    a = None if alive is None else torch.from_numpy(alive.astype(np.uint8)).to(DEV)
    r, zz = dt(rays), dt(z)
    slot = torch.full((n, ke - kb), -9, device=DEV, dtype=torch.int32)
    kept = torch.full((1,), -7, device=DEV, dtype=torch.int64)
    ws = torch.empty(need.value, device=DEV, dtype=torch.uint8)
    plib.check(L.pny_occupancy_classify_segment(
        None if b is None else C.c_void_p(b.data_ptr()), None if b is None else (C.c_int32 * 3)(*dims),
        None if b is None else (C.c_double * 3)(*box[0]), None if b is None else (C.c_double * 3)(*box[1]), int(outside_empty),
        C.c_void_p(r.data_ptr()), C.c_void_p(zz.data_ptr()), n, k, kb, ke, None if a is None else C.c_void_p(a.data_ptr()),
        C.c_void_p(slot.data_ptr()), C.c_void_p(kept.data_ptr()), C.c_void_p(ws.data_ptr()), need.value, plib.stream_of(torch.device(DEV))))
    return slot.cpu().numpy(), int(kept.item())


# --------------------------------------------------------------------------- 1: the transmittance update
def update_case(name):
    """(rays, z, samp, S, t_min) fp32 numpy."""
    if name == "oracle":              # 70 rays x 16 samples, the oracle's own per-sample output of the test scene, S = 4
        sc, rays, draws, zc, oc = coarse_oracle(3)
        r, z, s = (np.concatenate([v.numpy(), v.numpy()[:70 - N_RAYS]]) for v in (rays, zc, oc))
        s = s.copy()
        s[N_RAYS:, :, 3] *= 7.0       # (the second copy more opaque: rays die at different boundaries)
        return r, z, s, 4, 0.5
    rng = np.random.default_rng(len(name))
    n, K, S = (5, 192, 2) if name == "chunks" else (9, 24, 5)
    z = np.sort(rng.uniform(0.8, 1.8, size=(n, K)).astype(np.float32), axis=1)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 3:6], rays[:, 6], rays[:, 7] = (0.0, 0.0, 1.0), 0.8, 1.8
    samp = rng.uniform(0.0, 1.0, size=(n, K, 4)).astype(np.float32)
    samp[..., 3] = rng.uniform(-2.0, 30.0 if name == "uneven" else 3.0, size=(n, K))      # sigma < 0 among them
    samp[1, 3, 3] = np.nan            # a NaN sigma counts as 0
    samp[2] = 0.0                     # a ray of culled rows: every factor exactly 1
    z[3, -1] = 1.9                    # a depth beyond far: a negative last delta, a factor above 1
    samp[3, -1, 3] = 5.0
    samp[4, :, 3] = 40.0              # an opaque ray: dead at the first boundary
    return rays, z, samp, S, (0.05 if name == "chunks" else 0.3)


@pytest.mark.parametrize("name", ["oracle", "chunks", "uneven"])
def test_update_equals_the_restatement(name):
    rays, z, samp, S, t_min = update_case(name)
    n, K = z.shape
    b = tref.bounds(K, S)
    if name == "chunks":
        assert b == [0, 96, 192]
    if name == "uneven":
        assert np.diff(b).tolist() == [4, 5, 5, 5, 5]
    want_T = tref.transmittance(rays, z, samp)[:, b]                    # (n, S' + 1), on the UNMASKED samples: the stage is model-free
    rd, zd, sd = dt(rays), dt(z), dt(samp)
    runs = []
    for _ in range(2):
        T = torch.ones(n, device=DEV)
        alive = torch.ones(n, device=DEV, dtype=torch.uint8)
        now = np.ones(n, dtype=bool)
        trace = []
        for j in range(len(b) - 1):
            count = dev_update(rd, zd, sd, b[j], b[j + 1], t_min, T, alive)
            got_T, got_alive = T.cpu().numpy(), alive.cpu().numpy().astype(bool)
            trace.append((got_T.copy(), got_alive.copy(), count))
            with np.errstate(invalid="ignore"):
                err = np.abs(got_T - want_T[:, j + 1])
                finite = np.isfinite(want_T[:, j + 1])
                assert (np.isfinite(got_T) == finite).all()
                assert (err[finite] <= t_bar(K)).all(), (name, j, err[finite].max())
                now_want = now & ~(want_T[:, j + 1] < np.float32(t_min))
                clear = ~(np.abs(want_T[:, j + 1].astype(np.float64) / t_min - 1.0) < MARGIN_T)
            # (a ray within the margin may go either way, and then its later bytes follow the device's own choice)
            settled = clear & (got_alive == now_want) | ~clear
            assert settled.all(), (name, j)
            assert (~got_alive | now).all(), "a ray that dies stays dead"
            now = got_alive
            assert count == int(got_alive.sum())
        runs.append(trace)
    for (T1, a1, c1), (T2, a2, c2) in zip(*runs):
        assert T1.tobytes() == T2.tobytes() and (a1 == a2).all() and c1 == c2, "a second call gives the same bits"
    final = runs[0][-1]
    report("update_max_abs_T_error[%s]" % name, "%.3g (bar %.3g), alive at the end %d / %d"
           % (np.nanmax(np.abs(final[0] - want_T[:, -1])), t_bar(K), final[2], n))
    if name != "oracle":
        assert final[1][2] and final[0][2] == 1.0, "culled rows leave T at exactly 1"
    assert 0 < final[2] < n, "the case has rays that die and rays that live"


# --------------------------------------------------------------------------- 2: the segment classification
@pytest.mark.parametrize("leg", ["alive", "grid", "both"])
def test_classify_segment_equals_the_restatement(leg):
    dims, K, S, n = oref.VOLUMES[0], 16, 4, 70
    bits, _ = oref.build(oref.case_volume(dims, seed=3), None, 0.8, 0)
    rays, z = oref.case_rays(n, K, seed=7)
    alive = None if leg == "grid" else (np.random.default_rng(5).random(n) < 0.6)
    grid = leg != "alive"
    full = oref.keep_mask(bits, dims, oref.BOX[0], oref.BOX[1], 1, rays, z) if grid else np.ones((n, K), dtype=bool)
    if alive is not None:
        full = full & alive[:, None]
    b = tref.bounds(K, S)
    for j in range(S):
        want, count = oref.slots(full[:, b[j]:b[j + 1]])
        got, kept = dev_classify_segment(bits if grid else None, dims, oref.BOX, 1, rays, z, b[j], b[j + 1], alive)
        assert kept == count and (got == want).all(), (leg, j, kept, count)
        assert 0 < count < n * (b[j + 1] - b[j])


def test_classify_segment_second_level_of_sums():
    """65540 x 16 samples in ONE segment: 1025 tiles, the second level of sums, with the column addressing and an alive mask."""
    dims, K, n = oref.VOLUMES[0], 16, 65540
    assert oref.scan_levels(n * K) == 2
    bits, _ = oref.build(oref.case_volume(dims, seed=3), None, 0.8, 0)
    rays, z = oref.case_rays(70, K, seed=7)
    reps = -(-n // 70)
    rays = np.tile(rays, (reps, 1))[:n]
    z = (np.tile(z, (reps, 1)) + (np.arange(reps * 70, dtype=np.float32)[:, None] % 97) * np.float32(0.003))[:n]
    alive = np.random.default_rng(6).random(n) < 0.7
    keep = oref.keep_mask(bits, dims, oref.BOX[0], oref.BOX[1], 0, rays, z) & alive[:, None]
    want, count = oref.slots(keep)
    got, kept = dev_classify_segment(bits, dims, oref.BOX, 0, rays, z, 0, K, alive)
    assert kept == count and 0 < count < n * K
    assert (got == want).all()


# --------------------------------------------------------------------------- the masked oracle
def terminated_oracle(ns, t_min, S, white, grid=None):
    """The contract, from the oracle's stages: -> dict of both passes, the keep masks, the alive sets and the usable rays.
    grid: None, or (bits, dims, box, outside_empty)."""
    sc, rays, draws, zc, oc = coarse_oracle(ns)
    rn = rays.numpy()
    if grid is None:
        gmask = lambda z: None
    else:
        gmask = lambda z: oref.keep_mask(grid[0], grid[1], grid[2][0], grid[2][1], grid[3], rn, z.numpy())
    with torch.no_grad():
        alive_c, keep_c, T_c = tref.alive_and_keep(rn, zc.numpy(), oc.numpy(), t_min, S, gmask(zc))
        wc, rgbc, dc = orc.composite(rays, zc, oc * torch.from_numpy(keep_c)[..., None].float(), white)
        samps = [zc, orc.sample_fine(rays, wc, draws["u_fine"], draws["u_fine2"], KC), orc.sample_fine_depth(rays, dc, draws["g_depth"], 0.01)]
        zf, _ = torch.sort(torch.cat(samps, dim=-1), dim=-1)
        of = fine_oracle(ns, zf)
        alive_f, keep_f, T_f = tref.alive_and_keep(rn, zf.numpy(), of.numpy(), t_min, S, gmask(zf))
        wf, rgbf, df = orc.composite(rays, zf, of * torch.from_numpy(keep_f)[..., None].float(), white)
    # usable rays, before any run
    w = wc + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    ok = ((cdf[:, None, :] - torch.from_numpy(draws["u_fine"])[:, :, None]).abs().amin(dim=(1, 2)) >= MARGIN_CDF).numpy()
    ok &= tref.clear_of_threshold(T_c, t_min, MARGIN_T) & tref.clear_of_threshold(T_f, t_min, MARGIN_T)
    if grid is not None:
        for z in (zc, zf):
            for nudge in (-MARGIN_Z, MARGIN_Z):
                ok &= (gmask(z + nudge) == gmask(z)).all(axis=1)
    return dict(rays=rays, draws=draws, ok=ok, keep=(keep_c, keep_f), alive=(alive_c, alive_f), z=(zc, zf),
                coarse=dict(weights=wc, rgb=rgbc, depth=dc), fine=dict(weights=wf, rgb=rgbf, depth=df))


def check_render(ref, out, dbg, cull, tol=TOL):
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
    for i, name in enumerate(("coarse", "fine")):
        keep = ref["keep"][i]
        samp = dbg["sample_" + name][0].cpu().numpy()
        assert (samp[ok][~keep[ok]] == 0.0).all(), "a sample that was not kept has an exactly zero row"
        if ok.all():
            assert cull[name] == (int(keep.sum()), keep.size), (name, cull[name], int(keep.sum()))
    return worst


def terminated_render(net, ref, white, t_min, S):
    net.set_termination(t_min, S)
    out, dbg = render_debug(renderer(white), net, ref["rays"], ref["draws"], KC, KT)
    return out, dbg, net.last_cull(), net.last_termination()


# --------------------------------------------------------------------------- 3: render against the masked oracle
@pytest.mark.parametrize("precision", ["auto", "f32"])
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
@pytest.mark.parametrize("ns", [1, 3])
def test_terminated_render_equals_the_masked_oracle(ns, white, precision):
    net, _ = scene(ns, True)
    net.set_matrix_precision(precision)
    worst = 0.0
    try:
        for t_min in (0.9, 0.5):
            for S in (2, 4, 16):
                ref = terminated_oracle(ns, t_min, S, white)
                out, dbg, cull, segs = terminated_render(net, ref, white, t_min, S)
                worst = max(worst, check_render(ref, out, dbg, cull))
                print("TERMINATION-KEPT ns=%d t_min=%g S=%d coarse %d/%d fine %d/%d usable rays %d segments %d+%d"
                      % (ns, t_min, S, *cull["coarse"], *cull["fine"], ref["ok"].sum(), len(segs["coarse"]), len(segs["fine"])))
                for name in ("coarse", "fine"):
                    assert cull[name][1] == N_RAYS * (KC if name == "coarse" else KT)
                    assert sum(k for _, k in segs[name]) == cull[name][0] and 1 <= len(segs[name]) <= S
                    assert segs[name][0][0] == N_RAYS
                if t_min == 0.9:
                    assert cull["coarse"][0] < cull["coarse"][1] and cull["fine"][0] < cull["fine"][1]
                if ref["ok"].all():
                    for i, name in enumerate(("coarse", "fine")):
                        assert [a for a, _ in segs[name]] == ref["alive"][i].sum(axis=0)[:len(segs[name])].tolist()
    finally:
        net.set_termination(None)
        net.set_matrix_precision("auto")
    report("masked_oracle_max_abs_diff[ns=%d,%s,%s]" % (ns, "white" if white else "black", precision), "%.3g" % worst)


# --------------------------------------------------------------------------- 4: with a grid
@pytest.mark.parametrize("outside_empty", [True, False])
def test_with_a_grid_against_the_oracle_masked_by_both(outside_empty):
    ns, white, t_min, S = 3, True, 0.9, 4
    net, _ = scene(ns, True)
    sigma = slab_sigma(SLAB_T)
    bits, _ = oref.build(sigma, None, 0.5, 0)
    ref = terminated_oracle(ns, t_min, S, white, grid=(bits, SLAB_DIMS, SLAB_BOX, outside_empty))
    try:
        net.set_occupancy(grid_from(sigma, SLAB_BOX, outside_empty))
        out, dbg, cull, segs = terminated_render(net, ref, white, t_min, S)
        worst = check_render(ref, out, dbg, cull)
        grid_only = oref.keep_mask(bits, SLAB_DIMS, SLAB_BOX[0], SLAB_BOX[1], outside_empty, ref["rays"].numpy(), ref["z"][0].numpy())
        print("TERMINATION-KEPT grid outside_empty=%d coarse %d/%d fine %d/%d usable rays %d, the grid alone keeps %d coarse"
              % (outside_empty, *cull["coarse"], *cull["fine"], ref["ok"].sum(), grid_only.sum()))
        assert cull["coarse"][0] < cull["coarse"][1] and cull["fine"][0] < cull["fine"][1]
    finally:
        net.set_termination(None)
        net.set_occupancy(None)
    report("grid_and_termination_max_abs_diff[outside_empty=%d]" % outside_empty, "%.3g" % worst)


# --------------------------------------------------------------------------- 5: nothing terminates
def test_nothing_terminates_is_the_all_kept_culled_render():
    ns, white, S = 3, True, 4
    net, _ = scene(ns, True)
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    try:
        net.set_occupancy(grid_from(slab_sigma(SLAB_DIMS[0]), SLAB_BOX, False))      # every cell occupied: the all-kept culled render
        plain, _ = render_debug(renderer(white), net, rays, draws, KC, KT)
        assert net.last_cull() == {"coarse": (N_RAYS * KC, N_RAYS * KC), "fine": (N_RAYS * KT, N_RAYS * KT)}
        net.set_occupancy(None)
        net.set_termination(0.1, S)
        out, _ = render_debug(renderer(white), net, rays, draws, KC, KT)
        cull, segs = net.last_cull(), net.last_termination()
    finally:
        net.set_occupancy(None)
        net.set_termination(None)
    assert cull == {"coarse": (N_RAYS * KC, N_RAYS * KC), "fine": (N_RAYS * KT, N_RAYS * KT)}
    assert segs == {"coarse": [(N_RAYS, N_RAYS * KC // S)] * S, "fine": [(N_RAYS, N_RAYS * KT // S)] * S}
    worst = max(maxabs(out[p][k], plain[p][k]) for p in ("coarse", "fine") for k in ("rgb", "depth", "weights"))
    report("nothing_terminates_max_abs_diff_to_all_kept", "%.3g" % worst)
    assert worst < TOL


# --------------------------------------------------------------------------- 6: on, off, persistence
def test_on_off_and_persistence():
    ns, white = 1, True
    net, _ = scene(ns, True)
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    ren = renderer(white)
    keys = [(p, k) for p in ("coarse", "fine") for k in ("rgb", "depth", "weights")]
    same = lambda a, b: all(torch.equal(a[p][k], b[p][k]) for p, k in keys)
    zeros = {"coarse": (0, 0), "fine": (0, 0)}
    try:
        before, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert net.termination is None and net.last_termination() == {"coarse": [], "fine": []}
        net.set_termination(0.9, 4)
        assert net.termination == (0.9, 4)
        one, _ = render_debug(ren, net, rays, draws, KC, KT)
        cull, segs = net.last_cull(), net.last_termination()
        two, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert same(one, two) and net.last_cull() == cull and net.last_termination() == segs
        assert 0 < cull["coarse"][0] < cull["coarse"][1] and not same(one, before)
        # the setting is a rendering option: it survives encode(), on both sides
        net.test_encode(net.test_latent)
        assert net.termination == (0.9, 4)
        again, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert same(again, one) and net.last_cull() == cull
        # off: the frame from before the mode was ever set, bit for bit
        net.set_termination(None)
        assert net.termination is None
        after, _ = render_debug(ren, net, rays, draws, KC, KT)
        assert same(after, before) and net.last_cull() == zeros and net.last_termination() == {"coarse": [], "fine": []}
        # a grid without termination: today's path, ONE classification and one wait per pass
        net.set_occupancy(grid_from(slab_sigma(5), SLAB_BOX, True))
        render_debug(ren, net, rays, draws, KC, KT)
        cull, segs = net.last_cull(), net.last_termination()
        assert segs == {"coarse": [(N_RAYS, cull["coarse"][0])], "fine": [(N_RAYS, cull["fine"][0])]}
        with pytest.raises(ValueError):
            net.set_termination(1.0)
        with pytest.raises(ValueError):
            net.set_termination(0.5, 17)
    finally:
        net.set_occupancy(None)
        net.set_termination(None)


# --------------------------------------------------------------------------- 7: refusals
def test_refusals():
    ns, white = 1, True
    net, _ = scene(ns, True)
    L = plib.load()
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    ren = renderer(white)
    try:
        net.set_termination(0.5, 4)
        with pytest.raises(plib.PnyError, match="early ray termination on.*no-grad"):
            ren(net, dt(rays)[None])                                  # grad mode, a training net
        with pytest.raises(plib.PnyError, match="bind_parallel.*early ray termination"):
            _MultiDeviceRenderWrapper(net, ren, [0, 1], False)(dt(rays)[None])
        h = net._scene(0)
        assert L.pny_model_defer_weight_grads(net._h_model, 1, ns, 64, 64) == 0      # (a stash to stash into)
        assert L.pny_scene_stash_next_render(h, 1) == 0
        o, r = plib.RenderOpts(n_coarse=KC), plib.RenderOut()
        assert L.pny_render(h, plib.ptr(dt(rays)), N_RAYS, C.byref(o), C.byref(r), None) == plib.ERR_STATE
        assert b"early ray termination" in L.pny_last_error()
        assert L.pny_model_defer_weight_grads(net._h_model, 0, ns, 0, 0) == 0
        # a grouped scene: refused by name, and grouping a scene switches the mode off
        net.set_termination(None)
        assert L.pny_scene_set_groups(h, 2) == 0 and L.pny_scene_set_termination(h, 0.5, 4) == plib.ERR_ARG
        assert b"grouped" in L.pny_last_error()
        assert L.pny_scene_set_groups(h, 1) == 0
        for t_min, S, text in ((float("nan"), 4, b"NaN"), (1.0, 4, b"[0,1)"), (-0.1, 4, b"[0,1)"), (0.5, 0, b"segments"), (0.5, 17, b"segments")):
            assert L.pny_scene_set_termination(h, t_min, S) == plib.ERR_ARG and text in L.pny_last_error(), (t_min, S)
        # more or fewer than ONE object, a YOLO net
        net.num_objs = 2
        with pytest.raises(plib.PnyError, match="ONE encoded object"):
            net.set_termination(0.5)
        net.num_objs = 1
        net.yolo = True
        with pytest.raises(plib.PnyError, match="YOLO"):
            net.set_termination(0.5)
    finally:
        net.yolo, net.num_objs = False, 1
        net.set_termination(None)


def test_a_yolo_model_is_refused_by_the_library():
    net, _ = scene_pair(2, 64, 64, 1792, 21, 5, 3, 8300, yolo=True, lat_hw=(8, 8))
    L = plib.load()
    assert L.pny_scene_set_termination(net._scene(0), 0.5, 4) == plib.ERR_ARG and b"YOLO" in L.pny_last_error()
    assert L.pny_scene_set_termination(net._scene(0), 0.0, 4) == plib.OK


# --------------------------------------------------------------------------- 8: f16
def test_f16_mode_against_its_own_masked_samples():
    """Under set_matrix_precision('f16') a terminated render against that mode's own UNTERMINATED per-sample output, masked by
    the restatement on the depths the device drew and composited by pny_composite; the bar is test_gpu_f16.py's RENDER_TOL.  The
    usable rays follow from that mode's own sigma, before the terminated run."""
    ns, white, t_min, S = 3, True, 0.9, 4
    net, _ = scene(ns, True)
    L = plib.load()
    sc, rays, draws, zc, _ = coarse_oracle(ns)
    rd, rn = dt(rays), rays.numpy()
    st = plib.stream_of(torch.device(DEV))

    def composite(z, samp, k):
        w, rgb, d = torch.empty(N_RAYS, k, device=DEV), torch.empty(N_RAYS, 3, device=DEV), torch.empty(N_RAYS, device=DEV)
        plib.check(L.pny_composite(plib.ptr(rd), plib.ptr(z), plib.ptr(samp), N_RAYS, k, int(white), plib.ptr(w), plib.ptr(rgb), plib.ptr(d), st))
        return dict(weights=w, rgb=rgb, depth=d)

    def own_samples(z, k, coarse):
        xyz = (rd[:, None, :3] + z[..., None] * rd[:, None, 3:6]).reshape(1, -1, 3)
        vd = rd[:, None, 3:6].expand(-1, k, -1).reshape(1, -1, 3)
        with torch.no_grad():
            samp = net(xyz, coarse=coarse, viewdirs=vd)[0].reshape(N_RAYS, k, 4)
        assert net.last_launch_precision() == "f16"
        return samp

    net.set_matrix_precision("f16")
    try:
        # the mode's own coarse pass decides the usable rays and the coarse mask before the terminated run
        zc_d = dt(zc)
        samp_c = own_samples(zc_d, KC, True)
        _, keep_c, T_c = tref.alive_and_keep(rn, zc.numpy(), samp_c.cpu().numpy(), t_min, S)
        ok = tref.clear_of_threshold(T_c, t_min, MARGIN_T)
        want_c = composite(zc_d, (samp_c * torch.from_numpy(keep_c).to(DEV)[..., None]).contiguous(), KC)
        w = want_c["weights"].cpu() + 1e-5
        cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
        ok &= ((cdf[:, None, :] - torch.from_numpy(draws["u_fine"])[:, :, None]).abs().amin(dim=(1, 2)) >= MARGIN_CDF).numpy()
        # the fine depths that follow from the mode's own masked coarse pass, by the fine sampling's stage entry
        zf_d = torch.empty(N_RAYS, KT, device=DEV)
        u1, u2, g = dt(draws["u_fine"]), dt(draws["u_fine2"]), dt(draws["g_depth"])
        plib.check(L.pny_sample_fine(plib.ptr(rd), plib.ptr(zc_d), plib.ptr(want_c["weights"]), plib.ptr(want_c["depth"]), N_RAYS, KC, KF,
                                     KFD, 0.01, 0, plib.ptr(u1), plib.ptr(u2), plib.ptr(g), 0, plib.ptr(zf_d), st))
        samp_f = own_samples(zf_d, KT, False)
        _, keep_f, T_f = tref.alive_and_keep(rn, zf_d.cpu().numpy(), samp_f.cpu().numpy(), t_min, S)
        ok &= tref.clear_of_threshold(T_f, t_min, MARGIN_T)
        assert ok.sum() >= 32, "only %d of %d rays are unambiguous" % (ok.sum(), ok.size)
        net.set_termination(t_min, S)
        out, dbg = render_debug(renderer(white), net, rays, draws, KC, KT)
        cull = net.last_cull()
        net.set_termination(None)
        want_f = composite(zf_d, (samp_f * torch.from_numpy(keep_f).to(DEV)[..., None]).contiguous(), KT)
        sel = torch.from_numpy(ok).to(DEV)
        worst = 0.0
        for p, want in (("coarse", want_c), ("fine", want_f)):
            for name in ("rgb", "depth", "weights"):
                d = maxabs(out[p][name][0][sel], want[name][sel])
                worst = max(worst, d)
                assert d < F16_TOL, (p, name, d)
        assert 0 < cull["coarse"][0] < cull["coarse"][1] and 0 < cull["fine"][0] < cull["fine"][1]
        report("f16_terminated_vs_own_masked_samples_max_abs_diff", "%.3g, usable rays %d, kept %s" % (worst, ok.sum(), cull))
    finally:
        net.set_termination(None)
        net.set_matrix_precision("auto")
