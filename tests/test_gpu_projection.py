"""
The latent projection and the layout kernels that feed it (-m gpu, real MI355X), through the read-out pny_scene_projection
(include/pnyolo.h): the pixel-wise GEMM on each of its routes -- the 1x1-convolution path below 256 pixels, the tiled fp32
kernel, the tiled split-f16 kernel (csrc/encoder.hip run_pixel_linear) --, the NCHW <-> NHWC transpose of pny_scene_set_latent /
pny_scene_get_latent (csrc/render_kernels.hip), and the PACK_NT repack that builds the stacked lin_z operand at finalize and at
pny_model_refresh (csrc/pack.hip).  The rest of the suite sees the projected maps only behind a whole MLP at 1e-4.

Every float result is held to float64 on the float32 inputs; the cases, references, bars and where each bar comes from are in
tests/projection_ref.py, and tests/test_cpu_projection_ref.py shows without a GPU that the bars are what they claim to be (and
that a flush of f16 denormals would fail them).  Tiny models (view blocks + 1 residual blocks) built through the C ABI on
supplied latents.  Each sweep test prints one PROJECTION line with its error / bar; test_routes_seen prints the worst per route
and K.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import projection_ref as pr
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
GUARD_ROWS = 128
GUARD_BITS = 0x7FA5C3E1          # a NaN with a payload no kernel produces
PRECISIONS = plib.PRECISION      # name -> PNY_PRECISION_*


def stream():
    return plib.stream_of(torch.device(DEV))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F32).contiguous().to(DEV)


def guarded(n_floats, guard_floats):
    """A NaN-filled device buffer of n_floats with guard_floats of GUARD_BITS behind it."""
    buf = torch.full((n_floats + guard_floats,), float("nan"), device=DEV, dtype=F32)
    buf.view(torch.int32)[n_floats:] = GUARD_BITS
    return buf


def guard_intact(buf, n_floats):
    return bool((buf.view(torch.int32)[n_floats:] == GUARD_BITS).all())


# ------------------------------------------------------------------------------------------------ models and scenes through the ABI
class Model:
    """A model of n_blocks residual blocks, nvb of them per-view, at d_latent K; lin_z weights wz (2, nvb, 512, K) [coarse, fine],
    everything else seeded random weights."""

    def __init__(self, K, nvb, wz, n_blocks=None, has_fine=1):
        self.L = plib.load()
        self.K, self.nvb, self.nb, self.has_fine = K, nvb, n_blocks or pr.n_blocks_of(nvb), has_fine
        desc = plib.ModelDesc(d_latent=K, d_hidden=512, d_out=4, n_blocks=self.nb, combine_layer=nvb, num_freqs=6, freq_factor=1.5,
                              yolo=0, has_fine=has_fine, device=0, enc_use_first_pool=1)
        self.h = C.c_void_p()
        plib.check(self.L.pny_model_create(C.byref(self.h), C.byref(desc)))
        self.state = {}
        for f, pre in enumerate(("mlp_coarse.", "mlp_fine.")[:1 + has_fine]):
            sd = synth.mlp_state(7500 + f, d_latent=K, n_blocks=self.nb, combine_layer=nvb, prefix=pre)
            for b in range(nvb):
                sd[pre + "lin_z.%d.weight" % b] = np.ascontiguousarray(wz[f][b])
            self.state.update(sd)
        self.scenes = []

    def finalize(self):
        for name, a in self.state.items():
            shape = (C.c_int64 * a.ndim)(*a.shape)
            plib.check(self.L.pny_model_load_weights(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        plib.check(self.L.pny_model_finalize(self.h))
        return self

    def bind_all(self):
        """Every MLP tensor on the device where pny_model_refresh reads it; -> name -> device tensor."""
        self.params = {name: dev(a) for name, a in self.state.items()}
        for name, t in self.params.items():
            plib.check(self.L.pny_model_bind_param(self.h, name.encode(), plib.ptr(t)))
        return self.params

    def refresh(self):
        plib.check(self.L.pny_model_refresh(self.h, stream()))

    def scene(self, lat, precision="auto", cameras=False):
        """A scene on latent (ns, K, hl, wl) NCHW."""
        s = C.c_void_p()
        plib.check(self.L.pny_scene_create(C.byref(s), self.h))
        self.scenes.append(s)
        plib.check(self.L.pny_scene_set_precision(s, PRECISIONS[precision]))
        if lat is not None:
            ns, ch, hl, wl = lat.shape
            plib.check(self.L.pny_scene_set_latent(s, plib.ptr(dev(lat)), ns, ch, hl, wl, stream()))
            if cameras:
                poses, _ = synth.scene_cameras(ns)
                focal, c = np.array([[28.8, 28.8]], dtype=np.float32), np.array([[16.0, 16.0]], dtype=np.float32)
                plib.check(self.L.pny_scene_set_cameras(s, np.ascontiguousarray(poses, dtype=np.float32).ctypes.data_as(C.c_void_p), ns,
                                                        focal.ctypes.data_as(C.c_void_p), 1, c.ctypes.data_as(C.c_void_p), 1, 32, 32))
                plib.check(self.L.pny_scene_set_projection(s, plib.PROJECTION["on"]))    # queries read the projected maps
        torch.cuda.synchronize()
        return s

    def close(self):
        torch.cuda.synchronize()
        for s in self.scenes:
            self.L.pny_scene_destroy(s)
        self.L.pny_model_destroy(self.h)
        self.scenes, self.h = [], None


_MODELS = {}


def sweep_model(K, nvb):
    """The sweep's model at (K, view blocks), built once."""
    if (K, nvb) not in _MODELS:
        _MODELS[K, nvb] = Model(K, nvb, pr.weights(K, nvb)).finalize()
    return _MODELS[K, nvb]


def project(model, scene, npix, fine=0):
    """-> (map (npix, nvb 512) on the host, route code, every in-range float finite, guard intact)"""
    n = npix * model.nvb * pr.HID
    buf = guarded(n, GUARD_ROWS * model.nvb * pr.HID)
    route = C.c_int(0)
    plib.check(model.L.pny_scene_projection(scene, fine, plib.ptr(buf), n, C.byref(route), stream()))
    torch.cuda.synchronize()
    out = buf[:n].reshape(npix, model.nvb * pr.HID)
    return out.cpu().numpy(), route.value, bool(torch.isfinite(out).all()), guard_intact(buf, n)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the sweep
class Sweep:
    """Each (case, scene precision) once: error against float64, route, store checks, and a second run for determinism."""

    def __init__(self):
        self.done = {}

    def run(self, case, precision):
        key = (case["name"], precision)
        if key not in self.done:
            m = sweep_model(case["K"], case["nvb"])
            s = m.scene(pr.latent(case), precision)
            got, route, finite, guard = project(m, s, case["npix"])
            again, route2, _, _ = project(m, s, case["npix"])
            self.done[key] = dict(err=pr.err(got, pr.reference(case)[2]) if finite else float("inf"), route=route, finite=finite, guard=guard,
                                  same=route == route2 and np.array_equal(bits(got), bits(again)))
        return self.done[key]


@pytest.fixture(scope="module")
def sweep():
    return Sweep()


SCENES = ("f32", "auto")


@pytest.mark.parametrize("precision", SCENES)
@pytest.mark.parametrize("name", [c["name"] for c in pr.CASES])
def test_projection_vs_fp64(sweep, name, precision):
    """Every case on a scene pinned to F32 and on an AUTO scene: the reported route is the expected one and the error against
    float64, over the map's max, is within the route's bar."""
    case = pr.BY_NAME[name]
    r = sweep.run(case, precision)
    want = pr.expected_route(case, precision == "f32")
    bar = pr.bar(case, want)
    print("PROJECTION %-28s %-4s scene: route %s (%d), error %.3e, bar %.3e (%.2f of the bar)"
          % (name, precision, pr.route_name(r["route"]), r["route"], r["err"], bar, r["err"] / bar))
    assert pr.route_name(r["route"]) == want, (name, precision, r["route"])
    if want == "fallback":
        assert r["route"] in (111, 122, 811, 822)
    assert r["err"] <= bar, (name, precision, r["err"], bar)


def test_routes_seen(sweep):
    """The whole sweep per route and K: worst error / bar, and the fallback's instantiations."""
    worst, inst = {}, set()
    for case in pr.CASES:
        for precision in SCENES:
            r = sweep.run(case, precision)
            route = pr.route_name(r["route"])
            key = (route, case["K"], case["kind"] if route == "tiled_split" else "any")
            worst[key] = max(worst.get(key, (0.0, 1.0)), (r["err"], pr.bar(case, route)), key=lambda t: t[0] / t[1])
            if route == "fallback":
                inst.add((case["K"], r["route"]))
    for (route, K, kind), (e, bar) in sorted(worst.items()):
        print("PROJECTION route %-11s K %4d %-8s worst error %.3e, bar %.3e (%.2f of the bar)" % (route, K, kind, e, bar, e / bar))
    print("PROJECTION fallback instantiations (K, 100 SPLIT + 10 NT + MT): %s" % sorted(inst))
    assert {k[0] for k in worst} == {"fallback", "tiled_f32", "tiled_split"}
    assert {(k[0], k[1]) for k in worst} == {(r, K) for r in ("fallback", "tiled_f32", "tiled_split") for K in pr.KS}
    # if the fallback measures worse than the tiled fp32 kernel, that is recorded, not acted on
    for K in pr.KS:
        print("PROJECTION K %4d fallback %.3e vs tiled fp32 %.3e" % (K, worst["fallback", K, "any"][0], worst["tiled_f32", K, "any"][0]))


@pytest.mark.parametrize("precision", SCENES)
def test_stores_stay_inside(sweep, precision):
    """The output was NaN before the call and has 128 rows of guard behind it: every in-range float is finite afterwards (the
    guarded stores of a ragged last tile leave no pixel out) and no guard bit has changed (they write no pixel too many)."""
    ragged = 0
    for case in pr.CASES:
        r = sweep.run(case, precision)
        assert r["finite"], (case["name"], "a float of the map was not written")
        assert r["guard"], (case["name"], "a store went past the map")
        ragged += case["npix"] % pr.TILE != 0
    assert ragged >= 10


@pytest.mark.parametrize("precision", SCENES)
def test_two_runs_are_bit_identical(sweep, precision):
    for case in pr.CASES:
        assert sweep.run(case, precision)["same"], case["name"]


# ------------------------------------------------------------------------------------------------ position independence
def planted(case, pixels):
    """The case's latent with pixel pixels[0]'s channel row copied to the other pixels (ns = 1 maps)."""
    lat = pr.latent(case).copy()
    assert lat.shape[0] == 1
    flat = lat.reshape(case["K"], -1)
    for p in pixels[1:]:
        flat[:, p] = flat[:, pixels[0]]
    return lat


@pytest.mark.parametrize("precision", SCENES)
@pytest.mark.parametrize("name", ["K128_b5_px383_std1", "K1792_b3_px257_std0.05"])
def test_a_pixels_result_does_not_depend_on_its_position(name, precision):
    """One latent row at pixels 0, 127, 128 and npix - 1 of a ragged map (first and last column of a full tile, first column and
    last live column of the ragged one): on the tiled routes the four projected rows are bit-identical -- a pixel's sum runs in
    the same k order whatever its tile column, and the clamped staging loads of the dead columns do not reach it."""
    case = pr.BY_NAME[name]
    pixels = [0, 127, 128, case["npix"] - 1]
    m = sweep_model(case["K"], case["nvb"])
    got, route, finite, guard = project(m, m.scene(planted(case, pixels), precision), case["npix"])
    assert finite and guard and pr.route_name(route) == pr.expected_route(case, precision == "f32") != "fallback"
    for p in pixels[1:]:
        assert np.array_equal(bits(got[p]), bits(got[pixels[0]])), (name, precision, p)
    assert not np.array_equal(bits(got[1]), bits(got[0]))


def test_position_independence_on_the_fallback_is_reported():
    """The same on the 1x1-convolution path (255 = 3 x 85 pixels as one view): reported, not required."""
    case = dict(pr.BY_NAME["K128_b3_px255_std1"], ns=1, hl=1, wl=255)
    pixels = [0, 31, 32, 127, 128, 254]
    for K, nvb in ((128, 3), (512, 1)):
        c = dict(case, K=K, nvb=nvb)
        m = sweep_model(K, nvb)
        rs = np.random.RandomState(7)
        lat = rs.standard_normal((1, K, 1, 255)).astype(np.float32)
        for p in pixels[1:]:
            lat[0, :, 0, p] = lat[0, :, 0, pixels[0]]
        got, route, finite, guard = project(m, m.scene(lat, "f32"), c["npix"])
        assert finite and guard and pr.route_name(route) == "fallback"
        same = [p for p in pixels[1:] if np.array_equal(bits(got[p]), bits(got[pixels[0]]))]
        print("PROJECTION fallback K %d (instantiation %d): rows %s of %s bit-identical to row 0" % (K, route, same, pixels[1:]))
        assert pr.err(got, pr.project64(pr.rows_of(lat), pr.stacked(pr.weights(K, nvb)[0]))) <= pr.bar(c, "fallback")


# ------------------------------------------------------------------------------------------------ other precisions and models
TILED_CASE = "K128_b3_px257_std1"


def test_f16_and_f16_train_scenes_project_as_auto():
    case = pr.BY_NAME[TILED_CASE]
    m = sweep_model(case["K"], case["nvb"])
    want, route, _, _ = project(m, m.scene(pr.latent(case), "auto"), case["npix"])
    assert route == pr.ROUTE_TILED_SPLIT
    for precision in ("f16x2", "f16", "f16_train"):
        got, r, finite, guard = project(m, m.scene(pr.latent(case), precision), case["npix"])
        assert r == pr.ROUTE_TILED_SPLIT and finite and guard
        assert np.array_equal(bits(got), bits(want)), precision


def test_seven_blocks_project_fp32_on_auto():
    """More than 6 residual blocks: no split-f16 MLP kernel exists, so the AUTO scene's maps are the F32 scene's bit for bit."""
    case = pr.BY_NAME[TILED_CASE]
    m = Model(case["K"], case["nvb"], pr.weights(case["K"], case["nvb"]), n_blocks=7).finalize()
    try:
        a, ra, _, _ = project(m, m.scene(pr.latent(case), "auto"), case["npix"])
        f, rf, _, _ = project(m, m.scene(pr.latent(case), "f32"), case["npix"])
        assert ra == rf == pr.ROUTE_TILED_F32 and np.array_equal(bits(a), bits(f))
        assert pr.err(a, pr.reference(case)[2]) <= pr.bar(case, "tiled_f32")
    finally:
        m.close()


@pytest.mark.parametrize("precision", SCENES)
def test_fine_selects_the_fine_weights(precision):
    case = pr.BY_NAME[TILED_CASE]
    route = pr.expected_route(case, precision == "f32")
    m = sweep_model(case["K"], case["nvb"])
    s = m.scene(pr.latent(case), precision)
    coarse, _, _, _ = project(m, s, case["npix"], fine=0)
    fine, r, finite, guard = project(m, s, case["npix"], fine=1)
    assert finite and guard and pr.route_name(r) == route
    assert pr.err(fine, pr.reference(case, fine=1)[2]) <= pr.bar(case, route)
    assert pr.err(coarse, pr.reference(case, fine=0)[2]) <= pr.bar(case, route)
    assert pr.err(fine, pr.reference(case, fine=0)[2]) > 0.1           # ... and they are not each other's
    # a model without a fine MLP: fine = 1 is the coarse projection
    m1 = Model(case["K"], case["nvb"], pr.weights(case["K"], case["nvb"]), has_fine=0).finalize()
    try:
        s1 = m1.scene(pr.latent(case), precision)
        c1, _, _, _ = project(m1, s1, case["npix"], fine=0)
        f1, _, _, _ = project(m1, s1, case["npix"], fine=1)
        assert np.array_equal(bits(c1), bits(f1)) and np.array_equal(bits(c1), bits(coarse))
    finally:
        m1.close()


# ------------------------------------------------------------------------------------------------ refresh
# (maps of at least 2 x 2 pixels: the query's bilinear lookup divides by hl - 1 and wl - 1, as the reference's does)
REFRESH_CASES = ["K128_b5_px256_std0.05", "K512_b3_px15_std0.05", "K1792_b1_px270_std1"]


def query(m, s, n=64):
    rs = np.random.RandomState(n)
    xyz = dev(rs.uniform(-0.3, 0.3, size=(n, 3)))
    vd = dev(torch.nn.functional.normalize(torch.from_numpy(rs.standard_normal((n, 3)).astype(np.float32)), dim=-1).numpy())
    out = torch.full((n, 4), float("nan"), device=DEV, dtype=F32)
    plib.check(m.L.pny_query(s, plib.ptr(xyz), plib.ptr(vd), n, 1, plib.ptr(out), stream()))
    torch.cuda.synchronize()
    projected = C.c_int(-1)
    plib.check(m.L.pny_scene_last_mlp_stats(s, None, None, None, None, C.byref(projected)))
    assert projected.value == 1
    out = out.cpu().numpy()
    assert np.isfinite(out).all() and not np.array_equal(out[0], out[1])          # a live query: its rows depend on their points
    return out


@pytest.mark.parametrize("name", REFRESH_CASES)
def test_refresh_repacks_as_finalize_and_serves_no_stale_map(name):
    """lin_z weights bound with pny_model_bind_param, changed in place, pny_model_refresh: the projection (both MLPs, F32 and
    AUTO scene) is bit-equal to that of a fresh model finalized with the changed weights -- the device repack of the live
    tensors against the finalize repack --, and a projected query on a scene that had its maps cached differs from the one
    before the refresh and equals the fresh model's."""
    case = pr.BY_NAME[name]
    K, nvb, npix = case["K"], case["nvb"], case["npix"]
    w_old, w_new = pr.weights(K, nvb), pr.weights(K, nvb, seed=1)
    lat = pr.latent(case)
    live = Model(K, nvb, w_old).finalize()
    fresh = Model(K, nvb, w_new).finalize()
    try:
        params = live.bind_all()
        live.refresh()                                         # (a refresh with unchanged weights first: fixes the job table)
        scenes = {p: live.scene(lat, p, cameras=True) for p in SCENES}
        before = {p: project(live, scenes[p], npix)[0] for p in SCENES}
        q_before = {p: query(live, scenes[p]) for p in SCENES}                      # fills the scenes' cached maps
        for p in SCENES:
            assert pr.err(before[p], pr.reference(case)[2]) <= pr.bar(case, pr.expected_route(case, p == "f32"))
        for f, pre in enumerate(("mlp_coarse.", "mlp_fine.")):
            for b in range(nvb):
                params[pre + "lin_z.%d.weight" % b].copy_(dev(w_new[f][b]))
        live.refresh()
        x = pr.rows_of(lat)
        for p in SCENES:
            s_fresh = fresh.scene(lat, p, cameras=True)
            for fine in (0, 1):
                got, r1, finite, guard = project(live, scenes[p], npix, fine)
                want, r2, _, _ = project(fresh, s_fresh, npix, fine)
                assert finite and guard and r1 == r2
                assert np.array_equal(bits(got), bits(want)), (name, p, fine)
                ref = pr.project64(x, pr.stacked(w_new[fine]))
                assert pr.err(got, ref) <= pr.bar(case, pr.expected_route(case, p == "f32")), (name, p, fine)
            assert not np.array_equal(bits(project(live, scenes[p], npix)[0]), bits(before[p]))
            q_after = query(live, scenes[p])
            assert np.isfinite(q_after).all() and not np.array_equal(bits(q_after), bits(q_before[p])), (name, p, "a stale map was served")
            assert np.array_equal(bits(q_after), bits(query(fresh, s_fresh))), (name, p)
    finally:
        live.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------ the read-out's own contract
def test_read_out_refuses_and_leaves_the_cache_alone():
    case = pr.BY_NAME["K128_b1_px256_std1"]
    m = sweep_model(case["K"], case["nvb"])
    L = m.L
    n = case["npix"] * m.nvb * pr.HID
    s = m.scene(pr.latent(case), "auto", cameras=True)
    buf = guarded(n, 1024)
    buf.view(torch.int32)[:] = GUARD_BITS
    assert L.pny_scene_projection(s, 0, plib.ptr(buf), n - 1, None, stream()) == -1 and b"pny_scene_projection" in L.pny_last_error()
    assert L.pny_scene_projection(s, 0, None, n, None, stream()) == -1
    empty = m.scene(None, "auto")
    assert L.pny_scene_projection(empty, 0, plib.ptr(buf), n, None, stream()) == -2 and b"no latent" in L.pny_last_error()
    torch.cuda.synchronize()
    assert guard_intact(buf, 0)                                # no refused call wrote anything
    # works whatever the projection mode, with a NULL route, and leaves the cached maps of the scene as they were
    q0 = query(m, s)
    plib.check(L.pny_scene_set_projection(s, plib.PROJECTION["off"]))
    plib.check(L.pny_scene_projection(s, 0, plib.ptr(buf), n, None, stream()))
    plib.check(L.pny_scene_set_projection(s, plib.PROJECTION["auto"]))
    torch.cuda.synchronize()
    assert pr.err(buf[:n].reshape(case["npix"], -1).cpu().numpy(), pr.reference(case)[2]) <= pr.bar(case, "tiled_split")
    assert np.array_equal(bits(query(m, s)), bits(q0))
    # a model without per-view blocks projects nothing; a model that was never finalized has no weights
    m0 = Model(128, 0, pr.weights(128, 1), n_blocks=2).finalize()
    raw = Model(128, 1, pr.weights(128, 1))
    try:
        s0 = m0.scene(pr.latent(case), "auto")
        assert L.pny_scene_projection(s0, 0, plib.ptr(buf), n, None, stream()) == -1 and b"per-view" in L.pny_last_error()
        sr = raw.scene(pr.latent(case), "auto")
        assert L.pny_scene_projection(sr, 0, plib.ptr(buf), n, None, stream()) == -2 and b"finalize" in L.pny_last_error()
    finally:
        m0.close()
        raw.close()


# ------------------------------------------------------------------------------------------------ layout round trip
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (1, 31), (3, 11), (1, 257)])
def test_latent_layout_round_trip_is_bit_exact(hw, ns):
    """pny_scene_set_latent (NCHW -> NHWC) then pny_scene_get_latent (NHWC -> NCHW) at hl wl = 1, 15, 31, 33, 257 (below, at
    and across the 32 x 32 transpose tile), 1 and 3 views, 128 channels: every word comes back, -0.0 and a NaN payload
    included, into a destination that was NaN-filled and has a guard behind it."""
    hl, wl = hw
    assert hl * wl in (1, 15, 31, 33, 257)
    m = sweep_model(128, 1)
    rs = np.random.RandomState(100 * ns + hl * wl)
    src = rs.standard_normal((ns, 128, hl, wl)).astype(np.float32)
    words = src.view(np.int32).reshape(-1)
    words[0] = np.int32(-2 ** 31)                              # -0.0
    words[-1] = 0x7FC01234                                     # a NaN payload
    words[words.size // 2] = np.int32(-2 ** 31)
    n = src.size
    s = m.scene(src, "auto")
    shape = [C.c_int() for _ in range(4)]
    plib.check(m.L.pny_scene_latent_shape(s, *[C.byref(v) for v in shape]))
    assert [v.value for v in shape] == [ns, 128, hl, wl]
    dst = guarded(n, 4096)
    plib.check(m.L.pny_scene_get_latent(s, plib.ptr(dst), stream()))
    torch.cuda.synchronize()
    assert guard_intact(dst, n)
    assert np.array_equal(dst[:n].view(torch.int32).cpu().numpy(), words)
    # ... and what sits between the two transposes is the channel-last latent: the projection reads pixel rows of it
    if hl * wl * ns >= 15:
        case = dict(K=128, nvb=1, npix=ns * hl * wl, kind="ordinary")
        clean = np.nan_to_num(src, nan=0.5)
        got, route, finite, guard = project(m, m.scene(clean, "f32"), case["npix"])
        assert finite and guard
        ref = pr.project64(pr.rows_of(clean), pr.stacked(pr.weights(128, 1)[0]))
        assert pr.err(got, ref) <= pr.bar(case, pr.route_name(route))
