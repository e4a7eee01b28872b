"""
What tests/test_gpu_projection.py rests on, checked without a GPU (tests/projection_ref.py): the recorded restatement figures
behind the bars still hold, a flush of f16 denormals would fail every ordinary-magnitude split bar at least tenfold, the
magnitude range include/pnyolo.h states for the split arithmetic is the measured one, the case list covers what the sweep
promises, and the ABI declares the read-out.
"""
import ctypes as C
import re

import numpy as np
import pytest

import projection_ref as pr
from host_tools import built_lib, header_text  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib

HELD_SLACK = 1.1

_ERRS = {}


def errs(case):
    """(float32, split, flushed split) restatement errors of a case against float64, computed once."""
    if case["name"] not in _ERRS:
        x, w, r = pr.reference(case)
        _ERRS[case["name"]] = (pr.err(pr.project32(x, w), r), pr.err(pr.project_split(x, w), r), pr.err(pr.split_flushed(x, w), r))
    return _ERRS[case["name"]]


def held(name, measured, recorded):
    """A measured restatement error against the recorded figure (the bars are twice the RECORDED figure): within 10 % above,
    not below half of it."""
    print("%s: restatement vs float64 %.3e (recorded %.3e, bar %.3e)" % (name, measured, recorded, 2 * recorded))
    assert measured <= HELD_SLACK * recorded, "%s: %.3e exceeds the recorded %.3e" % (name, measured, recorded)
    assert measured >= 0.5 * recorded, "%s: recorded %.3e is more than twice the measured %.3e" % (name, recorded, measured)


@pytest.mark.parametrize("K", pr.KS)
def test_restatement_figures(K):
    mine = [c for c in pr.CASES if c["K"] == K]
    for c in mine:
        print("%-28s float32 %.3e  split %.3e  split, denormals flushed %.3e" % ((c["name"],) + errs(c)))
    held("K %d float32 matmul" % K, max(errs(c)[0] for c in mine), pr.F32_ERR[K])
    tiled = [c for c in mine if c["kind"] == "ordinary" and c["npix"] >= pr.TILED_FROM]
    assert {c["std"] for c in tiled} == set(pr.STD_ORDINARY)
    held("K %d three-product split" % K, max(errs(c)[1] for c in tiled), pr.SPLIT_ERR[K])
    env, = [c for c in mine if c["kind"] == "envelope"]
    held("K %d split at latent std 1e-3" % K, errs(env)[1], pr.ENVELOPE_ERR[K])
    # the envelope is the split arithmetic's own: far above float32 on the same inputs, which stays where it is at any magnitude
    assert errs(env)[1] >= 5 * errs(env)[0] and errs(env)[0] <= HELD_SLACK * pr.F32_ERR[K]


def test_bars_are_twice_the_figures():
    for c in pr.CASES:
        K = c["K"]
        assert pr.bar(c, "fallback") == pr.bar(c, "tiled_f32") == 2 * pr.F32_ERR[K]
        assert pr.bar(c, "tiled_split") == 2 * (pr.ENVELOPE_ERR if c["kind"] == "envelope" else pr.SPLIT_ERR)[K]
    for K in pr.KS:
        assert 0 < pr.SPLIT_ERR[K] <= 1.2 * pr.F32_ERR[K]          # at ordinary magnitudes the split costs nothing
        assert pr.ENVELOPE_ERR[K] < 1e-4 / 2                        # ... and the envelope's bar still sits under the end-to-end one


@pytest.mark.parametrize("K", pr.KS)
def test_a_denormal_flush_would_fail_every_ordinary_bar(K):
    for c in pr.CASES:
        if c["K"] == K and c["kind"] == "ordinary":
            flushed = errs(c)[2]
            print("%-28s flushed %.3e = %.0f x the split bar" % (c["name"], flushed, flushed / pr.bar(c, "tiled_split")))
            assert flushed >= pr.FLUSH_FACTOR * pr.bar(c, "tiled_split"), c["name"]


def test_planes_and_restatements_are_what_they_say():
    rs = np.random.RandomState(3)
    a = (rs.standard_normal(4096) * 0.05).astype(np.float32)
    a1, a2 = pr.planes(a)
    assert a1.dtype == a2.dtype == np.float32
    assert np.array_equal(a1, a.astype(np.float16).astype(np.float32))
    # the rest after two planes: half a unit of the second plane, which below 2^-14 is the denormal spacing 2^-24
    assert float(np.abs(a - (a1 + a2)).max()) <= 2.0 ** -25
    assert float((np.abs(a2) < pr.F16_MIN_NORMAL).mean()) > 0.9                 # "almost every second plane is denormal"
    f1, f2 = pr.planes(a, flush=True)
    assert float(np.abs(f2).max()) == 0.0 or float(np.abs(f2[f2 != 0]).min()) >= pr.F16_MIN_NORMAL
    assert np.array_equal(f1[np.abs(a1) >= pr.F16_MIN_NORMAL], a1[np.abs(a1) >= pr.F16_MIN_NORMAL])
    # small integers: every restatement is exact
    x = rs.randint(-8, 9, size=(37, 128)).astype(np.float32)
    w = rs.randint(-8, 9, size=(64, 128)).astype(np.float32)
    want = pr.project64(x, w)
    for got in (pr.project32(x, w), pr.project_split(x, w), pr.split_flushed(x, w), pr.mm32_blas(x, w)):
        assert np.array_equal(got.astype(np.float64), want)
    # mm32 sums in k order: a cancelling pair in front loses what comes after it only if summed last
    x = np.array([[2.0 ** 24, -2.0 ** 24, 1.0, 1.0]], dtype=np.float32)
    assert float(pr.mm32(x, np.ones((1, 4), dtype=np.float32))[0, 0]) == 2.0
    x = np.array([[2.0 ** 24, 1.0, 1.0, -2.0 ** 24]], dtype=np.float32)
    assert float(pr.mm32(x, np.ones((1, 4), dtype=np.float32))[0, 0]) == 0.0


# the range include/pnyolo.h states beside "22 significant bits" (DESIGN.md 4.1a has the table)
RANGE_FROM, RANGE_BELOW = 0.05, 0.005


@pytest.mark.parametrize("K", pr.KS)
def test_split_magnitude_range(K):
    """Operand magnitudes (standard deviation of the latent, or of the weights) from RANGE_FROM up to 1e3: the split restatement
    stays within 2 x the float32 one.  At RANGE_BELOW it has left that band at every K, and from there its error grows as
    1 / magnitude (the second plane's spacing is fixed at 2^-24)."""
    rs = np.random.RandomState(1)
    w0 = rs.standard_normal((512, K)).astype(np.float32)
    x0 = rs.standard_normal((128, K)).astype(np.float32)
    hdr = re.sub(r"\s+", " ", header_text())
    assert "standard deviation 0.05" in hdr and "1.7e-8 / s" in hdr
    for what in ("latent", "weights"):
        ratio = {}
        for s in (1e3, 1.0, RANGE_FROM, RANGE_BELOW, 1e-3):
            x = x0 * np.float32(s if what == "latent" else 1.0)
            w = w0 * np.float32(np.sqrt(2.0 / K) if what == "latent" else s)
            r = pr.project64(x, w)
            e32, es = pr.err(pr.project32(x, w), r), pr.err(pr.project_split(x, w), r)
            ratio[s] = es / e32
            print("K %4d %-7s std %-6g float32 %.2e split %.2e (%.1f x)" % (K, what, s, e32, es, ratio[s]))
            if s <= 1e-3:
                assert 0.5 * 1.7e-8 / s <= es <= 2 * 1.7e-8 / s
        assert all(ratio[s] <= 2.0 for s in (1e3, 1.0, RANGE_FROM)), (K, what, ratio)
        assert ratio[RANGE_BELOW] > 2.0 and ratio[1e-3] > ratio[RANGE_BELOW], (K, what, ratio)


def test_case_list_covers_the_sweep():
    cs = pr.CASES
    assert {c["K"] for c in cs} == set(pr.KS) and all(K % 128 == 0 for K in pr.KS)
    for K in pr.KS:
        assert {c["nvb"] for c in cs if c["K"] == K} >= {1, 3}
        assert sum(c["kind"] == "envelope" for c in cs if c["K"] == K) == 1
    assert {c["nvb"] for c in cs if c["K"] == 128} == {1, 3, 5}
    assert all(pr.n_blocks_of(c["nvb"]) <= 6 for c in cs)                        # the split route exists
    by_k = lambda K: {(c["npix"], c["ns"], c["hl"], c["wl"]) for c in cs if c["K"] == K}      # noqa: E731
    assert by_k(128) == {(15, 1, 3, 5), (255, 3, 5, 17), (256, 1, 16, 16), (257, 1, 1, 257), (383, 1, 1, 383)}
    assert by_k(1792) >= {(270, 2, 9, 15)} and by_k(512) >= {(5700, 3, 38, 50), (256, 1, 16, 16)}
    assert 5700 % pr.TILE == 68 and 270 % pr.TILE == 14 and 257 % pr.TILE == 1 and 383 % pr.TILE == 127
    for K in pr.KS:                 # every K on every route, and the fallback at both ends of its range somewhere
        assert {pr.expected_route(c, f) for c in cs if c["K"] == K for f in (True, False)} == {"fallback", "tiled_f32", "tiled_split"}
    assert {c["std"] for c in cs} == set(pr.STD_ORDINARY) | {pr.STD_ENVELOPE}
    assert all(c["npix"] >= pr.TILED_FROM for c in cs if c["kind"] == "envelope")
    assert pr.expected_route(pr.BY_NAME["K128_b3_px255_std1"], False) == "fallback"
    assert pr.expected_route(pr.BY_NAME["K128_b1_px256_std1"], False) == "tiled_split"
    assert pr.expected_route(pr.BY_NAME["K128_b1_px256_std1"], True) == "tiled_f32"
    # coarse and fine, and every block, have weights of their own
    w = pr.weights(128, 3)
    mats = w.reshape(6, -1)
    assert all(not np.array_equal(mats[i], mats[j]) for i in range(6) for j in range(i))
    assert abs(float(w.std()) / np.sqrt(2.0 / 128) - 1) < 0.01
    x, wz, r = pr.reference(pr.BY_NAME["K128_b3_px15_std0.05"])
    assert x.shape == (15, 128) and wz.shape == (3 * 512, 128) and r.shape == (15, 3 * 512) and r.dtype == np.float64
    lat = pr.latent(pr.BY_NAME["K128_b3_px15_std0.05"])
    assert np.array_equal(x[(0 * 3 + 2) * 5 + 4], lat[0, :, 2, 4])               # p = (v hl + y) wl + x


def test_abi_declares_the_projection_read_out(built_lib):
    """The route codes are the restatement's (they are the header's: tests/test_cpu_abi.py), and a bad call is refused."""
    assert plib.PROJECTION_ROUTE_TILED == {pr.ROUTE_TILED_F32: "f32", pr.ROUTE_TILED_SPLIT: "f16x2"}
    route = C.c_int(-7)
    assert built_lib.pny_scene_projection(None, 0, None, 0, C.byref(route), None) == -1
    assert b"pny_scene_projection" in built_lib.pny_last_error() and route.value == -7
