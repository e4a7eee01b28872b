"""
The model descriptions of tests/test_gpu_model_desc.py without a GPU: what pny_model_create refuses and accepts at the limits of
each field, and the conditions on that file's inputs, checked on the oracle alone -- they are what makes a pass there mean
something.
  * every case finds its relu-safe points at both margins in a pool gs.POOL x the need (its share is printed);
  * the float32 oracle's outputs lie within half the forward bar of the float64 oracle's, for every case;
  * for the cases whose top code frequency is 96 or more (the code's argument is formed in fp32 by contract, and half an ulp of
    an argument of several hundred reaches the top-frequency entries and, through cos(.) * freq, the gradients) the float32
    oracle's gradients lie within 0.5 x RTOL of the float64 oracle's, per tensor: a correct fp32 implementation can then meet
    RTOL.  The same for the render-backward cases.
"""
import ctypes as C

import pytest
import torch

import test_gpu_grad_shapes as gs
import test_gpu_model_desc as md
from helpers import RTOL
from host_tools import built_lib  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib
from test_gpu_parity import TOL

PNY_ERR_ARG, PNY_ERR_NOGPU = -1, -4
ADMIT = 0.5 * RTOL


def create(lib, **over):
    d = dict(d_latent=512, d_hidden=512, d_out=4, n_blocks=5, combine_layer=3, num_freqs=6, freq_factor=1.5, yolo=0, has_fine=1, device=0)
    d.update(over)
    h = C.c_void_p()
    rc = lib.pny_model_create(C.byref(h), C.byref(plib.ModelDesc(**d)))
    msg = lib.pny_last_error().decode() if rc != 0 else ""
    if rc == 0:
        lib.pny_model_destroy(h)
    return rc, msg


REFUSED = [(dict(num_freqs=-1), "num_freqs"), (dict(num_freqs=10), "num_freqs too large (d_in must be <= 64)"),
           (dict(d_out=0), "d_out out of range [1,64]"), (dict(d_out=65), "d_out out of range [1,64]"),
           (dict(n_blocks=0), "n_blocks out of range [1,8]"), (dict(n_blocks=9), "n_blocks out of range [1,8]"),
           (dict(combine_layer=-1), "combine_layer < 0"),
           (dict(d_latent=0), "d_latent must be a positive multiple of 128"), (dict(d_latent=64), "d_latent must be a positive multiple of 128"),
           (dict(d_latent=192), "d_latent must be a positive multiple of 128")]
ACCEPTED = [dict(num_freqs=0), dict(num_freqs=9), dict(num_freqs=9, freq_factor=3.141592653589793), dict(d_out=1, yolo=1, has_fine=0),
            dict(d_out=64, yolo=1, has_fine=0), dict(n_blocks=1, combine_layer=1000), dict(n_blocks=8, combine_layer=8), dict(n_blocks=8, combine_layer=0),
            dict(d_latent=128), dict(d_latent=2048)]


@pytest.mark.parametrize("over,msg", REFUSED, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_create_refuses(built_lib, over, msg):
    """The argument check comes before the device lookup: PNY_ERR_ARG and its message with or without a GPU."""
    rc, got = create(built_lib, **over)
    assert rc == PNY_ERR_ARG and "pny_model_create" in got and msg in got, (over, rc, got)


@pytest.mark.parametrize("over", ACCEPTED, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()))
def test_create_accepts_the_extreme_legal_values(built_lib, over):
    """Past the argument check: without a GPU the call ends in PNY_ERR_NOGPU, with one it succeeds."""
    rc, got = create(built_lib, **over)
    if torch.cuda.is_available():
        assert rc == 0, (over, rc, got)
    else:
        assert rc == PNY_ERR_NOGPU and "no HIP device" in got, (over, rc, got)


def test_table_is_inside_the_abi_limits():
    md.test_cases_hold_their_edges()
    for name, c in md.CASES.items():
        assert 0 <= c["code"][0] <= 9 and md.d_in_of(c) <= 64 and 1 <= c["d_out"] <= 64 and 1 <= c["nb"] <= 8, name
        assert c["cl"] >= 0 and c["L"] % 128 == 0 and c["L"] >= 128, name


# --------------------------------------------------------------------------- input conditions on the oracle alone
@pytest.mark.parametrize("ambig", [gs.AMBIG, gs.AMBIG_DEFAULT])
@pytest.mark.parametrize("name", list(md.CASES))
def test_cases_select_their_points(name, ambig):
    """n relu-safe points out of int(POOL * n) + 24 candidates; nothing else is left out."""
    case = md.CASES[name]
    _, sc = md.scene(name, with_net=False)
    xyz, vd, share = md.pick(sc, case, ambig, md.seed_of(name))
    assert xyz.shape == (case["n"], 3) and vd.shape == (case["n"], 3)
    if case["yolo"]:
        gs.assert_edges(sc, case, xyz)
        print("MODEL-DESC input %-15s margin %.0e: %d points (populations of pick_points)" % (name, ambig, len(xyz)))
    else:
        print("MODEL-DESC input %-15s margin %.0e: relu-safe share %.2f of %d candidates" % (name, ambig, share, int(gs.POOL * case["n"]) + 24))
        assert share * (int(gs.POOL * case["n"]) + 24) >= case["n"]


def test_f16_train_case_selects_its_points():
    r = md.reference("code9", gs.AMBIG_DEFAULT, n=gs.F16_TRAIN_MIN_SAMPLES)
    print("MODEL-DESC input code9 x %d points: relu-safe share %.2f" % (gs.F16_TRAIN_MIN_SAMPLES, r["share"]))
    assert len(r["xyz"]) == gs.F16_TRAIN_MIN_SAMPLES


@pytest.mark.parametrize("name", list(md.CASES))
def test_fp32_oracle_forward_gap(name):
    """max |f32 oracle - f64 oracle| on the case's points: the forward bars (TOL; 1e-4 in the backward body) leave a correct
    fp32 implementation at least half their width."""
    r64 = md.reference(name, gs.AMBIG)
    r32 = md.reference(name, gs.AMBIG, dtype=torch.float32)
    gap = float((r32["ref"].double() - r64["ref"]).abs().max())
    print("MODEL-DESC input %-15s forward: max |f32 - f64| %.2e (max |out| %.2f)" % (name, gap, float(r64["ref"].abs().max())))
    assert gap <= 0.5 * TOL


def gaps(a, b):
    """Per tensor: max |a - b| / max |b|."""
    return {k: float((a[k].double() - b[k]).abs().max()) / max(float(b[k].abs().max()), 1e-20) for k in b}


HIGH_FREQ = [n for n, c in md.CASES.items() if md.top_frequency(c) >= 96.0]


def test_high_frequency_cases_are_the_expected_ones():
    assert HIGH_FREQ == ["code9_pi", "code9", "code7"]


@pytest.mark.parametrize("ambig", [gs.AMBIG, gs.AMBIG_DEFAULT])
@pytest.mark.parametrize("name", HIGH_FREQ)
def test_fp32_oracle_gradient_gap(name, ambig):
    r64 = md.reference(name, ambig)
    r32 = md.reference(name, ambig, dtype=torch.float32)
    g = gaps(r32["params"], r64["params"])
    g["latent"] = gaps({"l": r32["lat"]}, {"l": r64["lat"]})["l"]
    worst = max(g, key=g.get)
    for k in sorted({worst, "lin_in.weight", "latent"}):
        print("MODEL-DESC input %-9s margin %.0e %-22s f32 vs f64 oracle gradient %.2e of the tensor's max%s"
              % (name, ambig, k, g[k], " (the worst tensor)" if k == worst else ""))
    assert g[worst] <= ADMIT, (name, worst, g[worst])


RENDER_NOT_ADMITTED = ("code9",)      # measured 3.7e-4 (mlp_coarse.lin_z.0.weight): the reference alone misses RTOL there


def render_gap(name):
    r64 = md.render_reference(name)
    assert r64["rays"].shape == (md.RENDER["n"], 8)
    r32 = md.render_reference(name, dtype=torch.float32)
    e_rgb = float((r32["fine_rgb"].double() - r64["fine_rgb"]).abs().max())
    g = {}
    for pre in ("mlp_coarse", "mlp_fine"):
        a, b = getattr(r32["sc"], pre), getattr(r64["sc"], pre)
        for k in b:
            if b[k].grad is not None:
                g[pre + "." + k] = gaps({k: a[k].grad}, {k: b[k].grad})[k]
    g["latent"] = gaps({"l": r32["lat"]}, {"l": r64["lat"]})["l"]
    worst = max(g, key=g.get)
    print("MODEL-DESC input render %-15s f32 vs f64 oracle: fine rgb %.2e, worst gradient %.2e (%s)" % (name, e_rgb, g[worst], worst))
    for pre in ("mlp_coarse", "mlp_fine"):       # both MLPs take a gradient worth comparing
        assert float(getattr(r64["sc"], pre)["lin_in.weight"].grad.abs().max()) > 1e-4, pre
    return e_rgb, worst, g[worst]


@pytest.mark.parametrize("name", md.RENDER_CASES)
def test_render_cases_find_their_rays_and_fp32_gap(name):
    """16 relu-safe rays, most depth samples unclamped (render_reference asserts it), and the float32 oracle's render gradients
    within 0.5 x RTOL of the float64 oracle's, fine rgb within half of 1e-4."""
    e_rgb, worst, gap = render_gap(name)
    assert e_rgb <= 0.5e-4 and gap <= ADMIT, (name, e_rgb, worst, gap)


@pytest.mark.parametrize("name", RENDER_NOT_ADMITTED)
def test_render_case_left_out_misses_the_admission(name):
    """Why code9 is not a render-backward case: its float32 reference is further from float64 than the admission allows (if this
    stops holding, the case can be admitted)."""
    assert name not in md.RENDER_CASES and md.top_frequency(md.CASES[name]) > md.top_frequency(md.CASES["code7"])
    e_rgb, worst, gap = render_gap(name)
    assert gap > ADMIT, (name, worst, gap)


def test_yolo_render_case_finds_its_rays():
    sc, rays, u, G = md.yolo_render_inputs()
    z = md.orc.sample_coarse(rays, u.shape[1], u)
    pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(-1, 3)
    taps, zc = gs.projection(sc, pts.numpy())
    live = (zc < 0).all(dim=0)
    print("MODEL-DESC input yolo_render: %d rays, %.2f of the samples live in every view, %.2f with a tap inside"
          % (len(rays), float(live.float().mean()), float((taps > 0).any(dim=0).float().mean())))
    assert float(live.float().mean()) > 0.5 and float((taps > 0).any(dim=0).float().mean()) > 0.25
