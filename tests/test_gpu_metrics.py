"""
The view metrics on the GPU (csrc/metrics.hip, include/pnyolo.h pny_view_metrics, metrics.compare_views / metrics.psnr) against
the fp64 restatement of the reference's scoring (tests/metrics_ref.py: skimage's SSIM on scipy's uniform_filter):
  * shape sweep: 3 non-square views whose window counts H - 6 and W - 6 take every value of {1, 2, T - 1, T, T + 1, 2 T + 1}
    once per axis (one window, one row of windows, a tile filled exactly, one window spilling into the next tile), plus one
    shape with three tiles on both axes; unclamped predictions so that the clamp is exercised;
  * both ground-truth layouts give identical bits; closed forms; low-contrast and bright pairs; 67 views of 7 x 7;
  * run-to-run bits, also after another shape used the same workspace; either output alone equals the combined call;
  * a NaN pixel makes ITS view's two metrics NaN and its byte 0;  metrics.psnr as vis_step uses it;
  * end to end: encode, render two 32 x 32 views, score them; equal to the restatement on the rendered tensor.

Tolerances come from the restatement's fp64 arithmetic, not from the kernel: SSIM 1e-9 absolute (a different fp64 summation
order measures about 1e-12, fp32 sums 1e-6 to 4e-5: tests/test_cpu_metrics.py), the MSE 1e-12 relative (at most 3 * 39 * 71
fp64 additions of positive terms: some 1e-14 in any order), PSNR 1e-9 dB; the bytes are bit-equal.
"""
import numpy as np
import pytest
import torch

import metrics_ref as mr
from helpers import DEV, load_mlp
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import metrics as pmetrics
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd import util as putil
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer

pytestmark = pytest.mark.gpu

T_H, T_W = 16, 32       # output windows per tile (csrc/pny_metrics.h METRICS_TILE_H, METRICS_TILE_W)
SSIM_TOL, MSE_RTOL, PSNR_TOL = 1e-9, 1e-12, 1e-9
# H - 6 over {1, 2, T_H - 1, T_H, T_H + 1, 2 T_H + 1}, W - 6 over the same of T_W, each once; then three tiles on both axes
SWEEP = [(1 + 6, T_W + 6), (2 + 6, 2 * T_W + 1 + 6), (T_H - 1 + 6, 1 + 6), (T_H + 6, T_W + 1 + 6), (T_H + 1 + 6, 2 + 6),
         (2 * T_H + 1 + 6, T_W - 1 + 6), (2 * T_H + 1 + 6, 2 * T_W + 1 + 6)]


def make_pair(seed, nv, h, w, sigma=0.05):
    """Random ground truth in [0, 1] and prediction = ground truth + N(0, sigma), unclamped; fp32 (NV, H, W, 3)."""
    rs = np.random.RandomState(seed)
    gt = rs.uniform(0, 1, size=(nv, h, w, 3)).astype(np.float32)
    sig = np.asarray(sigma, np.float32).reshape(-1, 1, 1, 1)
    return (gt + sig * rs.standard_normal(gt.shape).astype(np.float32)).astype(np.float32), gt


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_against_restatement(res, rgb, gt01, what=""):
    """Prints each figure before it asserts."""
    m_ref, p_ref, s_ref = mr.view_metrics(rgb, gt01)
    psnr, ssim = res.psnr.cpu().numpy(), res.ssim.cpu().numpy()
    assert psnr.dtype == np.float64 and ssim.dtype == np.float64 and psnr.shape == ssim.shape == (rgb.shape[0],)
    m_got = 10.0 ** (-psnr / 10.0)
    e_s, e_m, e_p = np.abs(ssim - s_ref).max(), (np.abs(m_got - m_ref) / m_ref).max(), np.abs(psnr - p_ref).max()
    print("%s %s: ssim err %.3g, mse rel err %.3g, psnr err %.3g dB" % (what, rgb.shape, e_s, e_m, e_p))
    assert e_s < SSIM_TOL and e_m < MSE_RTOL and e_p < PSNR_TOL
    if res.rgb8 is not None:
        assert res.rgb8.dtype == torch.uint8 and np.array_equal(res.rgb8.cpu().numpy(), mr.to_bytes(rgb))


@pytest.mark.parametrize("h,w", SWEEP)
def test_shape_sweep_against_the_restatement(h, w):
    assert h != w
    rgb, gt = make_pair(100 + h * 97 + w, 3, h, w)
    assert rgb.min() < 0 and rgb.max() > 1                    # the clamp is exercised
    res = pmetrics.compare_views(on_dev(rgb), on_dev(gt))
    check_against_restatement(res, rgb, gt, "sweep")
    flat = pmetrics.compare_views(on_dev(rgb).reshape(-1, 3), on_dev(gt), H=h, W=w)      # (NV * H * W, 3) with H, W given
    assert torch.equal(flat.psnr, res.psnr) and torch.equal(flat.ssim, res.ssim) and torch.equal(flat.rgb8, res.rgb8)


def test_both_ground_truth_layouts_give_identical_bits():
    nv, h, w = 3, 23, 39
    rs = np.random.RandomState(7)
    images = rs.uniform(-1, 1, size=(nv, 3, h, w)).astype(np.float32)              # the dataset's form
    gt01 = mr.gt_from_pm1(images)
    rgb = (gt01 + np.float32(0.05) * rs.standard_normal(gt01.shape).astype(np.float32)).astype(np.float32)
    a = pmetrics.compare_views(on_dev(rgb), on_dev(gt01), gt_layout="nhwc01")
    b = pmetrics.compare_views(on_dev(rgb), on_dev(images), gt_layout="nchw_pm1")
    assert torch.equal(a.psnr, b.psnr) and torch.equal(a.ssim, b.ssim) and torch.equal(a.rgb8, b.rgb8)
    check_against_restatement(b, rgb, gt01, "nchw_pm1")


def test_closed_forms():
    h, w = 9, 8
    x = np.random.RandomState(8).uniform(0, 1, size=(1, h, w, 3)).astype(np.float32)
    black, white, quarter = np.zeros_like(x), np.ones_like(x), np.full_like(x, 0.25)
    rgb, gt = np.concatenate([x, black, quarter]), np.concatenate([x, white, white])
    res = pmetrics.compare_views(on_dev(rgb), on_dev(gt))
    psnr, ssim = res.psnr.cpu().numpy(), res.ssim.cpu().numpy()
    print("closed forms: psnr %s ssim %s" % (psnr, ssim))
    assert abs(ssim[0] - 1.0) < 1e-12 and psnr[0] == np.inf                 # identical images
    assert abs(ssim[1] - 1e-4 / 1.0001) < 1e-12 and abs(psnr[1]) < 1e-12    # black against white: mse = 1
    assert abs(ssim[2] - (0.5 + 1e-4) / 1.0626) < 1e-12                     # constant 0.25 against constant 1
    assert abs(10.0 ** (-psnr[2] / 10.0) - 0.5625) < 1e-12
    assert np.array_equal(res.rgb8.cpu().numpy(), mr.to_bytes(rgb))


def test_low_contrast_and_bright_pairs():
    """Where fp32 sums fail: the covariance (about 1e-6) cancels against squared means of about 1 beside C2 = 9e-4."""
    h, w = 23, 22
    rs = np.random.RandomState(9)
    mk = lambda centre: (centre + rs.uniform(-1e-3, 1e-3, size=(1, h, w, 3))).astype(np.float32)   # noqa: E731
    rgb, gt = np.concatenate([mk(0.5), mk(0.98)]), np.concatenate([mk(0.5), mk(0.98)])
    check_against_restatement(pmetrics.compare_views(on_dev(rgb), on_dev(gt)), rgb, gt, "low contrast")


def test_many_small_views_keep_their_rows():
    nv = 67
    rgb, gt = make_pair(10, nv, 7, 7, sigma=0.01 * (1 + np.arange(nv)))
    res = pmetrics.compare_views(on_dev(rgb), on_dev(gt))
    check_against_restatement(res, rgb, gt, "67 views")
    assert len(set(res.psnr.cpu().tolist())) == nv           # every view has a value of its own


def test_bits_are_the_same_from_run_to_run():
    rgb, gt = (on_dev(a) for a in make_pair(11, 5, 39, 71))
    a = pmetrics.compare_views(rgb, gt)
    b = pmetrics.compare_views(rgb, gt)
    other = [on_dev(v) for v in make_pair(12, 9, 8, 23)]       # another shape through the same workspace
    pmetrics.compare_views(*other)
    putil.psnr(other[0], other[1])
    c = pmetrics.compare_views(rgb, gt)
    for r in (b, c):
        assert torch.equal(a.psnr, r.psnr) and torch.equal(a.ssim, r.ssim) and torch.equal(a.rgb8, r.rgb8)


def test_either_output_alone_equals_the_combined_call():
    rgb, gt = (on_dev(a) for a in make_pair(13, 3, 23, 39))
    both = pmetrics.compare_views(rgb, gt)
    only_m = pmetrics.compare_views(rgb, gt, want_uint8=False)
    only_b = pmetrics.compare_views(rgb, gt, want_metrics=False)
    assert only_m.rgb8 is None and torch.equal(only_m.psnr, both.psnr) and torch.equal(only_m.ssim, both.ssim)
    assert only_b.psnr is None and only_b.ssim is None and torch.equal(only_b.rgb8, both.rgb8)


def test_a_nan_pixel_reaches_its_own_view_only():
    rgb, gt = make_pair(14, 3, 23, 39)
    clean = pmetrics.compare_views(on_dev(rgb), on_dev(gt))
    bad = rgb.copy()
    bad[1, 17, 33, 2] = np.nan              # in the second tile of both axes
    res = pmetrics.compare_views(on_dev(bad), on_dev(gt))
    assert bool(torch.isnan(res.psnr[1])) and bool(torch.isnan(res.ssim[1]))
    for v in (0, 2):
        assert torch.equal(res.psnr[v], clean.psnr[v]) and torch.equal(res.ssim[v], clean.ssim[v])
    assert int(res.rgb8[1, 17, 33, 2]) == 0
    keep = torch.ones_like(res.rgb8, dtype=torch.bool)
    keep[1, 17, 33, 2] = False
    assert torch.equal(res.rgb8[keep], clean.rgb8[keep])


def test_psnr_as_vis_step_uses_it():
    rs = np.random.RandomState(15)
    for shape in ((128, 3), (5000, 3), (7,)):          # (5000, 3) takes more than one workgroup
        p, t = rs.uniform(-0.2, 1.2, size=shape).astype(np.float32), rs.uniform(0, 1, size=shape).astype(np.float32)
        got = putil.psnr(on_dev(p), on_dev(t))
        assert got.dim() == 0 and got.dtype == torch.float64 and got.device.type == "cuda"
        ref = -10.0 * np.log10(np.mean((p.astype(np.float64) - t.astype(np.float64)) ** 2))
        print("psnr %s: %.15g against %.15g" % (shape, float(got), ref))
        assert abs(float(got) - ref) < PSNR_TOL
    assert float(pmetrics.psnr(on_dev(p), on_dev(p))) == np.inf


def test_end_to_end_encode_render_score(golden):
    """The enc_render golden's scene: its images through the HIP trunk, two 32 x 32 target views rendered, scored against a
    ground truth in the dataset's form; the restatement runs on the same rendered tensor copied to the host."""
    g = golden("enc_render")
    seed, ns, H, W = int(g["seed"]), int(g["NS"]), int(g["H"]), int(g["W"])
    net = make_model(pconf.default_mv()["model"]).eval()
    load_mlp(net.mlp_coarse, seed * 10 + 1, 512, 4)
    load_mlp(net.mlp_fine, seed * 10 + 2, 512, 4)
    esd = synth.resnet34_state(seed * 10 + 4, residual_gain=float(g["residual_gain"]))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in esd.items()}, strict=False)
    net = net.to(DEV)
    net.encode(torch.from_numpy(synth.images(seed * 10 + 5, ns, H, W))[None], torch.from_numpy(g["src_poses"])[None],
               torch.tensor(float(g["focal"])), c=torch.from_numpy(g["c"])[None])
    nv, h, w = 2, 32, 32
    poses = torch.from_numpy(np.stack([synth.pose_spherical(th, -20.0, 1.3) for th in (120.0, 100.0)]).astype(np.float32))
    rays = putil.gen_rays(poses.to(DEV), w, h, torch.tensor(float(g["focal"]) * w / W), 0.8, 1.8,
                          c=torch.from_numpy(g["c"]).reshape(-1)[:2] * w / W)
    ren = NeRFRenderer(n_coarse=16, n_fine=8, n_fine_depth=4, depth_std=0.01, white_bkgd=True).eval()
    with torch.no_grad():
        rgb = ren(net, rays.reshape(1, -1, 8))["fine"]["rgb"][0]
    assert tuple(rgb.shape) == (nv * h * w, 3)
    images = synth.images(seed * 10 + 6, nv, h, w)
    res = pmetrics.compare_views(rgb, on_dev(images), gt_layout="nchw_pm1", H=h, W=w)
    host = rgb.cpu().numpy().reshape(nv, h, w, 3)
    assert np.isfinite(host).all() and float(host.std()) > 1e-3
    check_against_restatement(res, host, mr.gt_from_pm1(images), "end to end")
