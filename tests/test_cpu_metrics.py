"""
The view metrics without a GPU (include/pnyolo.h pny_view_metrics, metrics.compare_views / metrics.psnr):

  * the restatement the GPU tests compare against (tests/metrics_ref.py, skimage's SSIM written out on scipy's
    uniform_filter) against closed forms: identical images, black against white, constant against constant, the single
    window of a 7 x 7 image computed directly, and the boundary modes `reflect` and `constant` (the 3-pixel crop keeps the
    boundary out of the result);
  * the kernel's own arithmetic (csrc/pny_metrics.h compiled by g++, the way tests/test_cpu_train_batch.py compiles its
    header): S of a window from direct fp64 sums within 1e-9 of the restatement on random, low-contrast (0.5 +- 1e-3) and
    bright (0.98 +- 1e-3) pairs -- fp32 sums miss by 1e-6 to 4e-5 there, a different fp64 summation order by about 1e-12 --
    and the byte conversion bit-equal to numpy's on every k / 255, both fp32 neighbours of each, the clamp's cases and
    10 000 uniform draws;
  * the C ABI: bad arguments refused before any launch (the boundary itself: tests/test_cpu_abi.py);
  * the Python entry points refuse CPU tensors, fp64 tensors, mismatched shapes, H < 7 and an unknown layout by name.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as mr
from host_tools import CSRC, built_lib, header_code, header_text, host_header_program  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import metrics as pmetrics
from pixel_nerf_yolo_amd import util as putil


# --------------------------------------------------------------------------- the restatement against closed forms
def test_restatement_identical_images_give_exactly_one():
    x = np.random.RandomState(0).uniform(0, 1, size=(19, 23, 3))
    assert mr.ssim(x, x.copy()) == 1.0
    assert mr.psnr_of_mse(mr.mse(x, x)) == np.inf


def test_restatement_black_against_white():
    x, y = np.zeros((9, 8, 3)), np.ones((9, 8, 3))
    assert abs(mr.ssim(x, y) - 1e-4 / 1.0001) < 1e-15
    assert mr.psnr_of_mse(mr.mse(x, y)) == 0.0


def test_restatement_constant_against_constant():
    x, y = np.full((11, 9, 3), 0.25), np.ones((11, 9, 3))
    for ch in range(3):
        assert abs(mr.ssim_channel(x[..., ch], y[..., ch]) - (0.5 + 1e-4) / 1.0626) < 1e-14
    assert abs(mr.mse(x, y) - 0.5625) < 1e-16


def test_restatement_single_window_equals_direct_sums():
    rs = np.random.RandomState(1)
    for _ in range(20):
        x, y = rs.uniform(0, 1, size=(7, 7)), rs.uniform(0, 1, size=(7, 7))
        assert abs(mr.ssim_channel(x, y) - mr.window_s(x, y)) < 1e-13
    # every window of a larger image, too: the filtered map at (i + 3, j + 3) is the window whose corner is (i, j)
    x, y = rs.uniform(0, 1, size=(10, 12)), rs.uniform(0, 1, size=(10, 12))
    direct = np.mean([mr.window_s(x[i:i + 7, j:j + 7], y[i:i + 7, j:j + 7]) for i in range(4) for j in range(6)])
    assert abs(mr.ssim_channel(x, y) - direct) < 1e-13


def test_restatement_boundary_mode_never_reaches_the_result():
    rs = np.random.RandomState(2)
    x, y = rs.uniform(0, 1, size=(17, 13, 3)), rs.uniform(0, 1, size=(17, 13, 3))
    assert abs(mr.ssim(x, y, "reflect") - mr.ssim(x, y, "constant")) < 1e-14


# --------------------------------------------------------------------------- the kernel's header on the host
HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pny_metrics.h"
// one query per input line:  W x0 .. x48 y0 .. y48 (fp32 pixels of one window; direct fp64 sums) | B v (clamp, byte) |
//                            G g (ground truth from [-1, 1]) | P sse n
int main(int argc, char** argv) {
    printf("tile %d %d %d\n", pny::METRICS_TILE_H, pny::METRICS_TILE_W, pny::METRICS_WIN);
    FILE* f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) return 2;
    static char line[8192];
    static char* a[128];
    while (fgets(line, sizeof line, f)) {
        char* t = strtok(line, " \n");
        char kind = t[0];
        int n = 0;
        while ((t = strtok(0, " \n")) && n < 128) a[n++] = t;
        if (kind == 'W') {
            if (n != 98) return 4;
            double m[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < 49; ++i) {
                const double x = (double)strtof(a[i], 0), y = (double)strtof(a[49 + i], 0);
                m[0] += x, m[1] += y, m[2] += x * x, m[3] += y * y, m[4] += x * y;
            }
            printf("%a\n", pny::metrics_ssim_window(m[0], m[1], m[2], m[3], m[4]));
        } else if (kind == 'B') {
            const float x = pny::metrics_clamp01(strtof(a[0], 0));
            printf("%a %d\n", (double)x, (int)pny::metrics_byte(x));
        } else if (kind == 'G') {
            printf("%a\n", (double)pny::metrics_gt_from_pm1(strtof(a[0], 0)));
        } else if (kind == 'P') {
            printf("%a\n", pny::metrics_psnr(strtod(a[0], 0), strtod(a[1], 0)));
        } else {
            return 3;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    """csrc/pny_metrics.h compiled by g++: __device__ defined away, no fused multiply-add -- the product's own code, run on
    lines of queries."""
    program = host_header_program(tmp_path_factory.mktemp("metrics_host"), HOST_MAIN, include_dirs=(CSRC,))

    def run(queries):
        lines = program(queries)
        assert lines[0].startswith("tile ") and lines[0].split()[3] == "7" and len(lines) == 1 + len(queries)
        return lines[1:]
    return run


def hexes(v):
    return " ".join(float(x).hex() for x in np.asarray(v, np.float32).reshape(-1))


def window_pairs():
    rs = np.random.RandomState(3)
    pairs = [(rs.uniform(0, 1, size=(7, 7)), rs.uniform(0, 1, size=(7, 7))) for _ in range(40)]
    for centre in (0.5, 0.98):      # low contrast: the covariance is ~1e-6 beside C2 = 9e-4 and the means' squares ~1
        for _ in range(40):
            pairs.append((centre + rs.uniform(-1e-3, 1e-3, size=(7, 7)), centre + rs.uniform(-1e-3, 1e-3, size=(7, 7))))
    return [(x.astype(np.float32), y.astype(np.float32)) for x, y in pairs]


def test_header_window_s_against_the_restatement(host_header):
    pairs = window_pairs()
    got = [float.fromhex(v) for v in host_header(["W %s %s" % (hexes(x), hexes(y)) for x, y in pairs])]
    worst = 0.0
    for (x, y), s in zip(pairs, got):
        ref = mr.ssim_channel(x.astype(np.float64), y.astype(np.float64))      # the restatement: uniform_filter, cropped to 1 x 1
        worst = max(worst, abs(s - ref))
        assert abs(s - ref) < 1e-9, (s, ref)
        assert abs(s - mr.window_s(x, y)) < 1e-9
    print("worst |S - restatement| over %d windows: %.3g" % (len(pairs), worst))


def test_fp32_sums_would_miss_the_bar():
    """Why the bar is where it is: the same windows with the five sums taken in fp32 are off by more than 1e-9."""
    worst = 0.0
    for x, y in window_pairs()[40:]:
        s32 = [np.float32(0)] * 5
        for a, b in zip(x.reshape(-1), y.reshape(-1)):
            for i, term in enumerate((a, b, a * a, b * b, a * b)):
                s32[i] = np.float32(s32[i] + term)
        ux, uy = float(s32[0]) / 49, float(s32[1]) / 49
        vx, vy, vxy = (49 / 48 * (float(v) / 49 - m) for v, m in ((s32[2], ux * ux), (s32[3], uy * uy), (s32[4], ux * uy)))
        s = ((2 * ux * uy + mr.C1) * (2 * vxy + mr.C2)) / ((ux * ux + uy * uy + mr.C1) * (vx + vy + mr.C2))
        worst = max(worst, abs(s - mr.window_s(x, y)))
    assert worst > 1e-7


def byte_inputs():
    k = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    vals = [k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)), np.array([0, 1, -0.25, 1.5, -0.0], np.float32),
            np.random.RandomState(4).uniform(0, 1, size=10000).astype(np.float32),
            np.random.RandomState(5).uniform(-0.5, 1.5, size=1000).astype(np.float32)]
    return np.concatenate(vals)


def test_header_bytes_are_numpys(host_header):
    v = byte_inputs()
    got = [line.split() for line in host_header(["B %s" % float(x).hex() for x in v])]
    clamped = np.array([float.fromhex(g[0]) for g in got], np.float32)
    bytes_ = np.array([int(g[1]) for g in got], np.uint8)
    assert np.array_equal(clamped, mr.clamp(v))
    assert np.array_equal(bytes_, (np.clip(v, 0, 1) * np.float32(255)).astype(np.uint8))
    assert np.array_equal(bytes_, mr.to_bytes(v))
    assert bytes_[255] == 255 and bytes_[0] == 0 and len(set(bytes_[:256].tolist())) > 250
    # truncation, not rounding: some fl32(k / 255) * 255 fall just below k
    assert bool((bytes_[:256] != np.arange(256)).any()) or bool((bytes_[512:768] != np.arange(256)).any())


def test_header_nan_prediction_stays_nan_and_writes_zero(host_header):
    (clamped, byte), = [line.split() for line in host_header(["B nan"])]
    assert np.isnan(float.fromhex(clamped))
    assert int(byte) == 0


def test_header_ground_truth_and_psnr(host_header):
    g = np.random.RandomState(6).uniform(-1, 1, size=500).astype(np.float32)
    got = np.array([float.fromhex(v) for v in host_header(["G %s" % float(x).hex() for x in g])], np.float32)
    assert np.array_equal(got, g * np.float32(0.5) + np.float32(0.5))
    lines = host_header(["P %s %s" % (float(3.7).hex(), float(147).hex()), "P 0x0p+0 0x1p+4"])
    assert abs(float.fromhex(lines[0]) - mr.psnr_of_mse(3.7 / 147)) < 1e-12
    assert lines[1].strip() == "inf"


# --------------------------------------------------------------------------- C ABI
def test_entry_is_declared_bound_and_exported():
    """What is this entry's own (declared, bound, exported, its layout and constants: tests/test_cpu_abi.py)."""
    hdr = header_text()
    assert re.search(r"\bint\s+pny_view_metrics\s*\(\s*const\s+pny_view_metrics_desc\s*\*", header_code())
    # the comment of the entry names the reference lines it replaces, as every other entry does
    block = hdr[hdr.index("---- view metrics"):hdr.index("int pny_view_metrics")]
    assert "eval.py:288-345" in block and "calc_metrics.py:189-191" in block and "util.py:502" in block
    # the header's tile extents are the ones the GPU tests are built around
    h = open(os.path.join(CSRC, "pny_metrics.h")).read()
    assert re.search(r"METRICS_TILE_H\s*=\s*16\b", h) and re.search(r"METRICS_TILE_W\s*=\s*32\b", h)


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    """PNY_ERR_ARG (-1) with a message, whether or not a GPU is there (the pointers are never dereferenced by the host)."""
    call = built_lib.pny_view_metrics
    ok = dict(n_views=2, height=9, width=8, gt_layout=0, win_size=7)
    p = C.c_void_p(4096)

    def rc(rgb=p, gt=p, out=p, rgb8=p, **over):
        d = plib.ViewMetricsDesc(**dict(ok, **over))
        return call(C.byref(d), rgb, gt, out, rgb8, None)

    assert call(None, p, p, p, p, None) == -1
    assert rc(rgb=None) == -1 and b"null" in built_lib.pny_last_error()
    assert rc(gt=None) == -1 and b"null" in built_lib.pny_last_error()
    assert rc(out=None, rgb8=None) == -1 and b"both outputs" in built_lib.pny_last_error()
    for bad in (dict(n_views=0), dict(height=0), dict(width=-3)):
        assert rc(**bad) == -1 and b"positive" in built_lib.pny_last_error(), bad
    for bad in (dict(height=6), dict(width=6)):
        assert rc(**bad) == -1 and b"win_size" in built_lib.pny_last_error(), bad
    for bad in (dict(win_size=0), dict(win_size=11), dict(win_size=3)):
        assert rc(**bad) == -1 and b"win_size must be 7" in built_lib.pny_last_error(), bad
    assert rc(gt_layout=3) == -1 and rc(gt_layout=-1) == -1 and b"gt_layout" in built_lib.pny_last_error()
    assert rc(n_views=2 ** 15, height=2 ** 8, width=2 ** 8) == -1 and b"2^31" in built_lib.pny_last_error()     # 3 * 2^31
    assert rc(gt_layout=2) == -1 and b"8-bit" in built_lib.pny_last_error()                     # the flat form has no rgb8


# --------------------------------------------------------------------------- the Python entry points
def test_python_refuses_by_name():
    x = torch.zeros(2, 9, 8, 3)
    with pytest.raises(plib.PnyError, match="rgb is on cpu.*no CPU path"):
        pmetrics.compare_views(x, x)
    with pytest.raises(plib.PnyError, match="pred is on cpu.*no CPU path"):
        pmetrics.psnr(torch.zeros(128, 3), torch.zeros(128, 3))
    assert putil.psnr is pmetrics.psnr
    with pytest.raises(plib.PnyError, match="rgb must be fp32, got torch.float64"):
        pmetrics.compare_views(x.double(), x)
    with pytest.raises(plib.PnyError, match="gt must be fp32, got torch.float64"):
        pmetrics.compare_views(x, x.double())
    with pytest.raises(plib.PnyError, match="target must be fp32"):
        pmetrics.psnr(torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="rgb must be a tensor"):
        pmetrics.compare_views(x.numpy(), x)
    with pytest.raises(ValueError, match=r"gt has shape \(2, 9, 8, 3\).*needs \(2, 3, 9, 8\)"):
        pmetrics.compare_views(x, x, gt_layout="nchw_pm1")
    with pytest.raises(ValueError, match=r"gt has shape \(2, 8, 9, 3\)"):
        pmetrics.compare_views(x, torch.zeros(2, 8, 9, 3))
    with pytest.raises(ValueError, match="no broadcasting"):
        pmetrics.psnr(torch.zeros(4, 3), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="at least the SSIM window, 7; got 6 x 8"):
        pmetrics.compare_views(torch.zeros(1, 6, 8, 3), torch.zeros(1, 6, 8, 3))
    with pytest.raises(ValueError, match="gt_layout must be one of .*got 'nchw01'"):
        pmetrics.compare_views(x, x, gt_layout="nchw01")
    with pytest.raises(ValueError, match=r"not \(NV \* 9 \* 8, 3\)"):
        pmetrics.compare_views(torch.zeros(100, 3), x, H=9, W=8)
    with pytest.raises(ValueError, match=r"rgb must be \(NV, H, W, 3\)"):
        pmetrics.compare_views(torch.zeros(144, 3), x)
