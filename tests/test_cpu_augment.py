"""
The colour jitter without a GPU (include/pnyolo.h pny_color_jitter, augment.color_jitter, data.ColorJitterDataset(defer=True)):

  * the restatement the GPU tests compare against (tests/augment_ref.py, float64) against closed forms: a third of a turn maps
    red -> green -> blue, half a turn twice is the identity, saturation 0 gives the grey image, contrast 0 the constant mean,
    brightness 3 clamps at 1, and the factors (0, 1, 1, 1) are the identity within 4 * 2^-53;
  * the restatement against the project's host chain (data.adjust_* in torch fp32) on 6 random 37 x 53 images and 4 factor
    sets;
  * the kernel's own arithmetic (csrc/pny_augment.h compiled by g++, the way tests/test_cpu_metrics.py compiles its header):
    the per-pixel functions and the whole chain on 10 000 random pixels and edge pixels, within the bar;
  * the C ABI: every listed refusal before any launch (the boundary itself: tests/test_cpu_abi.py);
  * Python: refusals by name; the deferred dataset returns untouched images and exactly the factors the host path draws;
    get_split_dataset(jitter_on_device=True) wires it for `dvr_dtu` and `yolo`.

The bar (tests/augment_ref.py `bar`), in output units [-1, 1]: max(4 e_host, 64 * 2^-24), e_host being the worst difference of
the host fp32 chain from the restatement on the test's own inputs.  The factor 4 allows for a second fp32 implementation with
another operation order and an fp64 mean; the floor is 32 rounded fp32 operations on values in [0, 1], doubled by the output
map.  The chain is continuous across each of its branches, so no pixel is left out.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import augment_ref as ar
from host_tools import CSRC, built_lib, header_code, header_text, host_header_program  # noqa: F401
from pixel_nerf_yolo_amd import augment as paug
from pixel_nerf_yolo_amd import data as pdata
from pixel_nerf_yolo_amd import lib as plib

# (hue, saturation, brightness, contrast): the identity, the extremes, two corners of the reference's ranges
FACTOR_SETS = np.array([(0, 1, 1, 1), (0.5, 0, 3, 0), (-0.5, 2, 0.5, 2), (0.1, 0.9, 1.1, 0.9), (-0.1, 1.1, 0.9, 1.1)], np.float32)


def random_images(seed, nv, h, w):
    return np.random.RandomState(seed).uniform(-1, 1, size=(nv, 3, h, w)).astype(np.float32)


# --------------------------------------------------------------------------- the restatement against closed forms
def test_restatement_third_of_a_turn_permutes_the_primaries():
    red, green, blue = np.eye(3)
    assert np.abs(ar.hue(red, 1 / 3) - green).max() < 1e-12
    assert np.abs(ar.hue(ar.hue(red, 1 / 3), 1 / 3) - blue).max() < 1e-12
    assert np.abs(ar.hue(blue, 1 / 3) - red).max() < 1e-12
    assert np.abs(ar.hue(red, -1 / 3) - blue).max() < 1e-12


def test_restatement_half_a_turn_twice_is_the_identity():
    px = np.array([[1.0, 0.25, 0.0], [0.0, 1.0, 0.7], [0.3, 0.0, 1.0], [0.9, 0.8, 0.1]])      # saturated: one channel at 0
    for shift in (0.5, -0.5):
        assert np.abs(ar.hue(ar.hue(px, shift), shift) - px).max() < 1e-12
    assert np.abs(ar.hue(px, 0.5) - px).max() > 0.5


def test_restatement_saturation_zero_gives_the_grey_image():
    x = random_images(1, 2, 5, 7)
    out = ar.jitter(x, (0.0, 0.0, 1.0, 1.0))
    t = (x.astype(np.float64) + 1) / 2
    grey = 0.2989 * t[:, 0] + 0.587 * t[:, 1] + 0.114 * t[:, 2]
    assert np.abs(out - (2 * grey - 1)[:, None]).max() < 1e-15


def test_restatement_contrast_zero_gives_the_constant_mean():
    x = random_images(2, 3, 5, 7)
    out = ar.jitter(x, (0.0, 1.0, 1.0, 0.0))
    t = (x.astype(np.float64) + 1) / 2
    mean = (0.2989 * t[:, 0] + 0.587 * t[:, 1] + 0.114 * t[:, 2]).mean(axis=(1, 2))
    assert np.abs(out - (2 * mean - 1)[:, None, None, None]).max() < 1e-14
    assert len(set(np.round(mean, 12))) == 3                    # a mean per image, not one for all


def test_restatement_brightness_three_clamps_at_one():
    x = random_images(3, 1, 9, 8)
    out = ar.jitter(x, (0.0, 1.0, 3.0, 1.0))
    t = (x.astype(np.float64) + 1) / 2
    assert out.max() == 1.0 and bool((out[t > 1 / 3 + 1e-9] == 1.0).all())
    assert np.abs(out - (2 * np.minimum(3 * t, 1) - 1)).max() < 1e-14


def test_restatement_identity_factors_return_the_image():
    """(0, 1, 1, 1): the input map of an fp32 value, both blends with ratio 1 and the output map are exact in fp64, value and
    chroma pass through the hue step unchanged, and a channel v - c f carries the rounding of d, of d + 1 and of the product
    and the difference: at most 2 units of 2^-53 in [0, 1], 4 in output units."""
    x = random_images(4, 6, 37, 53)
    err = np.abs(ar.jitter(x, (0.0, 1.0, 1.0, 1.0)) - x).max()
    print("identity: worst error %.3g = %.2f * 2^-53" % (err, err / 2.0 ** -53))
    assert err <= 4 * 2.0 ** -53


# --------------------------------------------------------------------------- the restatement against data.adjust_*
def test_restatement_against_the_host_chain():
    x = random_images(5, 6, 37, 53)
    for f in FACTOR_SETS[[0, 2, 3, 4]]:
        ref = ar.jitter(x, f)
        _, e_host = ar.bar(x, f, ref)
        print("factors %s: host chain against the restatement %.3g (output units)" % (f.tolist(), e_host))
        # two implementations of the same real function, one in fp32: the floor of the bar alone
        assert e_host < ar.FLOOR
    u8 = np.random.RandomState(6).randint(0, 256, size=(2, 37, 53, 3)).astype(np.uint8)
    _, e_host = ar.bar(u8, FACTOR_SETS[3])
    print("bytes: host chain against the restatement %.3g" % e_host)
    assert e_host < ar.FLOOR


# --------------------------------------------------------------------------- the kernel's header on the host
HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pny_augment.h"
// one query per input line:
//   M x            float input map            -> t
//   Y b            byte input map             -> t
//   F hue sat r g b   saturation + hue of a pixel in [0, 1]   -> r g b grey
//   S t mean con bri  contrast, brightness, output map        -> out
//   P r g b        a pixel of the pending image, float format, in [-1, 1]   -> (nothing)
//   Q r g b        a pixel of the pending image, byte format                -> (nothing)
//   C hue sat bri con   the chain over the pending image as the kernel runs it: pass 1 with an fp64 sum in pixel order, the
//                       mean rounded to fp32, pass 2 -> one line `r g b` per pixel; the image is then dropped
int main(int argc, char** argv) {
    printf("jitter %d %d\n", pny::JITTER_THREADS, pny::JITTER_MAX_OBJS);
    FILE* f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) return 2;
    static char line[512];
    char* a[8];
    std::vector<float> img;
    while (fgets(line, sizeof line, f)) {
        char* t = strtok(line, " \n");
        const char kind = t[0];
        int n = 0;
        while ((t = strtok(0, " \n")) && n < 8) a[n++] = t;
        if (kind == 'M') {
            printf("%a\n", (double)pny::jitter_from_pm1(strtof(a[0], 0)));
        } else if (kind == 'Y') {
            printf("%a\n", (double)pny::jitter_from_byte((uint8_t)atoi(a[0])));
        } else if (kind == 'F') {
            float r = strtof(a[2], 0), g = strtof(a[3], 0), b = strtof(a[4], 0);
            const float y = pny::jitter_first(r, g, b, strtof(a[0], 0), strtof(a[1], 0));
            printf("%a %a %a %a\n", (double)r, (double)g, (double)b, (double)y);
        } else if (kind == 'S') {
            printf("%a\n", (double)pny::jitter_second(strtof(a[0], 0), strtof(a[1], 0), strtof(a[2], 0), strtof(a[3], 0)));
        } else if (kind == 'P') {
            for (int i = 0; i < 3; ++i) img.push_back(pny::jitter_from_pm1(strtof(a[i], 0)));
        } else if (kind == 'Q') {
            for (int i = 0; i < 3; ++i) img.push_back(pny::jitter_from_byte((uint8_t)atoi(a[i])));
        } else if (kind == 'C') {
            const float hue = strtof(a[0], 0), sat = strtof(a[1], 0), bri = strtof(a[2], 0), con = strtof(a[3], 0);
            const int n_px = (int)(img.size() / 3);
            double sum = 0.0;
            for (int i = 0; i < n_px; ++i) {
                float r = img[3 * i], g = img[3 * i + 1], b = img[3 * i + 2];
                sum += (double)pny::jitter_first(r, g, b, hue, sat);
            }
            const float mean = pny::jitter_mean(sum, n_px);
            for (int i = 0; i < n_px; ++i) {
                float r = img[3 * i], g = img[3 * i + 1], b = img[3 * i + 2];
                pny::jitter_first(r, g, b, hue, sat);
                printf("%a %a %a\n", (double)pny::jitter_second(r, mean, con, bri), (double)pny::jitter_second(g, mean, con, bri),
                       (double)pny::jitter_second(b, mean, con, bri));
            }
            img.clear();
        } else {
            return 3;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    """csrc/pny_augment.h compiled by g++: __device__ defined away, no fused multiply-add -- the product's own code, run on lines
    of queries."""
    program = host_header_program(tmp_path_factory.mktemp("augment_host"), HOST_MAIN, include_dirs=(CSRC,))

    def run(queries):
        lines = program(queries)
        assert lines[0] == "jitter 1024 64"
        return [[float.fromhex(v) for v in line.split()] for line in lines[1:]]
    return run


def hx(*vals):
    return " ".join(float(np.float32(v)).hex() for v in vals)


def edge_pixels():
    """(n, 3) fp32 in [0, 1]: black, white, greys, the six primaries and secondaries, pixels with two equal channels (the equal
    pair above and below the third), channels one ulp apart."""
    px = [(0, 0, 0), (1, 1, 1)] + [(g, g, g) for g in (0.25, 0.5, 1 / 3, 0.999)]
    px += [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]
    for lo, hi in ((0.2, 0.7), (0.0, 1.0), (0.4, 0.4000001)):
        px += [(hi, hi, lo), (hi, lo, hi), (lo, hi, hi), (lo, lo, hi), (lo, hi, lo), (hi, lo, lo)]
    for x in (0.5, 0.1, 1.0):
        x = np.float32(x)
        dn = np.nextafter(x, np.float32(0))
        px += [(x, dn, dn), (dn, x, dn), (dn, dn, x), (x, x, dn), (x, dn, x), (dn, x, x), (x, dn, np.nextafter(dn, np.float32(0)))]
    return np.array(px, np.float32)


def header_pixels():
    return np.concatenate([np.random.RandomState(7).uniform(0, 1, size=(10000, 3)).astype(np.float32), edge_pixels()])


def host_first(px, hue_f, sat):
    """data.adjust_hue(data.adjust_saturation(.)) in torch fp32 on (n, 3) pixels in [0, 1]."""
    t = torch.from_numpy(np.ascontiguousarray(px.T)).reshape(3, 1, -1)
    return pdata.adjust_hue(pdata.adjust_saturation(t, float(sat)), float(hue_f)).reshape(3, -1).T.numpy()


def test_header_input_maps(host_header):
    x = np.concatenate([np.float32([-1, 1, 0, -0.0]), np.random.RandomState(8).uniform(-1, 1, size=500).astype(np.float32)])
    got = np.array(host_header(["M " + hx(v) for v in x]))[:, 0]
    assert np.array_equal(got.astype(np.float32), (x + np.float32(1)) * np.float32(0.5)) and got[0] == 0.0 and got[1] == 1.0
    got = np.array(host_header(["Y %d" % b for b in range(256)]))[:, 0]
    assert np.array_equal(got.astype(np.float32), np.arange(256, dtype=np.float32) / np.float32(255)) and got[255] == 1.0


def test_header_pixel_functions_against_the_restatement(host_header):
    px = header_pixels()
    for hue_f, sat in FACTOR_SETS[:, :2]:
        got = np.array(host_header(["F %s %s" % (hx(hue_f, sat), hx(*p)) for p in px]))
        ref = ar.first(px.astype(np.float64), float(hue_f), float(sat))
        e_host = 2 * np.abs(host_first(px, hue_f, sat).astype(np.float64) - ref).max()
        bar = max(4 * e_host, ar.FLOOR)
        err = 2 * np.abs(got[:, :3] - ref).max()                 # [0, 1] values: doubled into output units
        err_grey = 2 * np.abs(got[:, 3] - ar.grey(ref)).max()
        print("first(hue %g, sat %g): header %.3g, grey %.3g, host %.3g, bar %.3g" % (hue_f, sat, err, err_grey, e_host, bar))
        assert err <= bar and err_grey <= bar
        assert got[:, :3].min() >= 0.0 and got[:, :3].max() <= 1.0
    rs = np.random.RandomState(9)
    q = np.concatenate([rs.uniform(0, 1, size=(2000, 2)), rs.uniform(0, 3, size=(2000, 2))], axis=1).astype(np.float32)
    q = np.concatenate([q, np.float32([(0, 0.5, 0, 3), (1, 0.5, 2, 0.5), (1, 0, 1, 3), (0.3, 0.7, 1, 1)])])
    got = np.array(host_header(["S " + hx(*row) for row in q]))[:, 0]
    ref = ar.second(q[:, 0].astype(np.float64), q[:, 1].astype(np.float64), q[:, 2].astype(np.float64), q[:, 3].astype(np.float64))
    print("second: header against the restatement %.3g" % np.abs(got - ref).max())
    assert np.abs(got - ref).max() <= ar.FLOOR and got.min() >= -1.0 and got.max() <= 1.0


@pytest.mark.parametrize("fmt", ["float", "bytes"])
def test_header_chain_against_the_restatement(host_header, fmt):
    """The pixels as ONE image of 1 x n, through the header's two passes as the kernel runs them."""
    px = header_pixels()
    if fmt == "float":
        img = (px * np.float32(2) - np.float32(1)).T.reshape(1, 3, 1, -1).copy()           # (NV = 1, 3, 1, n) in [-1, 1]
        img[0, :, 0, :4] = np.float32([[-1, 1, -1, 1], [-1, 1, 1, -1], [-1, 1, 1, 1]])      # exact -1 and 1
        lines = ["P " + hx(*img[0, :, 0, i]) for i in range(img.shape[-1])]
    else:
        img = np.round(px * 255).astype(np.uint8).reshape(1, 1, -1, 3)                      # (NV = 1, 1, n, 3)
        lines = ["Q %d %d %d" % tuple(p) for p in img[0, 0]]
    for f in FACTOR_SETS:
        got = np.array(host_header(lines + ["C " + hx(*f)])).T.reshape(1, 3, 1, -1)
        ref = ar.jitter(img, f)
        bar, e_host = ar.bar(img, f, ref)
        err = np.abs(got - ref).max()
        print("chain %s %s: header %.3g, host %.3g, bar %.3g" % (fmt, f.tolist(), err, e_host, bar))
        assert err <= bar
        assert got.min() >= -1.0 and got.max() <= 1.0


# --------------------------------------------------------------------------- C ABI
def test_entry_is_declared_bound_and_exported():
    """What is this entry's own (declared, bound, exported, its layout and constants: tests/test_cpu_abi.py)."""
    hdr = header_text()
    assert re.search(r"\bint\s+pny_color_jitter\s*\(\s*const\s+pny_color_jitter_desc\s*\*\s*desc\s*,\s*const\s+void\s*\*\s*images_dev\s*,"
                     r"\s*const\s+float\s*\*\s*factors_host\s*,\s*float\s*\*\s*out_dev\s*,\s*pny_stream\s+stream\s*\)", header_code())
    # the comment of the entry names the reference lines it replaces, as every other entry does
    block = hdr[hdr.index("---- colour jitter"):hdr.index("int pny_color_jitter")]
    assert "data_util.py:34-47" in block
    # the sources are part of the build
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " augment.hip" in mk and " augment_api.hip" in mk and " pny_augment.h" in mk


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    """PNY_ERR_ARG (-1) with a message, whether or not a GPU is there (the device pointers are never dereferenced by the host)."""
    call = built_lib.pny_color_jitter
    ok = dict(n_objs=2, n_views=3, height=9, width=8, in_format=0)
    p, p2 = C.c_void_p(4096), C.c_void_p(1 << 20)
    good = (C.c_float * 256)(*([0.0, 1.0, 1.0, 1.0] * 64))

    def rc(images=p, factors=good, out=p2, **over):
        d = plib.ColorJitterDesc(**dict(ok, **over))
        return call(C.byref(d), images, factors, out, None)

    def with_factor(obj, slot, value, **over):
        f = (C.c_float * 256)(*([0.0, 1.0, 1.0, 1.0] * 64))
        f[4 * obj + slot] = value
        return rc(factors=f, **over)

    err = built_lib.pny_last_error
    assert call(None, p, good, p2, None) == -1 and b"null" in err()
    assert rc(images=None) == -1 and b"null" in err()
    assert rc(factors=None) == -1 and b"null" in err()
    assert rc(out=None) == -1 and b"null" in err()
    for bad in (dict(n_objs=0), dict(n_views=-1), dict(height=0), dict(width=-3)):
        assert rc(**bad) == -1 and b"positive" in err(), bad
    assert rc(in_format=2) == -1 and rc(in_format=-1) == -1 and b"in_format" in err()
    assert rc(n_objs=65) == -1 and b"64 objects" in err()
    assert rc(n_objs=64, n_views=2 ** 9, height=2 ** 8, width=2 ** 8) == -1 and b"2^31" in err()     # 3 * 2^31 elements
    assert rc(n_objs=1, n_views=1, height=2 ** 16, width=2 ** 16) == -1 and b"2^31" in err()         # H * W alone overflows an int
    assert rc(n_objs=1, n_views=1, height=2 ** 15, width=21846) == -1 and b"2^31" in err()           # 2^31 + 3 * 2^15 elements
    for obj in (0, 1):
        for hue_f in (0.5001, -0.51, float("nan"), float("inf")):
            assert with_factor(obj, 0, hue_f) == -1 and b"hue" in err(), (obj, hue_f)
        for slot in (1, 2, 3):
            for v in (-1e-6, float("nan"), float("inf"), -float("inf")):
                assert with_factor(obj, slot, v) == -1 and b"finite and not negative" in err(), (obj, slot, v)
    assert with_factor(2, 1, -1.0, in_format=2) == -1 and b"in_format" in err()      # objects beyond n_objs are not read
    assert rc(out=p, in_format=1) == -1 and b"in place" in err()


# --------------------------------------------------------------------------- Python
def test_python_refuses_by_name():
    x = torch.zeros(2, 3, 9, 8)
    f = [0.0, 1.0, 1.0, 1.0]
    with pytest.raises(plib.PnyError, match="images is on cpu.*MI355X only"):
        paug.color_jitter(x, f)
    with pytest.raises(plib.PnyError, match="images is on cpu"):
        paug.color_jitter(torch.zeros(2, 9, 8, 3, dtype=torch.uint8), f)
    with pytest.raises(TypeError, match="images must be a tensor"):
        paug.color_jitter(x.numpy(), f)
    with pytest.raises(plib.PnyError, match="images must be fp32 .* or uint8 .*got torch.float64"):
        paug.color_jitter(x.double(), f)
    with pytest.raises(plib.PnyError, match="got torch.int32"):
        paug.color_jitter(torch.zeros(2, 9, 8, 3, dtype=torch.int32), f)
    with pytest.raises(ValueError, match=r"images must be \(NV, 3, H, W\) or \(SB, NV, 3, H, W\) for fp32, got \(3, 9, 8\)"):
        paug.color_jitter(x[0], f)
    with pytest.raises(ValueError, match=r"for fp32, got \(2, 9, 8, 3\)"):
        paug.color_jitter(torch.zeros(2, 9, 8, 3), f)                            # NHWC floats
    with pytest.raises(ValueError, match=r"for uint8, got \(2, 3, 9, 8\)"):
        paug.color_jitter(torch.zeros(2, 3, 9, 8, dtype=torch.uint8), f)         # NCHW bytes
    with pytest.raises(ValueError, match=r"got \(1, 1, 2, 3, 9, 8\)"):
        paug.color_jitter(x[None, None], f)
    with pytest.raises(ValueError, match=r"factors has shape \(2, 4\); 3 objects need \(3, 4\)"):
        paug.color_jitter(torch.zeros(3, 2, 3, 9, 8), torch.ones(2, 4))
    with pytest.raises(ValueError, match=r"factors has shape \(4,\); 3 objects need \(3, 4\)"):
        paug.color_jitter(torch.zeros(3, 2, 3, 9, 8), f)
    with pytest.raises(ValueError, match=r"factors has shape \(3,\); 1 object needs \(1, 4\).* or \(4,\)"):
        paug.color_jitter(x, f[:3])
    with pytest.raises(ValueError, match=r"factors has shape \(2, 4\); 1 object needs"):
        paug.color_jitter(x, torch.ones(2, 4))


class _Base(torch.utils.data.Dataset):
    """A synthetic base dataset with the attributes ColorJitterDataset inherits."""
    z_near, z_far, base_path, image_to_tensor = 0.5, 2.0, "synthetic", staticmethod(pdata.image_to_tensor_balanced)

    def __init__(self, n=3, nv=2, h=5, w=7):
        self.images = [torch.from_numpy(random_images(20 + i, nv, h, w)) for i in range(n)]

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return {"img_id": i, "images": self.images[i].clone()}


def test_deferred_dataset_draws_the_same_factors_and_leaves_the_images():
    base = _Base()
    host, deferred = pdata.ColorJitterDataset(base), pdata.ColorJitterDataset(base, defer=True)
    assert host.defer is False and deferred.defer is True and len(deferred) == 3 and deferred.z_far == 2.0
    for k in (0, 1, 7):
        np.random.seed(k)
        want = [np.random.uniform(-0.1, 0.1)] + [np.random.uniform(0.9, 1.1) for _ in range(3)]      # hue, sat, bri, con
        after_four = np.random.uniform()
        np.random.seed(k)
        a = host[1]
        assert np.random.uniform() == after_four                   # the host path makes exactly these four draws ...
        np.random.seed(k)
        b = deferred[1]
        assert np.random.uniform() == after_four                   # ... and the deferred path too
        assert "jitter" not in a and not torch.equal(a["images"], base.images[1])
        assert torch.equal(b["images"], base.images[1])           # untouched
        assert b["jitter"].dtype == torch.float32 and tuple(b["jitter"].shape) == (4,)
        assert torch.equal(b["jitter"], torch.tensor(want, dtype=torch.float32))
        # those factors reproduce the host path's images: the restatement with them is as close as with the fp64 draws
        assert np.abs(ar.jitter(base.images[1].numpy(), b["jitter"].numpy()) - a["images"].numpy()).max() < ar.FLOOR
    np.random.seed(3)
    batch = torch.utils.data.default_collate([deferred[0], deferred[2]])
    assert tuple(batch["jitter"].shape) == (2, 4) and tuple(batch["images"].shape) == (2, 2, 3, 5, 7)
    assert not torch.equal(batch["jitter"][0], batch["jitter"][1])


def _yolo_tree(root):
    rs = np.random.RandomState(1)
    d = os.path.join(root, "scene0")
    os.makedirs(d)
    for v in range(2):
        pdata.imwrite(os.path.join(d, "image_%04d.png" % v), rs.randint(0, 255, size=(16, 24, 3)).astype(np.uint8))
        np.save(os.path.join(d, "extrinsic_%04d.npy" % v), np.eye(4))
        with open(os.path.join(d, "projected_bboxes_%04d.txt" % v), "w") as fh:
            fh.write("1 0.30 0.40 0.20 0.30\n")
    np.save(os.path.join(d, "intrinsic_0000.npy"), np.array([[20.0, 0, 12.0], [0, 20.0, 8.0], [0, 0, 1]]))
    open(os.path.join(root, "train.lst"), "w").write("scene0\n")
    return {"yolo.image_scale": [1.0, 1.0], "model.mlp_coarse.num_scales": 1, "model.mlp_coarse.num_anchors_per_scale": 3,
            "yolo.cell_sizes": [4], "yolo.anchors": [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)]], "yolo.ignore_iou_thresh": 0.5}


def test_get_split_dataset_wires_the_deferred_jitter(tmp_path):
    from test_cpu_data import _dvr_tree
    root, _, _ = _dvr_tree(str(tmp_path / "dtu"), "dtu")
    os.rename(os.path.join(root, "02958343", "new_val.lst"), os.path.join(root, "02958343", "new_train.lst"))
    yroot = str(tmp_path / "yolo")
    os.makedirs(yroot)
    conf = _yolo_tree(yroot)
    for kind, path, kw in (("dvr_dtu", root, {}), ("yolo", yroot, {"conf": conf})):
        plain = pdata.get_split_dataset(kind, path, want_split="train", training=True, **kw)
        dev = pdata.get_split_dataset(kind, path, want_split="train", training=True, jitter_on_device=True, **kw)
        assert isinstance(plain, pdata.ColorJitterDataset) and plain.defer is False        # the default is unchanged
        assert isinstance(dev, pdata.ColorJitterDataset) and dev.defer is True
        assert dev.z_near == plain.z_near and dev.z_far == plain.z_far
        np.random.seed(11)
        a = plain[0]
        np.random.seed(11)
        b = dev[0]
        assert "jitter" not in a and tuple(b["jitter"].shape) == (4,)
        assert torch.equal(b["images"], dev.base_dset[0]["images"]) and not torch.equal(a["images"], b["images"])
        assert np.abs(ar.jitter(b["images"].numpy(), b["jitter"].numpy()) - a["images"].numpy()).max() < ar.FLOOR
