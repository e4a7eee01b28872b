"""
The device ingest without a GPU (include/pnyolo.h pny_ingest_views / pny_yolo_build_targets, augment.ingest_views,
util.build_yolo_targets, data.get_split_dataset(ingest_on_device=True)):

  * the kernels' own arithmetic (csrc/pny_ingest.h compiled by g++, the way tests/test_cpu_augment.py compiles its header): the
    byte map for all 256 bytes bit-equal to data.image_to_tensor_balanced; the bilinear taps and weights and the area windows
    against torch for every (in, out) pair up to 40; a whole bilinear resize with exact ties, byte for byte; the assignment walk
    on 200 random views against YOLODataset._get_all_bboxes, bit for bit, with distinct IoUs asserted;
  * the float64 restatements the GPU tests compare against (tests/ingest_ref.py) against data.py's host functions and closed
    forms: a constant image stays constant under every resize, 2:1 area is the 4-pixel mean;
  * the C ABI: every listed refusal before any launch (the boundary itself: tests/test_cpu_abi.py);
  * Python: refusals by argument name; on synthetic trees the ingest_on_device items of `yolo` and `srn` hold exactly the bytes,
    labels and intrinsics the default items are computed from; the `dvr*` and `multi_obj` types refuse the flag.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from host_tools import CSRC, built_lib, header_code, host_header_program  # noqa: F401
import ingest_ref as ir
from pixel_nerf_yolo_amd import augment as paug
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import data as pdata
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import util as putil

HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pny_ingest.h"
// one query per input line:
//   B                      -> 256 lines: the byte map
//   T in out               -> out lines `i0 i1 lambda`
//   A in out               -> out lines `start end`
//   I h w oh ow  + h*w lines `r g b`   -> oh*ow lines `r g b`: the bilinear resize, bytes
//   G n_scales A thresh H W cell.. then n_scales*A lines `aw ah`   the geometry of the walks that follow
//   V n  + n lines `cx cy w h cls`  -> per scale one line of the view's grid, flattened
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) return 2;
    static char line[512];
    pny::TargetsGeom g;
    memset(&g, 0, sizeof g);
    while (fgets(line, sizeof line, f)) {
        char kind = line[0];
        if (kind == 'B') {
            for (int b = 0; b < 256; ++b) printf("%a\n", (double)pny::ingest_byte_map((uint32_t)b));
        } else if (kind == 'T' || kind == 'A') {
            int in, out;
            if (sscanf(line + 1, "%d %d", &in, &out) != 2) return 3;
            for (int d = 0; d < out; ++d) {
                if (kind == 'T') {
                    int i0, i1;
                    float lam;
                    pny::ingest_bilinear_taps(d, (float)in / (float)out, in, i0, i1, lam);
                    printf("%d %d %a\n", i0, i1, (double)lam);
                } else {
                    int s, e;
                    pny::ingest_area_window(d, in, out, s, e);
                    printf("%d %d\n", s, e);
                }
            }
        } else if (kind == 'I') {
            int h, w, oh, ow;
            if (sscanf(line + 1, "%d %d %d %d", &h, &w, &oh, &ow) != 4) return 3;
            std::vector<uint32_t> px((size_t)h * w * 3);
            for (int i = 0; i < h * w; ++i) {
                if (!fgets(line, sizeof line, f) || sscanf(line, "%u %u %u", &px[3 * i], &px[3 * i + 1], &px[3 * i + 2]) != 3) return 3;
            }
            for (int y = 0; y < oh; ++y)
                for (int x = 0; x < ow; ++x) {
                    int y0, y1, x0, x1;
                    float ly, lx;
                    pny::ingest_bilinear_taps(y, (float)h / (float)oh, h, y0, y1, ly);
                    pny::ingest_bilinear_taps(x, (float)w / (float)ow, w, x0, x1, lx);
                    uint32_t o[3];
                    for (int c = 0; c < 3; ++c)
                        o[c] = pny::ingest_bilinear_u8(px[(y0 * w + x0) * 3 + c], px[(y0 * w + x1) * 3 + c], px[(y1 * w + x0) * 3 + c],
                                                       px[(y1 * w + x1) * 3 + c], lx, ly);
                    printf("%u %u %u\n", o[0], o[1], o[2]);
                }
        } else if (kind == 'G') {
            int H, W, n = 0, used = 0;
            double th;
            if (sscanf(line + 1, "%d %d %la %d %d%n", &g.n_scales, &g.n_anchors, &th, &H, &W, &used) != 5) return 3;
            g.thresh = (float)th;
            char* p = line + 1 + used;
            for (int s = 0; s < g.n_scales; ++s) {
                int cell = (int)strtol(p, &p, 10);
                g.hs[s] = H / cell, g.ws[s] = W / cell;
            }
            for (n = 0; n < g.n_scales * g.n_anchors; ++n) {
                double aw, ah;
                if (!fgets(line, sizeof line, f) || sscanf(line, "%la %la", &aw, &ah) != 2) return 3;
                g.anchors[2 * n] = (float)aw, g.anchors[2 * n + 1] = (float)ah;
            }
        } else if (kind == 'V') {
            const int n = atoi(line + 1);
            std::vector<std::vector<float> > grids(g.n_scales);
            float* ptr[pny::TARGETS_MAX_SCALES] = {0, 0, 0, 0};
            for (int s = 0; s < g.n_scales; ++s) {
                grids[s].assign((size_t)g.hs[s] * g.ws[s] * g.n_anchors * 6, 0.0f);
                ptr[s] = grids[s].data();
            }
            float iou[pny::TARGETS_MAX_ANCHORS];
            for (int b = 0; b < n; ++b) {
                double box[5];
                if (!fgets(line, sizeof line, f) || sscanf(line, "%la %la %la %la %la", box, box + 1, box + 2, box + 3, box + 4) != 5) return 3;
                pny::targets_assign_box(g, box, ptr, iou);
            }
            for (int s = 0; s < g.n_scales; ++s) {
                for (size_t i = 0; i < grids[s].size(); ++i) printf("%a ", (double)grids[s][i]);
                printf("\n");
            }
        } else {
            return 4;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    """csrc/pny_ingest.h compiled by g++: __host__ / __device__ defined away, no fused multiply-add -- the product's own code."""
    program = host_header_program(tmp_path_factory.mktemp("ingest_host"), HOST_MAIN,
                                  defines=("__device__=", "__host__=", "__forceinline__=inline"), include_dirs=(CSRC,))
    return lambda queries: [line.split() for line in program(queries)]


def test_header_byte_map_is_the_hosts_for_all_256_bytes(host_header):
    got = np.array([float.fromhex(r[0]) for r in host_header(["B"])])
    host = pdata.image_to_tensor_balanced(np.arange(256, dtype=np.uint8).reshape(16, 16, 1)).reshape(-1).numpy()
    assert got.shape == (256,) and np.array_equal(got.astype(np.float32), host) and np.array_equal(got, host.astype(np.float64))
    assert got[0] == -1.0 and got[255] == 1.0
    assert np.abs(host.astype(np.float64) - ir.byte_map(np.arange(256))).max() <= 2.0 ** -24


PAIRS = [(i, o) for i in range(1, 41) for o in range(1, 41)]


def test_header_bilinear_taps_against_torch_for_every_pair_up_to_40(host_header):
    rows = host_header(["T %d %d" % p for p in PAIRS])
    k = exact = 0
    for n_in, n_out in PAIRS:
        got = rows[k:k + n_out]
        k += n_out
        i0 = np.array([int(r[0]) for r in got])
        i1 = np.array([int(r[1]) for r in got])
        lam = np.array([float.fromhex(r[2]) for r in got]).astype(np.float32)
        assert (0 <= i0).all() and (i0 <= i1).all() and (i1 <= n_in - 1).all() and (i1 - i0 <= 1).all()
        assert (lam >= 0).all() and (lam < 1).all()
        w = np.zeros((n_out, n_in), np.float32)
        w[np.arange(n_out), i0] += np.float32(1) - lam
        w[np.arange(n_out), i1] += lam
        # torch's weights: the resize of the identity, tap k of output d in [k, d].  Both evaluate src = scale (dst + 0.5) - 0.5
        # below 64 with at most two roundings (torch's build fuses the multiply-add, as the header does): each within 2^-18 of
        # the real value, so the weights within 2^-17 of each other -- also where src sits at an integer and the taps shift by one
        ref = F.interpolate(torch.eye(n_in)[None], size=n_out, mode="linear", align_corners=False)[0].numpy().T
        assert np.abs(w.astype(np.float64) - ref).max() <= 2.0 ** -17, (n_in, n_out)
        exact += int(np.array_equal(w, ref))
        r0, r1, rl = ir._taps(n_in, n_out)
        wr = np.zeros((n_out, n_in))
        np.add.at(wr, (np.arange(n_out), r0), 1 - rl)
        np.add.at(wr, (np.arange(n_out), r1), rl)
        assert np.abs(wr - ref).max() <= 2.0 ** -17, (n_in, n_out)
    print("bilinear weights bit-equal to torch's for %d of %d (in, out) pairs" % (exact, len(PAIRS)))
    assert k == len(rows)


def test_header_area_windows_against_torch_for_every_pair_up_to_40(host_header):
    rows = host_header(["A %d %d" % p for p in PAIRS])
    k = 0
    for n_in, n_out in PAIRS:
        got = np.array([[int(v) for v in r] for r in rows[k:k + n_out]])
        k += n_out
        ref = F.interpolate(torch.eye(n_in, dtype=torch.float64)[None], size=n_out, mode="area")[0].numpy().T     # (out, in)
        for d in range(n_out):
            s, e = got[d]
            assert 0 <= s < e <= n_in
            inside = np.zeros(n_in, bool)
            inside[s:e] = True
            assert np.array_equal(ref[d] != 0, inside), (n_in, n_out, d)
            assert np.allclose(ref[d, s:e], 1.0 / (e - s), rtol=1e-15)
        rs, re_ = ir.area_windows(n_in, n_out)
        assert np.array_equal(got[:, 0], rs) and np.array_equal(got[:, 1], re_)
    assert k == len(rows)


def test_header_bilinear_resize_with_exact_ties_is_the_hosts_byte_for_byte(host_header):
    """27 x 48 -> 13 x 24 by (0.5, 0.47407): x is 2:1 (lambda = 0.5), y is 27 / 13; and 8 x 12 -> 4 x 6, both axes 2:1, where
    every output is a mean of four bytes: sums = 2 mod 4 are exact ties, rounded half to even."""
    rs = np.random.RandomState(3)
    for (h, w), (fx, fy) in (((8, 12), (0.5, 0.5)), ((27, 48), (0.5, 0.47407)), ((5, 4), (2.0, 2.0))):
        img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        img[:2, :2] = [[[1, 0, 255], [0, 2, 255]], [[0, 0, 254], [1, 1, 255]]]        # sums 2, 3, 1019: 0.5 -> 0, 0.75 -> 1, 254.75
        host = pdata.resize_bilinear_u8(img, fx, fy)
        oh, ow = host.shape[:2]
        rows = host_header(["I %d %d %d %d" % (h, w, oh, ow)] + ["%d %d %d" % tuple(p) for p in img.reshape(-1, 3)])
        got = np.array([[int(v) for v in r] for r in rows], np.uint8).reshape(oh, ow, 3)
        ref = ir.bilinear(img[None], oh, ow)[0]
        if (fx, fy) == (0.5, 0.5):
            ties = np.abs(ref - np.floor(ref) - 0.5) < 1e-12
            assert ties.sum() > 10 and np.array_equal(got, host)
            assert np.array_equal(got[ties], (2 * np.round(ref[ties] / 2)).astype(np.uint8))        # half to even
            assert got[0, 0].tolist() == [0, 1, 255]
        assert np.abs(got.astype(np.float64) - ref).max() <= 0.5 + 1e-4
        assert np.abs(host.astype(np.float64) - ref).max() <= 0.5 + 1e-4
        assert np.abs(got.astype(np.int32) - host.astype(np.int32)).max() <= 1


def random_views(seed, n_views, anchors, max_boxes=6):
    """Boxes whose IoUs against the anchors are pairwise distinct (redrawn otherwise); sizes spread over the anchors' range."""
    rs = np.random.RandomState(seed)
    views = []
    for _ in range(n_views):
        boxes = []
        for _ in range(rs.randint(0, max_boxes + 1)):
            while True:
                w, h = np.exp(rs.uniform(np.log(0.01), np.log(0.95), size=2))
                box = [float(rs.uniform(0, 1)), float(rs.uniform(0, 1)), float(w), float(h), float(rs.randint(0, 5))]
                if ir.distinct_ious([[box]], anchors):
                    break
            boxes.append(box)
        if boxes and rs.rand() < 0.5:                         # a second box in the cell of the first, of like size
            b = boxes[0]
            boxes.append([b[0], b[1], b[2] * 1.01, b[3] * 0.99, 1.0])
            if not ir.distinct_ious([[boxes[-1]]], anchors):
                boxes.pop()
        views.append(boxes)
    return views


def walk_queries(views, height, width, cells, anchors, n_anchors, thresh):
    q = ["G %d %d %s %d %d %s" % (len(cells), n_anchors, float(np.float32(thresh)).hex(), height, width, " ".join(str(c) for c in cells))]
    q += ["%s %s" % (float(np.float32(a[0])).hex(), float(np.float32(a[1])).hex()) for a in np.asarray(anchors).reshape(-1, 2)]
    for v in views:
        q.append("V %d" % len(v))
        q += [" ".join(float(x).hex() for x in b) for b in v]
    return q


def test_header_walk_against_get_all_bboxes_on_200_random_views(host_header):
    height, width, cells, A = 64, 96, [32, 16, 8], 3
    views = random_views(11, 200, ir.YOLO_ANCHORS)
    assert ir.distinct_ious(views, ir.YOLO_ANCHORS) and sum(len(v) for v in views) > 400
    rows = host_header(walk_queries(views, height, width, cells, ir.YOLO_ANCHORS, A, ir.YOLO_IGNORE_IOU))
    host = ir.host_targets(views, height, width, cells, ir.YOLO_ANCHORS, A, ir.YOLO_IGNORE_IOU)
    assert len(rows) == 200 * 3
    marks = 0
    for v in range(200):
        stable = ir.yolo_targets(views[v], height, width, cells, ir.YOLO_ANCHORS, A, ir.YOLO_IGNORE_IOU)
        for s in range(3):
            got = np.array([float.fromhex(x) for x in rows[3 * v + s]], np.float64).astype(np.float32)
            want = host[v][s][0].numpy()
            assert np.array_equal(got.reshape(want.shape), want), (v, s)
            assert np.array_equal(stable[s], want), (v, s)
            marks += int((want[..., 0] == -1).sum())
    assert marks > 20                                       # the ignore branch is exercised


def test_header_walk_with_duplicated_anchors_takes_the_lower_index(host_header):
    anchors = [[0.1, 0.1], [0.1, 0.1], [0.3, 0.3], [0.1, 0.1], [0.3, 0.3], [0.3, 0.3]]
    views = [[[0.3, 0.3, 0.1, 0.1, 2.0], [0.3, 0.3, 0.1, 0.1, 3.0], [0.7, 0.2, 0.3, 0.3, 1.0]]]
    rows = host_header(walk_queries(views, 32, 32, [16, 8], anchors, 3, 0.5))
    want = ir.yolo_targets(views[0], 32, 32, [16, 8], anchors, 3, 0.5)
    for s in range(2):
        got = np.array([float.fromhex(x) for x in rows[s]]).astype(np.float32).reshape(want[s].shape)
        assert np.array_equal(got, want[s])
    # anchors 0, 1 and 3 tie at IoU 1 and are visited in that order.  First box: anchor 0 takes scale 0, anchor 1 is marked,
    # anchor 3 takes scale 1.  Second box, same cell: all three are taken or marked, so it falls to anchors 2 and 4.
    assert want[0][0, 0, 0, 0] == 1 and want[0][0, 0, 0, 5] == 2 and want[0][0, 0, 1, 0] == -1
    assert want[1][1, 1, 0, 0] == 1 and want[1][1, 1, 0, 5] == 2
    assert want[0][0, 0, 2, 0] == 1 and want[0][0, 0, 2, 5] == 3 and want[1][1, 1, 1, 0] == 1 and want[1][1, 1, 1, 5] == 3


# --------------------------------------------------------------------------- the restatements
def test_restatement_against_the_host_functions():
    rs = np.random.RandomState(5)
    u8 = rs.randint(0, 256, size=(2, 27, 45, 3)).astype(np.uint8)
    assert np.abs(ir.host_images(u8).numpy().astype(np.float64) - ir.images_nchw(u8)).max() <= 2.0 ** -24
    for (fx, fy) in ((0.5, 0.47407), (1.7, 1.3), (0.31, 0.9)):
        host, res = ir.host_bilinear(u8, fx, fy)
        ref = ir.bilinear(u8, res.shape[1], res.shape[2])
        err = np.abs(res.astype(np.float64) - ref).max()
        print("bilinear (%g, %g): host bytes against the unrounded restatement %.6f" % (fx, fy, err))
        assert err <= 0.5 + 1e-4
    for size in ((9, 15), (13, 22), (27, 45), (30, 50)):
        host = F.interpolate(ir.host_images(u8), size=size, mode="area").numpy()
        err = np.abs(host.astype(np.float64) - ir.area(ir.images_nchw(u8), *size)).max()
        k = ir.largest_window(27, 45, *size)
        print("area %s: host against the restatement %.3g, window %d" % (size, err, k))
        assert err <= (k + 8) * 2.0 ** -24


def test_restatement_closed_forms():
    const = np.full((1, 7, 9, 3), 77, np.uint8)
    for oh, ow in ((7, 9), (3, 4), (10, 20), (1, 1)):
        assert np.abs(ir.bilinear(const, oh, ow) - 77.0).max() < 1e-12
        assert np.abs(ir.area(ir.images_nchw(const), oh, ow) - ir.byte_map(77)).max() < 1e-15
    rs = np.random.RandomState(6)
    u8 = rs.randint(0, 256, size=(2, 12, 18, 3)).astype(np.uint8)
    x = ir.images_nchw(u8)
    four = (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) / 4
    assert np.abs(ir.area(x, 6, 9) - four).max() < 1e-15
    assert np.abs(ir.bilinear(u8, 6, 9) - np.moveaxis((four * 0.5 + 0.5) * 255, 1, -1)).max() < 1e-10    # 2:1 bilinear too
    assert np.array_equal(ir.bilinear(u8, 12, 18), u8.astype(np.float64))                                  # 1:1 is the identity


def test_restatement_of_the_srn_mask_and_box():
    img = np.full((3, 8, 10, 3), 255, np.uint8)
    img[0, 2:5, 3:7] = 10
    img[0, 6, 1] = (255, 3, 3)                # one byte at 255: outside, as `(img != 255).all(axis=-1)` has it
    img[1, 7, 0] = (0, 0, 254)
    m, b = ir.srn_mask_bbox(img)
    assert m.shape == (3, 1, 8, 10) and m[0].sum() == 12 and m[0, 0, 6, 1] == 0 and m[1].sum() == 1 and m[2].sum() == 0
    assert b.tolist() == [[3, 2, 6, 4], [0, 7, 0, 7], [10, 8, -1, -1]]


# --------------------------------------------------------------------------- C ABI
def test_entries_are_declared_bound_and_exported():
    """What is these entries' own (declared, bound, exported, their layouts and constants: tests/test_cpu_abi.py)."""
    code = header_code()
    assert re.search(r"\bint\s+pny_ingest_views\s*\(\s*const\s+pny_ingest_desc\s*\*\s*desc\s*,\s*const\s+uint8_t\s*\*\s*images_dev\s*,"
                     r"\s*float\s*\*\s*out_dev\s*,\s*float\s*\*\s*mask_dev\s*,\s*float\s*\*\s*bbox_dev\s*,\s*pny_stream\s+stream\s*\)", code)
    assert re.search(r"\bint\s+pny_yolo_build_targets\s*\(\s*const\s+pny_yolo_targets_desc\s*\*\s*desc\s*,\s*const\s+double\s*\*\s*boxes_dev\s*,"
                     r"\s*const\s+int32_t\s*\*\s*n_boxes_dev\s*,\s*const\s+float\s*\*\s*anchors_host\s*,\s*float\s*\*\s*const\s*\*\s*targets_dev\s*,"
                     r"\s*pny_stream\s+stream\s*\)", code)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " ingest.hip" in mk and " ingest_api.hip" in mk and " pny_ingest.h" in mk


def test_ingest_refuses_bad_arguments_before_any_launch(built_lib):
    """PNY_ERR_ARG (-1) with a message, whether or not a GPU is there (the device pointers are never dereferenced by the host)."""
    call, err = built_lib.pny_ingest_views, built_lib.pny_last_error
    ok = dict(n_views=2, height=9, width=8, channels=3, out_height=9, out_width=8, resize=0, white_mask=0)
    p, p2, p3, p4 = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))

    def rc(images=p, out=p2, mask=None, bbox=None, **over):
        d = plib.IngestDesc(**dict(ok, **over))
        return call(C.byref(d), images, out, mask, bbox, None)

    assert call(None, p, p2, None, None, None) == -1 and b"null" in err()
    assert rc(images=None) == -1 and b"null" in err()
    assert rc(out=None) == -1 and b"null" in err()
    for bad in (dict(n_views=0), dict(height=-1), dict(width=0), dict(out_height=0, resize=2), dict(out_width=-2, resize=1)):
        assert rc(**bad) == -1 and b"positive" in err(), bad
    for ch in (0, 1, 2, 5):
        assert rc(channels=ch) == -1 and b"channels" in err()
    assert rc(resize=3) == -1 and rc(resize=-1) == -1 and b"unknown resize" in err()
    assert rc(out_height=8) == -1 and b"PNY_RESIZE_NONE" in err()
    assert rc(out_width=9) == -1 and b"PNY_RESIZE_NONE" in err()
    assert rc(n_views=1, height=2 ** 16, width=2 ** 16, out_height=4, out_width=4, resize=2) == -1 and b"2^31" in err()
    assert rc(n_views=2 ** 10, height=2 ** 10, width=2 ** 10, channels=4, out_height=4, out_width=4, resize=2) == -1 and b"2^31" in err()
    assert rc(n_views=2 ** 10, height=4, width=4, out_height=2 ** 10, out_width=2 ** 10, resize=1) == -1 and b"2^31" in err()
    assert rc(mask=p3) == -1 and b"need white_mask" in err()
    assert rc(bbox=p4) == -1 and b"need white_mask" in err()
    assert rc(white_mask=1) == -1 and b"white_mask needs" in err()
    assert rc(white_mask=1, mask=p3) == -1 and b"white_mask needs" in err()
    assert rc(white_mask=1, bbox=p4) == -1 and b"white_mask needs" in err()
    assert rc(white_mask=2, mask=p3, bbox=p4) == -1 and b"0 or 1" in err()
    assert rc(white_mask=1, mask=p3, bbox=p4, resize=1, out_height=4, out_width=4) == -1 and b"BILINEAR_U8" in err()


def test_targets_refuse_bad_arguments_before_any_launch(built_lib):
    call, err = built_lib.pny_yolo_build_targets, built_lib.pny_last_error
    ok = dict(n_views=2, max_boxes=3, height=64, width=96, n_scales=2, cell_sizes=(C.c_int32 * 4)(32, 16, 0, 0), n_anchors=3,
              ignore_iou_thresh=0.5)
    p, p2 = C.c_void_p(4096), C.c_void_p(8192)
    anchors = (C.c_float * 128)(*([0.1] * 128))
    grids = (C.c_void_p * 4)(1 << 20, 2 << 20, 3 << 20, 4 << 20)

    def rc(boxes=p, counts=p2, anc=anchors, tg=grids, **over):
        d = plib.YoloTargetsDesc(**dict(ok, **over))
        return call(C.byref(d), boxes, counts, anc, tg, None)

    assert call(None, p, p2, anchors, grids, None) == -1 and b"null" in err()
    for kw in (dict(boxes=None), dict(counts=None), dict(anc=None), dict(tg=None), dict(tg=(C.c_void_p * 4)(1 << 20, None, None, None))):
        assert rc(**kw) == -1 and b"null" in err(), kw
    for bad in (dict(n_views=0), dict(max_boxes=0), dict(height=0), dict(width=-1)):
        assert rc(**bad) == -1 and b"positive" in err(), bad
    assert rc(n_scales=0) == -1 and rc(n_scales=5) == -1 and b"n_scales" in err()
    assert rc(n_anchors=0) == -1 and rc(n_anchors=65) == -1 and rc(n_anchors=33) == -1 and b"at most 64" in err()
    for cells in ((0, 16, 0, 0), (32, -1, 0, 0), (65, 16, 0, 0), (32, 97, 0, 0)):
        assert rc(cell_sizes=(C.c_int32 * 4)(*cells)) == -1 and b"cell size" in err(), cells
    for th in (-0.1, float("nan"), float("inf")):
        assert rc(ignore_iou_thresh=th) == -1 and b"ignore_iou_thresh" in err(), th
    assert rc(n_views=2 ** 20, max_boxes=2 ** 10) == -1 and b"2^31" in err()
    assert rc(n_views=2 ** 16, height=2 ** 10, width=2 ** 10, n_scales=1, cell_sizes=(C.c_int32 * 4)(1, 0, 0, 0)) == -1 and b"2^31" in err()


# --------------------------------------------------------------------------- Python
def test_ingest_views_refuses_by_name():
    u8 = torch.zeros(2, 9, 8, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match="images_u8 must be a tensor"):
        paug.ingest_views(u8.numpy())
    with pytest.raises(plib.PnyError, match="images_u8 must be uint8 .*got torch.float32"):
        paug.ingest_views(u8.float())
    with pytest.raises(ValueError, match=r"images_u8 must be \(NV, H, W, C\) or \(SB, NV, H, W, C\) with C = 3 or 4, got \(9, 8, 3\)"):
        paug.ingest_views(u8[0])
    with pytest.raises(ValueError, match=r"got \(2, 3, 9, 8\)"):
        paug.ingest_views(torch.zeros(2, 3, 9, 8, dtype=torch.uint8))            # NCHW bytes
    with pytest.raises(ValueError, match="resize must be None, 'none', 'bilinear_u8' or 'area', got 'cubic'"):
        paug.ingest_views(u8, size=(4, 4), resize="cubic")
    with pytest.raises(ValueError, match="scale and size are both given"):
        paug.ingest_views(u8, size=(4, 4), scale=(0.5, 0.5))
    with pytest.raises(ValueError, match="scale goes with resize='bilinear_u8'.*got resize='area'"):
        paug.ingest_views(u8, scale=(0.5, 0.5), resize="area")
    with pytest.raises(ValueError, match="scale must be a pair"):
        paug.ingest_views(u8, scale=0.5)
    with pytest.raises(ValueError, match=r"scale \(0.01, 0.01\) gives an empty 0 x 0 output"):
        paug.ingest_views(u8, scale=(0.01, 0.01))
    with pytest.raises(ValueError, match="size needs resize='area' or resize='bilinear_u8', got resize=None"):
        paug.ingest_views(u8, size=(4, 4))
    with pytest.raises(ValueError, match="size must be positive"):
        paug.ingest_views(u8, size=(0, 4), resize="area")
    with pytest.raises(ValueError, match=r"resize='area' needs size=\(OH, OW\)"):
        paug.ingest_views(u8, resize="area")
    with pytest.raises(ValueError, match="white_mask goes with resize='area' or no resize"):
        paug.ingest_views(u8, scale=(0.5, 0.5), white_mask=True)
    with pytest.raises(plib.PnyError, match="images_u8 is on cpu.*MI355X only"):
        paug.ingest_views(u8)


def test_build_yolo_targets_refuses_by_name():
    lab, cnt = ir.pack_labels([[[0.5, 0.5, 0.1, 0.1, 0]], [[0.2, 0.2, 0.1, 0.1, 1], [0.3, 1.0, 0.1, 0.1, 2]]])
    args = dict(height=64, width=96, cell_sizes=[32], anchors=ir.YOLO_ANCHORS[:3], ignore_iou_thresh=0.5, device="cpu")
    with pytest.raises(ValueError, match=r"labels\[1, 1\] = \[0.3, 1.0, .*\(view 1, row 1\): cx and cy must lie in \[0, 1\)"):
        putil.build_yolo_targets(lab, cnt, **args)
    for col, v in ((0, -0.01), (2, 0.0), (3, float("inf")), (2, float("nan"))):
        bad = lab.copy()
        bad[0, 0, col] = v
        with pytest.raises(ValueError, match=r"labels\[0, 0\].*view 0, row 0"):
            putil.build_yolo_targets(bad, cnt, **args)
    bad = lab.copy()
    bad[0, 1] = [7, 7, -1, -1, 0]                                # beyond n_labels[0]: not read
    with pytest.raises(plib.PnyError, match="device is cpu.*MI355X only"):
        putil.build_yolo_targets(bad, np.array([1, 1], np.int32), **args)
    with pytest.raises(ValueError, match=r"labels must be \(NV, MAXB, 5\).*got \(2, 5\)"):
        putil.build_yolo_targets(lab[0], cnt, **args)
    with pytest.raises(ValueError, match=r"n_labels must be \(2,\) integers in 0 .. 2"):
        putil.build_yolo_targets(lab, np.array([1, 3]), **args)
    with pytest.raises(ValueError, match=r"n_labels must be \(2,\)"):
        putil.build_yolo_targets(lab, np.array([1]), **args)
    with pytest.raises(ValueError, match=r"anchors must be \(num_scales \* A, 2\) with 2 scales"):
        putil.build_yolo_targets(lab, cnt, **dict(args, cell_sizes=[32, 16]))
    with pytest.raises(ValueError, match="cell_sizes must hold 1 .. 4 scales, got 5"):
        putil.build_yolo_targets(lab, cnt, **dict(args, cell_sizes=[32, 16, 8, 4, 2]))


def test_conf_yolo_carries_the_dataset_block():
    c = pconf.yolo()
    assert c["yolo.image_scale"] == [0.5, 0.47407] and c["yolo.cell_sizes"] == [32] and c["yolo.ignore_iou_thresh"] == ir.YOLO_IGNORE_IOU
    assert [a for sub in c["yolo.anchors"] for a in sub] == ir.YOLO_ANCHORS


# --------------------------------------------------------------------------- datasets
def _yolo_tree(root, stage):
    rs = np.random.RandomState(1)
    d = os.path.join(root, "scene0")
    os.makedirs(d)
    H, W = 27, 48
    rows = [[(1, 0.30, 0.40, 0.20, 0.30), (0, 0.80, 0.75, 0.10, 0.12), (2, 0.31, 0.41, 0.21, 0.29)], [], [(3, 0.5, 0.5, 0.05, 0.04)]]
    imgs = []
    for v in range(3):
        img = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        imgs.append(img)
        pdata.imwrite(os.path.join(d, "image_%04d.png" % v), img)
        E = np.eye(4)
        E[:3, 3] = [0.1 * v, 0.2, 3.0]
        np.save(os.path.join(d, "extrinsic_%04d.npy" % v), E)
        with open(os.path.join(d, "projected_bboxes_%04d.txt" % v), "w") as fh:
            fh.write("".join("%d %r %r %r %r\n" % r for r in rows[v]))
    np.save(os.path.join(d, "intrinsic_0000.npy"), np.array([[100.0, 0, 24.0], [0, 100.0, 13.5], [0, 0, 1]]))
    open(os.path.join(root, stage + ".lst"), "w").write("scene0\n")
    conf = {"yolo.image_scale": [0.5, 0.47407], "model.mlp_coarse.num_scales": 1, "model.mlp_coarse.num_anchors_per_scale": 3,
            "yolo.cell_sizes": [4], "yolo.anchors": [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)]], "yolo.ignore_iou_thresh": 0.5}
    return conf, np.stack(imgs), rows


def test_yolo_items_carry_the_bytes_and_labels_the_default_items_come_from(tmp_path):
    import warnings
    root = str(tmp_path)
    conf, imgs, rows = _yolo_tree(root, "test")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # np.loadtxt on the empty label file of view 1
        plain = pdata.get_split_dataset("yolo", root, want_split="test", training=False, conf=conf)[0]
        ds = pdata.get_split_dataset("yolo", root, want_split="test", training=False, conf=conf, ingest_on_device=True)
        it = ds[0]
    assert ds.ingest_on_device is True and set(it) == {"path", "img_id", "focal", "images_u8", "labels", "n_labels", "image_scale",
                                                       "poses", "c"}
    assert it["images_u8"].dtype == torch.uint8 and np.array_equal(it["images_u8"].numpy(), imgs)
    assert it["n_labels"].tolist() == [3, 0, 1] and it["n_labels"].dtype == torch.int32
    assert tuple(it["labels"].shape) == (3, 3, 5) and it["labels"].dtype == torch.float64
    for v in range(3):
        for k, (cls, cx, cy, w, h) in enumerate(rows[v]):
            assert it["labels"][v, k].tolist() == [cx, cy, w, h, float(cls)]
    assert it["image_scale"].tolist() == [0.5, 0.47407]
    for key in ("focal", "c", "poses"):
        assert torch.equal(it[key], plain[key])
    # the default item is exactly the host chain on those bytes, and its grids the host walk on those labels
    host, _ = ir.host_bilinear(it["images_u8"].numpy(), *it["image_scale"].tolist())
    assert torch.equal(plain["images"], host) and tuple(host.shape) == (3, 3, 13, 24)
    views = [it["labels"][v, :int(it["n_labels"][v])].tolist() for v in range(3)]
    grids = ir.host_targets(views, 13, 24, [4], conf["yolo.anchors"][0], 3, 0.5)
    for v in range(3):
        assert torch.equal(grids[v][0][0], plain["bboxes"][v][0])
    # the training split composes with the deferred jitter, and refuses the host jitter
    os.rename(os.path.join(root, "test.lst"), os.path.join(root, "train.lst"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr = pdata.get_split_dataset("yolo", root, want_split="train", conf=conf, ingest_on_device=True, jitter_on_device=True)
        b = tr[0]
    assert isinstance(tr, pdata.ColorJitterDataset) and tr.defer and tuple(b["jitter"].shape) == (4,) and "images_u8" in b
    with pytest.raises(ValueError, match="needs jitter_on_device=True"):
        pdata.get_split_dataset("yolo", root, want_split="train", conf=conf, ingest_on_device=True)


def test_srn_items_carry_the_bytes_the_default_items_come_from(tmp_path):
    from test_cpu_data import _srn_tree
    path, truth = _srn_tree(str(tmp_path), "val")
    for size in ((16, 16), (8, 8)):
        plain = pdata.get_split_dataset("srn", path, want_split="val", training=False, image_size=size)[1]
        ds = pdata.get_split_dataset("srn", path, want_split="val", training=False, image_size=size, ingest_on_device=True)
        it = ds[1]
        assert set(it) == {"path", "img_id", "focal", "c", "images_u8", "image_size", "poses"}
        assert np.array_equal(it["images_u8"].numpy(), truth[1][1]) and it["image_size"].tolist() == list(size)
        for key in ("focal", "c", "poses"):
            assert torch.equal(it[key], plain[key]), key
        imgs, masks, bbox = ir.host_srn(it["images_u8"].numpy(), size)
        assert torch.equal(plain["images"], imgs) and torch.equal(plain["masks"], masks) and torch.equal(plain["bbox"], bbox)
    ws = pdata.SRNDataset(path, stage="val", image_size=(8, 8), world_scale=2.0, ingest_on_device=True)[0]
    ref = pdata.SRNDataset(path, stage="val", image_size=(8, 8), world_scale=2.0)[0]
    assert torch.equal(ws["focal"], ref["focal"]) and torch.equal(ws["poses"], ref["poses"])


def test_other_dataset_types_refuse_the_flag(tmp_path):
    for kind, name in (("dvr", "DVRDataset"), ("dvr_gen", "DVRDataset"), ("dvr_dtu", "DVRDataset"), ("multi_obj", "MultiObjectDataset")):
        with pytest.raises(NotImplementedError, match="ingest_on_device is not implemented for dataset type %r \\(%s\\)" % (kind, name)):
            pdata.get_split_dataset(kind, str(tmp_path), ingest_on_device=True)
