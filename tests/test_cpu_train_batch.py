"""
The training batch sampler without a GPU (include/pnyolo.h pny_sample_train_batch, util.sample_train_batch):

  * the C ABI: bad arguments come back as PNY_ERR_ARG before anything is launched (the boundary itself:
    tests/test_cpu_abi.py);
  * the kernel's own pixel arithmetic (csrc/pny_train_batch.h compiled by g++, the way tests/test_cpu_philox.py compiles
    pny_rng.h) gives exactly the (view, y, x) the reference's trainer chose for the draws recorded in
    tests/golden/train_batch.npz (tools/make_train_batch_golden.py);
  * the seeded integers equal a restatement on the oracle's Philox (tests/train_batch_ref.py) exactly: several seeds, one
    with a non-zero high word, a draw index beyond 2^32 - 1, n = 1, 2, 819 200 and 2^31.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from host_tools import CSRC, built_lib, header_code, header_text, host_header_program  # noqa: F401
import train_batch_ref as tb
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import util as putil

CASES = ("a_uni", "a_box", "b_uni", "b_box")


# --------------------------------------------------------------------------- C ABI
def test_entry_is_declared_bound_and_exported():
    """What is this entry's own (declared, bound, exported, its mirrors' layout: tests/test_cpu_abi.py)."""
    hdr = header_text()
    assert re.search(r"\bint\s+pny_sample_train_batch\s*\(\s*const\s+pny_train_batch_desc\s*\*", header_code())
    # the comment of the entry names the reference lines it replaces, as every other entry does
    block = hdr[:hdr.index("int pny_sample_train_batch")]
    block = block[block.rindex("pny_gen_rays_range"):]
    assert "PixelNerfTrainer.py:76-123" in block and "util.py:222-237" in block


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    """Shapes and required pointers are checked on the host: PNY_ERR_ARG (-1) with a message, whether or not a GPU is there
    (the pointers are never dereferenced by the host)."""
    call = built_lib.pny_sample_train_batch
    ok = dict(n_objs=2, n_views=3, height=8, width=8, n_rays=4, z_near=0.5, z_far=2.0, focal_rows=1, focal_cols=1, c_rows=1,
              seed=1, draw_offset=0)
    p = C.c_void_p(4096)    # stands for a device pointer (16-byte aligned)

    def rc(desc=None, images=p, poses=p, focal=p, c=None, boxes=None, draws=None, rays=p, rgb=p, **over):
        d = plib.TrainBatchDesc(**dict(ok, **over)) if desc is None else desc
        return call(C.byref(d) if d else None, images, poses, focal, c, boxes, draws, rays, rgb, None, None)

    assert call(None, p, p, p, None, None, None, p, p, None, None) == -1
    for missing in ("images", "poses", "focal", "rays", "rgb"):
        assert rc(**{missing: None}) == -1 and b"null" in built_lib.pny_last_error(), missing
    for bad in (dict(n_objs=0), dict(n_views=0), dict(height=0), dict(width=-1), dict(n_rays=0)):
        assert rc(**bad) == -1 and b"shape" in built_lib.pny_last_error(), bad
    assert rc(focal_rows=3) == -1 and rc(focal_cols=3) == -1 and b"focal" in built_lib.pny_last_error()
    assert rc(c=p, c_rows=3) == -1
    assert rc(n_views=2 ** 16, height=2 ** 8, width=2 ** 8) == -1 and b"2^32" in built_lib.pny_last_error()
    assert rc(rays=C.c_void_p(4100)) == -1 and b"aligned" in built_lib.pny_last_error()
    # replay: the pointers the mode reads must be there
    empty = plib.TrainBatchDraws()
    assert rc(draws=C.byref(empty)) == -1 and b"pix_inds_dev" in built_lib.pny_last_error()
    only_pix = plib.TrainBatchDraws(pix_inds_dev=4096)
    assert rc(draws=C.byref(only_pix), boxes=p) == -1 and b"image_ids_dev" in built_lib.pny_last_error()


def test_no_gpu_is_loud():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU path"):
        putil.sample_train_batch(torch.zeros(1, 2, 3, 8, 8), torch.eye(4).expand(1, 2, 4, 4), torch.tensor(10.0), 0.5, 2.0, 4)


# --------------------------------------------------------------------------- the kernel's header on the host
HOST_MAIN = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pny_train_batch.h"
// one query per input line:  F flat nv h w | B view u_x u_y cmin rmin cmax rmax h w | I seed stream idx n |
//                            S seed idx nv h w (the four seeded draws of one ray)
int main(int argc, char** argv) {
    printf("streams %u %u %u %u\n", (unsigned)pny::STREAM_BATCH_PIX, (unsigned)pny::STREAM_BATCH_VIEW,
           (unsigned)pny::STREAM_BATCH_X, (unsigned)pny::STREAM_BATCH_Y);
    FILE* f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) return 2;
    char line[512];
    while (fgets(line, sizeof line, f)) {
        char* t = strtok(line, " \n");
        char kind = t[0];
        char* a[16];
        int n = 0;
        while ((t = strtok(0, " \n")) && n < 16) a[n++] = t;
        if (kind == 'F') {
            pny::BatchPixel p = pny::pixel_from_flat(strtoll(a[0], 0, 10), atoi(a[1]), atoi(a[2]), atoi(a[3]));
            printf("%d %d %d\n", p.view, p.y, p.x);
        } else if (kind == 'B') {
            float box[4] = {strtof(a[3], 0), strtof(a[4], 0), strtof(a[5], 0), strtof(a[6], 0)};
            pny::BatchPixel p = pny::pixel_from_bbox(atoi(a[0]), strtof(a[1], 0), strtof(a[2], 0), box, atoi(a[7]), atoi(a[8]));
            printf("%d %d %d\n", p.view, p.y, p.x);
        } else if (kind == 'I') {
            printf("%u\n", pny::index_at(strtoull(a[0], 0, 10), (uint32_t)strtoul(a[1], 0, 10), strtoull(a[2], 0, 10),
                                        (uint32_t)strtoul(a[3], 0, 10)));
        } else if (kind == 'S') {
            const uint64_t seed = strtoull(a[0], 0, 10), idx = strtoull(a[1], 0, 10);
            const int nv = atoi(a[2]), h = atoi(a[3]), w = atoi(a[4]);
            printf("%lld %d %a %a\n", (long long)pny::seeded_flat(seed, idx, (uint32_t)((int64_t)nv * h * w)),
                   pny::seeded_view(seed, idx, nv), (double)pny::seeded_u_x(seed, idx), (double)pny::seeded_u_y(seed, idx));
        } else {
            return 3;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    """csrc/pny_train_batch.h (and pny_rng.h under it) compiled by g++: an empty hip/hip_runtime.h, __device__ defined away,
    no fused multiply-add -- the product's own code, run on lines of queries."""
    tmp = tmp_path_factory.mktemp("train_batch_host")
    (tmp / "hip").mkdir()
    (tmp / "hip" / "hip_runtime.h").write_text("")
    program = host_header_program(tmp, HOST_MAIN, include_dirs=(tmp, CSRC))

    def run(queries):
        lines = program(queries)
        assert lines[0] == "streams 5 6 7 8" and len(lines) == 1 + len(queries)
        return lines[1:]
    return run


def test_fixture_is_what_the_tool_describes(golden):
    g = golden("train_batch")
    SB, NV, H, W, B = (int(v) for v in g["shape"])
    assert (SB, NV, H, W, B) == (2, 5, 24, 16, 64) and H != W
    assert g["a_focal"].size == 1 and "a_c" not in g and g["b_focal"].shape == (SB, 2) and g["b_c"].shape == (SB, 2)
    bb = g["a_bboxes"]
    assert np.array_equal(bb, g["b_bboxes"]) and bb.shape == (SB, NV, 4)
    assert any(tuple(b) == (0, 0, W - 1, H - 1) for b in bb.reshape(-1, 4))          # touches every border
    assert any(b[0] == b[2] and b[1] < b[3] for b in bb.reshape(-1, 4))                # one pixel wide
    for key in CASES:
        pix = g[key + "_pix"]
        assert pix.shape == (SB, B, 3) and pix.dtype == np.int32
        assert pix[..., 0].min() >= 0 and pix[..., 0].max() < NV and pix[..., 1].max() < H and pix[..., 2].max() < W
        if key.endswith("box"):    # the boxes that matter were drawn from
            box = bb[np.arange(SB)[:, None], pix[..., 0]]
            assert bool(((pix[..., 2] >= box[..., 0]) & (pix[..., 2] <= box[..., 2]) & (pix[..., 1] >= box[..., 1])
                         & (pix[..., 1] <= box[..., 3])).all())
            assert bool(((pix[0, :, 0] == 1) & (pix[0, :, 2] == 7)).any()) and bool((pix[0, :, 0] == 0).any())


@pytest.mark.parametrize("key", CASES)
def test_host_compiled_header_picks_the_reference_pixels(golden, host_header, key):
    g = golden("train_batch")
    SB, NV, H, W, B = (int(v) for v in g["shape"])
    q = []
    for s in range(SB):
        for r in range(B):
            if key.endswith("uni"):
                q.append("F %d %d %d %d" % (g[key + "_pix_inds"][s, r], NV, H, W))
            else:
                v = int(g[key + "_image_ids"][s, r])
                box = g[key[0] + "_bboxes"][s, v]
                q.append("B %d %s %s %s %d %d" % (v, float(g[key + "_u_x"][s, r]).hex(), float(g[key + "_u_y"][s, r]).hex(),
                                                   " ".join(float(b).hex() for b in box), H, W))
    got = np.array([[int(v) for v in line.split()] for line in host_header(q)]).reshape(SB, B, 3)
    assert np.array_equal(got, g[key + "_pix"]), np.argwhere(got != g[key + "_pix"])[:5]
    # and the tests' own restatement agrees with the reference (it stands in for it in the seeded GPU tests)
    if key.endswith("uni"):
        mine = tb.flat_to_pix(g[key + "_pix_inds"], H, W)
    else:
        mine = np.stack([tb.bbox_to_pix(g[key + "_image_ids"][s], g[key + "_u_x"][s], g[key + "_u_y"][s], g[key[0] + "_bboxes"][s])
                         for s in range(SB)])
    assert np.array_equal(mine, g[key + "_pix"])


def test_host_compiled_header_guards_memory(host_header):
    """Out-of-range replayed draws and boxes beyond the image land inside it (the clamp valid input never reaches)."""
    NV, H, W = 3, 6, 4
    q = ["F -1 %d %d %d" % (NV, H, W), "F %d %d %d %d" % (NV * H * W, NV, H, W), "F %d %d %d %d" % (2 ** 40, NV, H, W),
         "B 1 0x1.fffffep-1 0x1.fffffep-1 0 0 100 100 %d %d" % (H, W), "B 1 0.5 0.5 -50 -50 -20 -20 %d %d" % (H, W),
         "B 1 nan 0.5 0 0 3 5 %d %d" % (H, W), "B 2 0.25 0.75 1e30 -1e30 2e30 1e30 %d %d" % (H, W)]
    got = [[int(v) for v in line.split()] for line in host_header(q)]
    assert got[0] == [0, 0, 0] and got[1] == [NV - 1, H - 1, W - 1] and got[2] == [NV - 1, H - 1, W - 1]
    assert got[3] == [1, H - 1, W - 1] and got[4] == [1, 0, 0]
    for v, y, x in got[5:]:
        assert 0 <= y < H and 0 <= x < W


SEEDS = (0, 42, 1234 + 7919, 2 ** 40 + 7, 2 ** 63 + 2 ** 32 + 5, 2 ** 64 - 1)
INDICES = (0, 1, 2, 3, 4, 5, 127, 128, 511, 99991, 2 ** 32 - 1, 2 ** 32 + 6, 2 ** 33 + 3)     # s * B + r, beyond 2^32 - 1 too
NS = (1, 2, 5, 819200, 49 * 300 * 400, 2 ** 31, 2 ** 32 - 1)


def test_seeded_integers_equal_the_restatement_on_the_oracle(host_header):
    cases = [(seed, stream, idx, n) for seed in SEEDS for stream in (tb.STREAM_BATCH_PIX, tb.STREAM_BATCH_VIEW) for idx in INDICES
             for n in NS]
    got = [int(line) for line in host_header(["I %d %d %d %d" % c for c in cases])]
    for (seed, stream, idx, n), v in zip(cases, got):
        # written out once more, on the raw words: word idx % 4 of counter idx // 4
        w = orc.philox4x32_10(((idx >> 2) & tb.M32, idx >> 34, stream, orc.PHILOX_COUNTER3), (seed & tb.M32, seed >> 32))[idx & 3]
        assert v == (int(w) * n) >> 32 == int(tb.batch_index(seed, stream, idx, n)), (seed, stream, idx, n)
        assert 0 <= v < n
    assert len({v for c, v in zip(cases, got) if c[3] == 2 ** 31}) > 100      # (not a constant)
    assert all(v == 0 for c, v in zip(cases, got) if c[3] == 1)


def test_seeded_draws_of_a_ray_use_their_four_streams(host_header):
    NV, H, W = 50, 128, 128
    cases = [(seed, idx) for seed in SEEDS for idx in INDICES]
    lines = host_header(["S %d %d %d %d %d" % (seed, idx, NV, H, W) for seed, idx in cases])
    for (seed, idx), line in zip(cases, lines):
        f = line.split()
        assert int(f[0]) == int(tb.batch_index(seed, tb.STREAM_BATCH_PIX, idx, NV * H * W))
        assert int(f[1]) == int(tb.batch_index(seed, tb.STREAM_BATCH_VIEW, idx, NV))
        assert float.fromhex(f[2]) == float(orc.philox_uniform(seed, tb.STREAM_BATCH_X, idx))
        assert float.fromhex(f[3]) == float(orc.philox_uniform(seed, tb.STREAM_BATCH_Y, idx))


def test_seeded_pix_layout_and_statistics():
    """The restatement the GPU tests compare against: an object's batch does not depend on the other objects of the call, the
    integers cover [0, n) evenly (chi-square over the views), every pixel is inside its box."""
    seed, SB, B, NV, H, W = 2 ** 40 + 7, 4, 128, 5, 24, 16
    full = tb.seeded_pix(seed, SB, B, NV, H, W)
    for s in range(SB):
        assert np.array_equal(full[s], tb.seeded_pix(seed, 1, B, NV, H, W, draw_offset=s * B)[0])
    v = tb.batch_index(seed, tb.STREAM_BATCH_VIEW, np.arange(1 << 16), NV)
    counts = np.bincount(v, minlength=NV)
    assert len(counts) == NV and float(((counts - 65536 / NV) ** 2 / (65536 / NV)).sum()) < 18.5      # chi-square, 4 dof, p = 0.001
    rs = np.random.RandomState(3)
    lo = rs.randint(0, 8, size=(SB, NV, 2))
    boxes = np.concatenate([lo, lo + rs.randint(0, 8, size=(SB, NV, 2))], -1).astype(np.float32)
    pix = tb.seeded_pix(seed, SB, B, NV, H, W, bboxes=boxes)
    box = boxes[np.arange(SB)[:, None], pix[..., 0]]
    assert bool(((pix[..., 2] >= box[..., 0]) & (pix[..., 2] <= box[..., 2]) & (pix[..., 1] >= box[..., 1]) & (pix[..., 1] <= box[..., 3])).all())
