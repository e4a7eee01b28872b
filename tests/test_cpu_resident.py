"""
The resident store without a GPU (include/pnyolo.h pny_resident_train_batch / pny_ingest_views_indexed, data.ResidentViews):

  * the kernels' own arithmetic (csrc/pny_resident.h compiled by g++ with pny_ingest.h and pny_train_batch.h under it, the way
    tests/test_cpu_ingest.py compiles its header) against the restatement (tests/resident_ref.py): the pixel every ray of a
    share picks, seeded and replayed, uniform and from boxes, with the object's own view count; the colour of that pixel under
    every resize; the clamps of ids, view counts, first rows and draws;
  * the C ABI: every listed refusal before any launch, with the argument named (the boundary itself: tests/test_cpu_abi.py);
  * Python: refusals by argument name; from_dataset on synthetic `srn` and `dvr` trees holds exactly the items' bytes and
    cameras and refuses an image that is no byte map; the tables with unequal view counts and after a later add; a store on
    the CPU refuses to draw.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from host_tools import CSRC, built_lib, header_code, header_text, host_header_program  # noqa: F401
import ingest_ref as ir
import resident_ref as rr
from pixel_nerf_yolo_amd import data as pdata
from pixel_nerf_yolo_amd import lib as plib

HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "pny_resident.h"
// one query per input line:
//   G h w c oh ow resize                 the store's geometry; forgets the objects
//   O nv has_boxes  + one line of nv*h*w*c bytes  (+ one line of nv*4 floats)      the next object
//   S obj max_views seed draw_index      a seeded ray      -> `obj view y x r g b` (clamped object; hex floats)
//   U obj max_views pix_ind              a replayed ray, uniform mode
//   B obj max_views image_id u_x u_y     a replayed ray, bbox mode
//   C v n | N n_views max_views | F first_row nv n_rows     the clamps
struct Obj {
    std::vector<uint8_t> bytes;
    std::vector<float> boxes;
    int nv;
};
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    std::istringstream in(text);
    std::string line;
    pny::ResidentGeom g;
    memset(&g, 0, sizeof g);
    std::vector<Obj> objs;
    while (std::getline(in, line)) {
        std::istringstream q(line);
        char kind;
        q >> kind;
        if (kind == 'G') {
            q >> g.h >> g.w >> g.c >> g.oh >> g.ow >> g.resize;
            g.scale_y = (float)g.h / (float)g.oh, g.scale_x = (float)g.w / (float)g.ow;
            objs.clear();
        } else if (kind == 'O') {
            Obj o;
            int has_boxes;
            q >> o.nv >> has_boxes;
            if (!std::getline(in, line)) return 3;
            std::istringstream b(line);
            o.bytes.resize((size_t)o.nv * g.h * g.w * g.c);
            for (size_t i = 0; i < o.bytes.size(); ++i) {
                int v;
                if (!(b >> v)) return 3;
                o.bytes[i] = (uint8_t)v;
            }
            if (has_boxes) {
                if (!std::getline(in, line)) return 3;
                std::istringstream bb(line);
                std::string tok;
                while (bb >> tok) o.boxes.push_back(strtof(tok.c_str(), 0));
                if ((int)o.boxes.size() != o.nv * 4) return 3;
            }
            objs.push_back(o);
        } else if (kind == 'S' || kind == 'U' || kind == 'B') {
            long long id;
            int max_views;
            q >> id >> max_views;
            const int obj = pny::resident_clamp(id, (int)objs.size());
            const Obj& o = objs[obj];
            const int nv = pny::resident_view_count(o.nv, max_views);
            const float* boxes = o.boxes.empty() ? 0 : o.boxes.data();
            pny::BatchPixel p;
            if (kind == 'S') {
                unsigned long long seed, di;
                q >> seed >> di;
                p = pny::resident_pick(nv, g.oh, g.ow, boxes, seed, di, 0, 0, 0, 0);
            } else if (kind == 'U') {
                long long flat;
                q >> flat;
                const int64_t fl = flat;
                p = pny::resident_pick(nv, g.oh, g.ow, 0, 0, 0, &fl, 0, 0, 0);
            } else {
                long long image;
                std::string sx, sy;
                q >> image >> sx >> sy;
                const int64_t im = image;
                const float ux = strtof(sx.c_str(), 0), uy = strtof(sy.c_str(), 0);
                p = pny::resident_pick(nv, g.oh, g.ow, boxes, 0, 0, 0, &im, &ux, &uy);
            }
            if (p.view < 0 || p.view >= o.nv || p.y < 0 || p.y >= g.oh || p.x < 0 || p.x >= g.ow) return 5;
            float rgb[3];
            pny::resident_rgb(o.bytes.data() + (size_t)p.view * g.h * g.w * g.c, g, p.y, p.x, pny::IngestLoadBytes(), rgb);
            printf("%d %d %d %d %a %a %a\n", obj, p.view, p.y, p.x, (double)rgb[0], (double)rgb[1], (double)rgb[2]);
        } else if (kind == 'C') {
            long long v;
            int n;
            q >> v >> n;
            printf("%d\n", pny::resident_clamp(v, n));
        } else if (kind == 'N') {
            int nv, mx;
            q >> nv >> mx;
            printf("%d\n", pny::resident_view_count(nv, mx));
        } else if (kind == 'F') {
            int first, nv;
            long long rows;
            q >> first >> nv >> rows;
            printf("%lld\n", (long long)pny::resident_first_row(first, nv, rows));
        } else {
            return 4;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    """csrc/pny_resident.h (pny_ingest.h, pny_train_batch.h and pny_rng.h under it) compiled by g++: an empty hip/hip_runtime.h,
    __host__ / __device__ defined away, no fused multiply-add -- the product's own code, run on lines of queries."""
    tmp = tmp_path_factory.mktemp("resident_host")
    (tmp / "hip").mkdir()
    (tmp / "hip" / "hip_runtime.h").write_text("")
    program = host_header_program(tmp, HOST_MAIN, defines=("__device__=", "__host__=", "__forceinline__=inline"),
                                  include_dirs=(tmp, CSRC))
    return lambda queries: [line.split() for line in program(queries)]


def store_queries(objs, resize, oh, ow, boxes=None):
    ch = objs[0]["u8"].shape[-1]
    q = ["G %d %d %d %d %d %d" % (rr.H, rr.W, ch, oh, ow, plib.RESIZE[resize])]
    for k, o in enumerate(objs):
        q.append("O %d %d" % (len(o["u8"]), int(boxes is not None)))
        q.append(" ".join(str(int(b)) for b in o["u8"].reshape(-1)))
        if boxes is not None:
            q.append(" ".join(float(v).hex() for v in boxes[k].reshape(-1)))
    return q


def check_rows(rows, want_obj, want_pix, objs, resize, oh, ow):
    """rows `obj view y x r g b` of the host-compiled header against the restatement: the pixel exactly, the colour to the
    restatement's bar -- and, where the ingest gives bytes, as exactly the map of a byte."""
    got = np.array([[int(v) for v in r[:4]] for r in rows])
    assert np.array_equal(got[:, 0], want_obj) and np.array_equal(got[:, 1:], want_pix), np.argwhere(got[:, 1:] != want_pix)[:5]
    rgb = np.array([[float.fromhex(v) for v in r[4:]] for r in rows])
    assert np.array_equal(rgb.astype(np.float32), rgb)                        # fp32 values
    table = ir.host_images(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, -1)).numpy()[0, 0].reshape(-1)
    cache = {}
    for (o, v, y, x), c in zip(got, rgb):
        if o not in cache:
            cache[o] = rr.ingest_f64(objs[o]["u8"], resize, oh, ow)
        ref, bar = cache[o]
        assert np.abs(c - (ref[v, :, y, x] * 0.5 + 0.5)).max() <= 0.5 * bar + 2.0 ** -24, (o, v, y, x)
        if resize == "none":
            want = ir.host_images(objs[o]["u8"][v:v + 1]).numpy()[0, :, y, x]
            assert np.array_equal(c.astype(np.float32), want * np.float32(0.5) + np.float32(0.5))
        elif resize == "bilinear_u8":
            assert np.isin(c.astype(np.float32), table * np.float32(0.5) + np.float32(0.5)).all()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("resize,size", rr.GEOMS)
def test_header_picks_the_one_object_batchs_pixels_and_the_ingests_colour(host_header, channels, resize, size):
    objs = rr.make_store(channels)
    oh, ow = size
    obj_ids, B, seed, off = [2, 0, 2, 1], 37, 2 ** 40 + 7, 1000
    mx = max(rr.VIEWS)
    for boxes in (None, rr.make_boxes(oh, ow)):
        q = store_queries(objs, resize, oh, ow, boxes)
        want_obj, want_pix = [], []
        for s, o in enumerate(obj_ids):
            q += ["S %d %d %d %d" % (o, mx, seed, off + s * B + r) for r in range(B)]
            want_obj += [o] * B
            want_pix.append(rr.share_pix(rr.VIEWS[o], oh, ow, B, None if boxes is None else boxes[o], seed=seed, draw_offset=off + s * B))
        rows = host_header(q)
        check_rows(rows, np.array(want_obj), np.concatenate(want_pix), objs, resize, oh, ow)
        views = {(r[0], r[1]) for r in rows}
        assert len(views) >= 6                                                  # the object's own view count enters the draws


def test_header_replays_and_clamps(host_header):
    objs = rr.make_store(3)
    resize, (oh, ow) = "area", (5, 7)
    boxes = rr.make_boxes(oh, ow)
    mx = max(rr.VIEWS)
    rs = np.random.RandomState(7)
    # uniform replay: in range, and outside the object's own grid (object 3 has ONE view: every index of another view is outside)
    flats = list(rs.randint(0, 5 * oh * ow, 40)) + [-1, -2 ** 40, 5 * oh * ow, 2 ** 40]
    q = store_queries(objs, resize, oh, ow)
    want_obj, want_pix = [], []
    for o in (1, 3, 0):
        q += ["U %d %d %d" % (o, mx, fl) for fl in flats]
        want_obj += [o] * len(flats)
        want_pix.append(rr.share_pix(rr.VIEWS[o], oh, ow, len(flats), draws={"pix_inds": np.array(flats)}))
    # out-of-range object ids land on the first and the last object; a record's view count is held to max_views
    q += ["U -5 %d 3" % mx, "U 99 %d 3" % mx, "U 1 2 %d" % (4 * oh * ow + 3)]
    rows = host_header(q)
    check_rows(rows[:-3], np.array(want_obj), np.concatenate(want_pix), objs, resize, oh, ow)
    assert [int(v) for v in rows[-3][:4]] == [0, 0, 0, 3] and [int(v) for v in rows[-2][:4]] == [3, 0, 0, 3]
    assert [int(v) for v in rows[-1][:4]] == [1, 1, oh - 1, ow - 1]              # 5 views held to 2: the grid's last pixel
    # bbox replay: image ids outside the views, uniforms outside [0, 1)
    ids = list(rs.randint(0, 5, 30)) + [-1, 5, 2 ** 40, 2, 3]
    ux = list(rs.rand(30).astype(np.float32)) + [0.5, 0.5, 0.5, -0.75, 7.5]
    uy = list(rs.rand(30).astype(np.float32)) + [0.25, 0.5, 0.5, 9.0, -3.0]
    q = store_queries(objs, resize, oh, ow, boxes)
    want_obj, want_pix = [], []
    for o in (1, 2):
        q += ["B %d %d %d %s %s" % (o, mx, i, float(x).hex(), float(y).hex()) for i, x, y in zip(ids, ux, uy)]
        want_obj += [o] * len(ids)
        want_pix.append(rr.share_pix(rr.VIEWS[o], oh, ow, len(ids), boxes[o],
                                     draws={"image_ids": np.array(ids), "u_x": np.array(ux, np.float32), "u_y": np.array(uy, np.float32)}))
    check_rows(host_header(q), np.array(want_obj), np.concatenate(want_pix), objs, resize, oh, ow)
    # the clamps themselves
    got = [int(r[0]) for r in host_header(["C -1 4", "C 0 4", "C 3 4", "C 4 4", "C %d 4" % 2 ** 40, "N 0 5", "N -3 5", "N 3 5", "N 9 5",
                                           "F -1 3 10", "F 0 3 10", "F 7 3 10", "F 8 3 10", "F 2147483647 1 10"])]
    assert got == [0, 0, 3, 3, 3, 1, 1, 3, 5, 0, 0, 7, 7, 9]


# --------------------------------------------------------------------------- C ABI
def test_entries_are_declared_and_cite_what_they_replace():
    """What is these entries' own (declared, bound, exported: tests/test_cpu_abi.py)."""
    code = header_code()
    assert re.search(r"\bint\s+pny_resident_train_batch\s*\(\s*const\s+pny_train_batch_desc\s*\*\s*desc\s*,", code)
    assert re.search(r"\bint\s+pny_ingest_views_indexed\s*\(\s*const\s+pny_ingest_desc\s*\*\s*desc\s*,\s*const\s+void\s*\*\s*objs_dev", code)
    hdr = header_text()
    block = hdr[hdr.index("---- resident views"):hdr.index("int pny_resident_train_batch")]
    assert "PixelNerfTrainer.py:76-133" in block and "SRNDataset.py:61-136" in block and "DVRDataset.py:110-275" in block
    for name in ("resident.hip", "resident_api.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert "PixelNerfTrainer.py:76-133" in text and "__getitem__" in text, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " resident.hip" in mk and " resident_api.hip" in mk and " pny_resident.h" in mk and " pny_ray.h" in mk
    assert re.search(r"#define\s+PNY_ABI_VERSION\s+11\b", code)                 # the change only adds functions


def test_train_batch_refuses_bad_arguments_before_any_launch(built_lib):
    """PNY_ERR_ARG (-1) naming the argument, whether or not a GPU is there (the device pointers are never dereferenced by the
    host)."""
    call, err = built_lib.pny_resident_train_batch, built_lib.pny_last_error
    ok = dict(n_objs=4, n_views=5, height=12, width=10, n_rays=37, z_near=0.5, z_far=2.0, focal_rows=0, focal_cols=0, c_rows=0,
              seed=1, draw_offset=0)
    p = C.c_void_p(4096)
    args = dict(channels=3, out_height=6, out_width=5, resize=2, objs=p, n_store=4, obj_ids=p, poses=p, n_rows=11, focal=p, c=None,
                boxes=None, draws=None, rays=p, rgb=p, pix=None)

    def rc(desc=True, **over):
        a = dict(args, **{k: v for k, v in over.items() if k in args})
        d = plib.TrainBatchDesc(**dict(ok, **{k: v for k, v in over.items() if k in ok}))
        return call(C.byref(d) if desc else None, a["channels"], a["out_height"], a["out_width"], a["resize"], a["objs"], a["n_store"],
                    a["obj_ids"], a["poses"], a["n_rows"], a["focal"], a["c"], a["boxes"], a["draws"], a["rays"], a["rgb"], a["pix"], None)

    assert rc(desc=False) == -1 and b"desc is null" in err()
    for missing, name in (("objs", b"objs_dev"), ("obj_ids", b"obj_ids_dev"), ("poses", b"poses_dev"), ("focal", b"focal_dev"),
                          ("rays", b"rays_dev"), ("rgb", b"rgb_gt_dev")):
        assert rc(**{missing: None}) == -1 and name + b" is null" in err(), missing
    for bad, name in ((dict(n_objs=0), b"desc.n_objs"), (dict(n_views=0), b"desc.n_views"), (dict(n_rays=-1), b"desc.n_rays"),
                      (dict(n_store=0), b"n_store_objs"), (dict(n_rows=0), b"n_rows"), (dict(height=0), b"height and width"),
                      (dict(width=-2), b"height and width"), (dict(out_height=0), b"out_height and out_width"),
                      (dict(out_width=-1), b"out_height and out_width")):
        assert rc(**bad) == -1 and name in err() and b"positive" in err(), bad
    for ch in (0, 1, 2, 5):
        assert rc(channels=ch) == -1 and b"channels must be 3 or 4" in err()
    assert rc(resize=3) == -1 and rc(resize=-1) == -1 and b"unknown resize" in err()
    assert rc(resize=0) == -1 and b"PNY_RESIZE_NONE needs out_height == height" in err()
    assert rc(resize=0, out_height=12, out_width=9) == -1 and b"PNY_RESIZE_NONE" in err()
    # an object's n_views * OH * OW at the draw's limit: 2^32 is refused, one view fewer is not the reason for a refusal
    assert rc(n_views=2 ** 16, out_height=2 ** 8, out_width=2 ** 8, resize=1) == -1 and b"desc.n_views * out_height * out_width" in err()
    assert b"2^32" in err()
    assert rc(n_objs=2 ** 16, n_rays=2 ** 15) == -1 and b"2^31 - 1 rays" in err()
    assert rc(height=2 ** 15, width=2 ** 15, resize=1) == -1 and b"2^31 bytes" in err()
    assert rc(out_height=2 ** 15, out_width=2 ** 15, resize=1) == -1 and b"2^31 elements" in err()
    assert rc(rays=C.c_void_p(4100)) == -1 and b"rays_dev must be 16-byte aligned" in err()
    assert rc(objs=C.c_void_p(4100)) == -1 and b"objs_dev must be 8-byte aligned" in err()
    empty = plib.TrainBatchDraws()
    assert rc(draws=C.byref(empty)) == -1 and b"pix_inds_dev" in err()
    only_pix = plib.TrainBatchDraws(pix_inds_dev=4096)
    assert rc(draws=C.byref(only_pix), boxes=p) == -1 and b"image_ids_dev" in err()


def test_indexed_ingest_refuses_bad_arguments_before_any_launch(built_lib):
    call, err = built_lib.pny_ingest_views_indexed, built_lib.pny_last_error
    ok = dict(n_views=7, height=12, width=10, channels=4, out_height=20, out_width=13, resize=1, white_mask=0)
    p = C.c_void_p(4096)
    args = dict(objs=p, n_store=4, max_views=5, obj_of=p, view_of=p, out=p)

    def rc(desc=True, **over):
        a = dict(args, **{k: v for k, v in over.items() if k in args})
        d = plib.IngestDesc(**dict(ok, **{k: v for k, v in over.items() if k in ok}))
        return call(C.byref(d) if desc else None, a["objs"], a["n_store"], a["max_views"], a["obj_of"], a["view_of"], a["out"], None)

    assert rc(desc=False) == -1 and b"desc is null" in err()
    for missing, name in (("objs", b"objs_dev"), ("obj_of", b"obj_of_dev"), ("view_of", b"view_of_dev"), ("out", b"out_dev")):
        assert rc(**{missing: None}) == -1 and name + b" is null" in err(), missing
    for bad, name in ((dict(n_views=0), b"desc.n_views"), (dict(n_store=-1), b"n_store_objs"), (dict(max_views=0), b"max_views"),
                      (dict(height=0), b"height and width"), (dict(width=0), b"height and width"),
                      (dict(out_height=-3), b"out_height and out_width"), (dict(out_width=0), b"out_height and out_width")):
        assert rc(**bad) == -1 and name in err() and b"positive" in err(), bad
    for ch in (0, 2, 5):
        assert rc(channels=ch) == -1 and b"channels must be 3 or 4" in err()
    assert rc(resize=7) == -1 and b"unknown resize" in err()
    assert rc(resize=0) == -1 and b"PNY_RESIZE_NONE" in err()
    assert rc(white_mask=1) == -1 and b"white_mask must be 0" in err()
    assert rc(max_views=2 ** 16, out_height=2 ** 8, out_width=2 ** 8) == -1 and b"max_views * out_height * out_width" in err()
    assert rc(n_views=2 ** 12, out_height=2 ** 10, out_width=2 ** 10) == -1 and b"2^31 output elements" in err()
    assert rc(objs=C.c_void_p(4097)) == -1 and b"8-byte aligned" in err()


# --------------------------------------------------------------------------- Python
def cpu_store(channels=3, boxes=False, **kw):
    objs = rr.make_store(channels)
    st = pdata.ResidentViews("cpu", **kw)
    for k, o in enumerate(objs):
        bb = rr.make_boxes(*(kw.get("size") or (rr.H, rr.W)))[k] if boxes else None
        assert st.add(o["u8"], o["poses"], o["focal"], c=o["c"], bbox=bb, labels="rows of %d" % k) == k
    return st, objs


def test_constructor_and_add_refuse_by_name():
    RV = pdata.ResidentViews
    with pytest.raises(ValueError, match="resize must be None, 'none', 'bilinear_u8' or 'area', got 'cubic'"):
        RV("cpu", size=(4, 4), resize="cubic")
    with pytest.raises(ValueError, match="scale and size are both given"):
        RV("cpu", size=(4, 4), scale=(0.5, 0.5))
    with pytest.raises(ValueError, match="scale goes with resize='bilinear_u8'.*got resize='area'"):
        RV("cpu", scale=(0.5, 0.5), resize="area")
    with pytest.raises(ValueError, match="scale must be a pair"):
        RV("cpu", scale=0.5)
    with pytest.raises(ValueError, match="size needs resize='area' or resize='bilinear_u8', got resize=None"):
        RV("cpu", size=(4, 4))
    with pytest.raises(ValueError, match="size must be positive"):
        RV("cpu", size=(0, 4), resize="area")
    with pytest.raises(ValueError, match=r"resize='area' needs size=\(OH, OW\)"):
        RV("cpu", resize="area")
    with pytest.raises(ValueError, match="white_bbox goes with resize='area' or no resize"):
        RV("cpu", scale=(0.5, 0.5), white_bbox=True)
    st = RV("cpu", size=(6, 5), resize="area")
    u8, poses = np.zeros((2, 12, 10, 3), np.uint8), np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    with pytest.raises(TypeError, match="images_u8 must be a tensor or an array"):
        st.add([[1]], poses, 10.0)
    with pytest.raises(ValueError, match=r"images_u8 must be \(NV, H, W, C\) uint8 with C = 3 or 4, got \(2, 12, 10, 3\) torch.float32"):
        st.add(u8.astype(np.float32), poses, 10.0)
    with pytest.raises(ValueError, match=r"images_u8 must be .*got \(2, 3, 12, 10\)"):
        st.add(np.zeros((2, 3, 12, 10), np.uint8), poses, 10.0)                  # NCHW bytes
    with pytest.raises(ValueError, match=r"poses must be \(2, 4, 4\), got \(3, 4, 4\)"):
        st.add(u8, np.zeros((3, 4, 4), np.float32), 10.0)
    with pytest.raises(ValueError, match="focal must be a scalar or"):
        st.add(u8, poses, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="c must be None or"):
        st.add(u8, poses, 10.0, c=[1.0])
    with pytest.raises(ValueError, match=r"bbox must be \(2, 4\)"):
        st.add(u8, poses, 10.0, bbox=np.zeros((3, 4)))
    assert len(st) == 0 and st.add(u8, poses, 10.0) == 0
    with pytest.raises(ValueError, match=r"images_u8 is \(H, W, C\) = \(12, 10, 4\); the store holds \(12, 10, 3\)"):
        st.add(np.zeros((1, 12, 10, 4), np.uint8), poses[:1], 10.0)
    with pytest.raises(ValueError, match="bbox is given, the objects of the store have no boxes: all or none"):
        st.add(u8, poses, 10.0, bbox=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="the store computes its own"):
        pdata.ResidentViews("cpu", white_bbox=True).add(u8, poses, 10.0, bbox=np.zeros((2, 4)))
    with pytest.raises(plib.PnyError, match="images_u8 is on cpu"):              # the boxes are made by the device ingest
        pdata.ResidentViews("cpu", white_bbox=True).add(u8, poses, 10.0)


def test_tables_with_unequal_view_counts_and_objects_added_later():
    st, objs = cpu_store(4, boxes=True, size=(5, 7), resize="area")
    assert len(st) == 4 and [st.n_views(k) for k in range(4)] == list(rr.VIEWS) and st.decoded == (12, 10, 4) and st.out_size == (5, 7)
    assert st.labels(2) == "rows of 2"
    t = st.tables()
    assert st.tables() is t                                                      # built once
    rec = t["objs"].numpy().view(np.dtype([("views", np.uint64), ("n_views", np.int32), ("first_row", np.int32)])).reshape(-1)
    assert t["objs"].dtype == torch.uint8 and tuple(t["objs"].shape) == (4, 16)
    assert rec["n_views"].tolist() == [2, 5, 3, 1] and rec["first_row"].tolist() == [0, 2, 7, 10]
    assert rec["views"].tolist() == [v.data_ptr() for v in st._views]
    assert t["n_views"].tolist() == [2, 5, 3, 1] and t["first_row"].tolist() == [0, 2, 7, 10] and t["max_views"] == 5 and t["n_rows"] == 11
    assert torch.equal(t["poses"], torch.from_numpy(np.concatenate([o["poses"] for o in objs])))
    assert torch.equal(t["bboxes"], torch.from_numpy(np.concatenate(rr.make_boxes(5, 7))))
    assert torch.equal(t["focal"], torch.from_numpy(np.stack([o["focal"] for o in objs])))
    assert torch.equal(t["c"], torch.from_numpy(np.stack([o["c"] for o in objs])))
    for k, o in enumerate(objs):
        assert st._views[k].dtype == torch.uint8 and np.array_equal(st._views[k].numpy(), o["u8"])
    views_bytes = sum(o["u8"].size for o in objs)
    assert views_bytes < st.nbytes < views_bytes + 11 * (64 + 16) + 4 * 64
    # an object added after the first tables: FRESH tensors, the old ones untouched (launches in flight keep theirs)
    old = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in t.items()}
    six = np.zeros((6, 12, 10, 4), np.uint8)
    assert st.add(six, np.tile(np.eye(4, dtype=np.float32), (6, 1, 1)), 3.0, bbox=np.tile(np.float32([0, 0, 6, 4]), (6, 1))) == 4
    t2 = st.tables()
    assert t2 is not t and t2["objs"].data_ptr() != t["objs"].data_ptr() and t2["poses"].data_ptr() != t["poses"].data_ptr()
    for k, v in old.items():
        assert torch.equal(t[k], v) if isinstance(v, torch.Tensor) else t[k] == v
    assert t2["n_views"].tolist() == [2, 5, 3, 1, 6] and t2["first_row"].tolist() == [0, 2, 7, 10, 11] and t2["max_views"] == 6
    assert t2["focal"][4].tolist() == [3.0, 3.0] and t2["c"][4].tolist() == [3.5, 2.5]      # a scalar focal; c None: (OW / 2, OH / 2)
    assert torch.equal(t2["poses"][:11], t["poses"])


def test_ids_are_validated_on_the_host_and_a_cpu_store_refuses_to_draw():
    st, _ = cpu_store(3)
    kw = dict(ray_batch_size=8, z_near=0.5, z_far=2.0, seed=1)
    with pytest.raises(ValueError, match="obj_ids holds 4; the store has 4 objects"):
        st.batch([0, 4], [[0], [0]], **kw)
    with pytest.raises(ValueError, match="obj_ids holds -1"):
        st.batch([-1], [[0]], **kw)
    with pytest.raises(ValueError, match="obj_ids must be 1-dimensional"):
        st.batch([[0, 1]], [[0], [0]], **kw)
    with pytest.raises(ValueError, match="obj_ids must be .* of integers"):
        st.batch([0.5], [[0]], **kw)
    with pytest.raises(ValueError, match=r"src_view_ids\[1\]\[0\] = 2; object 0 has 2 views"):
        st.batch([2, 0], [[2], [2]], **kw)
    with pytest.raises(ValueError, match=r"src_view_ids\[0\]\[1\] = 1; object 3 has 1 view$"):
        st.batch([3], [[0, 1]], **kw)
    with pytest.raises(ValueError, match=r"src_view_ids must be \(2, NS\)"):
        st.batch([2, 0], [[0]], **kw)
    with pytest.raises(ValueError, match="ray_batch_size must be positive"):
        st.batch([0], [[0]], **dict(kw, ray_batch_size=0))
    with pytest.raises(ValueError, match="seed has no effect"):
        st.batch([0], [[0]], draws={"pix_inds": np.zeros((1, 8), np.int64)}, **kw)
    with pytest.raises(ValueError, match=r"view_ids\[0\]\[0\] = 5; object 1 has 5 views"):
        st.source_views(1, [5, 0])
    with pytest.raises(plib.PnyError, match=r"ResidentViews.batch: the store is on cpu.*MI355X only"):
        st.batch([2, 0, 2, 1], [[0], [1], [2], [4]], **kw)
    with pytest.raises(plib.PnyError, match=r"ResidentViews.source_views: the store is on cpu"):
        st.source_views([1, 1], [[4, 0], [0, 0]])
    with pytest.raises(ValueError, match="the store is empty"):
        pdata.ResidentViews("cpu").tables()


def test_epoch_is_a_seeded_permutation_in_batches():
    st, _ = cpu_store(3)
    for k in range(3):
        st.add(np.zeros((1, 12, 10, 3), np.uint8), np.eye(4, dtype=np.float32)[None], 1.0, c=[1.0, 1.0])
    a, b = list(st.epoch(2, seed=5)), list(st.epoch(2, seed=5))
    assert a == b and len(a) == 3 and all(len(ids) == 2 for ids in a)            # 7 objects: the last one dropped
    full = list(st.epoch(2, seed=5, drop_last=False))
    assert full[:3] == a and sorted(i for ids in full for i in ids) == list(range(7))
    assert list(st.epoch(2, seed=5, epoch=1)) != a and list(st.epoch(2, seed=6)) != a
    assert all(isinstance(i, int) for ids in a for i in ids)


# --------------------------------------------------------------------------- datasets
def test_from_dataset_on_an_srn_tree_holds_the_items_bytes_and_cameras(tmp_path):
    from test_cpu_data import _srn_tree
    path, truth = _srn_tree(str(tmp_path), "val")
    for size, resize in (((16, 16), "none"), ((8, 8), "area")):
        ds = pdata.get_split_dataset("srn", path, want_split="val", training=False, image_size=size, ingest_on_device=True)
        st = pdata.ResidentViews.from_dataset(ds, "cpu", white_bbox=False)
        assert len(st) == 2 and st.resize == resize and st.out_size == size and st.decoded == (16, 16, 3) and not st.white_bbox
        t = st.tables()
        for k in range(2):
            it = ds[k]
            assert np.array_equal(st._views[k].numpy(), truth[k][1]) and torch.equal(st._views[k], it["images_u8"])
            assert torch.equal(t["poses"][3 * k:3 * k + 3], it["poses"])
            assert t["focal"][k].tolist() == [float(it["focal"])] * 2 and torch.equal(t["c"][k], it["c"])
        assert t["bboxes"] is None
        one = pdata.ResidentViews.from_dataset(ds, "cpu", indices=[1], white_bbox=False)
        assert len(one) == 1 and torch.equal(one._views[0], ds[1]["images_u8"])
    with pytest.raises(plib.PnyError, match="images_u8 is on cpu"):              # SRN's boxes by default: the device ingest
        pdata.ResidentViews.from_dataset(ds, "cpu")


def test_from_dataset_on_a_yolo_tree_keeps_the_scale_and_the_label_rows(tmp_path):
    import warnings
    from test_cpu_ingest import _yolo_tree
    root = str(tmp_path)
    conf, imgs, rows = _yolo_tree(root, "train")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # np.loadtxt on the empty label file of view 1
        ds = pdata.get_split_dataset("yolo", root, want_split="train", conf=conf, ingest_on_device=True, jitter_on_device=True)
        st = pdata.ResidentViews.from_dataset(ds, "cpu")      # the deferred jitter's factors are the trainer's, not the store's
        it = ds[0]
    assert len(st) == 1 and st.resize == "bilinear_u8" and st.decoded == (27, 48, 3) and st.out_size == (13, 24) and not st.white_bbox
    assert np.array_equal(st._views[0].numpy(), imgs) and st.tables()["bboxes"] is None
    labels, n_labels = st.labels(0)
    assert torch.equal(labels, it["labels"]) and n_labels.tolist() == [3, 0, 1]
    assert torch.equal(st.tables()["focal"][0], it["focal"]) and torch.equal(st.tables()["c"][0], it["c"])
    assert torch.equal(st.tables()["poses"], it["poses"])


def test_from_dataset_requantises_dvr_items_and_refuses_a_non_byte_image(tmp_path):
    from test_cpu_data import _dvr_tree
    root, obj, truth = _dvr_tree(str(tmp_path / "shapenet"), "shapenet")
    ds = pdata.get_split_dataset("dvr", root, want_split="val", training=False)
    it = ds[0]
    st = pdata.ResidentViews.from_dataset(ds, "cpu")
    assert len(st) == 1 and st.resize == "none" and st.decoded == (12, 16, 3) and st.out_size == (12, 16)
    assert np.array_equal(st._views[0].numpy(), np.stack([t[0] for t in truth]))
    assert torch.equal(ir.host_images(st._views[0].numpy()), it["images"])       # the same fp32 bits through the byte map
    t = st.tables()
    assert torch.equal(t["poses"], it["poses"]) and torch.equal(t["bboxes"], it["bbox"])
    assert t["focal"][0].tolist() == [float(np.float32(it["focal"]))] * 2 and t["c"][0].tolist() == [8.0, 6.0]
    root2, _, truth2 = _dvr_tree(str(tmp_path / "dtu"), "dtu")
    dtu = pdata.get_split_dataset("dvr_dtu", root2, want_split="val", training=False)
    sd = pdata.ResidentViews.from_dataset(dtu, "cpu")
    assert np.array_equal(sd._views[0].numpy(), np.stack([t[0] for t in truth2])) and sd.tables()["bboxes"] is None
    assert torch.equal(sd.tables()["focal"][0], dtu[0]["focal"]) and torch.equal(sd.tables()["c"][0], dtu[0]["c"])
    # an area-resized item is no byte map: refused by view
    small = pdata.DVRDataset(root, stage="val", image_size=(6, 8))
    with pytest.raises(ValueError, match=r"item 0 \(.*obj0\): images\[0\] is not the byte map of 8-bit pixels"):
        pdata.ResidentViews.from_dataset(small, "cpu")

    class Off(torch.utils.data.Dataset):
        def __len__(self):
            return 1

        def __getitem__(self, i):
            item = dict(it)
            item["images"] = it["images"].clone()
            item["images"][2, 1, 3, 4] += 2.0 ** -20
            return item

    with pytest.raises(ValueError, match=r"images\[2\] is not the byte map"):
        pdata.ResidentViews.from_dataset(Off(), "cpu")
