"""
The resident store on the device (data.ResidentViews over pny_resident_train_batch / pny_ingest_views_indexed), held to the
path it stands in for, bit for bit: a share of a batch is ``util.sample_train_batch`` of ONE object on
``augment.ingest_views`` of that object's views with ``draw_offset = s * B``; the source views are ``augment.ingest_views``
of the gathered bytes (and ``augment.color_jitter`` of that).

The store: four objects of 2, 5, 3 and 1 views of 12 x 10 (tests/resident_ref.py), C = 3 and 4, random bytes with 255s and
exact bilinear ties; no resize, area to 6 x 5 and 5 x 7, bilinear_u8 to 7 x 9 and 20 x 13.  B = 37 (one workgroup, not a
multiple of the wave) and 300 (a second workgroup for share 3 alone, shares straddling workgroups).
"""
import functools
import time

import numpy as np
import pytest
import torch

import resident_ref as rr
from helpers import DEV
from pixel_nerf_yolo_amd import augment as paug
from pixel_nerf_yolo_amd import data as pdata
from pixel_nerf_yolo_amd import util as putil

pytestmark = pytest.mark.gpu

OBJ_IDS = [2, 0, 2, 1]
Z_NEAR, Z_FAR = 0.8, 1.8
SEED, OFFSET = 2 ** 40 + 7, 1000
SPIN_CYCLES = 100_000_000                   # torch.cuda._sleep: about 50 ms of one wave spinning on the clock


def store_kw(resize, size):
    return {} if resize == "none" else dict(size=size, resize=resize)


@functools.lru_cache(maxsize=None)
def store(channels, geom, boxes):
    """The tests' store on the device, its host objects, its boxes, and per object the parent path's ingest of its views."""
    resize, size = rr.GEOMS[geom]
    objs = rr.make_store(channels)
    bb = rr.make_boxes(*size) if boxes else None
    st = pdata.ResidentViews(DEV, **store_kw(resize, size))
    for k, o in enumerate(objs):
        st.add(o["u8"], o["poses"], o["focal"], c=o["c"], bbox=None if bb is None else bb[k])
    ingested = [paug.ingest_views(torch.from_numpy(o["u8"]).to(DEV), **store_kw(resize, size)) for o in objs]
    return st, objs, bb, ingested


def parent_share(objs, bb, ingested, o, B, **kw):
    """Share of object o by the parent path: a one-object sample_train_batch on the ingest of its views."""
    ob = objs[o]
    return putil.sample_train_batch(ingested[o][None], torch.from_numpy(ob["poses"])[None], torch.from_numpy(ob["focal"])[None],
                                    Z_NEAR, Z_FAR, B, c=torch.from_numpy(ob["c"])[None],
                                    bboxes=None if bb is None else torch.from_numpy(bb[o])[None], **kw)


def replay_draws(bb, size, B, seed):
    """(SB, B) draws of every share, inside its object's range, with a handful outside it."""
    rs = np.random.RandomState(seed)
    oh, ow = size
    nv = np.array([rr.VIEWS[o] for o in OBJ_IDS])[:, None]
    if bb is None:
        d = {"pix_inds": (rs.randint(0, 2 ** 31, size=(4, B)) % (nv * oh * ow)).astype(np.int64)}
        d["pix_inds"][:, :4] = [-1, -2 ** 40, 5 * oh * ow, 2 ** 40]
        return d
    d = {"image_ids": (rs.randint(0, 2 ** 31, size=(4, B)) % nv).astype(np.int64), "u_x": rs.rand(4, B).astype(np.float32),
         "u_y": rs.rand(4, B).astype(np.float32)}
    d["image_ids"][:, :3] = [-1, 5, 2 ** 40]
    d["u_x"][:, 3:5], d["u_y"][:, 3:5] = [-0.75, 7.5], [9.0, -3.0]
    return d


# --------------------------------------------------------------------------- the ray batch
@pytest.mark.parametrize("boxes", [False, True], ids=["uniform", "bbox"])
@pytest.mark.parametrize("geom", range(len(rr.GEOMS)), ids=["%s_%dx%d" % (r, s[0], s[1]) for r, s in rr.GEOMS])
@pytest.mark.parametrize("channels", [3, 4])
def test_ray_batch_is_the_one_object_batch_on_the_ingested_views(channels, geom, boxes):
    st, objs, bb, ingested = store(channels, geom, boxes)
    size = rr.GEOMS[geom][1]
    for B in (37, 300):
        for replay in (False, True):
            draws = replay_draws(bb, size, B, seed=B) if replay else None
            got = st.batch(OBJ_IDS, None, B, Z_NEAR, Z_FAR, seed=None if replay else SEED, draws=draws,
                           draw_offset=0 if replay else OFFSET)
            assert got["src_images"] is None and got["src_poses"] is None
            assert tuple(got["rays"].shape) == (4, B, 8) and tuple(got["rgb_gt"].shape) == (4, B, 3)
            assert tuple(got["pix"].shape) == (4, B, 3) and got["pix"].dtype == torch.int32
            views = set()
            for s, o in enumerate(OBJ_IDS):
                kw = dict(draws={k: v[s:s + 1] for k, v in draws.items()}) if replay else dict(seed=SEED, draw_offset=OFFSET + s * B)
                rays, rgb, pix = parent_share(objs, bb, ingested, o, B, **kw)
                what = (channels, rr.GEOMS[geom], boxes, B, replay, s)
                assert torch.equal(got["pix"][s], pix[0]), what
                assert torch.equal(got["rays"][s], rays[0]), what
                assert torch.equal(got["rgb_gt"][s], rgb[0]), what
                assert int(pix[0, :, 0].max()) < rr.VIEWS[o]
                views |= {(o, int(v)) for v in pix[0, :, 0].unique()}
                want_pix = rr.share_pix(rr.VIEWS[o], size[0], size[1], B, None if bb is None else bb[o],
                                        **({"draws": {k: v[s] for k, v in draws.items()}} if replay else
                                           {"seed": SEED, "draw_offset": OFFSET + s * B}))
                assert np.array_equal(pix[0].cpu().numpy(), want_pix), what          # and both are the restatement's pixels
            if B == 300:
                assert len(views) == 2 + 5 + 3                                       # every view of every drawn object
            if boxes and not replay:
                box = torch.from_numpy(bb[1])[got["pix"][3, :, 0].cpu().long()]
                p = got["pix"][3].cpu().float()
                assert bool(((p[:, 2] >= box[:, 0]) & (p[:, 2] <= box[:, 2]) & (p[:, 1] >= box[:, 1]) & (p[:, 1] <= box[:, 3])).all())
                assert bool((p[got["pix"][3, :, 0].cpu() == 0][:, 1:] == torch.tensor([2.0, 3.0])).all())   # the one-pixel box
            assert torch.equal(got["focal"].cpu(), torch.from_numpy(np.stack([objs[o]["focal"] for o in OBJ_IDS])))
            assert torch.equal(got["c"].cpu(), torch.from_numpy(np.stack([objs[o]["c"] for o in OBJ_IDS])))


def test_rgb_gt_is_the_restatements_value_at_the_sampled_pixel():
    """The parent path is the bar above; this holds both to the float64 restatement, so that a shared mistake shows."""
    for geom, (resize, size) in enumerate(rr.GEOMS):
        st, objs, _, _ = store(3, geom, False)
        got = st.batch(OBJ_IDS, None, 300, Z_NEAR, Z_FAR, seed=SEED)
        pix, rgb = got["pix"].cpu().numpy(), got["rgb_gt"].cpu().numpy().astype(np.float64)
        for s, o in enumerate(OBJ_IDS):
            ref, bar = rr.ingest_f64(objs[o]["u8"], resize, *size)
            want = ref[pix[s, :, 0], :, pix[s, :, 1], pix[s, :, 2]] * 0.5 + 0.5
            err = np.abs(rgb[s] - want).max()
            print("rgb_gt %s %s share %d: max error %.3g against the restatement, bar %.3g" % (resize, size, s, err, 0.5 * bar + 2.0 ** -24))
            assert err <= 0.5 * bar + 2.0 ** -24


# --------------------------------------------------------------------------- the source views
SRC_LISTS = ([(1, 4)], [(1, 4), (2, 0), (1, 4), (0, 1), (3, 0), (1, 0), (2, 2)])       # (object, view): repeated, out of order


@pytest.mark.parametrize("geom", range(len(rr.GEOMS)), ids=["%s_%dx%d" % (r, s[0], s[1]) for r, s in rr.GEOMS])
@pytest.mark.parametrize("channels", [3, 4])
def test_source_views_are_the_ingest_of_the_gathered_bytes(channels, geom):
    st, objs, _, _ = store(channels, geom, False)
    resize, size = rr.GEOMS[geom]
    rs = np.random.RandomState(5)
    for pairs in SRC_LISTS:
        obj_of, view_of = [p[0] for p in pairs], [p[1] for p in pairs]
        want = paug.ingest_views(torch.from_numpy(rr.gather(objs, obj_of, view_of)).to(DEV), **store_kw(resize, size))
        got = st.source_views(obj_of, [[v] for v in view_of])
        assert tuple(got.shape) == (len(pairs), 1, 3) + size and torch.equal(got[:, 0], want)
        factors = np.stack([rs.uniform(-0.1, 0.1, len(pairs)), rs.uniform(0.9, 1.1, len(pairs)), rs.uniform(0.9, 1.1, len(pairs)),
                            rs.uniform(0.9, 1.1, len(pairs))], -1).astype(np.float32)
        jit = st.source_views(obj_of, [[v] for v in view_of], jitter=factors)
        assert torch.equal(jit, paug.color_jitter(want[:, None].contiguous(), factors)) and not torch.equal(jit, got)
    # several views per object, and ONE object given as an int
    got = st.source_views([1, 2], [[4, 0, 4], [2, 2, 1]])
    want = paug.ingest_views(torch.from_numpy(rr.gather(objs, [1, 1, 1, 2, 2, 2], [4, 0, 4, 2, 2, 1])).to(DEV), **store_kw(resize, size))
    assert torch.equal(got.reshape(6, 3, *size), want)
    assert torch.equal(st.source_views(1, [4, 0, 4]), got[0])


def test_batch_hands_back_the_source_views_and_their_cameras():
    st, objs, bb, _ = store(4, 2, True)
    src = [[2, 0], [1, 1], [0, 2], [4, 3]]
    factors = np.tile(np.float32([0.05, 1.1, 0.9, 1.05]), (4, 1))
    got = st.batch(OBJ_IDS, src, 37, Z_NEAR, Z_FAR, seed=SEED, jitter=factors)
    plain = st.batch(OBJ_IDS, src, 37, Z_NEAR, Z_FAR, seed=SEED)
    flat_o, flat_v = [o for o, vs in zip(OBJ_IDS, src) for _ in vs], [v for vs in src for v in vs]
    want = paug.ingest_views(torch.from_numpy(rr.gather(objs, flat_o, flat_v)).to(DEV), size=(5, 7), resize="area").reshape(4, 2, 3, 5, 7)
    assert torch.equal(plain["src_images"], want) and torch.equal(got["src_images"], paug.color_jitter(want, factors))
    assert torch.equal(got["src_poses"].cpu(), torch.from_numpy(np.stack([objs[o]["poses"][vs] for o, vs in zip(OBJ_IDS, src)])))
    for k in ("rays", "rgb_gt", "pix", "focal", "c", "src_poses"):
        assert torch.equal(got[k], plain[k]), k                                      # the jitter touches the source views only


# --------------------------------------------------------------------------- clamping
def test_out_of_range_device_ids_are_clamped_into_the_store():
    """Ids that only the device sees cannot be refused; they must land on the store's own objects and views.  Shown through
    values: every output equals that of the clamped ids, so nothing outside the store was read."""
    for boxes in (False, True):
        st, _, _, _ = store(3, 1, boxes)
        bad_o = torch.tensor([-3, 9, 1, 2 ** 31 - 1], dtype=torch.int64, device=DEV)
        bad_v = torch.tensor([[-1, 7], [0, 1], [5, 2 ** 31 - 1], [-2 ** 31, 0]], dtype=torch.int64, device=DEV)
        got = st.batch(bad_o, bad_v, 37, Z_NEAR, Z_FAR, seed=SEED)
        want = st.batch([0, 3, 1, 3], [[0, 1], [0, 0], [4, 4], [0, 0]], 37, Z_NEAR, Z_FAR, seed=SEED)
        for k in want:
            assert torch.equal(got[k], want[k]), (boxes, k)
        assert torch.equal(st.source_views(bad_o.to(torch.int32), bad_v.to(torch.int32)), want["src_images"])


# --------------------------------------------------------------------------- determinism, no wait
def test_two_runs_give_the_same_bits_and_objects_added_later_join_the_store():
    st, objs, bb, _ = store(4, 4, True)
    src = [[2, 0], [1, 1], [0, 2], [4, 3]]
    a = st.batch(OBJ_IDS, src, 300, Z_NEAR, Z_FAR, seed=SEED)
    b = st.batch(OBJ_IDS, src, 300, Z_NEAR, Z_FAR, seed=SEED)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["pix"], st.batch(OBJ_IDS, src, 300, Z_NEAR, Z_FAR, seed=SEED + 1)["pix"])
    # a store of its own (the cached one stays as it is): a fifth object after a first batch
    resize, size = rr.GEOMS[4]
    mine = pdata.ResidentViews(DEV, size=size, resize=resize)
    for k, o in enumerate(objs):
        mine.add(o["u8"], o["poses"], o["focal"], c=o["c"], bbox=bb[k])
    first = mine.batch(OBJ_IDS, src, 37, Z_NEAR, Z_FAR, seed=SEED)
    assert mine.add(objs[1]["u8"][::-1].copy(), objs[1]["poses"][::-1].copy(), objs[1]["focal"], c=objs[1]["c"], bbox=bb[1][::-1].copy()) == 4
    again = mine.batch(OBJ_IDS + [4], src + [[0, 4]], 37, Z_NEAR, Z_FAR, seed=SEED)
    for k in first:
        assert torch.equal(again[k][:4], first[k]), k
    assert torch.equal(again["src_images"][4, 0], again["src_images"][3, 0])         # view 0 of the reversed copy is view 4 of object 1
    assert mine.nbytes > st.nbytes and len(mine) == 5


def test_srn_boxes_are_made_at_fill_time_and_an_empty_mask_is_refused():
    objs = rr.make_store(3)
    st = pdata.ResidentViews(DEV, size=(6, 5), resize="area", white_bbox=True)
    for o in objs:
        st.add(torch.from_numpy(o["u8"]).to(DEV), o["poses"], o["focal"], c=o["c"])      # device bytes are taken as they are
    want = torch.cat([paug.ingest_views(torch.from_numpy(o["u8"]).to(DEV), size=(6, 5), resize="area", white_mask=True)[2] for o in objs])
    assert torch.equal(st.tables()["bboxes"], want)
    white = objs[1]["u8"].copy()
    white[3, :, :, 1] = 255
    with pytest.raises(ValueError, match=r"images_u8\[3\] has an empty white-background mask"):
        st.add(white, objs[1]["poses"], objs[1]["focal"])
    assert len(st) == 4


def test_batch_returns_while_a_spin_holds_its_stream():
    """The device of tests/test_gpu_streams.py, restated: a timed spin on the stream, the batch enqueued behind it, and the spin's
    event still pending when the batch has returned -- a call that waited for the device would have outlasted the spin.  The spin
    ends by itself."""
    st, _, _, _ = store(3, 2, True)
    src = [[1, 0], [1, 0], [0, 2], [4, 3]]
    factors = np.tile(np.float32([0.05, 1.1, 0.9, 1.05]), (4, 1))
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        warm = st.batch(OBJ_IDS, src, 300, Z_NEAR, Z_FAR, seed=SEED, jitter=factors)      # code objects, tables, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SPIN_CYCLES)
        event = torch.cuda.Event()
        event.record(side)
        got = st.batch(OBJ_IDS, src, 300, Z_NEAR, Z_FAR, seed=SEED, jitter=factors)
    pending = not event.query()
    host_ms = 1e3 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    print("batch enqueued in %.2f ms of host time, inside a spin of %d cycles" % (host_ms, SPIN_CYCLES))
    assert pending, "the spin had ended when batch returned (host time %.2f ms): the call waited for the device" % host_ms
    for k in warm:
        assert torch.equal(got[k], warm[k]), k
