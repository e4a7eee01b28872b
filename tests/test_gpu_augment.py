"""
The colour jitter on the GPU (csrc/augment.hip, include/pnyolo.h pny_color_jitter, augment.color_jitter) against the fp64
restatement of the chain (tests/augment_ref.py):
  * the chain in both input formats at (NV, H, W) = (1, 1, 1) the smallest image, (3, 1, 7) a single row, (2, 5, 7) an odd byte
    stride of 105, (2, 31, 33) / (1, 32, 32) / (1, 25, 41) = 1023 / 1024 / 1025 pixels around the workgroup's 1024 threads,
    (3, 37, 53) odd sizes, (2, 128, 128) a training size; one object and three objects with factors of their own; the factors
    (0, 1, 1, 1), (0.5, 0, 3, 0), (-0.5, 2, 0.5, 2), the eight corners of the reference's ranges and random draws inside them;
    random inputs with planted black, white, grey and primary pixels (exact -1 and 1 in the float format); nothing filtered;
  * a float tensor one element and a byte tensor one byte into a larger buffer: inside the bar, and the same bits as aligned;
  * bitwise: in place, run to run, an image in a batch against the image alone, view selection before or after;
  * a non-default stream; 65 objects (two launches) against per-object calls; a deferred ColorJitterDataset end to end.

The bar (tests/augment_ref.py `bar`), in output units [-1, 1]: max(4 e_host, 64 * 2^-24), e_host being the worst difference of
the project's host fp32 chain (data.adjust_*; bytes through image_to_tensor_balanced first) from the restatement on the very
inputs of the case.  Its reasons are in tests/test_cpu_augment.py.
"""
import itertools

import numpy as np
import pytest
import torch

import augment_ref as ar
from helpers import DEV
from pixel_nerf_yolo_amd import augment as paug
from pixel_nerf_yolo_amd import data as pdata

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 1, 7), (2, 5, 7), (2, 31, 33), (1, 32, 32), (1, 25, 41), (3, 37, 53), (2, 128, 128)]
FIXED = [(0, 1, 1, 1), (0.5, 0, 3, 0), (-0.5, 2, 0.5, 2)]
CORNERS = [(h, s, b, c) for h in (-0.1, 0.1) for s, b, c in itertools.product((0.9, 1.1), repeat=3)]
# black, white, grey, the primaries and secondaries, as bytes
PLANTED = np.array([(0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255),
                    (255, 0, 255)], np.uint8)


def factor_sets(seed, n_random=5):
    rs = np.random.RandomState(seed)
    rand = [(rs.uniform(-0.1, 0.1), rs.uniform(0.9, 1.1), rs.uniform(0.9, 1.1), rs.uniform(0.9, 1.1)) for _ in range(n_random)]
    return np.array(FIXED + CORNERS + rand, np.float32)              # 24 sets: eight groups of three objects


def make_images(seed, fmt, lead, h, w):
    """Random images of `lead` + (3, H, W) floats in [-1, 1] or `lead` + (H, W, 3) bytes; image j carries the planted pixels,
    rotated by j, at its first pixels (as many as it has)."""
    rs = np.random.RandomState(seed)
    n_img = int(np.prod(lead))
    u8 = rs.randint(0, 256, size=(n_img, h * w, 3)).astype(np.uint8)
    f32 = rs.uniform(-1, 1, size=(n_img, h * w, 3)).astype(np.float32)
    for j in range(n_img):
        for p in range(min(len(PLANTED), h * w)):
            u8[j, p] = PLANTED[(p + j) % len(PLANTED)]
            f32[j, p] = np.where(PLANTED[(p + j) % len(PLANTED)] == 128, 0.0, PLANTED[(p + j) % len(PLANTED)] / 127.5 - 1.0)
    if fmt == "bytes":
        return u8.reshape(tuple(lead) + (h, w, 3))
    assert h * w < 2 or (f32.min() == -1.0 and f32.max() == 1.0)
    return np.ascontiguousarray(np.moveaxis(f32.reshape(tuple(lead) + (h, w, 3)), -1, -3))


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_against_restatement(got, images, factors, what, ref=None, host=None):
    """Prints each figure before it asserts; returns (error, e_host).  `ref` and `host`: the restatement and the host chain on
    these inputs where the caller already has them."""
    ref = ar.jitter(images, factors) if ref is None else ref
    host = ar.host_chain(images, factors) if host is None else host
    e_host = float(np.abs(host.astype(np.float64) - ref).max())
    bar = max(4.0 * e_host, ar.FLOOR)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s %s: kernel %.3g, host chain %.3g, bar %.3g" % (what, images.shape, err, e_host, bar))
    assert np.isfinite(got).all() and got.min() >= -1.0 and got.max() <= 1.0
    assert err <= bar
    return err, e_host


@pytest.mark.parametrize("fmt", ["float", "bytes"])
@pytest.mark.parametrize("nv,h,w", SHAPES)
def test_chain_against_fp64(nv, h, w, fmt):
    """Every factor set with three objects in one call (factors of their own) and with each of those objects alone; the
    restatement and the host chain are computed once per group and shared, and each call is held to the bar of its own inputs."""
    sets = factor_sets(1000 + nv * 100 + h)
    three = make_images(nv * 7 + h, fmt, (3, nv), h, w)
    dev_three = on_dev(three)
    for g in range(0, len(sets), 3):
        f = sets[g:g + 3]
        ref, host = ar.jitter(three, f), ar.host_chain(three, f)
        out = paug.color_jitter(dev_three, torch.from_numpy(f))
        assert tuple(out.shape) == (3, nv, 3, h, w) and out.dtype == torch.float32
        check_against_restatement(out, three, f, "SB 3 %s sets %d-%d" % (fmt, g, g + 2), ref, host)
        for o in range(3):                                           # one object, (4,) factors
            out = paug.color_jitter(dev_three[o], f[o])
            assert tuple(out.shape) == (nv, 3, h, w)
            check_against_restatement(out, three[o], f[o], "SB 1 %s %s" % (fmt, f[o].tolist()), ref[o], host[o])


@pytest.mark.parametrize("nv,h,w", [(2, 32, 32), (3, 37, 53)])
def test_misaligned_bases(nv, h, w):
    """The 16-byte paths need an aligned base: one element (float) or one byte into a buffer they must not be taken."""
    f = factor_sets(5)[[3, 9, 14]]
    for fmt in ("float", "bytes"):
        images = make_images(40 + h, fmt, (3, nv), h, w)
        aligned = on_dev(images)
        assert aligned.data_ptr() % 16 == 0
        want = paug.color_jitter(aligned, f)
        for shift in (1, 2, 3):
            buf = torch.zeros(aligned.numel() + 8, dtype=aligned.dtype, device=DEV)
            view = buf[shift:shift + aligned.numel()].view(aligned.shape)
            view.copy_(aligned)
            assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + shift * aligned.element_size()
            got = paug.color_jitter(view, f)
            check_against_restatement(got, images, f, "%s input %d element(s) in" % (fmt, shift))
            assert torch.equal(got, want)                            # the order of the sums does not depend on the alignment
            assert torch.equal(view, aligned) and float(buf[:shift].float().abs().sum()) == 0 and float(buf[shift + aligned.numel():].float().abs().sum()) == 0
        obuf = torch.full((want.numel() + 8,), 7.0, device=DEV)      # a misaligned output
        oview = obuf[1:1 + want.numel()].view(want.shape)
        assert paug.color_jitter(aligned, f, out=oview) is oview
        assert torch.equal(oview, want) and float(obuf[0]) == 7.0 and bool((obuf[1 + want.numel():] == 7.0).all())
    # in place at a misaligned base
    images = make_images(41, "float", (3, nv), h, w)
    want = paug.color_jitter(on_dev(images), f)
    buf = torch.zeros(want.numel() + 8, device=DEV)
    view = buf[1:1 + want.numel()].view(want.shape)
    view.copy_(on_dev(images))
    paug.color_jitter(view, f, out=view)
    assert torch.equal(view, want)


def test_in_place_and_run_to_run_bits():
    for nv, h, w in ((3, 37, 53), (2, 128, 128)):
        images = on_dev(make_images(50, "float", (2, nv), h, w))
        f = factor_sets(6)[[2, 12]]
        a = paug.color_jitter(images, f)
        b = paug.color_jitter(images, f)
        assert torch.equal(a, b)
        work = images.clone()
        res = paug.color_jitter(work, f, out=work)
        assert res is work and torch.equal(work, a)
        u8 = on_dev(make_images(51, "bytes", (2, nv), h, w))
        assert torch.equal(paug.color_jitter(u8, f), paug.color_jitter(u8, f))


@pytest.mark.parametrize("fmt", ["float", "bytes"])
def test_an_image_in_a_batch_equals_the_image_alone(fmt):
    """Nothing of one image -- its mean, its index, its object's factors -- reaches another.  (2, 5, 7): images at an odd byte
    stride; (2, 37, 53): at strides that are no multiple of 16 bytes."""
    for nv, h, w in ((2, 5, 7), (2, 37, 53), (2, 32, 32)):
        sb = 3
        images = on_dev(make_images(60 + h, fmt, (sb, nv), h, w))
        f = factor_sets(7)[[4, 13, 1]]
        batch = paug.color_jitter(images, f)
        for o in range(sb):
            for v in range(nv):
                alone = paug.color_jitter(images[o, v:v + 1].clone(), f[o])
                assert torch.equal(batch[o, v], alone[0]), (o, v)


def test_selecting_views_commutes_with_the_jitter():
    """The YOLO trainer may jitter only its source views: the factors are per object, the contrast mean per image."""
    images = on_dev(make_images(70, "float", (2, 5), 37, 53))
    f = factor_sets(8)[[5, 14]]
    sel = torch.tensor([3, 0, 3], device=DEV)
    assert torch.equal(paug.color_jitter(images, f)[:, sel], paug.color_jitter(images[:, sel], f))
    u8 = on_dev(make_images(71, "bytes", (2, 5), 5, 7))
    assert torch.equal(paug.color_jitter(u8, f)[:, sel], paug.color_jitter(u8[:, sel], f))


def test_a_non_default_stream_gives_the_same_bits():
    images = on_dev(make_images(80, "float", (2, 3), 37, 53))
    f = factor_sets(9)[[10, 2]]
    want = paug.color_jitter(images, f)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = paug.color_jitter(images, f)
    side.synchronize()
    assert torch.equal(got, want)


def test_65_objects_take_two_launches():
    sb, nv, h, w = 65, 1, 5, 7
    rs = np.random.RandomState(10)
    f = np.stack([rs.uniform(-0.5, 0.5, sb), rs.uniform(0, 2, sb), rs.uniform(0, 2, sb), rs.uniform(0, 2, sb)], 1).astype(np.float32)
    for fmt in ("float", "bytes"):
        host = make_images(90, fmt, (sb, nv), h, w)
        images = on_dev(host)
        got = paug.color_jitter(images, f)
        assert tuple(got.shape) == (sb, nv, 3, h, w)
        for o in range(sb):
            assert torch.equal(got[o], paug.color_jitter(images[o], f[o])), o
        check_against_restatement(got, host, f, "65 objects %s" % fmt)


class _Base(torch.utils.data.Dataset):
    z_near, z_far, base_path, image_to_tensor = 0.5, 2.0, "synthetic", staticmethod(pdata.image_to_tensor_balanced)

    def __init__(self):
        self.images = [torch.from_numpy(make_images(100 + i, "float", (3,), 25, 41)) for i in range(2)]

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return {"img_id": i, "images": self.images[i].clone()}


def test_end_to_end_deferred_dataset():
    """Two items of a deferred ColorJitterDataset, collated, jittered on the device, against the host dataset under the same
    seed (the host path applies the fp64 draws, the device their fp32 roundings: a relative 6e-8, far inside the bar)."""
    base = _Base()
    np.random.seed(12)
    host = torch.stack([pdata.ColorJitterDataset(base)[i]["images"] for i in range(2)]).numpy()
    np.random.seed(12)
    deferred = pdata.ColorJitterDataset(base, defer=True)
    batch = torch.utils.data.default_collate([deferred[i] for i in range(2)])
    assert tuple(batch["jitter"].shape) == (2, 4) and torch.equal(batch["images"], torch.stack(base.images))
    images = batch["images"].to(DEV)
    out = paug.color_jitter(images, batch["jitter"])
    err, e_host = check_against_restatement(out, batch["images"].numpy(), batch["jitter"].numpy(), "end to end")
    diff = float(np.abs(out.cpu().numpy().astype(np.float64) - host).max())
    print("end to end: device against the host dataset %.3g" % diff)
    assert diff <= max(4 * e_host, ar.FLOOR) and float(np.abs(host - batch["images"].numpy()).max()) > 1e-3
