"""
Cases, plain references, bars and recorded figures of the sweep of the list-of-feature-maps latent
(tests/test_cpu_latent_levels.py, tests/test_gpu_latent_levels.py; include/pnyolo.h pny_latent_levels,
pny_latent_levels_backward, pny_scene_set_latent_levels; reference src/model/encoder.py:126-137).

References.  The latent is F.interpolate(bilinear, align_corners=True) of every map to the first map's size and torch.cat
along the channels, the maps' gradients are its autograd -- both in float64 ON THE FLOAT32 INPUTS.

Errors are max |got - ref| over a tensor, divided by max(1, max |ref|) for the latent and by the float64 tensor's max |.| for a
map's gradient (the convention of tests/trunk_stage_ref.py).

Bars.  Each bar is TWICE the largest error of the float32 restatement -- the same ATen calls in float32 on the CPU -- against
float64 over this sweep's cases (the kernels blend and sum in another order than ATen does).  The figures are recorded as
*_ERR32; the CPU test measures them again (within 10 % above, not below half) and shows the bars under their caps, CAP_ACT and
CAP_GRAD, on every case.  The kernels' own errors set nothing.

Cases.  Six lists of level sizes (level 0 first: odd ratios down to 1 x 1, a level of the latent's own size, levels larger than
the latent, a 1 x 1 latent, a single-row latent, the real data's 2 : 1 pyramid), each with the channel counts (4, 8, 12, 4)
(every level a multiple of 4: the 16-byte path) and (3, 5, 2, 7) (the scalar path), with one and two images, with level 0
alone, and stretched to 8 levels.

Marker runs.  One pixel per level -- the last, in channels 0 and C_i - 1, of every image -- set to 100 x the input's standard
deviation: a channel offset or a stride that is off moves it where no bar would see a plain value.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

F32, F64 = torch.float32, torch.float64
MARKER = 100.0
CAP_ACT, CAP_GRAD = 2e-4, 1e-4

# largest float32-restatement error over the sweep's cases, measured on the CPU (tests/test_cpu_latent_levels.py)
FWD_ERR32 = 9.7e-7
BWD_ERR32 = 1.03e-6
FWD_BAR, BWD_BAR = 2 * FWD_ERR32, 2 * BWD_ERR32

SIZES = {
    "odd_ratios": ((9, 15), (5, 8), (3, 4), (1, 1)),
    "same_size": ((9, 15), (9, 15)),
    "larger_than_level0": ((9, 15), (17, 29), (10, 16)),
    "latent_1x1": ((1, 1), (3, 4), (1, 5)),
    "single_row": ((1, 7), (1, 4), (2, 13)),
    "real_data_like": ((16, 30), (8, 15), (4, 8)),
}
CHANNELS = ((4, 8, 12, 4), (3, 5, 2, 7))
MAX_LEVELS = 8


def cases(name):
    """dicts name, sizes, channels, n, tag: the case's levels with both channel tuples and n = 1, 2; level 0 alone; 8 levels."""
    sizes = SIZES[name]
    k = len(sizes)
    out = []
    for ch in CHANNELS:
        for n in (1, 2):
            out.append(dict(name=name, sizes=sizes, channels=ch[:k], n=n, tag="plain"))
    for j, ch in enumerate(CHANNELS):
        out.append(dict(name=name, sizes=sizes[:1], channels=ch[:1], n=1 + j, tag="one_level"))
        out.append(dict(name=name, sizes=tuple(sizes[i % k] for i in range(MAX_LEVELS)),
                        channels=tuple(ch[i % 4] for i in range(MAX_LEVELS)), n=2 - j, tag="eight_levels"))
    return out


def all_cases():
    return [c for name in SIZES for c in cases(name)]


def case_id(c):
    return "%s-%s-c%s-n%d" % (c["name"], c["tag"], "x".join(str(v) for v in c["channels"][:2]), c["n"])


def inputs(c, markers=False):
    """float32 NCHW maps and the upstream gradient of the latent, (n, sum C, h0, w0)."""
    rs = np.random.RandomState(21000 + 97 * sorted(SIZES).index(c["name"]) + 13 * c["channels"][0] + 5 * c["n"] + len(c["sizes"]))
    maps = [torch.from_numpy(rs.randn(c["n"], ch, h, w).astype(np.float32)) for ch, (h, w) in zip(c["channels"], c["sizes"])]
    g = torch.from_numpy(rs.randn(c["n"], sum(c["channels"]), *c["sizes"][0]).astype(np.float32))
    if markers:
        for m in maps:
            m[:, 0, -1, -1] = MARKER
            m[:, -1, -1, -1] = MARKER
    return maps, g


def latent_ref(maps, dtype=F64):
    """The reference's branch, restated: (n, sum C, h0, w0)."""
    size0 = tuple(maps[0].shape[-2:])
    return torch.cat([Fn.interpolate(m.to(dtype), size0, mode="bilinear", align_corners=True) for m in maps], dim=1)


def grads_ref(maps, g, dtype=F64):
    leaves = [m.to(dtype).requires_grad_(True) for m in maps]
    return list(torch.autograd.grad(latent_ref(leaves, dtype), leaves, g.to(dtype)))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def rel_err(got, ref, kind):
    """max |got - ref| over the float64 tensor's max (kind "grad") or over max(1, that) (kind "act")."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite result"
    m = float(ref.abs().max())
    s = max(1.0, m) if kind == "act" else m
    e = float((got - ref).abs().max())
    return e / s if s > 0.0 else e


def marker_channels(c):
    """Latent channels that a marker run may change: channel 0 and C_i - 1 of every level."""
    out, off = set(), 0
    for ch in c["channels"]:
        out.update((off, off + ch - 1))
        off += ch
    return sorted(out)
