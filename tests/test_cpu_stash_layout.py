"""The training stash's layout (pixel-nerf-yolo_amd/csrc/stash.h): a stand-alone host program prints every named slot, and
the numbers are checked against a transcription of the layout COMMENT of that header (not of its code)."""
import itertools

import pytest

from host_tools import CSRC, host_header_program

MODELS = [(5, 3), (3, 1000), (2, 0), (4, 1), (7, 3)]   # (n_blocks, combine_layer)
CONFIGS = [(nb, cl, ns, L) for (nb, cl), ns, L in itertools.product(MODELS, (1, 3), (512, 1792))]
SLOT, SMALL = 64 * 512, 64 * 64

PROGRAM = r"""
#include <cstdio>
#include "stash.h"
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) return 2;
    int nb, cl, ns, L;
    while (fscanf(f, "%d %d %d %d", &nb, &cl, &ns, &L) == 4) {   // one `n_blocks combine_layer ns L` per line
        const pny::StashLayout l = pny::stash_layout(nb, cl, ns, L);
        const int nvb = l.nvb(), npost = l.npost();
        printf("cfg %d %d %d %d\nnvb %d\nnpost %d\nx_tile %lld\ndy_tile %lld\n", nb, cl, ns, L, nvb, npost, l.x_tile, l.dy_tile);
        for (int v = 0; v < ns; ++v) {
            printf("x_in.%d %u\nx_z.%d %u\ndy_lin_in.%d %u\n", v, l.x_in(v), v, l.x_z(v), v, l.dy_lin_in(v));
            for (int b = 0; b < nvb; ++b)
                printf("x_h.%d.%d %u\nx_net.%d.%d %u\ndy_dnet.%d.%d %u\ndy_dh.%d.%d %u\ndy_fc1.%d.%d %u\n", v, b, l.x_h(v, b), v, b,
                       l.x_net(v, b), v, b, l.dy_dnet(v, b), v, b, l.dy_dh(v, b), v, b, l.dy_fc1(v, b));
        }
        for (int i = 0; i < npost; ++i)
            printf("x_post_h.%d %u\nx_post_net.%d %u\ndy_post_dnet.%d %u\ndy_post_dh.%d %u\ndy_post_fc1.%d %u\n", i, l.x_post_h(i), i,
                   l.x_post_net(i), i, l.dy_post_dnet(i), i, l.dy_post_dh(i), i, l.dy_post_fc1(i));
        printf("x_top %u\ndy_raw %u\ndy_top %u\ndy_dhm %u\n", l.x_top(), l.dy_raw(), l.dy_top(), l.dy_dhm());
        for (int b = 0; b < nvb; ++b) printf("dy_fc1_stride.%d %d\n", b, l.dy_fc1_stride(b));
    }
    return 0;
}
"""


def expected(nb, cl, ns, L):
    """The comment above StashLayout, slot by slot: name -> (offset, size) in floats, for the X and the dY record."""
    nvb = min(cl, nb)
    npost = nb - nvb
    x, dy, o = {}, {}, 0
    for v in range(ns):          # X: NS views x { x_in (16 rows), z (L/4 rows), per view block: relu(h_in), relu(net) }
        x["x_in.%d" % v] = (o, SMALL); o += SMALL
        x["x_z.%d" % v] = (o, 64 * L); o += 64 * L
        for b in range(nvb):
            x["x_h.%d.%d" % (v, b)] = (o, SLOT); o += SLOT
            x["x_net.%d.%d" % (v, b)] = (o, SLOT); o += SLOT
    for i in range(npost):       # + post part { per post block: relu(h_in), relu(net) ; relu(h_top) }
        x["x_post_h.%d" % i] = (o, SLOT); o += SLOT
        x["x_post_net.%d" % i] = (o, SLOT); o += SLOT
    x["x_top"] = (o, SLOT); o += SLOT
    x_tile, o = o, 0
    for v in range(ns):          # dY: NS views x { per view block: dnet, dh_in }
        for b in range(nvb):
            dy["dy_dnet.%d.%d" % (v, b)] = (o, SLOT); o += SLOT
            dy["dy_dh.%d.%d" % (v, b)] = (o, SLOT); o += SLOT
    dy["dy_raw"] = (o, SMALL); o += SMALL   # + post part { d_raw (16 rows), dh_top, per post block: dnet, dh_in }
    dy["dy_top"] = (o, SLOT); o += SLOT
    for i in range(npost):
        dy["dy_post_dnet.%d" % i] = (o, SLOT); o += SLOT
        dy["dy_post_dh.%d" % i] = (o, SLOT); o += SLOT
    return nvb, npost, x, x_tile, dy, o


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    program = host_header_program(tmp_path_factory.mktemp("stash"), PROGRAM, std="c++17", defines=(), include_dirs=(CSRC,),
                                  extra_flags=("-O0", "-Wall", "-Wextra", "-Werror"))
    out, cur = {}, None
    for line in program(["%d %d %d %d" % c for c in CONFIGS]):
        k, *vals = line.split()
        if k == "cfg":
            cur = out.setdefault(tuple(int(t) for t in vals), {})
        else:
            cur[k] = int(vals[0])
    return out


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "nb%d-cl%d-ns%d-L%d" % c)
def test_stash_slots_match_the_layout_comment(printed, cfg):
    nb, cl, ns, L = cfg
    got = dict(printed[cfg])
    nvb, npost, x, x_tile, dy, dy_tile = expected(*cfg)
    assert (got.pop("nvb"), got.pop("npost"), got.pop("x_tile"), got.pop("dy_tile")) == (nvb, npost, x_tile, dy_tile)
    # derived names
    dhm = dy["dy_post_dh.0"][0] if npost > 0 else dy["dy_top"][0]
    assert got.pop("dy_dhm") == dhm
    assert (dhm == dy["dy_top"][0]) == (npost == 0)
    for v in range(ns):
        assert got.pop("dy_lin_in.%d" % v) == (dy["dy_dh.%d.0" % v][0] if nvb > 0 else dhm)
        for b in range(nvb):
            assert got.pop("dy_fc1.%d.%d" % (v, b)) == (dy["dy_dh.%d.%d" % (v, b + 1)][0] if b + 1 < nvb else dhm)
    for i in range(npost):
        assert got.pop("dy_post_fc1.%d" % i) == (dy["dy_post_dh.%d" % (i + 1)][0] if i + 1 < npost else dy["dy_top"][0])
    for b in range(nvb):    # the view stride of the dY part, or 0 where dy_fc1 is dhm
        assert got.pop("dy_fc1_stride.%d" % b) == (2 * nvb * SLOT if b + 1 < nvb else 0)
    # every slot: the offset of the transcription; together they tile each record exactly (disjoint, inside, no gap)
    want = {k: o for k, (o, _) in list(x.items()) + list(dy.items())}
    assert got == want
    for rec, size in ((x, x_tile), (dy, dy_tile)):
        end = 0
        for o, n in sorted(rec[k] for k in rec):
            assert o == end
            end = o + n
        assert end == size
