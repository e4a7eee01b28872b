"""
The occupancy grid without a GPU: csrc/pny_occupancy.h compiled for the host by g++ against its numpy restatement
(tests/occupancy_ref.py), bit for bit, on the volumes and rays the GPU tests hold the kernels to; the entry points' refusals,
which arrive before any launch; the header, still strict C99 at ABI version 11; the Makefile.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import occupancy_ref as oref
from host_tools import CSRC, built_lib, c99_program, header_code, host_header_program  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib

HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pny_occupancy.h"
using namespace pny;

template <class T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) exit(3); }
template <class T> static void wr(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) exit(4); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* q = fopen(argv[1], "r");
    if (!q) return 2;
    char cmd[32], fin[1024], fout[1024];
    while (fscanf(q, "%31s %1023s %1023s", cmd, fin, fout) == 3) {
        FILE* in = fopen(fin, "rb");
        FILE* out = fopen(fout, "wb");
        if (!in || !out) return 2;
        if (!strcmp(cmd, "build")) {
            int32_t h[5];                       // X Y Z dilate two
            float thresh;
            rd(in, h, 5), rd(in, &thresh, 1);
            const size_t n = (size_t)h[0] * h[1] * h[2];
            std::vector<float> s1(n), s2(h[4] ? n : 0);
            rd(in, s1.data(), n), rd(in, s2.data(), s2.size());
            OccBuildArgs a;
            a.sigma = s1.data(), a.sigma2 = h[4] ? s2.data() : nullptr, a.d.x = h[0], a.d.y = h[1], a.d.z = h[2];
            a.thresh = thresh, a.dilate = h[3], a.bits = nullptr, a.occupied = nullptr;
            a.n_words = (uint32_t)occ_words(occ_cells(h[0], h[1], h[2]));
            std::vector<uint32_t> bits(a.n_words);
            for (uint32_t w = 0; w < a.n_words; ++w) bits[w] = occ_word(a, w);
            wr(out, bits.data(), bits.size());
        } else {
            int32_t h[7];                       // X Y Z outside_empty n k words
            double c[6];
            rd(in, h, 7), rd(in, c, 6);
            std::vector<uint32_t> bits(h[6]);
            std::vector<float> rays((size_t)h[4] * 8), z((size_t)h[4] * h[5]);
            rd(in, bits.data(), bits.size()), rd(in, rays.data(), rays.size()), rd(in, z.data(), z.size());
            OccGrid g;
            g.bits = bits.data(), g.outside_empty = h[3];
            occ_grid_axes(g, h, c, c + 3);
            std::vector<int64_t> cell(z.size());
            std::vector<int8_t> keep(z.size());
            for (size_t s = 0; s < z.size(); ++s) {
                const float* r = rays.data() + (s / h[5]) * 8;
                cell[s] = occ_sample_cell(g, r, r + 3, z[s]);
                keep[s] = occ_keep(g, r, r + 3, z[s]) ? 1 : 0;
            }
            wr(out, cell.data(), cell.size()), wr(out, keep.data(), keep.size());
        }
        fclose(in), fclose(out);
        printf("ok\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("occupancy_host")
    return host_header_program(tmp, HOST_MAIN, defines=("__device__=", "__host__=", "__forceinline__=inline"), include_dirs=(CSRC,)), tmp


def host_build(host_header, sigma, sigma2, thresh, dilate):
    run, tmp = host_header
    fin, fout = str(tmp / "b_in.bin"), str(tmp / "b_out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(list(sigma.shape) + [dilate, int(sigma2 is not None)], dtype=np.int32).tobytes())
        f.write(np.float32(thresh).tobytes())
        f.write(np.ascontiguousarray(sigma, dtype=np.float32).tobytes())
        if sigma2 is not None:
            f.write(np.ascontiguousarray(sigma2, dtype=np.float32).tobytes())
    assert run(["build %s %s" % (fin, fout)]) == ["ok"]
    return np.fromfile(fout, dtype=np.uint32)


def host_classify(host_header, bits, dims, box, outside_empty, rays, z):
    run, tmp = host_header
    fin, fout = str(tmp / "c_in.bin"), str(tmp / "c_out.bin")
    n, k = z.shape
    with open(fin, "wb") as f:
        f.write(np.asarray(list(dims) + [int(outside_empty), n, k, bits.size], dtype=np.int32).tobytes())
        f.write(np.asarray(list(box[0]) + list(box[1]), dtype=np.float64).tobytes())
        f.write(bits.astype(np.uint32).tobytes() + rays.astype(np.float32).tobytes() + z.astype(np.float32).tobytes())
    assert run(["classify %s %s" % (fin, fout)]) == ["ok"]
    raw = open(fout, "rb").read()
    cell = np.frombuffer(raw[: 8 * n * k], dtype=np.int64).reshape(n, k)
    keep = np.frombuffer(raw[8 * n * k:], dtype=np.int8).reshape(n, k).astype(bool)
    return cell, keep


# --------------------------------------------------------------------------- the restatement against itself
def test_restated_fma_rounds_once():
    """The restatement's fused multiply-add on cases where rounding the double sum a second time would differ, and against
    exact rational arithmetic on random operands."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.normal(size=4000).astype(np.float32)
    b = rng.normal(size=4000).astype(np.float32)
    c = (rng.normal(size=4000) * 10.0 ** rng.integers(-6, 3, size=4000)).astype(np.float32)
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a tie of the fp32 rounding; an addend of +- 2^-60, lost in the double sum, decides it
    a[2:4], b[2:4], c[2:4] = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12), (np.float32(2.0 ** -60), np.float32(-2.0 ** -60))
    got = oref.fmaf(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (i, a[i], b[i], c[i], got[i])
    assert got[2] == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23) and got[3] == np.float32(1.0 + 2.0 ** -11)


def test_restated_dilation_is_the_chebyshev_ball():
    raw = np.zeros((6, 5, 9), dtype=bool)
    sigma = np.zeros((7, 6, 10), dtype=np.float32)
    # a single corner above the threshold at grid point (3, 3, 3): raw cells 2 .. 3 per axis, then the box around them
    sigma[3, 3, 3] = 1.0
    for d in (0, 1, 4):
        got = oref.cells_occupied(sigma, None, 0.5, d)
        want = np.zeros_like(raw)
        want[max(2 - d, 0):4 + d, max(2 - d, 0):4 + d, max(2 - d, 0):4 + d] = True
        assert (got == want).all(), d


# --------------------------------------------------------------------------- the header against the restatement
@pytest.mark.parametrize("dims", oref.VOLUMES)
def test_build_matches_the_restatement_bit_for_bit(host_header, dims):
    cells = oref.n_cells(dims)
    for two in (False, True):
        vols = oref.case_volume(dims, seed=11 + sum(dims), two=two)
        s1, s2 = (vols[0], vols[1]) if two else (vols, None)
        for thresh in oref.thresholds():
            for dilate in (0, 1, 4):
                want, count = oref.build(s1, s2, thresh, dilate)
                got = host_build(host_header, s1, s2, thresh, dilate)
                assert got.size == oref.n_words(dims) == want.size
                assert (got == want).all(), (dims, two, thresh, dilate)
                assert int(sum(bin(int(w)).count("1") for w in got)) == count
                if cells % 32:
                    assert int(got[-1]) >> (cells % 32) == 0, "padding bits past the last cell must be 0"
                if thresh == -np.inf:
                    assert count == cells
                if thresh == np.inf and dilate == 0:
                    nan = np.isnan(s1) | (np.isnan(s2) if two else False)
                    assert count == int(oref.cells_occupied(np.where(nan, 1.0, 0.0).astype(np.float32), None, 0.5, 0).sum())


@pytest.mark.parametrize("outside_empty", (0, 1))
def test_classification_matches_the_restatement_bit_for_bit(host_header, outside_empty):
    dims = oref.VOLUMES[0]
    bits, _ = oref.build(oref.case_volume(dims, seed=3), None, 0.8, 0)
    rays, z = oref.case_rays(70, 16, seed=7)
    want_cell = oref.sample_cells(dims, oref.BOX[0], oref.BOX[1], rays, z)
    want_keep = oref.keep_mask(bits, dims, oref.BOX[0], oref.BOX[1], outside_empty, rays, z)
    cell, keep = host_classify(host_header, bits, dims, oref.BOX, outside_empty, rays, z)
    assert (cell == want_cell).all()
    assert (keep == want_keep).all()
    # what the cases are there for
    inside = want_cell >= 0
    assert inside.any() and (~inside).any() and 0 < want_keep[inside].sum() < inside.sum()
    assert want_cell[0, 0] == 0, "a sample exactly on c1 is in cell 0"
    assert (want_cell[0:6:2, -1] == -1).all(), "a sample exactly on c2 is outside"
    assert (want_cell[7::2][:3] == -1).all(), "a ray inside the upper face of the box is outside: t = cells is not below cells"
    assert (want_cell[6::2][:3] >= 0).any(), "a ray inside the lower face is inside where it crosses the box"
    assert np.isnan(z).any() and (want_cell[np.isnan(z)] == -1).all()
    assert (want_keep[~inside] == (not outside_empty)).all()
    slot, count = oref.slots(want_keep)
    assert count == want_keep.sum() and (np.diff(slot[slot >= 0]) == 1).all() and slot.max() == count - 1


# --------------------------------------------------------------------------- the entry points
def _i3(*v):
    return (C.c_int32 * 3)(*v)


def _d3(*v):
    return (C.c_double * 3)(*v)


def test_words(built_lib):
    out = C.c_int64(-1)
    for dims in oref.VOLUMES + ((128, 128, 128),):
        assert built_lib.pny_occupancy_words(_i3(*dims), C.byref(out)) == plib.OK
        assert out.value == oref.n_words(dims)
    assert out.value == 127 ** 3 // 32 + 1
    assert built_lib.pny_occupancy_words(_i3(2, 1, 2), C.byref(out)) == plib.ERR_ARG
    assert built_lib.pny_occupancy_words(None, C.byref(out)) == plib.ERR_ARG
    assert built_lib.pny_occupancy_words(_i3(2, 2, 2), None) == plib.ERR_ARG
    assert built_lib.pny_occupancy_classify_workspace_bytes(1120, C.byref(out)) == plib.OK and out.value == 256
    assert built_lib.pny_occupancy_classify_workspace_bytes(1024 * 1024 + 1, C.byref(out)) == plib.OK and out.value == 4352 + 256
    assert built_lib.pny_occupancy_classify_workspace_bytes(-1, C.byref(out)) == plib.ERR_ARG
    assert built_lib.pny_occupancy_classify_workspace_bytes(2 ** 30 + 1, C.byref(out)) == plib.ERR_ARG
    assert built_lib.pny_occupancy_classify_workspace_bytes(8, None) == plib.ERR_ARG


def test_refusals_arrive_before_any_launch(built_lib):
    """Every call here carries fake device pointers: a launch would fault or report a HIP error, a refusal is PNY_ERR_ARG."""
    L, p = built_lib, C.c_void_p(4096)
    ok3, box = _i3(4, 4, 4), (_d3(-1, -1, -1), _d3(1, 1, 1))

    def refused(rc, text):
        assert rc == plib.ERR_ARG, rc
        assert text in L.pny_last_error().decode(), L.pny_last_error()

    refused(L.pny_occupancy_build(None, None, ok3, 0.5, 1, p, p, None), "null")
    refused(L.pny_occupancy_build(p, None, None, 0.5, 1, p, p, None), "null")
    refused(L.pny_occupancy_build(p, None, ok3, 0.5, 1, None, p, None), "null")
    refused(L.pny_occupancy_build(p, None, _i3(4, 1, 4), 0.5, 1, p, p, None), "at least 2")
    refused(L.pny_occupancy_build(p, None, _i3(2048, 2048, 2048), 0.5, 1, p, p, None), "2^31")
    for dilate in (-1, 5):
        refused(L.pny_occupancy_build(p, None, ok3, 0.5, dilate, p, p, None), "dilate")
    refused(L.pny_occupancy_build(p, None, ok3, float("nan"), 1, p, p, None), "NaN")

    def classify(bits=p, dims=ok3, c1=box[0], c2=box[1], rays=p, z=p, n=4, k=4, slot=p, kept=p, ws=p, ws_bytes=4096):
        return L.pny_occupancy_classify(bits, dims, c1, c2, 0, rays, z, n, k, slot, kept, ws, ws_bytes, None)

    for name in ("bits", "dims", "c1", "c2", "rays", "z", "slot", "kept", "ws"):
        refused(classify(**{name: None}), "null")
    refused(classify(dims=_i3(1, 4, 4)), "at least 2")
    refused(classify(c2=_d3(1, -1, 1)), "c2 must be above c1")
    refused(classify(c2=_d3(1, float("inf"), 1)), "finite")
    refused(classify(c1=_d3(float("nan"), -1, -1)), "finite")
    refused(classify(k=0), "k >= 1")
    refused(classify(n=-1), "n >= 0")
    refused(classify(n=2 ** 28, k=5), "2^30")
    refused(classify(rays=C.c_void_p(4100)), "aligned")
    refused(classify(ws_bytes=255), "workspace")
    refused(classify(ws=C.c_void_p(4100)), "workspace")
    refused(L.pny_scene_set_occupancy(None, p, ok3, box[0], box[1], 0, None), "null")
    refused(L.pny_scene_last_cull(None, None, None), "null")


# --------------------------------------------------------------------------- header, binding, build
def test_header_is_still_strict_c99_at_version_11(built_lib, tmp_path):
    names = ("pny_occupancy_words", "pny_occupancy_build", "pny_occupancy_classify_workspace_bytes", "pny_occupancy_classify",
             "pny_scene_set_occupancy", "pny_scene_last_cull")
    run = c99_program(tmp_path, '#include <stdio.h>\n#include "pnyolo.h"\n'
                      "typedef int (*words_fn)(const int32_t[3], int64_t*);\n"
                      "typedef int (*cull_fn)(pny_scene*, int64_t[2], int64_t[2]);\n"
                      "int main(void) { words_fn w = pny_occupancy_words; cull_fn c = pny_scene_last_cull; (void)w; (void)c;\n"
                      '  printf("%d\\n", PNY_ABI_VERSION); return 0; }\n', link=True)()
    assert run.returncode == 0 and run.stdout.strip() == "11", (run.returncode, run.stdout, run.stderr)
    code = header_code()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, code) and n in plib.SIGNATURES, n
    assert not re.search(r"#\s*define\s+PNY_OCC", code), "the occupancy section adds no constant"
    assert "pny_occupancy" not in "".join(re.findall(r"typedef\s+struct[^;{]*\{", code)), "and no struct"


def test_sources_are_in_the_makefile():
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    srcs = re.search(r"(?m)^SRCS\s*=(.*)$", make).group(1).split()
    assert "occupancy.hip" in srcs and "occupancy_api.hip" in srcs
    assert "pny_occupancy.h" in re.search(r"(?m)^%\.o:(.*)$", make).group(1).split()
    for name in ("occupancy.hip", "occupancy_api.hip", "pny_occupancy.h"):
        assert os.path.exists(os.path.join(CSRC, name))
