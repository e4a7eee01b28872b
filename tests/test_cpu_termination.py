"""
Early ray termination without a GPU: csrc/pny_termination.h compiled for the host by g++ against its numpy restatement
(tests/termination_ref.py) -- the segment bounds exactly, the sequential transmittance within K * 2^-22 -- the alive rule, the
entry points' refusals, which arrive before any launch, and the header, binding and Makefile.

The bar on T: expf within 1 ulp of a value <= 1, two additions and one multiplication per factor, under four roundings of 2^-24;
the factors are <= 1, so the errors add: K * 4 * 2^-24 = K * 2^-22 absolute.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import termination_ref as tref
from host_tools import CSRC, built_lib, c99_program, header_code, host_header_program  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib

HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pny_termination.h"
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
        if (!strcmp(cmd, "bounds")) {           // K 1 .. kmax, S 1 .. smax: S' then the S' + 1 bounds, one after the other
            int32_t h[2];
            rd(in, h, 2);
            for (int K = 1; K <= h[0]; ++K)
                for (int S = 1; S <= h[1]; ++S) {
                    const int32_t sp = term_segments(K, S);
                    wr(out, &sp, 1);
                    for (int j = 0; j <= sp; ++j) {
                        const int32_t b = term_bound(K, sp, j);
                        wr(out, &b, 1);
                    }
                }
        } else {                                // n K S, t_min; rays, z, samp -> T (n, S' + 1), alive (n, S' + 1) after each bound
            int32_t h[3];
            float t_min;
            rd(in, h, 3), rd(in, &t_min, 1);
            const int n = h[0], K = h[1], sp = term_segments(K, h[2]);
            std::vector<float> rays((size_t)n * 8), z((size_t)n * K), samp((size_t)n * K * 4);
            rd(in, rays.data(), rays.size()), rd(in, z.data(), z.size()), rd(in, samp.data(), samp.size());
            std::vector<float> T((size_t)n * (sp + 1));
            std::vector<int8_t> alive((size_t)n * (sp + 1));
            for (int r = 0; r < n; ++r) {
                float t = 1.0f;
                bool a = true;
                T[(size_t)r * (sp + 1)] = t, alive[(size_t)r * (sp + 1)] = 1;
                for (int j = 0; j < sp; ++j) {
                    t *= term_product(z.data() + (size_t)r * K, samp.data() + (size_t)r * K * 4, K, term_bound(K, sp, j),
                                      term_bound(K, sp, j + 1), rays[(size_t)r * 8 + 7]);
                    a = term_alive(a, t, t_min);
                    T[(size_t)r * (sp + 1) + j + 1] = t, alive[(size_t)r * (sp + 1) + j + 1] = a ? 1 : 0;
                }
            }
            wr(out, T.data(), T.size()), wr(out, alive.data(), alive.size());
        }
        fclose(in), fclose(out);
        printf("ok\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("termination_host")
    return host_header_program(tmp, HOST_MAIN, defines=("__device__=", "__host__=", "__forceinline__=inline"), include_dirs=(CSRC,)), tmp


def host_transmittance(host_header, rays, z, samp, t_min, S):
    run, tmp = host_header
    fin, fout = str(tmp / "t_in.bin"), str(tmp / "t_out.bin")
    n, K = z.shape
    with open(fin, "wb") as f:
        f.write(np.asarray([n, K, S], dtype=np.int32).tobytes() + np.float32(t_min).tobytes())
        f.write(rays.astype(np.float32).tobytes() + z.astype(np.float32).tobytes() + samp.astype(np.float32).tobytes())
    assert run(["T %s %s" % (fin, fout)]) == ["ok"]
    sp = min(S, K)
    raw = open(fout, "rb").read()
    T = np.frombuffer(raw[: 4 * n * (sp + 1)], dtype=np.float32).reshape(n, sp + 1)
    alive = np.frombuffer(raw[4 * n * (sp + 1):], dtype=np.int8).reshape(n, sp + 1).astype(bool)
    return T, alive


def case(n, K, seed, gain=3.0):
    """rays, z, samp: sorted depths in [0.8, 1.8], sigma in [-2, gain] with a NaN, a ray of zero rows, a depth beyond far, an opaque ray."""
    rng = np.random.default_rng(seed)
    z = np.sort(rng.uniform(0.8, 1.8, size=(n, K)).astype(np.float32), axis=1)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 3:6], rays[:, 6], rays[:, 7] = (0.0, 0.0, 1.0), 0.8, 1.8
    samp = rng.uniform(0.0, 1.0, size=(n, K, 4)).astype(np.float32)
    samp[..., 3] = rng.uniform(-2.0, gain, size=(n, K))
    samp[1, K // 3, 3] = np.nan
    samp[2] = 0.0
    z[3, -1] = 1.9
    samp[3, -1, 3] = 5.0
    samp[0, :, 3] = 40.0           # an opaque ray
    return rays, z, samp


# --------------------------------------------------------------------------- bounds
def test_bounds_equal_the_restatement_for_every_k_and_s(host_header):
    run, tmp = host_header
    fin, fout = str(tmp / "b_in.bin"), str(tmp / "b_out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([200, 16], dtype=np.int32).tobytes())
    assert run(["bounds %s %s" % (fin, fout)]) == ["ok"]
    got = np.fromfile(fout, dtype=np.int32).tolist()
    at = 0
    for K in range(1, 201):
        for S in range(1, 17):
            want = tref.bounds(K, S)
            sp = got[at]
            assert sp == min(S, K) == len(want) - 1
            assert got[at + 1: at + 2 + sp] == want, (K, S)
            at += 2 + sp
            assert want[0] == 0 and want[-1] == K and all(a < b for a, b in zip(want, want[1:])), "whole range, no gap, ascending"
            assert max(np.diff(want)) == -(-K // sp), "the largest segment sizes the workspace"
    assert at == len(got)
    assert np.diff(tref.bounds(24, 5)).tolist() == [4, 5, 5, 5, 5] and tref.bounds(192, 2) == [0, 96, 192]


# --------------------------------------------------------------------------- transmittance and alive
@pytest.mark.parametrize("n,K,S", [(70, 16, 4), (5, 192, 2), (9, 24, 5), (4, 3, 16)])
def test_host_transmittance_against_the_restatement(host_header, n, K, S):
    rays, z, samp = case(n, K, seed=K + S, gain=30.0 if K < 100 else 3.0)
    t_min = 0.3
    b = tref.bounds(K, S)
    want = tref.transmittance(rays, z, samp)[:, b]
    T, alive = host_transmittance(host_header, rays, z, samp, t_min, S)
    assert np.isfinite(want).all() and np.isfinite(T).all(), "a NaN sigma counts as 0"
    err = np.abs(T - want)
    assert (err <= K * 2.0 ** -22).all(), err.max()
    assert (T[2] == 1.0).all() and alive[2].all(), "zero rows: every factor is exactly 1"
    assert tref.factors(rays, z, samp)[3, -1] > 1.0, "a depth beyond far: a negative last delta, a factor above 1"
    assert (alive[:, 1:] <= alive[:, :-1]).all(), "alive is monotone: a ray that dies stays dead"
    clear = ~(np.abs(want.astype(np.float64) / t_min - 1.0) < 1e-3).any(axis=1)
    want_alive = np.logical_and.accumulate(~(want < np.float32(t_min)), axis=1)
    assert (alive[clear] == want_alive[clear]).all()
    assert alive[:, 0].all() and 0 < alive[:, -1].sum() < n


def test_restated_alive_and_keep():
    """The restatement against itself: with no grid and nothing masked before a boundary its T is the plain one; a dead ray's
    samples are not kept and its T stays; a NaN transmittance keeps the ray alive."""
    rays, z, samp = case(9, 24, seed=4, gain=30.0)
    alive, keep, T = tref.alive_and_keep(rays, z, samp, 0.3, 5)
    b = tref.bounds(24, 5)
    plain = tref.transmittance(rays, z, samp)[:, b]
    for j in range(5):
        seg = slice(b[j], b[j + 1])
        assert (keep[:, seg] == alive[:, j:j + 1]).all()
        live = alive[:, j]
        assert np.allclose(T[live, j + 1], plain[live, j + 1], rtol=0, atol=24 * 2.0 ** -22)
        assert (T[~live, j + 1] == T[~live, j]).all()
    assert (alive[:, 1:] <= alive[:, :-1]).all() and not alive[:, -1].all() and alive[2].all()
    # a NaN: an infinite delta times a zero sigma
    z2 = z.copy()
    z2[5, 2] = np.inf
    samp2 = samp.copy()
    samp2[5, :, 3] = 0.0
    alive2, keep2, T2 = tref.alive_and_keep(rays, z2, samp2, 0.3, 5)
    assert np.isnan(T2[5, 1:]).all() and alive2[5].all() and keep2[5].all()
    # a grid's verdict masks sigma: the factor of a culled sample is exactly 1
    gk = np.zeros((9, 24), dtype=bool)
    alive3, keep3, T3 = tref.alive_and_keep(rays, z, samp, 0.3, 5, grid_keep=gk)
    assert not keep3.any() and alive3.all() and (T3 == 1.0).all()


# --------------------------------------------------------------------------- the entry points
def test_refusals_arrive_before_any_launch(built_lib):
    """Every call here carries fake device pointers: a launch would fault or report a HIP error, a refusal is PNY_ERR_ARG."""
    L, p = built_lib, C.c_void_p(4096)
    ok3 = (C.c_int32 * 3)(4, 4, 4)
    box = ((C.c_double * 3)(-1, -1, -1), (C.c_double * 3)(1, 1, 1))

    def refused(rc, text):
        assert rc == plib.ERR_ARG, rc
        assert text in L.pny_last_error().decode(), L.pny_last_error()

    def update(rays=p, z=p, samp=p, n=4, k=8, kb=0, ke=4, t_min=0.5, T=p, alive=p, count=p):
        return L.pny_termination_update(rays, z, samp, n, k, kb, ke, t_min, T, alive, count, None)

    for name in ("rays", "z", "samp", "T", "alive"):
        refused(update(**{name: None}), "null")
    refused(update(n=-1), "n >= 0")
    refused(update(k=0), "k >= 1")
    for kb, ke in ((-1, 4), (4, 4), (5, 4), (0, 9)):
        refused(update(kb=kb, ke=ke), "k_begin")
    refused(update(t_min=float("nan")), "NaN")
    refused(update(t_min=1.0), "[0,1)")
    refused(update(t_min=-0.5), "[0,1)")
    refused(update(n=2 ** 28, k=5, ke=5), "2^30")
    refused(update(samp=C.c_void_p(4100)), "aligned")

    def classify(bits=p, dims=ok3, c1=box[0], c2=box[1], rays=p, z=p, n=4, k=8, kb=2, ke=6, alive=p, slot=p, kept=p, ws=p, ws_bytes=4096):
        return L.pny_occupancy_classify_segment(bits, dims, c1, c2, 0, rays, z, n, k, kb, ke, alive, slot, kept, ws, ws_bytes, None)

    for name in ("dims", "c1", "c2", "rays", "z", "slot", "kept", "ws"):
        refused(classify(**{name: None}), "null")
    refused(classify(dims=(C.c_int32 * 3)(1, 4, 4)), "at least 2")
    refused(classify(c2=(C.c_double * 3)(1, -1, 1)), "c2 must be above c1")
    refused(classify(k=0), "k >= 1")
    refused(classify(n=-1), "n >= 0")
    for kb, ke in ((-1, 4), (4, 4), (5, 4), (0, 9)):
        refused(classify(kb=kb, ke=ke), "k_begin")
    refused(classify(n=2 ** 28, k=5, kb=0, ke=1), "2^30")
    refused(classify(rays=C.c_void_p(4100)), "aligned")
    refused(classify(ws_bytes=255), "workspace")
    refused(classify(ws=C.c_void_p(4100)), "workspace")
    refused(L.pny_scene_set_termination(None, 0.5, 4), "null")
    n = C.c_int(0)
    refused(L.pny_scene_last_segments(None, 0, None, None, 0, C.byref(n)), "null")


# --------------------------------------------------------------------------- header, binding, build
def test_header_is_still_strict_c99_at_version_11(built_lib, tmp_path):
    names = ("pny_scene_set_termination", "pny_scene_last_segments", "pny_termination_update", "pny_occupancy_classify_segment")
    run = c99_program(tmp_path, '#include <stdio.h>\n#include "pnyolo.h"\n'
                      "typedef int (*set_fn)(pny_scene*, float, int);\n"
                      "typedef int (*seg_fn)(pny_scene*, int, int64_t*, int64_t*, int, int*);\n"
                      "int main(void) { set_fn a = pny_scene_set_termination; seg_fn b = pny_scene_last_segments; (void)a; (void)b;\n"
                      '  printf("%d\\n", PNY_ABI_VERSION); return 0; }\n', link=True)()
    assert run.returncode == 0 and run.stdout.strip() == "11", (run.returncode, run.stdout, run.stderr)
    code = header_code()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, code) and n in plib.SIGNATURES and hasattr(built_lib, n), n
    assert not re.search(r"#\s*define\s+PNY_TERM", code), "the termination section adds no constant"


def test_sources_are_in_the_makefile():
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    srcs = re.search(r"(?m)^SRCS\s*=(.*)$", make).group(1).split()
    assert "termination.hip" in srcs and "occupancy.hip" in srcs
    assert "pny_termination.h" in re.search(r"(?m)^%\.o:(.*)$", make).group(1).split()
    for name in ("termination.hip", "pny_termination.h"):
        assert os.path.exists(os.path.join(CSRC, name))
