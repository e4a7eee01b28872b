"""
The renderers' seeded random draws (Philox4x32-10 inside the kernels, pixel-nerf-yolo_amd/csrc/pny_rng.h) against the
oracle's independent restatement of the generator (oracle/pnyolo_oracle.py: philox4x32_10, philox_uniform, philox_normal,
seeded_draws).  No GPU: the published known-answer vectors, the kernels' own header compiled for the host, and the index
layouts of seeded_draws.  tests/test_gpu_seeded.py holds the kernels to the same restatement.
"""
import numpy as np
import pytest

import pnyolo_oracle as orc
from host_tools import CSRC, host_header_program

# |g_kernel - g_float64| of one Box-Muller normal: the fp32 product 2 pi u2 is off by at most half an ulp of 6.28 (2.4e-7) and
# enters through |r sin| <= 5.77; accurate logf / sqrtf / cosf add a few ulp of a value below 5.77 (ulp 4.8e-7): about 4e-6.
NORMAL_ABS_TOL = 1e-5


# Random123 (the Philox authors' library), kat_vectors, "philox4x32 10": counter, key -> output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,expect", KAT)
def test_philox_known_answer_vectors(counter, key, expect):
    assert tuple(int(x) for x in orc.philox4x32_10(counter, key)) == expect


def test_philox_known_answer_vectors_vectorised():
    """The same three vectors as one array call (the form seeded_draws uses)."""
    c = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    k = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    out = orc.philox4x32_10(c, k)
    for i in range(4):
        assert [int(x) for x in out[i]] == [kat[2][i] for kat in KAT]


# (seed, stream, idx): all four uniform lanes and both normal lanes, idx across multiples of 4, an index with a non-zero high
# word, the renderer's first seeds, a seed with a non-zero high word, the largest seed
HOST_CASES = [(seed, stream, idx)
              for seed in (0, 42, 1234 + 7919, 4321 + 7919, 2 ** 40 + 7, 2 ** 63 + 2 ** 32 + 5, 2 ** 64 - 1)
              for stream in (orc.STREAM_COARSE, orc.STREAM_FINE, orc.STREAM_FINE2, orc.STREAM_DEPTH)
              for idx in (0, 1, 2, 3, 4, 5, 6, 7, 8, 1023, 1024, 1025, 99991, 2 ** 32 + 6, 2 ** 33 + 3)]

HOST_MAIN = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "pny_rng.h"
int main(int argc, char** argv) {
    static const unsigned ids[4] = {pny::STREAM_COARSE, pny::STREAM_FINE, pny::STREAM_FINE2, pny::STREAM_DEPTH};
    printf("streams %u %u %u %u\n", ids[0], ids[1], ids[2], ids[3]);
    FILE* f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) return 2;
    unsigned long long seed, idx;
    unsigned stream;
    while (fscanf(f, "%llu %u %llu", &seed, &stream, &idx) == 3) {   // one `seed stream idx` per line
        uint32_t r[4];
        pny::Philox(seed).draw(idx, stream, r);   // the raw words of COUNTER idx
        printf("%08x %08x %08x %08x %a %a\n", r[0], r[1], r[2], r[3], (double)pny::uniform_at(seed, stream, idx),
               (double)pny::normal_at(seed, stream, idx));
    }
    return 0;
}
"""


def test_kernel_header_on_the_host_equals_the_oracle(tmp_path):
    """csrc/pny_rng.h itself, compiled by g++ (an empty hip/hip_runtime.h, __device__ defined away, no fused multiply-add):
    raw words and uniforms equal the oracle's exactly; the fp32 Box-Muller normal (glibc's logf / cosf / sqrtf here) is within
    NORMAL_ABS_TOL of the float64 value.  Measured: max |g - g64| = 7.9e-7 over the 420 cases (the
    kernels on the MI355X: 1.6e-6 over 5 x 2^16 normals, tests/test_gpu_seeded.py)."""
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("")
    lines = host_header_program(tmp_path, HOST_MAIN, include_dirs=(tmp_path, CSRC))(["%d %d %d" % case for case in HOST_CASES])
    assert lines[0] == "streams %d %d %d %d" % (orc.STREAM_COARSE, orc.STREAM_FINE, orc.STREAM_FINE2, orc.STREAM_DEPTH)
    assert len(lines) == 1 + len(HOST_CASES)
    worst = 0.0
    for (seed, stream, idx), line in zip(HOST_CASES, lines[1:]):
        f = line.split()
        words = tuple(int(x, 16) for x in f[:4])
        ref = orc.philox4x32_10((idx & 0xFFFFFFFF, idx >> 32, stream, orc.PHILOX_COUNTER3), (seed & 0xFFFFFFFF, seed >> 32))
        assert words == tuple(int(x) for x in ref), (seed, stream, idx)
        u = orc.philox_uniform(seed, stream, idx)
        assert u.dtype == np.float32 and float.fromhex(f[4]) == float(u), (seed, stream, idx, f[4], float(u))
        g64, g32 = orc.philox_normal(seed, stream, idx)
        err = abs(float.fromhex(f[5]) - float(g64))
        worst = max(worst, err)
        assert err <= NORMAL_ABS_TOL, (seed, stream, idx, f[5], float(g64))
        assert abs(float(g32) - float(g64)) <= 2.0 ** -22      # the fp32 rounding of a value below 8
    print("host build of pny_rng.h: max |normal_at - float64| = %.3e over %d cases" % (worst, len(HOST_CASES)))


def test_uniform_and_normal_pick_the_documented_lanes():
    """uniform idx = word idx % 4 of counter idx // 4; normal idx = words 2 (idx % 2), 2 (idx % 2) + 1 of counter idx // 2."""
    seed = 2 ** 40 + 7
    for idx in (0, 1, 2, 3, 4, 7, 2 ** 32 + 5):
        w = orc.philox4x32_10(((idx >> 2) & 0xFFFFFFFF, idx >> 34, orc.STREAM_FINE, orc.PHILOX_COUNTER3), (seed & 0xFFFFFFFF, seed >> 32))
        assert float(orc.philox_uniform(seed, orc.STREAM_FINE, idx)) == (int(w[idx & 3]) >> 8) / 2.0 ** 24
        w = orc.philox4x32_10(((idx >> 1) & 0xFFFFFFFF, idx >> 33, orc.STREAM_DEPTH, orc.PHILOX_COUNTER3), (seed & 0xFFFFFFFF, seed >> 32))
        u1, u2 = orc.philox_normal_inputs(seed, orc.STREAM_DEPTH, idx)
        assert float(u1) == 1.0 - (int(w[2 * (idx & 1)]) >> 8) / 2.0 ** 24 and float(u2) == (int(w[2 * (idx & 1) + 1]) >> 8) / 2.0 ** 24


def test_seeded_draws_layout_and_ranges():
    seed, kc, kf, kfd = 1234 + 7919, 33, 31, 7
    a, b = orc.seeded_draws(seed, 5, kc, kf, kfd), orc.seeded_draws(seed, 41, kc, kf, kfd)
    assert a["u_coarse"].shape == (5, kc) and a["u_fine"].shape == a["u_fine2"].shape == (5, kf - kfd) and a["g_depth"].shape == (5, kfd)
    for k in a:      # a draw at (ray, column) does not depend on the number of rays
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k][:5]), k
    # the layouts, written out: draw (ray, column) sits at stream position ray * columns + column
    assert float(b["u_coarse"][17, 5]) == float(orc.philox_uniform(seed, orc.STREAM_COARSE, 17 * kc + 5))
    assert float(b["u_fine"][40, 23]) == float(orc.philox_uniform(seed, orc.STREAM_FINE, 40 * (kf - kfd) + 23))
    assert float(b["u_fine2"][40, 23]) == float(orc.philox_uniform(seed, orc.STREAM_FINE2, 40 * (kf - kfd) + 23))
    assert float(b["g_depth"][9, 6]) == float(orc.philox_normal(seed, orc.STREAM_DEPTH, 9 * kfd + 6)[1])
    # four different streams: no equal entries at equal stream position
    n = 4096
    idx = np.arange(n)
    u = [orc.philox_uniform(seed, s, idx) for s in (orc.STREAM_COARSE, orc.STREAM_FINE, orc.STREAM_FINE2, orc.STREAM_DEPTH)]
    for i in range(4):
        assert float(u[i].min()) >= 0.0 and float(u[i].max()) < 1.0
        assert abs(float(u[i].mean()) - 0.5) < 4 * (1 / 12.0 / n) ** 0.5
        for j in range(i + 1, 4):
            assert not bool((u[i] == u[j]).any()), (i, j)        # (24-bit values: a chance match has probability 2^-12 per pair of streams)
            assert abs(float(np.corrcoef(u[i], u[j])[0, 1])) < 4 / n ** 0.5
    assert not np.array_equal(orc.seeded_draws(seed, 5, kc, kf, kfd)["u_coarse"], orc.seeded_draws(seed + 1, 5, kc, kf, kfd)["u_coarse"])
    # the high key word matters
    assert not np.array_equal(orc.philox_uniform(7, 1, idx), orc.philox_uniform(2 ** 32 + 7, 1, idx))
    u1, u2 = orc.philox_normal_inputs(seed, orc.STREAM_DEPTH, np.arange(1 << 16))
    assert float(u1.min()) > 0.0 and float(u1.max()) <= 1.0 and float(u2.min()) >= 0.0 and float(u2.max()) < 1.0
    g64, g32 = orc.philox_normal(seed, orc.STREAM_DEPTH, np.arange(1 << 16))
    assert g32.dtype == np.float32 and float(np.abs(g64).max()) <= (2 * 24 * np.log(2.0)) ** 0.5
    assert abs(float(g64.mean())) < 4 / 256.0 and abs(float(g64.var()) - 1.0) < 4 * (2.0 / 65536) ** 0.5
    # no fine pass / no depth samples: empty tensors of the right shape
    e = orc.seeded_draws(seed, 3, 16, 0, 0)
    assert e["u_fine"].shape == (3, 0) and e["g_depth"].shape == (3, 0)


def test_seeded_backward_case_has_enough_unambiguous_rays():
    """Precondition of tests/test_gpu_seeded.py's gradient comparisons, from the oracle alone: of the candidate rays rendered on
    the seed the renderer will use, at least half and at least 48 have every relu input outside the margin."""
    from helpers import SEEDED_BWD, seeded_bwd_case
    _, _, rays, draws, weight, seed = seeded_bwd_case(with_net=False)
    assert seed == SEEDED_BWD["base_seed"] + 7919 and rays.shape[0] == SEEDED_BWD["n"]
    n_clean = int(weight.sum())
    assert n_clean >= 48 and 2 * n_clean >= rays.shape[0], n_clean
