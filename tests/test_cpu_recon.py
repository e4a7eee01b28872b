"""
The mesh extraction without a GPU (include/pnyolo.h pny_grid_points / pny_mc_*, pixel_nerf_yolo_amd.recon, csrc/mc_table.h):

  * the committed case table: regenerating it reproduces the file byte for byte; for all 256 cases it uses exactly the cut
    edges, closes inside the cell up to the face segments, draws on every face segments that depend on the face's four corner
    bits only and that the neighbouring cell sees reversed (no cracks); cases 0 and 255 are empty;
  * the restatement the GPU tests compare against (tests/recon_ref.py) on analytic fields -- closed 2-manifolds of Euler
    characteristic 2, 0 and 4 with positive volume, the ball's vertices within a cell diagonal of its surface -- and on random
    fields, where only "every directed edge as often as its reverse" holds (a fan diagonal can lie in a shared ambiguous face);
  * the kernels' own arithmetic and table (csrc/pny_recon.h and csrc/mc_table.h compiled by g++ into a sequential marching
    cubes) against the restatement, bit for bit; its grid against numpy's linspace; the workspace layout;
  * the C ABI: declared, bound, exported, still version 11, still strict C99, every listed refusal before any launch;
  * save_obj: the bytes of a literal restatement of the reference's loop.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import recon_ref as rr
from host_tools import CSRC, ROOT, built_lib, c99_program, header_code, host_header_program  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import recon as precon

TABLE_H = os.path.join(CSRC, "mc_table.h")


@pytest.fixture(scope="module")
def header_table():
    """(constants, MC_NUM_TRIS, triangles per case as lists of edge triples) of the committed header."""
    consts, counts, rows = rr.parse_header(open(TABLE_H).read())
    tris = []
    for row in rows:
        used = [int(e) for e in row if e >= 0]
        assert len(used) % 3 == 0 and list(row[len(used):]) == [-1] * (len(row) - len(used)) and len(used) < len(row)
        tris.append([tuple(used[i:i + 3]) for i in range(0, len(used), 3)])
    return consts, counts, tris


# --------------------------------------------------------------------------- the table
def test_regenerating_the_table_reproduces_the_committed_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mc_table
    finally:
        sys.path.pop(0)
    assert gen_mc_table.render(gen_mc_table.build()) == open(TABLE_H).read()


def test_header_constants_and_the_restated_table(header_table):
    consts, counts, tris = header_table
    ref_tris, ref_rows, ref_counts = rr.table()
    assert tris == ref_tris and (counts == ref_counts).all()
    assert consts == {"MC_MAX_TRIS": int(ref_counts.max()), "MC_ROW": ref_rows.shape[1], "MC_TOTAL_TRIS": int(ref_counts.sum())}
    print("table: at most %d triangles per case, %d in all" % (consts["MC_MAX_TRIS"], consts["MC_TOTAL_TRIS"]))
    assert tris[0] == [] and tris[255] == []


def cut_edges(case):
    return {e for e, (a, b) in enumerate(rr.EDGES) if ((case >> a) ^ (case >> b)) & 1}


def test_every_case_uses_exactly_its_cut_edges(header_table):
    _, counts, tris = header_table
    for case in range(256):
        assert {e for t in tris[case] for e in t} == cut_edges(case), case
        assert counts[case] == len(tris[case])
        assert all(len(set(t)) == 3 for t in tris[case]), case


def boundary_edges(tris):
    """Directed triangle edges not matched by their reverse inside the cell (each directed edge may occur once)."""
    d = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(d)) == len(d), "a directed edge twice"
    return {e for e in d if (e[1], e[0]) not in d}


def test_triangles_close_inside_the_cell_up_to_the_face_segments(header_table):
    """Every directed triangle edge that is not a face segment is matched by its reverse (the fan diagonals), and every face
    segment is the edge of exactly one triangle."""
    _, _, tris = header_table
    for case in range(256):
        segs = [s for face in rr.FACES for s in rr.face_segments(case, face)]
        assert len(set(segs)) == len(segs)
        assert boundary_edges(tris[case]) == set(segs), case


def segments_on_face(tris, face):
    """The table's boundary edges that lie in `face`."""
    _, _, edges = face
    return {(a, b) for a, b in boundary_edges(tris) if a in edges and b in edges}


def test_face_segments_depend_on_the_face_only_and_the_neighbour_sees_them_reversed(header_table):
    """The no-cracks condition, on the committed table: per face and per pattern of its four corner bits the boundary edges in
    that face are the same in all 16 cases that show the pattern, every boundary edge lies in a face, and the cell across the
    face (same corners, same edges, opposite normal) has them reversed."""
    _, _, tris = header_table
    per_face = []
    for face in rr.FACES:
        _, corners, _ = face
        seen = {}
        for case in range(256):
            pattern = tuple((case >> c) & 1 for c in corners)
            segs = segments_on_face(tris[case], face)
            assert seen.setdefault(pattern, segs) == segs, (corners, pattern, case)
        assert len(seen) == 16
        per_face.append(seen)
    for case in range(256):
        in_faces = set().union(*[segments_on_face(tris[case], f) for f in rr.FACES])
        assert in_faces == boundary_edges(tris[case]), case
    edge_id = {frozenset(e): i for i, e in enumerate(rr.EDGES)}
    for d in range(3):
        lo, hi = rr.FACES[2 * d], rr.FACES[2 * d + 1]          # faces at offset 0 and 1 along d
        assert all(rr.CORNERS[c][d] == 0 for c in lo[1]) and all(rr.CORNERS[c][d] == 1 for c in hi[1])
        across = {e: edge_id[frozenset(c ^ (1 << d) for c in rr.EDGES[e])] for e in hi[2]}    # this cell's hi face = the next cell's lo face
        for pattern, segs in per_face[2 * d + 1].items():
            inside_next = {c ^ (1 << d) for c, bit in zip(hi[1], pattern) if bit}
            pattern_next = tuple(int(c in inside_next) for c in lo[1])
            assert {(across[b], across[a]) for a, b in segs} == per_face[2 * d][pattern_next], (d, pattern)


# --------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def analytic_meshes():
    out = {}
    for name, (field, iso, chi) in rr.ANALYTIC.items():
        f = field()
        out[name] = (f, rr.avoid_iso(f, iso), chi) + rr.extract_mesh(f, iso)
    return out


@pytest.mark.parametrize("name", sorted(rr.ANALYTIC))
def test_restatement_on_analytic_fields_gives_closed_oriented_manifolds(analytic_meshes, name):
    _, _, chi, v, t = analytic_meshes[name]
    vol = rr.signed_volume(v, t)
    print("%s: %d vertices, %d triangles, Euler %d, signed volume %.3f cells" % (name, len(v), len(t), rr.euler_characteristic(len(v), t), vol))
    assert len(t) > 0 and t.dtype == np.int32 and v.dtype == np.float32
    assert sorted(set(t.reshape(-1).tolist())) == list(range(len(v)))          # welded: every vertex used, none missing
    assert rr.is_closed_manifold(t)
    assert rr.euler_characteristic(len(v), t) == chi
    assert vol > 0.0


def test_restated_ball_vertices_lie_within_a_cell_diagonal_of_the_surface(analytic_meshes):
    _, iso, _, v, _ = analytic_meshes["ball"]
    diagonal = float(np.linalg.norm(2.0 / (np.array(rr.ANALYTIC_DIMS) - 1.0)))
    r = np.linalg.norm(rr.to_unit(v, rr.ANALYTIC_DIMS) - rr.BALL_CENTRE, axis=1)
    worst = float(np.abs(r - (rr.BALL_RADIUS - float(iso))).max())
    print("ball: vertices within %.4f of the surface, cell diagonal %.4f" % (worst, diagonal))
    assert worst < diagonal


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_restatement_on_random_fields_is_balanced(seed):
    f = rr.random_field(seed)
    v, t = rr.extract_mesh(f, rr.avoid_iso(f, 0.1))
    print("seed %d: %d vertices, %d triangles, closed manifold: %s" % (seed, len(v), len(t), rr.is_closed_manifold(t)))
    assert len(t) > 0 and rr.is_balanced(t)
    assert sorted(set(t.reshape(-1).tolist())) == list(range(len(v)))


def test_restated_grid_is_numpys_and_the_origin_has_no_direction():
    g = rr.gen_grid((-1, -0.5, 0.25), (1, 2, 0.75), (5, 4, 3))
    assert g.shape == (60, 3) and g.dtype == np.float32
    assert (g[:3, 2] == np.linspace(0.25, 0.75, 3, dtype=np.float32)).all() and (g[::12, 0] == np.linspace(-1, 1, 5, dtype=np.float32)).all()
    d = rr.view_dirs(rr.gen_grid((-1, -1, -1), (1, 1, 1), (3, 3, 3)))
    assert np.isfinite(d).all() and (d[13] == 0).all() and abs(float(np.linalg.norm(d[0])) - 1.0) < 1e-6


# --------------------------------------------------------------------------- the kernels' header on the host
HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pny_recon.h"
#include "mc_table.h"
using namespace pny;
// one query per input line:
// M in out   : int32 X Y Z, float iso, X*Y*Z floats  ->  int32 V T, V*3 floats, T*3 int32 (a sequential marching cubes)
// G in out   : int32 X Y Z, 6 doubles c1 c2          ->  X*Y*Z*6 floats (xyz, dirs)
// L X Y Z    : prints the workspace layout
static unsigned cuts(const std::vector<float>& s, int X, int Y, int Z, int x, int y, int z, float iso) {
    const size_t p = ((size_t)x * Y + y) * Z + z;
    const bool in = mc_inside(s[p], iso);
    unsigned m = 0;
    if (x + 1 < X && mc_inside(s[p + (size_t)Y * Z], iso) != in) m |= 1u;
    if (y + 1 < Y && mc_inside(s[p + Z], iso) != in) m |= 2u;
    if (z + 1 < Z && mc_inside(s[p + 1], iso) != in) m |= 4u;
    return m;
}
static int query(int argc, char** argv) {
    if (argc < 3) return 2;
    if (argv[1][0] == 'L') {
        const McLayout l = mc_layout(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        printf("%lld %lld %lld %zu %zu %zu %zu %zu\n", (long long)l.n_points, (long long)l.n1, (long long)l.n2, l.voff, l.toff, l.sums1,
               l.sums2, l.bytes);
        return 0;
    }
    FILE* f = fopen(argv[2], "rb");
    FILE* o = fopen(argv[3], "wb");
    if (!f || !o) return 3;
    int32_t d[3];
    if (fread(d, 4, 3, f) != 3) return 4;
    const int X = d[0], Y = d[1], Z = d[2];
    const size_t n = (size_t)X * Y * Z;
    if (argv[1][0] == 'G') {
        double c[6];
        if (fread(c, 8, 6, f) != 6) return 4;
        const int sz[3] = {X, Y, Z};
        double step[3];
        for (int k = 0; k < 3; ++k) step[k] = (c[3 + k] - c[k]) / (double)(sz[k] - 1);
        for (int x = 0; x < X; ++x)
            for (int y = 0; y < Y; ++y)
                for (int z = 0; z < Z; ++z) {
                    float v[6];
                    v[0] = grid_coord(x, X, c[0], step[0], c[3]), v[1] = grid_coord(y, Y, c[1], step[1], c[4]);
                    v[2] = grid_coord(z, Z, c[2], step[2], c[5]);
                    grid_dir(v[0], v[1], v[2], v[3], v[4], v[5]);
                    fwrite(v, 4, 6, o);
                }
        fclose(o);
        return 0;
    }
    float iso;
    std::vector<float> s(n);
    if (fread(&iso, 4, 1, f) != 1 || fread(s.data(), 4, n, f) != n) return 4;
    std::vector<int32_t> first(n);
    std::vector<float> verts;
    for (int x = 0; x < X; ++x)
        for (int y = 0; y < Y; ++y)
            for (int z = 0; z < Z; ++z) {
                const size_t p = ((size_t)x * Y + y) * Z + z;
                first[p] = (int32_t)(verts.size() / 3);
                const unsigned m = cuts(s, X, Y, Z, x, y, z, iso);
                const float fx = (float)x, fy = (float)y, fz = (float)z;
                if (m & 1u) verts.push_back(mc_cut(x, s[p], s[p + (size_t)Y * Z], iso)), verts.push_back(fy), verts.push_back(fz);
                if (m & 2u) verts.push_back(fx), verts.push_back(mc_cut(y, s[p], s[p + Z], iso)), verts.push_back(fz);
                if (m & 4u) verts.push_back(fx), verts.push_back(fy), verts.push_back(mc_cut(z, s[p], s[p + 1], iso));
            }
    std::vector<int32_t> tris;
    for (int x = 0; x + 1 < X; ++x)
        for (int y = 0; y + 1 < Y; ++y)
            for (int z = 0; z + 1 < Z; ++z) {
                unsigned cs = 0;
                for (int c = 0; c < 8; ++c)
                    if (mc_inside(s[((size_t)(x + (c & 1)) * Y + (y + ((c >> 1) & 1))) * Z + (z + (c >> 2))], iso)) cs |= 1u << c;
                int k = 0;
                for (; k < MC_ROW && MC_TRI_TABLE[cs][k] >= 0; ++k) {
                    int dx, dy, dz, axis;
                    mc_edge(MC_TRI_TABLE[cs][k], dx, dy, dz, axis);
                    const unsigned m = cuts(s, X, Y, Z, x + dx, y + dy, z + dz, iso);
                    if (!(m & (1u << axis))) return 5;
                    tris.push_back(first[((size_t)(x + dx) * Y + (y + dy)) * Z + (z + dz)] + __builtin_popcount(m & ((1u << axis) - 1u)));
                }
                if (k != 3 * MC_NUM_TRIS[cs]) return 6;
            }
    int32_t counts[2] = {(int32_t)(verts.size() / 3), (int32_t)(tris.size() / 3)};
    fwrite(counts, 4, 2, o);
    fwrite(verts.data(), 4, verts.size(), o);
    fwrite(tris.data(), 4, tris.size(), o);
    fclose(o);
    return 0;
}
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) return 2;
    static char line[4096];
    while (fgets(line, sizeof line, f)) {
        char* a[8] = {argv[0]};
        int n = 1;
        for (char* t = strtok(line, " \n"); t && n < 8; t = strtok(0, " \n")) a[n++] = t;
        const int rc = query(n, a);
        if (rc) return rc;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_header(tmp_path_factory):
    """csrc/pny_recon.h and csrc/mc_table.h compiled by g++: __host__ / __device__ defined away, no fused multiply-add."""
    tmp = tmp_path_factory.mktemp("recon_host")
    return host_header_program(tmp, HOST_MAIN, defines=("__device__=", "__host__=", "__forceinline__=inline"), include_dirs=(CSRC,)), tmp


def host_mesh(host_header, field, iso):
    run, tmp = host_header
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array(field.shape, dtype=np.int32).tobytes() + np.float32(iso).tobytes() + np.ascontiguousarray(field, dtype=np.float32).tobytes())
    run(["M %s %s" % (fin, fout)])
    raw = open(fout, "rb").read()
    nv, nt = np.frombuffer(raw[:8], dtype=np.int32)
    v = np.frombuffer(raw[8:8 + 12 * nv], dtype=np.float32).reshape(-1, 3)
    t = np.frombuffer(raw[8 + 12 * nv:], dtype=np.int32).reshape(-1, 3)
    assert len(t) == nt
    return v, t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_header_arithmetic_and_table_give_the_restated_mesh_bit_for_bit(host_header, analytic_meshes):
    for name, (f, iso, _, v, t) in analytic_meshes.items():
        hv, ht = host_mesh(host_header, f, iso)
        assert same_bits(hv, v) and same_bits(ht, t), name
    for seed in (1, 4):
        f = rr.random_field(seed)
        v, t = rr.extract_mesh(f, 0.1)
        hv, ht = host_mesh(host_header, f, 0.1)
        assert same_bits(hv, v) and same_bits(ht, t), seed
    for case in range(256):
        f = rr.single_cell(case)
        v, t = rr.extract_mesh(f, 0.25)
        hv, ht = host_mesh(host_header, f, 0.25)
        assert same_bits(hv, v) and same_bits(ht, t) and len(t) == rr.table()[2][case], case


def test_header_grid_is_numpys_linspace_bit_for_bit(host_header):
    run, tmp = host_header
    for c1, c2, reso in (((-1, -0.5, 0.25), (1, 2, 0.75), (5, 4, 3)), ((-1, -1, -1), (1, 1, 1), (3, 3, 3)),
                         ((-0.3, 0.1, -7.7), (0.9, 0.30000001, 1e-3), (128, 7, 33))):
        fin, fout = str(tmp / "g.bin"), str(tmp / "g_out.bin")
        with open(fin, "wb") as f:
            f.write(np.array(reso, dtype=np.int32).tobytes() + np.array(c1 + c2, dtype=np.float64).tobytes())
        run(["G %s %s" % (fin, fout)])
        got = np.fromfile(fout, dtype=np.float32).reshape(-1, 6)
        grid = rr.gen_grid(c1, c2, reso)
        assert same_bits(np.ascontiguousarray(got[:, :3]), grid), reso
        assert same_bits(np.ascontiguousarray(got[:, 3:]), rr.view_dirs(grid)), reso


def test_workspace_layout(host_header, built_lib):
    run, _ = host_header
    for dims in ((2, 2, 2), (17, 15, 13), (32, 32, 1024 // 32 + 1), (128, 128, 65), (1024, 1024, 682)):
        got = [int(v) for v in run(["L %d %d %d" % dims])[0].split()]
        n = dims[0] * dims[1] * dims[2]
        n1 = -(-n // plib.MC_SCAN_TILE)
        n2 = -(-n1 // plib.MC_SCAN_TILE) if n1 > plib.MC_SCAN_TILE else 0
        up = lambda b: -(-b // 256) * 256  # noqa: E731
        assert got[:3] == [n, n1, n2] and n2 <= plib.MC_SCAN_TILE
        assert got[3:] == [0, up(4 * n), 2 * up(4 * n), 2 * up(4 * n) + up(8 * n1), 2 * up(4 * n) + up(8 * n1) + up(8 * n2)]
        assert precon.workspace_bytes(dims) == got[-1]


# --------------------------------------------------------------------------- the C ABI
def test_entries_are_declared_bound_and_exported():
    """The entries' exact parameter lists (declared, bound, exported, the argument counts: tests/test_cpu_abi.py)."""
    flat = re.sub(r"\s+", "", header_code())
    decls = {
        "pny_grid_points": ["const double* c1_host", "const double* c2_host", "const int32_t* reso_host", "int64_t i0", "int64_t i1",
                            "float* xyz_dev", "float* dirs_dev", "pny_stream stream"],
        "pny_mc_workspace_bytes": ["const int32_t* dims_host", "int64_t* bytes"],
        "pny_mc_count": ["const float* sigma_dev", "const int32_t* dims_host", "float iso", "void* workspace_dev", "int32_t* counts_dev",
                         "pny_stream stream"],
        "pny_mc_emit": ["const float* sigma_dev", "const int32_t* dims_host", "float iso", "const void* workspace_dev", "int64_t n_vertices",
                        "int64_t n_triangles", "float* vertices_dev", "int32_t* triangles_dev", "pny_stream stream"],
    }
    for name, args in decls.items():
        assert "int" + name + "(" + ",".join(arg.replace(" ", "") for arg in args) + ");" in flat, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " recon.hip" in mk and " recon_api.hip" in mk and " pny_recon.h" in mk and " mc_table.h" in mk


C99_MAIN = r"""
#include <stdio.h>
#include "pnyolo.h"
int main(void) {
    int (*a)(const double*, const double*, const int32_t*, int64_t, int64_t, float*, float*, pny_stream) = pny_grid_points;
    int (*b)(const int32_t*, int64_t*) = pny_mc_workspace_bytes;
    int (*c)(const float*, const int32_t*, float, void*, int32_t*, pny_stream) = pny_mc_count;
    int (*d)(const float*, const int32_t*, float, const void*, int64_t, int64_t, float*, int32_t*, pny_stream) = pny_mc_emit;
    printf("%d\n", a != 0 && b != 0 && c != 0 && d != 0);
    return 0;
}
"""


def test_header_is_strict_c99(built_lib, tmp_path):
    """Every entry has exactly the C type a host would write for it."""
    run = c99_program(tmp_path, C99_MAIN, link=True)()
    assert run.returncode == 0 and run.stdout.split() == ["1"], (run.returncode, run.stdout, run.stderr)


def test_grid_points_refuses_bad_arguments_before_any_launch(built_lib):
    """PNY_ERR_ARG (-1) with a message, whether or not a GPU is there (the device pointers are never dereferenced by the host)."""
    call, err = built_lib.pny_grid_points, built_lib.pny_last_error
    p, p2 = C.c_void_p(4096), C.c_void_p(8192)
    d3, i3 = C.c_double * 3, C.c_int32 * 3

    def rc(c1=(-1, -1, -1), c2=(1, 1, 1), reso=(5, 4, 3), i0=0, i1=60, xyz=p, dirs=p2):
        return call(None if c1 is None else d3(*c1), None if c2 is None else d3(*c2), None if reso is None else i3(*reso), i0, i1, xyz, dirs, None)

    for kw in (dict(c1=None), dict(c2=None), dict(reso=None), dict(xyz=None), dict(dirs=None)):
        assert rc(**kw) == -1 and b"null" in err(), kw
    for reso in ((1, 4, 3), (5, 0, 3), (5, 4, -2)):
        assert rc(reso=reso) == -1 and b"at least 2" in err(), reso
    for kw in (dict(c2=(1, -1, 1)), dict(c2=(1, 1, -2)), dict(c1=(1, -1, -1))):
        assert rc(**kw) == -1 and b"above c1" in err(), kw
    for kw in (dict(c1=(float("nan"), -1, -1)), dict(c2=(1, float("inf"), 1)), dict(c1=(-1, -1, float("-inf")))):
        assert rc(**kw) == -1 and b"finite" in err(), kw
    for kw in (dict(i0=-1), dict(i1=61), dict(i0=7, i1=7), dict(i0=8, i1=7)):
        assert rc(**kw) == -1 and b"i0" in err(), kw
    assert rc(reso=(1024, 1024, 683), i1=10) == -1 and b"2^31" in err()
    assert rc(reso=(2 ** 20, 2 ** 20, 2 ** 20), i1=10) == -1 and b"2^31" in err()


def test_marching_cubes_entries_refuse_bad_arguments_before_any_launch(built_lib):
    err = built_lib.pny_last_error
    p, p2, p3, p4 = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))
    i3 = C.c_int32 * 3
    nbytes = C.c_int64(0)
    assert built_lib.pny_mc_workspace_bytes(None, C.byref(nbytes)) == -1 and b"null" in err()
    assert built_lib.pny_mc_workspace_bytes(i3(4, 4, 4), None) == -1 and b"null" in err()
    assert built_lib.pny_mc_workspace_bytes(i3(4, 1, 4), C.byref(nbytes)) == -1 and b"at least 2" in err()
    assert built_lib.pny_mc_workspace_bytes(i3(1024, 1024, 683), C.byref(nbytes)) == -1 and b"2^31" in err()
    assert built_lib.pny_mc_workspace_bytes(i3(1024, 1024, 682), C.byref(nbytes)) == 0 and nbytes.value > 8 * 1024 * 1024 * 682

    def count(sigma=p, dims=(4, 5, 6), iso=0.5, ws=p2, counts=p3):
        return built_lib.pny_mc_count(sigma, None if dims is None else i3(*dims), iso, ws, counts, None)

    def emit(sigma=p, dims=(4, 5, 6), iso=0.5, ws=p2, nv=3, nt=1, v=p3, t=p4):
        return built_lib.pny_mc_emit(sigma, None if dims is None else i3(*dims), iso, ws, nv, nt, v, t, None)

    for kw in (dict(sigma=None), dict(dims=None), dict(ws=None), dict(counts=None)):
        assert count(**kw) == -1 and b"null" in err(), kw
    for kw in (dict(sigma=None), dict(dims=None), dict(ws=None), dict(v=None), dict(t=None)):
        assert emit(**kw) == -1 and b"null" in err(), kw
    for fn in (count, emit):
        for dims in ((1, 5, 6), (4, 0, 6), (4, 5, -1)):
            assert fn(dims=dims) == -1 and b"at least 2" in err(), dims
        assert fn(dims=(1024, 1024, 683)) == -1 and b"2^31" in err()
        for iso in (float("nan"), float("inf"), float("-inf")):
            assert fn(iso=iso) == -1 and b"finite" in err(), iso
    assert emit(nv=-1) == -1 and b"negative" in err()
    assert emit(nt=-1) == -1 and b"negative" in err()
    assert emit(nv=3 * 120 + 1) == -1 and emit(nt=5 * 120 + 1) == -1 and b"more vertices or triangles" in err()
    # an empty mesh launches nothing and is no error: neither half has anything to write, and no pointer is needed
    assert emit(nv=0, nt=0, v=None, t=None) == 0


# --------------------------------------------------------------------------- Python
def reference_save_obj(vertices, triangles, path, vert_rgb=None):
    """The reference's loop (src/util/recon.py:90-106), restated line by line."""
    with open(path, "w") as file:
        if vert_rgb is None:
            for v in vertices:
                file.write("v %.4f %.4f %.4f\n" % (v[0], v[1], v[2]))
        else:
            for idx, v in enumerate(vertices):
                c = vert_rgb[idx]
                file.write("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (v[0], v[1], v[2], c[0], c[1], c[2]))
        for f in triangles:
            f_plus = f + 1
            file.write("f %d %d %d\n" % (f_plus[0], f_plus[1], f_plus[2]))


def test_save_obj_writes_the_references_bytes(tmp_path):
    v = np.array([[0.0, 1.5, -2.25], [1e-5, 0.12345, 0.12355], [3.0, -0.00004, 123456.789], [0.5, 0.25, 0.125], [-1.0, 2.0, 1.0 / 3.0]])
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 3]], dtype=np.int32)
    rgb = np.random.RandomState(3).rand(5, 3)
    for colours in (None, rgb):
        for vv in (v, v.astype(np.float32)):
            a, b = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
            precon.save_obj(vv, t, a, vert_rgb=colours)
            reference_save_obj(vv, t, b, vert_rgb=colours)
            assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 100
    import torch
    precon.save_obj(torch.from_numpy(v), torch.from_numpy(t), str(tmp_path / "c.obj"))
    reference_save_obj(v, t, str(tmp_path / "e.obj"))
    assert open(str(tmp_path / "c.obj"), "rb").read() == open(str(tmp_path / "e.obj"), "rb").read()
    with pytest.raises(ValueError, match="vert_rgb"):
        precon.save_obj(v, t, str(tmp_path / "d.obj"), vert_rgb=rgb[:4])


def test_python_refuses_by_name():
    import torch
    with pytest.raises(ValueError, match="reso"):
        precon.grid_points((-1, -1, -1), (1, 1, 1), (1, 4, 4))
    with pytest.raises(ValueError, match="c2 > c1"):
        precon.grid_points((-1, -1, -1), (1, -1, 1), (4, 4, 4))
    with pytest.raises(ValueError, match="three"):
        precon.grid_points((-1, -1), (1, 1, 1), (4, 4, 4))
    with pytest.raises(TypeError, match="tensor"):
        precon.extract_mesh(np.zeros((3, 3, 3), dtype=np.float32), 0.5)
    with pytest.raises(ValueError, match="contiguous fp32"):
        precon.extract_mesh(torch.zeros(3, 3, 3, dtype=torch.float64), 0.5)
    with pytest.raises(ValueError, match="contiguous fp32"):
        precon.extract_mesh(torch.zeros(3, 3), 0.5)
    with pytest.raises(plib.PnyError, match="no CPU path"):
        precon.extract_mesh(torch.zeros(3, 3, 3), 0.5)

    class NoScene:
        num_objs, d_out = 0, 4
    with pytest.raises(plib.PnyError, match="ONE encoded object"):
        precon.sigma_grid(NoScene(), reso=(4, 4, 4))
