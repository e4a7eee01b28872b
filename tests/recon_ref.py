"""
The mesh extraction restated in vectorised numpy (csrc/pny_recon.h's conventions, sharing no code with the kernels or with
tools/gen_mc_table.py): the case table derived again from the cube's geometry, the grid of util.gen_grid with the fp32 view
directions, marching cubes with the library's ordering and fp32 vertex formula (bit-comparable), the analytic fields the tests
use, and the mesh property checks.
"""
import itertools

import numpy as np

# --------------------------------------------------------------------------- the cube
CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])


def _edges():
    """Per edge id 4 * axis + k: (owner corner, other corner).  The owner is the lower end; k holds the owner's two other
    offsets, lower axis in bit 0."""
    out = []
    for axis in range(3):
        rest = [a for a in range(3) if a != axis]
        for k in range(4):
            off = np.zeros(3, dtype=int)
            off[rest[0]], off[rest[1]] = k & 1, k >> 1
            a = int(off @ [1, 2, 4])
            out.append((a, a + (1 << axis)))
    return out


EDGES = _edges()
EDGE_OWNER_OFFSET = np.array([CORNERS[a] for a, _ in EDGES])       # (12, 3)
EDGE_AXIS = np.arange(12) // 4
EDGE_MID2 = np.array([CORNERS[a] + CORNERS[b] for a, b in EDGES])  # twice the midpoint


def _faces():
    """Per face: (outward normal, its four corners, its four edges)."""
    out = []
    for d, side in itertools.product(range(3), (0, 1)):
        corners = [c for c in range(8) if CORNERS[c][d] == side]
        edges = [e for e, (a, b) in enumerate(EDGES) if a in corners and b in corners]
        n = np.zeros(3, dtype=int)
        n[d] = 2 * side - 1
        out.append((n, corners, edges))
    return out


FACES = _faces()


def _orient(n, e0, e1, inside):
    """e0 -> e1 or e1 -> e0: the inside corners the segment separates from the rest lie on its right, seen from outside the cell
    (all of them lie on one side, so their summed side decides)."""
    p, q = EDGE_MID2[e0], EDGE_MID2[e1]
    s = sum(int(np.dot(np.cross(n, q - p), 2 * CORNERS[c] - p)) for c in inside)
    assert s != 0
    return (e0, e1) if s < 0 else (e1, e0)


def face_segments(case, face):
    """Directed segments of one face of one case: a function of the face's four corner bits."""
    n, corners, edges = face
    inside = [c for c in corners if (case >> c) & 1]
    cut = [e for e in edges if ((case >> EDGES[e][0]) ^ (case >> EDGES[e][1])) & 1]
    if len(cut) == 0:
        return []
    if len(cut) == 2:
        return [_orient(n, cut[0], cut[1], inside)]
    assert len(cut) == 4 and len(inside) == 2
    segs = []
    for c in inside:              # cut the inside corner off: the two face edges that meet at it
        e0, e1 = [e for e in edges if c in EDGES[e]]
        segs.append(_orient(n, e0, e1, [c]))
    return segs


def case_triangles(case):
    follow = {}
    for face in FACES:
        for a, b in face_segments(case, face):
            assert a not in follow
            follow[a] = b
    assert set(follow) == set(follow.values())
    tris, left = [], set(follow)
    while left:
        start = min(left)
        loop = [start]
        left.discard(start)
        while follow[loop[-1]] != start:
            loop.append(follow[loop[-1]])
            left.discard(loop[-1])
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


_TABLE = None


def table():
    """(triangles per case as lists of edge triples, rows (256, 3 * max + 1) int8 ending in -1, counts (256,))."""
    global _TABLE
    if _TABLE is None:
        tris = [case_triangles(c) for c in range(256)]
        width = 3 * max(len(t) for t in tris) + 1
        rows = -np.ones((256, width), dtype=np.int8)
        for c, t in enumerate(tris):
            flat = [e for tri in t for e in tri]
            rows[c, :len(flat)] = flat
        _TABLE = (tris, rows, np.array([len(t) for t in tris]))
    return _TABLE


def parse_header(text):
    """MC_MAX_TRIS, MC_ROW, MC_TOTAL_TRIS, MC_NUM_TRIS (256,) and MC_TRI_TABLE (256, MC_ROW) of csrc/mc_table.h."""
    import re
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(MC_MAX_TRIS|MC_ROW|MC_TOTAL_TRIS)\s+(\d+)", code)}
    arrays = re.findall(r"\[\s*(?:256|MC_ROW)\s*\]\s*=\s*\{(.*?)\};", code, flags=re.S)
    nums = [np.array([int(v) for v in re.findall(r"-?\d+", a)]) for a in arrays]
    return consts, nums[0], nums[1].reshape(256, consts["MC_ROW"])


# --------------------------------------------------------------------------- the grid
def gen_grid(c1, c2, reso):
    """util.gen_grid(*zip(c1, c2, reso), ij_indexing=True) as numpy: (X Y Z, 3) fp32."""
    axes = [np.linspace(lo, hi, sz, dtype=np.float32) for lo, hi, sz in zip(c1, c2, reso)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def view_dirs(grid):
    """recon.py:54 in fp32, the norm summed left to right; the origin gets (0, 0, 0)."""
    g = grid.astype(np.float32)
    x, y, z = g[:, 0], g[:, 1], g[:, 2]
    n = np.sqrt((x * x + y * y) + z * z)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = -g / n[:, None]
    d[(g == 0).all(axis=1)] = 0.0
    return d.astype(np.float32)


# --------------------------------------------------------------------------- marching cubes
def extract_mesh(sigma, iso):
    """vertices (V, 3) fp32 in index coordinates and triangles (T, 3) int32 of an (X, Y, Z) fp32 volume, in the library's order."""
    s = np.ascontiguousarray(sigma, dtype=np.float32)
    iso = np.float32(iso)
    X, Y, Z = s.shape
    inside = s > iso
    cuts = np.zeros((X, Y, Z, 3), dtype=bool)
    cuts[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cuts[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cuts[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    key = np.flatnonzero(cuts.reshape(-1))                    # owner * 3 + axis, ascending
    owner, axis = key // 3, key % 3
    stride = np.array([Y * Z, Z, 1])
    flat = s.reshape(-1)
    a, b = flat[owner], flat[owner + stride[axis]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (iso - a) / (b - a)
    idx = np.stack(np.unravel_index(owner, (X, Y, Z)), axis=1)
    vertices = idx.astype(np.float32)
    along = vertices[np.arange(len(key)), axis] + t.astype(np.float32)
    vertices[np.arange(len(key)), axis] = along
    vid = -np.ones(X * Y * Z * 3, dtype=np.int64)
    vid[key] = np.arange(len(key))

    case = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << c
    _, rows, _ = table()
    cell_rows = rows[case.reshape(-1)]                         # (cells, width)
    used = cell_rows >= 0
    cell_of = np.repeat(np.arange(case.size), used.sum(axis=1))
    edge = cell_rows[used].astype(np.int64)                    # cell order, then table order
    cx, cy, cz = np.unravel_index(cell_of, case.shape)
    off = EDGE_OWNER_OFFSET[edge]
    own = ((cx + off[:, 0]) * Y + (cy + off[:, 1])) * Z + (cz + off[:, 2])
    tri = vid[own * 3 + EDGE_AXIS[edge]]
    assert (tri >= 0).all()
    return vertices.astype(np.float32), tri.reshape(-1, 3).astype(np.int32)


# --------------------------------------------------------------------------- fields
ANALYTIC_DIMS = (17, 15, 13)
BALL_CENTRE, BALL_RADIUS = np.array([0.07, -0.03, 0.05]), 0.6


def unit_grid(dims):
    """(X, Y, Z, 3) float64 points of linspace(-1, 1, .) per axis."""
    return np.stack(np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in dims], indexing="ij"), axis=-1)


def ball_field(dims=ANALYTIC_DIMS, centre=BALL_CENTRE, radius=BALL_RADIUS):
    return (radius - np.linalg.norm(unit_grid(dims) - centre, axis=-1)).astype(np.float32)


def torus_field(dims=ANALYTIC_DIMS, major=0.55, minor=0.2):
    p = unit_grid(dims)
    ring = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - major
    return (minor - np.sqrt(ring ** 2 + p[..., 2] ** 2)).astype(np.float32)


def two_balls_field(dims=ANALYTIC_DIMS):
    p = unit_grid(dims)
    a = 0.35 - np.linalg.norm(p - np.array([0.4, 0.0, 0.0]), axis=-1)
    b = 0.3 - np.linalg.norm(p - np.array([-0.45, 0.1, -0.1]), axis=-1)
    return np.maximum(a, b).astype(np.float32)


# name -> (field, iso, Euler characteristic)
ANALYTIC = {"ball": (ball_field, 0.013, 2), "torus": (torus_field, 0.011, 0), "two_balls": (two_balls_field, 0.007, 4)}


def random_field(seed, dims=(7, 6, 5), pad=-10.0):
    """A standard-normal field padded by one layer of `pad`."""
    inner = np.random.RandomState(seed).randn(*dims).astype(np.float32)
    return np.pad(inner, 1, constant_values=np.float32(pad))


def single_cell(case, lo=-1.0, hi=1.0):
    """The (2, 2, 2) volume of one case: corner c inside when bit c is set."""
    v = np.full((2, 2, 2), lo, dtype=np.float32)
    for c in range(8):
        if (case >> c) & 1:
            v[tuple(CORNERS[c])] = hi * (1.0 + 0.125 * c)      # different values: different cut positions
    return v


def avoid_iso(field, iso):
    """The isosurface tests use must not equal a sample (a cut would sit on a grid point)."""
    assert not (field == np.float32(iso)).any()
    return np.float32(iso)


# --------------------------------------------------------------------------- mesh properties
def directed_edges(tri):
    t = np.asarray(tri, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)


def _edge_counts(tri):
    e = directed_edges(tri)
    keys, counts = np.unique(e[:, 0] * (int(e.max()) + 1) + e[:, 1], return_counts=True)
    return e, keys, counts, int(e.max()) + 1


def is_closed_manifold(tri):
    """Every undirected edge lies in exactly two triangles, once per direction."""
    if len(tri) == 0:
        return True
    e, keys, counts, base = _edge_counts(tri)
    reverse = (keys % base) * base + keys // base
    return bool((counts == 1).all() and np.isin(reverse, keys).all() and (e[:, 0] != e[:, 1]).all())


def is_balanced(tri):
    """The weaker property: every directed edge occurs as often as its reverse."""
    if len(tri) == 0:
        return True
    _, keys, counts, base = _edge_counts(tri)
    fwd = dict(zip(keys.tolist(), counts.tolist()))
    return all(fwd.get((k % base) * base + k // base, 0) == n for k, n in fwd.items())


def euler_characteristic(n_vertices, tri):
    e = np.sort(directed_edges(tri), axis=1)
    return int(n_vertices) - len(np.unique(e, axis=0)) + len(tri)


def signed_volume(vertices, tri):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def to_unit(vertices, dims):
    """Index coordinates -> the coordinates of unit_grid(dims)."""
    return np.asarray(vertices, dtype=np.float64) * (2.0 / (np.array(dims) - 1.0)) - 1.0
