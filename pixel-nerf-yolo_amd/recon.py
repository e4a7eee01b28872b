"""
Mesh extraction on the library's kernels (csrc/recon.hip): the reference's src/util/recon.py, which samples sigma on a regular
grid through the network, moves every slab to the host and runs PyMCubes there.  Here the grid points are generated on the
device, the sigma volume stays there, and marching cubes is a handful of launches that give an indexed, welded mesh:

  sigma_grid(net, c1, c2, reso, ...)          -> (X, Y, Z) fp32 device tensor
  extract_mesh(sigma, isosurface)             -> vertices (V, 3) fp32, triangles (T, 3) int32, device, index coordinates
  marching_cubes(occu_net, c1, c2, reso, ...) -> the reference's call: numpy float64 vertices in world units, int32 triangles
  save_obj(vertices, triangles, path, ...)    -> the reference's OBJ file, byte for byte

Conventions (csrc/pny_recon.h): a grid point is inside when sigma > isosurface, strictly, so a NaN sigma is outside; every cut
grid edge carries one vertex, linearly interpolated in fp32, owned by the edge's lower end; vertices are ordered by owner, then
axis, triangles by cell, then table order; normals point out of the dense region.  The result has the same bits on every run.

Deliberate differences from the reference: the triangulation and the vertex order are this library's own (the vertex SET is
marching cubes': one per cut edge); a grid point exactly at the origin gets the view direction (0, 0, 0), not NaN; a sigma equal
to the isosurface gives zero-area triangles, which are kept.  fp32 tensors on an MI355X only; there is no CPU path and no
fallback.
"""
import ctypes as C
import warnings

import numpy as np
import torch

from . import lib as _lib
from .lib import check, stream_of

_WHO = "pixel_nerf_yolo_amd.recon"


def _triple(v, name, kind):
    try:
        out = [kind(x) for x in v]
    except (TypeError, ValueError):
        out = []
    if len(out) != 3:
        raise ValueError("%s: %s must hold three %ss, got %r" % (_WHO, name, kind.__name__, v))
    return out


def _grid_args(c1, c2, reso):
    c1, c2, reso = _triple(c1, "c1", float), _triple(c2, "c2", float), _triple(reso, "reso", int)
    if min(reso) < 2:
        raise ValueError("%s: every reso must be at least 2, got %s" % (_WHO, reso))
    if not all(np.isfinite(c1 + c2)) or not all(b > a for a, b in zip(c1, c2)):
        raise ValueError("%s: c1 and c2 must be finite with c2 > c1 on every axis, got %s and %s" % (_WHO, c1, c2))
    if reso[0] * reso[1] * reso[2] > _lib.MC_MAX_POINTS:
        raise ValueError("%s: reso %s has 2^31 / 3 points or more" % (_WHO, reso))
    return (C.c_double * 3)(*c1), (C.c_double * 3)(*c2), (C.c_int32 * 3)(*reso), reso


def grid_points(c1, c2, reso, i0=0, i1=None, device="cuda:0", out=None):
    """Flat indices [i0, i1) of ``util.gen_grid(*zip(c1, c2, reso), ij_indexing=True)`` and their fake view directions
    (recon.py:54; the origin gets (0, 0, 0)), one launch.
    :param out optional (xyz, dirs) pair of contiguous fp32 device tensors of at least (i1 - i0, 3); their first rows are written
    :return xyz (i1 - i0, 3), dirs (i1 - i0, 3) fp32 on the device"""
    a, b, r, reso = _grid_args(c1, c2, reso)
    n = reso[0] * reso[1] * reso[2]
    i1 = n if i1 is None else int(i1)
    i0 = int(i0)
    if not 0 <= i0 < i1 <= n:
        raise ValueError("%s: need 0 <= i0 < i1 <= %d, got %d and %d" % (_WHO, n, i0, i1))
    if out is None:
        dev = torch.device(device)
        xyz, dirs = (torch.empty(i1 - i0, 3, device=dev, dtype=torch.float32) for _ in range(2))
    else:
        xyz, dirs = out
        for t, what in ((xyz, "out[0]"), (dirs, "out[1]")):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < i1 - i0:
                raise ValueError("%s: %s must be a contiguous fp32 tensor of at least (%d, 3)" % (_WHO, what, i1 - i0))
        dev = xyz.device
    if dev.type != "cuda" or dirs.device != dev:
        raise _lib.PnyError("%s: the grid is written on an MI355X only (there is no CPU path)" % _WHO)
    with torch.cuda.device(dev):
        check(_lib.load().pny_grid_points(a, b, r, i0, i1, C.c_void_p(xyz.data_ptr()), C.c_void_p(dirs.data_ptr()), stream_of(dev)))
    return xyz[: i1 - i0], dirs[: i1 - i0]


def sigma_grid(net, c1=(-1, -1, -1), c2=(1, 1, 1), reso=(128, 128, 128), sigma_idx=3, eval_batch_size=100000, coarse=True):
    """Channel ``sigma_idx`` of ``net`` on the grid of recon.py:43, slab by slab of ``eval_batch_size`` points, with the fake view
    directions of recon.py:54.  Nothing goes to the host.  Needs a prior ``net.encode()`` of ONE object.
    :return (X, Y, Z) fp32 device tensor"""
    _, _, _, reso = _grid_args(c1, c2, reso)
    if getattr(net, "num_objs", 0) != 1:
        raise _lib.PnyError("%s.sigma_grid: net must hold ONE encoded object (call net.encode() with one object first); it holds %d"
                            % (_WHO, getattr(net, "num_objs", 0)))
    sigma_idx, bs = int(sigma_idx), int(eval_batch_size)
    if not 0 <= sigma_idx < net.d_out:
        raise ValueError("%s.sigma_grid: sigma_idx %d is outside the net's %d output channels" % (_WHO, sigma_idx, net.d_out))
    if bs < 1:
        raise ValueError("%s.sigma_grid: eval_batch_size must be positive, got %d" % (_WHO, bs))
    dev = net._device()
    n = reso[0] * reso[1] * reso[2]
    bs = min(bs, n)
    vol = torch.empty(n, device=dev, dtype=torch.float32)
    bufs = (torch.empty(bs, 3, device=dev, dtype=torch.float32), torch.empty(bs, 3, device=dev, dtype=torch.float32))
    with torch.no_grad():
        for i0 in range(0, n, bs):
            i1 = min(i0 + bs, n)
            xyz, dirs = grid_points(c1, c2, reso, i0, i1, out=bufs)
            out = net(xyz[None], coarse=coarse, viewdirs=dirs[None])
            vol[i0:i1].copy_(out[0, :, sigma_idx])
    return vol.view(*reso)


def extract_mesh(sigma, isosurface, workspace=None):
    """Marching cubes over a contiguous fp32 (X, Y, Z) device tensor.  The two counts are the one host read.
    :param workspace optional uint8 device tensor of at least ``workspace_bytes(sigma.shape)`` bytes to reuse between calls
    :return vertices (V, 3) fp32 in index coordinates, triangles (T, 3) int32, on sigma's device"""
    if not isinstance(sigma, torch.Tensor):
        raise TypeError("%s.extract_mesh: sigma must be a tensor, got %s" % (_WHO, type(sigma).__name__))
    if sigma.dtype != torch.float32 or sigma.dim() != 3 or not sigma.is_contiguous():
        raise ValueError("%s.extract_mesh: sigma must be a contiguous fp32 (X, Y, Z) tensor, got %s %s"
                         % (_WHO, sigma.dtype, tuple(sigma.shape)))
    if sigma.device.type != "cuda":
        raise _lib.PnyError("%s.extract_mesh: sigma is on %s; the extraction runs on an MI355X only (there is no CPU path)"
                            % (_WHO, sigma.device))
    dims = [int(v) for v in sigma.shape]
    if min(dims) < 2 or dims[0] * dims[1] * dims[2] > _lib.MC_MAX_POINTS:
        raise ValueError("%s.extract_mesh: every dimension must be at least 2 and 3 X Y Z below 2^31, got %s" % (_WHO, dims))
    iso = float(isosurface)
    if not np.isfinite(np.float32(iso)):
        raise ValueError("%s.extract_mesh: isosurface must be finite in fp32, got %r" % (_WHO, isosurface))
    sigma = sigma.detach()
    dev, L = sigma.device, _lib.load()
    need = workspace_bytes(dims)
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    elif (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != dev
          or workspace.data_ptr() % 256):
        raise ValueError("%s.extract_mesh: workspace must be a contiguous, 256-byte aligned uint8 tensor of at least %d bytes on %s"
                         % (_WHO, need, dev))
    d = (C.c_int32 * 3)(*dims)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        st = stream_of(dev)
        check(L.pny_mc_count(C.c_void_p(sigma.data_ptr()), d, iso, C.c_void_p(workspace.data_ptr()), C.c_void_p(counts.data_ptr()), st))
        nv, nt = (int(v) for v in counts.cpu())
        if nv < 0 or nt < 0:
            raise _lib.PnyError("%s.extract_mesh: the mesh has 2^31 triangles or more" % _WHO)
        vertices = torch.empty(nv, 3, device=dev, dtype=torch.float32)
        triangles = torch.empty(nt, 3, device=dev, dtype=torch.int32)
        check(L.pny_mc_emit(C.c_void_p(sigma.data_ptr()), d, iso, C.c_void_p(workspace.data_ptr()), nv, nt,
                            C.c_void_p(vertices.data_ptr()) if nv else None, C.c_void_p(triangles.data_ptr()) if nt else None, st))
    return vertices, triangles


def workspace_bytes(dims):
    """Bytes of the workspace ``extract_mesh`` needs for a (X, Y, Z) volume (pny_mc_workspace_bytes)."""
    d = (C.c_int32 * 3)(*[int(v) for v in dims])
    out = C.c_int64(0)
    check(_lib.load().pny_mc_workspace_bytes(d, C.byref(out)))
    return int(out.value)


class OccupancyGrid:
    """A bitfield over the cells of a sigma volume (csrc/pny_occupancy.h), as ``occupancy_grid`` builds it and
    ``net.set_occupancy`` attaches it: ``bits`` (uint32 device tensor, cell f = bit f & 31 of word f >> 5), ``dims`` (X, Y, Z grid
    points: (X - 1)(Y - 1)(Z - 1) cells), the box ``c1`` .. ``c2``, ``outside_empty``; ``n_cells`` and ``n_occupied`` (the count is
    on the device until first asked for: one host read)."""

    def __init__(self, bits, dims, c1, c2, outside_empty, occupied):
        self.bits, self.dims, self.c1, self.c2 = bits, tuple(int(v) for v in dims), tuple(float(v) for v in c1), tuple(float(v) for v in c2)
        self.outside_empty = bool(outside_empty)
        self.n_cells = (self.dims[0] - 1) * (self.dims[1] - 1) * (self.dims[2] - 1)
        self._occupied, self._n_occupied = occupied, None

    @property
    def n_occupied(self):
        if self._n_occupied is None:
            self._n_occupied = int(self._occupied.item())
        return self._n_occupied

    def __repr__(self):
        return "OccupancyGrid(dims=%s, c1=%s, c2=%s, outside_empty=%s)" % (self.dims, self.c1, self.c2, self.outside_empty)


def occupancy_words(dims):
    """uint32 words of the bitfield of a (X, Y, Z) volume (pny_occupancy_words)."""
    out = C.c_int64(0)
    check(_lib.load().pny_occupancy_words((C.c_int32 * 3)(*[int(v) for v in dims]), C.byref(out)))
    return int(out.value)


def _volume(v, dev, what):
    if not isinstance(v, torch.Tensor):
        v = torch.as_tensor(np.asarray(v, dtype=np.float32))
    v = v.detach().to(dev, torch.float32).contiguous()
    if v.dim() != 3 or min(v.shape) < 2:
        raise ValueError("%s.occupancy_grid: %s must be a (X, Y, Z) volume with every dimension at least 2, got %s"
                         % (_WHO, what, tuple(v.shape)))
    return v


def occupancy_grid(net, c1=(-1, -1, -1), c2=(1, 1, 1), reso=(128, 128, 128), *, sigma_thresh, dilate=1, outside_empty=False,
                   eval_batch_size=100000, sigma=None):
    """The occupancy grid of ONE encoded object for ``net.set_occupancy``: the cells of the box c1 .. c2 where no-grad renders may
    skip the MLP (csrc/pny_occupancy.h).  A cell is occupied when any of its 8 corners has ``not sigma <= sigma_thresh`` (a NaN is
    occupied) in the coarse MLP's volume or, when the net has ``mlp_fine``, in the fine MLP's, or when a cell within Chebyshev
    distance ``dilate`` (0 .. 4) is.  Without ``sigma`` the volumes come from ``sigma_grid`` (``coarse=True``, and ``coarse=False``
    with a fine MLP).
    WARNING (marching_cubes' own): sigma depends on the view direction here, and the grid is learnt on fake directions pointing at
    the origin.  The mode is therefore approximate: ``dilate`` and a low threshold are the safety margin.
    :param sigma_thresh required: the library does not choose one
    :param outside_empty False keeps the samples outside the box (they are evaluated as without a grid), True rejects them
    :param sigma one (X, Y, Z) fp32 volume or a pair of the same shape to build from instead (``reso`` is then their shape):
        synthetic fields of tests and tools; ``net`` may be None when they are device tensors
    :return OccupancyGrid"""
    thresh, dilate = float(sigma_thresh), int(dilate)
    if np.isnan(thresh):
        raise ValueError("%s.occupancy_grid: sigma_thresh must not be a NaN" % _WHO)
    if not 0 <= dilate <= 4:
        raise ValueError("%s.occupancy_grid: dilate must be in 0 .. 4, got %d" % (_WHO, dilate))
    if sigma is None:
        vols = [sigma_grid(net, c1, c2, reso, eval_batch_size=eval_batch_size, coarse=True)]
        if getattr(net, "mlp_fine", None) is not None:
            vols.append(sigma_grid(net, c1, c2, reso, eval_batch_size=eval_batch_size, coarse=False))
    else:
        pair = list(sigma) if isinstance(sigma, (list, tuple)) else [sigma]
        if not 1 <= len(pair) <= 2:
            raise ValueError("%s.occupancy_grid: sigma must be one volume or a pair, got %d" % (_WHO, len(pair)))
        dev = pair[0].device if isinstance(pair[0], torch.Tensor) and pair[0].device.type == "cuda" else net._device()
        vols = [_volume(v, dev, "sigma") for v in pair]
        if len(vols) == 2 and vols[1].shape != vols[0].shape:
            raise ValueError("%s.occupancy_grid: the two sigma volumes differ in shape: %s and %s"
                             % (_WHO, tuple(vols[0].shape), tuple(vols[1].shape)))
    dims = [int(v) for v in vols[0].shape]
    a, b, d, _ = _grid_args(c1, c2, dims)
    dev = vols[0].device
    if dev.type != "cuda":
        raise _lib.PnyError("%s.occupancy_grid: the grid is built on an MI355X only (there is no CPU path)" % _WHO)
    bits = torch.empty(occupancy_words(dims), device=dev, dtype=torch.int32)
    occupied = torch.empty(1, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        check(_lib.load().pny_occupancy_build(C.c_void_p(vols[0].data_ptr()), C.c_void_p(vols[1].data_ptr()) if len(vols) == 2 else None,
                                              d, thresh, dilate, C.c_void_p(bits.data_ptr()), C.c_void_p(occupied.data_ptr()),
                                              stream_of(dev)))
    return OccupancyGrid(bits.view(torch.uint32), dims, list(a), list(b), outside_empty, occupied)


def marching_cubes(occu_net, c1=[-1, -1, -1], c2=[1, 1, 1], reso=[128, 128, 128], isosurface=50.0, sigma_idx=3,
                   eval_batch_size=100000, coarse=True, device=None, return_tensors=False):
    """The reference's ``recon.marching_cubes`` (recon.py:12-78), same signature and defaults, on the device.
    WARNING (the reference's): does not make much sense with viewdirs in current form, since sigma depends on viewdirs.
    :param device accepted for the reference's signature; the net's own device is used and another one is refused
    :param return_tensors True: the scaled fp32 device tensors instead of numpy arrays
    :return vertices (V, 3) float64 ``index * (c2 - c1) / reso + c1`` (the reference divides by reso, not reso - 1), triangles
    (T, 3) int32, numpy arrays"""
    if occu_net.use_viewdirs:
        warnings.warn("Running marching cubes with fake view dirs (pointing to origin), output may be invalid")
    if device is not None and torch.device(device) != torch.device(occu_net._device()):
        raise _lib.PnyError("%s.marching_cubes: device %s is not the net's (%s)" % (_WHO, device, occu_net._device()))
    is_train = occu_net.training
    occu_net.eval()
    try:
        sigma = sigma_grid(occu_net, c1, c2, reso, sigma_idx, eval_batch_size, coarse)
    finally:
        if is_train:
            occu_net.train()
    vertices, triangles = extract_mesh(sigma, isosurface)
    lo, hi, n = np.array(c1), np.array(c2), np.array(reso)
    if return_tensors:
        scale = torch.tensor((hi - lo) / n, dtype=torch.float32, device=vertices.device)
        return vertices * scale + torch.tensor(lo, dtype=torch.float32, device=vertices.device), triangles
    v = vertices.cpu().numpy().astype(np.float64)
    v *= (hi - lo) / n
    return v + lo, triangles.cpu().numpy()


def save_obj(vertices, triangles, path, vert_rgb=None):
    """The reference's ``recon.save_obj`` (recon.py:81-106): ``v %.4f %.4f %.4f`` per vertex (three more columns with
    ``vert_rgb``), then ``f %d %d %d`` per triangle, 1-based.  One format call per block, no Python loop over lines."""
    v = np.asarray(vertices.detach().cpu() if torch.is_tensor(vertices) else vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(triangles.detach().cpu() if torch.is_tensor(triangles) else triangles).reshape(-1, 3).astype(np.int64) + 1
    if vert_rgb is not None:
        c = np.asarray(vert_rgb.detach().cpu() if torch.is_tensor(vert_rgb) else vert_rgb, dtype=np.float64).reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise ValueError("%s.save_obj: vert_rgb has %d rows, vertices %d" % (_WHO, c.shape[0], v.shape[0]))
        v = np.concatenate([v, c], axis=1)
    v_line = "v " + " ".join(["%.4f"] * v.shape[1]) + "\n"
    with open(path, "w") as file:      # one format call per block, not per line
        file.write((v_line * v.shape[0]) % tuple(v.ravel().tolist()))
        file.write(("f %d %d %d\n" * f.shape[0]) % tuple(f.ravel().tolist()))
