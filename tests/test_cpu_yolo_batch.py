"""
The YOLO training batch without a GPU (include/pnyolo.h pny_yolo_train_batch, util.yolo_train_batch / stage_yolo_targets):

  * the header declares the entry and cites what it replaces (the boundary itself: tests/test_cpu_abi.py);
  * every bad argument comes back as PNY_ERR_ARG before anything is launched (the device pointers here are made up and are
    never dereferenced);
  * the offsets the entry reports (its size query: no launch) equal the reference's for the three cases of
    tests/golden/yolo_train_batch.npz (tools/make_yolo_batch_golden.py);
  * stage_yolo_targets gives the reference's stacked tensors for the dataset's nested structure;
  * the numpy restatement of the row order (tests/yolo_batch_ref.py) agrees with the fixture.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import yolo_batch_ref as yb
from host_tools import built_lib, header_code, header_text  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import util as putil


# --------------------------------------------------------------------------- C ABI
def test_entry_is_declared_bound_and_exported():
    """What is this entry's own (declared, bound, exported, its layout and limits: tests/test_cpu_abi.py)."""
    hdr = header_text()
    assert re.search(r"\bint\s+pny_yolo_train_batch\s*\(\s*const\s+pny_yolo_batch_desc\s*\*", header_code())
    block = hdr[:hdr.index("int pny_yolo_train_batch")]
    block = block[block.rindex("int pny_sample_train_batch"):]
    assert "YoloTrainer.py:93-129" in block and "util.py:808-876" in block


# --------------------------------------------------------------------------- argument checks
OK = dict(n_views_all=5, n_views=3, height=40, width=56, n_scales=3, cell_sizes=(8, 16, 32, 0), n_anchors=3, z_near=1.0, z_far=6.0)
DEVP = 4096     # stands for a device pointer (16-byte aligned); never dereferenced by the host


def call(L, desc=None, poses="ok", views=(4, 0, 2), focal="ok", c="ok", grids=(DEVP, DEVP, DEVP, DEVP), rays=DEVP, tout=DEVP,
         offsets="ok", **over):
    k = dict(OK, **over)
    k["cell_sizes"] = (C.c_int32 * 4)(*k["cell_sizes"])
    d = plib.YoloBatchDesc(**k) if desc is None else desc
    p = torch.eye(4).repeat(max(k["n_views_all"], 1), 1, 1).contiguous()
    ids = (C.c_int64 * len(views))(*views) if views is not None else None
    two = (C.c_float * 2)(44.0, 47.5)
    off = (C.c_int64 * 5)(*([-7] * 5))
    rc = L.pny_yolo_train_batch(C.byref(d) if d else None, C.c_void_p(p.data_ptr()) if poses == "ok" else poses,
                                ids, two if focal == "ok" else focal, two if c == "ok" else c,
                                (C.c_void_p * 4)(*grids) if grids is not None else None, C.c_void_p(rays) if rays else None,
                                C.c_void_p(tout) if tout else None, off if offsets == "ok" else offsets, None)
    return rc, list(off), L.pny_last_error()


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    L = built_lib
    for missing in ("desc", "poses", "views", "focal", "c", "grids", "offsets"):
        rc, _, msg = call(L, **({missing: None} if missing != "desc" else {"desc": False}))
        assert rc == -1 and b"null" in msg, missing
    assert call(L, rays=None)[0] == -1 and call(L, tout=None)[0] == -1          # one output without the other
    for bad in ((5, 0, 2), (-1, 0, 2), (4, 0, 2 ** 33)):
        rc, _, msg = call(L, views=bad)
        assert rc == -1 and b"view id" in msg, bad
    for n in (0, 5, -1):
        rc, _, msg = call(L, n_scales=n)
        assert rc == -1 and b"n_scales" in msg, n
    for cells in ((0, 16, 32, 0), (8, 41, 32, 0), (8, 16, 57, 0), (-8, 16, 32, 0)):      # 0; larger than H; larger than W; negative
        rc, _, msg = call(L, cell_sizes=cells)
        assert rc == -1 and b"cell size" in msg, cells
    rc, _, msg = call(L, grids=(DEVP, 0, DEVP, DEVP))
    assert rc == -1 and b"target grid" in msg
    rc, _, msg = call(L, rays=DEVP + 4)
    assert rc == -1 and b"aligned" in msg
    rc, _, msg = call(L, n_views=17, views=tuple(range(5)) * 3 + (0, 1))
    assert rc == -1 and b"n_views" in msg and b"16" in msg
    assert call(L, n_views=0)[0] == -1
    for bad in (dict(n_views_all=0), dict(height=0), dict(width=-3), dict(n_anchors=0)):
        rc, _, msg = call(L, **bad)
        assert rc == -1 and b"shape" in msg, bad
    singular = torch.zeros(5, 4, 4)
    rc, _, msg = call(L, poses=C.c_void_p(singular.data_ptr()))
    assert rc == -1 and b"singular" in msg
    rc, _, msg = call(L, focal=(C.c_float * 2)(0.0, 47.5))
    assert rc == -1 and b"focal" in msg


def test_size_query_reports_the_reference_offsets_without_a_launch(built_lib, golden):
    g = golden("yolo_train_batch")
    for case in yb.CASES:
        k = yb.fixture_case(g, case)
        cells = tuple(k["cells"]) + (0,) * (4 - len(k["cells"]))
        rc, off, msg = call(built_lib, poses=None, views=None, focal=None, c=None, grids=None, rays=None, tout=None,
                            n_views_all=k["NV"], n_views=len(k["views"]), height=k["H"], width=k["W"], n_scales=len(k["cells"]),
                            cell_sizes=cells, n_anchors=k["A"])
        n = len(k["cells"]) + 1
        assert rc == 0, msg
        assert off[:n] == k["offsets"].tolist() == yb.offsets(len(k["views"]), k["H"], k["W"], k["cells"]).tolist()
        assert off[n:] == [-7] * (5 - n), "only n_scales + 1 offsets are written"
    # the limit the documentation gives: 16 views x 4 scales
    rc, off, _ = call(built_lib, rays=None, tout=None, n_views_all=3, n_views=16, height=8, width=8, n_scales=4, cell_sizes=(1, 2, 4, 8))
    assert rc == 0 and off == [0, 1024, 1280, 1344, 1360]


# --------------------------------------------------------------------------- the fixture and the restatement
def test_fixture_is_what_the_tool_describes(golden):
    g = golden("yolo_train_batch")
    a, b, c = (yb.fixture_case(g, k) for k in yb.CASES)
    assert (a["H"], a["W"], a["cells"], a["NV"], a["views"].tolist(), a["A"]) == (40, 56, [8, 16, 32], 5, [4, 0, 2], 3)
    assert [t.shape[1:3] for t in a["grids"]] == [(5, 7), (2, 3), (1, 1)] and int(a["offsets"][-1]) == 126
    assert (b["H"], b["W"], b["cells"], b["NV"], b["views"].tolist(), b["A"]) == (70, 100, [32], 2, [1], 3)
    assert b["H"] % 32 and b["W"] % 32 and b["grids"][0].shape == (2, 2, 3, 3, 6)
    assert (c["H"], c["W"], c["cells"], c["NV"], c["views"].tolist(), c["A"]) == (64, 72, [4, 8], 4, [3, 1, 2], 2)
    assert c["offsets"].tolist() == [0, 864, 1080]
    for k in (a, b, c):
        assert k["focal"][0] != k["focal"][1] and abs(k["c"][0] - k["W"] / 2) > 0.5 and abs(k["c"][1] - k["H"] / 2) > 0.5
        for p in k["poses"]:                                   # rigid, with a real rotation
            assert np.allclose(p[:3, :3] @ p[:3, :3].T, np.eye(3), atol=1e-5) and np.abs(p[:3, :3] - np.eye(3)).max() > 0.1
            assert np.array_equal(p[3], [0, 0, 0, 1]) and np.abs(p[:3, 3]).max() > 1.0
        for s, grid in enumerate(k["grids"]):
            assert np.array_equal(grid, yb.coded_grids(k["NV"], k["H"], k["W"], k["cells"], k["A"])[s]), "the values encode their place"
            assert k["rays"][s].shape == (k["targets"][s].shape[0], 8) and k["rays"][s].dtype == np.float32


@pytest.mark.parametrize("case", yb.CASES)
def test_restatement_of_the_row_order_agrees_with_the_reference(golden, case):
    k = yb.fixture_case(golden("yolo_train_batch"), case)
    mine = yb.gather_targets(k["grids"], k["views"])
    for s in range(len(k["cells"])):
        assert np.array_equal(mine[s], k["targets"][s])
    # the rays: the oracle's gen_rays_yolo of EVERY view at each scale (fp32 focal / cell, c / cell), gathered the same way
    import pnyolo_oracle as orc
    full = []
    for cell in k["cells"]:
        f, c = torch.from_numpy(k["focal"]) / cell, torch.from_numpy(k["c"]) / cell
        full.append(orc.gen_rays_yolo(k["poses"], k["W"] // cell, k["H"] // cell, f, c, *k["z"]).numpy())
    for s, r in enumerate(yb.gather_rays(full, k["views"])):
        assert r.shape == k["rays"][s].shape and float(np.abs(r - k["rays"][s]).max()) < 1e-5


@pytest.mark.parametrize("case", yb.CASES)
def test_stage_yolo_targets_reproduces_the_stacked_tensors(golden, case):
    """The dataset's nested structure -> one (NV, Hs, Ws, A, 6) tensor per scale, bit for bit the reference's stack + squeeze.
    Staged on the CPU here (the device is only where the result lives)."""
    k = yb.fixture_case(golden("yolo_train_batch"), case)
    nested = [tuple(torch.from_numpy(grid[v:v + 1].copy()) for grid in k["grids"]) for v in range(k["NV"])]
    assert len(nested) == k["NV"] and nested[0][0].shape == (1,) + k["grids"][0].shape[1:]
    staged = putil.stage_yolo_targets(nested, "cpu")
    assert len(staged) == len(k["cells"])
    for s, t in enumerate(staged):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == k["grids"][s].shape
        assert np.array_equal(t.numpy(), k["grids"][s])


def test_no_gpu_is_loud(golden):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    k = yb.fixture_case(golden("yolo_train_batch"), "b")
    with pytest.raises(RuntimeError, match="no CPU path"):
        putil.yolo_train_batch(torch.from_numpy(k["poses"]), k["views"], k["focal"], k["c"], [torch.from_numpy(t) for t in k["grids"]],
                               k["H"], k["W"], k["cells"], *k["z"])
