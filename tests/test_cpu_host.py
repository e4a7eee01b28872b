"""
CPU-side checks (no GPU): the C-ABI library loads (its boundary is tests/test_cpu_abi.py's), the host mirrors expose the
reference's interface (names, state_dict keys, config defaults), errors are loud without a GPU, and the multi-process sharding
logic works over gloo.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from host_tools import ROOT, built_lib  # noqa: F401
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import dist as pdist
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import PixelNeRFNet, make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer, YoloRenderer, make_renderer


def test_no_wide_store_with_sgpr_soffset_is_followed_by_a_write_of_its_data(built_lib):
    """The write-data hazard of profiles/r03_anomalies.md (B), checked statically on the built code objects: a > 64-bit buffer
    store with an SGPR soffset directly followed by an instruction that writes its data registers is a form the compiler does
    not guard and gfx950 gets wrong (tools/check_store_hazard.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_store_hazard", os.path.join(ROOT, "tools", "check_store_hazard.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    if not os.path.exists(chk.OBJDUMP):
        pytest.skip("llvm-objdump not installed")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        objs = chk.code_objects(plib.LIB_PATH, tmp)
        assert objs, "no gfx950 code object in the library"
        bad = [b for o in objs for b in chk.scan(o)]
    assert not bad, bad[:3]
    # the scanner itself, on the two ISA shapes of profiles/r03_anomaly_b_isa.txt (failing) and on the guarded forms
    listing = """
0000000000001900 <kernel_a>:
	buffer_store_dwordx4 v[2:5], v19, s[60:63], s41 offen          // 000000001900: E07C1000
	v_and_b32_e32 v2, 0x3800, v11                                   // 000000001908: 260416FF
	buffer_store_dwordx4 v[88:91], v232, s[60:63], s8 offen        // 000000001910: E07C1000
	s_nop 0                                                         // 000000001918: BF800000
	v_mul_f32_e32 v88, v2, v34                                      // 00000000191C: 0AB04502
	buffer_store_dwordx4 v[88:91], v232, s[60:63], 0 offen         // 000000001920: E07C1000
	v_mul_f32_e32 v88, v2, v34                                      // 000000001928: 0AB04502
	buffer_store_dwordx4 v[10:13], v232, s[60:63], s8 offen        // 000000001930: E07C1000
	v_mul_f32_e32 v14, v2, v34                                      // 000000001938: 0AB04502
"""
    import subprocess
    real_run = subprocess.run

    class _R:
        stdout = listing
    try:
        chk.subprocess.run = lambda *a, **k: _R()
        hits = chk.scan("unused")
    finally:
        chk.subprocess.run = real_run
    assert len(hits) == 1 and hits[0][0] == "kernel_a" and "v[2:5]" in hits[0][1] and hits[0][2].startswith("v_and_b32")


def test_no_gpu_is_loud(built_lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ctypes as C
    h = C.c_void_p()
    desc = plib.ModelDesc(d_latent=512, d_hidden=512, d_out=4, n_blocks=5, combine_layer=3, num_freqs=6,
                          freq_factor=1.5, yolo=0, has_fine=1, device=0)
    rc = built_lib.pny_model_create(C.byref(h), C.byref(desc))
    assert rc == -4 and b"no HIP device" in built_lib.pny_last_error()
    with pytest.raises(plib.PnyError):
        plib.check(rc)
    net = make_model(pconf.default_mv()["model"]).eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.encode(torch.zeros(1, 1, 3, 64, 64), torch.eye(4)[None, None], torch.tensor(60.0))


def test_desc_validation(built_lib):
    import ctypes as C
    h = C.c_void_p()
    bad = plib.ModelDesc(d_latent=512, d_hidden=256, d_out=4, n_blocks=5, combine_layer=3, num_freqs=6,
                         freq_factor=1.5, yolo=0, has_fine=1, device=0)
    assert built_lib.pny_model_create(C.byref(h), C.byref(bad)) == -1
    assert b"d_hidden" in built_lib.pny_last_error()
    bad2 = plib.ModelDesc(d_latent=500, d_hidden=512, d_out=4, n_blocks=5, combine_layer=3, num_freqs=6,
                          freq_factor=1.5, yolo=0, has_fine=1, device=0)
    assert built_lib.pny_model_create(C.byref(h), C.byref(bad2)) == -1
    assert built_lib.pny_model_create(None, None) == -1


def test_state_dict_keys_match_reference_checkpoint_layout():
    """names/shapes a `pixel_nerf_latest` checkpoint holds."""
    net = make_model(pconf.default_mv()["model"])
    sd = net.state_dict()
    for mlp in ("mlp_coarse", "mlp_fine"):
        assert tuple(sd[mlp + ".lin_in.weight"].shape) == (512, 42)
        for i in range(3):
            assert tuple(sd["%s.lin_z.%d.weight" % (mlp, i)].shape) == (512, 512)
        for i in range(5):
            for fc in ("fc_0", "fc_1"):
                assert tuple(sd["%s.blocks.%d.%s.weight" % (mlp, i, fc)].shape) == (512, 512)
        assert tuple(sd[mlp + ".lin_out.weight"].shape) == (4, 512)
        assert sum(v.numel() for k, v in sd.items() if k.startswith(mlp + ".")) == 3438596
    assert tuple(sd["code._freqs"].shape) == (1, 12, 1) and tuple(sd["code._phases"].shape) == (1, 12, 1)
    assert tuple(sd["encoder.model.conv1.weight"].shape) == (64, 3, 7, 7)
    assert "encoder.model.layer4.2.bn2.running_var" in sd and "encoder.model.bn1.num_batches_tracked" in sd
    assert "encoder.model.layer2.0.downsample.1.running_mean" in sd
    assert not any(k.startswith("encoder.model.fc") for k in sd)
    # our synthetic generators produce loadable state
    miss = net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.resnet34_state(1).items()}, strict=False)
    assert not miss.unexpected_keys
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(2).items()}, strict=True)
    # reference init: fc_1 weights and all biases zero (resnetfc.py:36-39)
    fresh = make_model(pconf.default_mv()["model"])
    assert float(fresh.mlp_coarse.blocks[0].fc_1.weight.abs().max()) == 0.0
    assert float(fresh.mlp_coarse.lin_in.bias.abs().max()) == 0.0


def test_yolo_conf_model_and_renderer():
    c = pconf.yolo()
    net = make_model(c["model"])
    assert net.yolo and net.d_out == 21 and net.mlp_fine is None and net.d_latent == 1792
    assert tuple(net.state_dict()["mlp_coarse.lin_z.0.weight"].shape) == (512, 1792)
    assert sum(p.numel() for p in net.mlp_coarse.parameters()) == 5413397
    ren = make_renderer(c)
    assert isinstance(ren, YoloRenderer) and ren.n_coarse == 128 and ren.eval_batch_size == 128
    assert ren.num_anchors_per_scale == 3
    assert isinstance(make_renderer(pconf.default_mv()), NeRFRenderer)


def test_renderer_interface_and_sched():
    ren = NeRFRenderer.from_conf(pconf.default_mv()["renderer"], lindisp=False, eval_batch_size=50000)
    assert (ren.n_coarse, ren.n_fine, ren.n_fine_depth, ren.using_fine, ren.eval_batch_size) == (64, 32, 16, True, 50000)
    assert ren.white_bkgd and ren.sched is None
    assert set(ren.state_dict().keys()) == {"iter_idx", "last_sched"}
    ren2 = NeRFRenderer(n_coarse=16, n_fine=0, sched=[[2, 4], [32, 64], [8, 16]])
    ren2.sched_step(3)
    assert (ren2.n_coarse, ren2.n_fine, int(ren2.last_sched)) == (32, 8, 1)
    ren2.sched_step(1)
    assert (ren2.n_coarse, ren2.n_fine, int(ren2.last_sched)) == (64, 16, 2)
    # eval scripts mutate these attributes (eval.py:142-148 of the reference)
    ren.n_coarse, ren.n_fine, ren.using_fine = 128, 0, False


def test_weight_change_detection():
    """PixelNeRFNet._weights_key must change for every way the weights can change (the native copy is re-uploaded
    when it does): in-place updates, load_state_dict, .data assignment, a replaced Parameter, a replaced submodule,
    the fine MLP detached."""
    net = make_model(pconf.default_mv()["model"]).eval()
    k0 = net._weights_key()
    assert net._weights_key() == k0
    with torch.no_grad():
        net.mlp_coarse.lin_in.bias.add_(1.0)                       # optimizer-style in-place update
    k1 = net._weights_key()
    assert k1 != k0
    net.load_state_dict(net.state_dict())                          # in-place copy
    k2 = net._weights_key()
    assert k2 != k1
    net.mlp_fine.lin_out.weight.data = torch.zeros_like(net.mlp_fine.lin_out.weight)
    k3 = net._weights_key()
    assert k3 != k2
    net.mlp_coarse.blocks[0].fc_0.weight = torch.nn.Parameter(torch.zeros(512, 512))   # a new Parameter object
    k4 = net._weights_key()
    assert k4 != k3
    net.mlp_coarse.blocks[1] = type(net.mlp_coarse.blocks[1])(512)                      # a new submodule
    k5 = net._weights_key()
    assert k5 != k4
    net.mlp_fine = None
    assert net._weights_key() != k5


def test_refresh_rule_on_hand_made_keys():
    """PixelNeRFNet._follows_in_place / _mark_trunk_stale, the one statement of the rule that _sync() and optim.Adam.step() both
    follow: the native copy follows a change of the weights key on the device only when it reads the MLP parameters in place
    and nothing but MLP / encoder tensors moved, in place; an encoder tensor that moved marks the inference trunk stale."""
    net = make_model(pconf.default_mv()["model"]).eval()
    old = (("mlp_coarse.lin_in.weight", 1000, 3), ("encoder.model.conv1.weight", 2000, 5), ("code._freqs", 3000, 0))

    def changed(i, ptr=None, version=None):
        row = old[i]
        return old[:i] + ((row[0], row[1] if ptr is None else ptr, row[2] if version is None else version),) + old[i + 1:]

    assert not net._follows_in_place(old, old)                      # a fresh model: the library reads no parameter in place
    net._dev_bound = True                                           # (what _sync() finds on the device for contiguous fp32 MLPs)
    assert net._follows_in_place(old, old) is True
    assert net._follows_in_place(old, changed(0, version=4)) is True
    net._mark_trunk_stale(old, changed(0, version=4))
    assert net._enc_stale is False                                  # an MLP step does not touch the trunk
    assert net._follows_in_place(old, changed(1, version=6)) is True
    net._mark_trunk_stale(old, changed(1, version=6))
    assert net._enc_stale is True
    assert net._follows_in_place(old, changed(2, version=1)) is False      # a code. buffer written: re-upload
    assert net._follows_in_place(old, changed(0, ptr=1064)) is False       # a storage moved
    assert net._follows_in_place(old, changed(1, ptr=2064, version=6)) is False
    assert net._follows_in_place(old, old[:2]) is False and net._follows_in_place(old[:2], old) is False
    assert net._follows_in_place(None, old) is False


def test_camera_pair_formats():
    """model._camera_pairs: focal / c as encode() takes them (reference models.py:125-148) -> (N, 2) fp32 host rows."""
    from pixel_nerf_yolo_amd.model import _camera_pairs

    def rows(v, **kw):
        out = _camera_pairs(v, **kw)
        assert out.dtype == torch.float32 and out.device.type == "cpu" and out.is_contiguous() and out.dim() == 2
        return out.tolist()
    assert rows(65.5) == [[65.5, 65.5]]
    assert rows(torch.tensor(65.5, dtype=torch.float64)) == [[65.5, 65.5]]
    assert rows(torch.tensor([10.0, 20.0, 30.0])) == [[10.0, 10.0], [20.0, 20.0], [30.0, 30.0]]
    assert rows(np.array([[31.5, 24.25]])) == [[31.5, 24.25]]
    assert rows(torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]).t().contiguous().t()) == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]
    assert rows(None, default=(63 * 0.5, 48 * 0.5)) == [[31.5, 24.0]]     # c = None: the centre of a 63 x 48 (W x H) image


def test_sched_step_matches_reference(golden):
    """tests/golden/sched.npz: the reference's NeRFRenderer driven through the same step sequence."""
    g = golden("sched")
    ren = NeRFRenderer(n_coarse=16, n_fine=4, sched=g["sched"].tolist())
    for st, row in zip(g["steps"].tolist(), g["rows"].tolist()):
        ren.sched_step(st)
        assert [ren.n_coarse, ren.n_fine, int(ren.iter_idx), int(ren.last_sched)] == row


def test_unsupported_configs_are_refused():
    c = pconf.default_mv()
    c.d["model"]["mlp_coarse"]["use_spade"] = True
    with pytest.raises(NotImplementedError):
        make_model(c["model"])
    c = pconf.default_mv()
    c.d["model"]["encoder"]["index_padding"] = "border"
    with pytest.raises(NotImplementedError):
        make_model(c["model"])
    c = pconf.default_mv()
    c.d["model"]["use_code_viewdirs"] = True
    with pytest.raises(NotImplementedError):
        make_model(c["model"])


def test_shard_bounds_cover_exactly():
    for n in (0, 1, 63, 64, 16384, 160000, 12345):
        for world in (1, 2, 4, 8):
            spans = [pdist.shard_bounds(n, world, r) for r in range(world)]
            per = spans[0][2]
            assert per % 64 == 0 and per * world >= n
            covered = sum(hi - lo for lo, hi, _ in spans)
            assert covered == n
            for r, (lo, hi, _) in enumerate(spans):
                assert lo == min(n, r * per) and lo <= hi <= n


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("n", [1000, 50])
def test_render_sharded_gloo_world2(n):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    import dist_worker
    procs = [ctx.Process(target=dist_worker.run, args=(r, 2, port, n, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True, (n, 3)), (1, True, (n, 3))]


def test_allreduce_gradients_gloo_world2():
    """Data-parallel training's one exchange step (dist.allreduce_gradients): mean over ranks, missing gradients count as
    zeros, frozen parameters are skipped, bucket limit respected."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    import dist_worker
    procs = [ctx.Process(target=dist_worker.run_grads, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True, 1, 3), (1, True, 1, 3)]


def test_bench_json_contract_fields():
    import json
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--describe"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("metric", "unit", "config", "flop_per_ray"):
        assert k in d
    assert d["unit"] == "rays/s" and d["config"]["workload"].startswith("C2")
    assert abs(d["flop_per_ray"] - 2.6218e9) / 2.6218e9 < 1e-3


def test_checkpoint_contract_matches_reference(tmp_path):
    """load_weights / save_weights against tests/golden/ckpt.json, which tools/make_golden.py captured by driving the
    reference's PixelNeRFNet (models.py:320-370) through the same sequence: which file each (resume, opt_init)
    combination loads, the bare `return` (None) for opt_init without resume, the warning for a missing file, and the
    trainer's epochNum calls (trainer.py:246-256) that only snapshot the file on disk."""
    import json
    import shutil
    import warnings
    from types import SimpleNamespace

    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "ckpt.json")))
    conf = pconf.default_mv()["model"]

    def fresh(marker):
        net = make_model(conf)
        with torch.no_grad():
            net.mlp_coarse.lin_out.bias.fill_(marker)
        return net

    def marker_of(sd):
        return float(sd["mlp_coarse.lin_out.bias"][0])

    root = tmp_path / "exp"
    last_files = None
    for case in rec["load"]:
        if case["files"] != last_files:
            shutil.rmtree(root, ignore_errors=True)
            root.mkdir()
            for fn, mk in (("pixel_nerf_init", 1.0), ("pixel_nerf_latest", 2.0)):
                if fn in case["files"]:
                    torch.save(fresh(mk).state_dict(), str(root / fn))
            last_files = case["files"]
        args = SimpleNamespace(checkpoints_path=str(tmp_path), name="exp", resume=case["resume"])
        net = fresh(0.0)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ret = net.load_weights(args, opt_init=case["opt_init"])
        got = {"marker_after": marker_of(net.state_dict()), "returns_self": ret is net, "returns_none": ret is None,
               "warned": any("does not exist" in str(x.message) for x in w)}
        assert got == {k: case[k] for k in got}, (case, got)
    shutil.rmtree(root, ignore_errors=True)
    root.mkdir()
    args = SimpleNamespace(checkpoints_path=str(tmp_path), name="exp", resume=True)
    for step in rec["save"]:
        ret = fresh(step["marker"]).save_weights(args, **step["kwargs"])
        assert (ret is not None) == step["returns_self"]
        files = {fn: marker_of(torch.load(str(root / fn), map_location="cpu", weights_only=True))
                 for fn in sorted(os.listdir(root))}
        assert files == step["files"], (step, files)


@pytest.mark.parametrize("n_dev", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1000])
def test_ray_ranges_split_a_call_into_whole_64_ray_groups(n, n_dev):
    """render._ray_ranges, the one place that splits a call's rays over the devices of bind_parallel: one (lo, hi) per device,
    contiguous from 0 to n, every start and every length but the last non-empty one a multiple of 64 (the kernels' ray
    group), empty ranges only at the end."""
    from pixel_nerf_yolo_amd.render import _ray_ranges
    ranges = _ray_ranges(n, n_dev)
    assert len(ranges) == n_dev
    assert ranges[0][0] == 0 and ranges[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert all(lo % 64 == 0 or lo == hi == n for lo, hi in ranges)
    full = [(lo, hi) for lo, hi in ranges if hi > lo]
    assert full == ranges[:len(full)] and len(full) >= 1
    assert all(lo % 64 == 0 for lo, _ in full) and all((hi - lo) % 64 == 0 for lo, hi in full[:-1])
    assert sum(hi - lo for lo, hi in full) == n
