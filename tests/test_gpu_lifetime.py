"""
Lifetime of what the library allocates on the device: one cycle builds everything a model, its scenes, the training trunk, an
optimizer and a NaN / Inf monitor can own, uses it once and destroys it; free device memory must not go down from cycle to
cycle.  The owning types are csrc/dev_resource.h; the figures behind the bar are in profiles/lifetime.md.

What this test cannot see: events, streams and pinned host memory do not move torch.cuda.mem_get_info (test_cpu_dev_resource.py
counts those against fakes), and another process on the same card can move it: the test reads once and does not retry.
"""
import gc

import numpy as np
import pytest
import torch

from helpers import DEV, load_mlp, render_loss
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.optim import Adam
from pixel_nerf_yolo_amd.render import NeRFRenderer
from pixel_nerf_yolo_amd.util import FiniteMonitor, gen_rays

pytestmark = pytest.mark.gpu

SB, NS, H, W, KC, KF, KFD, RAYS = 2, 2, 64, 64, 8, 8, 4, 128
WARMUP, CYCLES = 2, 6
# The smallest device buffer a cycle allocates: DeferredStash::absmax (csrc/api_internal.h), the two words of running max |dY|
# that the f16 weight-gradient GEMMs of the deferred flush scale by: 8 bytes.  A buffer leaked once per cycle costs at least
# CYCLES times its size, so half of the smallest one is a bar that every single leak is over, twelve times.
SMALLEST_BUFFER_BYTES = 8
BAR_BYTES = SMALLEST_BUFFER_BYTES // 2


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(torch.device(DEV))[0]


class Rig:
    """The Python objects of the cycles, built once: the native handles behind them are what a cycle creates and destroys."""

    def __init__(self):
        c = pconf.default_mv()
        self.net = make_model(c["model"], stop_encoder_grad=False)
        enc = synth.resnet34_state(4100, residual_gain=0.25)
        self.net.load_state_dict({k: torch.from_numpy(v) for k, v in enc.items()}, strict=False)
        load_mlp(self.net.mlp_coarse, 4101, 512, 4)
        load_mlp(self.net.mlp_fine, 4102, 512, 4)
        self.net = self.net.to(DEV).train()
        self.ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).train()
        self.params = dict(self.net.trainable_mlp_parameters())
        self.opt = Adam(list(self.params.values()), lr=1e-4, model=self.net)
        rs = np.random.RandomState(4103)
        self.images = torch.from_numpy(np.stack([synth.images(4104 + i, NS, H, W) for i in range(SB)]))
        poses = [synth.scene_cameras(NS, radius=1.3 + 0.1 * i) for i in range(SB)]
        self.poses = torch.from_numpy(np.stack([p[0] for p in poses]).astype(np.float32))
        self.focal, self.cc = torch.tensor(0.9 * W), torch.tensor([[W * 0.5, H * 0.5]])
        tgt = torch.from_numpy(np.stack([p[1] for p in poses]).astype(np.float32)).to(DEV)
        rays = gen_rays(tgt, W, H, self.focal, 0.8, 1.8, c=self.cc[0]).reshape(SB, -1, 8)
        self.rays = rays[:, torch.from_numpy(rs.choice(H * W, RAYS, replace=False)).to(DEV)].contiguous()
        self.gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, RAYS, 3)).astype(np.float32)).to(DEV)
        self.latent = torch.from_numpy(synth.latent(4105, SB * NS, 512, H // 2, W // 2)).to(DEV)
        self.G = torch.from_numpy(rs.standard_normal((SB * NS, 512, H // 2, W // 2)).astype(np.float32)).to(DEV) * 1e-3

    def cycle(self):
        """-> device bytes the cycle held just before it destroyed its handles."""
        net, opt = self.net, self.opt
        before = free_bytes()
        net.zero_grad(set_to_none=True)
        net.set_matrix_precision("auto")
        net.set_deterministic(True)
        net.enable_kernel_timing(True)
        # a model with encoder weights and a fine MLP, two scenes, 2 views of 64 x 64 each through the inference trunk
        with torch.no_grad():
            net.encode(self.images, self.poses, self.focal, c=self.cc)
        assert net._h_model is not None and len(net._h_scenes) == SB and net._h_group is None
        net.set_matrix_precision("f16_train")      # builds the single-plane images, plain and transposed
        # a stashing render into the deferred reservation, its backward with a bound latent gradient (deterministic: the fixed-point
        # accumulator), the flush of the deferred weight gradients
        lat = self.latent.clone().requires_grad_()
        net.encode(self.images, self.poses, self.focal, c=self.cc, latent=lat)
        out = self.ren(net, self.rays, want_weights=True)
        render_loss(out, self.gt, True).backward()
        assert lat.grad is not None and net.last_latent_grad_deterministic()
        assert net.last_backward_precision() == "f16" and net.last_flush_precision() == "f16", \
            (net.last_backward_precision(), net.last_flush_precision())
        assert all(p.grad is not None for p in self.params.values())
        # the training trunk, forward and backward
        net.encode(self.images, self.poses, self.focal, c=self.cc)
        (net.differentiable_latent() * self.G).sum().backward()
        assert net.encoder.model.conv1.weight.grad is not None
        opt.step()                                  # one native Adam launch and the refresh of the packed weights behind it
        mon = FiniteMonitor(("grads",), DEV)
        mon.watch("grads", list(self.params.values()), list(self.params), grads=True)
        mon.check("grads")
        assert mon.report()["grads"][:2] == (False, False)
        held = before - free_bytes()
        mon.close()
        opt._free_native()
        net._free_native()
        del lat, out, mon
        gc.collect()
        return held


def test_device_memory_returns_after_every_cycle(monkeypatch):
    """Free device memory after WARMUP + CYCLES cycles against free device memory after WARMUP cycles (which leave torch's
    allocator with the blocks it needs).  The bar is half of the smallest device buffer of a cycle; measured before the owning
    handles existed: a drop of 0 bytes over 6 cycles, of a footprint of 1.49 GB per cycle (profiles/lifetime.md)."""
    monkeypatch.setenv("PNYOLO_GROUP", "0")        # one scene per object
    for var in ("PNYOLO_MLP_PRECISION", "PNYOLO_PROJECTION", "PNYOLO_STASH_GB", "PNYOLO_SPLIT_FLUSH", "PNYOLO_TRUNK",
                "PNYOLO_TRUNK_NO_SIDE_STREAM"):
        monkeypatch.delenv(var, raising=False)
    rig = Rig()
    for _ in range(WARMUP):
        rig.cycle()
    start = free_bytes()
    held = [rig.cycle() for _ in range(CYCLES)]
    drop = start - free_bytes()
    print("LIFETIME: free device memory dropped by %d bytes over %d cycles (bar %d); a cycle held %s bytes before its destroy"
          % (drop, CYCLES, BAR_BYTES, sorted(set(held))))
    assert min(held) > 0, held
    assert drop < BAR_BYTES, "free device memory dropped by %d bytes over %d cycles (one cycle holds %d)" % (drop, CYCLES, max(held))
