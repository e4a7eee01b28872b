"""The oracle's trunk in float64 (spatial_encoder(dtype=torch.float64)), the arbiter of tests/test_gpu_trunk.py, against its
default float32 arithmetic (which tests/test_oracle_golden.py holds to the reference): the same function to fp32 rounding,
forward and autograd.  CPU only."""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from pixel_nerf_yolo_amd import synth


def _state(enc, dtype):
    return {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_("running" not in k)
            for k, v in enc.items() if "num_batches" not in k}


@pytest.mark.parametrize("training", [False, True])
def test_oracle_trunk_fp64_matches_fp32(training):
    n, H, W = 2, 32, 40
    enc = synth.resnet34_state(1803, residual_gain=0.25)
    images = synth.images(1804, n, H, W)
    G = torch.from_numpy(np.random.RandomState(5).standard_normal((n, 512, H // 2, W // 2)))
    sd32, sd64 = _state(enc, torch.float32), _state(enc, torch.float64)
    lat32, lv32 = orc.spatial_encoder(sd32, images, training=training)
    lat64, lv64 = orc.spatial_encoder(sd64, images, training=training, dtype=torch.float64)
    assert lat32.dtype == torch.float32 and lat64.dtype == torch.float64 and all(t.dtype == torch.float64 for t in lv64)
    # the default is the float32 arithmetic itself, bit for bit
    sd32b = _state(enc, torch.float32)
    assert torch.equal(orc.spatial_encoder(sd32b, images, training=training, dtype=torch.float32)[0], lat32)
    scale = max(1.0, float(lat64.abs().max()))
    assert float((lat32.double() - lat64).abs().max()) <= 1e-5 * scale
    (lat32 * G.float()).sum().backward()
    (lat64 * G).sum().backward()
    checked = 0
    for k, t in sd64.items():
        if t.grad is None:
            assert k.startswith(("encoder.model.layer4", "encoder.model.fc")) or "running" in k, k
            continue
        g32 = sd32[k].grad.double()
        assert float((g32 - t.grad).abs().max()) <= 2e-5 * float(t.grad.abs().max()), k
        checked += 1
    assert checked >= 80
    # batch statistics step the float64 running statistics in place, as they step the float32 ones
    for k, t in sd64.items():
        if "running" in k and not k.startswith("encoder.model.layer4"):
            moved = not torch.equal(t, torch.from_numpy(enc[k]).double())
            assert moved == training, k
            assert float((sd32[k].double() - t).abs().max()) <= 1e-6 * max(1.0, float(t.abs().max())), k


def test_oracle_trunk_fp64_gradients_reach_fp32_leaves():
    """Leaves of another dtype are converted differentiably: fp32 parameters receive the fp64 graph's gradients."""
    enc = synth.resnet34_state(1803, residual_gain=0.25)
    sd32 = _state(enc, torch.float32)
    lat = orc.spatial_encoder(sd32, synth.images(1804, 1, 32, 32), dtype=torch.float64)[0]
    assert lat.dtype == torch.float64
    lat.sum().backward()
    assert sd32["encoder.model.conv1.weight"].grad is not None
    assert sd32["encoder.model.conv1.weight"].grad.dtype == torch.float32
