"""
Host-side mirror of the reference's model layer (src/model/): ``make_model`` and
``PixelNeRFNet`` with the same constructor, ``encode`` / ``forward`` / ``load_weights``
signatures and the same state_dict key names, executing on libpnyolo.so.

torch is used for what it is good at here: holding parameters / checkpoints (state_dict
compatibility with the reference's ``pixel_nerf_latest`` files), device memory and streams.
No torch operator runs on the hot path: ``encode`` and ``forward`` hand raw device pointers to
the C ABI (include/pnyolo.h).  Forward only -- a call under autograd raises (backward is the
"next" row of SURVEY.md 8f).
"""
import contextlib
import ctypes as C
import os
import os.path as osp
import types
import warnings

import numpy as np
import torch
from torch import nn

from . import lib as _lib
from .lib import ModelDesc, check, ptr, stream_of


# ------------------------------------------------------------------ parameter containers
class _ResnetBlockFC(nn.Module):
    """Parameters of one block; init as reference src/model/resnetfc.py:19-51."""

    def __init__(self, size):
        super().__init__()
        self.fc_0 = nn.Linear(size, size)
        self.fc_1 = nn.Linear(size, size)
        nn.init.constant_(self.fc_0.bias, 0.0)
        nn.init.kaiming_normal_(self.fc_0.weight, a=0, mode="fan_in")
        nn.init.constant_(self.fc_1.bias, 0.0)
        nn.init.zeros_(self.fc_1.weight)


# Bumped by every parameter / buffer / submodule registration in the process (see PixelNeRFNet._weights_key).
_STRUCT_EPOCH = [0]


def _bump_struct_epoch(*_args, **_kwargs):
    _STRUCT_EPOCH[0] += 1


for _reg in ("register_module_parameter_registration_hook", "register_module_buffer_registration_hook",
             "register_module_module_registration_hook"):
    getattr(torch.nn.modules.module, _reg)(_bump_struct_epoch)


class ResnetFC(nn.Module):
    """Parameter container with the reference's names / shapes / init
    (src/model/resnetfc.py:66-132, from_conf :188-205).  The arithmetic lives in csrc/mlp.hip."""

    def __init__(self, d_in, d_out=4, n_blocks=5, d_latent=0, d_hidden=128, beta=0.0, combine_layer=1000,
                 combine_type="average", use_spade=False):
        super().__init__()
        if beta > 0 or use_spade or combine_type != "average":
            raise NotImplementedError("libpnyolo supports ReLU, no SPADE, average combine (the shipped configs)")
        self.lin_in = nn.Linear(d_in, d_hidden)
        nn.init.constant_(self.lin_in.bias, 0.0)
        nn.init.kaiming_normal_(self.lin_in.weight, a=0, mode="fan_in")
        self.lin_out = nn.Linear(d_hidden, d_out)
        nn.init.constant_(self.lin_out.bias, 0.0)
        nn.init.kaiming_normal_(self.lin_out.weight, a=0, mode="fan_in")
        self.n_blocks, self.d_latent, self.d_in, self.d_out, self.d_hidden = n_blocks, d_latent, d_in, d_out, d_hidden
        self.combine_layer, self.combine_type, self.use_spade = combine_layer, combine_type, use_spade
        self.blocks = nn.ModuleList([_ResnetBlockFC(d_hidden) for _ in range(n_blocks)])
        if d_latent != 0:
            n_lin_z = min(combine_layer, n_blocks)
            self.lin_z = nn.ModuleList([nn.Linear(d_latent, d_hidden) for _ in range(n_lin_z)])
            for i in range(n_lin_z):
                nn.init.constant_(self.lin_z[i].bias, 0.0)
                nn.init.kaiming_normal_(self.lin_z[i].weight, a=0, mode="fan_in")

    @classmethod
    def from_conf(cls, conf, d_in, **kwargs):
        if not conf.get_bool("yolo", False):
            d_out = conf.get_int("d_out", 4)
        else:
            d_out = conf.get_int("d_out", 7) * conf.get_int("num_anchors_per_scale", 3)
        return cls(d_in, d_out=d_out, n_blocks=conf.get_int("n_blocks", 5), d_hidden=conf.get_int("d_hidden", 128),
                   beta=conf.get_float("beta", 0.0), combine_layer=conf.get_int("combine_layer", 1000),
                   combine_type=conf.get_string("combine_type", "average"),
                   use_spade=conf.get_bool("use_spade", False), **kwargs)

    def forward(self, *a, **k):
        raise RuntimeError("ResnetFC is evaluated inside libpnyolo's fused kernel; call PixelNeRFNet.forward")


class PositionalEncoding(nn.Module):
    """Buffers `_freqs`, `_phases` as in reference src/model/code.py:11-28 (checkpoint keys)."""

    def __init__(self, num_freqs=6, d_in=3, freq_factor=np.pi, include_input=True):
        super().__init__()
        self.num_freqs, self.d_in, self.freq_factor, self.include_input = num_freqs, d_in, freq_factor, include_input
        freqs = freq_factor * 2.0 ** torch.arange(0, num_freqs)
        self.d_out = num_freqs * 2 * d_in + (d_in if include_input else 0)
        self.register_buffer("_freqs", torch.repeat_interleave(freqs, 2).view(1, -1, 1))
        ph = torch.zeros(2 * num_freqs)
        ph[1::2] = np.pi * 0.5
        self.register_buffer("_phases", ph.view(1, -1, 1))

    @classmethod
    def from_conf(cls, conf, d_in=3):
        return cls(conf.get_int("num_freqs", 6), d_in, conf.get_float("freq_factor", np.pi),
                   conf.get_bool("include_input", True))


def _basic_block(cin, cout, stride):
    blk = nn.Module()
    blk.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
    blk.bn1 = nn.BatchNorm2d(cout)
    blk.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
    blk.bn2 = nn.BatchNorm2d(cout)
    if stride != 1 or cin != cout:
        blk.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))
    return blk


def _resnet34_params():
    """Parameter container with the ResNet-34 key names the reference's checkpoints hold
    (`encoder.model.*`).  layer4 is carried for strict state_dict loading only."""
    m = nn.Module()
    m.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    m.bn1 = nn.BatchNorm2d(64)
    cin = 64
    for li, (cout, n) in enumerate([(64, 3), (128, 4), (256, 6), (512, 3)], start=1):
        setattr(m, "layer%d" % li, nn.Sequential(
            *[_basic_block(cin if b == 0 else cout, cout, 2 if (b == 0 and li > 1) else 1) for b in range(n)]))
        cin = cout
    return m


class SpatialEncoder(nn.Module):
    """Configuration + parameters of the spatial encoder (reference src/model/encoder.py:13-77).
    backbone 'resnet34' runs in csrc/encoder.hip; backbone 'custom' (YOLOv7, whose source and
    weights are outside the reference tree) has no kernels: its output must be supplied through
    ``PixelNeRFNet.encode(..., latent=...)``."""

    def __init__(self, backbone="resnet34", pretrained=True, num_layers=4, index_interp="bilinear",
                 index_padding="border", upsample_interp="bilinear", feature_scale=1.0, use_first_pool=True,
                 norm_type="batch"):
        super().__init__()
        self.use_custom_resnet = backbone == "custom"
        if self.use_custom_resnet:
            self.latent_size = 1792  # reference custom_encoder.py:22
            self.model = nn.Module()
        else:
            if backbone != "resnet34" or num_layers != 4 or norm_type != "batch" or feature_scale != 1.0:
                raise NotImplementedError("libpnyolo's encoder kernels cover backbone=resnet34, num_layers=4, batch "
                                          "norm, feature_scale=1 (every shipped conf/exp/*.conf)")
            self.latent_size = [0, 64, 128, 256, 512, 1024][num_layers]
            self.model = _resnet34_params()
            # `pretrained` ImageNet weights cannot be downloaded here; they arrive via load_weights
        if index_interp != "bilinear" or index_padding != "zeros" or upsample_interp != "bilinear":
            raise NotImplementedError("libpnyolo supports bilinear indexing with zeros padding "
                                      "(conf/default.conf:49 of the reference)")
        self.num_layers = num_layers
        self.use_first_pool = use_first_pool
        self.index_interp, self.index_padding, self.upsample_interp = index_interp, index_padding, upsample_interp

    def forward_torch(self, x):
        """The trunk as a differentiable torch graph (reference encoder.py:110-173, resnet34 branch): the ATen alternative to the
        library's training trunk (csrc/encoder_train.hip, model._TrunkFunction), taken by ``PixelNeRFNet.encode`` with
        PNYOLO_TRUNK=torch or when the library cannot read the trunk's parameters in place.  Convolutions and batch norms
        (train-mode statistics when ``self.training``) run through ATen and autograd, and the renderer's backward hands
        d loss / d latent back to this graph (pny_scene_bind_latent_grad)."""
        import torch.nn.functional as F
        if self.use_custom_resnet:
            raise RuntimeError("backbone=custom has no trunk here: supply the latent")
        m = self.model

        def block(blk, t):
            out = torch.relu(blk.bn1(blk.conv1(t)))
            out = blk.bn2(blk.conv2(out))
            return torch.relu(out + (blk.downsample(t) if hasattr(blk, "downsample") else t))

        x = torch.relu(m.bn1(m.conv1(x)))
        latents = [x]
        if self.use_first_pool:
            x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        for layer in (m.layer1, m.layer2, m.layer3):
            for blk in layer:
                x = block(blk, x)
            latents.append(x)
        size = latents[0].shape[-2:]
        return torch.cat([F.interpolate(t, size, mode="bilinear", align_corners=True) for t in latents], dim=1)

    @classmethod
    def from_conf(cls, conf):
        return cls(conf.get_string("backbone"), pretrained=conf.get_bool("pretrained", True),
                   num_layers=conf.get_int("num_layers", 4), index_interp=conf.get_string("index_interp", "bilinear"),
                   index_padding=conf.get_string("index_padding", "border"),
                   upsample_interp=conf.get_string("upsample_interp", "bilinear"),
                   feature_scale=conf.get_float("feature_scale", 1.0),
                   use_first_pool=conf.get_bool("use_first_pool", True))


def make_mlp(conf, d_in, d_latent=0, allow_empty=False, **kwargs):
    """reference src/model/model_util.py:5-15"""
    mlp_type = conf.get_string("type", "mlp")
    if mlp_type == "resnet":
        return ResnetFC.from_conf(conf, d_in, d_latent=d_latent, **kwargs)
    if mlp_type == "empty" and allow_empty:
        return None
    raise NotImplementedError("Unsupported MLP type (libpnyolo implements type = resnet)")


def make_encoder(conf, **kwargs):
    """reference src/model/model_util.py:18-26"""
    if conf.get_string("type", "spatial") != "spatial":
        raise NotImplementedError("Unsupported encoder type")
    return SpatialEncoder.from_conf(conf, **kwargs)


# ------------------------------------------------------------------ the model
class PixelNeRFNet(nn.Module):
    """Drop-in for reference src/model/models.py:15 (constructor :16-90, encode :92-151,
    forward :153-318, load/save_weights :320-370)."""

    def __init__(self, conf, stop_encoder_grad=False):
        super().__init__()
        # native handles (created lazily on the module's CUDA device); first, so that _free_native() finds them on an object
        # whose construction raised below
        self._h_model = None
        self._h_device = None
        self._h_has_fine = False
        self._h_scenes = []
        # Super-batch in ONE scene (include/pnyolo.h pny_scene_set_groups): the training render of SB > 1 objects runs on this
        # handle -- one MLP launch per pass over every object's tiles.  _group = dict(SB, NS) while it holds the last encode();
        # the per-object handles are then filled on first use (_scenes_pending: the encode()'s cameras, _fill_scene).
        self._h_group = None
        self._group = None
        self._scenes_pending = None
        self._conf = conf                  # kept for replicas on other devices (render._MultiDeviceRenderWrapper)
        self._encode_epoch = 0             # bumped by every encode(): replicas re-fetch the scene state when it moved
        self._last_encode = None
        self.encoder = make_encoder(conf["encoder"])
        self.use_encoder = conf.get_bool("use_encoder", True)
        self.use_xyz = conf.get_bool("use_xyz", False)
        self.normalize_z = conf.get_bool("normalize_z", True)
        self.stop_encoder_grad = stop_encoder_grad
        self.use_code = conf.get_bool("use_code", False)
        self.use_code_viewdirs = conf.get_bool("use_code_viewdirs", True)
        self.use_viewdirs = conf.get_bool("use_viewdirs", False)
        self.use_global_encoder = conf.get_bool("use_global_encoder", False)
        if not (self.use_encoder and self.use_xyz and self.normalize_z and self.use_code and self.use_viewdirs
                and not self.use_code_viewdirs and not self.use_global_encoder):
            raise NotImplementedError(
                "libpnyolo implements the shipped flag set: use_encoder, use_xyz, normalize_z, use_code, "
                "use_viewdirs, not use_code_viewdirs, no global encoder (conf/default.conf of the reference)")
        d_latent = self.encoder.latent_size
        self.code = PositionalEncoding.from_conf(conf["code"], d_in=3)
        if not self.code.include_input:
            raise NotImplementedError("code.include_input = False is not supported")
        d_in = self.code.d_out + 3
        self.latent_size = self.encoder.latent_size
        self.mlp_coarse = make_mlp(conf["mlp_coarse"], d_in, d_latent)
        # assignable: eval.py:140 of the reference sets `net.mlp_fine = None` for coarse-only runs
        self.mlp_fine = make_mlp(conf["mlp_fine"], d_in, d_latent, allow_empty=True)
        self.yolo = conf.get_bool("mlp_coarse.yolo", False)
        self.d_in = d_in
        if not self.yolo:
            self.d_out = conf.get_int("mlp_coarse.d_out", 4)
        else:
            self.d_out = conf.get_int("mlp_coarse.d_out", 7) * conf.get_int("mlp_coarse.num_anchors_per_scale", 3)
        self.d_latent = d_latent
        self.num_objs = 0
        self.num_views_per_obj = 1
        self._last_call_group = False
        self._tracked, self._tracked_sig = [], None   # _weights_key: the (name, tensor) list and the structure it was built for
        self._synced_key = None            # the weights key the native copy holds
        self._dev_bound = False            # the library reads every MLP parameter in place (pny_model_bind_param)
        self._trunk_bound = False          # ... and every parameter of the trunk: the training trunk can run
        self._enc_stale = False            # the inference trunk's folded copy is behind the live encoder tensors
        self._latent_src = None            # the latent of the last encode() that takes a gradient (differentiable_latent)
        self._latent_channel_last = False  # ... stands for a list of feature maps: (SB * NS, Hl, Wl, L) (latent_meta)
        self._defer_token = 0              # bumped by every training forward: whose stash reservation is it (render._RenderFunction)
        self._bound_grads = None           # the flat gradient buffer of the last backward, alive while it is bound
        self._side_streams, self._flush_stream, self._trunk_stream = None, None, None   # _own_streams: made on first use
        self._lat_grad_event = None        # where the last latent gradient was complete (render._mark_latent_grad)
        self._last_trunk_wait = None       # which ordering the last trunk backward took (for the tests)
        self._trunk_generation = 0         # bumped by every training-trunk forward: whose activations does the library hold
        self._timing = False
        self._occupancy = None             # set_occupancy: the grid attached to the one encoded object
        self._termination = None           # set_termination: (t_min, segments), a rendering option that outlives encode()
        # What a no-grad call does when one of its f16 (F16X2 / F16) launches met a value outside the f16 range (include/pnyolo.h
        # pny_model_range_status): 'relaunch' (default) = wait for the call, and if the guard fired repeat it on the fp32
        # kernels with a warning, keeping the scenes pinned to f32 from then on; 'raise' = wait and raise PnyRangeError;
        # 'lazy' = do not wait: the next library call on the model fails with PNY_ERR_RANGE (what training calls always do --
        # their launches overlap on side streams).  Env PNYOLO_F16_RANGE.
        self.f16_range_policy = os.environ.get("PNYOLO_F16_RANGE", "relaunch")
        self._projection = None  # None = library default (auto, or env PNYOLO_PROJECTION)
        self._precision = None   # None = library default (auto, or env PNYOLO_MLP_PRECISION)
        self._deterministic = "auto"   # set_deterministic: the latent gradient's path, decided at every backward

    # ---------------------------------------------------------------- native plumbing
    def _device(self):
        dev = self.mlp_coarse.lin_in.weight.device
        if dev.type != "cuda":
            raise RuntimeError("PixelNeRFNet (libpnyolo) runs on an MI355X only: move the module to a cuda device "
                               "first (there is no CPU path)")
        return dev

    def _free_native(self):
        L = _lib.load()
        for s in self._h_scenes:
            L.pny_scene_destroy(s)
        self._h_scenes = []
        if self._h_group is not None:
            L.pny_scene_destroy(self._h_group)
        self._h_group, self._group, self._scenes_pending = None, None, None
        if self._h_model is not None:
            L.pny_model_destroy(self._h_model)
            self._h_model = None
        self._dev_bound = False

    def __del__(self):
        try:
            self._free_native()
        except Exception:
            pass

    def _weights_key(self):
        """Identity of every parameter / buffer value: (storage pointer, in-place version counter).  Building the
        state_dict costs ~170 us per call, so the tensor list is cached and rebuilt only after a structural change
        anywhere (a parameter, buffer or submodule registered or replaced: PyTorch's global registration hooks bump
        _STRUCT_EPOCH) or when the fine MLP is attached / detached."""
        sig = (_STRUCT_EPOCH[0], id(self.mlp_fine))
        if sig != self._tracked_sig:
            self._tracked = list(self.state_dict(keep_vars=True).items())
            self._tracked_sig = sig
        return tuple((k, v.data_ptr(), v._version) for k, v in self._tracked)

    def _sync(self):
        """Create the native model on first use; re-upload weights when parameters changed
        (load_weights, load_state_dict, optimizer step).  Scenes survive a weight reload; a move to
        another device rebuilds everything."""
        L = _lib.load()
        dev = self._device()
        if self._h_model is not None and self._h_device != str(dev):
            self._free_native()
        key = self._weights_key()
        if self._h_model is None:
            mc = self.mlp_coarse
            has_fine = any(k[0].startswith("mlp_fine.") for k in key)
            desc = ModelDesc(d_latent=self.d_latent, d_hidden=mc.d_hidden, d_out=self.d_out, n_blocks=mc.n_blocks,
                             combine_layer=min(mc.combine_layer, 1 << 20), num_freqs=self.code.num_freqs,
                             freq_factor=float(self.code.freq_factor), yolo=int(self.yolo),
                             has_fine=int(has_fine), device=dev.index or 0,
                             enc_use_first_pool=int(getattr(self.encoder, "use_first_pool", True)))
            h = C.c_void_p()
            check(L.pny_model_create(C.byref(h), C.byref(desc)))
            self._h_model, self._h_device, self._h_has_fine, self._synced_key = h, str(dev), has_fine, None
        if self.mlp_fine is not None and not self._h_has_fine:
            raise RuntimeError("a fine MLP was attached after the native model was created without one")
        if key != self._synced_key:
            h = self._h_model
            if self._follows_in_place(self._synced_key, key):
                self._mark_trunk_stale(self._synced_key, key)
                check(L.pny_model_refresh(h, stream_of(dev)))
            else:
                for name, t in self.state_dict().items():
                    if name.endswith("num_batches_tracked"):
                        continue
                    a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
                    shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
                    check(L.pny_model_load_weights(h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
                check(L.pny_model_finalize(h))
                self._enc_stale = False
                self._dev_bound = True
                self._trunk_bound = True
                for name, t in self.state_dict(keep_vars=True).items():
                    if name.startswith("mlp_"):
                        ok = t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                        self._dev_bound = self._dev_bound and ok
                        if ok:
                            check(L.pny_model_bind_param(h, name.encode(), C.c_void_p(t.data_ptr())))
                    elif name.startswith("encoder.model.") and not name.endswith("num_batches_tracked") \
                            and not name.startswith(("encoder.model.layer4", "encoder.model.fc")):
                        # the training-mode trunk (pny_trunk_train_forward / _backward) reads its parameters and steps the
                        # running statistics where PyTorch keeps them
                        ok = t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                        self._trunk_bound = self._trunk_bound and ok
                        if ok:
                            check(L.pny_model_bind_param(h, name.encode(), C.c_void_p(t.data_ptr())))
            self._synced_key = key
        # `net.mlp_fine = None` (reference eval.py:140): fine pass falls back to the coarse MLP
        check(L.pny_model_use_fine(self._h_model, int(self.mlp_fine is not None)))

    def _follows_in_place(self, old, new):
        """Can the native copy follow the change of the weights key from `old` to `new` on the device, without a re-upload?
        Yes when it reads the MLP parameters in place and only MLP or encoder tensors changed IN PLACE (same storage, new
        version: an optimizer step).  _sync() then refreshes the packed operands with one launch; optim.Adam's step does it
        in its own launch.  Anything else (a tensor replaced, a buffer outside them written) is a re-upload."""
        return (old is not None and self._dev_bound and len(old) == len(new) and
                all(a[:2] == b[:2] and (a[2] == b[2] or a[0].startswith(("mlp_", "encoder."))) for a, b in zip(old, new)))

    def _mark_trunk_stale(self, old, new):
        """Encoder tensors stepped in place between the keys `old` and `new` (encoder training: the training trunk reads the
        live parameters itself) only mark the INFERENCE trunk's folded copy stale; it is re-uploaded when that trunk is next
        needed (encode() outside training)."""
        if any(a[2] != b[2] and a[0].startswith("encoder.") for a, b in zip(old, new)):
            self._enc_stale = True

    def _new_scene(self, group=False):
        L = _lib.load()
        s = C.c_void_p()
        check(L.pny_scene_create(C.byref(s), self._h_model))
        check(L.pny_scene_enable_timing(s, int(self._timing)))
        if self._projection is not None:
            check(L.pny_scene_set_projection(s, _lib.PROJECTION[self._projection]))
        if self._precision is not None:
            check(L.pny_scene_set_precision(s, _lib.PRECISION[self._precision]))
        if self._termination is not None and not group:
            check(L.pny_scene_set_termination(s, *self._termination))
        return s

    def _scene(self, i):
        if self._scenes_pending is not None:
            self._materialise_scenes()
        while len(self._h_scenes) <= i:
            self._h_scenes.append(self._new_scene())
        return self._h_scenes[i]

    def _group_scene(self):
        """The handle that holds a whole super-batch (pny_scene_set_groups); None unless the last encode() filled it."""
        return self._h_group if self._group is not None else None

    def _handles(self):
        return list(self._h_scenes) + ([self._h_group] if self._h_group is not None else [])

    def _last_grouped(self):
        """True when the last render call was one launch on the grouped scene, which then holds the call's records."""
        return self._last_call_group and self._group is not None

    def _last_handle(self, scene):
        """The handle that holds the last call's records of object `scene`."""
        return self._h_group if self._last_grouped() else self._scene(scene)

    def _stat_handles(self):
        return [self._h_group] if self._last_grouped() else self._h_scenes[: max(self.num_objs, 1)]

    @staticmethod
    def _cam_rows(t, sb, SB, NS):
        """focal / c rows of object sb: batch 1 broadcasts, batch SB is per object, batch SB*NS per view."""
        if t.shape[0] == 1:
            return t[:1]
        if t.shape[0] == SB * NS:
            return t[sb * NS:(sb + 1) * NS]
        if t.shape[0] == SB:
            return t[sb:sb + 1]
        raise ValueError("focal / c batch must be 1, SB or SB*NS")

    def _fill_scene(self, s, cams, first, count, n_objs=1, levels=None, latent=None, images=None):
        """Give scene handle `s` the views [first, first + count) of an encode(): their cameras (`cams`: the host-side poses
        (SB * NS, 4, 4), focal and c rows, W, H, SB, NS) and their latent from ONE source, on the current stream -- the
        feature maps (`levels` = (device maps, their shapes): pny_scene_set_latent_levels), a latent tensor
        (SB * NS, L, Hl, Wl) on the device (the caller's, or the rows copied out of the grouped handle), or the images (the
        library's trunk).  No source: the scene is encoded already (pny_scenes_encode).  One object's scene takes that object's
        focal / c rows as they are (the library broadcasts a single row); n_objs > 1 makes `s` the grouped scene of that
        many objects (pny_scene_set_groups), with one row per view."""
        L = _lib.load()
        st = stream_of(self._device())
        SB, NS = cams["SB"], cams["NS"]

        def rows(t):
            if n_objs == 1:
                return self._cam_rows(t, first // NS, SB, NS).contiguous()
            return torch.cat([self._cam_rows(t, sb, SB, NS).expand(NS, 2) for sb in range(first // NS, (first + count) // NS)],
                             dim=0).contiguous()
        f, c, p = rows(cams["focal"]), rows(cams["c"]), cams["poses"][first:first + count].contiguous()
        check(L.pny_scene_set_cameras(s, ptr(p), count, ptr(f), f.shape[0], ptr(c), c.shape[0], cams["W"], cams["H"]))
        if n_objs > 1:
            check(L.pny_scene_set_groups(s, n_objs))
        if levels is not None:
            maps, shapes = levels
            ptrs = (C.c_void_p * len(maps))(*[m[first:first + count].data_ptr() for m in maps])
            ch, hs, ws = _levels_arrays(shapes)
            check(L.pny_scene_set_latent_levels(s, ptrs, ch, hs, ws, len(maps), count, st))
        elif latent is not None:
            lat = latent[first:first + count]
            check(L.pny_scene_set_latent(s, ptr(lat), count, lat.shape[1], lat.shape[2], lat.shape[3], st))
        elif images is not None:
            check(L.pny_scene_encode(s, ptr(images[first:first + count]), count, cams["H"], cams["W"], st))

    def _materialise_scenes(self):
        """Per-object scene handles from the grouped one (cameras from the encode() arguments, latent copied out of it): only
        when something other than the training render asks for them after a grouped encode()."""
        cams, self._scenes_pending = self._scenes_pending, None
        lat = self._read_latent(self._h_group)
        for sb in range(cams["SB"]):
            self._fill_scene(self._scene(sb), cams, sb * cams["NS"], cams["NS"], latent=lat)

    def enable_kernel_timing(self, on=True):
        """HIP-event timing of the MLP launches (bench.py's roofline leg)."""
        self._timing = bool(on)
        for s in self._handles():
            check(_lib.load().pny_scene_enable_timing(s, int(on)))

    def set_latent_projection(self, mode):
        """'auto' | 'on' | 'off' (include/pnyolo.h pny_scene_set_projection): whether the fused kernel
        interpolates per-scene projected latent maps (lin_z applied once per latent pixel) or runs the
        lin_z GEMMs per sample in the reference's operation order."""
        if mode not in _lib.PROJECTION:
            raise ValueError("latent projection mode must be one of %s" % sorted(_lib.PROJECTION))
        self._projection = mode
        for s in self._handles():
            check(_lib.load().pny_scene_set_projection(s, _lib.PROJECTION[mode]))
        return self

    def set_matrix_precision(self, mode):
        """'auto' | 'f32' | 'f16x2' | 'f16' (include/pnyolo.h pny_scene_set_precision): the matrix arithmetic of projected
        launches -- fp32 MFMA, or fp32 operands split into two f16 planes on the f16 matrix cores (same measured
        error, 5.3x the matrix rate).  'f16' (opt-in, outside the 1e-4 parity bar) runs no-grad projected
        launches on ONE f16 plane per operand; training forwards and backwards of an 'f16' model run as 'auto'.
        'f16_train' (opt-in, outside the parity bar) runs no-grad launches as 'f16' and training too on one
        f16 plane per operand: the stashing forward, the dX chain, the weight and latent gradients (fp32 accumulation,
        power-of-two gradient scaling inside the library, fp32 parameters and gradients).
        Launches without projection always run fp32.  Applies to every scene handle, the grouped one included."""
        if mode not in _lib.PRECISION:
            raise ValueError("matrix precision must be one of %s" % sorted(_lib.PRECISION))
        self._precision = mode
        for s in self._handles():
            check(_lib.load().pny_scene_set_precision(s, _lib.PRECISION[mode]))
        return self

    def set_occupancy(self, grid):
        """Attach ``grid`` (recon.OccupancyGrid, from ``recon.occupancy_grid``) to the ONE encoded object, or detach with None
        (include/pnyolo.h pny_scene_set_occupancy; csrc/pny_occupancy.h).  No-grad renders then evaluate the MLPs only at the depth
        samples the grid keeps and composite as if the others had returned (0, 0, 0, 0): an opt-in, approximate mode, like
        set_matrix_precision('f16').  Each render waits for the device twice (the kept count of each pass).  The scene copies the
        bits.  ``encode()`` drops the grid; queries, YOLO renders and training ignore or refuse it."""
        L = _lib.load()
        if grid is None:
            if self._h_model is not None:
                for s in self._handles():
                    check(L.pny_scene_set_occupancy(s, None, None, None, None, 0, None))
            self._occupancy = None
            return self
        if self.yolo:
            raise _lib.PnyError("PixelNeRFNet.set_occupancy: a YOLO model aggregates by objectness, not by sigma; an occupancy grid "
                                "does not apply to it")
        if self.num_objs != 1:
            raise _lib.PnyError("PixelNeRFNet.set_occupancy: net must hold ONE encoded object (call net.encode() with one object "
                                "first); it holds %d" % self.num_objs)
        self._sync()
        dev = self._device()
        bits = grid.bits
        if bits.device != dev or bits.dtype != torch.uint32 or not bits.is_contiguous():
            raise ValueError("PixelNeRFNet.set_occupancy: grid.bits must be a contiguous uint32 tensor on %s" % dev)
        d, a, b = (C.c_int32 * 3)(*grid.dims), (C.c_double * 3)(*grid.c1), (C.c_double * 3)(*grid.c2)
        with torch.cuda.device(dev):
            check(L.pny_scene_set_occupancy(self._scene(0), C.c_void_p(bits.data_ptr()), d, a, b, int(grid.outside_empty), stream_of(dev)))
        self._occupancy = grid
        return self

    @property
    def occupancy(self):
        """The attached recon.OccupancyGrid, or None."""
        return self._occupancy

    def last_cull(self):
        """{"coarse": (kept, total), "fine": (kept, total)} samples of the last render of the object; zeros when it used no grid
        (include/pnyolo.h pny_scene_last_cull)."""
        kept, total = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        check(_lib.load().pny_scene_last_cull(self._scene(0), kept, total))
        return {"coarse": (int(kept[0]), int(total[0])), "fine": (int(kept[1]), int(total[1]))}

    def set_termination(self, t_min, segments=4):
        """Early ray termination for no-grad renders of the ONE encoded object, or off with ``t_min=None`` (include/pnyolo.h
        pny_scene_set_termination; csrc/pny_termination.h).  Each pass is rendered in ``segments`` (1 .. 16) depth-ordered segments,
        and a ray whose transmittance has fallen below ``t_min`` (0 < t_min < 1) at a segment boundary is not evaluated in the
        later ones; the composite sees (0, 0, 0, 0) there.  An opt-in, approximate mode, like set_occupancy, and it works with or
        without a grid; how close the frame stays to the default one is the caller's choice of ``t_min`` (there is no default).
        Each render waits for the device once per issued segment.  The setting is a rendering option, not a property of the
        encoded object: UNLIKE the grid, which ``encode()`` drops, it survives ``encode()``.  Queries, YOLO renders and training
        ignore or refuse it."""
        L = _lib.load()
        if t_min is None:
            if self._h_model is not None:
                for s in self._handles():
                    check(L.pny_scene_set_termination(s, 0.0, 1))
            self._termination = None
            return self
        t_min, segments = float(t_min), int(segments)
        if not 0.0 < t_min < 1.0:
            raise ValueError("PixelNeRFNet.set_termination: t_min must be in (0, 1) (None switches the mode off), got %r" % t_min)
        if not 1 <= segments <= 16:
            raise ValueError("PixelNeRFNet.set_termination: segments must be in 1 .. 16, got %d" % segments)
        if self.yolo:
            raise _lib.PnyError("PixelNeRFNet.set_termination: a YOLO model aggregates by objectness, not by sigma; early ray "
                                "termination does not apply to it")
        if self.num_objs != 1:
            raise _lib.PnyError("PixelNeRFNet.set_termination: net must hold ONE encoded object (call net.encode() with one object "
                                "first); it holds %d" % self.num_objs)
        self._sync()
        self._termination = (t_min, segments)
        self._scene(0)                     # (a handle created from here on takes the setting in _new_scene)
        for s in self._h_scenes:
            check(L.pny_scene_set_termination(s, t_min, segments))
        return self

    @property
    def termination(self):
        """(t_min, segments) of set_termination, or None."""
        return self._termination

    def last_termination(self):
        """{"coarse": [(alive_rays, kept), ...], "fine": [...]}: per pass of the last render of the object, the rays alive in and
        the samples evaluated by every segment that was issued (include/pnyolo.h pny_scene_last_segments).  One segment per pass
        with only a grid attached, none when the render took no culled path."""
        out = {}
        for i, name in enumerate(("coarse", "fine")):
            alive, kept, n = (C.c_int64 * 16)(), (C.c_int64 * 16)(), C.c_int(0)
            check(_lib.load().pny_scene_last_segments(self._scene(0), i, alive, kept, 16, C.byref(n)))
            out[name] = [(int(alive[j]), int(kept[j])) for j in range(n.value)]
        return out

    def set_deterministic(self, mode):
        """'auto' | True | False: whether d loss / d latent is computed bit-reproducibly (include/pnyolo.h
        pny_model_set_deterministic: exact fixed-point sums instead of float atomics; the one gradient of the library that is
        not deterministic otherwise).  'auto' (default) follows torch.use_deterministic_algorithms at every backward.  False
        under torch's flag makes a backward that computes a latent gradient raise, as torch's own nondeterministic ops do
        (a warning under warn_only).  Applies to every scene handle and to bind_parallel's replicas."""
        if not (mode is True or mode is False or (isinstance(mode, str) and mode == "auto")):
            raise ValueError("deterministic mode must be 'auto', True or False, not %r" % (mode,))
        self._deterministic = mode
        return self

    def _latent_grad_deterministic(self):
        """Decide the latent gradient's path for the backward about to run (set_deterministic) and hand it to the library."""
        flag = torch.are_deterministic_algorithms_enabled()
        det = flag if self._deterministic == "auto" else self._deterministic
        if flag and not det:
            msg = ("the latent gradient of PixelNeRFNet (float-atomic scatter) does not have a deterministic implementation "
                   "under set_deterministic(False), but torch.use_deterministic_algorithms(True) is set: call "
                   "net.set_deterministic(True) or 'auto'")
            if not torch.is_deterministic_algorithms_warn_only_enabled():
                raise RuntimeError(msg)
            warnings.warn(msg)
        check(_lib.load().pny_model_set_deterministic(self._h_model, int(det)))

    def last_latent_grad_deterministic(self, scene=0):
        """True when the last backward of scene `scene` (or of the grouped scene, when the last call was grouped) that
        computed a latent gradient took the deterministic path (include/pnyolo.h pny_scene_last_latent_grad_mode)."""
        return bool(_lib._get_int(_lib.load().pny_scene_last_latent_grad_mode, self._last_handle(scene)))

    def range_status(self, clear=False):
        """Bits (include/pnyolo.h PNY_RANGE_*) the F16X2 kernels of this model have reported so far; does not synchronise."""
        if self._h_model is None:
            return 0
        v = C.c_uint(0)
        check(_lib.load().pny_model_range_status(self._h_model, C.byref(v), int(bool(clear))))
        return int(v.value)

    def check_f16_range(self):
        """Wait for the device and raise PnyRangeError if an f16 (F16X2 / F16) launch left the f16 range since the last clear."""
        if self._h_model is None:
            return
        torch.cuda.synchronize(self._device())
        bits = self.range_status(clear=True)
        if bits:
            raise _lib.PnyRangeError(self._range_message(bits))

    @staticmethod
    def _range_message(bits):
        what = ", ".join(n for b, n in sorted(_lib.RANGE_BITS.items()) if bits & b)
        return ("an f16 (F16X2 / F16) launch met a value outside the f16 range (%s: |x| >= 65520, infinite or NaN); its results are "
                "invalid.  Pin the fp32 kernels with net.set_matrix_precision('f32') (or PNYOLO_MLP_PRECISION=f32)" % what)

    def guard_f16_range(self, call):
        """Runs a no-grad render / query (`call`, repeatable) under `f16_range_policy` and returns its result.  The guard can
        fire in two places: inside the call, when the flag was already up when it entered the library (a weight repacked out
        of range by the refresh of this very call, a lazily reported earlier launch: PnyRangeError from the library), or
        after it, when one of its own F16X2 launches met the value (found by waiting for the stream)."""
        pol = self.f16_range_policy
        try:
            out = call()
            if pol == "lazy" or not any(self.last_launch_f16x2(i) for i in range(len(self._h_scenes))):
                return out
            torch.cuda.current_stream(self._device()).synchronize()
            bits = self.range_status(clear=False)
            if not bits:
                return out
        except _lib.PnyRangeError:
            if pol != "relaunch":
                raise
            bits = self.range_status(clear=False)
        self.range_status(clear=True)
        if pol == "raise":
            raise _lib.PnyRangeError(self._range_message(bits))
        warnings.warn("libpnyolo: " + self._range_message(bits) + " -- repeating the call on the fp32 kernels; this model "
                      "stays on them (f16_range_policy = 'relaunch')")
        self.set_matrix_precision("f32")
        return call()

    def last_launch_f16x2(self, scene=0):
        """True when the last MLP launch of scene `scene` ran an f16-family kernel (f16x2 or f16): the range guard applies."""
        return self._last_precision_code(scene) != 0

    def last_launch_precision(self, scene=0):
        """The arithmetic of the last MLP launch of scene `scene`: 'f32' | 'f16x2' | 'f16'."""
        return _lib.LAST_PRECISION[self._last_precision_code(scene)]

    def last_backward_precision(self, scene=0):
        """The arithmetic of the dX chain of the last backward of scene `scene` (or of the grouped scene, when the last
        call was grouped): 'f32' | 'f16x2' | 'f16' (include/pnyolo.h pny_scene_last_backward_precision)."""
        return _lib.LAST_PRECISION[_lib._get_int(_lib.load().pny_scene_last_backward_precision, self._last_handle(scene))]

    def _last_precision_code(self, scene):
        return _lib._get_int(_lib.load().pny_scene_last_precision, self._last_handle(scene))

    def project_latent(self):
        """Compute the projected maps of the encoded scenes now (otherwise done lazily by the first
        large render call after encode)."""
        self._sync()
        for i in range(self.num_objs):
            check(_lib.load().pny_scene_project(self._scene(i), stream_of(self._device())))
        return self

    def last_mlp_stats(self, full=False):
        """(executed GEMM FLOPs, kernel ms, launches) of the last call, summed over scenes; with
        full=True a dict that also carries the reference-order FLOP count and the projection flag."""
        L = _lib.load()
        fl = ref = ms = 0.0
        n = 0
        proj = False
        for s in self._stat_handles():
            a, r, b, c, p = C.c_double(), C.c_double(), C.c_double(), C.c_int(), C.c_int()
            check(L.pny_scene_last_mlp_stats(s, C.byref(a), C.byref(r), C.byref(b), C.byref(c), C.byref(p)))
            fl += a.value
            ref += r.value
            ms += b.value
            n += c.value
            proj = proj or bool(p.value)
        if full:
            return dict(flops=fl, flops_reference=ref, kernel_ms=ms, launches=n, projected=proj)
        return fl, ms, n

    def last_backward_stats(self):
        """dict(flops=[3], kernel_ms=[3]) of the last backward call, summed over scenes: stash forward, dX chain,
        weight-gradient GEMMs (include/pnyolo.h pny_scene_last_backward_stats)."""
        L = _lib.load()
        fl, ms = [0.0] * 3, [0.0] * 3
        for s in self._stat_handles():
            a, b = (C.c_double * 3)(), (C.c_double * 3)()
            check(L.pny_scene_last_backward_stats(s, a, b))
            for i in range(3):
                fl[i] += a[i]
                ms[i] += b[i]
        return dict(flops=fl, kernel_ms=ms)

    # ---------------------------------------------------------------- training plumbing
    def trainable_mlp_parameters(self):
        """[(state_dict name, Parameter)] of the MLP parameters that require grad, in a fixed order."""
        out = []
        for pre, mlp in (("mlp_coarse.", self.mlp_coarse), ("mlp_fine.", self.mlp_fine)):
            if mlp is not None:
                out += [(pre + k, p) for k, p in mlp.named_parameters() if p.requires_grad]
        return out

    def check_differentiable(self):
        """Called by a training render / query when the latent of the last encode() carries no graph.  Fine with a frozen
        encoder (reference: --freeze_enc / stop_encoder_grad, train/train.py:70-73, models.py:33-35); with a trainable one the
        gradient would silently stop at the latent, so this is an error: encode() must run in train() mode with grad enabled
        (the library's training trunk, model._TrunkFunction) or be given a latent that requires grad."""
        if not self.stop_encoder_grad and any(p.requires_grad for p in self.encoder.parameters()):
            raise NotImplementedError(
                "the encoder has trainable parameters but the latent of the last encode() carries no graph (encode() ran in "
                "eval() mode or under no_grad): call net.encode(...) in train() mode with grad enabled, or freeze the encoder "
                "(make_model(conf, stop_encoder_grad=True) / requires_grad_(False) on net.encoder, the reference's --freeze_enc)")

    def differentiable_latent(self):
        """The latent tensor of the last encode(latent=...) if it requires grad and autograd is recording in train() mode
        (the render / query backward then returns d loss / d latent for it), else None."""
        if torch.is_grad_enabled() and self.training:
            return self._latent_src
        return None

    def latent_meta(self, lat):
        """What a render / query backward needs of the differentiable latent `lat`: ((SB * NS, L, Hl, Wl), device, dtype,
        channel-last).  A tensor latent is NCHW and takes its gradient in that layout; the stand-in of a list of feature maps
        (_LevelsFunction) is shaped like the library's own (SB * NS, Hl, Wl, L) buffer and takes that buffer as it is."""
        if self._latent_channel_last:
            n, hl, wl, l_ch = lat.shape
            return (n, l_ch, hl, wl), lat.device, lat.dtype, True
        return tuple(lat.shape), lat.device, lat.dtype, False

    @contextlib.contextmanager
    def latent_grad(self, meta, handles):
        """``with net.latent_grad(meta, handles) as lg:`` around the library's backward calls on the scene handles, for the
        latent that `meta` describes (latent_meta).  Entry: a zeroed (SB * NS, Hl, Wl, L) accumulator bound in equal slices to
        the handles (pny_scene_bind_latent_grad): the per-object scenes take their own views each, the grouped scene takes it
        whole.  Its zero fill runs on the current stream, so enter BEFORE side streams fork from that stream.  ``lg.result()``
        unbinds and is what the backward returns for the latent: (gradient,) in the latent's own layout (SB * NS, L, Hl, Wl),
        device and dtype -- for a list of feature maps the channel-last buffer itself, which pny_latent_levels_backward reads
        (_LevelsFunction) -- or () for meta = None (no differentiable latent: nothing is bound).  A block that raises leaves
        nothing bound either: the buffer dies with the exception, and a scene left bound to it would accumulate into freed
        memory (or fail again) in its next backward."""
        if meta is None:
            yield types.SimpleNamespace(result=tuple)
            return
        bind = _lib.load().pny_scene_bind_latent_grad
        (n_lat, l_ch, hl, wl), lat_dev, lat_dtype, channel_last = meta
        self._latent_grad_deterministic()
        buf = torch.zeros(n_lat, hl, wl, l_ch, device=self._device(), dtype=torch.float32)
        nsv = n_lat // len(handles)
        for i, h in enumerate(handles):
            check(bind(h, ptr(buf[i * nsv:(i + 1) * nsv])))

        def result():
            for h in handles:
                check(bind(h, None))
            return (buf if channel_last else buf.permute(0, 3, 1, 2).contiguous().to(lat_dev, lat_dtype),)   # packed NCHW
        try:
            yield types.SimpleNamespace(result=result)
        except Exception:
            for h in handles:
                bind(h, None)
            raise

    def _bind_flat_grads(self, named_shapes, dev):
        """Zeroed gradient buffers on `dev` for (state_dict name, shape) pairs, bound to the native model by name
        (pny_model_bind_grad) -> (flat, buffers in the same order).  The buffers are views of ONE flat allocation (one fill, on
        the current stream, instead of one per tensor) and start at multiples of 64 floats (the reduction writes float4 rows)."""
        sizes = [int(np.prod(shape)) for _, shape in named_shapes]
        offs = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in sizes])]).astype(np.int64)
        flat = torch.zeros(max(int(offs[-1]), 1), device=dev, dtype=torch.float32)
        grads = [flat[int(o):int(o) + n].view(shape) for o, n, (_, shape) in zip(offs, sizes, named_shapes)]
        for (name, _), g in zip(named_shapes, grads):
            check(_lib.load().pny_model_bind_grad(self._h_model, name.encode(), ptr(g)))
        return flat, grads

    def bind_mlp_grads(self):
        """Fresh zeroed gradient buffers for trainable_mlp_parameters(), bound to the native model by name; returns them in
        the same order.  Only the flat tensor they are views of is kept alive here, so that autograd's AccumulateGrad can
        adopt the returned views as `.grad` instead of cloning each of them."""
        self._sync()
        named_shapes = [(k, tuple(p.shape)) for k, p in self.trainable_mlp_parameters()]
        self._bound_grads, grads = self._bind_flat_grads(named_shapes, self._device())
        return grads

    def _own_streams(self, attr, dev, n=None):
        """self.<attr>, the side streams this model keeps for one purpose, on `dev`: a list of at least n streams (n = None:
        a single stream, not a list), made on first use and remade when the device changed or more are needed."""
        have = getattr(self, attr)
        pool = [have] if n is None and have is not None else (have or [])
        if len(pool) < (n or 1) or pool[0].device != dev:
            pool = [torch.cuda.Stream(dev) for _ in range(n or 1)]
            setattr(self, attr, pool[0] if n is None else pool)
        return pool[0] if n is None else pool

    def fork_streams(self, n):
        """n stream contexts for n independent scenes: the current stream for the first scene (None) and n - 1 side streams
        ordered behind it for the others (all None when there is a single scene or PNYOLO_SCENE_STREAMS=0).  The current
        stream takes part because the runtime maps streams onto FOUR hardware queues, one of which is the current stream's:
        with four side streams two scenes of the reference's default super-batch (SB = 4) shared a queue and ran one after
        the other while two queues idled (kernel trace of a training step)."""
        if n <= 1 or os.environ.get("PNYOLO_SCENE_STREAMS", "1") == "0":
            return [None] * n
        dev = self._device()
        pool = self._own_streams("_side_streams", dev, n - 1)
        main = torch.cuda.current_stream(dev)
        for st in pool[:n - 1]:
            st.wait_stream(main)
        return [None] + pool[:n - 1]

    def join_streams(self, streams):
        main = torch.cuda.current_stream(self._device())
        for st in streams:
            if st is not None:
                main.wait_stream(st)

    def last_flush_stats(self):
        """(GEMM FLOPs, kernel ms) of the last deferred weight-gradient flush (pny_model_last_flush_stats)."""
        a, b = C.c_double(), C.c_double()
        check(_lib.load().pny_model_last_flush_stats(self._h_model, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_flush_precision(self):
        """The arithmetic of the last deferred weight-gradient flush's GEMM: 'f32' | 'f16x2' | 'f16'
        (include/pnyolo.h pny_model_last_flush_precision)."""
        return _lib.LAST_PRECISION[_lib._get_int(_lib.load().pny_model_last_flush_precision, self._h_model)]

    def invalidate_weights(self):
        """Force a re-upload of the parameters at the next call.  Needed after writes that PyTorch does not version:
        ``p.data.copy_(w)`` / ``p.data.zero_()`` leave ``p._version`` and ``data_ptr()`` unchanged."""
        self._synced_key = None
        return self

    # ---------------------------------------------------------------- reference API
    def encode(self, images, poses, focal, z_bounds=None, c=None, latent=None):
        """
        :param images (NS, 3, H, W) or (SB, NS, 3, H, W), in [-1, 1]
        :param poses (NS, 4, 4) or (SB, NS, 4, 4) cam->world (YOLO mode: world->cam extrinsics)
        :param focal () or (N) or (N, 2);  :param c None or () or (N) or (N, 2)
        :param latent optional (SB*NS, L, Hl, Wl): encoder bypass (required for backbone=custom); or the list / tuple of
            feature maps (SB*NS, C_i, h_i, w_i) as a pyramid backbone returns it: every map is resized to the first map's size
            (bilinear, align_corners=True) and the channels are concatenated, as the reference's SpatialEncoder.forward does
            for backbone=custom (src/model/encoder.py:126-137) -- in one launch, straight into the scene's channel-last latent
            (pny_scene_set_latent_levels).  Maps that require grad receive d loss / d map from the render / query backward.
        """
        levels = None
        if isinstance(latent, (list, tuple)):
            n_views = int(images.shape[0] * images.shape[1]) if images.dim() == 5 else int(images.shape[0])
            levels = check_latent_levels(latent, n_views, self.d_latent)
        self._sync()
        L = _lib.load()
        dev = self._device()
        if self._occupancy is not None:     # learnt on the object encoded before (the library drops its copy on its own too)
            self.set_occupancy(None)
        if self._termination is not None and images.size(0) != 1:
            raise _lib.PnyError("PixelNeRFNet.encode: the net has early ray termination on (net.set_termination), which serves ONE "
                                "encoded object; this call encodes %d: switch it off with net.set_termination(None)" % images.size(0))
        self.num_objs = images.size(0)
        if images.dim() == 5:
            assert poses.dim() == 4 and poses.size(1) == images.size(1)
            self.num_views_per_obj = images.size(1)
            images = images.reshape(-1, *images.shape[2:])
            poses = poses.reshape(-1, 4, 4)
        else:
            self.num_views_per_obj = 1
        NS, SB = self.num_views_per_obj, self.num_objs
        H, W = int(images.shape[-2]), int(images.shape[-1])
        trains_trunk = (latent is None and not self.encoder.use_custom_resnet and torch.is_grad_enabled() and self.training
                        and not self.stop_encoder_grad and any(p.requires_grad for p in self.encoder.parameters()))
        aten_trunk = trains_trunk and not self._native_trunk_training()
        if latent is None and not self.encoder.use_custom_resnet and not aten_trunk and (H < 32 or W < 32):
            # the library's trunks (pny_scene_encode, pny_trunk_train_forward) need every level of the pyramid at least 2 x 2;
            # only the ATen training graph (forward_torch: PNYOLO_TRUNK=torch, or batch norm modules in mixed modes) takes any size
            raise ValueError("encode(): the library's ResNet-34 trunk needs images of at least 32 x 32 pixels, got %d x %d "
                             "(H x W); pass the latent via encode(..., latent=...) instead" % (H, W))
        focal, c = _camera_pairs(focal), _camera_pairs(c, default=(W * 0.5, H * 0.5))
        poses_h = poses.detach().to("cpu", torch.float32).contiguous()
        self._encode_epoch += 1
        self._last_encode = dict(poses=poses_h.reshape(SB, NS, 4, 4) if images is not None else poses_h, focal=focal, c=c, H=H, W=W,
                                 NS=NS, SB=SB, five_d=self.num_views_per_obj == NS)
        cams = dict(poses=poses_h, focal=focal, c=c, W=W, H=H, SB=SB, NS=NS)   # what _fill_scene reads
        if latent is None and self.encoder.use_custom_resnet:
            raise RuntimeError("backbone=custom (YOLOv7) has no kernels in this build (its source and weights are "
                               "outside the reference tree): pass the backbone output via encode(..., latent=...)")
        # Encoder training (the reference's default: train/train.py without --freeze_enc): the trunk runs on the library's training
        # kernels under autograd (_TrunkFunction; the ATen graph forward_torch as the alternative) and its output enters like a
        # supplied latent; the render backward returns d loss / d latent to it
        if trains_trunk:
            if not aten_trunk:
                tp = self._trunk_trainable()
                latent = _TrunkFunction.apply(self, images.detach().to(dev, torch.float32).contiguous(), *[p for _, p in tp])
            else:   # (batch norm modules in eval() mode under autograd, or parameters the library cannot read in place)
                latent = self.encoder.forward_torch(images.to(dev, torch.float32))
        # a latent that requires grad (this trunk's, or a trainable encoder outside the library): the render backward returns
        # d loss / d latent for it (render._RenderFunction, pny_scene_bind_latent_grad)
        self._latent_src = latent if (torch.is_tensor(latent) and latent.requires_grad) else None
        self._latent_channel_last = levels is not None
        if levels is not None:
            # the maps as the library reads them (fp32, packed NCHW, on the device); the tensor that stands for the assembled
            # latent in the render's graph carries the maps' graph (_LevelsFunction)
            maps = [m.detach().to(dev, torch.float32).contiguous() for m in latent]
            token = _LevelsFunction.apply(self, levels, *latent)
            self._latent_src = token if token.requires_grad else None
            source = dict(levels=(maps, levels))
        elif latent is not None:
            latent = latent.detach().to(dev, torch.float32).contiguous()
            assert latent.dim() == 4 and latent.shape[0] == SB * NS, "latent must be (SB*NS, L, Hl, Wl)"
            source = dict(latent=latent)
        else:
            if self._enc_stale:   # the trunk's weights were trained since their last upload
                self._synced_key = None
                self._sync()
            images = images.detach().to(dev, torch.float32).contiguous()
            source = dict(images=images)
        self._group, self._scenes_pending = None, None
        if (SB > 1 and SB * NS <= 16 and os.environ.get("PNYOLO_GROUP", "1") != "0" and torch.is_grad_enabled() and self.training
                and (self.trainable_mlp_parameters() or self._latent_src is not None)):
            # Training on a super-batch: ONE grouped scene (pny_scene_set_groups) holds every object's views, so that each MLP
            # pass of the render and of its backward is one launch over all objects' tiles (the reference flattens the
            # super-batch the same way, nerf.py:283-288).  The per-object handles are filled only if something asks for them.
            if self._h_group is None:
                self._h_group = self._new_scene(group=True)
            self._fill_scene(self._h_group, cams, 0, SB * NS, n_objs=SB, **source)
            self._group = dict(SB=SB, NS=NS)
            self._scenes_pending = cams
            return
        scenes = [self._scene(sb) for sb in range(SB)]
        # the library's trunk over a super-batch: ONE pass over all SB * NS images (as the reference's encode flattens them),
        # cameras per scene below
        batch_encode = "images" in source and SB > 1
        if batch_encode:
            arr = (C.c_void_p * SB)(*[s_ for s_ in scenes])
            check(L.pny_scenes_encode(arr, SB, ptr(images), NS, H, W, stream_of(dev)))
            source = {}
        streams = [None] * SB if batch_encode else self.fork_streams(SB)   # independent scenes: one stream each
        for sb in range(SB):
            with torch.cuda.stream(streams[sb]):
                self._fill_scene(scenes[sb], cams, sb * NS, NS, **source)
        self.join_streams(streams)

    # ---------------------------------------------------------------- encoder training on the library's trunk
    def _trunk_bn_modules(self):
        m = self.encoder.model
        mods = [m.bn1]
        for layer in (m.layer1, m.layer2, m.layer3):
            for blk in layer:
                mods += [blk.bn1, blk.bn2] + ([blk.downsample[1]] if hasattr(blk, "downsample") else [])
        return mods

    def _native_trunk_training(self):
        """The training-mode trunk runs on the library's kernels (csrc/encoder_train.hip) when batch norm works on batch
        statistics (every BatchNorm2d of the trunk in train() mode, momentum set, affine) and the parameters are readable in
        place; PNYOLO_TRUNK=torch forces the ATen graph (SpatialEncoder.forward_torch)."""
        if os.environ.get("PNYOLO_TRUNK", "native") == "torch" or not self._trunk_bound:
            return False
        bns = self._trunk_bn_modules()
        return (all(b.momentum is not None and b.affine and b.track_running_stats for b in bns)
                and len({bool(b.training) for b in bns}) == 1)     # all on batch statistics, or all on the running ones

    def _trunk_trainable(self):
        """(state_dict name, parameter) of the trunk parameters that take a gradient (layer4 / fc are not part of the trunk)."""
        return [("encoder." + k, p) for k, p in self.encoder.named_parameters()
                if p.requires_grad and k.startswith("model.") and not k.startswith(("model.layer4", "model.fc"))]

    def latent(self, sb=0):
        """(NS, L, Hl, Wl) latent of scene `sb` as the reference keeps it in encoder.latent."""
        return self._read_latent(self._scene(sb))

    def _read_latent(self, s):
        """The latent that scene handle `s` holds, (ns, L, Hl, Wl), copied out on the current stream."""
        L = _lib.load()
        dims = [C.c_int() for _ in range(4)]
        check(L.pny_scene_latent_shape(s, *[C.byref(d) for d in dims]))
        out = torch.empty([d.value for d in dims], device=self._device(), dtype=torch.float32)
        check(L.pny_scene_get_latent(s, ptr(out), stream_of(out.device)))
        return out

    def forward(self, xyz, coarse=True, viewdirs=None, far=False):
        """
        Predict (r, g, b, sigma) at world space points xyz (after encode()).
        :param xyz (SB, B, 3);  :param viewdirs (SB, B, 3)  ->  (SB, B, d_out)
        """
        if torch.is_grad_enabled() and xyz.requires_grad:
            raise RuntimeError("libpnyolo does not differentiate w.r.t. the query points: detach xyz")
        # autograd path in train() mode only: eval-mode calls outside no_grad (the reference's eval scripts are not
        # consistent about it) return plain tensors, as before
        if torch.is_grad_enabled() and self.training:
            params, lat = self.trainable_mlp_parameters(), self.differentiable_latent()
            if params or lat is not None:
                if lat is None:
                    self.check_differentiable()
                return _QueryFunction.apply(self, xyz, bool(coarse), viewdirs, len(params), *[p for _, p in params],
                                            *([lat] if lat is not None else []))
        return self.guard_f16_range(lambda: self._query(xyz, coarse, viewdirs))

    def _query(self, xyz, coarse, viewdirs):
        self._sync()
        L = _lib.load()
        dev = self._device()
        SB, B, _ = xyz.shape
        assert SB == self.num_objs, "super-batch of xyz must match the encoded scenes"
        assert viewdirs is not None, "use_viewdirs is set: viewdirs are required"
        self._last_call_group = False
        xyz = xyz.detach().to(dev, torch.float32).contiguous()
        viewdirs = viewdirs.detach().to(dev, torch.float32).reshape(SB, B, 3).contiguous()
        out = torch.empty(SB, B, self.d_out, device=dev, dtype=torch.float32)
        use_coarse = bool(coarse) or self.mlp_fine is None
        st = stream_of(dev)
        for sb in range(SB):
            check(L.pny_query(self._scene(sb), ptr(xyz[sb]), ptr(viewdirs[sb]), B, int(use_coarse), ptr(out[sb]), st))
        return out

    # ---------------------------------------------------------------- checkpoints
    def load_weights(self, args, opt_init=False, strict=True, device=None):
        """Same contract as reference models.py:320-349.  The file loaded is
        <checkpoints_path>/<name>/pixel_nerf_init when ``opt_init or not args.resume`` and pixel_nerf_latest
        otherwise; ``opt_init and not args.resume`` is a no-op that returns None (the reference's bare ``return``);
        a missing file warns -- it does not fail -- unless opt_init.  The file is a plain state_dict and is read
        with weights_only=True."""
        if opt_init and not args.resume:
            return
        ckpt_name = "pixel_nerf_init" if opt_init or not args.resume else "pixel_nerf_latest"
        model_path = "%s/%s/%s" % (args.checkpoints_path, args.name, ckpt_name)
        if device is None:
            device = self.mlp_coarse.lin_in.weight.device   # the reference asks self.poses.device: same module device
        if osp.exists(model_path):
            print("Load", model_path)
            self.load_state_dict(torch.load(model_path, map_location=device, weights_only=True), strict=strict)
        elif not opt_init:
            warnings.warn(
                ("WARNING: {} does not exist, not loaded!! Model will be re-initialized.\n"
                 + "If you are trying to load a pretrained model, STOP since it's not in the right place. "
                 + "If training, unless you are startin a new experiment, please remember to pass --resume."
                 ).format(model_path))
        return self

    def save_weights(self, args, opt_init=False, epochNum=""):
        """Same contract as reference models.py:351-370: the current pixel_nerf_latest (pixel_nerf_init with
        opt_init) is first copied to pixel_nerf_backup<epochNum> (pixel_nerf_init_backup); the state_dict is written
        only when ``epochNum == ""`` -- the trainer's ``epochNum="_best"`` / ``str(epoch - 1)`` calls
        (train/trainlib/trainer.py:246,251) only snapshot the file already on disk."""
        from shutil import copyfile
        ckpt_name = "pixel_nerf_init" if opt_init else "pixel_nerf_latest"
        backup_name = "pixel_nerf_init_backup" if opt_init else "pixel_nerf_backup" + epochNum
        ckpt_path = osp.join(args.checkpoints_path, args.name, ckpt_name)
        ckpt_backup_path = osp.join(args.checkpoints_path, args.name, backup_name)
        if osp.exists(ckpt_path):
            copyfile(ckpt_path, ckpt_backup_path)
        if epochNum == "":
            torch.save(self.state_dict(), ckpt_path)
        return self


def check_latent_levels(maps, n_views, d_latent):
    """encode(latent=[m0, m1, ...]): the list's shapes, or ValueError -> ((C_i, h_i, w_i) per level)."""
    if len(maps) == 0:
        raise ValueError("encode(latent=[...]): empty list of feature maps")
    if len(maps) > _lib.MAX_LATENT_LEVELS:
        raise ValueError("encode(latent=[...]): %d feature maps, more than %d levels" % (len(maps), _lib.MAX_LATENT_LEVELS))
    for i, m in enumerate(maps):
        if not torch.is_tensor(m) or m.dim() != 4 or not m.is_floating_point():
            raise ValueError("encode(latent=[...]): map %d is not a 4-D float tensor (SB*NS, C, h, w)" % i)
    for i, m in enumerate(maps):
        if m.shape[0] != n_views:
            raise ValueError("encode(latent=[...]): leading sizes differ: map %d has %d, the images have SB*NS = %d"
                             % (i, m.shape[0], n_views))
        if min(m.shape[1:]) < 1:
            raise ValueError("encode(latent=[...]): map %d is empty" % i)
    total = sum(int(m.shape[1]) for m in maps)
    if total != d_latent:
        raise ValueError("encode(latent=[...]): the maps' channels sum to %d, d_latent is %d" % (total, d_latent))
    return tuple((int(m.shape[1]), int(m.shape[2]), int(m.shape[3])) for m in maps)


def _levels_arrays(levels):
    n = len(levels)
    return [(C.c_int * n)(*[lv[k] for lv in levels]) for k in range(3)]


def _camera_pairs(v, default=None):
    """focal / c in the formats of the reference (models.py:125-148) -> (N, 2) fp32 rows on the host: a scalar is both
    components of one row, (N,) is one value per row for both components, (N, 2) is taken as it is; None is the one row
    `default` (c: the image centre)."""
    if v is None:
        return torch.tensor([default], dtype=torch.float32)
    v = torch.as_tensor(v, dtype=torch.float32).cpu()
    if v.dim() == 0:
        v = v[None, None].repeat(1, 2)
    elif v.dim() == 1:
        v = v.unsqueeze(-1).repeat(1, 2)
    return v.contiguous()


class _LevelsFunction(torch.autograd.Function):
    """The feature maps of encode(latent=[...]) under autograd.  The output STANDS FOR the scene latent in the graphs of the
    render / query calls: it has the shape of the library's channel-last latent, (SB * NS, Hl, Wl, L), and no storage of that
    size (one element, expanded) -- the latent itself lives in the scene handles, where encode() assembles it
    (pny_scene_set_latent_levels).  Backward: the channel-last d loss / d latent buffer of the render backward
    (PixelNeRFNet.latent_grad) goes to pny_latent_levels_backward, one launch, which writes the gradient of every map
    that requires grad in the map's own NCHW shape.  No (n, L, Hl, Wl) tensor and no transpose on the way there or back."""

    @staticmethod
    def forward(ctx, net, levels, *maps):
        ctx.net, ctx.levels = net, levels
        ctx.metas = [(m.device, m.dtype) for m in maps]
        n, (_, hl, wl) = maps[0].shape[0], levels[0]
        return torch.empty(1, device=net._device(), dtype=torch.float32).expand(n, hl, wl, sum(lv[0] for lv in levels))

    @staticmethod
    def backward(ctx, g):
        net, levels = ctx.net, ctx.levels
        dev = net._device()
        g = g.detach().to(dev, torch.float32).contiguous()
        n = g.shape[0]
        outs = [torch.empty(n, *lv, device=dev, dtype=torch.float32) if need else None
                for lv, need in zip(levels, ctx.needs_input_grad[2:])]
        ptrs = (C.c_void_p * len(levels))(*[None if o is None else o.data_ptr() for o in outs])
        ch, hs, ws = _levels_arrays(levels)
        with torch.cuda.device(dev):
            check(_lib.load().pny_latent_levels_backward(ptr(g), ptrs, ch, hs, ws, len(levels), n, stream_of(dev)))
        return (None, None) + tuple(None if o is None else o.to(d, t) for o, (d, t) in zip(outs, ctx.metas))


class _TrunkFunction(torch.autograd.Function):
    """The ResNet-34 trunk in training mode on the library's kernels (pny_trunk_train_forward / _backward, reference
    src/model/encoder.py:139-173 under autograd): images (n, 3, H, W) -> latent (n, 512, H/2, W/2); backward fills the
    gradients of the trainable trunk parameters.  Batch statistics, running statistics stepped as nn.BatchNorm2d does."""

    @staticmethod
    def forward(ctx, net, images, *params):
        net._sync()
        L = _lib.load()
        dev = net._device()
        n, _, H, W = images.shape
        hl, wl = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        lat = torch.empty(n, 512, hl, wl, device=dev, dtype=torch.float32)
        bns = net._trunk_bn_modules()
        bn_eval = not bns[0].training
        check(L.pny_trunk_train_forward(net._h_model, ptr(images), n, H, W, float(bns[0].momentum), int(bn_eval), ptr(lat),
                                        stream_of(dev)))
        # The library keeps the saved activations of ONE training forward per model: a later forward replaces them, and the
        # backward of this graph must then refuse instead of differentiating against the other forward's activations
        net._trunk_generation = ctx.generation = net._trunk_generation + 1
        if not bn_eval:
            with torch.no_grad():
                for b in bns:
                    b.num_batches_tracked += 1
            net._enc_stale = True     # the inference trunk's folded batch norm is stale now (running statistics moved)
        ctx.net = net
        ctx.named_shapes = [(k, tuple(p.shape)) for (k, _), p in zip(net._trunk_trainable(), params)]
        return lat

    @staticmethod
    def backward(ctx, d_lat):
        net = ctx.net
        if net._trunk_generation != ctx.generation:
            raise RuntimeError("the library's training trunk holds the activations of a later encode() than this graph's: a "
                               "training encode() was superseded before its backward (call backward() before the next "
                               "training encode(), or PNYOLO_TRUNK=torch for gradient accumulation over several encodes)")
        L = _lib.load()
        dev = net._device()
        h = net._h_model
        ev, net._lat_grad_event = net._lat_grad_event, None
        ev = ev[0] if ev is not None and ev[1]() is d_lat and d_lat._version == ev[2] else None
        d_lat = d_lat.detach().to(dev, torch.float32).contiguous()
        # The trunk's backward needs d loss / d latent and nothing else of the renderer's backward: it runs on a stream of its
        # own that starts behind the point where the latent gradient was complete (render._RenderFunction.backward records it
        # in front of the MLPs' weight-gradient flush), beside that flush; the caller's stream takes it back at the end.
        # The event covers only the tensor that render backward returned: when autograd summed d_lat from several consumers
        # (two renders, another loss term on the latent, bind_parallel's per-device shares) or the event is a leftover of
        # another latent's render, d_lat is another tensor, written on the caller's stream after the event -- wait for that.
        main = torch.cuda.current_stream(dev)
        side = main if os.environ.get("PNYOLO_TRUNK_STREAM", "1") == "0" else net._own_streams("_trunk_stream", dev)
        # (which of the two orderings ran, for the tests: "event" overlaps the weight-gradient flush, "stream" waits for it)
        net._last_trunk_wait = "same stream" if side is main else ("event" if ev is not None else "stream")
        if side is not main:
            if ev is not None:
                side.wait_event(ev)
            else:
                side.wait_stream(main)
        with torch.cuda.stream(side):
            flat, grads = net._bind_flat_grads(ctx.named_shapes, dev)
            try:
                check(L.pny_trunk_train_backward(h, ptr(d_lat), stream_of(dev)))
            finally:
                for k, _ in ctx.named_shapes:
                    check(L.pny_model_bind_grad(h, k.encode(), None))
        if side is not main:
            d_lat.record_stream(side)
            flat.record_stream(main)
            main.wait_stream(side)
        return (None, None) + tuple(grads)


class _QueryFunction(torch.autograd.Function):
    """PixelNeRFNet.forward under autograd: pny_query forward, pny_query_backward into bound gradient buffers."""

    @staticmethod
    def forward(ctx, net, xyz, coarse, viewdirs, n_params, *params):
        lat = params[n_params] if len(params) > n_params else None
        ctx.lat_meta = None if lat is None else net.latent_meta(lat)
        out = net._query(xyz, coarse, viewdirs)
        dev = net._device()
        ctx.net, ctx.coarse = net, coarse
        ctx.xyz = xyz.detach().to(dev, torch.float32).contiguous()
        ctx.dirs = viewdirs.detach().to(dev, torch.float32).reshape(ctx.xyz.shape).contiguous()
        return out

    @staticmethod
    def backward(ctx, g_out):
        net = ctx.net
        L = _lib.load()
        dev = net._device()
        grads = net.bind_mlp_grads()
        g_out = g_out.detach().to(dev, torch.float32).contiguous()
        use_coarse = bool(ctx.coarse) or net.mlp_fine is None
        st = stream_of(dev)
        SB = ctx.xyz.shape[0]
        scenes = [net._scene(sb) for sb in range(SB)]
        with net.latent_grad(ctx.lat_meta, scenes) as lg:
            for sb in range(SB):
                check(L.pny_query_backward(scenes[sb], ptr(ctx.xyz[sb]), ptr(ctx.dirs[sb]), ctx.xyz.shape[1], int(use_coarse),
                                           ptr(g_out[sb]), _lib.ACC_ADD, st))
            extra = lg.result()
        net._lat_grad_event = None      # (unmarked: a trunk backward behind this one waits for the whole stream)
        return (None, None, None, None, None) + tuple(grads) + extra


def make_model(conf, *args, **kwargs):
    """reference src/model/__init__.py:4-11"""
    model_type = conf.get_string("type", "pixelnerf")
    if model_type == "pixelnerf":
        return PixelNeRFNet(conf, *args, **kwargs)
    raise NotImplementedError("Unsupported model type", model_type)
