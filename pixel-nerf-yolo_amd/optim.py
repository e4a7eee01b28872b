"""
``Adam``: drop-in for ``torch.optim.Adam`` (the reference's optimizer, train/trainlib/trainer.py:53) whose ``step()`` is one
library call per parameter group: ONE launch updates every tensor of the group (csrc/optim.hip), and with ``model=net`` the
same call rebuilds the model's packed operands behind the update (what ``pny_model_refresh`` does), so the step's tail needs
no ATen operator and no second trip through ``PixelNeRFNet._sync()``.

Same constructor arguments, state layout (``step`` / ``exp_avg`` / ``exp_avg_sq``) and ``state_dict()`` as torch's class: a
state file written by one loads into the other (the reference's ``_optim`` file included), ``ExponentialLR`` and the other
schedulers work (``lr`` is read from ``param_groups`` at every step).  There is no CPU path and no fallback: parameters and
gradients are fp32 tensors on an MI355X.
"""
import ctypes as C

import torch

from . import lib as _lib
from .lib import AdamHyper, check, stream_of

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "foreach", "fused", "decoupled_weight_decay")
_ALIGN = 64   # elements: every tensor's moments start on a 256-byte boundary of the flat allocation


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's arithmetic (no amsgrad, no maximize) on the library's kernel.

    :param model optional PixelNeRFNet whose parameters (or some of them) this optimizer steps: ``step()`` then rebuilds its
        packed operands in the same library call and brings the model's bookkeeping up to date (version counters,
        ``_synced_key``, the inference trunk's staleness), and a weight that the step moved out of the f16 range is reported
        (``net.range_status()``: PNY_RANGE_WEIGHT) by the step that moved it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, model=None):
        given = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable, foreach=foreach,
                     fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        for name in _UNSUPPORTED:
            if given[name]:
                raise NotImplementedError("pixel_nerf_yolo_amd.optim.Adam does not support %s=%r (one fused launch per "
                                          "parameter group is the only implementation)" % (name, given[name]))
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("pixel_nerf_yolo_amd.optim.Adam takes lr as a Python float (a tensor lr belongs to "
                                      "capturable=True)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: %r" % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: %r" % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        # the keys of torch.optim.Adam's param_groups, so that a state_dict of either class loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        self._slots = {}      # parameter -> (exp_avg, exp_avg_sq): views of the flat allocations
        self._flats = []      # the flat allocations (kept alive)
        self._native = {}     # device -> dict(handle, index {parameter: tensor index})
        self._sig = None      # the parameters' storage pointers the handles were built for
        self._mlp_ids = (None, ())   # (the model's structure signature, ids of its MLP parameters)
        self.model = model
        super().__init__(params, defaults)

    # ---------------------------------------------------------------- state
    def _ensure_slots(self):
        """Moments for every parameter that has none yet: views of ONE flat allocation per moment and device (one zero fill).
        A parameter that moved to another device since takes its moments along."""
        new = {}
        for group in self.param_groups:
            for p in group["params"]:
                slot = self._slots.get(p)
                if slot is None or slot[0].device != p.device:
                    new.setdefault(p.device, []).append(p)
        for dev, ps in new.items():
            offs, total = [], 0
            for p in ps:
                offs.append(total)
                total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
            flat_m = torch.zeros(max(total, 1), device=dev, dtype=torch.float32)
            flat_v = torch.zeros(max(total, 1), device=dev, dtype=torch.float32)
            self._flats.append((flat_m, flat_v))
            for p, o in zip(ps, offs):
                m, v = flat_m[o:o + p.numel()].view(p.shape), flat_v[o:o + p.numel()].view(p.shape)
                old = self._slots.get(p)
                if old is not None:
                    m.copy_(old[0])
                    v.copy_(old[1])
                self._slots[p] = (m, v)
                st = self.state.get(p)
                if st:
                    st["exp_avg"], st["exp_avg_sq"] = m, v
        if new:
            self._free_native()

    def load_state_dict(self, state_dict):
        """torch's loader, then the loaded moments are copied into the flat buffers (which the library keeps reading) and
        ``step`` becomes the CPU float tensor of non-capturable torch Adam."""
        super().load_state_dict(state_dict)
        loaded = {p: (st["exp_avg"], st["exp_avg_sq"]) for p, st in self.state.items() if st}
        self._ensure_slots()
        with torch.no_grad():
            for p, (m_in, v_in) in loaded.items():
                st = self.state[p]
                m, v = self._slots[p]
                m.copy_(m_in)
                v.copy_(v_in)
                st["exp_avg"], st["exp_avg_sq"] = m, v
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    # ---------------------------------------------------------------- native plumbing
    def _free_native(self):
        if self._native:
            L = _lib.load()
            for nat in self._native.values():
                L.pny_optim_destroy(nat["handle"])
        self._native = {}

    def __del__(self):
        try:
            self._free_native()
        except Exception:
            pass

    def _bind(self):
        """The library's handle per device: every parameter of every group with its moments, in group order (a group is a
        contiguous index range).  Rebuilt when a parameter's storage moved or a group was added."""
        sig = tuple(p.data_ptr() for g in self.param_groups for p in g["params"])
        if self._native and sig == self._sig:
            return
        self._free_native()
        L = _lib.load()
        for group in self.param_groups:
            for p in group["params"]:
                nat = self._native.get(p.device)
                if nat is None:
                    h = C.c_void_p()
                    check(L.pny_optim_create(C.byref(h), p.device.index or 0))
                    nat = self._native[p.device] = dict(handle=h, index={})
                m, v = self._slots[p]
                i = L.pny_optim_add_tensor(nat["handle"], C.c_void_p(p.data_ptr()), C.c_void_p(m.data_ptr()),
                                           C.c_void_p(v.data_ptr()), p.numel())
                if i < 0:
                    check(i)
                nat["index"][p] = i
        self._sig = sig

    @staticmethod
    def _check_tensor(t, what):
        if t.device.type != "cuda":
            raise _lib.PnyError("pixel_nerf_yolo_amd.optim.Adam.step(): %s is on %s; the optimizer runs on an MI355X only "
                                "(there is no CPU path)" % (what, t.device))
        if t.is_sparse or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.PnyError("pixel_nerf_yolo_amd.optim.Adam.step(): %s must be a dense, contiguous fp32 tensor (got %s, "
                                "%s)" % (what, t.dtype, "contiguous" if t.is_sparse or t.is_contiguous() else "strided"))

    def _model_in_step(self, net):
        """The model's parameter key if its native copy can follow this step on the device (it exists on the model's device and
        differs from the parameters by in-place updates at most: PixelNeRFNet._follows_in_place, _sync's own condition for a
        refresh), else None: the step then only updates, and the model's next _sync() does what it always did."""
        if net._h_model is None or net._h_device != str(net._device()):
            return None
        key = net._weights_key()
        return key if net._follows_in_place(net._synced_key, key) else None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.load()
        # what steps: per group the parameters that have a gradient (torch skips the others; their `step` does not advance)
        work = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            for p in ps:
                self._check_tensor(p, "a parameter")
                self._check_tensor(p.grad, "a gradient")
                if p.grad.device != p.device:
                    raise _lib.PnyError("pixel_nerf_yolo_amd.optim.Adam.step(): a gradient lives on another device than its parameter")
            if ps:
                work.append((group, ps))
        if not work:
            return loss
        self._ensure_slots()
        self._bind()
        calls = []
        for group, ps in work:
            by = {}     # (device, steps taken) -> parameters: one launch each (one per group unless parameters joined late)
            for p in ps:
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"], st["exp_avg_sq"] = self._slots[p]
                by.setdefault((p.device, float(st["step"])), []).append(p)
            beta1, beta2 = group["betas"]
            for (dev, t), sel in by.items():
                nat = self._native[dev]
                idx = [nat["index"][p] for p in sel]
                first, n = min(idx), max(idx) - min(idx) + 1
                grads = (C.c_void_p * n)()
                for p, i in zip(sel, idx):
                    grads[i - first] = p.grad.data_ptr()
                hyper = AdamHyper(lr=float(group["lr"]), beta1=float(beta1), beta2=float(beta2), eps=float(group["eps"]),
                                  weight_decay=float(group["weight_decay"]), step=int(t) + 1)
                calls.append((dev, nat["handle"], hyper, grads, first, n, sel))
        net = self.model
        old = key = None
        if net is not None:
            key = self._model_in_step(net)
            old = net._synced_key
        refresh_on = None
        if key is not None:
            if self._mlp_ids[0] != net._tracked_sig:
                self._mlp_ids = (net._tracked_sig, {id(v) for k, v in net._tracked if k.startswith("mlp_")})
            mlp = self._mlp_ids[1]
            stepped = any(id(p) in mlp for c in calls for p in c[6])
            if stepped or any(a[2] != b[2] and a[0].startswith("mlp_") for a, b in zip(old, key)):
                dev = net._device()
                on = [i for i, c in enumerate(calls) if c[0] == dev]
                refresh_on = on[-1] if on else None
        for i, (dev, handle, hyper, grads, first, n, sel) in enumerate(calls):
            h_model = net._h_model if i == refresh_on else None
            check(L.pny_optim_adam_step(handle, C.byref(hyper), grads, first, n, h_model, stream_of(dev)))
            for p in sel:
                self.state[p]["step"] += 1
            # the parameters changed behind PyTorch's back: their version counters say so (autograd's in-place checks,
            # PixelNeRFNet._weights_key, bind_parallel's replicas)
            torch.autograd.graph.increment_version(sel)
        if key is not None:
            if refresh_on is None and any(a[2] != b[2] and a[0].startswith("mlp_") for a, b in zip(old, key)):
                return loss   # (MLP weights moved and no launch of this step ran on the model's device: _sync() refreshes)
            new = net._weights_key()
            net._mark_trunk_stale(old, new)     # as _sync(): the inference trunk's folded copy is re-uploaded when next needed
            net._synced_key = new
        return loss
