"""
Host-side mirror of the reference's renderer layer (src/render/): ``NeRFRenderer``,
``_RenderWrapper`` / ``bind_parallel``, ``YoloRenderer``, ``make_renderer`` with the reference's
signatures and return conventions, executing on libpnyolo.so.

A render call is ONE C-ABI call per scene (pny_render / pny_yolo_render): sampling, point
generation, the fused MLP, compositing, importance sampling and the sort all stay on the device.
A training super-batch that one grouped scene holds (model.encode, pny_scene_set_groups) is ONE
call for all its objects.  Both are the same code: G launches of R rays each (``_launches``), on
row g of every tensor's (G, R, ...) view, forward (``NeRFRenderer._render``) and backward
(``_RenderFunction.backward``) alike.
The reference's ``eval_batch_size`` point-chunking exists only to bound its (rows x 554)
intermediates; fusion removes them, so the attribute is kept for interface compatibility and
ignored.

Random draws: the reference jitters unconditionally (nerf.py:117) and draws three more tensors
in the fine pass -- they are inputs of the path.  By default a per-call Philox seed is used
(in-kernel generation); ``renderer.draws = dict(u_coarse=, u_fine=, u_fine2=, g_depth=)`` replays
explicit tensors instead (parity mode, consumed by the next call; ``noise_coarse=, noise_fine=``
replay the training sigma noise).  The library takes them for every stage or for none.
"""
import ctypes as C
import os
import weakref

import torch

from . import lib as _lib
from .lib import RenderOpts, RenderOut, check, ptr, stream_of


class _RenderWrapper(torch.nn.Module):
    """reference src/render/nerf.py:21-48"""

    def __init__(self, net, renderer, simple_output):
        super().__init__()
        self.net = net
        self.renderer = renderer
        self.simple_output = simple_output

    def forward(self, rays, want_weights=False):
        if rays.shape[0] == 0:
            return (torch.zeros(0, 3, device=rays.device), torch.zeros(0, device=rays.device))
        outputs = self.renderer(self.net, rays, want_weights=want_weights and not self.simple_output)
        if self.simple_output:
            part = outputs["fine"] if self.renderer.using_fine else outputs["coarse"]
            return part["rgb"], part["depth"]
        return outputs  # plain nested dict, as DotMap.toDict() in the reference


class _MultiDeviceRenderWrapper(torch.nn.Module):
    """``bind_parallel(net, gpus)`` with more than one device in ONE process: the drop-in for the reference's
    ``torch.nn.DataParallel(_RenderWrapper(...), gpus, dim=1)`` (src/render/nerf.py:360-377; called by train/train.py:78 and
    eval/eval.py:150 with ``--gpu_id "0 1 ..."``) without its per-call replication.  The reference re-broadcasts every
    parameter and the latent to every device on EVERY call; here each listed device holds a PERSISTENT
    replica of the native model and of the encoded scenes:
      * weights go up once and are re-sent only when the master's parameters changed (version counters),
      * latent and cameras are re-sent only after the master's ``encode()`` (the encoder runs once, on the master),
      * a call splits the rays on dim 1 into one contiguous range per device, enqueues every range on its device's stream
        without waiting, and gathers the tiles on ``gpus[0]`` with peer copies.
    Results: a ray renders to the same bits whatever range it is in (slice invariance), so with explicit draws
    the assembled output equals the single-device call bit for bit; with Philox draws each range has its own seed.
    Every split call goes through ``_split`` (ranges from ``_ray_ranges``, per-range seed, draws and replica, the renderer's
    state restored afterwards); on its device a range is an ordinary renderer call: one library call per scene, or one on the
    replica's grouped scene in training.
    Training calls (grad mode) split the same way (_train_split): every device runs the training forward and backward of its ray
    range on its replica, the replica's parameters enter the graph as device copies of the master's (``_leaves``, ``p.to(device)``: autograd
    carries each device's gradients back and sums them into the master's ``.grad``, as DataParallel's replicate / gather do), and
    the replicas pick the stepped weights up at the next call.  A latent that takes a gradient (trainable encoder: the trunk runs
    once, on the master) is a leaf of every device's graph in the same way: each device returns its share of d loss / d latent.
    dist.py (one process per GPU, one gradient all-reduce) stays the recommended multi-GPU path: no Python serialisation of
    the per-device launches."""

    def __init__(self, net, renderer, gpus, simple_output):
        super().__init__()
        self.net, self.renderer, self.simple_output = net, renderer, simple_output
        self.gpus = [int(g) for g in gpus]
        self._replicas = [None] * len(self.gpus)   # [0] is `net` itself when it lives on gpus[0]
        self._seen = [None] * len(self.gpus)       # (weights key, encode epoch) each replica was last synchronised to
        self._warned = False

    def _replica(self, i):
        from .model import PixelNeRFNet
        net = self.net
        dev = torch.device("cuda", self.gpus[i])
        if i == 0 and net._device() == dev:
            return net
        r = self._replicas[i]
        if r is None:
            r = PixelNeRFNet(net._conf, stop_encoder_grad=True)
            if net.mlp_fine is None:
                r.mlp_fine = None
            r.load_state_dict(net.state_dict(), strict=False)
            r = r.to(dev).eval()
            for (_, pr), (_, pm) in zip(r.named_parameters(), net.named_parameters()):
                pr.requires_grad_(pm.requires_grad)
            r._projection, r._precision = net._projection, net._precision
            self._replicas[i] = r
        r._deterministic = net._deterministic   # (every call: a setting changed after the replica was made holds too)
        key = (net._weights_key(), net._encode_epoch)
        if self._seen[i] != key:
            if self._seen[i] is not None and self._seen[i][0] != key[0]:
                # in place, and only the tensors the master changed: the replica's refresh path (one repack launch).  Copying an
                # untouched buffer too (code._freqs) would bump its version, and the replica's _sync() answers a change outside
                # the MLPs and the trunk with a full re-upload, which waits for the device on every training step
                was = self._seen[i][0]
                same = {a[0] for a, b in zip(was, key[0]) if a == b} if len(was) == len(key[0]) else set()
                with torch.no_grad():
                    for (k, dst), (_, src) in zip(r.state_dict().items(), net.state_dict().items()):
                        if k not in same:
                            dst.copy_(src)
                if (net.mlp_fine is None) != (r.mlp_fine is None):
                    r.mlp_fine = None
            le = net._last_encode
            if le is None:
                raise RuntimeError("bind_parallel(net, gpus): call net.encode(...) before rendering")
            r.train(net.training)          # (a training master: the replica's encode() fills its grouped scene too)
            with torch.cuda.device(dev):
                lat = torch.cat([net.latent(sb) for sb in range(le["SB"])]).to(dev)
                images = torch.zeros(le["SB"], le["NS"], 3, le["H"], le["W"])
                r.encode(images, le["poses"], le["focal"], c=le["c"], latent=lat)
            self._seen[i] = key
        r._latent_channel_last = net._latent_channel_last   # (the layout of the master's latent leaf: latent_meta)
        return r

    def forward(self, rays, want_weights=False):
        if rays.shape[0] == 0:
            return (torch.zeros(0, 3, device=rays.device), torch.zeros(0, device=rays.device))
        net, ren = self.net, self.renderer
        if net.occupancy is not None:
            raise _lib.PnyError("bind_parallel(net, gpus): the net has an occupancy grid attached (net.set_occupancy), which the "
                                "per-device replicas do not carry; render on one device, or detach it with net.set_occupancy(None)")
        if net.termination is not None:
            raise _lib.PnyError("bind_parallel(net, gpus): the net has early ray termination on (net.set_termination), which the "
                                "per-device replicas do not carry; render on one device, or switch it off with net.set_termination(None)")
        want_weights = want_weights and not self.simple_output
        training = torch.is_grad_enabled() and net.training and (net.trainable_mlp_parameters() or net.differentiable_latent() is not None)
        B = rays.shape[1]
        n_dev = len(self.gpus)
        if training and B >= 64 * n_dev:
            outputs = self._train_split(rays, want_weights)
        elif training or B < 64 * n_dev:
            outputs = ren(net, rays, want_weights=want_weights)
        else:
            outputs = self._render_split(rays, want_weights)
        if self.simple_output:
            part = outputs["fine"] if "fine" in outputs else outputs["coarse"]
            return part["rgb"], part["depth"]
        return outputs

    def _split(self, SB, B, body, train=False, prefetch=False, guard=None):
        """One call over (SB, B) rays split on B across the devices.  For every non-empty range of _ray_ranges, in order:
        fetch the replica, make its device current, give the renderer the range's own seed (``_calls + i``), its rows of the
        explicit draws and (YOLO) the replica as its net, and run ``body(replica, device, lo, hi)``.  Once every device has
        its work, ``guard(i, replica, again)`` looks at each range; ``again()`` repeats it, and a result it returns replaces
        the range's.  The renderer's state is restored whatever happens.  Returns the results in range order."""
        net, ren, n_dev = self.net, self.renderer, len(self.gpus)
        yolo = isinstance(ren, YoloRenderer)
        draws, calls, ren.draws = ren.draws, ren._calls, None
        ranges = [(i, lo, hi) for i, (lo, hi) in enumerate(_ray_ranges(B, n_dev)) if hi > lo]

        def visit(i, lo, hi, r):
            dev = torch.device("cuda", self.gpus[i])
            with torch.cuda.device(dev):
                ren._calls = calls + i
                if yolo:
                    ren.net = r
                if draws is not None:
                    ren.draws = {k: torch.as_tensor(v).reshape(SB, B, -1)[:, lo:hi].reshape(SB * (hi - lo), -1) for k, v in draws.items()}
                return body(r, dev, lo, hi)

        try:
            reps = {i: self._replica(i) for i, _, _ in ranges} if prefetch else {}
            outs = []
            for i, lo, hi in ranges:
                if i not in reps:
                    reps[i] = self._replica(i)
                if train:
                    reps[i].train()
                outs.append(visit(i, lo, hi, reps[i]))
            for j, (i, lo, hi) in enumerate(ranges if guard is not None else ()):
                again = guard(i, reps[i], lambda: visit(i, lo, hi, reps[i]))
                if again is not None:
                    outs[j] = again
        finally:
            ren._calls, ren.draws = calls + n_dev, None
            if yolo:
                ren.net = net
        return outs

    def _leaves(self):
        """The leaves of the per-device training graphs: -> (number of MLP parameters, leaves(device)).  ``leaves(device)``
        are the master's trainable MLP parameters, then its latent if that takes a gradient (trainable encoder: each device
        returns its share), as differentiable copies on that device."""
        net = self.net
        src = [p for _, p in net.trainable_mlp_parameters()]
        n_params = len(src)
        lat_src = net.differentiable_latent()
        if lat_src is None:
            net.check_differentiable()
        else:
            src.append(lat_src)
        return n_params, lambda dev: [p if p.device == dev else p.to(dev) for p in src]

    def _train_split(self, rays, want_weights):
        """Training call over several devices (see the class docstring): _RenderFunction per device on its replica, with
        differentiable device copies of the master's parameters as the graph's leaves."""
        ren = self.renderer
        n_params, leaves = self._leaves()
        kf = int(ren.n_fine) if (ren.using_fine and ren.n_fine > 0) else 0
        dev0 = torch.device("cuda", self.gpus[0])

        def body(r, dev, lo, hi):
            outs = _RenderFunction.apply(ren, r, rays[:, lo:hi].to(dev), kf > 0, n_params, *leaves(dev))
            return [o.to(dev0) for o in outs]
        parts = self._split(rays.shape[0], rays.shape[1], body, train=True)
        cat = [torch.cat([p[j] for p in parts], dim=1) if parts[0][j].numel() else parts[0][j] for j in range(6)]
        return _result(cat, kf > 0, want_weights)

    def _render_split(self, rays, want_weights):
        ren = self.renderer
        master_policy = self.net.f16_range_policy

        def guard(i, r, again):   # f16-range guard (model.guard_f16_range): wait per device, repeat a range on fp32
            if master_policy == "lazy" or not any(r.last_launch_f16x2(s) for s in range(len(r._h_scenes))):
                return None
            torch.cuda.current_stream(torch.device("cuda", self.gpus[i])).synchronize()
            bits = r.range_status(clear=False)
            if not bits:
                return None
            r.range_status(clear=True)
            if master_policy == "raise":
                raise _lib.PnyRangeError(r._range_message(bits))
            import warnings
            warnings.warn("libpnyolo: " + r._range_message(bits) + " -- repeating the rays of cuda:%d on the fp32 kernels" % self.gpus[i])
            r.set_matrix_precision("f32")
            return again()
        outs = self._split(rays.shape[0], rays.shape[1], prefetch=True, guard=guard,   # (every replica first, then the launches)
                           body=lambda r, dev, lo, hi: ren._render(r, rays[:, lo:hi].to(dev), want_weights, save=False)[0])
        dev0 = torch.device("cuda", self.gpus[0])
        return {p: {k: torch.cat([o[p][k].to(dev0) for o in outs], dim=1) for k in outs[0][p]} for p in outs[0]}


class _MultiDeviceYoloWrapper(_MultiDeviceRenderWrapper):
    """``YoloRenderer.bind_parallel(net, gpus)`` with several devices (reference src/render/yolo.py:116-121 wraps the renderer in
    DataParallel(dim=1)): the same persistent replicas, the rays (flattened to (N, 8) as YoloRenderer.forward does) split into
    one contiguous range per device, the (n, anchors, 7) results concatenated on gpus[0]."""

    def __init__(self, net, renderer, gpus):
        super().__init__(net, renderer, gpus, simple_output=False)

    def forward(self, rays):
        net, ren = self.net, self.renderer
        training = torch.is_grad_enabled() and net.training and (net.trainable_mlp_parameters() or net.differentiable_latent() is not None)
        flat = rays.reshape(-1, 8)
        N = flat.shape[0]
        if N < 64 * len(self.gpus):
            ren.net = net
            return ren(rays)
        dev0 = torch.device("cuda", self.gpus[0])
        if training:   # as _train_split: per-device graphs whose leaves are device copies of the master's
            n_params, leaves = self._leaves()
            return torch.cat(self._split(1, N, train=True, body=lambda r, dev, lo, hi: _YoloRenderFunction.apply(
                ren, flat[lo:hi].to(dev), n_params, *leaves(dev)).to(dev0)), dim=0)

        def guard(i, r, again):
            if net.f16_range_policy == "lazy" or not r.last_launch_f16x2():
                return
            torch.cuda.current_stream(torch.device("cuda", self.gpus[i])).synchronize()
            bits = r.range_status(clear=True)
            if bits:
                raise _lib.PnyRangeError(r._range_message(bits))
        outs = self._split(1, N, guard=guard, body=lambda r, dev, lo, hi: ren._render(flat[lo:hi].to(dev))[0])
        return torch.cat([o.to(dev0) for o in outs], dim=0)


def _ray_ranges(n, n_dev):
    """(lo, hi) of the contiguous range of n rays that each of n_dev devices takes: whole 64-ray groups per device, so the
    trailing ranges may be empty."""
    per = -(-(-(-n // n_dev)) // 64) * 64
    return [(min(n, i * per), min(n, (i + 1) * per)) for i in range(n_dev)]


def _result(outs, has_fine, want_weights):
    """The renderer's nested result from (rgb, depth, weights) of the coarse and of the fine pass."""
    keys = ("rgb", "depth", "weights") if want_weights else ("rgb", "depth")
    res = {"coarse": dict(zip(keys, outs[:3]))}
    if has_fine:
        res["fine"] = dict(zip(keys, outs[3:6]))
    return res


def _mark_latent_grad(model, extra, dev):
    """Record where on the current stream the latent gradient `extra` (this backward's d loss / d latent, if any) is complete,
    together with a weak reference to that very tensor and its version: model._TrunkFunction.backward starts behind the event
    only when the gradient it receives IS that tensor, unmodified (autograd adds another consumer's gradient into it in place
    when it can), and otherwise waits for the whole stream.  A backward without a latent gradient
    clears the mark."""
    model._lat_grad_event = None
    if extra:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        model._lat_grad_event = (ev, weakref.ref(extra[0]), extra[0]._version)


class _RenderFunction(torch.autograd.Function):
    """NeRFRenderer.forward under autograd: forward = the ordinary pny_render (with its z / per-sample outputs kept),
    backward = pny_render_backward per launch of the forward, which accumulates into gradient buffers bound to the MLP parameters."""

    @staticmethod
    def forward(ctx, renderer, model, rays, has_fine, n_params, *params):
        # params = the trainable MLP parameters, optionally followed by the differentiable latent of encode(latent=...)
        lat = params[n_params] if len(params) > n_params else None
        ctx.lat_meta = None if lat is None else model.latent_meta(lat)
        # Reserve the model-level stash for every scene's tiles (pny_model_defer_weight_grads): the forward then writes the
        # GEMM operands the backward needs while it evaluates the MLPs (no recompute), the scenes' backward calls run on
        # side streams and ONE weight-gradient GEMM per MLP follows.  If the reservation exceeds the stash budget: plain
        # forward, scene-after-scene backward with recompute in chunks.
        model._sync()
        L = _lib.load()
        SB, B = rays.shape[0], rays.shape[1]
        kc = int(renderer.n_coarse)
        kt = kc + int(renderer.n_fine) if has_fine else 0
        tiles = lambda pts: -(-pts // 64)
        fine_mlp = model.mlp_fine is not None
        ct = tiles(B * kc) + (tiles(B * kt) if (has_fine and not fine_mlp) else 0)
        ft = tiles(B * kt) if (has_fine and fine_mlp) else 0
        ctx.deferred = L.pny_model_defer_weight_grads(model._h_model, 1, model.num_views_per_obj, SB * ct, SB * ft) == 0
        model._defer_token = ctx.token = model._defer_token + 1
        res, saved = renderer._render(model, rays, want_weights=True, save=True, stash=ctx.deferred)
        saved["depth_coarse"] = res["coarse"]["depth"]
        ctx.renderer, ctx.model, ctx.saved, ctx.has_fine = renderer, model, saved, has_fine
        ctx.white_bkgd = bool(renderer.white_bkgd)
        ctx.set_materialize_grads(False)
        outs = [res["coarse"]["rgb"], res["coarse"]["depth"], res["coarse"]["weights"]]
        if has_fine:
            outs += [res["fine"]["rgb"], res["fine"]["depth"], res["fine"]["weights"]]
        else:
            outs += [rays.new_zeros(0), rays.new_zeros(0), rays.new_zeros(0)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_rgb_c, g_depth_c, g_w_c, g_rgb_f, g_depth_f, g_w_f):
        model, sv, ren = ctx.model, ctx.saved, ctx.renderer
        L = _lib.load()
        dev = model._device()
        grads = model.bind_mlp_grads()            # zeroed fp32 buffers, one per trainable MLP parameter, bound by name
        SB, B = sv["rays"].shape[0], sv["rays"].shape[1]

        def prep(t):
            if t is None or t.numel() == 0:
                return None
            return t.detach().to(dev, torch.float32).contiguous()

        ups = [prep(x) for x in (g_rgb_c, g_depth_c, g_w_c, g_rgb_f, g_depth_f, g_w_f)]
        # The reservation made by the forward is still ours unless another training forward ran in between: then this
        # call computes its weight gradients immediately (ACC_IMMEDIATE), scene after scene, with recompute.
        deferred = ctx.deferred and model._defer_token == ctx.token
        acc = _lib.ACC_ADD if deferred else _lib.ACC_ADD | _lib.ACC_IMMEDIATE
        group = bool(sv.get("group"))
        if group and not deferred:
            raise RuntimeError("the grouped training forward lost its stash reservation (another training forward ran before "
                               "this backward): call backward() before the next forward, or set PNYOLO_GROUP=0")
        handles, G, R = _launches(model, group, SB, B)    # the forward's launches (NeRFRenderer._render)
        rows = lambda t: None if t is None else t.view(G, R, *t.shape[2:])
        names = [k for k in _SAVED_BUFFERS if k in sv]
        if not ren._detach_fine_depth:
            names.append("depth_coarse")
        rays, sv_rows, up_rows = rows(sv["rays"]), {k: rows(sv[k]) for k in names}, [rows(p) for p in ups]

        def structs(g):
            return (_lib.RenderSaved(**{k: t[g].data_ptr() for k, t in sv_rows.items()}),
                    _lib.RenderGrads(*[None if t is None else t[g].data_ptr() for t in up_rows]))
        calls = [structs(g) for g in range(G)]
        # d loss / d latent, accumulated by every scene's call into its own slice (channel-last).  Its zero fill runs on the
        # current stream, so it is enqueued BEFORE the side streams fork from that stream: scenes 1.. add into the buffer
        # with atomics from their own streams, and nothing else would order those behind the fill.
        with model.latent_grad(ctx.lat_meta, handles) as lg:
            streams = model.fork_streams(G) if deferred else [None] * G

            def run(g, bits):
                with torch.cuda.stream(streams[g]):
                    check(L.pny_render_backward(handles[g], ptr(rays[g]), R, C.byref(sv["opts"][g]), C.byref(calls[g][0]),
                                                C.byref(calls[g][1]), acc | bits, stream_of(dev)))
            # Optional (PNYOLO_SPLIT_FLUSH=1, per-object scenes): every scene's FINE pass first, then mlp_fine's weight-gradient flush
            # on a stream of its own BESIDE the coarse passes instead of behind them.  Measured: no gain -- 12.5-13.5 ms per step
            # against 12.3-12.5: the chain kernels hold 152 KiB of a CU's LDS and the weight-gradient GEMM 128 KiB, so the two never
            # share a CU and the "quarter-busy" coarse chains cannot be filled in.  Off by default; kept because it is tested (bits
            # 4 / 8 of accumulate).
            split = (deferred and not group and ctx.has_fine and model.mlp_fine is not None
                     and os.environ.get("PNYOLO_SPLIT_FLUSH", "0") == "1")
            fstream = None
            if split:
                for g in range(G):
                    run(g, _lib.ACC_FINE_ONLY)      # (the fine pass only; the coarse passes follow -- include/pnyolo.h pny_render_backward)
                fstream = model._own_streams("_flush_stream", dev)
                fstream.wait_stream(torch.cuda.current_stream(dev))
                for st_ in streams:
                    if st_ is not None:
                        fstream.wait_stream(st_)
                with torch.cuda.stream(fstream):
                    check(L.pny_model_flush_weight_grads(model._h_model, _lib.ACC_ADD | _lib.FLUSH_FINE_ONLY, stream_of(dev)))
            for g in range(G):
                run(g, _lib.ACC_COARSE_ONLY if split else 0)
            if deferred:
                model.join_streams(streams)
            # d loss / d latent is complete here, BEFORE the weight-gradient flush is enqueued: the encoder's backward (the
            # trunk's kernels, model._TrunkFunction) starts behind this point on its own stream and runs beside the flush
            extra = lg.result()
        _mark_latent_grad(model, extra, dev)
        if deferred:
            check(L.pny_model_flush_weight_grads(model._h_model, _lib.ACC_ADD | (_lib.FLUSH_COARSE_ONLY if split else 0), stream_of(dev)))
            if fstream is not None:
                torch.cuda.current_stream(dev).wait_stream(fstream)
            check(L.pny_model_defer_weight_grads(model._h_model, 0, 0, 0, 0))
        return (None, None, None, None, None) + tuple(grads) + extra


_SAVED_BUFFERS = ("z_coarse", "sample_coarse", "z_fine", "sample_fine")   # per-sample outputs of the forward that the backward reads


def _launches(model, group, SB, B):
    """The library launches of one render call or of its backward: -> (scene handles, G, R) for G launches of R rays each.
    Grouped, it is one launch over the SB * B rays on the handle that holds the whole super-batch; otherwise one launch of B
    rays per object's scene.  Every tensor of the call -- rays, draws, results, saved buffers, upstream gradients -- is
    (SB, B, ...) in memory, so launch g takes row g of its (G, R, ...) view either way."""
    if group:
        return [model._h_group], 1, SB * B
    return [model._scene(sb) for sb in range(SB)], SB, B


class NeRFRenderer(torch.nn.Module):
    """Drop-in for reference src/render/nerf.py:51 (ctor :68-102, forward :257-309,
    sched_step :324-344, from_conf :346-358, bind_parallel :360-377)."""

    def __init__(self, n_coarse=128, n_fine=0, n_fine_depth=0, noise_std=0.0, depth_std=0.01,
                 eval_batch_size=100000, white_bkgd=False, lindisp=False, sched=None):
        super().__init__()
        self.n_coarse, self.n_fine, self.n_fine_depth = n_coarse, n_fine, n_fine_depth
        self.noise_std, self.depth_std = noise_std, depth_std
        self.eval_batch_size = eval_batch_size  # unused: no materialised per-point intermediates
        self.white_bkgd = white_bkgd
        self.lindisp = lindisp
        if lindisp:
            print("Using linear displacement rays")
        self.using_fine = n_fine > 0
        self.sched = sched
        if sched is not None and len(sched) == 0:
            self.sched = None
        self.register_buffer("iter_idx", torch.tensor(0, dtype=torch.long), persistent=True)
        self.register_buffer("last_sched", torch.tensor(0, dtype=torch.long), persistent=True)
        self.draws = None          # explicit random draws for the next call (parity mode)
        self.base_seed = 1234
        self._calls = 0
        self._debug_out = None             # test aid: {RenderOut field: tensor} that the next calls also write (one launch per scene)
        self._detach_fine_depth = False    # test aid: the backward treats the depth samples as constants

    def forward(self, model, rays, want_weights=False):
        """
        :param rays [origins (3), directions (3), near (1), far (1)] (SB, B, 8)
        :return dict(coarse=dict(rgb (SB,B,3), depth (SB,B)[, weights (SB,B,Kc)]), fine=dict(...))
        ``fine`` is absent when n_fine == 0 (callers test ``len(fine) > 0``, PixelNerfTrainer.py:140-143).

        Under autograd (grad mode on, ``model.train()`` and MLP parameters that require grad) the call goes through ``_RenderFunction``:
        same forward kernels, and ``loss.backward()`` fills ``.grad`` of the MLP parameters through
        pny_render_backward (include/pnyolo.h).  With an unfrozen encoder (the reference's default, train/train.py:66-73) the
        backward also returns d loss / d latent to the latent of the last ``encode()`` -- the library's training trunk
        (model._TrunkFunction) or a latent supplied by the caller."""
        if self.sched is not None and self.last_sched.item() > 0:
            self.n_coarse = self.sched[1][self.last_sched.item() - 1]
            self.n_fine = self.sched[2][self.last_sched.item() - 1]
        assert len(rays.shape) == 3
        grad_mode = torch.is_grad_enabled() and model.training
        params = model.trainable_mlp_parameters() if grad_mode else []
        lat_src = model.differentiable_latent()
        if not params and lat_src is None:
            draws, calls = self.draws, self._calls

            def call():   # repeatable: the same draws / seeds when the f16-range guard asks for the call again
                self.draws, self._calls = draws, calls
                return self._render(model, rays, want_weights, save=False)[0]
            return model.guard_f16_range(call)
        if model.occupancy is not None:
            raise _lib.PnyError("NeRFRenderer: the net has an occupancy grid attached (net.set_occupancy), which serves no-grad "
                                "renders only; this call takes gradients: detach the grid with net.set_occupancy(None), or render "
                                "under torch.no_grad()")
        if model.termination is not None:
            raise _lib.PnyError("NeRFRenderer: the net has early ray termination on (net.set_termination), which serves no-grad "
                                "renders only; this call takes gradients: switch it off with net.set_termination(None), or render "
                                "under torch.no_grad()")
        if lat_src is None:
            model.check_differentiable()     # (with a differentiable latent the caller's own encoder takes the gradient)
        kf = int(self.n_fine) if (self.using_fine and self.n_fine > 0) else 0
        outs = _RenderFunction.apply(self, model, rays, kf > 0, len(params), *[p for _, p in params],
                                     *([lat_src] if lat_src is not None else []))
        return _result(outs, kf > 0, want_weights)

    def _render(self, model, rays, want_weights, save, stash=False):
        """The pny_render launches of one call (_launches): one per scene, or one on the grouped scene.  save=True also returns
        what the backward needs: the detached device rays, the sample depths and the per-sample MLP outputs of both passes, and
        the options of every launch."""
        model._sync()
        L = _lib.load()
        dev = model._device()
        SB, B = rays.shape[0], rays.shape[1]
        assert SB == model.num_objs, "super-batch of rays must match the encoded scenes"
        rays = rays.detach().to(dev, torch.float32).contiguous()
        if rays.data_ptr() % 16:
            rays = rays.clone()  # the kernel reads a ray row as two 16-byte words
        kc, kf, kfd = int(self.n_coarse), int(self.n_fine), int(self.n_fine_depth)
        use_fine = self.using_fine and kf > 0
        if not use_fine:
            kf = kfd = 0
        f32 = dict(device=dev, dtype=torch.float32)
        res = {"coarse": {"rgb": torch.empty(SB, B, 3, **f32), "depth": torch.empty(SB, B, **f32)}}
        if want_weights:
            res["coarse"]["weights"] = torch.empty(SB, B, kc, **f32)
        if use_fine:
            res["fine"] = {"rgb": torch.empty(SB, B, 3, **f32), "depth": torch.empty(SB, B, **f32)}
            if want_weights:
                res["fine"]["weights"] = torch.empty(SB, B, kc + kf, **f32)
        saved = None
        extra = dict(self._debug_out or {})
        if save:
            saved = {"rays": rays, "z_coarse": torch.empty(SB, B, kc, **f32), "sample_coarse": torch.empty(SB, B, kc, 4, **f32),
                     "opts": []}
            if use_fine:
                saved["z_fine"] = torch.empty(SB, B, kc + kf, **f32)
                saved["sample_fine"] = torch.empty(SB, B, kc + kf, 4, **f32)
            for k in _SAVED_BUFFERS:
                if k in saved:
                    saved[k] = extra.pop(k, saved[k])   # a debug capture of the same buffer: share it
        draws, self.draws = self.draws, None
        self._calls += 1
        keep = []       # the uploaded draws: read again by the backward (depth samples)
        # Training on a super-batch held by ONE grouped scene (model.encode, pny_scene_set_groups): a single pny_render over
        # the SB * B rays -- one MLP launch per pass over every object's tiles instead of SB launches on side streams.  Needs
        # whole 64-sample tiles per object in both passes; otherwise one launch per object (model._scene fills its handles).
        model._last_call_group = False
        group = (stash and model._group_scene() is not None and SB == model._group["SB"] and (B * kc) % 64 == 0
                 and (not use_fine or (B * (kc + kf)) % 64 == 0) and not extra)
        handles, G, R = _launches(model, group, SB, B)
        streams = model.fork_streams(G)       # scenes are independent: one side stream each (None = current stream)
        rows = lambda t: t.view(G, R, *t.shape[2:])
        bufs = {k + "_" + p: t for p in res for k, t in res[p].items()}     # RenderOut's fields: results, debug captures, saved
        bufs.update(extra)
        if save:
            bufs.update({k: saved[k] for k in _SAVED_BUFFERS if k in saved})
        bufs, rays_g = {k: rows(t) for k, t in bufs.items()}, rows(rays)

        def draw(g, name, cols, scale=None):
            """Device pointer of launch g's rows of the explicit draw `name` (None when it is not supplied: the library then
            draws in the kernel), kept alive.  With `scale` it is sigma noise: drawn here unless supplied, and scaled."""
            if cols == 0:
                return None
            if draws is not None and name in draws:
                t = torch.as_tensor(draws[name], dtype=torch.float32).reshape(G, R, cols)[g].to(dev)
            elif scale is not None:
                t = torch.randn(R, cols, device=dev, dtype=torch.float32)
            else:
                return None
            t = (t * scale if scale is not None else t).contiguous()
            keep.append(t)
            return t.data_ptr()

        def opts(g):
            o = RenderOpts(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=float(self.depth_std),
                           white_bkgd=int(bool(self.white_bkgd)), lindisp=int(bool(self.lindisp)),
                           seed=(self.base_seed + 7919 * self._calls + g) & 0xFFFFFFFFFFFFFFFF)
            o.u_coarse_dev = draw(g, "u_coarse", kc)
            o.u_fine_dev = draw(g, "u_fine", kf - kfd)
            o.u_fine2_dev = draw(g, "u_fine2", kf - kfd)
            o.g_depth_dev = draw(g, "g_depth", kfd)
            if self.training and self.noise_std > 0.0:
                # sigma noise (nerf.py:231-232), training only: drawn here (or replayed from draws["noise_coarse" /
                # "noise_fine"], unit normals) and handed to the composite kernels already scaled
                o.sigma_noise_coarse_dev = draw(g, "noise_coarse", kc, float(self.noise_std))
                if use_fine:
                    o.sigma_noise_fine_dev = draw(g, "noise_fine", kc + kf, float(self.noise_std))
            return o

        for g, h in enumerate(handles):
            with torch.cuda.stream(streams[g]):
                o, out = opts(g), RenderOut(**{k: t[g].data_ptr() for k, t in bufs.items()})
                if save:
                    saved["opts"].append(o)
                if stash:   # training forward into the reserved stash (pny_scene_stash_next_render)
                    check(L.pny_scene_stash_next_render(h, 1))
                check(L.pny_render(h, ptr(rays_g[g]), R, C.byref(o), C.byref(out), stream_of(dev)))
        model.join_streams(streams)
        model._last_call_group = group
        if save:
            saved["keep"], saved["group"] = keep, group
        return res, saved

    def sched_step(self, steps=1):
        """Sample-count schedule of the reference (nerf.py:324-344): sched = [iterations, n_coarse, n_fine];
        once iter_idx passes sched[0][i] the renderer switches to (sched[1][i], sched[2][i])."""
        if self.sched is None:
            return
        self.iter_idx += steps
        milestones, coarse_counts, fine_counts = self.sched
        stage = int(self.last_sched.item())
        while stage < len(milestones) and int(self.iter_idx.item()) >= milestones[stage]:
            self.n_coarse, self.n_fine = coarse_counts[stage], fine_counts[stage]
            print("INFO: NeRF sampling resolution changed on schedule ==> c", self.n_coarse, "f", self.n_fine)
            stage += 1
        self.last_sched.fill_(stage)

    @classmethod
    def from_conf(cls, conf, white_bkgd=False, lindisp=False, eval_batch_size=100000):
        return cls(conf.get_int("n_coarse", 128), conf.get_int("n_fine", 0),
                   n_fine_depth=conf.get_int("n_fine_depth", 0), noise_std=conf.get_float("noise_std", 0.0),
                   depth_std=conf.get_float("depth_std", 0.01), white_bkgd=conf.get_float("white_bkgd", white_bkgd),
                   lindisp=lindisp, eval_batch_size=conf.get_int("eval_batch_size", eval_batch_size),
                   sched=conf.get_list("sched", None))

    def bind_parallel(self, net, gpus=None, simple_output=False):
        """reference nerf.py:360-377.  The reference wraps the module in a single-process ``DataParallel(dim=1)`` that
        re-broadcasts all parameters and the latent on every call; a `gpus` list longer than one gives the same call
        signature on persistent per-device replicas instead (_MultiDeviceRenderWrapper).  The recommended multi-GPU path
        stays one process per GPU (dist.py: per-rank ray generation + one RCCL all-gather)."""
        if gpus is not None and len(gpus) > 1:
            return _MultiDeviceRenderWrapper(net, self, gpus, simple_output=simple_output)
        return _RenderWrapper(net, self, simple_output=simple_output)


class YoloRenderer(torch.nn.Module):
    """Drop-in for reference src/render/yolo.py:3 (forward :37-114, from_conf :28-35,
    bind_parallel :116-121)."""

    def __init__(self, n_coarse, eval_batch_size, num_scales, num_anchors_per_scale):
        super().__init__()
        self.net = None
        self.n_coarse = n_coarse
        self.eval_batch_size = eval_batch_size  # unused (see module docstring)
        self.num_scales = num_scales
        self.num_anchors_per_scale = num_anchors_per_scale
        self.draws = None
        self.base_seed = 4321
        self._calls = 0
        self._debug_raw = None     # test aid: (n, n_coarse, d_out) tensor that the next calls write the per-sample vectors to

    def bind_net(self, net):
        self.net = net

    @classmethod
    def from_conf(cls, conf):
        return cls(conf.get_int("renderer.n_coarse", 128), conf.get_int("renderer.eval_batch_size", 1024),
                   conf.get_int("model.mlp_coarse.num_scales", 1),
                   conf.get_int("model.mlp_coarse.num_anchors_per_scale", 3))

    def forward(self, rays):
        """rays (..., 8) flattened to (N, 8) as the reference does (SB is folded away: only SB=1
        is meaningful, yolo.py:38,81) -> (N, num_anchors_per_scale, 7).  Under autograd (trainable MLP parameters,
        grad mode on) the result carries a graph: backward = pny_yolo_render_backward (YoloTrainer.py:160-186)."""
        net = self.net
        params = net.trainable_mlp_parameters() if (torch.is_grad_enabled() and net.training) else []
        lat = net.differentiable_latent()
        if params or lat is not None:
            if lat is None:
                net.check_differentiable()
            return _YoloRenderFunction.apply(self, rays, len(params), *[p for _, p in params], *([lat] if lat is not None else []))
        draws, calls = self.draws, self._calls

        def call():
            self.draws, self._calls = draws, calls
            return self._render(rays)[0]
        return net.guard_f16_range(call)

    def _render(self, rays, keep_raw=False):
        net = self.net
        net._sync()
        L = _lib.load()
        dev = net._device()
        rays = rays.detach().to(dev, torch.float32).reshape(-1, 8).contiguous()
        if rays.data_ptr() % 16:
            rays = rays.clone()
        n = rays.shape[0]
        out = torch.empty(n, self.num_anchors_per_scale, 7, device=dev, dtype=torch.float32)
        draws, self.draws = self.draws, None
        self._calls += 1
        u = None
        if draws is not None:
            u = torch.as_tensor(draws["u_coarse"], dtype=torch.float32).reshape(n, self.n_coarse).to(dev).contiguous()
        raw = self._debug_raw
        if raw is None and keep_raw:
            raw = torch.empty(n, int(self.n_coarse), net.d_out, device=dev, dtype=torch.float32)
        seed = (self.base_seed + 7919 * self._calls) & 0xFFFFFFFFFFFFFFFF
        check(L.pny_yolo_render(net._scene(0), ptr(rays), n, int(self.n_coarse), ptr(u), seed, ptr(out), ptr(raw),
                                stream_of(dev)))
        return out, dict(rays=rays, u=u, seed=seed, raw=raw, n_coarse=int(self.n_coarse))

    def bind_parallel(self, net, gpus=None):
        """reference yolo.py:116-121 (DataParallel(self, gpus, dim=1) for several devices: here persistent per-device
        replicas, _MultiDeviceYoloWrapper)."""
        self.net = net
        if gpus is not None and len(gpus) > 1:
            return _MultiDeviceYoloWrapper(net, self, gpus)
        return self


class _YoloRenderFunction(torch.autograd.Function):
    """YoloRenderer.forward under autograd: pny_yolo_render forward (raw per-sample vectors kept),
    pny_yolo_render_backward into gradient buffers bound to the parameters of mlp_coarse."""

    @staticmethod
    def forward(ctx, renderer, rays, n_params, *params):
        lat = params[n_params] if len(params) > n_params else None
        ctx.lat_meta = None if lat is None else renderer.net.latent_meta(lat)
        out, saved = renderer._render(rays, keep_raw=True)
        ctx.renderer, ctx.saved, ctx.net = renderer, saved, renderer.net   # (the net of THIS call: a per-device replica under bind_parallel)
        return out

    @staticmethod
    def backward(ctx, g_out):
        net, sv = ctx.net, ctx.saved
        L = _lib.load()
        dev = net._device()
        grads = net.bind_mlp_grads()
        g_out = g_out.detach().to(dev, torch.float32).contiguous()
        scene = net._scene(0)
        with net.latent_grad(ctx.lat_meta, [scene]) as lg:
            check(L.pny_yolo_render_backward(scene, ptr(sv["rays"]), sv["rays"].shape[0], sv["n_coarse"], ptr(sv["u"]),
                                             sv["seed"], ptr(sv["raw"]), ptr(g_out), _lib.ACC_ADD, stream_of(dev)))
            extra = lg.result()
        net._lat_grad_event = None      # (unmarked: a trunk backward behind this one waits for the whole stream)
        return (None, None, None) + tuple(grads) + extra


def make_renderer(conf, lindisp=False):
    """reference src/render/render_util.py:5-12"""
    renderer_type = conf.get_string("renderer.type", "nerf")
    if renderer_type == "nerf":
        return NeRFRenderer.from_conf(conf["renderer"], lindisp=lindisp)
    if renderer_type == "yolo":
        return YoloRenderer.from_conf(conf)
    raise NotImplementedError("Unsupported renderer type")
