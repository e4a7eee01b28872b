#!/usr/bin/env python3
"""The host-side parts of a YOLO training step around the renderer, the loss and the backward, two ways:

  (a) batch construction
      reference_style: the reference's call-site sequence (train/trainlib/YoloTrainer.py:93-129) on this package's API as it was
                       before util.yolo_train_batch: per scale and view one `.to(device)` of a target grid, stack + squeeze,
                       util.gen_rays_yolo of the selected views, two indexings by image_ord, two reshapes;
      one_launch:      util.stage_yolo_targets (one stack and one copy per scale) + util.yolo_train_batch (one kernel);
  (b) the finiteness tests of ONE mini-batch
      reference_style: YoloTrainer.py:163-178 and :188-194 -- four `if torch.is{nan,inf}(x).any()` on the render and the targets,
                       then torch.isnan(p.grad).any() and torch.isinf(p.grad).any() for every parameter of the net;
      monitor:         util.FiniteMonitor: check(render), check(targets), check(grads) -- three launches, no read (the step's
                       single read, report(), is timed on its own);
  (c) a whole training step: encode of a supplied latent that requires grad, the renders, the losses, the backwards, the
      finiteness tests and the logged values, on the model of conf.yolo() (L = 1792)
      looped:          the trainer's loop (YoloTrainer.py:149-208) on the per-mini-batch API: per mini-batch of 128 rays one
                       render, loss.YoloLoss, backward(retain_graph=True), three FiniteMonitor checks and five .item();
      one_pass:        util.yolo_train_batch(flat=True), ONE render of all rays, loss.YoloLoss.forward_batches, ONE backward,
                       the three checks once, one step_terms.tolist();
      at the shipped geometry (960 x 512, cell 32, 3 views: 1440 rays, 12 mini-batches) and at three scales (cells 8, 16, 32).
      Both legs end with FiniteMonitor.report() + reset() and start from gradients set to None.  blocking_reads counts the
      step's device -> host reads at the tool's own call sites (.item(), .tolist(), report()); torch.profiler files a 4-byte
      .item() under copies_other.

Shapes: the shipped configuration (conf/exp/yolo.conf of the reference: one scale of cell 32, 3 of 49 views, 3 anchors,
128-ray mini-batches) on a 600 x 800 frame, and the same with three scales (cells 8, 16, 32).  The gradients are zero-filled
buffers of the model's real parameter list (conf.yolo()); the render and targets of a mini-batch are (128, 3, 7) / (128, 3, 6).
Per leg, after warm-up, each call on its own with the device idle at the start: wall_ms = host clock from the call to a device
synchronise behind it, issue_ms = host clock until the call returns.  Median (p25, p75) over --calls calls.  Kernel launches,
device copies by direction and the host's stream / device synchronisations are counted by torch.profiler on one further call
(the tool's own synchronise at the end of that call taken off); a blocking read shows as a device-to-host copy.  The
reference-style batch leg keeps `focal` and `c` on the device, where the reference's trainer puts them (YoloTrainer.py:65-66),
and so reads them back once per scale inside gen_rays_yolo; the one-launch leg takes them from the CPU, as the dataset hands
them over: that part of the difference is the call site's, not the kernels'.  Prints one JSON line per leg and writes them
to profiles/yolo_step_sweep.json.

usage: python tools/yolo_step_sweep.py [--calls 30] [--warmup 5] [--step-calls 20] [--out profiles/yolo_step_sweep.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, NV, NS, A, MB = 600, 800, 49, 3, 3, 128
SHAPES = {"shipped_1_scale": [32], "three_scales": [8, 16, 32]}
Z_NEAR, Z_FAR = 1.0, 6.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-calls", type=int, default=20, help="timed calls of each whole-step leg (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_step_sweep.json"))
    args = ap.parse_args()
    assert args.calls >= 20 and args.step_calls >= 20, "median of at least 20 calls"

    import numpy as np
    import torch

    import pnyolo_pkg
    pnyolo_pkg.load()
    from pixel_nerf_yolo_amd import conf as pconf, synth
    from pixel_nerf_yolo_amd.model import make_model
    from pixel_nerf_yolo_amd.lib import PnyError as plib_errors
    from pixel_nerf_yolo_amd.util import FiniteMonitor, gen_rays_yolo, stage_yolo_targets, yolo_train_batch

    dev = torch.device("cuda", 0)

    def counted(fn):
        """Device kernels, device copies by direction and host-side synchronisations of one call (torch.profiler)."""
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        c = dict(kernel_launches=0, copies_h2d=0, copies_d2h=0, copies_other=0, host_synchronisations=-1)
        for e in prof.events():
            name = e.name.lower()
            if str(e.device_type).endswith("CUDA"):
                if name.startswith(("memcpy", "memset")):
                    c["copies_d2h" if "dtoh" in name else "copies_h2d" if "htod" in name else "copies_other"] += 1
                else:
                    c["kernel_launches"] += 1
            elif name in ("hipstreamsynchronize", "hipdevicesynchronize", "hipeventsynchronize"):
                c["host_synchronisations"] += 1
        return c

    def timed(fn, calls=None):
        calls = args.calls if calls is None else calls
        wall, issue = [], []
        for it in range(args.warmup + calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= args.warmup:
                wall.append((t2 - t0) * 1e3)
                issue.append((t1 - t0) * 1e3)
            del out

        def q(v):
            return [round(float(np.percentile(v, p)), 4) for p in (50, 25, 75)]
        return dict(wall_ms=q(wall), issue_ms=q(issue), **counted(fn))

    rows = []
    flipyz = np.diag([1.0, -1.0, -1.0, 1.0])
    poses = torch.from_numpy(np.stack([np.linalg.inv(synth.pose_spherical(360.0 * v / NV, -20.0, 4.0).astype(np.float64) @ flipyz)
                                       for v in range(NV)]).astype(np.float32))          # data["poses"][0], CPU
    focal, c = torch.tensor([700.0, 705.0], device=dev), torch.tensor([400.0, 300.0], device=dev)   # all_focals / all_c, on the device (:65-66)
    image_ord = torch.tensor([7, 30, 18])
    rs = np.random.RandomState(3)

    # ---- (a) batch construction
    for shape, cells in SHAPES.items():
        all_bboxes = [tuple(torch.from_numpy(rs.rand(1, H // cell, W // cell, A, 6).astype(np.float32)) for cell in cells) for _ in range(NV)]

        def reference_style():
            """YoloTrainer.py:93-129 in this tool's words, on the package's earlier API: per scale, every view's grid copied to
            the device on its own and stacked (:97-101), gen_rays_yolo of the selected views at the grid's size with the device-side
            intrinsics divided by the cell (:104-115), rays and grids taken at image_ord and flattened (:120-125)."""
            rays, targets = [], []
            for s, cell in enumerate(cells):
                grid = torch.stack([view[s].to(device=dev) for view in all_bboxes]).squeeze(1)
                r = gen_rays_yolo(poses[image_ord], W // cell, H // cell, focal / cell, c / cell, Z_NEAR, Z_FAR, device=dev)
                rays.append(r.reshape(-1, 8))
                targets.append(grid[image_ord].reshape(-1, A, 6))
            return rays, targets

        focal_h, c_h = focal.cpu(), c.cpu()                      # data["focal"] / data["c"] as the dataset hands them over

        def one_launch():
            grids = stage_yolo_targets(all_bboxes, dev)
            return yolo_train_batch(poses, image_ord, focal_h, c_h, grids, H, W, cells, Z_NEAR, Z_FAR)

        for leg, fn in (("reference_style", reference_style), ("one_launch", one_launch)):
            row = dict(part="batch", shape=shape, cells=cells, H=H, W=W, NV=NV, NS=NS, A=A,
                       rays=int(sum(NS * (H // cl) * (W // cl) for cl in cells)), leg=leg, calls=args.calls, **timed(fn))
            rows.append(row)
            print(json.dumps(row), flush=True)

    # ---- (b) the finiteness tests of one mini-batch
    net = make_model(pconf.yolo()["model"]).to(dev)
    params = list(net.parameters())
    for p in params:
        p.grad = torch.zeros_like(p)
    render, bboxes_gt = torch.rand(MB, A, 7, device=dev), torch.rand(1, MB, A, 6, device=dev)

    def reference_checks():
        """YoloTrainer.py:163-178 and :188-194 in this tool's words: NaN and Inf tests of the render and the targets, each
        decided on the host, then the same two tests over every parameter's gradient."""
        hits = 0
        for x in (render, bboxes_gt):
            hits += bool(torch.isnan(x).any()) + bool(torch.isinf(x).any())
        grads = [p.grad for p in params if p.grad is not None]
        hits += any(bool(torch.isnan(g).any()) for g in grads)
        hits += any(bool(torch.isinf(g).any()) for g in grads)
        return hits

    mon = FiniteMonitor(("render", "targets", "grads"), dev)
    mon.watch("grads", params, grads=True)

    def monitor_checks():
        mon.check("render", render)
        mon.check("targets", bboxes_gt)
        mon.check("grads")

    def monitor_report():
        out = mon.report()
        mon.reset()
        return out

    n_el = int(sum(p.numel() for p in params))
    for leg, fn in (("reference_style", reference_checks), ("monitor", monitor_checks), ("monitor_report_per_step", monitor_report)):
        row = dict(part="finite_checks_per_mini_batch" if leg != "monitor_report_per_step" else "finite_report_per_step", leg=leg,
                   parameter_tensors=len(params), parameter_elements=n_el, mini_batch=MB, calls=args.calls, **timed(fn))
        rows.append(row)
        print(json.dumps(row), flush=True)
    mon.close()
    del net, params, mon

    # ---- (c) a whole training step, looped and in one pass
    from pixel_nerf_yolo_amd import loss as ploss
    from pixel_nerf_yolo_amd.render import YoloRenderer
    SH, SW, LAT_HW = 512, 960, (64, 120)                         # the shipped frame (1920 x 1080 by yolo.image_scale) and a latent of 1 / 8
    conf = pconf.yolo()
    net = make_model(conf["model"]).to(dev).train()
    ren = YoloRenderer.from_conf(conf)
    render_par = ren.bind_parallel(net)
    crit = ploss.YoloLoss(A, 1.0, 20.0, 1.0, 1.0)                # yolo.weights of the shipped conf
    lat = (0.5 * torch.randn(NS, net.d_latent, *LAT_HW, generator=torch.Generator().manual_seed(5))).to(dev).requires_grad_()
    s_focal, s_c = torch.tensor([840.0, 846.0]), torch.tensor([480.0, 256.0])
    src_poses, no_images = poses[image_ord][None], torch.zeros(1, NS, 3, SH, SW)   # (encode reads the poses on the host)
    names = [n for n, _ in net.named_parameters()]
    params = list(net.parameters())
    mon = FiniteMonitor(("render", "targets", "grads"), dev)
    mon.watch("grads", params, names, grads=True)
    all_anchors = [torch.tensor(a, device=dev) for a in conf["yolo.anchors"]]

    failed = False
    for shape, cells in SHAPES.items():
        if failed:
            break
        anchors = all_anchors[-len(cells):]
        gen = torch.Generator().manual_seed(6)
        grids = []
        for cell in cells:                                       # dataset-like targets: 25 % object cells, 10 % ignored
            g = torch.rand(NV, SH // cell, SW // cell, A, 6, generator=gen)
            u = g[..., 0].clone()
            g[..., 0] = torch.where(u < 0.25, torch.ones(()), torch.where(u < 0.35, -torch.ones(()), torch.zeros(())))
            g[..., 3:5] = 0.02 + 0.88 * g[..., 3:5]
            g[..., 5] = torch.floor(2.0 * g[..., 5]).clamp(max=1.0)
            grids.append(g.to(dev))

        def begin():
            net.zero_grad(set_to_none=True)
            lat.grad = None
            net.encode(no_images, src_poses, s_focal[None], c=s_c[None], latent=lat)

        reads = [0]                                              # blocking device -> host reads, counted where the step makes them

        def end():
            report = mon.report()
            reads[0] += 1
            mon.reset()
            return report

        def looped():
            begin()
            all_rays, all_bboxes_gt = yolo_train_batch(poses, image_ord, s_focal, s_c, grids, SH, SW, cells, Z_NEAR, Z_FAR)
            totals, mini_batch = [0.0] * 5, 0
            for s, (rays_on_scale, bboxes_on_scale) in enumerate(zip(all_rays, all_bboxes_gt)):
                for rays, bboxes_gt in zip(torch.split(rays_on_scale.unsqueeze(0), MB, dim=1),
                                           torch.split(bboxes_on_scale.unsqueeze(0), MB, dim=1)):
                    mini_batch += 1
                    render = render_par(rays).reshape(1, rays.shape[1], A, 7)
                    mon.check("render", render)
                    mon.check("targets", bboxes_gt)
                    out = crit(render, bboxes_gt, anchors[s])
                    out[0].backward(retain_graph=True)
                    mon.check("grads")
                    for j, o in enumerate(out):
                        totals[j] += o.item()
                        reads[0] += 1
            return [t / mini_batch for t in totals], end()

        def one_pass():
            begin()
            rays, bboxes_gt, rows = yolo_train_batch(poses, image_ord, s_focal, s_c, grids, SH, SW, cells, Z_NEAR, Z_FAR, flat=True)
            render = render_par(rays[None]).reshape(1, rays.shape[0], A, 7)
            mon.check("render", render)
            mon.check("targets", bboxes_gt)
            loss_sum, step_terms = crit.forward_batches(render, bboxes_gt[None], anchors, rows, MB)
            loss_sum.backward()
            mon.check("grads")
            logged = step_terms.tolist()[1:]
            reads[0] += 1
            return logged, end()

        n_rays = int(sum(NS * (SH // cl) * (SW // cl) for cl in cells))
        n_mb = int(sum(-(-NS * (SH // cl) * (SW // cl) // MB) for cl in cells))
        for leg, fn in (("looped", looped), ("one_pass", one_pass)):
            row = dict(part="whole_step", shape=shape, cells=cells, H=SH, W=SW, NS=NS, A=A, rays=n_rays, mini_batches=n_mb,
                       d_latent=int(net.d_latent), latent_hw=list(LAT_HW), leg=leg, calls=args.step_calls)
            try:
                reads[0] = 0
                logged, report = fn()
                row.update(logged=[round(v, 6) for v in logged], clean=not any(r[0] or r[1] for r in report.values()),
                           blocking_reads=reads[0], **timed(fn, args.step_calls))
            except (plib_errors, RuntimeError) as e:             # reported, not hidden; nothing more is started behind an error
                row["error"], failed = "%s: %s" % (type(e).__name__, e), True
            rows.append(row)
            print(json.dumps(row), flush=True)
            if failed:
                break
    mon.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), note="median, p25, p75 per timing entry; counts are torch.profiler's for one call; the reference_style batch leg "
                            "reads focal and c back from the device once per scale (they live there in the reference's trainer), "
                            "the one_launch leg takes them from the CPU", rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
