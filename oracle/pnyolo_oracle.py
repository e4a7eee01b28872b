"""
ORACLE -- TEST INFRASTRUCTURE ONLY.  A CPU restatement (torch CPU tensors used as a plain
fp32 array library) of the pixelNeRF-YOLO rendering hot path of kofinandi/pixel-nerf-yolo.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this file,
and only as the checker / the timed CPU baseline -- never as a product path.  The product
(pixel-nerf-yolo_amd/) fails loudly when libpnyolo.so or a GPU is missing; it never falls
back to this code.

Pinning: every function below is checked in tests/test_oracle_golden.py against fixtures
captured by tools/make_golden.py from the reference itself imported on CPU in the build
container (the reference has no golden vectors of its own).  Two boundaries stay
PARITY UNPINNED because the third-party code is absent from the container: torchvision's
ResNet-34 definition (restated from the public architecture, arithmetic = torch conv2d /
batch_norm) and the NeRF-YOLO `models.yolo.Model` backbone (its output, the latent, is an
input here).

Each function cites the reference file:line (relative to /root/reference) it follows.
"""
import math

import torch
import torch.nn.functional as F

f32 = torch.float32


def T(x, dtype=None):
    return torch.as_tensor(x, dtype=f32 if dtype is None else dtype)


# ----------------------------------------------------------------------------- rays
def gen_rays(poses, width, height, focal, z_near, z_far, c=None):
    """src/util/util.py:115-145 (unproj_map) + :240-278 (gen_rays), ndc branch dead.
    poses (B,4,4) cam->world; focal scalar or (fx,fy); c (cx,cy) or None -> image centre.
    Pixel coordinates are integers (no +0.5); camera looks down -z; dirs are unit length."""
    poses = T(poses)
    focal = T(focal).reshape(-1)
    fx, fy = (float(focal[0]), float(focal[0])) if focal.numel() == 1 else (float(focal[0]), float(focal[1]))
    if c is None:
        cx, cy = width * 0.5, height * 0.5
    else:
        c = T(c).reshape(-1)
        cx, cy = float(c[0]), float(c[1])
    ys = (torch.arange(height, dtype=f32) - cy) / fy
    xs = (torch.arange(width, dtype=f32) - cx) / fx
    Y = ys[:, None].expand(height, width)
    X = xs[None, :].expand(height, width)
    d = torch.stack((X, -Y, -torch.ones_like(X)), dim=-1)
    d = d / torch.norm(d, dim=-1, keepdim=True)
    B = poses.shape[0]
    R = poses[:, :3, :3]
    dirs = torch.einsum("bij,hwj->bhwi", R, d)
    orig = poses[:, None, None, :3, 3].expand(B, height, width, 3)
    near = torch.full((B, height, width, 1), float(z_near), dtype=f32)
    far = torch.full((B, height, width, 1), float(z_far), dtype=f32)
    return torch.cat((orig, dirs, near, far), dim=-1)


def gen_rays_yolo(poses, width, height, focal, c, z_near, z_far):
    """src/util/util.py:808-876.  poses (B,4,4) WORLD->cam extrinsics; direction =
    inv(E)[:3,:3] . K^-1 [x+0.49, y+0.49, 1] (not normalised, +z forward); origin = inv(E)[:3,3].
    The reference builds a (W,H) grid and permutes to (H,W)."""
    poses = T(poses)
    focal = T(focal).reshape(-1)
    c = T(c).reshape(-1)
    K = torch.tensor([[focal[0], 0, c[0]], [0, focal[1], c[1]], [0, 0, 1]], dtype=f32)
    Kinv = torch.inverse(K)
    xs = torch.linspace(0, width - 1, width) + 0.49
    ys = torch.linspace(0, height - 1, height) + 0.49
    gx = xs[None, :].expand(height, width)
    gy = ys[:, None].expand(height, width)
    pix = torch.stack((gx, gy, torch.ones_like(gx)), dim=-1)  # (H,W,3)
    dcam = torch.einsum("ij,hwj->hwi", Kinv, pix)
    out = []
    for b in range(poses.shape[0]):
        Einv = torch.inverse(poses[b])
        dw = torch.einsum("ij,hwj->hwi", Einv[:3, :3], dcam)
        o = Einv[:3, 3][None, None].expand(height, width, 3)
        near = torch.full((height, width, 1), float(z_near), dtype=f32)
        far = torch.full((height, width, 1), float(z_far), dtype=f32)
        out.append(torch.cat((o, dw, near, far), dim=-1))
    return torch.stack(out)


# ----------------------------------------------------------------------------- sampling
def sample_coarse(rays, n_coarse, u, lindisp=False):
    """src/render/nerf.py:104-121 (same arithmetic in src/render/yolo.py:15-26).
    u (N,Kc) ~ U[0,1) is the renderer's first random draw (unconditional, also in eval).  The arithmetic is rays' dtype."""
    near, far = rays[:, 6:7], rays[:, 7:8]
    step = 1.0 / n_coarse
    t = torch.linspace(0, 1 - step, n_coarse, dtype=rays.dtype)[None, :].repeat(rays.shape[0], 1)
    t = t + T(u, rays.dtype) * step
    if not lindisp:
        return near * (1 - t) + far * t
    return 1 / (1 / near * (1 - t) + 1 / far * t)


def sample_fine(rays, weights, u, u2, n_coarse, lindisp=False):
    """src/render/nerf.py:126-154.  u, u2 (N, Kf-Kfd): the 2nd and 3rd random draws."""
    w = weights + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    inds = torch.searchsorted(cdf, T(u, cdf.dtype).contiguous(), right=True).to(cdf.dtype) - 1.0
    inds = torch.clamp_min(inds, 0.0)
    t = (inds + T(u2, cdf.dtype)) / n_coarse
    near, far = rays[:, 6:7], rays[:, 7:8]
    if not lindisp:
        return near * (1 - t) + far * t
    return 1 / (1 / near * (1 - t) + 1 / far * t)


def sample_fine_depth(rays, depth, g, depth_std):
    """src/render/nerf.py:156-167.  g (N,Kfd) ~ N(0,1): the 4th random draw."""
    z = depth[:, None].repeat(1, g.shape[1])
    z = z + T(g, z.dtype) * depth_std
    return torch.max(torch.min(z, rays[:, 7:8]), rays[:, 6:7])


def composite(rays, z, out, white_bkgd, sigma_noise=None):
    """src/render/nerf.py:184-188 (deltas, last = far - z_last) and :229-250
    (alpha, shifted cumprod transmittance, weights, rgb/depth sums, white background).
    out (N,K,4) = per-sample [sigmoid rgb, relu sigma] from the model.  sigma_noise (N,K): the training-time
    `randn_like(sigmas) * noise_std` (nerf.py:231-232), a random draw like the others."""
    deltas = torch.cat([z[:, 1:] - z[:, :-1], rays[:, 7:8] - z[:, -1:]], -1)
    rgbs, sigmas = out[..., :3], out[..., 3]
    if sigma_noise is not None:
        sigmas = sigmas + T(sigma_noise, sigmas.dtype)
    alphas = 1 - torch.exp(-deltas * torch.relu(sigmas))
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-10], -1)
    Tr = torch.cumprod(shifted, -1)
    weights = alphas * Tr[:, :-1]
    rgb = torch.sum(weights.unsqueeze(-1) * rgbs, -2)
    depth = torch.sum(weights * z, -1)
    if white_bkgd:
        rgb = rgb + 1 - weights.sum(dim=1).unsqueeze(-1)
    return weights, rgb, depth


def yolo_aggregate(out, n_anchors=3):
    """src/render/yolo.py:96-114.  out (N,K,A*7) raw -> (N,A,7) = [max_k p, sum_k p*v/(sum_k p+1e-5)]."""
    N, K, _ = out.shape
    o = out.reshape(N, K, n_anchors, 7)
    p = torch.sigmoid(o[..., 0])
    ps = p.sum(dim=1)
    v = (o[..., 1:] * p.unsqueeze(-1)).sum(dim=1) / (ps.unsqueeze(-1) + 1e-5)
    return torch.cat([p.max(dim=1)[0].unsqueeze(-1), v], dim=-1)


# ----------------------------------------------------------------------------- model pieces
def positional_encoding(x, num_freqs=6, freq_factor=1.5):
    """src/model/code.py:11-42: out = [x, sin(f0 x), sin(f0 x + pi/2), sin(f1 x), ...] with the
    argument formed as fp32 (phase + x*freq; float64 for a float64 x); cos is obtained as sin(. + pi/2)."""
    dt = torch.float64 if x.dtype == torch.float64 else f32
    freqs = freq_factor * 2.0 ** torch.arange(0, num_freqs, dtype=dt)
    fr = torch.repeat_interleave(freqs, 2).view(1, -1, 1).to(dt)
    ph = torch.zeros(2 * num_freqs, dtype=dt)
    ph[1::2] = math.pi * 0.5
    ph = ph.view(1, -1, 1).to(dt)
    e = x.unsqueeze(1).repeat(1, num_freqs * 2, 1)
    e = torch.sin(ph + e * fr)
    return torch.cat((x, e.view(x.shape[0], 2 * num_freqs * x.shape[1])), dim=-1)   # (sized: num_freqs may be 0)


def encode_cameras(poses, focal, c, width, height, yolo=False, dtype=None):
    """src/model/models.py:115-148: cam->world poses inverted analytically to world->cam
    [R^T | -R^T t] (YOLO mode: extrinsics used as given); focal -> (.,2) with fy negated
    (non-YOLO); principal point defaults to the image centre.  dtype: the arithmetic (None = f32)."""
    dt = f32 if dtype is None else dtype
    poses = T(poses, dt).reshape(-1, 4, 4)
    if not yolo:
        rot = poses[:, :3, :3].transpose(1, 2)
        trans = -torch.bmm(rot, poses[:, :3, 3:])
        w2c = torch.cat((rot, trans), dim=-1)
    else:
        w2c = poses[:, :3, :4].clone()
    focal = T(focal, dt)
    if focal.dim() == 0:
        focal = focal[None, None].repeat(1, 2)
    elif focal.dim() == 1:
        focal = focal.unsqueeze(-1).repeat(1, 2)
    else:
        focal = focal.clone()
    if not yolo:
        focal[..., 1] *= -1.0
    if c is None:
        c = torch.tensor([[width * 0.5, height * 0.5]], dtype=dt)
    else:
        c = T(c, dt)
        if c.dim() == 0:
            c = c[None, None].repeat(1, 2)
        elif c.dim() == 1:
            c = c.unsqueeze(-1).repeat(1, 2)
    return w2c, focal, c


def index_latent(latent, uv, width, height, dtype=None):
    """src/model/encoder.py:79-108 with index_padding=zeros (conf/default.conf:49),
    align_corners=True, bilinear.  latent (NS,L,Hl,Wl); uv (NS,P,2) in image pixels.
    Returns (NS,P,L).  The bilinear lookup (F.grid_sample in the reference) is written out
    tap by tap: unnormalise ((g+1)/2)*(size-1), floor, 4 weighted taps, out-of-range taps = 0.
    dtype: the arithmetic (None = f32); latent and uv are converted differentiably."""
    dt = f32 if dtype is None else dtype
    latent, uv = T(latent, dt), T(uv, dt)
    NS, L, Hl, Wl = latent.shape
    ls = torch.tensor([Wl, Hl], dtype=dt)
    ls = ls / (ls - 1) * 2.0  # latent_scaling, encoder.py:170-172 (fp32 arithmetic)
    scale = ls / torch.tensor([width, height], dtype=dt)
    g = uv * scale - 1.0
    ix = ((g[..., 0] + 1) / 2) * (Wl - 1)
    iy = ((g[..., 1] + 1) / 2) * (Hl - 1)
    x0 = torch.floor(ix)
    y0 = torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    w_nw = (x1 - ix) * (y1 - iy)
    w_ne = (ix - x0) * (y1 - iy)
    w_sw = (x1 - ix) * (iy - y0)
    w_se = (ix - x0) * (iy - y0)
    lat = latent.permute(0, 2, 3, 1).reshape(NS, Hl * Wl, L)

    def tap(xi, yi, w):
        # Non-finite coordinates (0/0 or x/0 projections in YOLO mode) fail every bounds comparison: the tap reads
        # nothing, but its weight is NaN and ATen's vectorised CPU kernel multiplies masked value * weight, so the
        # sample comes out NaN (pinned by tests/golden/yolo_cull.npz: the reference reports "latent contains nan"
        # and then zeroes those rows, models.py:262-264).
        ok = (xi >= 0) & (xi <= Wl - 1) & (yi >= 0) & (yi <= Hl - 1)
        zero = torch.zeros_like(xi)
        idx = (torch.where(ok, yi, zero) * Wl + torch.where(ok, xi, zero)).long()
        v = torch.gather(lat, 1, idx.unsqueeze(-1).expand(-1, -1, L))
        return v * (w * ok.to(dt)).unsqueeze(-1)

    return tap(x0, y0, w_nw) + tap(x1, y0, w_ne) + tap(x0, y1, w_sw) + tap(x1, y1, w_se)


def _lin(sd, name, x):
    return torch.addmm(sd[name + ".bias"], x, sd[name + ".weight"].t())


# Test aid for gradient comparisons: when set to a list, every relu input of resnetfc() appends its per-query-point
# min |.| (B,) -- a point whose smallest |pre-activation| is below the fp32 agreement of two implementations has an
# ambiguous relu mask, and its gradient is not comparable across implementations (the gradient is discontinuous there).
RELU_TRACE = None


def _relu(t, rows_per_point):
    if RELU_TRACE is not None:
        m = t.detach().abs().min(dim=-1)[0]
        RELU_TRACE.append(m.reshape(rows_per_point, -1).min(dim=0)[0])
    return torch.relu(t)


def resnetfc(sd, z, x, ns, n_blocks=5, combine_layer=3, dtype=None):
    """src/model/resnetfc.py:134-186 (+ :53-62 block, util.py:489-499 combine):
    rows ordered view-major within a scene: row = v*B + b.  z (ns*B,L), x (ns*B,d_in).
    dtype: the arithmetic (None = f32); parameters and inputs are converted differentiably."""
    if dtype is not None:
        sd = {k: T(v, dtype) for k, v in sd.items()}
        z, x = T(z, dtype), T(x, dtype)
    h = _lin(sd, "lin_in", x)
    nv = ns
    for blk in range(n_blocks):
        if blk == combine_layer:
            h = h.reshape(ns, -1, h.shape[-1]).mean(dim=0)
            nv = 1
        if blk < combine_layer:
            h = h + _lin(sd, "lin_z.%d" % blk, z)
        net = _lin(sd, "blocks.%d.fc_0" % blk, _relu(h, nv))
        dx = _lin(sd, "blocks.%d.fc_1" % blk, _relu(net, nv))
        h = h + dx
    return _lin(sd, "lin_out", _relu(h, nv))


class Scene:
    """Per-scene state the reference keeps in module buffers after encode()
    (src/model/models.py:74-87,114-148; src/model/encoder.py:73-76,169-172)."""

    def __init__(self, mlp_coarse, mlp_fine, latent, poses, focal, c, width, height, yolo=False,
                 n_blocks=5, combine_layer=3, dtype=None, num_freqs=6, freq_factor=1.5):
        """num_freqs, freq_factor: the positional code of query() (conf model.code; d_in = 6 + 6 * num_freqs).
        dtype: the arithmetic of query / render / yolo_render on this scene (None = f32; torch.float64 = the
        high-precision arbiter of the GPU gradient sweeps).  Parameter and latent tensors assigned after construction
        may be of any dtype: they are converted differentiably where they are used."""
        self.dtype = f32 if dtype is None else dtype
        self.mlp_coarse = {k: T(v, dtype) for k, v in mlp_coarse.items()}
        self.mlp_fine = None if mlp_fine is None else {k: T(v, dtype) for k, v in mlp_fine.items()}
        self.latent = T(latent, dtype)
        self.w2c, self.focal, self.c = encode_cameras(poses, focal, c, width, height, yolo, dtype)
        self.width, self.height = width, height
        self.yolo = yolo
        self.ns = self.latent.shape[0]
        self.n_blocks, self.combine_layer = n_blocks, combine_layer
        self.num_freqs, self.freq_factor = num_freqs, freq_factor


def query(scene, xyz, viewdirs, coarse=True, dtype=None):
    """src/model/models.py:153-318 for SB=1 with the shipped flags (use_xyz, normalize_z,
    use_code, use_viewdirs, not use_code_viewdirs).  xyz, viewdirs (B,3) -> (B,d_out):
    [sigmoid rgb, relu sigma], or the raw vector in YOLO mode.  dtype: the arithmetic (None = the scene's)."""
    dt = getattr(scene, "dtype", f32) if dtype is None else dtype
    xyz, viewdirs = T(xyz, dt), T(viewdirs, dt)
    ns, B = scene.ns, xyz.shape[0]
    w2c = T(scene.w2c, dt)
    R, t = w2c[:, :, :3], w2c[:, :, 3]
    xr = torch.matmul(R[:, None], xyz[None, :, :, None])[..., 0]  # (ns,B,3) rotation only
    xc = xr + t[:, None]
    code = positional_encoding(xr.reshape(-1, 3), getattr(scene, "num_freqs", 6), getattr(scene, "freq_factor", 1.5))
    vd = torch.matmul(R[:, None], viewdirs[None, :, :, None])[..., 0].reshape(-1, 3)
    x_in = torch.cat((code, vd), dim=1)
    if not scene.yolo:
        uv = -xc[:, :, :2] / xc[:, :, 2:]
    else:
        uv = xc[:, :, :2] / xc[:, :, 2:]
    foc, cc = T(scene.focal, dt), T(scene.c, dt)
    foc = foc if foc.shape[0] > 1 else foc.expand(ns, 2)
    cc = cc if cc.shape[0] > 1 else cc.expand(ns, 2)
    uv = uv * foc[:, None] + cc[:, None]
    lat = index_latent(scene.latent, uv, scene.width, scene.height, dt).reshape(ns * B, -1)
    if scene.yolo:
        behind = (xc[:, :, 2] >= 0).reshape(-1, 1)  # models.py:224,254-264: zero where z >= 0 or NaN
        lat = torch.where(behind | torch.isnan(lat), torch.zeros_like(lat), lat)
    sd = scene.mlp_coarse if (coarse or scene.mlp_fine is None) else scene.mlp_fine
    out = resnetfc(sd, lat, x_in, ns, scene.n_blocks, scene.combine_layer, dt)
    if scene.yolo:
        return out
    return torch.cat([torch.sigmoid(out[:, :3]), torch.relu(out[:, 3:4])], dim=-1)


def _query_rays(scene, rays, z, coarse, chunk, dtype=None):
    N, K = z.shape
    pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(-1, 3)
    dirs = rays[:, None, 3:6].expand(-1, K, -1).reshape(-1, 3)
    outs = [query(scene, pts[i:i + chunk], dirs[i:i + chunk], coarse, dtype) for i in range(0, pts.shape[0], chunk)]
    return torch.cat(outs, 0).reshape(N, K, -1)


def render(scene, rays, n_coarse, n_fine, n_fine_depth, u_coarse, u_fine=None, u_fine2=None, g_depth=None,
           depth_std=0.01, white_bkgd=True, lindisp=False, chunk=50000, detach_fine_depth=False, noise_coarse=None,
           noise_fine=None, dtype=None):
    """src/render/nerf.py:257-309 (forward) for SB=1: coarse pass, then fine pass on
    sort(cat(z_coarse, z_fine, z_depth)) with the fine MLP.  The four random draws are inputs.
    Under autograd the reference detaches the coarse weights for importance sampling (nerf.py:132) but NOT the coarse
    depth the depth samples are centred on (nerf.py:296-298): the fine loss reaches the coarse MLP through the sample
    positions.  detach_fine_depth=True cuts that path (a test aid for the stages of the backward pass; the default is
    the reference's behaviour).  dtype: the arithmetic (None = the scene's)."""
    dt = getattr(scene, "dtype", f32) if dtype is None else dtype
    rays = T(rays, dt)
    res = {}
    zc = sample_coarse(rays, n_coarse, u_coarse, lindisp)
    oc = _query_rays(scene, rays, zc, True, chunk, dt)
    wc, rgbc, dc = composite(rays, zc, oc, white_bkgd, noise_coarse)
    res["coarse"] = dict(z=zc, out=oc, weights=wc, rgb=rgbc, depth=dc)
    if n_fine > 0:
        samps = [zc]
        if n_fine - n_fine_depth > 0:
            samps.append(sample_fine(rays, wc, u_fine, u_fine2, n_coarse, lindisp))
        if n_fine_depth > 0:
            samps.append(sample_fine_depth(rays, dc.detach() if detach_fine_depth else dc, g_depth, depth_std))
        zf, _ = torch.sort(torch.cat(samps, dim=-1), dim=-1)
        of = _query_rays(scene, rays, zf, False, chunk, dt)
        wf, rgbf, df = composite(rays, zf, of, white_bkgd, noise_fine)
        res["fine"] = dict(z=zf, out=of, weights=wf, rgb=rgbf, depth=df)
    return res


def yolo_render(scene, rays, n_coarse, u_coarse, n_anchors=3, chunk=50000, dtype=None):
    """src/render/yolo.py:37-114: coarse sampling only, raw MLP vectors, probability-weighted
    aggregation along each ray.  dtype: the arithmetic (None = the scene's)."""
    dt = getattr(scene, "dtype", f32) if dtype is None else dtype
    rays = T(rays, dt)
    z = sample_coarse(rays, n_coarse, u_coarse)
    raw = _query_rays(scene, rays, z, True, chunk, dt)
    return dict(z=z, raw=raw, out=yolo_aggregate(raw, n_anchors))


# ----------------------------------------------------------------------------- encoder
def _bn(sd, name, x, training=False):
    """nn.BatchNorm2d as torchvision's ResNet holds it (eps 1e-5, momentum 0.1): eval() mode normalises with the running
    statistics; train() mode with the batch's and steps running_mean / running_var IN PLACE (sd's tensors)."""
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"],
                        sd[name + ".bias"], training=training, momentum=0.1, eps=1e-5)


def _block(sd, p, x, stride, training=False, relu=torch.relu):
    idt = x
    if (p + "downsample.0.weight") in sd:
        idt = _bn(sd, p + "downsample.1", F.conv2d(x, sd[p + "downsample.0.weight"], stride=stride), training)
    out = relu(_bn(sd, p + "bn1", F.conv2d(x, sd[p + "conv1.weight"], stride=stride, padding=1), training))
    out = _bn(sd, p + "bn2", F.conv2d(out, sd[p + "conv2.weight"], padding=1), training)
    return relu(out + idt)


def spatial_encoder(sd, images, prefix="encoder.model.", use_first_pool=True, training=False, dtype=None, relu=None):
    """src/model/encoder.py:139-173 with num_layers=4, use_first_pool; batch norm in eval() mode, or -- training=True, the
    trunk as train/train.py leaves it without --freeze_enc -- on batch statistics (running statistics of `sd` stepped in place):
    conv1/bn1/relu -> L0; maxpool, layer1 -> L1; layer2 -> L2; layer3 -> L3; every level
    bilinearly upsampled (align_corners=True) to L0's size; channel concat (64+64+128+256).
    ResNet-34 BasicBlock layout [3,4,6] restated from the public architecture (torchvision is
    absent: PARITY UNPINNED at that boundary).  Returns (latent NCHW, [levels]).
    dtype: the arithmetic (None = f32; torch.float64 = the high-precision arbiter of the GPU trunk tests); parameters and images are
    converted differentiably, so leaves of another dtype still receive their gradients, and a float64 state's running
    statistics are stepped in place like a float32 one's.
    relu: a trace aid -- the function every relu of the trunk calls, in forward order (None = torch.relu): a hook that records
    the pre-activations or sets one unit's mask the other way (what an fp32 evaluation does to a unit within its rounding of
    zero)."""
    sd = {k[len(prefix):]: T(v, dtype) for k, v in sd.items() if k.startswith(prefix)}
    x = T(images, dtype)
    relu = torch.relu if relu is None else relu
    x = relu(_bn(sd, "bn1", F.conv2d(x, sd["conv1.weight"], stride=2, padding=3), training))
    levels = [x]
    if use_first_pool:  # encoder.py:145-146 (sn64.conf sets use_first_pool = False)
        x = F.max_pool2d(x, 3, 2, 1)
    for li, n in ((1, 3), (2, 4), (3, 6)):
        for b in range(n):
            x = _block(sd, "layer%d.%d." % (li, b), x, 2 if (b == 0 and li > 1) else 1, training, relu)
        levels.append(x)
    size = levels[0].shape[-2:]
    ups = [F.interpolate(l, size, mode="bilinear", align_corners=True) for l in levels]
    return torch.cat(ups, dim=1), levels


# ----------------------------------------------------------------------------- YOLO detection tail
def iou_xywh(a, b):
    """src/util/util.py:576-611 (is_pred=True) on [x, y, w, h] rows, fp32 op for op (numpy float32
    scalars: the same IEEE single-precision +,-,*,/ torch performs on its 1-element tensors)."""
    import numpy as np
    f = np.float32
    a = [f(v) for v in a]
    b = [f(v) for v in b]
    two = f(2.0)
    ax1, ay1, ax2, ay2 = a[0] - a[2] / two, a[1] - a[3] / two, a[0] + a[2] / two, a[1] + a[3] / two
    bx1, by1, bx2, by2 = b[0] - b[2] / two, b[1] - b[3] / two, b[0] + b[2] / two, b[1] + b[3] / two
    zero = f(0.0)
    inter = max(min(ax2, bx2) - max(ax1, bx1), zero) * max(min(ay2, by2) - max(ay1, by1), zero)
    union = abs((ax2 - ax1) * (ay2 - ay1)) + abs((bx2 - bx1) * (by2 - by1)) - inter
    return inter / (union + f(1e-6))


def cells_to_bboxes(cells, anchors, h, w, is_predictions=True):
    """src/util/util.py:633-689 for one image: cells (h,w,A,7|6) -> (h*w*A, 6) [class, score, x, y, w, h]."""
    c = T(cells)
    A = c.shape[2]
    box = c[..., 1:5].clone()
    if is_predictions:
        box[..., 0:2] = torch.sigmoid(box[..., 0:2])
        box[..., 2:] = torch.exp(box[..., 2:]) * T(anchors).reshape(1, 1, A, 2)
        cls = torch.argmax(c[..., 5:], dim=-1).unsqueeze(-1).to(f32)
    else:
        cls = c[..., 5:6]
    cx = torch.arange(w, dtype=f32).reshape(1, w, 1, 1).expand(h, w, A, 1)
    cy = torch.arange(h, dtype=f32).reshape(h, 1, 1, 1).expand(h, w, A, 1)
    x = (1 / w) * (box[..., 0:1] + cx)
    y = (1 / h) * (box[..., 1:2] + cy)
    wh = 1 / torch.tensor([w, h], dtype=f32) * box[..., 2:4]
    return torch.cat((cls, c[..., 0:1], x, y, wh), dim=-1).reshape(h * w * A, 6)


def nms(boxes, iou_threshold, threshold):
    """src/util/util.py:691-722.  boxes (n,6) fp32.  Confidence / size filters compare as Python
    floats; the suppression loop removes from the list it iterates, so the element following a
    removed one is skipped for that round.  Returns (kept rows, highest confidence, above-threshold count)."""
    rows = [[float(v) for v in r] for r in T(boxes).reshape(-1, 6).tolist()]
    highest = max(r[1] for r in rows)
    cand = [r for r in rows if r[1] > threshold]
    above = len(cand)
    cand = [r for r in cand if 10e-4 < r[4] < 10e4 and 10e-4 < r[5] < 10e4]
    order = sorted(range(len(cand)), key=lambda i: -cand[i][1])  # stable, descending
    lst = [cand[i] for i in order]
    thr32 = float(T(iou_threshold))
    kept = []
    while lst:
        first = lst.pop(0)
        kept.append(first)
        i = 0
        while i < len(lst):
            if float(iou_xywh(first[2:], lst[i][2:])) > thr32:
                # list.remove(box) deletes the FIRST element equal to box: an identical row further up (still there only
                # because the iterator skipped it) goes instead; the iterator then points past the element that moved here
                del lst[lst.index(lst[i])]
            i += 1
    return kept, highest, above


def tp_fp_fn(targets, preds, nms_iou, nms_t, match_iou):
    """src/util/util.py:765-802."""
    t, _, _ = nms(targets, nms_iou, nms_t)
    p, _, _ = nms(preds, nms_iou, nms_t)
    if len(t) == 0:
        return 0, len(p), 0
    if len(p) == 0:
        return 0, 0, len(t)
    m32 = float(T(match_iou))
    tp = fp = fn = 0
    for pb in p:
        if max(float(iou_xywh(pb[2:], tb[2:])) for tb in t) > m32:
            tp += 1
        else:
            fp += 1
    for tb in t:
        if max(float(iou_xywh(tb[2:], pb[2:])) for pb in p) < m32:
            fn += 1
    return tp, fp, fn


# ----------------------------------------------------------------------------- seeded random draws
# The renderers' DEFAULT source of draws: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
# as 1, 2, 3", SC'11) evaluated inside the kernels at (seed, stream, index).  Restated here from the paper's round
# function and the documented counter layout -- NOT parsed from pixel-nerf-yolo_amd/csrc/pny_rng.h: the tests are that
# two independent writings agree (tests/test_cpu_philox.py, tests/test_gpu_seeded.py).
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57            # the two round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85            # key increments per round (golden ratio, sqrt(3) - 1)
PHILOX_COUNTER3 = 0x9E3779B9                             # the renderer's fixed fourth counter word
STREAM_COARSE, STREAM_FINE, STREAM_FINE2, STREAM_DEPTH = 1, 2, 3, 4   # third counter word: which draw of the renderer


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: four words, key: two words; each a Python int or an integer array (broadcast against each
    other).  Returns the four output words as numpy uint64 arrays holding 32-bit values."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    c0, c1, c2, c3 = [np.asarray(x, dtype=np.uint64) & m32 for x in counter]
    k0, k1 = [np.asarray(x, dtype=np.uint64) & m32 for x in key]
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(PHILOX_W0)) & m32
        k1 = (k1 + np.uint64(PHILOX_W1)) & m32
    return c0, c1, c2, c3


def _philox_words(seed, stream, counter_idx):
    import numpy as np
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ci = np.asarray(counter_idx, dtype=np.uint64)
    return philox4x32_10((ci & np.uint64(0xFFFFFFFF), ci >> np.uint64(32), int(stream), PHILOX_COUNTER3),
                         (seed & 0xFFFFFFFF, seed >> 32))


def _u01(x):
    """Top 24 bits of a word as a multiple of 2^-24 in [0, 1): exact in fp32 and in fp64."""
    import numpy as np
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def philox_uniform(seed, stream, idx):
    """The uniform in [0, 1) at position idx of a stream: four per counter (counter = idx // 4, word = idx % 4).
    float32, exact."""
    import numpy as np
    idx = np.asarray(idx, dtype=np.uint64)
    w = np.stack(_philox_words(seed, stream, idx >> np.uint64(2)), -1)
    return _u01(np.take_along_axis(w, (idx & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]).astype(np.float32)


def philox_normal_inputs(seed, stream, idx):
    """(u1 in (0, 1], u2 in [0, 1)) of the Box-Muller normal at idx: two normals per counter (counter = idx // 2), normal
    idx % 2 takes words 2 * (idx % 2) and 2 * (idx % 2) + 1; u1 = 1 - u01(first word).  float64, exact in fp32."""
    import numpy as np
    idx = np.asarray(idx, dtype=np.uint64)
    w = np.stack(_philox_words(seed, stream, idx >> np.uint64(1)), -1)
    lane = (np.uint64(2) * (idx & np.uint64(1))).astype(np.int64)[..., None]
    u1 = 1.0 - _u01(np.take_along_axis(w, lane, -1)[..., 0])
    u2 = _u01(np.take_along_axis(w, lane + 1, -1)[..., 0])
    return u1, u2


def philox_normal(seed, stream, idx):
    """Box-Muller normal at idx: sqrt(-2 ln u1) cos(2 pi u2), evaluated in float64.  Returns (float64, rounded to float32).
    |g| <= sqrt(2 * 24 * ln 2) = 5.77."""
    import numpy as np
    u1, u2 = philox_normal_inputs(seed, stream, idx)
    g = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return g, g.astype(np.float32)


def seeded_draws(seed, n, kc, kf, kfd):
    """Every draw of one seeded render launch over n rays, with the kernels' index layouts (ray * columns + column, rays
    numbered within the launch): u_coarse (n, kc), u_fine and u_fine2 (n, kf - kfd), g_depth (n, kfd), float32,
    as render() / yolo_render() take them."""
    import numpy as np

    def index(cols):
        return (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(max(cols, 0))
                + np.arange(max(cols, 0), dtype=np.uint64)[None, :])
    kimp = max(kf - kfd, 0)
    return dict(u_coarse=philox_uniform(seed, STREAM_COARSE, index(kc)),
                u_fine=philox_uniform(seed, STREAM_FINE, index(kimp)),
                u_fine2=philox_uniform(seed, STREAM_FINE2, index(kimp)),
                g_depth=philox_normal(seed, STREAM_DEPTH, index(kfd))[1])
