/*
 * pnyolo.h -- C ABI of libpnyolo.so: the MI355X (gfx950) rendering hot path of
 * pixelNeRF-YOLO.  Plain pointers and sizes only; no torch types.
 *
 * The reference (kofinandi/pixel-nerf-yolo) is pure Python/PyTorch and has no FFI of its own:
 * the boundary it offers is the Python object protocol between its trainers / eval scripts
 * and src/render + src/model.  Each entry point below names the reference
 * interface it stands in for (file:line relative to the reference tree); the Python classes in
 * pixel-nerf-yolo_amd/ re-create those interfaces on top of this ABI.
 *
 * Conventions
 *   - every function returns 0 on success or a negative pny_status; it never throws.
 *     pny_last_error() returns a thread-local message for the last failure.
 *   - *_dev pointers are device (HIP) pointers owned by the caller and borrowed for the call;
 *     *_host pointers are host memory.  All floating point data is fp32, row-major (one exception:
 *     the fp64 results of pny_view_metrics).
 *   - work is enqueued on the caller's stream (hipStream_t passed as void*); the library does
 *     not synchronise except where a function says so.
 *   - a pny_model owns packed weights; a pny_scene owns the per-scene state the reference keeps
 *     in module buffers after encode() (latent, world->cam poses, intrinsics) plus a grow-only
 *     workspace.  One model / scene per device and per caller thread.
 *   - streams: the calls on one scene are ordered by the stream they are enqueued on.  A call that
 *     arrives on a different stream than the previous call on the same scene is ordered behind it by
 *     the library (one event record + stream wait, paid on the switch only), so a scene may migrate
 *     between streams; two streams must not drive the same scene concurrently from two threads.
 *     The previous stream must still exist at the switch or have been destroyed after draining.
 */
#ifndef PNYOLO_H
#define PNYOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNY_ABI_VERSION 11

typedef enum pny_status {
    PNY_OK = 0,
    PNY_ERR_ARG = -1,      /* bad argument / unsupported configuration */
    PNY_ERR_STATE = -2,    /* call order (e.g. render before weights / latent / cameras) */
    PNY_ERR_HIP = -3,      /* HIP runtime error (message carries hipGetErrorString) */
    PNY_ERR_NOGPU = -4,    /* no gfx950 device visible */
    PNY_ERR_RANGE = -5     /* an earlier F16X2 / F16 launch met a value outside the f16 range (pny_model_range_status) */
} pny_status;

typedef struct pny_model pny_model;
typedef struct pny_scene pny_scene;
typedef void* pny_stream; /* hipStream_t */

/* Values the reference reads from conf["model"] (src/model/models.py:21-83,
 * src/model/resnetfc.py:189-205, src/model/code.py:45-52). */
typedef struct pny_model_desc {
    int32_t d_latent;      /* encoder.latent_size: 512 (ResNet34, encoder.py:67) or 1792 (YOLO) */
    int32_t d_hidden;      /* mlp.d_hidden; this build supports 512 */
    int32_t d_out;         /* 4, or 7*num_anchors_per_scale = 21 in YOLO mode (models.py:80-83) */
    int32_t n_blocks;      /* mlp.n_blocks (5) */
    int32_t combine_layer; /* mlp.combine_layer (3): cross-view mean before this block */
    int32_t num_freqs;     /* code.num_freqs (6) */
    float freq_factor;     /* code.freq_factor (1.5) */
    int32_t yolo;          /* mlp_coarse.yolo: raw outputs, extrinsics used as given, z>=0 culling */
    int32_t has_fine;      /* mlp_fine.type != empty */
    int32_t device;        /* HIP device ordinal */
    int32_t enc_use_first_pool; /* encoder.use_first_pool (encoder.py:145-146); 0 in conf/exp/sn64.conf */
} pny_model_desc;

int pny_version(void);
const char* pny_last_error(void);

/* make_model(conf["model"]) -- src/model/__init__.py:4-11, src/model/models.py:16-90 */
int pny_model_create(pny_model** out, const pny_model_desc* desc);
void pny_model_destroy(pny_model* m);

/* PixelNeRFNet.load_weights -> load_state_dict, one call per state_dict tensor
 * (src/model/models.py:320-349).  name is the state_dict key ("mlp_coarse.lin_in.weight",
 * "mlp_fine.blocks.3.fc_1.bias", "encoder.model.layer2.0.downsample.1.running_var", ...);
 * unknown keys (code._freqs, layer4.*, fc.*, num_batches_tracked) are accepted and ignored.
 * data_host: fp32, shape as in the state_dict. */
int pny_model_load_weights(pny_model* m, const char* name, const float* data_host,
                           const int64_t* shape, int ndim);
/* Packs the loaded tensors into the MFMA operand order and uploads them.  Fails with
 * PNY_ERR_STATE and names the first missing MLP tensor.  Synchronous.  May be called again after
 * further pny_model_load_weights calls (weights changed); scenes of the model stay valid. */
int pny_model_finalize(pny_model* m);
/* Training: device-side weight refresh.  pny_model_bind_param tells the library where a state_dict tensor of the MLPs
 * lives on the device (fp32, contiguous, its state_dict shape; borrowed until rebound); after the parameters changed
 * in place (optimizer.step()), pny_model_refresh re-creates every packed operand of both MLPs from those tensors with
 * one kernel launch on `stream` (no host round trip, asynchronous; ordered behind the scenes' earlier calls).
 * The first refresh after a pny_model_bind_param rewrites its table of parameter pointers with a copy on `stream`, ordered
 * behind the previous refresh's launch on whatever stream that ran: a refresh still queued reads the binding it was given.
 * pny_model_finalize must have run once (it fixes the layout).  The inference trunk's folded weights are not refreshed (they
 * follow pny_model_load_weights + finalize); the training trunk (pny_trunk_train_forward) reads its bound parameters directly. */
int pny_model_bind_param(pny_model* m, const char* name, const float* param_dev);
int pny_model_refresh(pny_model* m, pny_stream stream);
/* `net.mlp_fine = None` (reference eval/eval.py:140): with enable=0 the fine pass of pny_render and
 * pny_query(coarse=0) evaluate mlp_coarse.  Default 1 (ignored when the model has no fine MLP). */
int pny_model_use_fine(pny_model* m, int enable);

int pny_scene_create(pny_scene** out, pny_model* m);
void pny_scene_destroy(pny_scene* s);

/* Camera half of PixelNeRFNet.encode (src/model/models.py:115-148).
 * poses_host (ns,4,4): cam->world, inverted here to world->cam [R^T | -R^T t]; in YOLO mode
 * they are world->cam extrinsics and used as given.  focal_host (nf,2), c_host (nc,2) with
 * nf, nc in {1, ns}; fy is negated here in non-YOLO mode as the reference does.
 * Host-only: the cameras are kept in the handle and travel to the device as kernel arguments of each
 * later launch (no device copy, no synchronisation; launches already enqueued keep the cameras they
 * were launched with). */
int pny_scene_set_cameras(pny_scene* s, const float* poses_host, int ns, const float* focal_host, int nf,
                          const float* c_host, int nc, int width, int height);
/* Super-batch in ONE scene (ABI 11).  The reference flattens a super-batch everywhere: NeRFRenderer.forward takes rays
 * (SB, B, 8) and composites (SB * B) rays in one pass (src/render/nerf.py:283-288), PixelNeRFNet.forward conditions object o's
 * points on ITS views out of the (SB * NS) encoded ones (src/model/models.py:160-246, util.repeat_interleave).  With
 * n_objs > 1 the scene's ns views (cameras and latent, object-major) are n_objs objects' view lists of ns / n_objs views each,
 * and every later render / query / backward call splits its rays (points) into n_objs equal consecutive shares, share o seeing
 * views [o * ns / n_objs, (o + 1) * ns / n_objs): one MLP launch per pass covers all objects' tiles.  Every share's sample
 * count (rays x samples per ray, in both passes) must be a multiple of 64 -- PNY_ERR_ARG otherwise, and the caller falls
 * back to one scene per object; the backward of a grouped scene needs the deferred stash (pny_model_defer_weight_grads).
 * ns <= 16 views in total.  n_objs = 1 restores the default. */
int pny_scene_set_groups(pny_scene* s, int n_objs);
/* Encoder bypass: installs a latent (ns, L, Hl, Wl) NCHW as SpatialEncoder.forward would leave
 * it in self.latent (src/model/encoder.py:169-172); repacked to NHWC on device. */
int pny_scene_set_latent(pny_scene* s, const float* latent_dev, int ns, int channels, int hl, int wl,
                         pny_stream stream);
/* The latent of a backbone that hands back a LIST of feature maps (SpatialEncoder.forward with backbone = "custom",
 * src/model/encoder.py:126-137: every map resized to the first map's size by F.interpolate(bilinear, align_corners = True),
 * then torch.cat along the channels).  Level i is fp32 NCHW (n, channels[i], h[i], w[i]) on the device; maps_dev, channels, h
 * and w are HOST arrays of n_levels entries (1 .. PNY_MAX_LATENT_LEVELS).  A level may be smaller than level 0, of its size
 * (then copied bit for bit) or larger; a channel count is any positive number (levels whose count and channel offset are
 * multiples of 4 move as 16-byte words).  Resampling restates ATen's upsample_bilinear2d in float32: scale = (h_i - 1) /
 * (h_0 - 1), 0 when h_0 == 1; src = scale * dst; i0 = (int)src; i1 = i0 + (i0 < h_i - 1); l1 = src - i0; l0 = 1 - l1;
 * l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11).
 * pny_latent_levels: ONE launch writes the channel-last latent (n, h[0], w[0], sum channels), level i at channel offset
 *   channels[0] + .. + channels[i - 1], into the caller's buffer; every element is written.  Needs no model.
 * pny_latent_levels_backward: the adjoint, ONE launch: d_latent (n, h[0], w[0], sum channels) channel-last -> per level its
 *   NCHW gradient (n, channels[i], h[i], w[i]), WRITTEN (not added); a NULL entry of d_maps_dev skips that level.  A gather in a
 *   fixed order of summation, no atomics: the same bits on every run.
 * pny_scene_set_latent_levels: assembles straight into the scene's latent (ns = n views) and leaves the scene as
 *   pny_scene_set_latent does -- same checks (sum channels == d_latent, ns <= 16, Hl Wl L < 2^31), projected maps marked stale --
 *   without an NCHW copy of the latent and without a transpose.
 * None allocates (the scene entry: the scene's latent, as pny_scene_set_latent), copies or waits.  PNY_ERR_ARG, before any
 * launch, with the function's name in pny_last_error(): a NULL pointer (a map included), n_levels outside 1 .. 8, a size, a
 * channel count or n below 1, a level of 2^31 pixels or more. */
#define PNY_MAX_LATENT_LEVELS 8
int pny_latent_levels(const float* const* maps_dev, const int* channels, const int* h, const int* w, int n_levels, int n,
                      float* latent_nhwc_dev, pny_stream stream);
int pny_latent_levels_backward(const float* d_latent_nhwc_dev, float* const* d_maps_dev /* entries may be NULL */, const int* channels,
                               const int* h, const int* w, int n_levels, int n, pny_stream stream);
int pny_scene_set_latent_levels(pny_scene* s, const float* const* maps_dev, const int* channels, const int* h, const int* w,
                                int n_levels, int ns, pny_stream stream);
/* SpatialEncoder.forward, ResNet-34 trunk, eval-mode batch norm (src/model/encoder.py:139-173).
 * images_dev (ns,3,H,W) in [-1,1].  Leaves the 512-channel latent (H/2 x W/2) in the scene. */
int pny_scene_encode(pny_scene* s, const float* images_dev, int ns, int height, int width, pny_stream stream);
/* The same for the n_scenes objects of a super-batch (PixelNeRFNet.encode with images (SB, NS, 3, H, W), src/model/models.py:
 * 92-151, flattens them into ONE encoder call): images_dev (n_scenes * ns, 3, H, W), scene i owns images [i * ns, (i + 1) * ns).
 * One pass of the trunk over all of them (41 launches instead of 41 per scene); every scene must belong to the same model,
 * and all of them are entered on `stream`. */
int pny_scenes_encode(pny_scene** scenes, int n_scenes, const float* images_dev, int ns, int height, int width, pny_stream stream);
/* Copies the scene latent out as (ns, L, Hl, Wl) NCHW (test / debugging aid). */
int pny_scene_get_latent(pny_scene* s, float* latent_dev, pny_stream stream);
int pny_scene_latent_shape(pny_scene* s, int* ns, int* channels, int* hl, int* wl);

/* util.gen_rays (src/util/util.py:240-278, yolo_mode=0: poses cam->world, unit dirs, integer
 * pixel centres) and util.gen_rays_yolo (src/util/util.py:808-876, yolo_mode=1: poses are
 * world->cam extrinsics, K^-1 [x+.49,y+.49,1], not normalised).  out_dev (b,H,W,8). */
int pny_gen_rays(const float* poses_host, int b, int width, int height, const float focal[2],
                 const float c[2], float z_near, float z_far, int yolo_mode, float* out_dev,
                 pny_stream stream);
/* The same for rays [first_ray, first_ray + n_rays) of the flattened (b, H, W) pixel grid only:
 * out_dev (n_rays, 8), 16-byte aligned.  This is how a rank of a ray-sharded render produces its own
 * slice of a frame on its own device (no scatter of rays).  Asynchronous; the camera
 * blocks travel as kernel arguments (no device allocation, no copy, no synchronisation). */
int pny_gen_rays_range(const float* poses_host, int b, int width, int height, const float focal[2],
                       const float c[2], float z_near, float z_far, int yolo_mode, int64_t first_ray,
                       int64_t n_rays, float* out_dev, pny_stream stream);

/* The ray batch of one training step and its ground truth, for all SB objects in ONE launch: what
 * PixelNerfTrainer.calc_losses prepares per object (train/trainlib/PixelNerfTrainer.py:76-123: util.gen_rays of every
 * pixel of every view, an NHWC copy of images * 0.5 + 0.5, CPU pixel indices from torch.randint :112 or util.bbox_sample
 * src/util/util.py:222-237, two gathers), computed for the n_rays pixels per object it keeps.  Model-free, like
 * pny_gen_rays, whose ray arithmetic it shares: a sampled ray has the bits of that pixel's row of pny_gen_rays. */
typedef struct pny_train_batch_desc {
    int32_t n_objs;      /* SB */
    int32_t n_views;     /* NV views per object */
    int32_t height;
    int32_t width;
    int32_t n_rays;      /* B = ray_batch_size, per object */
    float z_near;
    float z_far;
    int32_t focal_rows;  /* focal_dev is (focal_rows, focal_cols): rows 1 (all objects) or SB (per object), */
    int32_t focal_cols;  /* cols 1 (fx = fy) or 2 (fx, fy) */
    int32_t c_rows;      /* c_dev is (c_rows, 2): 1 or SB; ignored when c_dev is NULL */
    uint64_t seed;       /* seeded mode (draws == NULL): Philox key */
    uint64_t draw_offset; /* seeded mode: ray r of object s uses draw index draw_offset + s * B + r, so object s of a call
                          * equals object 0 of a one-object call with draw_offset = s * B */
} pny_train_batch_desc;
/* Replay mode: the caller's draws, (SB, B) each, on the device.  Uniform mode reads pix_inds_dev (flat index into
 * (NV, H, W)); bbox mode reads image_ids_dev and u_x_dev, u_y_dev in [0, 1).  The ones the mode reads must be non-NULL.
 * Values outside their range are clamped to it (memory safety; the call cannot look at them without waiting). */
typedef struct pny_train_batch_draws {
    const int64_t* pix_inds_dev;
    const int64_t* image_ids_dev;
    const float* u_x_dev;
    const float* u_y_dev;
} pny_train_batch_draws;
/* images_dev (SB, NV, 3, H, W) in [-1, 1]; poses_dev (SB, NV, 4, 4) cam->world; focal_dev, c_dev as the descriptor says
 * (c_dev NULL: (W / 2, H / 2)); bboxes_dev (SB, NV, 4) `cmin rmin cmax rmax`, NULL = uniform over all pixels of all views.
 * bbox mode: view ~ U{0..NV-1}, x = trunc(u_x * (cmax + 1 - cmin) + cmin), y likewise from rows, in fp32 without fused
 * multiply-add, then clamped into the image (never reached by a box inside it).  draws NULL = seeded: integers are
 * (uint64) w * n >> 32 of one 32-bit Philox word (bias <= n / 2^32; NV * H * W < 2^32 is required), u_x / u_y 24-bit
 * uniforms, on four streams of their own.  Writes rays_dev (SB, B, 8) 16-byte aligned, rgb_gt_dev (SB, B, 3) =
 * images * 0.5 + 0.5 and, unless NULL, pix_dev (SB, B, 3) int32 [view, y, x].  All device pointers; one kernel enqueued on
 * `stream`, no allocation, no copy, no synchronisation.  PNY_ERR_ARG on a bad shape or a NULL required pointer. */
int pny_sample_train_batch(const pny_train_batch_desc* desc, const float* images_dev, const float* poses_dev,
                           const float* focal_dev, const float* c_dev, const float* bboxes_dev,
                           const pny_train_batch_draws* draws, float* rays_dev, float* rgb_gt_dev, int32_t* pix_dev,
                           pny_stream stream);

/* The rays and target cells of one YOLO training step for ONE object, over all scales and selected views, in ONE launch:
 * what YoloTrainer.calc_losses prepares per scale (train/trainlib/YoloTrainer.py:93-129: NV host->device copies of the
 * target grids, stack, util.gen_rays_yolo src/util/util.py:808-876 of the selected views at the scale's grid size, two
 * indexings by image_ord, two reshapes).  The reference's loop does not index the targets per object (:83), so one object
 * per call is the contract; a caller with several objects calls once per object.  Model-free, like pny_gen_rays, whose
 * yolo_mode = 1 arithmetic it shares: a ray of scale s has the bits of the same pixel of
 * pny_gen_rays_range(poses[view], 1, Ws, Hs, focal / cell, c / cell, ..., yolo_mode = 1). */
#define PNY_YOLO_BATCH_MAX_VIEWS 16
#define PNY_YOLO_BATCH_MAX_SCALES 4
typedef struct pny_yolo_batch_desc {
    int32_t n_views_all;   /* NV: views the object has (rows of poses_host, first dimension of every target grid) */
    int32_t n_views;       /* NS: selected views, 1 .. PNY_YOLO_BATCH_MAX_VIEWS */
    int32_t height;        /* full-resolution image */
    int32_t width;
    int32_t n_scales;      /* 1 .. PNY_YOLO_BATCH_MAX_SCALES */
    int32_t cell_sizes[PNY_YOLO_BATCH_MAX_SCALES]; /* scale s is the grid of Hs = height / cell, Ws = width / cell (integer division) */
    int32_t n_anchors;     /* A = num_anchors_per_scale, 1 .. 64 */
    float z_near;
    float z_far;
} pny_yolo_batch_desc;
/* poses_host (NV, 4, 4): world->cam extrinsics, as pny_gen_rays takes them with yolo_mode = 1.  view_ids_host (NS): the
 * object's row of image_ord -- any order, repeats allowed; an id outside [0, NV) is PNY_ERR_ARG.  focal[2], c[2]: the
 * full-resolution intrinsics; each scale's focal / cell and c / cell are formed in fp32 (an IEEE division, what the
 * reference's tensor division gives; for a power-of-two cell also what a multiplication by 1 / cell gives).
 * targets_dev[n_scales]: device pointers to the (NV, Hs, Ws, A, 6) fp32 target grids.
 * Writes rays_dev (R, 8), 16-byte aligned, and targets_out_dev (R, A, 6), R = NS * sum_s Hs Ws: scale s occupies rows
 * [off[s], off[s + 1]), inside a scale the rows are ordered (position in view_ids, y, x) -- the reference's reshape(-1, 8) /
 * reshape(-1, A, 6).  offsets_host (n_scales + 1 int64, host) receives off.  One kernel enqueued on `stream` (the selected
 * cameras and the scales' intrinsics travel as kernel arguments); no allocation, no copy, no synchronisation.
 * With rays_dev and targets_out_dev both NULL the call only fills offsets_host from the descriptor (how a caller sizes the
 * two buffers): the other pointers are not looked at and nothing is launched.
 * PNY_ERR_ARG before anything is launched: n_scales outside 1 .. 4, NS outside 1 .. 16 (the call never launches twice), A outside 1 .. 64, a cell
 * below 1 or larger than the image, a NULL pointer, an unaligned rays_dev, a singular pose, a zero focal length. */
int pny_yolo_train_batch(const pny_yolo_batch_desc* desc, const float* poses_host, const int64_t* view_ids_host,
                         const float focal[2], const float c[2], const float* const* targets_dev, float* rays_dev,
                         float* targets_out_dev, int64_t* offsets_host, pny_stream stream);

/* PixelNeRFNet.forward for one scene (src/model/models.py:153-318):
 * xyz_dev, viewdirs_dev (n,3) world space -> out_dev (n,d_out) = [sigmoid rgb, relu sigma]
 * (YOLO mode: raw).  coarse=0 selects mlp_fine when the model has one. */
int pny_query(pny_scene* s, const float* xyz_dev, const float* viewdirs_dev, int64_t n, int coarse,
              float* out_dev, pny_stream stream);

/* NeRFRenderer options (src/render/nerf.py:68-102, from_conf :346-358). */
typedef struct pny_render_opts {
    int32_t n_coarse;
    int32_t n_fine;        /* total fine samples incl. depth samples; 0 = coarse only */
    int32_t n_fine_depth;
    float depth_std;
    int32_t white_bkgd;
    int32_t lindisp;
    /* The renderer's random draws (nerf.py:117,141,147,164) are inputs of the path.  Either all
     * needed pointers are given (parity mode), or they are NULL and an in-kernel Philox stream
     * keyed by `seed` generates them (perf mode). */
    const float* u_coarse_dev; /* (n, n_coarse) U[0,1) */
    const float* u_fine_dev;   /* (n, n_fine-n_fine_depth) U[0,1): inverse-cdf draw */
    const float* u_fine2_dev;  /* (n, n_fine-n_fine_depth) U[0,1): in-bin jitter */
    const float* g_depth_dev;  /* (n, n_fine_depth) N(0,1) */
    uint64_t seed;
    /* Training only (src/render/nerf.py:231-232: sigmas + randn_like(sigmas) * noise_std): the noise ADDED to sigma before
     * the composite's relu, already scaled by noise_std; (n, n_coarse) and (n, n_coarse+n_fine), or NULL (no noise). */
    const float* sigma_noise_coarse_dev;
    const float* sigma_noise_fine_dev;
} pny_render_opts;

/* Any output pointer may be NULL. */
typedef struct pny_render_out {
    float* rgb_coarse;     /* (n,3) */
    float* depth_coarse;   /* (n) */
    float* weights_coarse; /* (n,n_coarse) */
    float* rgb_fine;       /* (n,3) */
    float* depth_fine;     /* (n) */
    float* weights_fine;   /* (n,n_coarse+n_fine) */
    float* z_coarse;       /* (n,n_coarse) */
    float* z_fine;         /* (n,n_coarse+n_fine) sorted */
    float* sample_coarse;  /* (n,n_coarse,4) per-sample [rgb, sigma] from the coarse MLP */
    float* sample_fine;    /* (n,n_coarse+n_fine,4) */
} pny_render_out;

/* NeRFRenderer.forward for one scene (src/render/nerf.py:257-309): rays_dev (n,8) =
 * [origin, dir, near, far], 16-byte aligned (rows are read as two 16-byte words; PNY_ERR_ARG otherwise). */
int pny_render(pny_scene* s, const float* rays_dev, int64_t n, const pny_render_opts* opts,
               const pny_render_out* out, pny_stream stream);

/* YoloRenderer.forward (src/render/yolo.py:37-114): coarse sampling only, raw (A*7)-vectors, rays_dev 16-byte aligned,
 * out_dev (n, A, 7) = [max_k p, sum_k p v / (sum_k p + 1e-5)].  raw_dev (n,K,A*7) optional. */
int pny_yolo_render(pny_scene* s, const float* rays_dev, int64_t n, int n_coarse, const float* u_coarse_dev,
                    uint64_t seed, float* out_dev, float* raw_dev, pny_stream stream);

/* Stage entry points (used by the renderer above; exported for stage-wise parity tests). */
/* NeRFRenderer.sample_coarse, src/render/nerf.py:104-121 */
int pny_sample_coarse(const float* rays_dev, int64_t n, int n_coarse, int lindisp, const float* u_dev,
                      uint64_t seed, float* z_dev, pny_stream stream);
/* NeRFRenderer.composite arithmetic, src/render/nerf.py:184-188,229-250.  sample_dev (n,K,4). */
int pny_composite(const float* rays_dev, const float* z_dev, const float* sample_dev, int64_t n, int k,
                  int white_bkgd, float* weights_dev, float* rgb_dev, float* depth_dev, pny_stream stream);
/* sample_fine + sample_fine_depth + cat + sort, src/render/nerf.py:126-167,291-301.
 * z_out_dev (n, n_coarse+n_fine) ascending. */
int pny_sample_fine(const float* rays_dev, const float* z_coarse_dev, const float* weights_dev,
                    const float* depth_dev, int64_t n, int n_coarse, int n_fine, int n_fine_depth,
                    float depth_std, int lindisp, const float* u_dev, const float* u2_dev,
                    const float* g_dev, uint64_t seed, float* z_out_dev, pny_stream stream);
/* YoloRenderer aggregation, src/render/yolo.py:96-114.  raw_dev (n,K,A*7) -> out_dev (n,A,7). */
int pny_yolo_aggregate(const float* raw_dev, int64_t n, int k, int n_anchors, float* out_dev,
                       pny_stream stream);

/* ---- YOLO detection tail (callers: train/trainlib/YoloTrainer.py:283-286,347) ----
 * Boxes are rows of 6 floats [class, score, x, y, w, h] as the reference's lists hold them. */
/* util.convert_cells_to_bboxes for one image (src/util/util.py:633-689): cells_dev (h,w,a,7) raw
 * predictions (is_predictions=1: sigmoid xy, exp(wh)*anchor, argmax class) or (h,w,a,6) targets;
 * anchors_host (a,2), a <= 4; boxes_dev (h*w*a, 6) in (y, x, anchor) order. */
int pny_cells_to_bboxes(const float* cells_dev, const float* anchors_host, int h, int w, int n_anchors,
                        int is_predictions, float* boxes_dev, pny_stream stream);
/* util.nms (src/util/util.py:691-722), n <= 8192, including the reference's remove-while-iterating
 * behaviour.  kept_dev (n,6): survivors in output order; meta_dev[0] = survivors, meta_dev[1] = boxes
 * above `threshold`; highest_conf_dev[0] = max score of all inputs (-inf when n == 0). */
int pny_nms(const float* boxes_dev, int n, double iou_threshold, double threshold, float* kept_dev, int* meta_dev,
            float* highest_conf_dev, pny_stream stream);
/* util.calculate_tp_fp_fn (src/util/util.py:765-802): nms on both lists, then IoU matching.
 * out_dev: int[3] = tp, fp, fn. */
int pny_tp_fp_fn(const float* target_boxes_dev, int nt, const float* pred_boxes_dev, int np, double nms_iou,
                 double nms_threshold, double match_iou, int* out_dev, pny_stream stream);

/* The detection scores of ALL views of a YOLO metric pass in ONE launch: what YoloTrainer.metric_step
 * (train/trainlib/YoloTrainer.py:338-354, driven by eval/eval_yolo.py) does per destination view -- the cells of every scale
 * turned into Python lists (:283-289, util.convert_cells_to_bboxes src/util/util.py:633-689), util.calculate_tp_fp_fn on the two
 * lists (:348; util.py:765-802 with nms :691-722 and iou :575-611) and the running sums of tp, fp, fn (:349-351) -- without a
 * launch chain and a device -> host read per view.  One 256-thread workgroup per view (grid = n_views) runs, for the target list
 * and then for the prediction list, in the same LDS: decode + the confidence and size filters + order-preserving compaction of
 * the survivors ("candidates"), the stable descending sort by confidence, the greedy suppression with the reference's list
 * semantics (exactly pny_nms'), then the matching of pny_tp_fp_fn, the view's record, and integer atomic adds into the totals.
 * The box decode and the IoU are the device code of pny_cells_to_bboxes / pny_nms / pny_tp_fp_fn (csrc/pny_detect.h), so every
 * count equals the per-view path's; all results are integers or copied floats: the same bits on every run.
 * One kernel enqueued on `stream`; no allocation, no copy, no synchronisation; anchors_host is read before the call returns.
 *
 * Input forms (desc->form):
 *   PNY_DETECT_CELLS  preds_dev[s] (n_views * Hs * Ws, n_anchors, 7) and targets_dev[s] (n_views * Hs * Ws, n_anchors, 6) for each
 *     scale s, Hs = height / cell_sizes[s], Ws = width / cell_sizes[s] (integer division), rows ordered (view, y, x): what
 *     pny_yolo_train_batch and pny_yolo_render give.  A view's list is its cells of scale 0, 1, ... in that order and, within a
 *     scale, in the (y, x, anchor) order of pny_cells_to_bboxes.  anchors_host (n_scales * n_anchors, 2).  The row pointers and
 *     offsets are not looked at.
 *   PNY_DETECT_BOXES  already decoded rows [class, score, x, y, w, h]: pred_rows_dev (n_pred_rows, 6) with pred_offsets_dev
 *     (n_views + 1 int32, on the device): view v owns rows [offsets[v], offsets[v + 1]); targets the same.  No decode.  The
 *     per-scale pointers, anchors_host and the geometry fields are not looked at.  The kernel checks every segment against
 *     0 <= offsets[v] <= offsets[v + 1] <= n_rows; a view whose segment fails has status PNY_DETECT_BAD_SEGMENT.
 *
 * Limit: a view may hold any number of cells or rows, but at most PNY_DETECT_MAX_CANDIDATES of one list of one view may pass the
 * filters (53 bytes of LDS each: 106 KB of gfx950's 160 KB at the limit; the real geometry, 30 x 16 + 15 x 8 + 7 x 4 cells x 3
 * anchors = 1884 boxes, fits whatever passes).  A view above it is NOT truncated: its status is non-zero, its tp, fp, fn and
 * kept counts are 0, it adds nothing to totals[0..2] and 1 to totals[3].
 *
 * Outputs:
 *   per_view_dev (n_views, 8) int32: tp, fp, fn, kept targets, kept predictions, targets above nms_threshold, predictions above
 *     nms_threshold (the third result of util.nms: counted before the size filter), status (0, or PNY_DETECT_* bits);
 *   highest_conf_dev (n_views, 2): the highest score over ALL boxes of the target and of the prediction list (-inf if empty);
 *   totals_dev 4 x int64: tp, fp, fn, failed views.  The call ADDS to them; the caller zeroes them before a pass;
 *   kept_targets_dev, kept_preds_dev: NULL or (n_views, max_kept, 6), the first max_kept survivors of each view in the
 *     reference's output order (the counts in the record are the full ones; rows past a view's count are left as they are).
 * PNY_ERR_ARG, before any launch, pny_last_error naming the field: a NULL desc or required pointer, an unknown form, n_views
 * below 1, n_scales outside 1 .. PNY_YOLO_BATCH_MAX_SCALES, n_anchors outside 1 .. 4 (the limit of pny_cells_to_bboxes), a cell
 * size below 1 or above the image, a view of 2^31 or more cells, negative row counts, a negative max_kept or one of 0 with a kept
 * pointer, non-finite thresholds. */
#define PNY_DETECT_MAX_CANDIDATES 2048
enum { PNY_DETECT_CELLS = 0, PNY_DETECT_BOXES = 1 };
enum { PNY_DETECT_TARGETS_OVERFLOW = 1, PNY_DETECT_PREDS_OVERFLOW = 2, PNY_DETECT_BAD_SEGMENT = 4 };   /* status bits */
#define PNY_DETECT_RECORD 8
typedef struct pny_detect_views_desc {
    int32_t form;          /* PNY_DETECT_CELLS or PNY_DETECT_BOXES */
    int32_t n_views;
    int32_t n_scales;      /* cells form: 1 .. PNY_YOLO_BATCH_MAX_SCALES */
    int32_t height;        /* cells form: the full-resolution image, as pny_yolo_batch_desc */
    int32_t width;
    int32_t cell_sizes[PNY_YOLO_BATCH_MAX_SCALES];
    int32_t n_anchors;     /* cells form: A per scale, 1 .. 4 */
    int32_t n_pred_rows;   /* boxes form: rows of pred_rows_dev */
    int32_t n_target_rows; /* boxes form: rows of target_rows_dev */
    int32_t max_kept;      /* rows per view of kept_targets_dev / kept_preds_dev */
    double nms_iou;        /* util.nms iou_threshold (compared in fp32, strictly) */
    double nms_threshold;  /* util.nms threshold (compared in double, strictly) */
    double match_iou;      /* calculate_tp_fp_fn's IoU (fp32; best > match_iou is a tp, best < match_iou a fn) */
} pny_detect_views_desc;
int pny_detect_views(const pny_detect_views_desc* desc, const float* const* preds_dev, const float* const* targets_dev,
                     const float* anchors_host, const float* pred_rows_dev, const int32_t* pred_offsets_dev,
                     const float* target_rows_dev, const int32_t* target_offsets_dev, int32_t* per_view_dev,
                     float* highest_conf_dev, int64_t* totals_dev, float* kept_targets_dev, float* kept_preds_dev,
                     pny_stream stream);

/* The three thresholds of a YOLO metric pass SWEPT in ONE launch: the integers of pny_detect_views at every setting of a grid
 * NMS IoU x confidence cut x match IoU, on a render that is made once.  The reference has one setting per pass:
 * YoloTrainer.metric_step (train/trainlib/YoloTrainer.py:338-354) scores at the config's nms_iou_threshold, nms_threshold and
 * match_iou_threshold, eval/eval_yolo.py runs the test loader again for another setting, and eval/gen_images_yolo.py:110-117 asks
 * for nms_threshold and nms_iou_threshold on stdin and encodes and renders again for every answer.  util.nms (src/util/util.py:691-722)
 * removes rows from the list it iterates over, so the kept lists at one (cut, NMS IoU) do not follow from those at another: one
 * 256-thread workgroup per (view, NMS IoU i, cut t) -- grid = n_views * n_nms_ious * n_conf_cuts -- runs the device code of
 * pny_detect_views for its view at its two values (csrc/pny_detect_views_core.h: one copy), in the same LDS map.  The match IoU
 * enters util.calculate_tp_fp_fn (util.py:765-802; the whole tail is util.py:691-797) only through the last comparison: the best
 * IoU of every kept prediction over the kept targets, and of every kept target over the kept predictions, is computed once
 * (util.py:776-797) and compared with all n_match_ious values: tp = predictions with best > m, fp = kept predictions - tp,
 * fn = targets with best < m; without a kept target (0, kept predictions, 0), without a kept prediction (0, 0, kept targets).
 * Setting (i, t, m) gives the integers pny_detect_views gives at nms_iou = nms_ious_host[i], nms_threshold = conf_cuts_host[t],
 * match_iou = match_ious_host[m]: cuts are compared in double, the IoUs rounded to fp32 once on the host, as there.
 * One kernel enqueued on `stream`; the thresholds travel by value in its arguments: no allocation, no copy, no
 * synchronisation; anchors_host and the three threshold arrays are read before the call returns.
 *
 * desc and the eight input pointers: as pny_detect_views, with the same checks.  desc->nms_iou, nms_threshold and match_iou are
 * ignored; desc->max_kept must be 0 (a sweep keeps no boxes: pny_detect_views at the chosen setting gives them).
 * Limits: 1 <= n_nms_ious <= 8, 1 <= n_conf_cuts <= 32, 1 <= n_match_ious <= 8, every value finite; order and duplicates are the
 * caller's.  Outputs, in C order:
 *   counts_dev (n_views, n_nms_ious, n_conf_cuts, n_match_ious, 3) int32: tp, fp, fn;
 *   lists_dev  (n_views, n_nms_ious, n_conf_cuts, 3) int32: kept targets, kept predictions, status (0, or PNY_DETECT_* bits);
 *   totals_dev (n_nms_ious, n_conf_cuts, n_match_ious, 4) int64: tp, fp, fn, refused views.  The call ADDS to them.
 * A (view, setting) is refused when more than PNY_DETECT_MAX_CANDIDATES boxes of one of its lists pass the filters at that cut,
 * or when the view's segment is bad: never truncated, its counts and kept counts are 0, it adds nothing to tp, fp, fn and 1 to
 * the refused word of every m of its (i, t).  The same view may be scored at a higher cut.
 * PNY_ERR_ARG, before any launch, pny_last_error naming the argument: what pny_detect_views refuses, a NULL output or threshold
 * array, a count outside its limits, a value that is not finite, max_kept != 0, 2^31 or more workgroups. */
int pny_detect_sweep(const pny_detect_views_desc* desc, const float* const* preds_dev, const float* const* targets_dev,
                     const float* anchors_host, const float* pred_rows_dev, const int32_t* pred_offsets_dev,
                     const float* target_rows_dev, const int32_t* target_offsets_dev, const double* nms_ious_host,
                     int32_t n_nms_ious, const double* conf_cuts_host, int32_t n_conf_cuts, const double* match_ious_host,
                     int32_t n_match_ious, int32_t* counts_dev, int32_t* lists_dev, int64_t* totals_dev, pny_stream stream);

/* Latent projection.  `x = x + lin_z[b](z)` (src/model/resnetfc.py:176-182) with z the bilinear
 * interpolation of the latent (src/model/encoder.py:101) is linear in the latent, so
 * lin_z[b](interp(latent)) == interp(lin_z[b](latent)) up to fp32 rounding: with projection ON the
 * library applies lin_z[b] to every latent PIXEL once per scene (cached until the latent or the
 * weights change) and the fused kernel interpolates the projected maps instead of running the lin_z
 * GEMMs per (sample, view).  Results stay inside the 1e-4 parity tolerance (tests/test_gpu_parity.py);
 * OFF executes the reference's operation order.  AUTO (default; env PNYOLO_PROJECTION=off|on
 * overrides at scene creation) projects every launch when the scene can use the F16X2 kernel (below), so that a ray's
 * result does not depend on the size of its batch; otherwise when a launch has >= 2x as many points as the latent has
 * pixels per view. */
#define PNY_PROJECTION_OFF 0
#define PNY_PROJECTION_ON 1
#define PNY_PROJECTION_AUTO 2
int pny_scene_set_projection(pny_scene* s, int mode);
/* Compute the projected maps now (coarse, and fine when the model has one) instead of lazily inside
 * the first large launch; a no-op when they are current.  Error when the mode is OFF. */
int pny_scene_project(pny_scene* s, pny_stream stream);
/* Read-out of the projection (exported for stage-wise tests; nothing in the library calls it).  Projects the scene's latent
 * with the coarse (fine = 0) or fine (fine != 0; the coarse one on a model without a fine MLP) MLP's stacked lin_z weights
 * into out_dev, (ns * hl * wl, view blocks * 512) row-major: out[p][512 b + n] = sum_k lin_z[b].weight[n][k] latent[v][k][y][x],
 * p = (v * hl + y) * wl + x, no bias.  It runs the function the cached maps are computed by, in the arithmetic they would
 * have on this scene now (pny_scene_set_precision), but neither reads nor fills nor invalidates the cache, whatever the
 * projection mode.  route (optional): the kernel that ran, PNY_PROJECTION_ROUTE_TILED_F32 / _TILED_F16X2 for the tiled GEMM
 * (maps of at least 256 pixels), else the 1x1-convolution path's instantiation, 100 SPLIT + 10 NT + MT as pny_trunk_conv
 * reports it (>= 111).  PNY_ERR_ARG: out_floats below the size above, a model without per-view blocks; PNY_ERR_STATE: no
 * finalized weights, no latent.  Asynchronous on `stream`. */
#define PNY_PROJECTION_ROUTE_TILED_F32 1
#define PNY_PROJECTION_ROUTE_TILED_F16X2 2
int pny_scene_projection(pny_scene* s, int fine, float* out_dev, int64_t out_floats, int* route, pny_stream stream);

/* Matrix arithmetic of PROJECTED launches.  F32: v_mfma_f32_32x32x2_f32 on fp32 operands.  F16X2: every fp32 operand
 * is split into two f16 planes, x = f16(x) + f16(x - f16(x)) (22 significant bits; the second plane may be denormal,
 * which the matrix cores honour), and a product is x1 w1 + x2 w1 + x1 w2 on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation: the same measured error against fp64 as the fp32 matrix path (tools/ubench/split_f16_check.hip,
 * 1.7e-6 vs 1.8e-6 at K = 512 on the network's magnitudes) at 5.3x its matrix rate; held to the same 1e-4 bar by the
 * same golden vectors.  The 22 bits hold for operands of ordinary magnitude only: an f16 denormal has the fixed spacing 2^-24, so the
 * second plane of a value below 2^-14 * 2^11 = 0.125 already keeps fewer than its 11 bits, and what two planes leave behind is up to
 * 2^-25 ABSOLUTE whatever the value.  Measured on the latent projection (K = 128 .. 1792, error over the map's max against
 * fp64, tests/projection_ref.py): with both operands -- latent and lin_z weights -- of standard deviation 0.05 or
 * more (up to 1e3, the largest tried) the split product stays within 2 x the error of an fp32 matmul (it is within 1.5 x); it
 * leaves that band between 0.02 (K = 128) and 0.005 (K = 1792), and below it the error is 1.7e-8 / s of the map's max for an
 * operand of standard deviation s: 1.7e-5 at 1e-3, 1.6e-4 at 1e-4, where fp32 stays at 5e-7 .. 2e-6.  A flush of f16 denormals
 * would cost 2e-4 .. 3e-4 at every magnitude; tests/test_gpu_projection.py holds the kernels a factor 50 or more below that.  Values beyond the f16 range (|x| > 65504 in an activation or weight) are NOT representable: use
 * F32 for such models (AUTO does so by itself when a WEIGHT loaded at pny_model_finalize is outside the range; weights changed
 * through pny_model_refresh and activations are not checked).  AUTO (default; env PNYOLO_MLP_PRECISION=f32|f16x2|f16 overrides at scene creation) otherwise
 * equals F16X2: every projected launch, whatever its size, so that a ray's result does not depend on the batch it is rendered
 * in.  Launches without projection (training forward, the reference operation order, batches below the projection
 * threshold) always run F32; models with more than 6 residual blocks or combine_layer = 0 always run F32.
 * The setting also selects the arithmetic of the latent projection and of the BACKWARD pass (pny_render_backward,
 * pny_query_backward, pny_yolo_render_backward, pny_model_flush_weight_grads): scenes not pinned to F32 run the dX chain and
 * the weight-gradient GEMMs as split-f16 products with power-of-two gradient scaling (csrc/mlp_bwd_h2.hip,
 * pny_dw_gemm_h2_kernel); a deferred flush runs fp32 when any contributing scene was pinned to F32.  Env
 * PNYOLO_BWD_PRECISION=f32|f16x2 overrides the backward's choice (read at every call).  The forward's fp32 fallbacks for more
 * than 6 residual blocks and for combine_layer = 0 do NOT apply to the backward: its kernels loop over any block count, so it
 * follows the scene's setting (and the override) for every model, and runs fp32 only when a weight is outside the f16 range.
 * Operation order: the no-grad launches of the F16X2 kernel run the fc_1 of the last per-view block ONCE per sample, on the mean
 * over views of relu(net + b_fc0) -- mean_v(h_v + fc_1(R_v)) = mean_v(h_v) + fc_1(mean_v R_v), exact in real arithmetic, one
 * fp32 sum per sample reordered in fp32, a single view bit for bit as before (csrc/mlp_h2.hip).  F32 launches,
 * the single-plane kernel of F16 / F16_TRAIN and every training forward keep the reference's per-view order. */
#define PNY_PRECISION_F32 0
#define PNY_PRECISION_F16X2 1
#define PNY_PRECISION_AUTO 2
/* F16 (opt-in, outside the 1e-4 parity claim): the no-grad projected forward launches of the scene -- pny_render, pny_query,
 * pny_yolo_render, coarse and fine MLP, single and grouped scenes -- run on the f16 matrix cores with ONE f16 plane per operand
 * (round to nearest) and fp32 accumulation: one v_mfma_f32_32x32x16_f16 per product instead of three and 2 bytes per weight
 * instead of 4 (csrc/mlp_h1.hip, one 64-sample tile shape for every launch size, so a ray's result still does not depend on
 * the batch it is rendered in).  Measured on MI355X: 1.84x the F16X2 kernel's speed on the C2 frame
 * (MLP kernel 42.8 vs 78.7 ms); max |error| 2.8e-3 on RGB / sigma against the reference's goldens, 77 dB PSNR against
 * an F32 render.  Everything else
 * on an F16 scene behaves exactly as AUTO: the training forward (stash) and every backward (gradients are bit-identical to an
 * AUTO scene's), the latent projection, and the fallbacks to fp32 (more than 6 blocks, combine_layer = 0, weights outside
 * the f16 range at finalize, unprojected launches).  The single-plane weight images are built when a scene of the model is
 * first set to F16 (a device synchronisation) and from then on kept current by pny_model_finalize / pny_model_refresh;
 * models without F16 scenes hold none.  The range guard below applies as for F16X2 (the plane has the range of F16X2's
 * first plane).  Env PNYOLO_MLP_PRECISION=f16 selects it at scene creation. */
#define PNY_PRECISION_F16 3
/* F16_TRAIN (opt-in, outside the 1e-4 parity claim): mixed-precision training -- F16 for the forward AND the backward.  No-grad
 * projected forwards run exactly as on an F16 scene (the same kernel, bit-identical results).  The training forward
 * (pny_scene_stash_next_render) runs the single-plane kernel's STASH instantiation and writes its own fp32 values to the
 * unchanged stash; the dX chain (csrc/mlp_bwd_h1.hip), the weight-gradient GEMMs (pny_dw_gemm_h1_kernel) and the latent
 * gradient (latent_grad_h1_kernel) multiply ONE f16 plane per operand with fp32 accumulation, in the same power-of-two scaled
 * gradient domains as F16X2 (per tile in the chain, per launch in the GEMMs): gradients stay deterministic and scale exactly
 * with the loss; parameters, gradients and optimizer state stay fp32.  The fp32 fallbacks of AUTO apply unchanged, and
 * PNYOLO_BWD_PRECISION=f32|f16x2 still overrides the backward.  A deferred flush (pny_model_flush_weight_grads) runs
 * single-plane only when every contributing scene ran the F16_TRAIN backward; with an F32 contributor it runs fp32,
 * otherwise split-f16.  The transposed single-plane images the chain needs (plane 0 of the split transposed images) are built
 * when a scene of the model is first set to F16_TRAIN and kept current like F16's.  The range guard applies as for F16X2:
 * training calls fail with PNY_ERR_RANGE.  When the stash reservation is missed, the backward recomputes the forward with the
 * fp32 stash kernel, as under AUTO.  Measured errors and speed: DESIGN.md 4.7.  Env PNYOLO_MLP_PRECISION=f16_train
 * selects it at scene creation.  (4 is not used: it stays an invalid mode, as it was before F16_TRAIN.) */
#define PNY_PRECISION_F16_TRAIN 5
int pny_scene_set_precision(pny_scene* s, int mode);
/* The kernel family of the last MLP launch of the scene: 0 fp32, 1 the F16X2 (split-f16) kernel, 2 the F16 (single-plane)
 * kernel.  Non-zero = an f16-family kernel ran and the range guard applies. */
int pny_scene_last_precision(pny_scene* s, int* f16x2);
/* The same codes for the dX chain of the last backward of the scene (or grouped scene): 0 fp32, 1 split-f16, 2 single-plane
 * (F16_TRAIN).  The weight-gradient GEMMs of an immediate backward run the same arithmetic; a deferred flush decides at
 * pny_model_flush_weight_grads (see F16_TRAIN above).  0 before any backward. */
int pny_scene_last_backward_precision(pny_scene* s, int* code);

/* Run-time guard of the F16X2 (and F16) arithmetic's range.  The split operands are f16 planes: a value of magnitude >= 65520 (or an
 * infinity) has no f16 representation, and a launch that meets one returns garbage where the reference -- fp32 throughout,
 * src/model/resnetfc.py:134-186; it only prints when its output holds a NaN, src/model/models.py:174-270 -- still returns
 * numbers.  Every F16X2 kernel therefore reports what it meets into one word per model that the host can read at any time
 * (pinned host memory, written with a system-scope atomic OR by the lanes that saw the value):
 *   PNY_RANGE_ACTIVATION  forward (render / query / training forward): a relu output or a lin_in input left the range;
 *   PNY_RANGE_GRADIENT    backward: the running max |dY| of a chain / weight-gradient launch is not finite (the chain works
 *                         in a per-tile scaled domain with 2^11 of headroom, csrc/mlp_bwd_h2.hip);
 *   PNY_RANGE_WEIGHT      pny_model_refresh repacked a weight of magnitude > 65504 or a NaN (pny_model_finalize checks on the
 *                         host and keeps AUTO on F32 by itself; a refresh runs on the device, after the launch decision).
 * pny_model_range_status returns the bits seen so far (`bits`, may be NULL) and, with clear != 0, resets them.  It does not
 * synchronise: the bits of a launch are complete once that launch has finished (synchronise its stream first).
 * While bits are set, every scene-level entry point (render, query, encode, backward ...) of the model fails with
 * PNY_ERR_RANGE -- results computed since the overflow are not to be trusted -- until they are cleared; PNY_RANGE_WEIGHT also
 * drops AUTO scenes to F32 until the next pny_model_finalize.  Recovery: clear, pny_scene_set_precision(F32), repeat the call
 * (pixel-nerf-yolo_amd/model.py does this transparently for no-grad calls: `f16_range_policy`). */
#define PNY_RANGE_ACTIVATION 1u
#define PNY_RANGE_GRADIENT 2u
#define PNY_RANGE_WEIGHT 4u
int pny_model_range_status(pny_model* m, unsigned* bits, int clear);

/* The ResNet-34 trunk in TRAINING mode (reference src/model/encoder.py:139-173 under autograd with the encoder unfrozen, the
 * default of train/train.py:66-73; batch norm on batch statistics as nn.BatchNorm2d in train()): forward and backward as this
 * library's kernels (csrc/encoder_train.hip).  Parameters are read where PyTorch keeps them: bind every `encoder.model.*`
 * tensor the trunk uses (conv `.weight`; bn `.weight`, `.bias`, `.running_mean`, `.running_var`) with pny_model_bind_param
 * first, and the gradient buffers of the trainable ones with pny_model_bind_grad.
 * pny_trunk_train_forward: images (n_images, 3, H, W) NCHW in [-1, 1] -> latent (n_images, 512, H/2, W/2) NCHW (the layout
 * PixelNeRFNet.encode(latent=) takes); running_mean / running_var are stepped in place with `momentum` (0.1 in the reference's
 * modules; 0 leaves them alone); bn_eval != 0 normalises with the running statistics instead (modules in eval() mode while
 * their parameters still train) and leaves them alone.  The activations stay in the model handle for ONE backward.
 * pny_trunk_train_backward: d loss / d latent (same shape) -> every bound gradient buffer is WRITTEN (conv weights in
 * (cout, cin, k, k), bn weight / bias).  Deterministic (no atomics). */
int pny_trunk_train_forward(pny_model* m, const float* images_dev, int n_images, int height, int width, float momentum, int bn_eval,
                            float* latent_nchw_dev, pny_stream stream);
int pny_trunk_train_backward(pny_model* m, const float* d_latent_nchw_dev, pny_stream stream);

/* Stage entry points of the trunk (exported for stage-wise tests; nothing in the library calls them).  Each runs ONE stage on
 * caller-chosen device tensors through the host launcher that the two calls above and the inference encoder use for that stage, needs no model handle, allocates its scratch per call, and -- the convolution, weight-gradient and batch-norm entries --
 * returns once `stream` has drained.  Activations are channel-last, (n, h, w, c) or (P, C) with P = n h w; weights and weight
 * gradients are (cout, cin, k, k) as PyTorch keeps them.  A convolution is named by its index in the trunk's table of
 * convolution + batch-norm units (stem, then per BasicBlock [downsample,] conv1, conv2): pny_trunk_unit gives a unit's
 * geometry and is PNY_ERR_ARG past the end of the table.  PNY_ERR_ARG, before any launch, with the function's name in
 * pny_last_error(): a NULL required pointer, a unit or level out of range, C not 64 / 128 / 256, a count below 1, sizes that
 * are not the unit's.
 * pny_trunk_conv: out = relu?(conv(in) * scale + shift + resid) per output channel.  transposed = 0: the unit's convolution,
 * in (n, hin, win, cin rounded up to 4) -> out (n, hout, wout, cout).  transposed = 1: the gradient of its input, in = the
 * gradient of its output (n, hin, win, cout) -> out (n, hout, wout, cin), (hout, wout) being the forward input's size (a
 * stride-2 unit maps two input sizes to one output size); scale / shift / resid then have cin channels; not for the stem.
 * variant (optional): the kernel instantiation launched, 100 SPLIT + 10 NT + MT (csrc/encoder.hip conv_mfma_kernel).
 * pny_trunk_conv_dw: dw = d loss / d weight from dy (n, hout, wout, cout) and the input x (n, hin, win, cin rounded up to 4);
 * splits / chunk (optional): the pixel slices the contraction was cut into, slice i = pixels [i chunk, (i + 1) chunk).
 * pny_trunk_bn_forward: out = relu?((y - mean) invstd gamma + beta + resid) on batch statistics (eps 1e-5), mean / invstd (C)
 * as the backward takes them; running_mean / running_var (both or neither) are stepped with `momentum` (0: left alone);
 * use_running != 0 normalises with them instead and leaves them alone.
 * pny_trunk_bn_backward: d_out -> dy; out = the forward's result as relu mask (out > 0), or NULL for no relu; g_out (the
 * masked d_out), d_gamma, d_beta optional.
 * pny_trunk_maxpool(_backward): max_pool2d(3, stride 2, pad 1), (n, hin, win, C) <-> (n, (hin - 1) / 2 + 1, (win - 1) / 2 + 1, C);
 * the gradient goes to the first maximum in scan order; d_in = result + add (add optional).
 * pny_trunk_upsample(_backward): pyramid level `level` (0 .. 3; 64, 64, 128, 256 channels at latent offsets 0, 64, 128, 256)
 * resampled (bilinear, align_corners = True) from (hin, win) to (h0, w0) into its channels of the (n, h0, w0, 512) latent,
 * whose other channels are left alone; the backward reads those channels of d_latent, d_in = result + add (add optional). */
int pny_trunk_unit(int unit, int* cin, int* cout, int* k, int* stride, int* pad);
int pny_trunk_conv(int unit, int transposed, const float* weight_dev, const float* in_dev, int n, int hin, int win, int hout, int wout,
                   const float* scale_dev, const float* shift_dev, const float* resid_dev, int relu, float* out_dev, int* variant,
                   pny_stream stream);
int pny_trunk_conv_dw(int unit, const float* dy_dev, const float* x_dev, int n, int hin, int win, float* dw_dev, int* splits, int64_t* chunk,
                      pny_stream stream);
int pny_trunk_bn_forward(const float* y_dev, int64_t P, int C, const float* gamma_dev, const float* beta_dev, const float* resid_dev, int relu,
                         float* running_mean_dev, float* running_var_dev, float momentum, int use_running, float* out_dev, float* mean_dev,
                         float* invstd_dev, pny_stream stream);
int pny_trunk_bn_backward(const float* d_out_dev, const float* out_dev, const float* y_dev, const float* mean_dev, const float* invstd_dev,
                          const float* gamma_dev, int64_t P, int C, int use_running, float* dy_dev, float* g_out_dev, float* d_gamma_dev,
                          float* d_beta_dev, pny_stream stream);
int pny_trunk_maxpool(const float* in_dev, int n, int hin, int win, int C, float* out_dev, pny_stream stream);
int pny_trunk_maxpool_backward(const float* in_dev, const float* g_dev, const float* add_dev, int n, int hin, int win, int C, float* d_in_dev,
                               pny_stream stream);
int pny_trunk_upsample(const float* in_dev, int n, int hin, int win, int level, int h0, int w0, float* latent_dev, pny_stream stream);
int pny_trunk_upsample_backward(const float* d_latent_dev, const float* add_dev, int n, int hin, int win, int level, int h0, int w0,
                                float* d_in_dev, pny_stream stream);

/* Introspection for bench.py: GEMM FLOPs (2/MAC, unpadded, MLP only) of the last pny_render /
 * pny_query on this scene -- `flops` as executed by the fused kernel, `flops_reference` as the
 * reference's operation order would execute them (equal when the projection is off) --, the HIP-event
 * time of its MLP kernel launches (enable_timing), the launch count, and whether the last launch
 * used the projected latent.  Any out pointer may be NULL. */
int pny_scene_last_mlp_stats(pny_scene* s, double* flops, double* flops_reference, double* kernel_ms, int* launches,
                             int* projected);
int pny_scene_enable_timing(pny_scene* s, int enable);

/* ---- Backward pass (callers: train/trainlib/PixelNerfTrainer.py:133-156 `loss.backward()`) ----
 * What autograd computes in the reference for the parameters of mlp_coarse / mlp_fine through
 * NeRFRenderer.composite (src/render/nerf.py:229-250), the output head (src/model/models.py:312-317), the cross-view
 * mean (src/util/util.py:489-499) and ResnetFC.forward (src/model/resnetfc.py:134-186).  Exact-fp32 MFMA throughout.
 * The forward call is the ordinary pny_render / pny_query (its optional z / per-sample outputs are what the backward
 * needs); inside the backward call the MLP chain is evaluated once more in the reference's operation order with every
 * GEMM operand stashed in HBM (bounded by PNYOLO_STASH_GB, default 16: larger batches are processed in chunks), then
 * the dX chain and the weight-gradient GEMMs run over the stash.
 * The fine pass's depth samples depend on the coarse depth in the reference (nerf.py:156-167: no detach): that path
 * (gradient w.r.t. sample positions through the positional code, the projection and the bilinear latent lookup) is
 * included.  The latent is differentiated through pny_scene_bind_latent_grad (below), and the ResNet-34 trunk from there by
 * pny_trunk_train_backward; not differentiated: the rays, the cameras. */

/* Gradient target of the state_dict entry `name` ("mlp_coarse.blocks.2.fc_1.weight", ...): a device buffer of the
 * parameter's shape (fp32, contiguous) that the backward calls write / add into.  NULL unbinds.  Borrowed until
 * rebound; parameters without a bound target get no gradient. */
int pny_model_bind_grad(pny_model* m, const char* name, float* grad_dev);

/* Gradient w.r.t. the scene's latent -- the backward of `F.grid_sample` (src/model/encoder.py:101) composed with lin_z
 * (src/model/resnetfc.py:176-182), i.e. what reaches `encoder.latent` in the reference when the encoder trains:
 * grad_dev is a caller-owned, caller-zeroed fp32 buffer of the latent's shape in the library's layout (ns, Hl, Wl, L)
 * (channel-last); every backward call on the scene ADDS into it (float atomics: reproducible to fp32 rounding, not bit for
 * bit, unless the model is deterministic: pny_model_set_deterministic).  NULL unbinds.  d_latent must be a multiple of 256.
 * The gradient is handed to whatever produced the latent (pny_scene_set_latent): pny_trunk_train_backward for the library's
 * trunk, the caller's own backbone otherwise. */
int pny_scene_bind_latent_grad(pny_scene* s, float* grad_dev);

/* Deterministic latent gradient (opt-in; default off).  enable != 0: from the next backward on, every scene of the model
 * (grouped scenes included) computes the latent gradient of pny_render_backward, pny_yolo_render_backward and
 * pny_query_backward without float atomics: each launch sums its contributions exactly, as 64-bit fixed-point integers on a
 * per-launch power-of-two scale chosen from a proven bound (csrc/latent_grad_det.hip), and adds the sum to grad_dev once.
 * The GEMM and its arithmetic (fp32, split f16, single-plane f16: pny_scene_set_precision) are those of the default path;
 * the result agrees with it to fp32 rounding.  Every other gradient of the library is deterministic already, so with this
 * mode a training step's gradients -- MLP parameters, latent, and the trunk's (computed from the latent gradient) -- are
 * guaranteed:
 *   - bit-identical across runs on the same GPU model, library build and launch shape (rays, samples, scenes, chunking);
 *   - NOT bit-identical across different chunkings (PNYOLO_STASH_GB) or batchings: every launch rounds its sum to fp32.
 * Cost: DESIGN.md 4.4 item 7.  A non-finite max |dY| or lin_z weight makes the launch's whole latent gradient NaN. */
int pny_model_set_deterministic(pny_model* m, int enable);
/* Which path the last backward of the scene that had a bound latent gradient took: 1 deterministic, 0 float atomics
 * (0 before any). */
int pny_scene_last_latent_grad_mode(pny_scene* s, int* deterministic);

/* Bits of the `accumulate` argument of the backward calls and of pny_model_flush_weight_grads. */
#define PNY_ACC_ADD 1            /* add to the bound gradients (0: overwrite them) */
#define PNY_ACC_IMMEDIATE 2      /* pny_render_backward: an outstanding reservation (pny_model_defer_weight_grads) belongs to another
                                    forward: recompute, and weight gradients at once into the bound buffers */
#define PNY_ACC_FINE_ONLY 4      /* pny_render_backward: only the fine pass of this backward */
#define PNY_ACC_COARSE_ONLY 8    /* pny_render_backward: only the coarse pass */
#define PNY_FLUSH_COARSE_ONLY 16 /* pny_model_flush_weight_grads: mlp_coarse's stash only */
#define PNY_FLUSH_FINE_ONLY 32   /* pny_model_flush_weight_grads: mlp_fine's stash only */

/* Backward of pny_query: d_out_dev (n, d_out) = dL/d(out).  accumulate = 0 overwrites the bound gradients of the
 * selected MLP, PNY_ACC_ADD adds to them. */
int pny_query_backward(pny_scene* s, const float* xyz_dev, const float* viewdirs_dev, int64_t n, int coarse,
                       const float* d_out_dev, int accumulate, pny_stream stream);

/* Backward of pny_composite (src/render/nerf.py:229-250): g_* = dL/d(rgb (n,3)), dL/d(depth (n)), dL/d(weights (n,k)),
 * any may be NULL.  d_sample_dev (n,k,4) = dL/d(per-sample [rgb, sigma]); d_z_dev (n,k), optional = dL/d(z) through
 * the deltas and the depth sum. */
int pny_composite_backward(const float* rays_dev, const float* z_dev, const float* sample_dev, int64_t n, int k,
                           int white_bkgd, const float* g_rgb_dev, const float* g_depth_dev, const float* g_weights_dev,
                           float* d_sample_dev, float* d_z_dev, pny_stream stream);

/* What the forward pny_render call left in its optional outputs (pny_render_out z_* / sample_*). */
typedef struct pny_render_saved {
    const float* z_coarse;      /* (n, n_coarse) */
    const float* sample_coarse; /* (n, n_coarse, 4) */
    const float* z_fine;        /* (n, n_coarse+n_fine) */
    const float* sample_fine;   /* (n, n_coarse+n_fine, 4) */
    const float* depth_coarse;  /* (n) the forward's coarse depth: the centre of the fine pass's depth samples.  Given, the
                                   fine loss is also propagated into mlp_coarse through those samples' positions, as the
                                   reference does (src/render/nerf.py:156-167, 296-298); NULL treats them as constants. */
} pny_render_saved;
/* Upstream gradients w.r.t. the outputs of pny_render; any may be NULL (= zero). */
typedef struct pny_render_grads {
    const float* rgb_coarse;     /* (n,3) */
    const float* depth_coarse;   /* (n) */
    const float* weights_coarse; /* (n,n_coarse) */
    const float* rgb_fine;
    const float* depth_fine;
    const float* weights_fine;
} pny_render_grads;
/* Backward of pny_render for one scene: composite backward + MLP backward of the fine pass (mlp_fine) and of the coarse
 * pass (mlp_coarse), into the bound gradients (accumulate as above; with one shared MLP the two passes add up).
 * PNY_ACC_FINE_ONLY: only the fine pass of this backward; PNY_ACC_COARSE_ONLY: only the coarse pass (call with
 * PNY_ACC_FINE_ONLY first: the coarse pass takes the depth-sample path's gradient the fine pass left in the scene) -- lets a
 * caller put mlp_fine's weight-gradient flush (pny_model_flush_weight_grads with PNY_FLUSH_FINE_ONLY) between the two.
 * PNY_ACC_IMMEDIATE: see above. */
int pny_render_backward(pny_scene* s, const float* rays_dev, int64_t n, const pny_render_opts* opts,
                        const pny_render_saved* saved, const pny_render_grads* grads, int accumulate, pny_stream stream);
/* Test / debugging aid: where the last pny_render_backward on this scene (with n_fine_depth > 0 and saved->depth_coarse) found
 * the forward's depth samples.  sel_dev (count = n * n_fine_depth int32, device): ray * (n_coarse + n_fine) + position in the
 * sorted fine depths, or -1 for a sample that the forward clamped to [near, far] (no gradient passes the clamp).  A sample
 * strictly inside (near, far) always has a position.  PNY_ERR_STATE when count is not that backward's n * n_fine_depth. */
int pny_scene_last_depth_sel(pny_scene* s, int32_t* sel_dev, int64_t count, pny_stream stream);
/* Stage entry points of that depth-sample path (used by pny_render_backward; exported for stage-wise tests, as
 * pny_composite_backward is).  The fine pass centres its n_fine_depth depth samples on the coarse depth without detaching it
 * (src/render/nerf.py:156-167, 296-298), so dL/dz of those samples is an extra dL/d(depth_coarse).
 * pny_locate_depth_samples: re-creates the forward's draw zz = depth_coarse + g * depth_std (g_dev (n,kfd), or NULL: the
 * seeded normals of pny_sample_fine under the same seed) and finds it in z_fine_dev (n,kt), the sorted output of
 * pny_sample_fine.  sel_dev (n*kfd int32) = ray * kt + the FIRST position holding the sample's depth, or -1 for a sample that
 * the clamp of nerf.py:166 caught (zz <= near or zz >= far).  n * kt must fit an int32.
 * pny_depth_grad_gather: g_out_dev (n) = g_in_dev (n) (NULL = 0) + the sum of dz_dev[sel] over the ray's entries with
 * sel >= 0, added in sample order in fp32 (a fixed order: bit-reproducible).  Every sel >= 0 must index dz_dev. */
int pny_locate_depth_samples(const float* rays_dev, const float* depth_coarse_dev, const float* g_dev, uint64_t seed,
                             const float* z_fine_dev, int64_t n, int kt, int kfd, float depth_std, int32_t* sel_dev,
                             pny_stream stream);
int pny_depth_grad_gather(const int32_t* sel_dev, const float* dz_dev, const float* g_in_dev, int64_t n, int kfd,
                          float* g_out_dev, pny_stream stream);

/* Backward of pny_yolo_render (src/render/yolo.py:96-114 aggregation + the MLP; caller: train/trainlib/YoloTrainer.py:160-186):
 * raw_dev (n, K, A*7) = the forward's raw_dev output, g_out_dev (n, A, 7) = dL/d(out); the sample depths are re-created
 * from u_coarse_dev / seed as the forward made them.  Gradients go to the bound targets of mlp_coarse. */
int pny_yolo_render_backward(pny_scene* s, const float* rays_dev, int64_t n, int n_coarse, const float* u_coarse_dev,
                             uint64_t seed, const float* raw_dev, const float* g_out_dev, int accumulate, pny_stream stream);
/* Backward of pny_yolo_aggregate alone (src/render/yolo.py:96-114; the stage pny_yolo_render_backward runs before the MLP,
 * exported for stage-wise tests): raw_dev (n,K,A*7), g_out_dev (n,A,7) = dL/d(out) -> d_raw_dev (n,K,A*7) = dL/d(raw), every
 * element written.  The gradient of max_k p goes to the first index that attains it, as torch.max(dim) sends it. */
int pny_yolo_aggregate_backward(const float* raw_dev, const float* g_out_dev, int64_t n, int k, int n_anchors,
                                float* d_raw_dev, pny_stream stream);

/* Deferred weight gradients.  A training batch holds several scenes (the reference's super-batch, SB objects x B rays,
 * train/train.py:23) whose backward calls are independent until the weight gradients are summed.  With deferral enabled
 * each pny_render_backward / pny_query_backward appends its tiles to a model-level stash (the calls of different scenes
 * may then run concurrently on different streams: nothing shared is written) and pny_model_flush_weight_grads runs ONE
 * weight-gradient GEMM per MLP over all of them (larger K per workgroup, one reduction).  coarse_tiles / fine_tiles =
 * 64-sample tiles to reserve for evaluations of mlp_coarse / mlp_fine: sum over the calls of ceil(points / 64).
 * PNY_ERR_ARG when the reservation exceeds the stash budget (the caller then stays in immediate mode).  The flush must be
 * ordered after the scenes' calls by the caller (same stream, or events). */
int pny_model_defer_weight_grads(pny_model* m, int enable, int ns, int64_t coarse_tiles, int64_t fine_tiles);
/* Stash in the forward.  With a reservation in place, enable = 1 makes the NEXT pny_render on this scene evaluate both
 * MLP passes with the stashing instantiation (reference operation order; rgb / sigma within fp32 rounding of the
 * projected evaluation) directly into the reservation; the pny_render_backward that follows (same reservation, z_* /
 * sample_* of that forward given in pny_render_saved) then skips its forward recompute and starts at the dX chain.
 * One-shot: the flag clears itself; a pass that does not fit the reservation runs the plain forward.
 * pny_model_flush_weight_grads: accumulate = PNY_ACC_ADD or 0, with PNY_FLUSH_COARSE_ONLY: flush mlp_coarse's stash only;
 * PNY_FLUSH_FINE_ONLY: mlp_fine's only (neither: both, mlp_coarse first). */
int pny_scene_stash_next_render(pny_scene* s, int enable);
int pny_model_flush_weight_grads(pny_model* m, int accumulate, pny_stream stream);
/* GEMM FLOPs and HIP-event time of the last flush. */
int pny_model_last_flush_stats(pny_model* m, double* flops, double* kernel_ms);
/* The arithmetic of the last flush's weight-gradient GEMM: 0 fp32, 1 split-f16, 2 single-plane (every contributor ran the
 * F16_TRAIN backward; see PNY_PRECISION_F16_TRAIN). */
int pny_model_last_flush_precision(pny_model* m, int* code);

/* Introspection for bench.py --mode train: GEMM FLOPs (2/MAC, unpadded) and HIP-event times (pny_scene_enable_timing)
 * of the three MLP kernels of the last pny_render_backward / pny_query_backward on this scene:
 * [0] stash forward (reference operation order), [1] dX chain, [2] weight-gradient GEMMs (+ reduction). */
int pny_scene_last_backward_stats(pny_scene* s, double flops[3], double kernel_ms[3]);

/* ---- optimizer: Adam over every tensor of a parameter group in ONE launch (csrc/optim.hip), with the packed operands of a
 * model rebuilt behind it.  The arithmetic is torch.optim.Adam's (no amsgrad, no maximize), per element in fp32:
 *   g = grad (+ weight_decay * p);  m += (g - m) * (1 - beta1);  v = v * beta2 + g * g * (1 - beta2);
 *   p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * with the scalars computed in double on the host.  Bit-reproducible (no atomics).  A handle is bound to one device.
 * pny_optim_add_tensor registers one tensor of `count` fp32 elements (parameter and both moments: device memory, 4-byte
 * aligned, borrowed for the handle's life) and returns its index (>= 0) or a negative status.
 * pny_optim_adam_step steps the tensors [first, first + n): grads_dev (host array of n device pointers, read during the call
 * only) gives each tensor's gradient, NULL = this tensor takes no step.  `step` is the 1-based count of the step being taken
 * (the same for every tensor of the call).  Asynchronous on `stream`; nothing waits for the device (the first step after
 * pny_optim_add_tensor uploads the work tables synchronously).  model may be NULL; otherwise the packed operands of `model`
 * are rebuilt behind the update on the same stream (what pny_model_refresh does, with its preconditions), so that the next
 * launch of any scene of the model sees the stepped weights and a weight moved out of the f16 range is reported
 * (PNY_RANGE_WEIGHT) by the step that moved it.  Not for graph capture. */
typedef struct pny_optim pny_optim;
typedef struct pny_adam_hyper {
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
} pny_adam_hyper;
int pny_optim_create(pny_optim** out, int device);
void pny_optim_destroy(pny_optim* o);
int pny_optim_add_tensor(pny_optim* o, float* param_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t count);
int pny_optim_adam_step(pny_optim* o, const pny_adam_hyper* h, float* const* grads_dev, int first, int n, pny_model* model,
                        pny_stream stream);

/* ---- training losses: the terms and, on request, the gradient w.r.t. the predictions in ONE launch each (csrc/loss.hip).
 * Model-free, raw device pointers, enqueued on `stream`; nothing waits for the device and the terms stay on the device.  Sums
 * are accumulated in fp64 in a fixed order without float atomics: the same inputs give the same bits on every run.  The
 * first call on a stream allocates that stream's reduction workspace (a few KB, kept); not for graph capture.
 * PNY_ERR_ARG on a NULL required pointer or a non-positive size.
 *
 * pny_rgb_loss: the rgb terms of PixelNerfTrainer.calc_losses (train/trainlib/PixelNerfTrainer.py:147-154) with the
 * criteria of model/loss.py:92-104 (MSELoss or L1Loss, reduction "mean"), over n contiguous fp32 elements each:
 *   rc = lambda_coarse * mean(e(coarse, gt));  rf = lambda_fine * mean(e(fine, gt));  t = rc + rf
 *   e(x, g) = (x - g)^2, or |x - g| where the pass's use_l1 is set.  fine_dev NULL = no fine pass: rf = 0, t = rc.
 * terms_dev[3] = {rc, rf, t}.  d_coarse_dev / d_fine_dev (n each, or NULL) receive dt/dcoarse and dt/dfine:
 * lambda * 2 (x - g) / n, or lambda * sign(x - g) / n with sign(0) = 0. */
typedef struct pny_rgb_loss_desc {
    int32_t use_l1_coarse; /* conf loss.rgb.use_l1 */
    int32_t use_l1_fine;   /* conf loss.rgb_fine.use_l1 */
    float lambda_coarse;   /* conf loss.lambda_coarse */
    float lambda_fine;     /* conf loss.lambda_fine */
} pny_rgb_loss_desc;
int pny_rgb_loss(const pny_rgb_loss_desc* desc, const float* coarse_dev, const float* fine_dev, const float* gt_dev, int64_t n,
                 float* terms_dev, float* d_coarse_dev, float* d_fine_dev, pny_stream stream);

/* pny_yolo_loss: YoloLoss.forward (src/model/loss.py:121-163, util.iou src/util/util.py:582-608).
 * pred_dev (cells, A, 5 + C) rows [p_obj, x, y, w, h, C class logits]; target_dev (cells, A, 6) rows [obj, x, y, w, h, class];
 * anchors_dev (A, 2) (w, h), on the device.  Per (cell, anchor):
 *   obj == 0: no-object term -max(log(1 - p_obj), -100) (BCELoss's clamp);
 *   obj == 1: object term (p_obj - iou * obj)^2 with iou of [sigmoid(x), sigmoid(y), exp(w) aw, exp(h) ah] and target[1:5],
 *             a constant for the gradient; box term (sigmoid(x) - tx)^2, (sigmoid(y) - ty)^2, (w - log(1e-6 + tw / aw))^2,
 *             (h - log(1e-6 + th / ah))^2; class term logsumexp(logits) - logits[class];
 *   any other obj (the dataset's -1 for ignored anchors): nothing.
 * Means: no-object over n_noobj, object and class over n_obj, box over 4 n_obj.  n_obj == 0: the three object terms are
 * exactly 0 (the reference returns a CPU torch.tensor(0) there).  n_noobj == 0: the no-object term and the total are NaN, as
 * ATen's mean over nothing.  A class outside [0, C) reads nothing out of bounds and makes the class term, the total and that
 * cell's logit gradients NaN (ATen raises a device assert there).  Unlike loss.py:145,147, pred and target are not modified.
 * terms_dev[5] = {total, box, object, no_object, class}, total = the weighted sum, the others unweighted as the reference
 * returns them.  counts_dev[2] (or NULL) = {n_obj, n_noobj}.  d_pred_dev (cells, A, 5 + C) (or NULL) = dtotal/dpred as
 * autograd gives it for the reference (BCE backward p / max(p (1 - p), 1e-12) / n_noobj); every element is written, zeros where no
 * gradient arrives.  cells * A must be below 2^31. */
typedef struct pny_yolo_loss_desc {
    int32_t num_anchors;   /* A = num_anchors_per_scale */
    int32_t num_classes;   /* C = pred's last dimension - 5 */
    float box_loss;        /* conf yolo.weights.* (loss.py:165-179) */
    float object_loss;
    float no_object_loss;
    float class_loss;
} pny_yolo_loss_desc;
int pny_yolo_loss(const pny_yolo_loss_desc* desc, const float* pred_dev, const float* target_dev, const float* anchors_dev,
                  int64_t cells, float* terms_dev, int32_t* counts_dev, float* d_pred_dev, pny_stream stream);

/* pny_yolo_loss_batches: the YOLO losses of ALL mini-batches of a training step in one launch, with the trainer's
 * per-mini-batch normalisation (train/trainlib/YoloTrainer.py:149-208: the rays of every scale are split into mini-batches
 * of ray_batch_size rows, YoloLoss is called and backpropagated per mini-batch, the five values are summed on the host and
 * divided by the number of mini-batches).  The accumulated gradient of that loop is the gradient of sum_m loss_m, which is
 * not YoloLoss over all rows: every loss_m divides by its own mini-batch's n_obj and n_noobj.
 * pred_dev (N, A, 5 + C) and target_dev (N, A, 6) hold the rows of all scales in flat order (pny_yolo_train_batch's row
 * order), N = sum rows[s]; anchors_dev (n_scales, A, 2).  Scale s owns ceil(rows[s] / batch_rows) consecutive mini-batches,
 * the last of a scale may be short, none straddles two scales; M = their number, pny_yolo_loss_batches_count.  One
 * workgroup per mini-batch; which rows it takes is computed from `batches` in the kernel (no table, no upload).
 * Per mini-batch m the arithmetic is pny_yolo_loss's on that slice with that scale's anchors (the same per-item code, the
 * n_obj == 0, n_noobj == 0 and class-out-of-range rules included): terms_seg_dev (M, 5) rows {total, box, object, no_object,
 * class}, counts_seg_dev (M, 2) (or NULL) rows {n_obj, n_noobj}, and d_pred_dev (N, A, 5 + C) (or NULL) = d (sum_m total_m) /
 * dpred, every element written.  A mini-batch of at most 1024 (row, anchor) pairs gives the bits of pny_yolo_loss on its slice;
 * a longer one the same counts and gradient, and terms that differ by the summation order.
 * step_dev[6] = {S(total), S(total) / M, S(box) / M, S(object) / M, S(no_object) / M, S(class) / M}: S adds the fp32 values
 * of terms_seg_dev in mini-batch order in fp64 (the trainer's `total += loss.item()`), each entry rounded to fp32 once.
 * step_dev[0] is the value whose gradient d_pred_dev is; step_dev[1..5] are the trainer's loss_dict.
 * PNY_ERR_ARG: a NULL required pointer, n_scales outside 1 .. 4, a non-positive rows[s] or batch_rows, M > 4096 (refused,
 * never truncated), num_anchors < 1, num_classes < 1, N * A >= 2^31. */
typedef struct pny_yolo_batches_desc {
    int32_t n_scales;      /* 1 .. 4 */
    int32_t batch_rows;    /* conf yolo.ray_batch_size */
    int64_t rows[4];       /* rows (rays) of each scale, flat order */
} pny_yolo_batches_desc;
int pny_yolo_loss_batches(const pny_yolo_loss_desc* desc, const pny_yolo_batches_desc* batches, const float* pred_dev,
                          const float* target_dev, const float* anchors_dev, float* terms_seg_dev, int32_t* counts_seg_dev,
                          float* step_dev, float* d_pred_dev, pny_stream stream);
int pny_yolo_loss_batches_count(const pny_yolo_batches_desc* batches); /* M, or a negative status */

/* ---- NaN / Inf monitor: the finiteness tests of a YOLO training step without a host wait (csrc/finite.hip).  Replaces the
 * `if torch.isnan(x).any()` / `torch.isinf(x).any()` tests on the render and the targets (train/trainlib/YoloTrainer.py:
 * 163-178) and the two per-parameter generator expressions over p.grad (:188-194), each of which is two launches and a
 * blocking read.  ONE kernel scans a table of fp32 tensors (a value is non-finite when its exponent bits are all ones; a
 * non-zero mantissa makes it a NaN) and records what it meets per caller-chosen group in two int32 words on the device:
 *   flags_dev[2 * group]      bits: PNY_FINITE_NAN = a NaN was seen, PNY_FINITE_INF = a +-Inf was seen
 *   flags_dev[2 * group + 1]  first: the lowest table index of a tensor in which either was seen; INT32_MAX after reset
 * combined with atomic OR / MIN: the words do not depend on the execution order and stay set across calls until
 * pny_finite_reset.  A scan that meets nothing writes nothing.  flags_dev holds 2 * (largest group + 1) words, 4-byte aligned;
 * the host reads it when it wants to (one copy per step).  Tensors are fp32, 4-byte aligned, any size; a count of 0 is legal.
 * pny_finite_add_tensor registers a tensor in the handle's table, which is kept on the device (for buffers whose address
 * is stable: gradients), and returns its table index (>= 0) or a negative status; it copies the entry to the device before it
 * returns (registration is not part of a step; should growing the table fail, the handle is left empty and every tensor has
 * to be registered again).  pny_finite_check scans the registered tensors [first, first + n) in one
 * launch; the index recorded is the table index.  pny_finite_check_tensors scans up to PNY_FINITE_MAX_IMMEDIATE tensors given
 * in host arrays (for the fresh render and target tensors of a mini-batch): pointers, counts and groups travel as kernel
 * arguments, the index recorded is the position in the arrays; the same kernel body.  pny_finite_reset sets n_groups pairs
 * to {0, INT32_MAX}.  The check and reset calls enqueue one kernel on `stream` (pny_finite_check_tensors and pny_finite_reset
 * on the current device) and neither allocate, copy nor wait.  PNY_ERR_ARG: a NULL pointer with a count > 0, a negative
 * count or group, n above the limit, a range outside the table, NULL or unaligned flags_dev. */
#define PNY_FINITE_NAN 1
#define PNY_FINITE_INF 2
#define PNY_FINITE_MAX_IMMEDIATE 8
typedef struct pny_finite pny_finite;
int pny_finite_create(pny_finite** out, int device);
void pny_finite_destroy(pny_finite* f);
int pny_finite_add_tensor(pny_finite* f, const float* dev, int64_t count, int group);
int pny_finite_check(pny_finite* f, int first, int n, int32_t* flags_dev, pny_stream stream);
int pny_finite_check_tensors(const float* const* ptrs, const int64_t* counts, const int32_t* groups, int n, int32_t* flags_dev,
                             pny_stream stream);
int pny_finite_reset(int32_t* flags_dev, int n_groups, pny_stream stream);

/* ---- view metrics: the clamped 8-bit image, PSNR and SSIM of every rendered view in ONE launch (csrc/metrics.hip).
 * Replaces the scoring tail of the reference's eval scripts (eval/eval.py:288-345, eval/calc_metrics.py:189-191), which bring
 * every render to the host and call skimage there, and util.psnr (src/util/util.py:502).  Model-free, raw device pointers,
 * enqueued on `stream`; nothing waits for the device and the results stay on the device.  Sums are accumulated in fp64 in a
 * fixed order without float atomics: the same inputs give the same bits on every run.  The first call on a stream allocates
 * that stream's reduction workspace (1 MiB, kept; a launch of more than 65 536 tiles replaces it, and that alone waits for the
 * device); not for graph capture.
 *
 * rgb_dev (NV, H, W, 3): the renders.  x = clamp(rgb, 0, 1) in fp32 (eval.py:288).
 * gt_dev: PNY_GT_NHWC_01   (NV, H, W, 3) in [0, 1], taken as given (calc_metrics.py);
 *         PNY_GT_NCHW_PM1  (NV, 3, H, W) in [-1, 1], the dataset's `images`: y = fl32(g * 0.5 + 0.5) (eval.py:315).
 * rgb8_dev (NV, H, W, 3) (or NULL) = (uint8) trunc(fl32(x * 255)), numpy's (all_rgb * 255).astype(np.uint8) (eval.py:291).
 * metrics_dev (NV, 2) (or NULL: the launch only converts) = per view {psnr, ssim}, fp64 because the reference reports Python
 * floats (the one exception to "all floating point data is fp32"):
 *   psnr = 10 log10(1 / mean((x - y)^2)) over the view's H * W * 3 elements, difference, squares and mean in fp64
 *          (skimage compare_psnr, data_range = 1); identical images give +inf;
 *   ssim = skimage compare_ssim(multichannel=True, data_range=1): win_size 7, uniform window, sample covariance, K1 = 0.01,
 *          K2 = 0.03; the mean of S over the (H - 6) (W - 6) windows inside the image, per channel, then over the 3 channels;
 *          the five moments of a window are fp64 sums.
 * A NaN prediction makes both metrics of ITS view NaN and writes byte 0.
 * PNY_GT_FLAT: util.psnr's form.  rgb_dev and gt_dev are (NV, height * width) plain elements, compared as given (no clamp, no
 * channels, any height and width >= 1): psnr = -10 log10(mean((p - t)^2)), ssim = NaN; rgb8_dev must be NULL.
 * PNY_ERR_ARG: a NULL desc, rgb_dev or gt_dev, both outputs NULL, a non-positive size, height or width below 7 (except
 * PNY_GT_FLAT), an unknown gt_layout, win_size other than 7, or 2^31 or more elements (NV * H * W * 3). */
#define PNY_GT_NHWC_01 0
#define PNY_GT_NCHW_PM1 1
#define PNY_GT_FLAT 2
typedef struct pny_view_metrics_desc {
    int32_t n_views, height, width; /* channels = 3 */
    int32_t gt_layout;              /* PNY_GT_NHWC_01 | PNY_GT_NCHW_PM1 | PNY_GT_FLAT */
    int32_t win_size;               /* 7; anything else is PNY_ERR_ARG in this build */
} pny_view_metrics_desc;
int pny_view_metrics(const pny_view_metrics_desc* desc, const float* rgb_dev, const float* gt_dev,
                     double* metrics_dev /* (NV, 2) {psnr, ssim}, or NULL */,
                     uint8_t* rgb8_dev /* (NV, H, W, 3), or NULL */, pny_stream stream);

/* ---- LPIPS (VGG-16): the third number of the reference's eval tail (eval/calc_metrics.py:186-246) on the device
 * (csrc/lpips.hip, csrc/pny_lpips.h; the 13 convolutions run on the trunk's exact-fp32 MFMA kernel).  LPIPS v0.1 with
 * net = "vgg", normalize = False, spatial = False, restated from the published definition:
 *   x in [-1, 1] -> (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450) (compiled in);
 *   VGG-16 `features` 0 .. 29 (3x3 convolutions with bias and relu, max_pool2d(2, 2) in floor mode), tapped behind relu1_2,
 *   relu2_2, relu3_3, relu4_3 and relu5_3; per tap f^ = f / (sqrt(sum_c f^2) + 1e-10), sum_c w[c] (f^0[c] - f^1[c])^2, the mean
 *   over the tap's pixels in fp64; the value is the sum of the five taps.
 * A handle holds the weights.  pny_lpips_load_weights takes host tensors by name, one call each: "conv0.weight" ..
 * "conv12.weight" (cout, cin, 3, 3) and "conv0.bias" .. "conv12.bias" (cout) in execution order, "lin0.weight" .. "lin4.weight"
 * with 64, 128, 256, 512, 512 elements in any shape; an unknown name or a wrong shape is PNY_ERR_ARG and names the tensor.
 * pny_lpips_finalize uploads them to the current device and packs the convolutions there, on `stream`; it returns when the
 * packing has run, names the first missing tensor (PNY_ERR_STATE), and may be called again after further loads.
 *
 * pny_lpips_forward scores n_pairs pairs: pred and gt are device tensors of n_pairs images in the forms below, out (n_pairs)
 * fp64 on the device.  It allocates nothing and waits for nothing: the caller passes `work`, pny_lpips_workspace_bytes(
 * desc->batch_size, H, W) bytes of device memory, 256-byte aligned.  desc->batch_size >= n_pairs is the batch the caller walks
 * its views in; the kernels' arithmetic follows from the layer, H and W alone, so a pair's value has the same bits in every
 * batch and on every run (no float atomics; the five taps add to `out` in stream order).  23 launches.
 *   PNY_LPIPS_F32_NHWC_01   (n, H, W, 3) fp32 in [0, 1]: t * 2 - 1 (a prediction is clamped to [0, 1] first if desc->clamp)
 *   PNY_LPIPS_F32_NCHW_PM1  (n, 3, H, W) fp32 in [-1, 1], taken as given
 *   PNY_LPIPS_U8_NHWC       (n, H, W, 3) bytes: (b / 255) * 2 - 1
 *   PNY_LPIPS_F32_NCHW_01   (n, 3, H, W) fp32 in [0, 1]: as NHWC_01
 * PNY_ERR_ARG: H or W below 16 (relu5_3 would be empty), or a batch whose largest activation, 2 n H W 64 floats, is 2^31
 * elements or more; the message says which.  PNY_ERR_STATE: not finalized.
 * pny_lpips_workspace_bytes runs on the host alone: 4 (r64(2n H W 4) + 2 r64(2n H W 64)) bytes, r64 = rounded up to 64 floats.
 *
 * The stages, for tests: pny_lpips_prepare writes the (2n, H, W, 4) scaled channel-last images (predictions first);
 * pny_lpips_maxpool2 pools a channel-last (n, h, w, c) tensor, c % 4 == 0, to (n, h / 2, w / 2, c); pny_lpips_distance scores one
 * tap tensor (2n, h, w, c), c in {64, 128, 256, 512}, against weights (c) and writes (accumulate = 0) or adds to out (n);
 * pny_lpips_conv runs VGG convolution `layer` (0 .. 12) alone on n channel-last images (n, h, w, cin; 4 channels for layer 0)
 * into (n, h, w, cout) and reports the instantiation it launched (100 SPLIT + 10 NT + MT), chosen as pny_lpips_forward chooses
 * it for a batch of n images at that layer. */
#define PNY_LPIPS_F32_NHWC_01 0
#define PNY_LPIPS_F32_NCHW_PM1 1
#define PNY_LPIPS_U8_NHWC 2
#define PNY_LPIPS_F32_NCHW_01 3
typedef struct pny_lpips pny_lpips;
typedef struct pny_lpips_desc {
    int32_t height, width;      /* channels = 3 */
    int32_t pred_kind, gt_kind; /* PNY_LPIPS_* */
    int32_t clamp;              /* clamp a float [0, 1] prediction to [0, 1] first (the lpips package does not: 0) */
    int32_t batch_size;         /* pairs per batch the workspace was sized for; 0: n_pairs */
} pny_lpips_desc;
int pny_lpips_create(pny_lpips** out);
void pny_lpips_destroy(pny_lpips* h);
int pny_lpips_load_weights(pny_lpips* h, const char* name, const float* data_host, const int64_t* shape, int ndim);
int pny_lpips_finalize(pny_lpips* h, pny_stream stream);
int pny_lpips_workspace_bytes(int n_pairs, int height, int width, size_t* bytes);
int pny_lpips_forward(pny_lpips* h, const pny_lpips_desc* desc, const void* pred_dev, const void* gt_dev, int n_pairs,
                      void* work_dev, double* out_dev, pny_stream stream);
int pny_lpips_prepare(const pny_lpips_desc* desc, const void* pred_dev, const void* gt_dev, int n_pairs, float* out_dev,
                      pny_stream stream);
int pny_lpips_maxpool2(const float* in_dev, int n, int h, int w, int c, float* out_dev, pny_stream stream);
int pny_lpips_distance(const float* tap_dev, const float* weight_dev, int n_pairs, int h, int w, int c, int accumulate,
                       double* out_dev, pny_stream stream);
int pny_lpips_conv(pny_lpips* h, int layer, const float* in_dev, int n, int height, int width, float* out_dev, int* variant,
                   pny_stream stream);

/* ---- colour jitter: the training-time augmentation of all views of all objects in ONE launch (csrc/augment.hip).
 * Replaces the four passes per view that the reference's ColorJitterDataset runs on CPU tensors in every __getitem__
 * (src/data/data_util.py:34-47; get_split_dataset wraps the training split of `yolo` and `dvr_dtu` in it,
 * src/data/__init__.py:12-76).  Model-free, raw device pointers, enqueued on `stream`: no workspace, no allocation, no
 * synchronisation, and the same input gives the same bits on every run (no atomics; one workgroup owns one image).
 *
 * images_dev: PNY_IMG_F32_NCHW_PM1  (n_objs, n_views, 3, H, W) fp32 in [-1, 1], the datasets' `images`: t = (x + 1) * 0.5;
 *             PNY_IMG_U8_NHWC       (n_objs, n_views, H, W, 3) bytes as decoded: t = x / 255.  Any byte alignment.
 * factors_host (n_objs, 4) = per object {hue, saturation, brightness, contrast}, the four draws of data_util.py:35-38 in
 * that order; read before the call returns.
 * out_dev (n_objs, n_views, 3, H, W) fp32 in [-1, 1]; for PNY_IMG_F32_NCHW_PM1 it may be images_dev (in place).
 * Per image, all in fp32, in this order (data_util.py:41-45):
 *   saturation  blend(t, grey(t), saturation), grey = 0.2989 r + 0.587 g + 0.114 b, blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)
 *   hue         RGB -> HSV, h <- (h + hue) mod 1, HSV -> RGB
 *   contrast    blend(t, mean, contrast), mean = the image's mean grey level after the two steps above (an fp64 sum in a fixed
 *               order, rounded to fp32)
 *   brightness  blend(t, 0, brightness)
 * and out = t * 2 - 1.
 * PNY_ERR_ARG, before any launch: a NULL pointer, a non-positive size, an unknown in_format, n_objs > PNY_JITTER_MAX_OBJS (the
 * caller splits), 2^31 or more elements (n_objs * n_views * H * W * 3), |hue| > 0.5, a negative or non-finite saturation,
 * brightness or contrast, out_dev == images_dev with PNY_IMG_U8_NHWC. */
enum { PNY_IMG_F32_NCHW_PM1 = 0, PNY_IMG_U8_NHWC = 1 };
#define PNY_JITTER_MAX_OBJS 64
typedef struct pny_color_jitter_desc {
    int32_t n_objs, n_views, height, width; /* channels = 3 */
    int32_t in_format;                      /* PNY_IMG_F32_NCHW_PM1 | PNY_IMG_U8_NHWC */
} pny_color_jitter_desc;
int pny_color_jitter(const pny_color_jitter_desc* desc, const void* images_dev, const float* factors_host, float* out_dev,
                     pny_stream stream);

/* ---- ingest: from decoded bytes to the tensors the trainer uses, on the device (csrc/ingest.hip; arithmetic in
 * csrc/pny_ingest.h).  Replaces what the reference's datasets do per view on CPU tensors between imread and the item: the
 * resize and normalisation of src/data/YOLODataset.py:79-225 (1920 x 1080 views scaled by image_scale) and the white-background
 * mask, bounding box, normalisation and area resize of src/data/SRNDataset.py:61-136.  File reading and PNG decoding stay on
 * the host.  Model-free, raw device pointers, enqueued on `stream`: no workspace, no allocation, no synchronisation, no
 * atomics; the same input gives the same bits on every run, for a view alone as for the same view inside a batch.
 * ONE launch; TWO with white_mask (the box is a second launch with one workgroup per view).  All arithmetic is fp32.
 *
 * images_dev (n_views, height, width, channels) bytes as decoded, any byte alignment; of a pixel's `channels` bytes the first
 *            three are used.
 * out_dev    (n_views, 3, out_height, out_width) fp32 in [-1, 1]: the byte map t = b / 255, out = (t - 0.5) / 0.5, bit-equal to
 *            ToTensor + Normalize(0.5, 0.5) for all 256 bytes, applied after
 *   PNY_RESIZE_NONE         nothing;
 *   PNY_RESIZE_BILINEAR_U8  cv2.resize(INTER_LINEAR) as this project's data.resize_bilinear_u8 restates it: half-pixel centres,
 *                           src = max(fma(scale, dst + 0.5, -0.5), 0), scale = in / out; i0 = min(floor(src), in - 1),
 *                           i1 = min(i0 + 1, in - 1), lambda = src - i0; four taps, rounded half to even back to a byte and
 *                           clamped to 0 .. 255.  Any ratio, enlarging included;
 *   or before
 *   PNY_RESIZE_AREA         F.interpolate(mode="area") of the mapped values: window [floor(i in / out), ceil((i + 1) in / out))
 *                           per axis, an fp32 sum in row-major order, one division by the element count.
 * white_mask = 1 (SRN): mask_dev (n_views, 1, out_height, out_width) = m after the same resize, m = 1 where none of the pixel's
 *            three bytes is 255 (`(img != 255).all(axis=-1)`, SRNDataset.py:81), else 0; bbox_dev (n_views, 4) =
 *            [cmin, rmin, cmax, rmax] of m at decoded resolution, each multiplied by (float)(out_height / (double)height) when
 *            resizing.  A view with an empty mask gets [width, height, -1, -1], unscaled: the host path raises there, the device
 *            path does not wait, so the caller tests bbox[:, 2] < 0.
 * PNY_ERR_ARG, before any launch: a NULL desc, images_dev or out_dev; a non-positive size; channels not 3 or 4; an unknown
 * resize; out size != size under PNY_RESIZE_NONE; 2^31 or more input or output elements; mask_dev or bbox_dev without
 * white_mask, or white_mask without both; white_mask with PNY_RESIZE_BILINEAR_U8 (no dataset does that). */
enum { PNY_RESIZE_NONE = 0, PNY_RESIZE_BILINEAR_U8 = 1, PNY_RESIZE_AREA = 2 };
typedef struct pny_ingest_desc {
    int32_t n_views, height, width; /* decoded size */
    int32_t channels;               /* 3 or 4: byte stride of a pixel; the first three are used */
    int32_t out_height, out_width;  /* == height, width for PNY_RESIZE_NONE */
    int32_t resize;                 /* PNY_RESIZE_* */
    int32_t white_mask;             /* 1: also the white-background mask and box (SRN) */
} pny_ingest_desc;
int pny_ingest_views(const pny_ingest_desc* desc, const uint8_t* images_dev /* (NV, H, W, C) */,
                     float* out_dev /* (NV, 3, OH, OW) in [-1, 1] */, float* mask_dev /* (NV, 1, OH, OW) or NULL */,
                     float* bbox_dev /* (NV, 4) or NULL */, pny_stream stream);

/* The YOLO target grids of all views in ONE launch: YOLODataset._get_all_bboxes (src/data/YOLODataset.py:156-225) for every
 * view, complete grids (zero fill included), exactly what the trainer stacks per scale (YoloTrainer.py:97-101) and
 * pny_yolo_train_batch takes.  One workgroup per view: all threads zero the view's grids, then one thread walks the view's
 * boxes in file order.
 * boxes_dev (n_views, max_boxes, 5) fp64 {cx, cy, w, h, cls}, normalised to the image; view v uses its first n_boxes_dev[v]
 * rows (clamped to 0 .. max_boxes).  anchors_host (n_scales * n_anchors, 2) {w, h}, read before the call returns.
 * targets_dev: n_scales device pointers (a host array), scale s being (n_views, Hs, Ws, n_anchors, 6) fp32 with
 * Hs = height / cell_sizes[s], Ws = width / cell_sizes[s] (integer division).
 * Per box: the IoU of (w, h), rounded to fp32, against every anchor in fp32 (min * min, (w h + aw ah) - inter, a division);
 * anchors are visited by descending IoU, ties by ascending index; cell i = (int)(Hs cy), j = (int)(Ws cx) in fp64; on each
 * scale the first visited anchor whose slot (i, j, anchor) is free gets [1, Ws cx - j, Hs cy - i, w Ws, h Hs, (int)cls]
 * (fp64, rounded once); a free slot visited later on that scale is set to -1 when its IoU > ignore_iou_thresh (fp32).  A box
 * whose cell lies outside a grid (cx or cy outside [0, 1)) is left out of that grid.
 * PNY_ERR_ARG, before any launch: a NULL pointer (a grid pointer included), a non-positive n_views, max_boxes, height or width,
 * n_scales outside 1 .. PNY_YOLO_BATCH_MAX_SCALES, n_anchors outside 1 .. 64 or n_scales * n_anchors above 64, a cell size below
 * 1 or above the image, a negative or non-finite ignore_iou_thresh, 2^31 or more elements in the boxes or in a grid. */
#define PNY_YOLO_TARGETS_MAX_ANCHORS 64
typedef struct pny_yolo_targets_desc {
    int32_t n_views, max_boxes;     /* rows per view in boxes_dev */
    int32_t height, width;          /* the resized image the grids refer to */
    int32_t n_scales;               /* 1 .. PNY_YOLO_BATCH_MAX_SCALES */
    int32_t cell_sizes[PNY_YOLO_BATCH_MAX_SCALES];
    int32_t n_anchors;              /* A per scale, 1 .. 64; n_scales * A <= 64 */
    float ignore_iou_thresh;
} pny_yolo_targets_desc;
int pny_yolo_build_targets(const pny_yolo_targets_desc* desc, const double* boxes_dev /* (NV, max_boxes, 5) cx cy w h cls */,
                           const int32_t* n_boxes_dev /* (NV) */, const float* anchors_host /* (n_scales * A, 2) */,
                           float* const* targets_dev /* n_scales pointers, (NV, Hs, Ws, A, 6) */, pny_stream stream);

/* ---- resident views: a dataset's decoded views stay on the device as bytes, and a training step's ray batch, ground truth
 * and source views are drawn straight from them (csrc/resident.hip; arithmetic in csrc/pny_resident.h, shared with
 * pny_ingest_views and pny_sample_train_batch).  Replaces what runs per step on the host before the trainer starts: the
 * reference's SRNDataset.__getitem__ (src/data/SRNDataset.py:61-136) and DVRDataset.__getitem__ (src/data/DVRDataset.py:110-275)
 * decode, normalise and resize ALL views of every object of the super-batch, the DataLoader copies them to the device, and
 * train/trainlib/PixelNerfTrainer.py:76-133 then reads ray_batch_size pixels and at most three source views per object from
 * them.  The caller owns the store; these entries only read it.
 *
 * The store: one decoded geometry (height, width, channels = 3 or 4, of which the first three bytes of a pixel are used) and
 * one output geometry (out_height, out_width, resize = PNY_RESIZE_*, as pny_ingest_views has them).  objs_dev is a device
 * table of n_store_objs 16-byte records
 *     { const uint8_t* views;   (n_views, height, width, channels) bytes of the object, on the device
 *       int32_t n_views;        1 .. max_views; objects may differ
 *       int32_t first_row; }    the object's first row of poses_dev and bboxes_dev
 * poses_dev (n_rows, 4, 4) cam->world and bboxes_dev (n_rows, 4) `cmin rmin cmax rmax` at output resolution (or NULL: uniform
 * mode) hold the views of all objects one after another; focal_dev (n_store_objs, 2) fx fy and c_dev (n_store_objs, 2) (or
 * NULL: (out_width / 2, out_height / 2)) are at output resolution.  All offsets are 64-bit.
 *
 * Both entries take raw device pointers and enqueue ONE kernel on `stream`: no allocation, no copy, no synchronisation, no
 * atomics; the same input gives the same bits on every run.  The call cannot look at device-side indices without waiting, so
 * the kernels clamp them into range (memory safety, as for replayed draws): an object id into [0, n_store_objs), a view id
 * into [0, n_views), a record's n_views into [1, max_views], its first_row into [0, n_rows - n_views], a draw as
 * pny_sample_train_batch clamps it.
 *
 * pny_resident_train_batch: share s of the batch is object obj_ids_dev[s] (repeats allowed).  Of `desc` it reads n_objs = SB,
 * n_views = max_views (the largest n_views of the store: the bound the draw's limit is checked against), height, width =
 * the DECODED size, n_rays = B, z_near, z_far, seed and draw_offset; focal_rows, focal_cols and c_rows are ignored (focal_dev
 * and c_dev have one row per store object).  Share s has the bits that pny_sample_train_batch gives for a ONE-object call
 * with draw_offset + s * B (or with rows s of `draws`) on pny_ingest_views(store resize) of that object's views, with its
 * poses, focal, c and boxes; the object's own n_views enters the draws as NV does there.  rgb_gt_dev = v * 0.5f + 0.5f with v
 * the fp32 pny_ingest_views writes at that output pixel, computed for the sampled pixel only.  Writes rays_dev (SB, B, 8)
 * 16-byte aligned, rgb_gt_dev (SB, B, 3) and, unless NULL, pix_dev (SB, B, 3) int32 [view within the object, y, x] at output
 * resolution.
 *
 * pny_ingest_views_indexed: pny_ingest_views without white_mask whose output view i is view view_of_dev[i] of object
 * obj_of_dev[i] of the store: out_dev (desc->n_views, 3, out_height, out_width), bit-equal to pny_ingest_views on the gathered
 * views.  desc->white_mask must be 0.
 *
 * PNY_ERR_ARG, before any launch, naming the argument: a NULL required pointer; a non-positive size or count; channels not 3
 * or 4; an unknown resize; out size != size under PNY_RESIZE_NONE; max_views * out_height * out_width >= 2^32 (the draw's
 * limit); 2^31 or more rays, bytes in a view, or output elements; a replay without the draws its mode reads; rays_dev not
 * 16-byte aligned; white_mask set. */
int pny_resident_train_batch(const pny_train_batch_desc* desc, int32_t channels, int32_t out_height, int32_t out_width,
                             int32_t resize, const void* objs_dev /* n_store_objs records */, int32_t n_store_objs,
                             const int32_t* obj_ids_dev /* (SB) */, const float* poses_dev /* (n_rows, 4, 4) */, int64_t n_rows,
                             const float* focal_dev /* (n_store_objs, 2) */, const float* c_dev /* (n_store_objs, 2) or NULL */,
                             const float* bboxes_dev /* (n_rows, 4) or NULL */, const pny_train_batch_draws* draws,
                             float* rays_dev, float* rgb_gt_dev, int32_t* pix_dev, pny_stream stream);
int pny_ingest_views_indexed(const pny_ingest_desc* desc, const void* objs_dev /* n_store_objs records */, int32_t n_store_objs,
                             int32_t max_views, const int32_t* obj_of_dev /* (n_views) */,
                             const int32_t* view_of_dev /* (n_views) */, float* out_dev /* (n_views, 3, OH, OW) */,
                             pny_stream stream);

/* ---- mesh extraction: the sigma grid and marching cubes of the reference's src/util/recon.py on the device (csrc/recon.hip;
 * conventions and arithmetic in csrc/pny_recon.h, the case table in csrc/mc_table.h, generated by tools/gen_mc_table.py).
 * Model-free, raw device pointers, enqueued on `stream`: no allocation, no copy, no synchronisation, no atomics; the same
 * input gives the same bits on every run.  Arrays named *_host are read before the call returns.
 *
 * pny_grid_points: ONE launch writes the flat indices [i0, i1) of the grid of util.gen_grid(*zip(c1, c2, reso),
 * ij_indexing=True) (x slowest, z fastest) to xyz_dev (i1 - i0, 3), and to dirs_dev (i1 - i0, 3) the fake view directions of
 * recon.py:54.  A coordinate is np.linspace(lo, hi, sz, dtype=float32): lo + i * ((hi - lo) / (sz - 1)) in double, the last
 * point exactly hi, rounded to fp32 (bit-equal to numpy's).  A direction is -p / |p| in fp32 from the rounded coordinates,
 * |p| = sqrt((x x + y y) + z z); a grid point exactly at the origin gets (0, 0, 0), where the reference's 0 / 0 gives NaN.
 * PNY_ERR_ARG, before any launch: a NULL pointer, a reso below 2, non-finite bounds, c2 <= c1 on an axis, 3 X Y Z >= 2^31,
 * i0 < 0, i1 > X Y Z or i0 >= i1. */
int pny_grid_points(const double* c1_host /* 3 */, const double* c2_host /* 3 */, const int32_t* reso_host /* 3: X Y Z */,
                    int64_t i0, int64_t i1, float* xyz_dev /* (i1 - i0, 3) */, float* dirs_dev /* (i1 - i0, 3) */,
                    pny_stream stream);

/* Marching cubes over sigma_dev, a (X, Y, Z) fp32 volume (dims_host = {X, Y, Z}), giving an indexed mesh in index coordinates:
 *   corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) and is inside when sigma > iso, strictly (a NaN is
 *   outside); a grid edge whose ends differ is cut, and the grid point at its lower end owns the vertex: with a the owner's
 *   sigma and b the neighbour's, t = (iso - a) / (b - a), coordinate (float)i + t along the edge, both fp32;
 *   vertices in ascending owner flat index, then axis x, y, z; triangles in ascending cell flat index (the cell's low corner),
 *   then table order; int32 indices; by the right-hand rule the normals point from sigma > iso to sigma < iso.
 * Every cut edge has exactly one vertex (the mesh is welded).  A sigma equal to iso gives zero-area triangles, which are kept.
 * pny_mc_workspace_bytes: the workspace pny_mc_count fills and pny_mc_emit reads, 8 bytes per grid point and 8 per 1024.
 * pny_mc_count: the per-point counts and their exclusive scan (2 launches up to 1024 * 1024 points, 4 above), and
 *   counts_dev = int32[2] {vertices, triangles}.  Reading them is the one host read between the two calls.  (More than 2^31 - 1
 *   triangles, which needs over 429 million grid points, read back negative and pny_mc_emit refuses them.)
 * pny_mc_emit: with the same sigma_dev, dims_host, iso and workspace, writes vertices_dev (n_vertices, 3) fp32 and
 *   triangles_dev (n_triangles, 3) int32, one launch each; a count of 0 launches nothing for that half (its pointer may be
 *   NULL).  Nothing is written past the counts given.
 * PNY_ERR_ARG, before any launch: a NULL pointer, a dimension below 2, 3 X Y Z >= 2^31, a non-finite iso; for pny_mc_emit a
 * negative count or one above what the volume can have. */
int pny_mc_workspace_bytes(const int32_t* dims_host /* 3: X Y Z */, int64_t* bytes);
int pny_mc_count(const float* sigma_dev /* (X, Y, Z) */, const int32_t* dims_host, float iso, void* workspace_dev,
                 int32_t* counts_dev /* int32[2]: vertices, triangles */, pny_stream stream);
int pny_mc_emit(const float* sigma_dev, const int32_t* dims_host, float iso, const void* workspace_dev, int64_t n_vertices,
                int64_t n_triangles, float* vertices_dev /* (V, 3) index coordinates */, int32_t* triangles_dev /* (T, 3) */,
                pny_stream stream);

/* ---- occupancy grid: skip empty space in no-grad renders of ONE encoded object (csrc/occupancy.hip; conventions and arithmetic
 * in csrc/pny_occupancy.h).  An opt-in, approximate mode the reference does not have.  The contract: a scene with a grid
 * attached renders, on the same rays and draws, what it renders without one if the MLP's (r, g, b, sigma) at every sample the
 * grid rejects were (0, 0, 0, 0) before the composite, in both passes; the MLP runs on the kept samples only.  With no grid
 * attached pny_render enqueues exactly what it always did.
 *
 * Cells: a sigma volume of dims = {X, Y, Z} grid points (x slowest, z fastest, as the mesh extraction reads it) has
 * (X - 1, Y - 1, Z - 1) cells; flat index f = (ix (Y - 1) + iy) (Z - 1) + iz is bit f & 31 of uint32 word f >> 5; bits past the
 * last cell are 0.  A corner is occupied when !(sigma <= thresh) -- a NaN is occupied -- in sigma_dev or, when given, in
 * sigma2_dev (the same shape: the fine MLP's sigma); a cell is occupied when a cell within Chebyshev distance `dilate` (0 .. 4)
 * has an occupied corner.  Sample to cell: p_a = fmaf(z, d_a, o_a), t_a = (p_a - (float)c1_a) * (float)((double)cells_a /
 * (c2_a - c1_a)), each operation rounded to fp32; inside iff 0 <= t_a < cells_a on all axes (a NaN is outside), cell index
 * (int)t_a.  outside_empty is a flag: 0 keeps a sample outside the box [c1, c2), 1 rejects it.
 *
 * pny_occupancy_words: the uint32 words of the bitfield of a volume.
 * pny_occupancy_build: ONE launch writes bits_dev (every word by one thread: the same bits on every run) and, unless NULL,
 *   occupied_dev = the int64 number of occupied cells (zeroed on the stream first, then integer atomic adds).
 * pny_occupancy_classify: a stage entry like pny_sample_coarse: the kernels a culled pny_render runs on its (n, k) depths
 *   z_dev of rays_dev (n, 8), 16-byte aligned.  slot_dev (n, k) int32 = the rank of a kept sample among the kept samples in
 *   ascending sample order, -1 for a rejected one; kept_dev = their int64 number, left on the device.  3 launches up to 2^20
 *   samples, 5 above; n k <= 2^30.  workspace_dev: 256-byte aligned, pny_occupancy_classify_workspace_bytes(n k) bytes.
 * pny_scene_set_occupancy: the scene COPIES the bits into a buffer it owns (on `stream`); bits_dev = NULL clears the grid (the
 *   other arguments are then ignored).  Refused for a YOLO model (its aggregation weighs by objectness, not sigma) and for a
 *   grouped scene.  Whatever changes the scene's sigma clears the grid: pny_scene_encode / pny_scenes_encode,
 *   pny_scene_set_latent, pny_scene_set_latent_levels, pny_scene_set_cameras; so does pny_scene_set_groups above 1.
 *   With a grid attached each pass of pny_render is: classify, ONE host read of the kept count M (so TWO host waits per call),
 *   gather M compact rows (40 bytes each), the MLP on M points, expand.  M = 0 launches no MLP kernel.  A pny_render told to
 *   stash for a backward (pny_scene_stash_next_render) returns PNY_ERR_STATE; pny_query, pny_yolo_render and every training
 *   entry ignore the grid.
 * pny_scene_last_cull: kept and total samples of the coarse [0] and fine [1] pass of the last pny_render; all 0 when it used
 *   no grid.
 * PNY_ERR_ARG, before any launch: a NULL pointer, a dimension below 2, 3 X Y Z >= 2^31, non-finite bounds, c2 <= c1 on an
 * axis, a NaN thresh, dilate outside 0 .. 4, n < 0, k < 1, n k > 2^30, a workspace too small or misaligned. */
int pny_occupancy_words(const int32_t dims[3], int64_t* words);
int pny_occupancy_build(const float* sigma_dev /* (X, Y, Z) */, const float* sigma2_dev /* or NULL */, const int32_t dims[3],
                        float thresh, int dilate, uint32_t* bits_dev, int64_t* occupied_dev /* or NULL */, pny_stream stream);
int pny_occupancy_classify_workspace_bytes(int64_t n_samples, int64_t* bytes);
int pny_occupancy_classify(const uint32_t* bits_dev, const int32_t dims[3], const double c1[3], const double c2[3],
                           int outside_empty, const float* rays_dev, const float* z_dev, int64_t n, int k, int32_t* slot_dev,
                           int64_t* kept_dev, void* workspace_dev, int64_t workspace_bytes, pny_stream stream);
int pny_scene_set_occupancy(pny_scene* s, const uint32_t* bits_dev /* NULL clears */, const int32_t dims[3], const double c1[3],
                            const double c2[3], int outside_empty, pny_stream stream);
int pny_scene_last_cull(pny_scene* s, int64_t kept[2], int64_t total[2]);

/* ---- early ray termination: stop evaluating a no-grad ray once it is opaque (csrc/termination.hip and the segment kernels of
 * csrc/occupancy.hip; conventions and arithmetic in csrc/pny_termination.h).  An opt-in, approximate mode the reference does not
 * have; it works with or without an occupancy grid.  A pass with K samples per ray is cut into S' = min(segments, K) depth
 * segments, segment j holding the samples [floor(j K / S'), floor((j + 1) K / S')).  The transmittance T at a segment boundary is
 * the product of the composite's own (1 - alpha + 1e-10f) over the samples before it, from the masked per-sample output.  Every
 * ray is alive in segment 0; it is alive in the next segment iff it was alive and !(T < t_min) at the boundary (a NaN keeps it
 * alive; a dead ray stays dead).  A sample is evaluated iff its ray is alive in its segment and the grid, when one is attached,
 * keeps it.  The contract is the grid's: the render equals the default render with the MLP's output at every sample that was not
 * evaluated replaced by (0, 0, 0, 0) before the composite, in both passes.  With the mode off pny_render enqueues what it
 * always did.
 *
 * pny_scene_set_termination: 0 < t_min < 1 and segments in 1 .. 16 switch the mode on, t_min == 0 switches it off (segments is
 *   then ignored).  Refused (PNY_ERR_ARG): a NaN t_min, t_min outside [0, 1), segments outside 1 .. 16, a YOLO model, a grouped
 *   scene.  The setting is a rendering option: unlike the grid it survives pny_scene_encode, pny_scene_set_latent and
 *   pny_scene_set_cameras; pny_scene_set_groups above 1 switches it off.  With the mode on each pass of pny_render is, per
 *   segment: classify, ONE host read of the kept count and the alive-ray count (one wait per issued segment), gather, the MLP on
 *   the kept points, expand, transmittance update.  A pass stops issuing segments once no ray is alive.  A pny_render told to
 *   stash for a backward returns PNY_ERR_STATE; pny_query, pny_yolo_render and every training entry ignore the setting.
 * pny_scene_last_segments: the record of pass 0 (coarse) or 1 (fine) of the last pny_render: *n_issued segments were issued
 *   (0 when the pass took no culled path, 1 with only a grid attached); alive_rays[j] and kept[j] of the first min(cap, *n_issued)
 *   are written.  alive_rays and kept may be NULL with cap = 0.
 * pny_termination_update: a stage entry, model-free, allocates nothing: T_dev[ray] *= the factors of the samples
 *   [k_begin, k_end) of sample_dev (n, k, 4) at the depths z_dev (n, k) (the delta after the last sample of a ray reaches to the
 *   ray's far, rays_dev column 7); alive_dev[ray] (bytes) = alive_dev[ray] && !(T_dev[ray] < t_min); alive_count_dev, unless
 *   NULL, = the int64 number of alive rays (zeroed on the stream first, then integer atomic adds).  ONE launch.  sample_dev is
 *   16-byte aligned.
 * pny_occupancy_classify_segment: pny_occupancy_classify on the columns [k_begin, k_end) of z_dev (n, k): slot_dev is
 *   (n, k_end - k_begin).  bits_dev = NULL: every cell is occupied (dims, c1, c2 are then ignored and may be NULL).
 *   alive_dev (n bytes) or NULL: a ray whose byte is 0 rejects all its samples.  workspace_dev: 256-byte aligned,
 *   pny_occupancy_classify_workspace_bytes(n (k_end - k_begin)) bytes.
 * PNY_ERR_ARG, before any launch: a NULL pointer, n < 0, k < 1, a column range outside 0 <= k_begin < k_end <= k, n k > 2^30, a
 *   NaN t_min or one outside [0, 1), a misaligned buffer, a workspace too small. */
int pny_scene_set_termination(pny_scene* s, float t_min, int segments);
int pny_scene_last_segments(pny_scene* s, int pass, int64_t* alive_rays, int64_t* kept, int cap, int* n_issued);
int pny_termination_update(const float* rays_dev, const float* z_dev, const float* sample_dev, int64_t n, int k, int k_begin,
                           int k_end, float t_min, float* T_dev, uint8_t* alive_dev, int64_t* alive_count_dev, pny_stream stream);
int pny_occupancy_classify_segment(const uint32_t* bits_dev /* or NULL */, const int32_t dims[3], const double c1[3],
                                   const double c2[3], int outside_empty, const float* rays_dev, const float* z_dev, int64_t n,
                                   int k, int k_begin, int k_end, const uint8_t* alive_dev /* or NULL */, int32_t* slot_dev,
                                   int64_t* kept_dev, void* workspace_dev, int64_t workspace_bytes, pny_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PNYOLO_H */
