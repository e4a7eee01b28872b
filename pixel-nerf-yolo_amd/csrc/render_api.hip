// C entry points that evaluate the MLP (include/pnyolo.h): pny_query, the render stages, pny_render / pny_yolo_render and the
// latent projection, with the one place that decides which kernel a launch runs.  Host-side C++; all arithmetic of the hot
// path is in the kernels (mlp.hip, mlp_h2.hip, render_kernels.hip, occupancy.hip, termination.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "api_internal.h"

using namespace pny;

// ---------------------------------------------------------------------------------- MLP launch
namespace pny {
int check_ready(pny_scene* s, const char* who) {
    if (!s) return fail(PNY_ERR_ARG, std::string(who) + ": null scene");
    if (!s->m->finalized) return fail(PNY_ERR_STATE, std::string(who) + ": weights not finalized (pny_model_finalize)");
    // f16-range guard: scenes pinned to F32 neither cause nor suffer from it (weights beyond the f16 range are legal there)
    const unsigned bits = s->precision == PNY_PRECISION_F32 ? 0u : range_bits(s->m);
    if (bits) {
        if (bits & PNY_RANGE_WEIGHT) s->m->f16_weights_ok = false;   // AUTO scenes run F32 from here on
        return fail(PNY_ERR_RANGE, std::string(who) + ": an earlier f16 (F16X2 / F16) launch left the f16 range (" +
                                       std::string(bits & PNY_RANGE_ACTIVATION ? "activation " : "") +
                                       std::string(bits & PNY_RANGE_GRADIENT ? "gradient " : "") +
                                       std::string(bits & PNY_RANGE_WEIGHT ? "weight " : "") +
                                       "beyond +-65504 or not finite): its results are invalid.  Clear with pny_model_range_status(m, 0, 1), pin "
                                       "pny_scene_set_precision(s, PNY_PRECISION_F32) and repeat the call");
    }
    if (!s->have_latent) return fail(PNY_ERR_STATE, std::string(who) + ": scene has no latent (pny_scene_encode / pny_scene_set_latent)");
    if (!s->have_cams) return fail(PNY_ERR_STATE, std::string(who) + ": scene has no cameras (pny_scene_set_cameras)");
    if (s->cam_ns != s->ns) return fail(PNY_ERR_STATE, std::string(who) + ": camera count != latent view count");
    if (s->n_objs > 1 && s->ns % s->n_objs)
        return fail(PNY_ERR_STATE, std::string(who) + ": grouped scene: the view count is not a multiple of the object count");
    if (obj_views(s) > 1 && s->m->desc.combine_layer >= s->m->desc.n_blocks)
        return fail(PNY_ERR_ARG, std::string(who) + ": multi-view scene needs combine_layer < n_blocks");
    return 0;
}

int view_blocks(const pny_model_desc& d) { return d.combine_layer < d.n_blocks ? d.combine_layer : d.n_blocks; }

double mlp_flops_per_point(const pny_model_desc& d, int ns, MlpPass pass) {
    const int nvb = view_blocks(d);
    const double per_view = (pass == PASS_CHAIN ? 0.0 : (double)d_in(d) * HID) +
                            (pass == PASS_FORWARD ? (double)nvb * d.d_latent * HID : 0.0) + 2.0 * nvb * HID * HID;
    const double post = 2.0 * (d.n_blocks - nvb) * HID * HID + (double)HID * d.d_out;
    const double once = pass == PASS_FORWARD_VIEW_MEAN ? (double)(ns - 1) * HID * HID : 0.0;   // fc_1 GEMMs that do not run
    return 2.0 * (ns * per_view + post - once);
}
}  // namespace pny

// ---------------------------------------------------------------------------------- routing
// Which kernel an MLP launch runs and on which latent, decided here and nowhere else (run_mlp launches what it says,
// ensure_projection projects when and how it says).  The rules are those of include/pnyolo.h pny_scene_set_precision /
// pny_scene_set_projection:
//   * f16 kernels read the projected latent only, exist for the shapes mlp_h2_supports accepts, and are never taken by a scene
//     pinned to F32.  Weights beyond the f16 range (f16_weights_ok false) keep every scene but one pinned to F16X2 off them.
//   * Single-plane f16 wherever the split kernel would run: no-grad launches of F16 and F16_TRAIN scenes, stashing (training)
//     forwards of F16_TRAIN scenes only -- an F16 scene trains as AUTO, on the split kernel.
//   * A plain launch is projected when the scene's mode says so; AUTO projects every launch of a scene whose launches can run
//     f16 (f16_default below), else launches of at least 2 x hl x wl points.  A stashing forward ignores the mode: it forces
//     the projection when it can run f16 (which there also needs L % 128 == 0), and otherwise runs fp32 on the raw latent.
//   * f16_default differs from "can run f16" in one case, on purpose: an F16X2 scene of a model whose weights left the f16 range
//     runs the split kernel where it is projected, but AUTO projection keeps the 2 x hl x wl threshold and the projection
//     itself stays on the fp32 matrix path.
//   * Split f16 on 32-sample tiles (mlp_h2s.hip: 4-wave workgroups, two per CU, the same arithmetic per sample bit for bit)
//     only for no-grad split-f16 launches of at most 32 x CUs points.  Measured (profiles/r02zk_split_sweep.log): a launch
//     that gives every CU at most ONE 32-sample tile takes 0.40-0.43 ms against 0.47-0.51 ms on 64-sample tiles; as soon as
//     two workgroups share a CU the doubled weight stream per sample costs more than the overlap of their phases returns (full
//     C2 frame: 61.7 vs 39.9 ms per launch).  PNYOLO_H2_SPLIT=0|1 overrides.
//   * PNYOLO_GRID (diagnostic: fewer resident workgroups) caps plain launches only.  Both variables are read at every call.
enum MlpKernel { K_F32_8x64 = MLP_8x64, K_F32_16x64 = MLP_16x64, K_F32_8x32 = MLP_8x32, K_H2, K_H2S, K_H1 };
struct MlpRoute {
    MlpKernel kernel;
    Prec prec;        // its arithmetic
    bool stash;       // STASH instantiation: writes the backward's operands into the model-level reservation
    bool projected;   // reads the projected latent maps
    int tile;         // samples per workgroup tile
    int grid_cap;     // resident workgroups
};

static bool f16_default(const pny_scene* s) {
    const pny_model* m = s->m;
    return s->precision != PNY_PRECISION_F32 && m->f16_weights_ok && mlp_h2_supports(m->desc.n_blocks, m->desc.combine_layer);
}

// whether a launch of n_points reads projected maps (force: whatever the scene's mode says)
static bool wants_projection(const pny_scene* s, long long n_points, bool force) {
    if (!s->m->has_zproj) return false;
    // 32-bit tap offsets, in BYTES in the f16 kernels' wave-owned gather (mlp_h2.hip h2wave_issue: one buffer resource per
    // view's map): a view's map stays under 4 GiB, larger ones stay direct
    if ((long long)s->hl * s->wl * view_blocks(s->m->desc) * HID >= (1ll << 30)) return false;
    if (force) return true;
    if (s->zp_mode == PNY_PROJECTION_OFF) return false;
    return s->zp_mode != PNY_PROJECTION_AUTO || f16_default(s) || n_points >= 2ll * s->hl * s->wl;
}

// stash: a stashing forward was asked for AND the reservation has room for it (otherwise the plain forward runs)
static MlpRoute route_mlp(const pny_scene* s, long long n_points, bool stash) {
    const pny_model_desc& d = s->m->desc;
    const int prec = s->precision;
    const bool can_f16 = prec != PNY_PRECISION_F32 && (s->m->f16_weights_ok || prec == PNY_PRECISION_F16X2) &&
                         mlp_h2_supports(d.n_blocks, d.combine_layer) && (!stash || s->L % 128 == 0);
    MlpRoute r;
    r.stash = stash;
    r.projected = stash ? can_f16 && wants_projection(s, n_points, true) : wants_projection(s, n_points, false);
    const bool f16 = r.projected && can_f16;
    const bool h1 = f16 && (prec == PNY_PRECISION_F16_TRAIN || (prec == PNY_PRECISION_F16 && !stash));
    bool h2s = f16 && !h1 && !stash && n_points <= 32ll * mlp_max_grid(MLP_8x64);
    if (f16 && !h1 && !stash)
        if (const char* e = getenv("PNYOLO_H2_SPLIT")) h2s = atoi(e) != 0;
    const int shape = (f16 || stash) ? MLP_8x64 : mlp_pick_variant(n_points);   // (the STASH instantiations are 8x64)
    r.kernel = h1 ? K_H1 : h2s ? K_H2S : f16 ? K_H2 : MlpKernel(shape);
    r.prec = h1 ? PREC_H1 : f16 ? PREC_H2 : PREC_F32;
    r.tile = h2s ? 32 : mlp_tile_samples(shape);
    r.grid_cap = h2s ? 2 * mlp_max_grid(MLP_8x64) : mlp_max_grid(shape);
    if (!stash)
        if (const char* e = getenv("PNYOLO_GRID")) {
            const int g = atoi(e);
            if (g > 0 && g < r.grid_cap) r.grid_cap = g;
        }
    return r;
}

// Projected latent: zp[v][y][x][b*512 + n] = sum_k lin_z[b].weight[n][k] * latent[v][y][x][k], computed
// once per (scene latent, weights) on the caller's stream and cached.  AUTO (wants_projection): with the f16x2 kernel
// available every launch is projected -- a lone 64-sample tile on it (0.5 ms) beats the 32-sample fp32 shape on the
// unprojected latent (1.0 ms) even with the one-off projection of the scene (0.3 ms per MLP at C2), and a ray's result then
// never depends on the size of the batch it is rendered in.  Without it (F32 scenes, more than 6 blocks): when the launch
// has at least twice as many points as the latent has pixels per view (the projection costs one lin_z per PIXEL instead of
// one per (sample, view); tiny training-size batches on large maps stay direct).
namespace pny {
// The projection itself, for the cache below and for the read-out (pny_scene_projection): MLP `which`'s stacked lin_z applied
// to every pixel of the scene's latent, into out (ns hl wl, view blocks x 512).  Scenes whose projected launches run the f16x2
// kernel project on the split-f16 matrix path too.  route: see run_pixel_linear.
static int project_latent(const pny_scene* s, int which, float* out, hipStream_t st, int* route) {
    const pny_model* m = s->m;
    if (!m->desc.has_fine) which = 0;
    const long long npix = (long long)s->ns * s->hl * s->wl;
    if (!run_pixel_linear(m->zproj[which], s->latent.f(), npix, out, st, f16_default(s), route))
        return fail(PNY_ERR_HIP, "latent projection launch failed");
    return 0;
}

int ensure_projection(pny_scene* s, int which, long long n_points, hipStream_t st, const float** zp, bool force) {
    *zp = nullptr;
    const pny_model* m = s->m;
    if (!wants_projection(s, n_points, force)) return 0;
    const int nvb = view_blocks(m->desc);
    if (s->zp_generation != m->generation) {
        s->zp_valid[0] = s->zp_valid[1] = false;
        s->zp_generation = m->generation;
    }
    if (!m->desc.has_fine) which = 0;
    if (!s->zp_valid[which]) {
        const long long npix = (long long)s->ns * s->hl * s->wl;
        int rc;
        if ((rc = s->zp[which].reserve((size_t)npix * nvb * HID * sizeof(float)))) return rc;
        if ((rc = project_latent(s, which, s->zp[which].f(), st, nullptr))) return rc;
        s->zp_valid[which] = true;
    }
    *zp = s->zp[which].f();
    return 0;
}

int fill_mlp_args(pny_scene* s, int mode, const float* xyz, const float* dirs, const float* rays, const float* z, int K,
                  long long n_points, int coarse, float* out, MlpArgs* pa) {
    const pny_model_desc& d = s->m->desc;
    MlpArgs& a = *pa;
    memset(&a, 0, sizeof(a));
    const bool fine_w = mlp_index(s->m, coarse) == 1;
    a.w = fine_w ? s->m->fine : s->m->coarse;
    a.n_blocks = d.n_blocks;
    use_images(a, f16_images(s->m, fine_w, false));   // (in the packed blob, like `w`)
    a.range_flag = s->m->range_flag();
    a.latent = s->latent.f();
    a.zp = nullptr;
    a.zp_stride = view_blocks(d) * HID;
    a.tap_stride = s->L;
    memcpy(a.cams, s->cams, sizeof(Cam) * (size_t)s->ns);
    a.xyz = xyz;
    a.dirs = dirs;
    a.rays = rays;
    a.z = z;
    a.out = out;
    a.n_points = n_points;
    a.K = K;
    a.mode = mode;
    a.NS = obj_views(s);
    a.obj_pts = 0;
    if (s->n_objs > 1) {   // grouped scene: equal consecutive shares, whole tiles per object (pny_scene_set_groups)
        if (n_points % s->n_objs || (n_points / s->n_objs) % 64)
            return fail(PNY_ERR_ARG, "grouped scene: every object's share of the samples must be the same multiple of 64");
        a.obj_pts = n_points / s->n_objs;
    }
    a.L = s->L;
    a.Hl = s->hl;
    a.Wl = s->wl;
    a.combine_layer = d.combine_layer;
    a.d_out = d.d_out;
    a.yolo = d.yolo;
    a.num_freqs = d.num_freqs;
    a.freq_factor = d.freq_factor;
    // latent_scaling / image_size in fp32 (reference encoder.py:97,170-172)
    const float lsx = (float)s->wl / ((float)s->wl - 1.0f) * 2.0f;
    const float lsy = (float)s->hl / ((float)s->hl - 1.0f) * 2.0f;
    a.sx = lsx / (float)s->width;
    a.sy = lsy / (float)s->height;
    const long long tiles = (n_points + 63) / 64;
    if (tiles > 0x7fffffffll) return fail(PNY_ERR_ARG, "too many points for one launch");
    a.n_tiles = (int)tiles;
    a.idx32 = (tiles * 64) < 0xffffffffll;
    if (mode == 1 && (reinterpret_cast<uintptr_t>(rays) & 15)) return fail(PNY_ERR_ARG, "rays must be 16-byte aligned");
    int rc;
    if ((rc = s->scratch.reserve(mlp_scratch_floats() * sizeof(float)))) return rc;
    a.scratch = s->scratch.f();
    return 0;
}
}  // namespace pny

// One MLP evaluation of a query / render call.  stash_pass (pny_scene_stash_next_render; 0 coarse, 1 fine pass of the
// render): the training forward -- the STASH instantiation of the routed kernel (64-sample tiles) writes every GEMM operand
// into the tiles this pass takes from the model-level reservation, and the backward of the same reservation epoch then
// starts at the dX chain (the f16 instantiations read the projected latent for the forward and gather the raw latent once more
// per view for lin_z's weight gradient; the same stash layout and contents).  Without room in the reservation the plain
// forward runs and the backward recomputes.
static int run_mlp(pny_scene* s, int mode, const float* xyz, const float* dirs, const float* rays, const float* z,
                   int K, long long n_points, int coarse, float* out, hipStream_t st, int stash_pass = -1) {
    if (n_points == 0) return 0;
    pny_model* m = s->m;
    const pny_model_desc& d = m->desc;
    MlpArgs a;
    int rc;
    if ((rc = fill_mlp_args(s, mode, xyz, dirs, rays, z, K, n_points, coarse, out, &a))) return rc;
    const int which = mlp_index(m, coarse);
    bool room = false;
    if (stash_pass >= 0) {
        s->stashed[stash_pass].valid = false;
        room = m->stash.book.has_room(which, obj_views(s), a.n_tiles);
    }
    const MlpRoute r = route_mlp(s, n_points, room);
    if (r.stash) {
        const StashedPass& sp = s->stashed[stash_pass] = m->stash.book.take_pass(which, a.n_tiles, n_points);
        a.lay = stash_layout(d, obj_views(s), s->L);
        a.stash_x = m->stash.x_record(a.lay, which, sp.tile0);
    }
    if (r.projected) {
        if ((rc = ensure_projection(s, which, n_points, st, &a.zp, r.stash))) return rc;
        a.tap_stride = a.zp_stride;
    }
    if (r.kernel == K_H1) {   // (F16_TRAIN scenes: the same no-grad kernel as F16's, so their no-grad results are F16's bit for bit)
        if ((rc = want_h1_images(m, s->precision == PNY_PRECISION_F16_TRAIN))) return rc;
        use_images(a, f16_images(m, which == 1, true));
    }
    const long long tiles = (n_points + r.tile - 1) / r.tile;
    if (tiles > 0x7fffffffll) return fail(PNY_ERR_ARG, "too many points for one launch");
    a.n_tiles = (int)tiles;
    a.idx32 = (tiles * r.tile) < 0xffffffffll;
    const int grid = (int)std::min<long long>(r.grid_cap, tiles);
    if ((rc = stamp_event(s->timing, s->ev, s->ev_used, st))) return rc;
    switch (r.kernel) {
    case K_H1: (r.stash ? launch_mlp_h1_stash : launch_mlp_h1)(a, grid, st); break;
    case K_H2: (r.stash ? launch_mlp_h2_stash : launch_mlp_h2)(a, grid, st); break;
    case K_H2S: launch_mlp_h2s(a, grid, st); break;
    default:
        if (r.stash)
            launch_mlp_stash(a, grid, st);
        else
            launch_mlp(a, r.kernel, grid, st);
    }
    PNY_HIP(hipGetLastError());
    if ((rc = stamp_event(s->timing, s->ev, s->ev_used, st))) return rc;
    s->last_prec = r.prec;
    s->last_projected = r.projected;
    // executed FLOPs: the non-stashing split-f16 kernels run the last per-view fc_1 once, on the mean over views (mlp_h2.hip)
    const bool view_mean = !r.stash && (r.kernel == K_H2 || r.kernel == K_H2S);
    s->last_flops += mlp_flops_per_point(d, obj_views(s), view_mean ? PASS_FORWARD_VIEW_MEAN : r.projected ? PASS_FORWARD_PROJECTED : PASS_FORWARD) *
                     (double)n_points;
    s->last_flops_ref += mlp_flops_per_point(d, obj_views(s), PASS_FORWARD) * (double)n_points;
    s->last_launches += 1;
    return 0;
}

static void begin_call(pny_scene* s) {
    s->ev_used = 0;
    s->last_flops = 0.0;
    s->last_flops_ref = 0.0;
    s->last_launches = 0;
}

// One MLP pass of a pny_render with an occupancy grid attached (pny_occupancy.h): classify the n x K depth samples, read the
// kept count M (the pass's ONE host wait), gather the kept samples' points into M compact rows, evaluate the MLP on them as a
// point list (pny_query's launch) and expand into `samp` (n, K, 4), a rejected sample getting (0, 0, 0, 0).  M == 0 launches
// no MLP kernel.
static int culled_mlp(pny_scene* s, const float* rays, const float* z, int64_t n, int K, int coarse, float* samp, hipStream_t st,
                      int pass) {
    const int64_t S = n * K;
    if (n > OCC_MAX_SAMPLES / K) return fail(PNY_ERR_ARG, "pny_render: more than 2^30 samples in a pass with an occupancy grid attached");
    if (reinterpret_cast<uintptr_t>(samp) % 16)
        return fail(PNY_ERR_ARG, "pny_render: per-sample buffers must be 16-byte aligned with an occupancy grid attached");
    int rc;
    const OccLayout l = occ_layout(S);
    const size_t o_sums = mc_align((size_t)S * sizeof(int32_t)), o_kept = o_sums + l.bytes;
    if ((rc = s->occ_work.reserve(o_kept + 256, "hipMalloc(occupancy workspace)"))) return rc;
    if ((rc = s->occ_count.reserve(sizeof(int64_t), "hipHostMalloc(occupancy count)"))) return rc;
    char* W = reinterpret_cast<char*>(s->occ_work.p);
    int32_t* slot = reinterpret_cast<int32_t*>(W);
    int64_t* kept_dev = reinterpret_cast<int64_t*>(W + o_kept);
    occupancy_classify(s->occ, rays, z, S, K, slot, kept_dev, W + o_sums, st);
    PNY_HIP(hipGetLastError());
    PNY_HIP(hipMemcpyAsync(s->occ_count.p, kept_dev, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PNY_HIP(hipStreamSynchronize(st));
    const int64_t M = *static_cast<const int64_t*>(s->occ_count.p);
    if (M < 0 || M > S) return fail(PNY_ERR_HIP, "pny_render: the occupancy classification returned an impossible count");
    s->cull_kept[pass] = M, s->cull_total[pass] = S;
    float* outc = nullptr;
    if (M > 0) {
        const size_t m3 = ((size_t)M * 3 + 63) & ~(size_t)63;
        if ((rc = s->occ_rows.reserve((2 * m3 + (size_t)M * 4) * sizeof(float), "hipMalloc(occupancy rows)"))) return rc;
        float* xyz = s->occ_rows.f();
        float* dirs = xyz + m3;
        outc = dirs + m3;
        launch_occupancy_gather(slot, rays, z, S, K, M, xyz, dirs, st);
        PNY_HIP(hipGetLastError());
        if ((rc = run_mlp(s, 0, xyz, dirs, nullptr, nullptr, 1, M, coarse, outc, st))) return rc;
    }
    launch_occupancy_expand(slot, outc, S, M, samp, st);
    PNY_HIP(hipGetLastError());
    s->seg_issued[pass] = 1, s->seg_alive[pass][0] = n, s->seg_kept[pass][0] = M;
    return 0;
}

// One MLP pass of a pny_render with early ray termination on (pny_termination.h), with or without a grid: the pass in
// S' = min(segments, K) depth segments.  Per segment: classify its columns for the rays still alive, read the kept count M and
// the alive-ray count together (the segment's ONE host wait), gather, the MLP on M points, expand into the segment's columns of
// `samp`, then multiply the rays' carried T by the segment's factors and clear the alive bytes of the rays below t_min (not
// after the last segment: nothing reads it).  Once no ray is alive the remaining columns are zeroed and no further segment is
// issued.  The workspace is sized by the largest segment and reused.
static int terminated_mlp(pny_scene* s, const float* rays, const float* z, int64_t n, int K, int coarse, float* samp, hipStream_t st,
                          int pass) {
    if (n > OCC_MAX_SAMPLES / K) return fail(PNY_ERR_ARG, "pny_render: more than 2^30 samples in a pass with early ray termination on");
    if (reinterpret_cast<uintptr_t>(samp) % 16)
        return fail(PNY_ERR_ARG, "pny_render: per-sample buffers must be 16-byte aligned with early ray termination on");
    int rc;
    const int Sp = term_segments(K, s->term_segments);
    const int ks_max = (K + Sp - 1) / Sp;
    const int64_t s_max = n * ks_max;
    const size_t o_sums = mc_align((size_t)s_max * sizeof(int32_t)), o_counts = o_sums + occ_layout(s_max).bytes;
    const size_t o_T = o_counts + 256, o_alive = o_T + mc_align((size_t)n * sizeof(float));
    if ((rc = s->occ_work.reserve(o_alive + mc_align((size_t)n), "hipMalloc(termination workspace)"))) return rc;
    if ((rc = s->occ_count.reserve(2 * sizeof(int64_t), "hipHostMalloc(termination counts)"))) return rc;
    char* W = reinterpret_cast<char*>(s->occ_work.p);
    int32_t* slot = reinterpret_cast<int32_t*>(W);
    int64_t* counts_dev = reinterpret_cast<int64_t*>(W + o_counts);   // [0] kept samples of the segment, [1] alive rays in it
    float* T = reinterpret_cast<float*>(W + o_T);
    uint8_t* alive = reinterpret_cast<uint8_t*>(W + o_alive);
    OccGrid g = s->occ;
    if (!s->occ_on) g.bits = nullptr;
    const float one = 1.0f;
    uint32_t one_bits;
    memcpy(&one_bits, &one, sizeof(one_bits));
    PNY_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T), (int)one_bits, (size_t)n, st));
    PNY_HIP(hipMemsetAsync(alive, 1, (size_t)n, st));
    int64_t kept_total = 0;
    s->cull_total[pass] = n * K;
    for (int j = 0; j < Sp; ++j) {
        const int kb = term_bound(K, Sp, j), ke = term_bound(K, Sp, j + 1);
        const int64_t Sj = n * (ke - kb);
        occupancy_classify_segment(g, rays, z, n, K, kb, ke, alive, slot, counts_dev, W + o_sums, st);
        PNY_HIP(hipGetLastError());
        // (segment 0: every ray is alive, no update has counted yet)
        PNY_HIP(hipMemcpyAsync(s->occ_count.p, counts_dev, (j ? 2 : 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PNY_HIP(hipStreamSynchronize(st));
        const int64_t M = static_cast<const int64_t*>(s->occ_count.p)[0], A = j ? static_cast<const int64_t*>(s->occ_count.p)[1] : n;
        if (M < 0 || M > Sj || A < 0 || A > n) return fail(PNY_ERR_HIP, "pny_render: the segment classification returned an impossible count");
        s->seg_alive[pass][j] = A, s->seg_kept[pass][j] = M;
        s->seg_issued[pass] = j + 1;
        kept_total += M;
        s->cull_kept[pass] = kept_total;
        if (A == 0) {   // every later sample is rejected too: columns [kb, K) of every row are zeros
            PNY_HIP(hipMemset2DAsync(samp + (size_t)kb * 4, (size_t)K * 4 * sizeof(float), 0, (size_t)(K - kb) * 4 * sizeof(float), (size_t)n, st));
            break;
        }
        float* outc = nullptr;
        if (M > 0) {
            const size_t m3 = ((size_t)M * 3 + 63) & ~(size_t)63;
            if ((rc = s->occ_rows.reserve((2 * m3 + (size_t)M * 4) * sizeof(float), "hipMalloc(occupancy rows)"))) return rc;
            float* xyz = s->occ_rows.f();
            float* dirs = xyz + m3;
            outc = dirs + m3;
            launch_occupancy_gather_segment(slot, rays, z, n, K, kb, ke, M, xyz, dirs, st);
            PNY_HIP(hipGetLastError());
            if ((rc = run_mlp(s, 0, xyz, dirs, nullptr, nullptr, 1, M, coarse, outc, st))) return rc;
        }
        launch_occupancy_expand_segment(slot, outc, n, K, kb, ke, M, samp, st);
        PNY_HIP(hipGetLastError());
        if (j + 1 < Sp) {
            PNY_HIP(hipMemsetAsync(counts_dev + 1, 0, sizeof(int64_t), st));
            TermUpdateArgs u;
            u.rays = rays, u.z = z, u.samp = samp, u.n = n, u.K = K, u.k_begin = kb, u.k_end = ke, u.t_min = s->term_t_min;
            u.T = T, u.alive = alive, u.alive_count = reinterpret_cast<unsigned long long*>(counts_dev + 1);
            launch_termination_update(u, st);
            PNY_HIP(hipGetLastError());
        }
    }
    return 0;
}

extern "C" {

int pny_query(pny_scene* s, const float* xyz_dev, const float* viewdirs_dev, int64_t n, int coarse, float* out_dev,
              pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_query"))) return rc;
    if (n < 0 || (n > 0 && (!xyz_dev || !viewdirs_dev || !out_dev))) return fail(PNY_ERR_ARG, "pny_query: bad argument");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    begin_call(s);
    return run_mlp(s, 0, xyz_dev, viewdirs_dev, nullptr, nullptr, 1, n, coarse, out_dev, (hipStream_t)stream);
}

int pny_sample_coarse(const float* rays_dev, int64_t n, int n_coarse, int lindisp, const float* u_dev, uint64_t seed,
                      float* z_dev, pny_stream stream) {
    if (n < 0 || n_coarse < 1 || (n > 0 && (!rays_dev || !z_dev))) return fail(PNY_ERR_ARG, "pny_sample_coarse: bad argument");
    launch_sample_coarse(rays_dev, n, n_coarse, lindisp, u_dev, seed, z_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_composite(const float* rays_dev, const float* z_dev, const float* sample_dev, int64_t n, int k, int white_bkgd,
                  float* weights_dev, float* rgb_dev, float* depth_dev, pny_stream stream) {
    if (n < 0 || k < 1 || (n > 0 && (!rays_dev || !z_dev || !sample_dev))) return fail(PNY_ERR_ARG, "pny_composite: bad argument");
    launch_composite(rays_dev, z_dev, sample_dev, n, k, white_bkgd, weights_dev, rgb_dev, depth_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_sample_fine(const float* rays_dev, const float* z_coarse_dev, const float* weights_dev, const float* depth_dev,
                    int64_t n, int n_coarse, int n_fine, int n_fine_depth, float depth_std, int lindisp,
                    const float* u_dev, const float* u2_dev, const float* g_dev, uint64_t seed, float* z_out_dev,
                    pny_stream stream) {
    if (n < 0 || n_coarse < 1 || n_fine < 0 || n_fine_depth < 0 || n_fine_depth > n_fine)
        return fail(PNY_ERR_ARG, "pny_sample_fine: bad sample counts");
    if (n > 0 && (!rays_dev || !z_coarse_dev || !weights_dev || !z_out_dev || (n_fine_depth > 0 && !depth_dev)))
        return fail(PNY_ERR_ARG, "pny_sample_fine: null argument");
    if ((size_t)(4 * n_coarse + 1 + 2 * n_fine) * 4 * sizeof(float) > 160 * 1024)
        return fail(PNY_ERR_ARG, "pny_sample_fine: n_coarse + n_fine too large for the LDS-resident sort");
    launch_sample_fine(rays_dev, z_coarse_dev, weights_dev, depth_dev, n, n_coarse, n_fine, n_fine_depth, depth_std,
                       lindisp, u_dev, u2_dev, g_dev, seed, z_out_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_aggregate(const float* raw_dev, int64_t n, int k, int n_anchors, float* out_dev, pny_stream stream) {
    if (n < 0 || k < 1 || n_anchors < 1 || (n > 0 && (!raw_dev || !out_dev))) return fail(PNY_ERR_ARG, "pny_yolo_aggregate: bad argument");
    launch_yolo_aggregate(raw_dev, n, k, n_anchors, out_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_render(pny_scene* s, const float* rays_dev, int64_t n, const pny_render_opts* o, const pny_render_out* out,
               pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_render"))) return rc;
    if (!o || !out || n < 0 || (n > 0 && !rays_dev)) return fail(PNY_ERR_ARG, "pny_render: bad argument");
    if (s->m->desc.yolo || s->m->desc.d_out != 4) return fail(PNY_ERR_ARG, "pny_render: model is in YOLO mode (use pny_yolo_render)");
    if (o->n_coarse < 1 || o->n_fine < 0 || o->n_fine_depth < 0 || o->n_fine_depth > o->n_fine)
        return fail(PNY_ERR_ARG, "pny_render: bad sample counts");
    const int kimp = o->n_fine - o->n_fine_depth;
    const bool any_u = o->u_coarse_dev || o->u_fine_dev || o->u_fine2_dev || o->g_depth_dev;
    if (any_u) {
        if (!o->u_coarse_dev || (kimp > 0 && (!o->u_fine_dev || !o->u_fine2_dev)) || (o->n_fine_depth > 0 && !o->g_depth_dev))
            return fail(PNY_ERR_ARG, "pny_render: explicit random draws must be given for every stage or for none");
    }
    // an occupancy grid (pny_scene_set_occupancy) is for no-grad renders: a culled pass writes no stash
    // ... and so is early ray termination (pny_scene_set_termination)
    const bool cull = s->occ_on || s->term_on;
    if (cull && s->stash_next) {
        s->stash_next = false;
        if (!s->occ_on)
            return fail(PNY_ERR_STATE, "pny_render: the scene has early ray termination on and was told to stash for a backward "
                                       "(pny_scene_stash_next_render); switch it off with pny_scene_set_termination(s, 0, 1) to train");
        return fail(PNY_ERR_STATE, "pny_render: the scene has an occupancy grid attached and was told to stash for a backward "
                                   "(pny_scene_stash_next_render); clear the grid with pny_scene_set_occupancy(s, NULL, ...) to train");
    }
    s->cull_kept[0] = s->cull_kept[1] = s->cull_total[0] = s->cull_total[1] = 0;
    s->seg_issued[0] = s->seg_issued[1] = 0;
    const auto culled_pass = s->term_on ? terminated_mlp : culled_mlp;
    if (n == 0) return PNY_OK;
    PNY_HIP(hipSetDevice(s->m->desc.device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = enter_stream(s, st))) return rc;
    begin_call(s);
    const int kc = o->n_coarse, kt = o->n_coarse + o->n_fine;
    // workspace carve (floats): z_c, samp_c, w_c, rgb_c(3)+depth_c, z_f, samp_f
    size_t off = 0;
    auto carve = [&](size_t nfl) {
        size_t r = off;
        off += (nfl + 63) & ~(size_t)63;
        return r;
    };
    const size_t o_zc = carve((size_t)n * kc), o_sc = carve((size_t)n * kc * 4), o_wc = carve((size_t)n * kc);
    const size_t o_dc = carve((size_t)n), o_rc = carve((size_t)n * 3);
    const size_t o_zf = carve((size_t)n * kt), o_sf = carve((size_t)n * kt * 4);
    if ((rc = s->work.reserve(off * sizeof(float)))) return rc;
    float* W = s->work.f();
    float* zc = out->z_coarse ? out->z_coarse : W + o_zc;
    float* sc = out->sample_coarse ? out->sample_coarse : W + o_sc;
    float* wc = out->weights_coarse ? out->weights_coarse : W + o_wc;
    float* dc = out->depth_coarse ? out->depth_coarse : W + o_dc;
    float* rgbc = out->rgb_coarse ? out->rgb_coarse : W + o_rc;

    const bool stash = s->stash_next;
    s->stash_next = false;
    s->stashed[0].valid = s->stashed[1].valid = false;
    launch_sample_coarse(rays_dev, n, kc, o->lindisp, o->u_coarse_dev, o->seed, zc, st);
    if (cull) {
        if ((rc = culled_pass(s, rays_dev, zc, n, kc, 1, sc, st, 0))) return rc;
    } else if ((rc = run_mlp(s, 1, nullptr, nullptr, rays_dev, zc, kc, (long long)n * kc, 1, sc, st, stash ? 0 : -1))) {
        return rc;
    }
    launch_composite(rays_dev, zc, sc, n, kc, o->white_bkgd, wc, rgbc, dc, st, o->sigma_noise_coarse_dev);
    if (o->n_fine > 0) {
        float* zf = out->z_fine ? out->z_fine : W + o_zf;
        float* sf = out->sample_fine ? out->sample_fine : W + o_sf;
        if ((size_t)(4 * kc + 1 + 2 * o->n_fine) * 4 * sizeof(float) > 160 * 1024)
            return fail(PNY_ERR_ARG, "pny_render: n_coarse + n_fine too large for the LDS-resident sort");
        launch_sample_fine(rays_dev, zc, wc, dc, n, kc, o->n_fine, o->n_fine_depth, o->depth_std, o->lindisp,
                           o->u_fine_dev, o->u_fine2_dev, o->g_depth_dev, o->seed, zf, st);
        if (cull) {
            if ((rc = culled_pass(s, rays_dev, zf, n, kt, 0, sf, st, 1))) return rc;
        } else if ((rc = run_mlp(s, 1, nullptr, nullptr, rays_dev, zf, kt, (long long)n * kt, 0, sf, st, stash ? 1 : -1))) {
            return rc;
        }
        launch_composite(rays_dev, zf, sf, n, kt, o->white_bkgd, out->weights_fine, out->rgb_fine, out->depth_fine, st,
                         o->sigma_noise_fine_dev);
    }
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_render(pny_scene* s, const float* rays_dev, int64_t n, int n_coarse, const float* u_coarse_dev,
                    uint64_t seed, float* out_dev, float* raw_dev, pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_yolo_render"))) return rc;
    const pny_model_desc& d = s->m->desc;
    if (!d.yolo || d.d_out % 7) return fail(PNY_ERR_ARG, "pny_yolo_render: model is not in YOLO mode");
    if (n < 0 || n_coarse < 1 || (n > 0 && (!rays_dev || !out_dev))) return fail(PNY_ERR_ARG, "pny_yolo_render: bad argument");
    if (n == 0) return PNY_OK;
    PNY_HIP(hipSetDevice(d.device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = enter_stream(s, st))) return rc;
    begin_call(s);
    const size_t nz = ((size_t)n * n_coarse + 63) & ~(size_t)63;
    if ((rc = s->work.reserve((nz + (size_t)n * n_coarse * d.d_out) * sizeof(float)))) return rc;
    float* z = s->work.f();
    float* raw = raw_dev ? raw_dev : s->work.f() + nz;
    launch_sample_coarse(rays_dev, n, n_coarse, 0, u_coarse_dev, seed, z, st);
    if ((rc = run_mlp(s, 1, nullptr, nullptr, rays_dev, z, n_coarse, (long long)n * n_coarse, 1, raw, st))) return rc;
    launch_yolo_aggregate(raw, n, n_coarse, d.d_out / 7, out_dev, st);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_scene_project(pny_scene* s, pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_scene_project"))) return rc;
    if (!s->m->has_zproj) return PNY_OK;  // no per-view blocks: nothing to project
    if (s->zp_mode == PNY_PROJECTION_OFF) return fail(PNY_ERR_STATE, "pny_scene_project: projection is switched off for this scene");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    const int keep = s->zp_mode;
    s->zp_mode = PNY_PROJECTION_ON;
    const float* zp = nullptr;
    rc = ensure_projection(s, 0, 0, (hipStream_t)stream, &zp);
    if (!rc && s->m->desc.has_fine && s->m->use_fine) rc = ensure_projection(s, 1, 0, (hipStream_t)stream, &zp);
    s->zp_mode = keep;
    if (rc) return rc;
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_scene_projection(pny_scene* s, int fine, float* out_dev, int64_t out_floats, int* route, pny_stream stream) {
    if (!s || !out_dev) return fail(PNY_ERR_ARG, "pny_scene_projection: null argument");
    const pny_model* m = s->m;
    if (!m->finalized) return fail(PNY_ERR_STATE, "pny_scene_projection: weights not finalized (pny_model_finalize)");
    if (!m->has_zproj) return fail(PNY_ERR_ARG, "pny_scene_projection: the model has no per-view blocks, nothing is projected");
    if (!s->have_latent) return fail(PNY_ERR_STATE, "pny_scene_projection: scene has no latent (pny_scene_encode / pny_scene_set_latent)");
    const long long need = (long long)s->ns * s->hl * s->wl * view_blocks(m->desc) * HID;
    if (out_floats < need)
        return fail(PNY_ERR_ARG, "pny_scene_projection: out_dev holds " + std::to_string((long long)out_floats) + " floats, the maps need " +
                                     std::to_string(need));
    PNY_HIP(hipSetDevice(m->desc.device));
    int rc;
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    int launched = 0;
    if ((rc = project_latent(s, fine ? 1 : 0, out_dev, (hipStream_t)stream, &launched))) return rc;
    if (route) *route = launched;
    return PNY_OK;
}

}  // extern "C"
