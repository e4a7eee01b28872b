// Private declarations shared by the host-side translation units of libpnyolo (the *_api.hip files).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "pny_common.h"
#include "dev_resource.h"
#include "encoder.h"
#include "pny_occupancy.h"
#include "pny_termination.h"
#include "stash_book.h"

namespace pny {

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

// One packed sub-buffer of the model and how to build it from the state_dict tensor(s) it comes from (pack.hip): recorded by
// pny_model_finalize, which runs it on uploaded copies of the tensors; pny_model_refresh runs it on the live parameters.
struct RepackEntry {
    int kind;
    std::string name, name2;
    size_t dst_off;      // float offset in the packed blob ...
    float* dst_abs;      // ... or an absolute device pointer (projection weights)
    int n_out, k_in, k_pad, count;
};

// planes per operand of the f16 weight- and latent-gradient GEMMs (ignored by their fp32 paths)
inline int gemm_planes(Prec p) { return p == PREC_H1 ? 1 : 2; }

// Deferred weight gradients (pny_model_defer_weight_grads): the reservation a training pny_render writes the GEMM operands into,
// every scene's backward appends its dY tiles to, and pny_model_flush_weight_grads turns into ONE weight-gradient GEMM per MLP
// ([0] mlp_coarse, [1] mlp_fine).  `book` does the counting (stash_book.h); the buffers are addressed through the accessors.
struct DeferredStash {
    StashBook book;
    DevBuf x[2], dy[2];                      // the GEMMs' B operands / the dY tiles, book.cap[w] records of the stash layout
    DevBuf partial[2], bias[2], tables[2];   // the flush GEMM's split partial sums and its work list
    PinnedStage stage[2];
    DevBuf absmax;                           // two words: running max |dY| of the deferred tiles per MLP (zeroed by its flush)
    Event flush_ev[4];                       // timing events around each MLP's flush GEMM
    double flush_flops = 0.0;                // pny_model_last_flush_stats
    int flush_launches = 0;
    Prec last_flush_prec = PREC_F32;         // pny_model_last_flush_precision: the flush's GEMM
    float* x_record(const StashLayout& lay, int which, long long tile) const { return lay.x_record(x[which].f(), tile); }
    float* dy_record(const StashLayout& lay, int which, long long tile) const { return lay.dy_record(dy[which].f(), tile); }
    unsigned* absmax_word(int which) const { return absmax.p ? reinterpret_cast<unsigned*>(absmax.p) + which : nullptr; }
};

// One set of f16 operand images of an MLP and the allocation they live in (raw-buffer addressing): lin_in / fc_0 / fc_1 as the
// forward kernels read them (mlp_h2.hip, mlp_h1.hip) and lin_out / fc_0 / fc_1 transposed for the backward chain
// (mlp_bwd_h2.hip, mlp_bwd_h1.hip).  Either the split-f16 images (MlpWeightsT::h2, in the model's packed blob) or the
// single-plane ones (pny_model::h1, a buffer of their own).
struct F16Images {
    const float* in;
    const float* fc0[MAX_BLOCKS];
    const float* fc1[MAX_BLOCKS];
    const float* out;         // lin_out for the forward's split-K product (PACK_H2O; split-f16 images only)
    const float* T_out;
    const float* T_fc0[MAX_BLOCKS];
    const float* T_fc1[MAX_BLOCKS];
    const float* base;
    size_t bytes;
};

// transposed packed weights of one MLP (A operands of the backward chain, mlp_bwd.hip)
struct MlpWeightsT {
    const float* w_in_plain;  // lin_in.weight as stored (512, d_in): input gradients (mlp_bwd.hip mlp_dz_kernel)
    const float* wT_out;
    const float* wT_fc0[MAX_BLOCKS];
    const float* wT_fc1[MAX_BLOCKS];
    const float* wzT_cat;     // [lin_z[0]^T | lin_z[1]^T | ...] (d_latent x n_view_blocks * 512), n-tile-major (latent_grad.hip)
    F16Images h2;             // split-f16 images (pack.hip PACK_H2 / PACK_H2T)
};

// the launch's f16 operand images (and the allocation the kernel addresses them in)
inline void use_images(MlpArgs& a, const F16Images& im) {
    a.w_base = im.base;
    a.w_bytes = (unsigned)im.bytes;
    a.h2_in = im.in;
    a.h2_out = im.out;
    for (int b = 0; b < a.n_blocks; ++b) {
        a.h2_fc0[b] = im.fc0[b];
        a.h2_fc1[b] = im.fc1[b];
    }
}
inline void use_images(BwdArgs& a, const F16Images& im) {
    a.w_base = im.base;
    a.w_bytes = (unsigned)im.bytes;
    a.h2T_out = im.T_out;
    for (int b = 0; b < a.n_blocks; ++b) {
        a.h2T_fc0[b] = im.T_fc0[b];
        a.h2T_fc1[b] = im.T_fc1[b];
    }
}

// Kernel timing (pny_scene_enable_timing): records the next event of `ev` on `st`, creating it on first use.  A timed launch
// is bracketed by two calls.
inline int stamp_event(bool timing, std::vector<Event>& ev, int& used, hipStream_t st) {
    if (!timing) return 0;
    if ((int)ev.size() <= used) {
        Event e;
        if (int rc = e.ensure(hipEventDefault, "hipEventCreate(timing)")) return rc;
        ev.push_back(std::move(e));
    }
    PNY_HIP(hipEventRecord(ev[used++], st));
    return 0;
}

// The first step of every handle's destroy entry.  Pinned blocks and job tables may still be read by queued copies and
// kernels, and freeing pinned memory waits for nothing: the device is drained before any member is released, so that no
// order of members or of their destructors is what keeps that safe.  Like every other entry point it makes the handle's
// device the calling thread's current one (the model's and the scene's destroy did not before).
inline void drain_device(int device) {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
}

}  // namespace pny

namespace pny {
struct TrunkTrain;                       // training-mode trunk: saved activations and scratch (encoder_train.hip)
void trunk_release(TrunkTrain* t);       // after the model's drain_device
void trunk_params_rebound(TrunkTrain* t);   // a trunk parameter was bound to new storage: re-resolve its pointers
}  // namespace pny

using namespace pny;  // private header of host-side translation units only

struct pny_model {
    pny_model_desc desc;
    std::map<std::string, HostTensor> host;  // state_dict tensors as loaded
    bool finalized = false;
    bool use_fine = true;
    DevBuf packed;                            // all MLP weights, one allocation
    MlpWeights coarse{}, fine{};
    MlpWeightsT coarse_t{}, fine_t{};        // transposed packs for the backward chain
    std::map<std::string, float*> grads;     // gradient targets by state_dict name (pny_model_bind_grad)
    std::map<std::string, const float*> params_dev;  // live parameter tensors on the device (pny_model_bind_param)
    std::vector<RepackEntry> repack;
    DevBuf repack_jobs;
    int n_repack_jobs = 0;
    long long repack_max_elems = 0;
    bool repack_ready = false;
    // the job table is rewritten in place after a re-bind: staged through pinned memory and uploaded on the refresh's stream,
    // behind the last repack launch on ANY stream (repack_ev), which may still be queued and reads the table it was given
    PinnedStage repack_stage;
    Event repack_ev;
    std::vector<struct pny_scene*> scenes;  // scenes created on this model (stream ordering of a refresh)
    DeferredStash stash;                     // deferred weight gradients: the training stash reservation
    bool deterministic = false;              // pny_model_set_deterministic: the latent gradient of every scene is bit-reproducible
    Stream aux_stream;                       // side stream of the weight-gradient GEMMs' clipped tiles (mlp_bwd.hip launch_dw_gemm)
    Event aux_fork, aux_join;
    EncoderWeights enc;                       // folded conv+bn (encoder.h)
    DevBuf enc_batch_work, enc_batch_lat;     // pny_scenes_encode: workspace and result of one trunk pass over several scenes
    bool has_encoder = false;
    TrunkTrain* trunk = nullptr;              // created by the first pny_trunk_train_forward
    // lin_z[0..nvb) of the coarse / fine MLP stacked into one (nvb*512 x d_latent) pixel-wise map
    ConvLayer zproj[2];
    std::vector<DevBuf> zproj_allocs;        // what zproj[] points into (a ConvLayer owns nothing)
    bool has_zproj = false;
    bool f16_weights_ok = true;   // every MLP weight is representable in the f16 range (checked at finalize; AUTO precision needs it)
    PinnedBuf range_block;                    // pinned host word the f16x2 kernels report PNY_RANGE_* bits into (pny_model_range_status)
    unsigned* range_flag() const { return static_cast<unsigned*>(range_block.p); }
    uint64_t generation = 0;                  // bumped by every finalize (scenes re-project)
    // single-plane f16 images of lin_in / fc_0 / fc_1 for PNY_PRECISION_F16 (mlp_h1.hip): built only once a scene of the model
    // is set to F16 (model_api.hip build_h1_images), then kept current by every finalize and refresh; [0] coarse, [1] fine MLP
    bool want_h1 = false, h1_ready = false;
    DevBuf h1_packed, h1_jobs;
    int n_h1_jobs = 0;
    long long h1_max_elems = 0;
    // ... and of the TRANSPOSED matrices (plane 0 of the PACK_H2T images) for the single-plane backward chain of
    // PNY_PRECISION_F16_TRAIN (mlp_bwd_h1.hip), in the same buffer: built only once a scene is set to F16_TRAIN
    bool want_h1t = false;
    F16Images h1[2] = {};
};

struct pny_scene {
    pny_model* m = nullptr;
    int ns = 0, L = 0, hl = 0, wl = 0;  // latent
    int width = 0, height = 0;
    bool have_cams = false, have_latent = false;
    int cam_ns = 0;
    int n_objs = 1;       // pny_scene_set_groups: the views are n_objs objects' view lists, ns / n_objs each (MlpArgs::obj_pts)
    Cam cams[MAX_VIEWS];  // host copy; handed to every MLP launch as kernel arguments
    DevBuf latent, work, scratch, enc_work;
    // projected latent of the coarse [0] / fine [1] MLP (see ensure_projection)
    DevBuf zp[2];
    bool zp_valid[2] = {false, false};
    uint64_t zp_generation = 0;
    int zp_mode = PNY_PROJECTION_AUTO;
    float* latent_grad = nullptr;   // (ns, hl, wl, L) caller-owned accumulator of d loss / d latent (pny_scene_bind_latent_grad)
    int precision = PNY_PRECISION_AUTO;   // matrix arithmetic of projected launches (pny_scene_set_precision)
    Prec last_prec = PREC_F32;       // pny_scene_last_precision: the kernel of the last MLP launch
    Prec last_bwd_prec = PREC_F32;   // pny_scene_last_backward_precision: the dX chain of the last backward
    bool last_projected = false;
    double last_flops_ref = 0.0;
    // timing of the MLP launches of the last call
    bool timing = false;
    std::vector<Event> ev;
    int ev_used = 0;
    double last_flops = 0.0;
    int last_launches = 0;
    // training workspace (train_api.hip)
    DevBuf dy_absmax;                        // one word: running max |dY| of the chunk in flight (non-deferred backward)
    // deterministic latent gradient (latent_grad_det.hip): the (ns, hl, wl, L) int64 fixed-point accumulator (all zero between
    // launches), and 32 bytes of scratch: the launch's scale (2 doubles), max |lin_z^T|, this scene's running max |dY| and the
    // copy of it the launch's GEMM scales by
    DevBuf lg_fixed, lg_words;
    int last_lg_det = 0;                     // pny_scene_last_latent_grad_mode
    DevBuf x_stash, dy_stash, dw_partial, dw_bias, dw_tables, d_samp, out_tmp, dz_tmp, sel_tmp, gdepth_tmp;
    long long sel_count = 0;                 // entries of sel_tmp the last pny_render_backward wrote (pny_scene_last_depth_sel)
    PinnedStage table_stage;
    // "stash in the forward": the next pny_render evaluates the MLPs with the STASH instantiation straight into the
    // model-level stash (deferred mode); what each pass wrote is remembered for the backward of the same epoch
    bool stash_next = false;
    StashedPass stashed[2];   // [0] coarse pass, [1] fine pass
    // HIP-event timing of the backward kernels of the last backward call (enable_timing): per MLP pass 4 events
    std::vector<Event> bev;
    int bev_used = 0;
    double bwd_flops[3] = {0.0, 0.0, 0.0};   // stash forward, dX chain, weight-gradient GEMMs
    StreamOrder order;                       // of this scene's calls across streams (dev_resource.h)
    // occupancy grid (pny_scene_set_occupancy; pny_occupancy.h): the scene's own copy of the bits, the workspace of a culled
    // pass (slot per sample, tile sums, the kept count), its compact rows (10 floats per KEPT sample) and the pinned word the
    // count is read into; cleared by everything that changes what the scene's sigma is
    bool occ_on = false;
    OccGrid occ{};
    DevBuf occ_bits, occ_work, occ_rows;
    PinnedBuf occ_count;
    int64_t cull_kept[2] = {0, 0}, cull_total[2] = {0, 0};   // pny_scene_last_cull: [0] coarse pass, [1] fine pass
    // early ray termination (pny_scene_set_termination; pny_termination.h): a rendering option, so nothing clears it but the
    // setter and pny_scene_set_groups above 1.  The per-ray T and alive byte live in occ_work, the two counts of a segment
    // (kept samples, alive rays) are read into occ_count together.
    bool term_on = false;
    float term_t_min = 0.0f;
    int term_segments = 1;
    // pny_scene_last_segments: per pass the issued segments' alive rays and kept samples
    int seg_issued[2] = {0, 0};
    int64_t seg_alive[2][TERM_MAX_SEGMENTS] = {}, seg_kept[2][TERM_MAX_SEGMENTS] = {};
};


namespace pny {
inline int enter_stream(pny_scene* s, hipStream_t st) { return s->order.enter(st); }
// the PNY_RANGE_* bits the f16 kernels have reported so far (pny_model_range_status)
inline unsigned range_bits(const pny_model* m) { return m->range_flag() ? __atomic_load_n(m->range_flag(), __ATOMIC_RELAXED) : 0u; }
int check_ready(pny_scene* s, const char* who);
int view_blocks(const pny_model_desc& d);
inline int d_in(const pny_model_desc& d) { return 3 + 6 * d.num_freqs + 3; }   // xyz, its positional code, view direction
// GEMM FLOPs (2 per MAC, unpadded) per query point over ns views: the forward as the reference computes it, the forward as the
// projected-latent variant executes it (lin_z moved to the per-scene projection), the backward's dX chain.  Every forward
// GEMM has one weight-gradient GEMM of the same size.
// PASS_FORWARD_VIEW_MEAN: a projected forward in the view-mean order of the non-stashing split-f16 kernels (mlp_h2.hip): the last
// per-view fc_1 runs once per sample instead of once per view
enum MlpPass { PASS_FORWARD, PASS_FORWARD_PROJECTED, PASS_CHAIN, PASS_FORWARD_VIEW_MEAN };
double mlp_flops_per_point(const pny_model_desc& d, int ns, MlpPass pass);
// single-plane f16 images (PNY_PRECISION_F16): marks the model as using them and builds them if it is finalized
int want_h1_images(pny_model* m, bool transposed = false);   // transposed: also the chain's images (PNY_PRECISION_F16_TRAIN)
// which MLP a pass evaluates: 0 mlp_coarse (the coarse pass, and every pass of a model without a fine MLP in use), 1 mlp_fine
inline int mlp_index(const pny_model* m, int coarse) { return (coarse || !m->desc.has_fine || !m->use_fine) ? 0 : 1; }
// the f16 images of the coarse / fine MLP: split, or single-plane (valid after want_h1_images)
inline const F16Images& f16_images(const pny_model* m, bool fine, bool single_plane) {
    return single_plane ? m->h1[fine ? 1 : 0] : (fine ? m->fine_t : m->coarse_t).h2;
}
inline int obj_views(const pny_scene* s) { return s->ns / (s->n_objs > 0 ? s->n_objs : 1); }   // views per object
inline StashLayout stash_layout(const pny_model_desc& d, int ns, int L) { return stash_layout(d.n_blocks, d.combine_layer, ns, L); }
// projected latent maps of the coarse (0) / fine (1) MLP, computed if stale; force = regardless of the scene's mode
int ensure_projection(pny_scene* s, int which, long long n_points, hipStream_t st, const float** zp, bool force = false);
// MlpArgs of a launch on this scene in the reference's operation order (no projected latent); tiles of 64 samples
int fill_mlp_args(pny_scene* s, int mode, const float* xyz, const float* dirs, const float* rays, const float* z, int K,
                  long long n_points, int coarse, float* out, MlpArgs* a);
// latent of a list of feature maps (latent_levels.hip): the shape checks of the pny_latent_levels* entries (`who` names the
// caller in the message), then the one launch that assembles the maps into a channel-last latent
int latent_levels_check(const char* who, const float* const* maps, const int* channels, const int* h, const int* w, int n_levels, int n,
                        long long* total_channels);
int latent_levels_assemble(const char* who, const float* const* maps, const int* channels, const int* h, const int* w, int n_levels, int n,
                           float* latent_nhwc, hipStream_t st);
// occupancy.hip
void launch_occupancy_build(const OccBuildArgs& a, hipStream_t st);
void launch_occupancy_classify(const OccClassifyArgs& a, const OccLayout& l, uint32_t* sums2, int64_t* kept, hipStream_t st);
void launch_occupancy_gather(const int32_t* slot, const float* rays, const float* z, int64_t n_samples, int K, int64_t m, float* xyz,
                             float* dirs, hipStream_t st);
void launch_occupancy_expand(const int32_t* slot, const float* outc, int64_t n_samples, int64_t m, float* out, hipStream_t st);
// ... the same three on the columns [k_begin, k_end) of the (n, K) buffers; slot is (n, k_end - k_begin)
void launch_occupancy_classify_segment(const OccSegmentArgs& a, const OccLayout& l, uint32_t* sums2, int64_t* kept, hipStream_t st);
void launch_occupancy_gather_segment(const int32_t* slot, const float* rays, const float* z, int64_t n, int K, int k_begin, int k_end,
                                     int64_t m, float* xyz, float* dirs, hipStream_t st);
void launch_occupancy_expand_segment(const int32_t* slot, const float* outc, int64_t n, int K, int k_begin, int k_end, int64_t m,
                                     float* out, hipStream_t st);
// termination.hip
void launch_termination_update(const TermUpdateArgs& a, hipStream_t st);
// the classification of n x k depth samples against grid g (occupancy_api.hip): checks nothing, launches
void occupancy_classify(const OccGrid& g, const float* rays, const float* z, int64_t n_samples, int k, int32_t* slot, int64_t* kept,
                        void* workspace, hipStream_t st);
// ... of the columns [k_begin, k_end) of n x k depth samples; g.bits null: every cell occupied; alive null: every ray alive
void occupancy_classify_segment(const OccGrid& g, const float* rays, const float* z, int64_t n, int k, int k_begin, int k_end,
                                const uint8_t* alive, int32_t* slot, int64_t* kept, void* workspace, hipStream_t st);
}  // namespace pny
