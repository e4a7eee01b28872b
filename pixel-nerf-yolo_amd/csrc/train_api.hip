// Training entry points of libpnyolo.so (include/pnyolo.h, "backward" section): the gradient the reference obtains with
// loss.backward() through NeRFRenderer.forward / PixelNeRFNet.forward (reference train/trainlib/PixelNerfTrainer.py:133-156,
// src/render/nerf.py:169-309, src/model/resnetfc.py:134-186).  Host-side C++: stash sizing, the weight-gradient GEMM
// work list and the launch sequence; all arithmetic is in mlp.hip (STASH forward) and mlp_bwd.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "api_internal.h"

using namespace pny;

namespace {

struct TrainPlan {
    StashLayout lay;
    std::vector<DwJob> jobs;
    std::vector<DwTarget> targets;  // same order as jobs
};

float* grad_of(const pny_model* m, const std::string& name) {
    auto it = m->grads.find(name);
    return it == m->grads.end() ? nullptr : it->second;
}

// Stash layout and the list of weight-gradient GEMMs of one MLP: each job is (dY slot and its per-view stride, rows, X slot and
// stride, columns, views reduced over, target tensors), the slots named by stash.h for view 0; stride 0 = one slot per tile.
TrainPlan build_plan(const pny_model* m, int ns, int L, const std::string& pre) {
    const pny_model_desc& d = m->desc;
    TrainPlan p;
    p.lay = stash_layout(d, ns, L);
    const StashLayout& l = p.lay;
    auto add = [&](unsigned dy_slot, int dy_stride, int a_rows, unsigned x_slot, int x_stride, int x_cols, int n_views,
                   const std::string& wname, int rows_valid, int cols_valid, const std::string& b0, const std::string& b1) {
        DwJob j;
        j.a_off = dy_slot;
        j.a_view = dy_stride;
        j.a_rows = a_rows;
        j.x_off = x_slot;
        j.x_view = x_stride;
        j.x_cols = x_cols;
        j.n_views = n_views;
        DwTarget t;
        memset(&t, 0, sizeof(t));
        t.w = grad_of(m, wname);
        t.b0 = b0.empty() ? nullptr : grad_of(m, b0);
        t.b1 = b1.empty() ? nullptr : grad_of(m, b1);
        t.rows = rows_valid;
        t.cols = cols_valid;
        t.prows = a_rows;
        t.pcols = x_cols;
        p.jobs.push_back(j);
        p.targets.push_back(t);
    };
    auto blk = [&](int b) { return pre + "blocks." + std::to_string(b); };
    auto lz = [&](int b) { return pre + "lin_z." + std::to_string(b); };
    // lin_out: d_out of the 64 rows of d_raw are valid
    add(l.dy_raw(), 0, D_IN_PAD, l.x_top(), 0, HID, 1, pre + "lin_out.weight", d.d_out, HID, pre + "lin_out.bias", "");
    for (int i = 0; i < l.npost(); ++i) {  // post-combine blocks
        const std::string b = blk(l.nvb() + i);
        add(l.dy_post_dnet(i), 0, HID, l.x_post_h(i), 0, HID, 1, b + ".fc_0.weight", HID, HID, b + ".fc_0.bias", "");
        add(l.dy_post_fc1(i), 0, HID, l.x_post_net(i), 0, HID, 1, b + ".fc_1.weight", HID, HID, b + ".fc_1.bias", "");
    }
    for (int b = 0; b < l.nvb(); ++b) {  // per-view blocks; lin_z[b + 1]'s bias shares fc_1's column sum
        add(l.dy_dnet(0, b), l.dy_view, HID, l.x_h(0, b), l.x_view, HID, ns, blk(b) + ".fc_0.weight", HID, HID, blk(b) + ".fc_0.bias", "");
        add(l.dy_fc1(0, b), l.dy_fc1_stride(b), HID, l.x_net(0, b), l.x_view, HID, ns, blk(b) + ".fc_1.weight", HID, HID, blk(b) + ".fc_1.bias",
            b + 1 < l.nvb() ? lz(b + 1) + ".bias" : std::string());
        add(l.dy_dh(0, b), l.dy_view, HID, l.x_z(0), l.x_view, L, ns, lz(b) + ".weight", HID, L, "", "");
    }
    add(l.dy_lin_in(0), l.dy_view, HID, l.x_in(0), l.x_view, D_IN_PAD, ns, pre + "lin_in.weight", HID, d_in(d), pre + "lin_in.bias",
        l.nvb() > 0 ? lz(0) + ".bias" : std::string());
    return p;
}

// Split every job's (tile, view) range over workgroups so that the grid has ~4 workgroups per CU with equal work.
void build_items(TrainPlan& p, int n_tiles, int cus, std::vector<DwItem>& items, long long* part_floats, long long* bias_floats,
                 int* n_full) {
    items.clear();
    double total = 0.0;
    std::vector<int> otiles(p.jobs.size());
    for (size_t j = 0; j < p.jobs.size(); ++j) {
        const DwJob& jb = p.jobs[j];
        otiles[j] = ((jb.a_rows + 255) / 256) * ((jb.x_cols + 255) / 256);
        total += (double)otiles[j] * jb.n_views * n_tiles;
    }
    double items_per_cu = 4.0;   // PNYOLO_DW_ITEMS_PER_CU: tuning knob (finer items = shorter tail, more partial sums)
    if (const char* e = getenv("PNYOLO_DW_ITEMS_PER_CU")) {
        const double v = atof(e);
        if (v >= 1.0 && v <= 64.0) items_per_cu = v;
    }
    const double per_item = std::max(1.0, total / (items_per_cu * cus));
    long long poff = 0, boff = 0;
    for (size_t j = 0; j < p.jobs.size(); ++j) {
        const DwJob& jb = p.jobs[j];
        const int tv = jb.n_views * n_tiles;
        int splits = (int)std::lround((double)tv / per_item);
        splits = std::max(1, std::min(splits, tv));
        const int per = (tv + splits - 1) / splits;
        splits = (tv + per - 1) / per;
        DwTarget& t = p.targets[j];
        t.splits = splits;
        t.part_off = poff;
        t.bias_off = boff;
        const int mts = (jb.a_rows + 255) / 256, nts = (jb.x_cols + 255) / 256;
        for (int sp = 0; sp < splits; ++sp)
            for (int mt = 0; mt < mts; ++mt)
                for (int nt = 0; nt < nts; ++nt) {
                    DwItem it;
                    it.job = (int)j;
                    it.mt = mt;
                    it.nt = nt;
                    it.tv_lo = sp * per;
                    it.tv_hi = std::min(tv, (sp + 1) * per);
                    it.part_off = poff + (long long)sp * jb.a_rows * jb.x_cols;
                    it.bias_off = boff + (long long)sp * jb.a_rows;
                    items.push_back(it);
                }
        poff += (long long)splits * jb.a_rows * jb.x_cols;
        boff += (long long)splits * jb.a_rows;
    }
    // complete 256 x 256 tiles first (they run the predicate-free instantiation), clipped ones after; within each group
    // longest first, so that the tail of the grid is made of short items
    auto full = [&](const DwItem& it) {
        const DwJob& jb = p.jobs[it.job];
        return (it.mt + 1) * 256 <= jb.a_rows && (it.nt + 1) * 256 <= jb.x_cols;
    };
    std::stable_sort(items.begin(), items.end(), [&](const DwItem& a, const DwItem& b) {
        const bool fa = full(a), fb = full(b);
        if (fa != fb) return fb;   // clipped tiles (lin_in's 64 columns, lin_out's 64 rows) first: they are mostly staging
        return (a.tv_hi - a.tv_lo) > (b.tv_hi - b.tv_lo);
    });
    *n_full = 0;
    for (const DwItem& it : items) *n_full += full(it) ? 1 : 0;
    // XCD-aware placement of the complete tiles: the four output tiles (mt, nt) of one K split read the same dY rows and X
    // columns twice each.  Consecutive workgroup ids go round-robin to the 8 XCDs (each with its own L2), so the four tiles of a
    // split are given ids 8 apart -- same XCD, dispatched together -- and the second read of an operand slab is an L2 hit instead
    // of another trip over the fabric.  (Groups of other sizes, e.g. lin_z at L = 1792 with 2 x 7 tiles, keep list order.)
    if (!getenv("PNYOLO_DW_NO_XCD_GROUPS")) {
        const size_t first = items.size() - (size_t)*n_full;
        std::vector<DwItem> out(items.begin(), items.begin() + first);
        std::vector<std::vector<DwItem>> groups;   // pending groups of exactly 4 tiles
        auto flush = [&]() {
            if (groups.size() == 8) {
                for (int j = 0; j < 4; ++j)
                    for (int g = 0; g < 8; ++g) out.push_back(groups[g][j]);
            } else {
                for (auto& g : groups) out.insert(out.end(), g.begin(), g.end());
            }
            groups.clear();
        };
        size_t i = first;
        while (i < items.size()) {
            size_t j = i + 1;
            while (j < items.size() && j - i < 4 && items[j].job == items[i].job && items[j].tv_lo == items[i].tv_lo) ++j;
            if (j - i == 4) {
                groups.emplace_back(items.begin() + i, items.begin() + j);
                if (groups.size() == 8) flush();
            } else {
                flush();
                out.insert(out.end(), items.begin() + i, items.begin() + j);
            }
            i = j;
        }
        flush();
        items.swap(out);
    }
    *part_floats = poff;
    *bias_floats = boff;
}

// Matrix arithmetic of the backward's GEMMs, decided here for all of them.  Asked for: the scene's precision setting (F32 pins
// the fp32 MFMA; F16_TRAIN = single-plane f16: mlp_bwd_h1.hip, dw_gemm_h1.hip, latent_grad_h1.hip; anything else = split f16:
// mlp_bwd_h2.hip pny_mlp_bwd_h2_kernel, dw_gemm_h2.hip pny_dw_gemm_h2_kernel); env PNYOLO_BWD_PRECISION=f32|f16x2 overrides (read
// at every call: tests vary it).  The dX chain reads the weights' f16 images, so weights beyond the f16 range put it on fp32;
// the weight- and latent-gradient GEMMs read activations and gradients only and stay on split f16 then, scaled by the max |dY|
// the chain tracks for them.
struct BwdRoute {
    Prec chain;          // dX-chain kernel
    bool track_absmax;   // the chain tracks max |dY|: the gradient GEMMs run f16
    Prec gemm() const { return !track_absmax ? PREC_F32 : chain == PREC_H1 ? PREC_H1 : PREC_H2; }   // weight and latent gradients
};
BwdRoute route_bwd(const pny_scene* s) {
    Prec want = s->precision == PNY_PRECISION_F32 ? PREC_F32 : s->precision == PNY_PRECISION_F16_TRAIN ? PREC_H1 : PREC_H2;
    if (const char* e = getenv("PNYOLO_BWD_PRECISION")) {
        if (!strcmp(e, "f32")) want = PREC_F32;
        if (!strcmp(e, "f16x2")) want = PREC_H2;
    }
    return {s->m->f16_weights_ok ? want : PREC_F32, want != PREC_F32};
}

// A zeroed device word (or two) for the chain kernels' atomic max
int ensure_absmax(DevBuf& b, size_t bytes) {
    if (b.p) return 0;
    int rc;
    if ((rc = b.reserve(bytes))) return rc;
    PNY_HIP(hipMemset(b.p, 0, bytes));
    return 0;
}

size_t stash_budget_bytes() {
    size_t v = (size_t)16 << 30;  // both stashes together; PNYOLO_STASH_GB overrides (read at every call: tests vary it)
    if (const char* e = getenv("PNYOLO_STASH_GB")) {
        const double g = atof(e);
        if (g > 0.001) v = (size_t)(g * (double)((size_t)1 << 30));
    }
    return v;
}

// Weight-gradient GEMMs over n_tiles tiles of the two stashes + deterministic split reduction into the bound gradients.
// dy_absmax: the chain kernels' running max |dY| of these tiles (device), or null for the fp32 matrix path
int run_weight_grads(pny_model* m, TrainPlan& plan, int n_tiles, const float* x_stash, const float* dy_stash, DevBuf& partial,
                     DevBuf& bias, DevBuf& tables, PinnedStage& stage, int accumulate, hipStream_t st,
                     const unsigned* dy_absmax = nullptr, int planes = 2) {
    int rc;
    if ((rc = m->aux_stream.ensure(hipStreamNonBlocking, "hipStreamCreate(weight-gradient side stream)"))) return rc;
    if ((rc = m->aux_fork.ensure(hipEventDisableTiming, "hipEventCreate(side stream fork)"))) return rc;
    if ((rc = m->aux_join.ensure(hipEventDisableTiming, "hipEventCreate(side stream join)"))) return rc;
    const int cus = mlp_max_grid(MLP_8x64);
    std::vector<DwItem> items;
    long long part_floats = 0, bias_floats = 0;
    int n_full = 0;
    build_items(plan, n_tiles, cus, items, &part_floats, &bias_floats, &n_full);
    if ((rc = partial.reserve((size_t)part_floats * sizeof(float)))) return rc;
    if ((rc = bias.reserve((size_t)bias_floats * sizeof(float)))) return rc;
    const size_t jb_bytes = plan.jobs.size() * sizeof(DwJob), it_bytes = items.size() * sizeof(DwItem),
                 tg_bytes = plan.targets.size() * sizeof(DwTarget);
    const size_t o_items = (jb_bytes + 255) & ~(size_t)255, o_targets = o_items + ((it_bytes + 255) & ~(size_t)255);
    const size_t total = o_targets + tg_bytes;
    // NOTE: a grown device table is only safe because growth happens before any kernel of this call uses it and after
    // the previous call's kernels (same stream) were enqueued: hipFree of DevBuf::reserve synchronises the device
    if ((rc = tables.reserve(total))) return rc;
    if ((rc = stage.prepare(total))) return rc;
    char* h = reinterpret_cast<char*>(stage.host.p);
    memcpy(h, plan.jobs.data(), jb_bytes);
    memcpy(h + o_items, items.data(), it_bytes);
    memcpy(h + o_targets, plan.targets.data(), tg_bytes);
    if ((rc = stage.upload(tables.p, total, st))) return rc;
    char* tb = reinterpret_cast<char*>(tables.p);
    launch_dw_gemm(reinterpret_cast<const DwJob*>(tb), reinterpret_cast<const DwItem*>(tb + o_items), (int)items.size() - n_full,
                   n_full, x_stash, dy_stash, plan.lay.x_tile, plan.lay.dy_tile, partial.f(), bias.f(), st, m->aux_stream,
                   m->aux_fork, m->aux_join, dy_absmax, planes);
    PNY_HIP(hipGetLastError());
    long long max_elems = 0;
    for (const DwTarget& t : plan.targets) max_elems = std::max(max_elems, (long long)t.rows * t.cols + t.rows);
    launch_dw_reduce(reinterpret_cast<const DwTarget*>(tb + o_targets), (int)plan.targets.size(), max_elems, partial.f(), bias.f(),
                     accumulate, st);
    PNY_HIP(hipGetLastError());
    return 0;
}

// One backward of an MLP evaluation over n_points query points, as its caller states it
struct MlpBackwardCall {
    int mode = 0;                  // 0: xyz / dirs; 1: rays + z with K samples per ray
    const float* xyz = nullptr;
    const float* dirs = nullptr;
    const float* rays = nullptr;
    const float* z = nullptr;
    int K = 1;
    long long n_points = 0;
    int coarse = 1;
    const float* d_out = nullptr;  // (n_points, d_out) = dL/d(out)
    int accumulate = 0;            // add to the bound gradients (this call's own weight-gradient GEMMs)
    // mode 1 only, optional: per ray kfd sample indices (ray * K + position, or -1) whose depth gradient through the MLP inputs is
    // added to dz_out (n_points)
    const int* dz_sel = nullptr;
    int kfd = 0;
    float* dz_out = nullptr;
    // what the forward pny_render stashed for this pass and the per-sample output it wrote (both, or the forward is recomputed)
    const StashedPass* stashed = nullptr;
    const float* fwd_out = nullptr;
    bool immediate = false;        // an outstanding reservation is not this call's: weight gradients at once, from the scene's own stash
};

// Where a backward's tiles go and who turns them into weight gradients
struct StashTarget {
    float* x = nullptr;            // record 0 of the call's (chunk's) tiles: the GEMMs' B operands ...
    float* dy = nullptr;           // ... and the dY tiles
    long long chunk_pts = 0;       // points per chunk: all of them, unless the scene's own stash is filled chunk after chunk
    unsigned* absmax = nullptr;    // word the chain adds its max |dY| to for the f16 gradient GEMMs (null: nobody reads it)
    bool have_x = false;           // the forward's tiles are reused: nothing is recomputed
    bool own_dw = false;           // this call runs its own weight-gradient GEMMs (else: pny_model_flush_weight_grads)
};

// The three stash targets: the tiles the forward pny_render already wrote into the reservation (same epoch); new tiles appended to
// the reservation, whose weight-gradient GEMM runs once over every scene's tiles at the flush; or the scene's own stash, filled in
// chunks that fit the budget.  The running max |dY| is per model and MLP in the reservation (every scene's chain adds to it,
// zeroed again by the flush) and per scene otherwise (zeroed in front of every chunk's chain).
int stash_target(pny_scene* s, const MlpBackwardCall& c, const StashLayout& lay, int which, const BwdRoute& r, StashTarget* t) {
    DeferredStash& ds = s->m->stash;
    const bool defer = ds.book.active && !c.immediate;
    t->have_x = defer && c.stashed && ds.book.owns(*c.stashed) && c.stashed->n_points == c.n_points && c.fwd_out;
    t->own_dw = !defer;
    if (s->n_objs > 1 && !defer)   // (the chunked recompute path would split an object's share)
        return fail(PNY_ERR_STATE, "grouped scene: the backward needs the deferred stash (pny_model_defer_weight_grads)");
    const size_t tile_bytes = (size_t)(lay.x_tile + lay.dy_tile) * sizeof(float);
    const long long max_tiles = (long long)(stash_budget_bytes() / tile_bytes);
    if (max_tiles < 1) return fail(PNY_ERR_ARG, "stash budget smaller than one tile");
    int rc;
    t->chunk_pts = c.n_points;   // one chunk in the reservation: it was made against the budget
    if (t->have_x) {
        t->x = ds.x_record(lay, c.stashed->which, c.stashed->tile0);
        t->dy = ds.dy_record(lay, c.stashed->which, c.stashed->tile0);
    } else if (defer) {
        const long long tiles = (c.n_points + 63) / 64;
        if (!ds.book.has_room(which, obj_views(s), tiles))
            return fail(PNY_ERR_STATE, obj_views(s) != ds.book.ns ? "deferred weight gradients: scene view count differs from the reservation"
                                                                  : "deferred weight gradients: more tiles than pny_model_defer_weight_grads reserved");
        const long long tile0 = ds.book.take(which, tiles);
        t->x = ds.x_record(lay, which, tile0);
        t->dy = ds.dy_record(lay, which, tile0);
    } else {
        // chunk boundaries on whole rays (mode 1) so that sample -> ray indexing stays local to the chunk
        const long long unit = c.mode == 1 ? c.K : 1;
        t->chunk_pts = std::max(unit, std::min(c.n_points, max_tiles * 64) / unit * unit);
        const long long chunk_tiles_max = (t->chunk_pts + 63) / 64;
        if ((rc = s->x_stash.reserve((size_t)chunk_tiles_max * lay.x_tile * sizeof(float)))) return rc;
        if ((rc = s->dy_stash.reserve((size_t)chunk_tiles_max * lay.dy_tile * sizeof(float)))) return rc;
        t->x = s->x_stash.f();
        t->dy = s->dy_stash.f();
    }
    if (defer) {
        ds.book.note_contributor(r.gemm());
        if ((rc = ensure_absmax(ds.absmax, 2 * sizeof(unsigned)))) return rc;
        t->absmax = ds.absmax_word(which);
    } else if (r.track_absmax) {
        if ((rc = ensure_absmax(s->dy_absmax, sizeof(unsigned)))) return rc;
        t->absmax = reinterpret_cast<unsigned*>(s->dy_absmax.p);
    }
    return 0;
}

// Deterministic latent gradient (pny_model_set_deterministic, latent_grad_det.hip): the chain tracks this scene's own running
// max |dY| (handed on to the stash target's word behind it), which sets the launch's fixed-point scale; the scene's int64 accumulator
// is all zero between launches
struct LatentGradDet {
    bool on = false;
    long long elems = 0;           // of the (ns, hl, wl, L) accumulator
    unsigned* max_word = nullptr;  // 0 between launches: zeroed at allocation and reset by every deterministic launch
};
int latent_grad_det_setup(pny_scene* s, hipStream_t st, LatentGradDet* lg) {
    lg->on = s->m->deterministic && s->latent_grad && view_blocks(s->m->desc) > 0;
    lg->elems = (long long)s->ns * s->hl * s->wl * s->L;
    if (!lg->on) return 0;
    int rc;   // (zeroed on THIS stream: a plain hipMemset would be ordered on the null stream, behind other scenes' work)
    if (!s->lg_words.p) {
        if ((rc = s->lg_words.reserve(32))) return rc;
        PNY_HIP(hipMemsetAsync(s->lg_words.p, 0, 32, st));
    }
    lg->max_word = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(s->lg_words.p) + 20);
    const size_t need = (size_t)lg->elems * sizeof(unsigned long long);
    if (s->lg_fixed.bytes < need) {
        if ((rc = s->lg_fixed.reserve(need))) return rc;
        PNY_HIP(hipMemsetAsync(s->lg_fixed.p, 0, need, st));
    }
    return 0;
}

// Arguments of the dX chain over one chunk (np points from p0) whose forward output is `out`
BwdArgs chain_args(const pny_scene* s, const MlpBackwardCall& c, int which, const BwdRoute& r, const StashLayout& lay, const StashTarget& t,
                   const LatentGradDet& lg, const float* out, long long p0, long long np) {
    const pny_model* m = s->m;
    const pny_model_desc& d = m->desc;
    const MlpWeightsT& wt = which ? m->fine_t : m->coarse_t;
    BwdArgs b;
    memset(&b, 0, sizeof(b));
    b.wT_out = wt.wT_out;
    for (int i = 0; i < d.n_blocks; ++i) {
        b.wT_fc0[i] = wt.wT_fc0[i];
        b.wT_fc1[i] = wt.wT_fc1[i];
    }
    b.w_base = m->packed.f();
    b.w_bytes = (unsigned)m->packed.bytes;
    b.x_stash = t.x;
    b.dy_stash = t.dy;
    b.lay = lay;
    b.out = out;
    b.d_out_grad = c.d_out + p0 * d.d_out;
    b.n_points = np;
    b.n_tiles = (int)((np + 63) / 64);
    b.NS = obj_views(s);
    b.n_blocks = d.n_blocks;
    b.combine_layer = d.combine_layer;
    b.d_out = d.d_out;
    b.yolo = d.yolo;
    b.dy_absmax = t.absmax;
    b.range_flag = m->range_flag();
    if (lg.on) {
        b.dy_absmax = lg.max_word;
        if (!t.absmax) b.range_flag = nullptr;   // (the fp32 path keeps its semantics: no f16 range guard)
    }
    // the chain's f16 images: split in the packed blob, single-plane in the model's h1 buffer (none: the fp32 chain)
    if (r.chain != PREC_F32) use_images(b, f16_images(m, which == 1, r.chain == PREC_H1));
    return b;
}

// Arguments of the depth-gradient kernel over the chunk of forward launch `a`: the selected samples' dL/dz through the MLP inputs
DzArgs dz_args(const pny_scene* s, const MlpBackwardCall& c, int which, const MlpArgs& a, const StashLayout& lay, const float* dy,
               const float* zp_maps, long long p0, long long np) {
    const pny_model_desc& d = s->m->desc;
    DzArgs dz;
    memset(&dz, 0, sizeof(dz));
    dz.dy_stash = dy;
    dz.lay = lay;
    dz.sel = c.dz_sel + (p0 / c.K) * c.kfd;
    dz.n_sel = (int)((np / c.K) * c.kfd);
    dz.p0 = p0;
    dz.rays = c.rays;
    dz.z = c.z;
    dz.K = c.K;
    dz.w_in = (which ? s->m->fine_t : s->m->coarse_t).w_in_plain;
    dz.d_in = d_in(d);
    dz.zp = zp_maps;
    dz.zp_stride = view_blocks(d) * HID;
    dz.NS = obj_views(s);
    dz.obj_pts = a.obj_pts;
    dz.Hl = s->hl;
    dz.Wl = s->wl;
    dz.yolo = d.yolo;
    dz.num_freqs = d.num_freqs;
    dz.freq_factor = d.freq_factor;
    dz.sx = a.sx;
    dz.sy = a.sy;
    dz.dz = c.dz_out;
    memcpy(dz.cams, s->cams, sizeof(Cam) * (size_t)s->ns);
    return dz;
}

// Gradient w.r.t. the latent of the chunk of forward launch `a` (encoder training): lin_z^T GEMM off the dY tiles + scatter into the taps
int latent_grad_step(pny_scene* s, const MlpArgs& a, int which, const BwdRoute& r, const StashLayout& lay, const StashTarget& t,
                     const LatentGradDet& lg, hipStream_t st) {
    const int nvb = view_blocks(s->m->desc);
    const float* wzT_cat = (which ? s->m->fine_t : s->m->coarse_t).wzT_cat;
    if (!wzT_cat) return fail(PNY_ERR_STATE, "latent gradient: transposed lin_z weights are missing");
    if (s->L % 256) return fail(PNY_ERR_ARG, "latent gradient: d_latent must be a multiple of 256");
    if (lg.on) {
        int rc;
        if ((rc = launch_latent_grad_det(a, t.dy, lay, wzT_cat, s->latent_grad, nvb, st, lg.max_word, r.gemm(),
                                         reinterpret_cast<unsigned long long*>(s->lg_fixed.p), lg.elems, s->lg_words.p)))
            return rc;
    } else {
        launch_latent_grad(a, t.dy, lay, wzT_cat, s->latent_grad, nvb, st, r.track_absmax ? t.absmax : nullptr, gemm_planes(r.gemm()));
    }
    s->last_lg_det = lg.on ? 1 : 0;
    PNY_HIP(hipGetLastError());
    return 0;
}

// Backward of one MLP evaluation: c.d_out -> bound parameter gradients (and the scene's latent and depth-sample gradients).
int mlp_backward(pny_scene* s, const MlpBackwardCall& c, hipStream_t st) {
    if (c.n_points == 0) return 0;
    pny_model* m = s->m;
    const pny_model_desc& d = m->desc;
    const int which = mlp_index(m, c.coarse);
    TrainPlan plan = build_plan(m, obj_views(s), s->L, which ? "mlp_fine." : "mlp_coarse.");
    const StashLayout& lay = plan.lay;
    const BwdRoute r = route_bwd(s);
    int rc;
    if (r.chain == PREC_H1 && (rc = want_h1_images(m, true))) return rc;
    StashTarget t;
    if ((rc = stash_target(s, c, lay, which, r, &t))) return rc;
    if ((rc = s->out_tmp.reserve((size_t)t.chunk_pts * d.d_out * sizeof(float)))) return rc;
    LatentGradDet lg;
    if ((rc = latent_grad_det_setup(s, st, &lg))) return rc;
    auto stamp = [&]() { return stamp_event(s->timing, s->bev, s->bev_used, st); };   // kernel timing for bench.py
    {   // GEMM FLOPs of the three kernels
        const double fwd = mlp_flops_per_point(d, obj_views(s), PASS_FORWARD) * (double)c.n_points;
        if (!t.have_x) s->bwd_flops[0] += fwd;   // the forward already stashed: nothing is recomputed
        s->bwd_flops[1] += mlp_flops_per_point(d, obj_views(s), PASS_CHAIN) * (double)c.n_points;
        s->bwd_flops[2] += fwd;   // every forward GEMM has one weight-gradient GEMM of the same size
    }
    const float* zp_maps = nullptr;
    if (c.dz_sel && view_blocks(d) > 0) {
        if ((rc = ensure_projection(s, which, 0, st, &zp_maps, true))) return rc;
        if (!zp_maps) return fail(PNY_ERR_ARG, "sample-depth gradients need the projected latent maps (latent too large)");
    }
    const int cus = mlp_max_grid(MLP_8x64);
    for (long long p0 = 0; p0 < c.n_points; p0 += t.chunk_pts) {
        const long long np = std::min(t.chunk_pts, c.n_points - p0);
        const int n_tiles = (int)((np + 63) / 64);
        const int grid = std::min(cus, n_tiles);
        // 1. forward in the reference's operation order, stashing every GEMM's B operand (unless the forward call already did)
        MlpArgs a;
        if ((rc = fill_mlp_args(s, c.mode, c.mode == 0 ? c.xyz + 3 * p0 : nullptr, c.mode == 0 ? c.dirs + 3 * p0 : nullptr,
                                c.mode == 1 ? c.rays + (p0 / c.K) * 8 : nullptr, c.mode == 1 ? c.z + p0 : nullptr, c.K, np, c.coarse,
                                s->out_tmp.f(), &a)))
            return rc;
        a.stash_x = t.x;
        a.lay = lay;
        if ((rc = stamp())) return rc;
        if (!t.have_x) {
            launch_mlp_stash(a, grid, st);
            PNY_HIP(hipGetLastError());
        }
        if ((rc = stamp())) return rc;
        // 2. dX chain
        const BwdArgs b = chain_args(s, c, which, r, lay, t, lg, t.have_x ? c.fwd_out : s->out_tmp.f(), p0, np);
        if (t.absmax && t.own_dw) PNY_HIP(hipMemsetAsync(t.absmax, 0, sizeof(unsigned), st));
        (r.chain == PREC_H1 ? launch_mlp_bwd_h1 : r.chain == PREC_H2 ? launch_mlp_bwd_h2 : launch_mlp_bwd)(b, grid, st);
        s->last_bwd_prec = r.chain;
        PNY_HIP(hipGetLastError());
        if (lg.on && t.absmax) launch_absmax_fold(t.absmax, lg.max_word, st);
        if ((rc = stamp())) return rc;
        // 2b. gradient w.r.t. the depths of the selected samples through the MLP inputs (fine pass of a render)
        if (c.dz_sel && c.mode == 1) {
            launch_mlp_dz(dz_args(s, c, which, a, lay, t.dy, zp_maps, p0, np), st);
            PNY_HIP(hipGetLastError());
        }
        // 2c. gradient w.r.t. the latent
        if (s->latent_grad && view_blocks(d) > 0 && (rc = latent_grad_step(s, a, which, r, lay, t, lg, st))) return rc;
        // 3. weight-gradient GEMMs over the two stashes + deterministic split reduction into the bound gradients
        if (t.own_dw &&
            (rc = run_weight_grads(m, plan, n_tiles, t.x, t.dy, s->dw_partial, s->dw_bias, s->dw_tables, s->table_stage,
                                   (c.accumulate || p0 > 0) ? 1 : 0, st, t.absmax, gemm_planes(r.gemm()))))
            return rc;
        if ((rc = stamp())) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

int pny_scene_bind_latent_grad(pny_scene* s, float* grad_dev) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_bind_latent_grad: null scene");
    s->latent_grad = grad_dev;
    return PNY_OK;
}

int pny_model_set_deterministic(pny_model* m, int enable) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_set_deterministic: null model");
    m->deterministic = enable != 0;
    return PNY_OK;
}

int pny_scene_last_latent_grad_mode(pny_scene* s, int* deterministic) {
    if (!s || !deterministic) return fail(PNY_ERR_ARG, "pny_scene_last_latent_grad_mode: null argument");
    *deterministic = s->last_lg_det;
    return PNY_OK;
}

int pny_model_bind_grad(pny_model* m, const char* name, float* grad_dev) {
    if (!m || !name) return fail(PNY_ERR_ARG, "pny_model_bind_grad: null argument");
    if (grad_dev)
        m->grads[name] = grad_dev;
    else
        m->grads.erase(name);
    return PNY_OK;
}

int pny_model_defer_weight_grads(pny_model* m, int enable, int ns, int64_t coarse_tiles, int64_t fine_tiles) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_defer_weight_grads: null model");
    DeferredStash& ds = m->stash;
    ds.book.close();   // passes stashed under the previous reservation are no longer valid
    if (!enable) return PNY_OK;
    if (ns < 1 || ns > MAX_VIEWS || coarse_tiles < 0 || fine_tiles < 0) return fail(PNY_ERR_ARG, "pny_model_defer_weight_grads: bad argument");
    PNY_HIP(hipSetDevice(m->desc.device));
    const StashLayout lay = stash_layout(m->desc, ns, m->desc.d_latent);   // (does not depend on the MLP)
    const size_t tile_bytes = (size_t)(lay.x_tile + lay.dy_tile) * sizeof(float);
    if ((size_t)(coarse_tiles + fine_tiles) * tile_bytes > stash_budget_bytes())
        return fail(PNY_ERR_ARG, "pny_model_defer_weight_grads: reservation exceeds the stash budget (PNYOLO_STASH_GB)");
    const long long tiles[2] = {coarse_tiles, fine_tiles};
    int rc;
    for (int w = 0; w < 2; ++w) {
        if ((rc = ds.x[w].reserve((size_t)tiles[w] * lay.x_tile * sizeof(float)))) return rc;
        if ((rc = ds.dy[w].reserve((size_t)tiles[w] * lay.dy_tile * sizeof(float)))) return rc;
    }
    ds.book.open(ns, tiles);
    return PNY_OK;
}

int pny_model_flush_weight_grads(pny_model* m, int accumulate, pny_stream stream) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_flush_weight_grads: null model");
    DeferredStash& ds = m->stash;
    if (!ds.book.active) return fail(PNY_ERR_STATE, "pny_model_flush_weight_grads: not in deferred mode");
    PNY_HIP(hipSetDevice(m->desc.device));
    hipStream_t st = (hipStream_t)stream;
    int rc;
    // only mlp_coarse's / only mlp_fine's stash (neither: both)
    const bool only_c = (accumulate & PNY_FLUSH_COARSE_ONLY) != 0, only_f = (accumulate & PNY_FLUSH_FINE_ONLY) != 0;
    accumulate &= PNY_ACC_ADD;
    if (!only_c) {   // (a coarse-only flush follows the fine-only one of the same step: keep its numbers)
        ds.flush_flops = 0.0;
        ds.flush_launches = 0;
    }
    for (Event& e : ds.flush_ev)
        if ((rc = e.ensure(hipEventDefault, "hipEventCreate(flush timing)"))) return rc;
    const pny_model_desc& d = m->desc;
    const double fwd = mlp_flops_per_point(d, ds.book.ns, PASS_FORWARD);
    const int last = only_c ? 0 : 1;   // the last MLP this call flushes
    for (int w = 0; w < 2; ++w) {
        if ((w == 0 && only_f) || (w == 1 && only_c)) continue;
        PNY_HIP(hipEventRecord(ds.flush_ev[2 * w], st));
        const long long n_tiles = ds.book.used[w];
        if (n_tiles > 0) {
            TrainPlan plan = build_plan(m, ds.book.ns, d.d_latent, w ? "mlp_fine." : "mlp_coarse.");
            const Prec gemm = ds.book.flush_gemm(ds.absmax.p != nullptr);
            const unsigned* absmax = gemm == PREC_F32 ? nullptr : ds.absmax_word(w);   // the f16 GEMMs scale by the running max |dY|
            if ((rc = run_weight_grads(m, plan, (int)n_tiles, ds.x_record(plan.lay, w, 0), ds.dy_record(plan.lay, w, 0), ds.partial[w],
                                       ds.bias[w], ds.tables[w], ds.stage[w], accumulate, st, absmax, gemm_planes(gemm))))
                return rc;
            ds.flush_flops += fwd * 64.0 * (double)n_tiles;
            ds.last_flush_prec = gemm;
            ds.flush_launches += 1;
        }
        PNY_HIP(hipEventRecord(ds.flush_ev[2 * w + 1], st));
        // (contributors: a fine-only flush is followed by the coarse-only one of the same step)
        ds.book.flushed(w, w == last && !only_f);
        if (unsigned* word = ds.absmax_word(w))   // the next step's chains start from 0
            PNY_HIP(hipMemsetAsync(word, 0, sizeof(unsigned), st));
    }
    return PNY_OK;
}


int pny_model_last_flush_precision(pny_model* m, int* code) {
    if (!m || !code) return fail(PNY_ERR_ARG, "pny_model_last_flush_precision: null argument");
    *code = m->stash.last_flush_prec;
    return PNY_OK;
}

int pny_model_last_flush_stats(pny_model* m, double* flops, double* kernel_ms) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_last_flush_stats: null model");
    const DeferredStash& ds = m->stash;
    if (flops) *flops = ds.flush_flops;
    if (kernel_ms) {
        *kernel_ms = 0.0;
        for (int w = 0; w < 2 && ds.flush_ev[0]; ++w) {
            PNY_HIP(hipEventSynchronize(ds.flush_ev[2 * w + 1]));
            float ms = 0.f;
            PNY_HIP(hipEventElapsedTime(&ms, ds.flush_ev[2 * w], ds.flush_ev[2 * w + 1]));
            *kernel_ms += ms;
        }
    }
    return PNY_OK;
}

int pny_scene_stash_next_render(pny_scene* s, int enable) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_stash_next_render: null scene");
    if (enable && !s->m->stash.book.active) return fail(PNY_ERR_STATE, "pny_scene_stash_next_render: reserve the stash first (pny_model_defer_weight_grads)");
    s->stash_next = enable != 0;
    return PNY_OK;
}

int pny_query_backward(pny_scene* s, const float* xyz_dev, const float* viewdirs_dev, int64_t n, int coarse,
                       const float* d_out_dev, int accumulate, pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_query_backward"))) return rc;
    if (n < 0 || (n > 0 && (!xyz_dev || !viewdirs_dev || !d_out_dev))) return fail(PNY_ERR_ARG, "pny_query_backward: bad argument");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    s->bev_used = 0;
    s->bwd_flops[0] = s->bwd_flops[1] = s->bwd_flops[2] = 0.0;
    // immediate: a deferred reservation that a training pny_render left outstanding belongs to that render's backward; this
    // call's weight gradients go straight into the buffers bound now
    MlpBackwardCall c;
    c.mode = 0;
    c.xyz = xyz_dev;
    c.dirs = viewdirs_dev;
    c.n_points = n;
    c.coarse = coarse;
    c.d_out = d_out_dev;
    c.accumulate = accumulate & PNY_ACC_ADD;
    c.immediate = true;
    return mlp_backward(s, c, (hipStream_t)stream);
}

int pny_composite_backward(const float* rays_dev, const float* z_dev, const float* sample_dev, int64_t n, int k, int white_bkgd,
                           const float* g_rgb_dev, const float* g_depth_dev, const float* g_weights_dev, float* d_sample_dev,
                           float* d_z_dev, pny_stream stream) {
    if (n < 0 || k < 1 || (n > 0 && (!rays_dev || !z_dev || !sample_dev || !d_sample_dev)))
        return fail(PNY_ERR_ARG, "pny_composite_backward: bad argument");
    if ((size_t)4 * 2 * k * sizeof(float) > 64 * 1024) return fail(PNY_ERR_ARG, "pny_composite_backward: too many samples per ray");
    launch_composite_bwd(rays_dev, z_dev, sample_dev, nullptr, n, k, white_bkgd, g_rgb_dev, g_depth_dev, g_weights_dev, d_sample_dev,
                         d_z_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_render_backward(pny_scene* s, const float* rays_dev, int64_t n, const pny_render_opts* o, const pny_render_saved* sv,
                        const pny_render_grads* g, int accumulate, pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_render_backward"))) return rc;
    if (!o || !sv || !g || n < 0 || (n > 0 && !rays_dev)) return fail(PNY_ERR_ARG, "pny_render_backward: bad argument");
    if (s->m->desc.yolo || s->m->desc.d_out != 4) return fail(PNY_ERR_ARG, "pny_render_backward: model is in YOLO mode");
    if (n == 0) return PNY_OK;
    const int kc = o->n_coarse, kt = o->n_coarse + o->n_fine;
    if (!sv->z_coarse || !sv->sample_coarse || (o->n_fine > 0 && (!sv->z_fine || !sv->sample_fine)))
        return fail(PNY_ERR_ARG, "pny_render_backward: the forward call's z / per-sample outputs are required");
    if ((size_t)4 * 2 * kt * sizeof(float) > 64 * 1024) return fail(PNY_ERR_ARG, "pny_render_backward: too many samples per ray");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = enter_stream(s, st))) return rc;
    s->bev_used = 0;
    s->bwd_flops[0] = s->bwd_flops[1] = s->bwd_flops[2] = 0.0;
    if ((rc = s->d_samp.reserve((size_t)n * kt * 4 * sizeof(float)))) return rc;
    const bool same_mlp = mlp_index(s->m, 0) == 0;  // both passes differentiate mlp_coarse
    const bool immediate = (accumulate & PNY_ACC_IMMEDIATE) != 0;   // ignore a deferred reservation that belongs to another forward
    // only the fine / only the coarse pass of this backward (the caller runs every scene's fine pass, starts the fine MLP's
    // weight-gradient flush beside the coarse passes, then the coarse passes: pny_model_flush_weight_grads)
    const bool do_fine = (accumulate & PNY_ACC_COARSE_ONLY) == 0, do_coarse = (accumulate & PNY_ACC_FINE_ONLY) == 0;
    bool first = true;
    const bool any_f = o->n_fine > 0 && (g->rgb_fine || g->depth_fine || g->weights_fine);
    const bool any_c = g->rgb_coarse || g->depth_coarse || g->weights_coarse;
    // The fine pass's depth samples are centred on the (attached) coarse depth (nerf.py:156-167, 296-298): the fine
    // loss reaches mlp_coarse through those samples' positions.  dL/dz of the fine samples = composite part + MLP-input
    // part; summed over a ray's unclamped depth samples it is an extra dL/d(depth_coarse).
    const int kfd = o->n_fine_depth;
    const bool depth_path = any_f && kfd > 0 && sv->depth_coarse;
    {   // a pass that was stashed by the forward but receives no gradient must not leave stale dY tiles for the flush
        const DeferredStash& ds = s->m->stash;
        const StashLayout lay = stash_layout(s->m->desc, obj_views(s), s->L);
        auto zero_pass = [&](const StashedPass& sp) -> int {
            if (!immediate && ds.book.owns(sp))
                PNY_HIP(hipMemsetAsync(ds.dy_record(lay, sp.which, sp.tile0), 0, (size_t)sp.tiles * lay.dy_tile * sizeof(float), st));
            return 0;
        };
        if (do_fine && !any_f && (rc = zero_pass(s->stashed[1]))) return rc;
        if (do_coarse && !(any_c || depth_path) && (rc = zero_pass(s->stashed[0]))) return rc;
    }
    MlpBackwardCall pass;   // what the two passes share; each fills in its own depths, gradient extras and stashed pass
    pass.mode = 1;
    pass.rays = rays_dev;
    pass.d_out = s->d_samp.f();
    pass.immediate = immediate;
    const float* g_depth_c = g->depth_coarse;
    if (any_f && !do_fine) {   // coarse-only call: the fine pass of this backward ran in an earlier call and left the depth path's sum
        if (depth_path) g_depth_c = s->gdepth_tmp.f();
        first = false;
    }
    if (any_f && do_fine) {
        float* dz = nullptr;
        int* sel = nullptr;
        if (depth_path) {
            if ((rc = s->dz_tmp.reserve((size_t)n * kt * sizeof(float)))) return rc;
            if ((rc = s->sel_tmp.reserve((size_t)n * kfd * sizeof(int)))) return rc;
            if ((rc = s->gdepth_tmp.reserve((size_t)n * sizeof(float)))) return rc;
            dz = s->dz_tmp.f();
            sel = reinterpret_cast<int*>(s->sel_tmp.p);
            launch_locate_depth_samples(rays_dev, sv->depth_coarse, o->g_depth_dev, o->seed, sv->z_fine, n, kt, kfd, o->depth_std, sel, st);
            s->sel_count = (long long)n * kfd;
        }
        launch_composite_bwd(rays_dev, sv->z_fine, sv->sample_fine, o->sigma_noise_fine_dev, n, kt, o->white_bkgd, g->rgb_fine,
                             g->depth_fine, g->weights_fine, s->d_samp.f(), dz, st);
        PNY_HIP(hipGetLastError());
        pass.z = sv->z_fine;
        pass.K = kt;
        pass.n_points = (long long)n * kt;
        pass.coarse = 0;
        pass.accumulate = accumulate & PNY_ACC_ADD;
        pass.dz_sel = sel;
        pass.kfd = kfd;
        pass.dz_out = dz;
        pass.stashed = &s->stashed[1];
        pass.fwd_out = sv->sample_fine;
        if ((rc = mlp_backward(s, pass, st))) return rc;
        if (depth_path) {
            launch_depth_grad_gather(sel, dz, g->depth_coarse, n, kfd, s->gdepth_tmp.f(), st);
            PNY_HIP(hipGetLastError());
            g_depth_c = s->gdepth_tmp.f();
        }
        first = false;
    }
    if (do_coarse && (any_c || depth_path)) {
        launch_composite_bwd(rays_dev, sv->z_coarse, sv->sample_coarse, o->sigma_noise_coarse_dev, n, kc, o->white_bkgd, g->rgb_coarse,
                             g_depth_c, g->weights_coarse, s->d_samp.f(), nullptr, st);
        PNY_HIP(hipGetLastError());
        pass.z = sv->z_coarse;
        pass.K = kc;
        pass.n_points = (long long)n * kc;
        pass.coarse = 1;
        pass.accumulate = ((accumulate & PNY_ACC_ADD) || (same_mlp && !first)) ? 1 : 0;
        pass.dz_sel = nullptr;
        pass.kfd = 0;
        pass.dz_out = nullptr;
        pass.stashed = &s->stashed[0];
        pass.fwd_out = sv->sample_coarse;
        if ((rc = mlp_backward(s, pass, st))) return rc;
    }
    return PNY_OK;
}

int pny_scene_last_depth_sel(pny_scene* s, int32_t* sel_dev, int64_t count, pny_stream stream) {
    if (!s || !sel_dev) return fail(PNY_ERR_ARG, "pny_scene_last_depth_sel: null argument");
    if (count != s->sel_count || !s->sel_tmp.p)
        return fail(PNY_ERR_STATE, "pny_scene_last_depth_sel: count differs from the last backward's n * n_fine_depth (or none ran)");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if (count > 0)
        PNY_HIP(hipMemcpyAsync(sel_dev, s->sel_tmp.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PNY_OK;
}

int pny_locate_depth_samples(const float* rays_dev, const float* depth_coarse_dev, const float* g_dev, uint64_t seed,
                             const float* z_fine_dev, int64_t n, int kt, int kfd, float depth_std, int32_t* sel_dev,
                             pny_stream stream) {
    if (n < 0 || kt < 1 || kfd < 0 || kfd > kt) return fail(PNY_ERR_ARG, "pny_locate_depth_samples: bad sample counts");
    if (n > 0 && kfd > 0 && (!rays_dev || !depth_coarse_dev || !z_fine_dev || !sel_dev))
        return fail(PNY_ERR_ARG, "pny_locate_depth_samples: null argument");
    if (n > (int64_t)0x7fffffff / kt) return fail(PNY_ERR_ARG, "pny_locate_depth_samples: n * kt does not fit the int32 positions");
    launch_locate_depth_samples(rays_dev, depth_coarse_dev, g_dev, seed, z_fine_dev, n, kt, kfd, depth_std, sel_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_depth_grad_gather(const int32_t* sel_dev, const float* dz_dev, const float* g_in_dev, int64_t n, int kfd, float* g_out_dev,
                          pny_stream stream) {
    if (n < 0 || kfd < 0 || (n > 0 && (!g_out_dev || (kfd > 0 && (!sel_dev || !dz_dev)))))
        return fail(PNY_ERR_ARG, "pny_depth_grad_gather: bad argument");
    launch_depth_grad_gather(sel_dev, dz_dev, g_in_dev, n, kfd, g_out_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_aggregate_backward(const float* raw_dev, const float* g_out_dev, int64_t n, int k, int n_anchors, float* d_raw_dev,
                                pny_stream stream) {
    if (n < 0 || k < 1 || n_anchors < 1 || (n > 0 && (!raw_dev || !g_out_dev || !d_raw_dev)))
        return fail(PNY_ERR_ARG, "pny_yolo_aggregate_backward: bad argument");
    launch_yolo_aggregate_bwd(raw_dev, g_out_dev, n, k, n_anchors, d_raw_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_render_backward(pny_scene* s, const float* rays_dev, int64_t n, int n_coarse, const float* u_coarse_dev, uint64_t seed,
                             const float* raw_dev, const float* g_out_dev, int accumulate, pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_yolo_render_backward"))) return rc;
    const pny_model_desc& d = s->m->desc;
    if (!d.yolo || d.d_out % 7) return fail(PNY_ERR_ARG, "pny_yolo_render_backward: model is not in YOLO mode");
    if (n < 0 || n_coarse < 1 || (n > 0 && (!rays_dev || !raw_dev || !g_out_dev))) return fail(PNY_ERR_ARG, "pny_yolo_render_backward: bad argument");
    if (n == 0) return PNY_OK;
    PNY_HIP(hipSetDevice(d.device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = enter_stream(s, st))) return rc;
    s->bev_used = 0;
    s->bwd_flops[0] = s->bwd_flops[1] = s->bwd_flops[2] = 0.0;
    const size_t nz = ((size_t)n * n_coarse + 63) & ~(size_t)63;
    if ((rc = s->d_samp.reserve((size_t)n * n_coarse * d.d_out * sizeof(float)))) return rc;
    if ((rc = s->dz_tmp.reserve(nz * sizeof(float)))) return rc;
    float* z = s->dz_tmp.f();
    launch_sample_coarse(rays_dev, n, n_coarse, 0, u_coarse_dev, seed, z, st);   // the forward's depths (same draws)
    launch_yolo_aggregate_bwd(raw_dev, g_out_dev, n, n_coarse, d.d_out / 7, s->d_samp.f(), st);
    PNY_HIP(hipGetLastError());
    MlpBackwardCall c;
    c.mode = 1;
    c.rays = rays_dev;
    c.z = z;
    c.K = n_coarse;
    c.n_points = (long long)n * n_coarse;
    c.coarse = 1;
    c.d_out = s->d_samp.f();
    c.accumulate = accumulate & PNY_ACC_ADD;
    c.immediate = true;   // (see pny_query_backward)
    return mlp_backward(s, c, st);
}

int pny_scene_last_backward_stats(pny_scene* s, double flops[3], double kernel_ms[3]) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_last_backward_stats: null scene");
    for (int i = 0; i < 3; ++i) {
        if (flops) flops[i] = s->bwd_flops[i];
        if (kernel_ms) kernel_ms[i] = 0.0;
    }
    if (kernel_ms && s->timing) {
        // events come in groups of 4 per chunk: before the stash forward, after it, after the chain, after the GEMMs + reduce
        // (the chunk's sample-depth kernel, when present, is counted with the GEMMs)
        for (int i = 0; i + 3 < s->bev_used; i += 4) {
            PNY_HIP(hipEventSynchronize(s->bev[i + 3]));
            for (int k = 0; k < 3; ++k) {
                float ms = 0.f;
                PNY_HIP(hipEventElapsedTime(&ms, s->bev[i + k], s->bev[i + k + 1]));
                kernel_ms[k] += ms;
            }
        }
    }
    return PNY_OK;
}

}  // extern "C"
