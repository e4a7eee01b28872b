// Bookkeeping of the training stash reservation (pny_model_defer_weight_grads): who holds how many 64-sample tiles of the two
// model-level stashes, whether a pass a forward stashed is still there, and which arithmetic the flush's weight-gradient GEMM
// runs.  Counting only -- no HIP, no buffers (those are DeferredStash, api_internal.h) -- so that a host compiler can build it alone
// (tests/test_cpu_stash_book.py).
#pragma once
#include <cstdint>

namespace pny {

// The 0 / 1 / 2 codes pny_scene_last_precision, pny_scene_last_backward_precision and pny_model_last_flush_precision report, and
// the matrix arithmetic of a kernel wherever the host code has to name it
enum Prec { PREC_F32 = 0, PREC_H2 = 1 /* split f16 (F16X2) */, PREC_H1 = 2 /* single-plane f16 (F16, F16_TRAIN) */ };

// What one MLP pass of a training pny_render wrote into the reservation (pny_scene_stash_next_render), remembered by the scene for
// the backward of the same epoch
struct StashedPass {
    bool valid = false;
    uint64_t epoch = 0;
    int which = 0;
    long long tile0 = 0, tiles = 0, n_points = 0;
};

// [0] mlp_coarse's stash, [1] mlp_fine's.  Only the operations below write the fields.
struct StashBook {
    bool active = false;
    int ns = 0;                               // views per object the tiles were sized for
    uint64_t epoch = 0;                       // names one reservation: bumped by close() and by open(), and by nothing else
    long long cap[2] = {0, 0}, used[2] = {0, 0};   // tiles reserved / handed out
    bool any_f32 = false, any_h2 = false;     // contributors since the last flush whose gradient GEMMs run fp32 / split f16

    // Passes stashed under the reservation that ends here are no longer owned.  (The contributor flags outlive it: only a
    // flush clears them.)
    void close() {
        active = false;
        used[0] = used[1] = 0;
        ++epoch;
    }
    void open(int views, const long long tiles[2]) {
        for (int w = 0; w < 2; ++w) {
            cap[w] = tiles[w];
            used[w] = 0;
        }
        ns = views;
        active = true;
        ++epoch;
    }
    // room for `tiles` more tiles of MLP `which`, for a scene of `views` views per object
    bool has_room(int which, int views, long long tiles) const { return active && views == ns && used[which] + tiles <= cap[which]; }
    // hands out the next `tiles` tiles (has_room first); returns the first of them
    long long take(int which, long long tiles) {
        const long long tile0 = used[which];
        used[which] += tiles;
        return tile0;
    }
    // ... and the record of them a forward leaves for its backward
    StashedPass take_pass(int which, long long tiles, long long n_points) {
        StashedPass sp;
        sp.valid = true;
        sp.epoch = epoch;
        sp.which = which;
        sp.tile0 = take(which, tiles);
        sp.tiles = tiles;
        sp.n_points = n_points;
        return sp;
    }
    // the pass's tiles are still in this reservation
    bool owns(const StashedPass& sp) const { return sp.valid && active && sp.epoch == epoch; }

    // Arithmetic of the flush's weight-gradient GEMM: every backward that leaves tiles for the flush notes the arithmetic of its own
    // gradient GEMMs; any fp32 contributor (or no running max |dY| to scale by) puts the flush on fp32, else any split-f16 one on
    // split f16, and only F16_TRAIN contributors alone on the single-plane GEMM.
    void note_contributor(Prec gemm) {
        if (gemm == PREC_F32) any_f32 = true;
        if (gemm == PREC_H2) any_h2 = true;
    }
    Prec flush_gemm(bool have_absmax) const { return (!have_absmax || any_f32) ? PREC_F32 : any_h2 ? PREC_H2 : PREC_H1; }
    // MLP `which` was flushed: its tiles are free again.  The epoch does NOT change: a coarse pass stashed before a fine-only flush
    // (PNYOLO_SPLIT_FLUSH: mlp_fine's flush runs between the scenes' fine and coarse passes) is still owned by its backward
    // afterwards.  clear_contributors: not after a fine-only flush, whose step's coarse-only flush still needs them.
    void flushed(int which, bool clear_contributors) {
        used[which] = 0;
        if (clear_contributors) any_f32 = any_h2 = false;
    }
};

}  // namespace pny
