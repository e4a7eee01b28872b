// The training stash: the one definition of its layout, for the kernels that write it (mlp.hip, mlp_h2.hip STASH forward;
// mlp_bwd.hip, mlp_bwd_h2.hip chain), the kernels that read it (dw_gemm, latent_grad, mlp_dz_kernel) and the host
// (train_api.hip).  Plain C++: a host compiler can include this file on its own (tests/test_cpu_stash_layout.py).
#pragma once

#if defined(__HIPCC__)
#define PNY_HD __host__ __device__ __forceinline__
#else
#define PNY_HD inline
#endif

namespace pny {

// Training stash (64-sample tiles; every tensor slot is [feature/4][64 samples] float4, i.e. the LDS B-operand layout):
//   X record of a tile  = NS views x { x_in (16 rows), z (L/4 rows), per view block b: relu(h_in(b)), relu(net(b)) }
//                         + post part { per post block: relu(h_in(b)), relu(net(b)) ; relu(h_top) }
//   dY record of a tile = NS views x { per view block b: dnet(b), dh_in(b) }
//                         + post part { d_raw (16 rows), dh_top, per post block b: dnet(b), dh_in(b) }
//     (dh_in of the first post-combine block holds dhm = dh / NS, the gradient every view's last block receives; when
//      there is no post-combine block dhm IS dh_top)
// Offsets are in floats.  SLOT = 64 * 512 floats.
constexpr int STASH_ROWS = 512;        // features of a slot: d_hidden
constexpr int STASH_SMALL_ROWS = 64;   // features of a 16-row slot (x_in, d_raw): the padded d_in / d_out
constexpr int STASH_SLOT = 64 * STASH_ROWS;
constexpr int STASH_SMALL = 64 * STASH_SMALL_ROWS;

// Record of tile `tile` in a stash whose records are `stride` floats apart
template <class T>
PNY_HD T* stash_record(T* base, long long stride, long long tile) { return base + tile * stride; }

// Every accessor returns the offset of a slot inside its tile record, in floats (a record stays below 2^31 bytes: the chain
// kernels address it with 32-bit byte offsets).  v = view, b = per-view block, i = post-combine block (block nvb + i).
struct StashLayout {
    long long x_tile, dy_tile;            // record strides
    int x_view, o_in, o_z, o_act;         // X: stride of a view's part; offsets of x_in, z and the block slots inside it
    int x_post;                           // X: offset of the post part
    int dy_view;                          // dY: stride of a view's part
    int dy_post;                          // dY: offset of the post part

    // per-view blocks (in front of the cross-view mean) and post-combine blocks
    PNY_HD int nvb() const { return dy_view / (2 * STASH_SLOT); }
    PNY_HD int npost() const { return (int)((x_tile - x_post) / (2 * STASH_SLOT)); }

    // ---- X record
    PNY_HD unsigned x_in(int v) const { return (unsigned)v * (unsigned)x_view + (unsigned)o_in; }
    PNY_HD unsigned x_z(int v) const { return (unsigned)v * (unsigned)x_view + (unsigned)o_z; }
    PNY_HD unsigned x_h(int v, int b) const { return x_view_slot(v, 2 * b); }           // relu(h_in(b))
    PNY_HD unsigned x_net(int v, int b) const { return x_view_slot(v, 2 * b + 1); }     // relu(net(b))
    PNY_HD unsigned x_post_h(int i) const { return x_post_slot(2 * i); }
    PNY_HD unsigned x_post_net(int i) const { return x_post_slot(2 * i + 1); }
    PNY_HD unsigned x_top() const { return x_post_slot(2 * npost()); }                  // relu(h_top)
    // ---- dY record
    PNY_HD unsigned dy_dnet(int v, int b) const { return dy_view_slot(v, 2 * b); }
    PNY_HD unsigned dy_dh(int v, int b) const { return dy_view_slot(v, 2 * b + 1); }    // dh_in(b): the gradient at block b's entry
    PNY_HD unsigned dy_raw() const { return (unsigned)dy_post; }
    PNY_HD unsigned dy_top() const { return dy_post_slot(0); }
    PNY_HD unsigned dy_post_dnet(int i) const { return dy_post_slot(1 + 2 * i); }
    PNY_HD unsigned dy_post_dh(int i) const { return dy_post_slot(2 + 2 * i); }
    // ---- derived names
    PNY_HD unsigned dy_dhm() const { return npost() > 0 ? dy_post_dh(0) : dy_top(); }
    // dY of lin_in (and of lin_z[0]'s bias): the gradient at the first block's entry (dhm, one per tile, without per-view
    // blocks: dy_view is 0 then)
    PNY_HD unsigned dy_lin_in(int v) const { return dy_view > 0 ? dy_dh(v, 0) : dy_dhm(); }
    // dY of fc_1 = the gradient of the residual stream behind the block: the next block's dh_in, dhm behind the last per-view
    // block, dh_top behind the last block
    PNY_HD unsigned dy_fc1(int v, int b) const { return b + 1 < nvb() ? dy_dh(v, b + 1) : dy_dhm(); }
    PNY_HD int dy_fc1_stride(int b) const { return b + 1 < nvb() ? dy_view : 0; }   // per-view stride of dy_fc1 (dhm: one per tile)
    PNY_HD unsigned dy_post_fc1(int i) const { return i + 1 < npost() ? dy_post_dh(i + 1) : dy_top(); }

    // ---- records
    template <class T>
    PNY_HD T* x_record(T* base, long long tile) const { return stash_record(base, x_tile, tile); }
    template <class T>
    PNY_HD T* dy_record(T* base, long long tile) const { return stash_record(base, dy_tile, tile); }

private:
    PNY_HD unsigned x_view_slot(int v, int s) const { return (unsigned)v * (unsigned)x_view + (unsigned)o_act + (unsigned)s * (unsigned)STASH_SLOT; }
    PNY_HD unsigned x_post_slot(int s) const { return (unsigned)x_post + (unsigned)s * (unsigned)STASH_SLOT; }
    PNY_HD unsigned dy_view_slot(int v, int s) const { return (unsigned)v * (unsigned)dy_view + (unsigned)s * (unsigned)STASH_SLOT; }
    PNY_HD unsigned dy_post_slot(int s) const { return (unsigned)dy_post + (unsigned)STASH_SMALL + (unsigned)s * (unsigned)STASH_SLOT; }
};

// Layout of a model with n_blocks residual blocks, the cross-view mean in front of block combine_layer, ns views per object
// and a latent of L channels.
PNY_HD StashLayout stash_layout(int n_blocks, int combine_layer, int ns, int L) {
    const int nvb = combine_layer < n_blocks ? combine_layer : n_blocks, npost = n_blocks - nvb;
    StashLayout l;
    l.o_in = 0;
    l.o_z = STASH_SMALL;
    l.o_act = STASH_SMALL + L * 64;
    l.x_view = l.o_act + 2 * nvb * STASH_SLOT;
    l.x_post = ns * l.x_view;
    l.x_tile = (long long)l.x_post + (long long)(2 * npost + 1) * STASH_SLOT;
    l.dy_view = 2 * nvb * STASH_SLOT;
    l.dy_post = ns * l.dy_view;
    l.dy_tile = (long long)l.dy_post + STASH_SMALL + (long long)(1 + 2 * npost) * STASH_SLOT;
    return l;
}

}  // namespace pny
