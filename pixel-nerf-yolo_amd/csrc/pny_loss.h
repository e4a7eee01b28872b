// Arguments of the two training-loss kernels (loss.hip) and their launchers, shared with the C entry points (loss_api.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pny {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_MAX_GRID = 128;        // workgroups of one launch at the most (= rows of the partial-sum table)
constexpr int LOSS_RGB_PER_GROUP = 2048;  // elements one workgroup takes before a second one is launched
constexpr int LOSS_YOLO_PER_GROUP = 1024; // (cell, anchor) pairs likewise
constexpr int LOSS_MAX_SUMS = 4;          // partial sums per workgroup (rgb: 2, yolo: 4)
// per-stream workspace: the ticket counter (its own 256 bytes), then LOSS_MAX_GRID x LOSS_MAX_SUMS doubles
constexpr size_t LOSS_WS_BYTES = 256 + (size_t)LOSS_MAX_GRID * LOSS_MAX_SUMS * sizeof(double);

struct RgbLossArgs {
    const float* coarse;
    const float* fine;       // or null: no fine pass
    const float* gt;
    long long n;
    int l1_coarse, l1_fine;
    float lambda_coarse, lambda_fine;
    float* terms;            // {rc, rf, t}
    float* d_coarse;         // or null
    float* d_fine;           // or null
    unsigned* ticket;
    double* partials;
};

struct YoloLossArgs {
    const float* pred;       // (cells, A, 5 + C)
    const float* target;     // (cells, A, 6)
    const float* anchors;    // (A, 2)
    long long items;         // cells * A
    int A, C;
    float w_box, w_obj, w_noobj, w_cls;
    float* terms;            // {total, box, object, no_object, class}
    int* counts;             // {n_obj, n_noobj}, or null
    float* d_pred;           // or null
    unsigned* ticket;
    double* partials;
};

constexpr int LOSS_MAX_SCALES = 4;        // scales of one yolo_loss_batches launch
constexpr int LOSS_MAX_SEGMENTS = 4096;   // mini-batches ("segments") of one yolo_loss_batches launch = its workgroups

// yolo_loss_batches_kernel: the YOLO loss of every mini-batch of a training step, one workgroup per mini-batch.  The
// mini-batches are computed from rows / batch_rows in the kernel: scale s owns ceil(rows[s] / batch_rows) consecutive ones.
struct YoloBatchesArgs {
    const float* pred;       // (sum rows, A, 5 + C)
    const float* target;     // (sum rows, A, 6)
    const float* anchors;    // (n_scales, A, 2)
    int n_scales, batch_rows;
    long long rows[LOSS_MAX_SCALES];
    int segments;            // M = the grid
    int A, C;
    float w_box, w_obj, w_noobj, w_cls;
    float* terms_seg;        // (M, 5) {total, box, object, no_object, class} per mini-batch
    int* counts_seg;         // (M, 2) {n_obj, n_noobj}, or null
    float* step;             // [6] {sum total, sum total / M, sum box / M, sum object / M, sum no_object / M, sum class / M}
    float* d_pred;           // or null
    unsigned* ticket;
};

int loss_grid(long long items, int per_group);
void launch_rgb_loss(const RgbLossArgs& a, hipStream_t st);
void launch_yolo_loss(const YoloLossArgs& a, hipStream_t st);
void launch_yolo_loss_batches(const YoloBatchesArgs& a, hipStream_t st);

}  // namespace pny
