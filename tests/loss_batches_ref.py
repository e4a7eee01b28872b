"""
fp64 restatement of a YOLO training step's losses as the reference's trainer computes them
(train/trainlib/YoloTrainer.py:149-208): the rows of every scale are cut into mini-batches of ray_batch_size rows, the loss
is called per mini-batch (tests/loss_ref.py, itself pinned to the reference's goldens) and backpropagated, and the five
values are read back as fp32 numbers, summed on the host and divided by the number of mini-batches.  The yardstick of
pny_yolo_loss_batches / loss.YoloLoss.forward_batches (test_cpu_yolo_loss_batches.py, test_gpu_yolo_loss_batches.py).
"""
import torch

import loss_ref

F64 = torch.float64


def segments(rows_per_scale, batch_rows):
    """-> [(scale, first row, rows)] in the trainer's order: per scale, torch.split of its rows by batch_rows."""
    out, base = [], 0
    for s, rows in enumerate(int(r) for r in rows_per_scale):
        out += [(s, base + r0, min(batch_rows, rows - r0)) for r0 in range(0, rows, batch_rows)]
        base += rows
    return out


def step_values(terms_seg):
    """The trainer's sums (:196-208) of per-mini-batch terms (M, 5): every value is read back as the fp32 number the loss
    returned (`.item()`), added in mini-batch order in the host's fp64 and divided by M at the end.
    -> (6,) fp64 {sum total, sum total / M, sum box / M, sum object / M, sum no_object / M, sum class / M}."""
    rows = terms_seg.detach().cpu().to(torch.float32).tolist()
    total = [0.0] * 5
    for r in rows:
        for j in range(5):
            total[j] += r[j]
    return torch.tensor([total[0]] + [t / len(rows) for t in total], dtype=F64)


def yolo_batches(pred, target, anchors, weights, rows_per_scale, batch_rows):
    """pred (N, A, 5 + C), target (N, A, 6), anchors: S tensors (A, 2) or one (S, A, 2)
    -> (terms (M, 5), counts (M, 2) int64, d (sum_m total_m) / d pred (N, A, 5 + C), step (6,)), fp64, on the CPU."""
    pred, target = pred.detach().cpu(), target.detach().cpu()
    terms, counts, grads = [], [], []
    for s, r0, n in segments(rows_per_scale, batch_rows):
        t, g, n_obj, n_noobj = loss_ref.yolo_with_grads(pred[r0:r0 + n], target[r0:r0 + n], anchors[s].detach().cpu(), weights)
        terms.append(t)
        counts.append([n_obj, n_noobj])
        grads.append(g)
    terms = torch.stack(terms)
    return terms, torch.tensor(counts, dtype=torch.int64), torch.cat(grads), step_values(terms)
