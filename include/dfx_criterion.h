/*
 * dfx_criterion.h -- C ABI of the training criterion: matching costs, linear sum assignment, set loss.
 *
 * Restates what the reference's HungarianMatcher + SetCriterion compute (ref models/matcher.py:45-100,
 * models/deformable_detr_multi_plusplus.py:353-546, models/segmentation.py:196-229, util/box_ops.py:32-69) for ALL
 * prediction sets of one criterion call - the last layer, the aux sets, enc_outputs - with one launch per kernel.
 *
 * Ragged layout.  Set s has Q_s queries, B images are shared.  The logits of all sets lie in one [rows, 3] fp32 buffer
 * and the boxes (cx, cy, w, h) in one [rows, 4] buffer, rows = B * sum(Q_s), set after set, image after image.  Targets
 * are stored once: labels [Ttot] int32, boxes [Ttot, 4] fp32, image after image.  The int32 descriptor `desc` holds
 *   desc[3*s + 0]   Q_s
 *   desc[3*s + 1]   first row of set s in the two buffers  (= B * sum of Q_s' over s' < s)
 *   desc[3*s + 2]   1: the labels of this set are all 0 (enc_outputs), 0: the stored labels
 *   desc[3*S + b]   tgt_off[b], b = 0 .. B: image b owns targets tgt_off[b] .. tgt_off[b+1]-1; tgt_off[B] = Ttot
 * and lives in device memory for the kernels, in host memory for dfx_lsap_ragged_f32.
 *
 * Three columns.  The classification loss weights the columns by (0, 1, 0.001f) and replaces the target of column 2 by
 * "the target of column 1 is not 1", as the reference's loss does: the entries are built for exactly 3 classes.
 * Labels outside 0..2 make the cost NaN (which the assignment refuses) and count as "no column" in the loss.
 *
 * Same conventions as dfx_msda.h: device pointers, caller-owned buffers, enqueue-only on `stream`, no allocation and no
 * synchronisation inside (graph-capturable), 0 / negative return code, text by dfx_last_error().  No atomics: every sum
 * is taken in an order fixed by the shapes alone, so a call gives the same bits every time.  The kernels read fp32,
 * evaluate the set loss and its gradients in fp64 per element and round once when they store.
 * Additions to the ABI: dfx_abi_version() stays.
 */
#ifndef DFX_CRITERION_H
#define DFX_CRITERION_H

#ifdef __cplusplus
extern "C" {
#endif

#define DFX_ENONFINITE (-4) /* dfx_lsap_*: the cost matrix holds a NaN or an infinity */

/* cost[...] of every (set, image, query, target-of-that-image) pair, the block-diagonal only: the matrix of (s, b) is a
 * contiguous row-major [Q_s, T_b] block at  Ttot * sum(Q_s' < s) + Q_s * tgt_off[b];  sum(Q_s) * Ttot floats in all.
 *   C = cost_bbox * L1(box, tbox) + cost_class * (pos - neg) + cost_giou * (-GIoU)
 * with p = sigmoid(logit[label]),  pos = 0.25 (1-p)^2 (-log(p + 1e-8)),  neg = 0.75 p^2 (-log(1 - p + 1e-8)). */
int dfx_match_cost_f32(const float *logits, const float *boxes, const int *tgt_labels, const float *tgt_boxes,
                       const int *desc, int S, int B, int rows, int Ttot,
                       float cost_class, float cost_bbox, float cost_giou, float *cost, void *stream);

/* row_target[rows]: global index (into the target arrays) of the target matched to the row, or -1.
 * out[S, 5] = loss_ce, class_error, loss_bbox, loss_giou, cardinality_error of every set:
 *   loss_ce            sum over the set's B*Q*3 elements of alpha_c * BCE(x, t) * (1 - p_t)^2, times inv_num_boxes; BCE in
 *                      the stable form max(x,0) - x t + log1p(exp(-|x|)); column 0 (alpha 0) is not evaluated
 *   class_error        100 - 100 * (matched rows whose arg-max is their label) / (matched rows); 100 without matched rows
 *   loss_bbox          sum of |box - tbox| over matched rows and 4 coordinates, times inv_num_boxes
 *   loss_giou          sum of 1 - GIoU over matched rows, times inv_num_boxes
 *   cardinality_error  mean over the images of | #(rows whose arg-max is not column 2) - T_b |
 * Arg-max ties go to the lowest index.  One workgroup per set. */
int dfx_set_loss_forward_f32(const float *logits, const float *boxes, const int *tgt_labels, const float *tgt_boxes,
                             const int *row_target, const int *desc, int S, int B, int rows, int Ttot,
                             double inv_num_boxes, float *out, void *stream);

/* Gradients of sum(grad_out * out) in closed form (nothing of the forward is replayed or kept); of grad_out [S, 5] only
 * columns 0, 2 and 3 are read.  grad_logits [rows, 3] and grad_boxes [rows, 4] are written in full; either may be NULL.
 * Column 0 of grad_logits and the box gradient of unmatched rows are exactly zero.  Where two box edges coincide exactly,
 * the max / min inside GIoU hands the whole gradient to the target's side (autograd splits it in two): a set of measure
 * zero on which the sub-gradient is not unique.  The clamp of the intersection's extent at 0 passes the gradient at exactly 0
 * too, as the reference's clamp(min=0) does: a prediction of zero width between the target's edges gets the derivative of
 * the intersection in its width, the only one there is on w >= 0. */
int dfx_set_loss_backward_f32(const float *grad_out, const float *logits, const float *boxes, const int *tgt_labels,
                              const float *tgt_boxes, const int *row_target, const int *desc, int S, int B, int rows,
                              int Ttot, double inv_num_boxes, float *grad_logits, float *grad_boxes, void *stream);

/* HOST code, no kernel and no stream: the rectangular linear sum assignment of one row-major [Q, T] fp32 matrix in host
 * memory by shortest augmenting paths (Crouse 2016), accumulated in double.  Writes min(Q, T) pairs sorted by row into
 * rows[] / cols[]; T == 0 or Q == 0 writes nothing.  A NaN or infinite entry: DFX_ENONFINITE. */
int dfx_lsap_f32(const float *cost, int Q, int T, int *rows, int *cols);

/* HOST code: dfx_lsap_f32 on every (s, b) block of a dfx_match_cost_f32 result copied to host memory, `desc` in host
 * memory too.  Writes row_target[rows] as dfx_set_loss_forward_f32 reads it.  The first block with a NaN or infinite
 * entry: DFX_ENONFINITE. */
int dfx_lsap_ragged_f32(const float *cost, const int *desc, int S, int B, int rows, int Ttot, int *row_target);

#ifdef __cplusplus
}
#endif
#endif /* DFX_CRITERION_H */
