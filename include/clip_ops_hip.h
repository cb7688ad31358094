/* clip_ops_hip.h -- C ABI of libclip_ops_hip.so: the small-tensor chains of the clip train step as single gfx950
 * kernels.
 *
 * The decoder / criterion side of a MeMOTR train step is hundreds of element-wise torch kernels on tensors of a
 * few thousand elements (matching cost, focal / L1 / GIoU losses, anchor embedding, box refinement).  On MI355X
 * each costs 5-7 us of queue time whatever its size, forward and again (2-3x) backward; these entry points
 * evaluate one whole chain per launch.  Arithmetic follows the reference formulas cited per function; all
 * tensors are fp32 (indices int64), device pointers, plain sizes and element strides -- no torch types.
 *
 * Every function returns 0 on success or a non-zero code (clipops_last_error() has the text) and launches on
 * `stream` (a hipStream_t passed as void*; NULL = the default stream).  Nothing here synchronises.
 */
#ifndef CLIP_OPS_HIP_H
#define CLIP_OPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIPOPS_ABI_VERSION 12

int clipops_abi_version(void);
const char *clipops_last_error(void);

/* Matching cost of `n_layers` decoder layers at once (reference models/matcher.py:83-121, focal-style class cost):
 *   cost[l,q,t] = w_bbox * |box[l,q] - gt_box[t]|_1 + w_class * (pos - neg)(sigmoid(logit[l,q,gt_label[t]]))
 *                 + w_giou * (-GIoU(xyxy(box[l,q]), xyxy(gt_box[t])))
 * logits: element (l,q,k) at logits[l*logit_sl + q*logit_sq + k]; boxes: (l,q,c) at boxes[l*box_sl + q*box_sq + c]
 * (cxcywh).  gt_labels (T) int64, gt_boxes (T,4) and cost (n_layers,Q,T) are contiguous.  A label outside [0, K) is
 * clamped into it (the reference's index would wrap or raise); T == 0 is a no-op. */
int clipops_match_cost_f32(const float *logits, long logit_sl, long logit_sq, const float *boxes, long box_sl,
                           long box_sq, const int64_t *gt_labels, const float *gt_boxes, int n_layers, int Q, int K,
                           int T, float w_class, float w_bbox, float w_giou, float *cost, void *stream);

/* L1 and GIoU loss of `n` (prediction, target) box pairs (reference models/criterion.py:417-440: l1_loss(reduction
 * none).sum(-1) and 1 - diag(generalized_box_iou(xyxy(pred), xyxy(tgt)))).
 * Prediction i is row  lay[i]*row_mul + row_add + qidx[i]  of `boxes` (rows of 4 floats, cxcywh); target i is row
 * gidx[i] of tgt_boxes (gidx == NULL: row i).  weight (n) may be NULL; both outputs are multiplied by it. */
/* (The backward follows torch's autograd where the function has a kink: a max / min of two equal corners passes half the
 * gradient to each side, clamp(min=0) passes it at exactly 0, |x| has slope 0 at 0 -- held to float64 autograd on boxes
 * that tie, share an edge or share a corner by tests/test_clip_ops_truth_gpu.py.) */
int clipops_pair_box_loss_fwd_f32(const float *boxes, const int64_t *lay, const int64_t *qidx, long row_mul,
                                  long row_add, const float *tgt_boxes, const int64_t *gidx, const float *weight,
                                  int n, float *l1, float *giou_loss, void *stream);
/* Gradient of the above with respect to the prediction rows: grad_boxes (same row layout as `boxes`) receives
 * plain stores for the n rows (the pairs of one call address distinct rows); the caller zero-fills it. */
int clipops_pair_box_loss_bwd_f32(const float *boxes, const int64_t *lay, const int64_t *qidx, long row_mul,
                                  long row_add, const float *tgt_boxes, const int64_t *gidx, const float *weight,
                                  int n, const float *grad_l1, const float *grad_giou, float *grad_boxes,
                                  void *stream);

/* IoU of n box pairs, no gradient (reference models/criterion.py:354-367, the `iou` field of the tracks):
 * iou[i] = IoU(xyxy(boxes[i]), xyxy(tgt_boxes[gidx[i]]))  (gidx == NULL: row i); boxes (n,4) cxcywh contiguous. */
int clipops_pair_iou_f32(const float *boxes, const float *tgt_boxes, const int64_t *gidx, int n, float *iou,
                         void *stream);

/* ---- per-frame bookkeeping of the criterion (round 6, ABI 10) ----
 * Which ground truth a carried track owns, and which ground truths nobody owns (reference models/criterion.py:166-182:
 * the `gt_ids_to_idx` dict -- the LAST ground truth wins when a frame repeats an id -- and the `unmatched` list):
 *   matched_idx[i] = max { j : gt_ids[j] == track_ids[i] }  or -1;   gt_free[j] = 1.0 if no track carries gt_ids[j] else 0.0
 * (float: it travels to the host in front of the cost tensor).  Replaces seven torch launches (compare / arange / product
 * / amax / subtract / any / not) by one. */
int clipops_track_ownership_i64(const int64_t *track_ids, int n_tracks, const int64_t *gt_ids, int n_gt,
                                int64_t *matched_idx, float *gt_free, void *stream);
/* Classification targets of every decoder layer for the focal loss (reference models/criterion.py:300-330):
 *   labels (n_layers, n_det + n_tracks) = K (background);  columns n_det.. of the layers with late[l] != 0 = the label of the
 *   ground truth the track owns (matched_idx, -1: background);  then labels[lay[p], q[p]] = gt_labels[g[p]] for the n_pairs
 *   matched (layer, detect query, ground truth) triples.  Replaces eleven torch launches (fill / gather / index_put /
 *   compare / clamp / gather / two fills / two selects / slice copy) by one. */
int clipops_focal_labels_i64(const int64_t *lay, const int64_t *q, const int64_t *g, int n_pairs,
                             const int64_t *gt_labels, int n_gt, const int64_t *matched_idx, int n_tracks,
                             const uint8_t *late, int n_layers, int n_det, int K, int64_t *labels, void *stream);

/* Sigmoid focal loss of stacked layers (reference models/criterion.py:442-467, RetinaNet form): per layer l
 *   loss[l] = sum_q mean_k  a_t * ce * (1 - p_t)^gamma,   target one-hot of labels[l,q] (label == K: background).
 * logits element (l,q,k) at logits[l*sl + q*sq + k]; labels (n_layers,Nq) int64 contiguous; loss (n_layers).
 * One workgroup per layer with a fixed-order reduction: results are run-to-run identical.  alpha < 0: no a_t weight.
 * Any gamma >= 1 and gamma == 0 are differentiated (gamma == 0: the modulating factor is constant, its derivative zero
 * even where 1 - p_t has rounded to 0); 0 < gamma < 1 has an infinite derivative there and is not supported.  Finite for
 * every finite logit (held on [-90, 90], past the overflow of expf at 88.72). */
int clipops_focal_fwd_f32(const float *logits, long sl, long sq, const int64_t *labels, int n_layers, int Nq, int K,
                          float alpha, float gamma, float *loss, void *stream);
/* grad_logits (n_layers,Nq,K) contiguous = grad_loss[l] * d loss[l] / d logit. */
int clipops_focal_bwd_f32(const float *logits, long sl, long sq, const int64_t *labels, int n_layers, int Nq, int K,
                          float alpha, float gamma, const float *grad_loss, float *grad_logits, void *stream);

/* Sine embedding of box coordinates (reference models/utils.py:78-85, `pos_to_pos_embed`): pos (n,K) ->
 * out (n, K*F),  out[i, k*F + j] = (j even ? sin : cos)((pos[i,k] * scale) / dim_t[j]);  dim_t (F) is the
 * temperature ladder the caller computed once (passed in so that both sides use the same floats). */
int clipops_sine_embed_fwd_f32(const float *pos, const float *dim_t, long n, int K, int F, float scale, float *out,
                               void *stream);
/* grad_pos (n,K) = sum_j grad_out[i, k*F + j] * d out / d pos. */
int clipops_sine_embed_bwd_f32(const float *pos, const float *dim_t, long n, int K, int F, float scale,
                               const float *grad_out, float *grad_pos, void *stream);

/* logit with both odds clamped (reference utils/utils.py:61-74, `inverse_sigmoid`), n elements:
 *   y = log(clamp(x, eps, 1) / clamp(1 - x, eps, 1));  the backward applies torch's clamp masks. */
int clipops_inverse_sigmoid_fwd_f32(const float *x, long n, float eps, float *y, void *stream);
int clipops_inverse_sigmoid_bwd_f32(const float *x, const float *grad_y, long n, float eps, float *grad_x, void *stream);

/* Iterative box refinement of the decoder (reference models/deformable_decoder.py:139-149, 4-d references):
 *   out = sigmoid(delta + inverse_sigmoid(ref)), n elements.  Backward from the saved `out`; grad_ref may be NULL. */
int clipops_refine_boxes_fwd_f32(const float *delta, const float *ref, long n, float eps, float *out, void *stream);
int clipops_refine_boxes_bwd_f32(const float *out, const float *ref, const float *grad_out, long n, float eps,
                                 float *grad_delta, float *grad_ref, void *stream);

/* Layer 0 of the Deformable-DETR variant (USE_DAB: False), both boxes from one `delta`; n_rows rows of four:
 *   out_head[r,c] = sigmoid(delta[r,c] + inverse_sigmoid(ref[r,c]))          -- the model's box head, 4-d reference
 *   out_dec[r,c]  = out_head[r,c] for c < 2, sigmoid(delta[r,c]) for c >= 2  -- the decoder's box, 2-d reference
 * out_head is bit-equal to clipops_refine_boxes_fwd_f32(delta, ref); out_dec's last two columns are bit-equal to
 * clipops_refine_boxes_fwd_f32(delta, 0.5) (inverse_sigmoid(0.5) is exactly 0).  The backward is
 * clipops_refine_boxes_bwd_f32 on out_head: out_dec is only ever used detached.  The outputs must not alias.
 * (Added without a new CLIPOPS_ABI_VERSION: no existing entry point changed, and a library built before it is
 *  caught twice -- the source hash of the build rebuilds it, and binding the symbol table fails on the missing name.) */
int clipops_refine_boxes_split_fwd_f32(const float *delta, const float *ref, long n_rows, float eps,
                                       float *out_head, float *out_dec, void *stream);

/* Column sums of a small row-major matrix: out[c] = sum_r x[r*cols + c] -- the bias gradient of a Linear over a few
 * hundred query rows.  torch's generic reduction takes 12-17 us for 310 x 256 .. 2048 on MI355X (one of ~400 such calls
 * per train step); this one tiles 32 columns x 8 row lanes per workgroup and sums in a fixed order.  All column-sum
 * entry points accumulate in fp64 and round once (error <= half an ulp of the result + the rounding of the partials in
 * the two-pass forms), whatever the cancellation between rows. */
int clipops_colsum_f32(const float *x, long rows, int cols, float *out, void *stream);
/* First pass for tall matrices: partial[k*cols + c] = sum of rows [k*chunk_rows, (k+1)*chunk_rows) of column c,
 * k < ceil(rows / chunk_rows); clipops_colsum_f32 over `partial` finishes (fixed order end to end). */
int clipops_colsum_partial_f32(const float *x, long rows, int cols, int chunk_rows, float *partial, void *stream);
/* The same from bf16 storage (fp32 partial sums): bias gradients of the bf16 linears -- torch's own multi-block
 * reduction returned garbage inside replayed hipGraphs (round 3, profiles/r03_graph_memset_probe.txt). */
int clipops_colsum_partial_bf16(const uint16_t *x, long rows, int cols, int chunk_rows, float *partial, void *stream);

/* Multi-head self-attention over the decoder queries (reference models/deformable_decoder.py:245-249: the
 * nn.MultiheadAttention call with query = key = tgt + pos, value = tgt; here after the input projections):
 *   out[b,i,h,:] = sum_j softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]  |  key_mask[b,j] == 0) * v[b,j,h,:]
 * head_dim is 32, L <= CLIPOPS_MHA_MAX_L; fp32, exact softmax (per-lane online softmax merged over the 8 lanes of a
 * query row), K and V of a head staged in LDS.  q / k / v are addressed as base + b*batch_stride + i*row_stride + h*32
 * (element strides), so the packed (B, L, 2E) projection of q and k needs no copy; key_mask (B, L) bytes, non-zero =
 * ignore that key, may be NULL; out (B, L, H*32) contiguous; lse (B, H, L) receives max + log(sum) per row for the
 * backward.  Replaces the AOTriton kernels behind F.scaled_dot_product_attention on this path.
 * A (batch, row) whose keys are ALL masked has no softmax: its out is NaN (0 * inf, what torch's softmax over -inf gives
 * too), its lse -inf, and the backward gives it and its keys zero gradients; other batches of the call are unaffected
 * bit for bit.  A row with ONE live key gets that key's v bit for bit. */
#define CLIPOPS_MHA_MAX_L 512
int clipops_mha_fwd_f32(const float *q, const float *k, const float *v, long q_bs, long q_rs, long k_bs, long k_rs,
                        long v_bs, long v_rs, const uint8_t *key_mask, int B, int H, int L, float scale, float *out,
                        float *lse, void *stream);
/* Gradients of the above.  grad_out (B, L, H*32) contiguous; grad_q / grad_k / grad_v are addressed like q / k / v
 * (each its own batch / row stride, so grad_q and grad_k can be the two halves of one (B, L, 2E) buffer).  Two kernels:
 * one by query rows (grad_q), one by key rows (grad_k, grad_v); probabilities are recomputed from lse, from the forward's
 * own score bits ((q * scale) . k in one summation order everywhere), and dO . O is summed in the order of dO . v: a row
 * with one live key gets grad_q = 0 and its key grad_k = 0 exactly, grad_v = the sum of dO.  Masked keys get exact zeros. */
int clipops_mha_bwd_f32(const float *q, const float *k, const float *v, long q_bs, long q_rs, long k_bs, long k_rs,
                        long v_bs, long v_rs, const uint8_t *key_mask, const float *out, const float *lse,
                        const float *grad_out, int B, int H, int L, float scale, float *grad_q, long gq_bs, long gq_rs,
                        float *grad_k, long gk_bs, long gk_rs, float *grad_v, long gv_bs, long gv_rs, void *stream);

/* Residual add + LayerNorm over rows of 256 floats (the post-norm blocks of the encoder / decoder layers, reference
 * models/deformable_encoder.py:104-106, :126-127, models/deformable_decoder.py:251-252, :271-272, :311-312):
 *   sum = x + res;  y = (sum - mean) * rstd * gamma + beta   (mean / biased variance over the 256 columns, eps inside
 *   the sqrt).  One wavefront per row, 4 floats per lane.  `sum` (rows,256) and `stats` (rows,2) = (mean, rstd) are
 *   kept for the backward.  Replaces an element-wise add + native_layer_norm (2 kernels) forward. */
#define CLIPOPS_LN_COLS 256
int clipops_add_layer_norm_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta, long rows,
                                   float eps, float *sum, float *y, float *stats, void *stream);
/* Backward: grad_sum (rows,256) = d/d(x) = d/d(res);  partial (ceil(rows/chunk_rows), 512) receives per-chunk column
 * sums of [grad_y * xhat | grad_y]; clipops_colsum_f32 over it yields [grad_gamma | grad_beta].  Replaces
 * layer_norm_grad_input + two gamma/beta kernels + the add's fan-out. */
int clipops_add_layer_norm_bwd_f32(const float *grad_y, const float *sum, const float *stats, const float *gamma,
                                   long rows, int chunk_rows, float *grad_sum, float *partial, void *stream);

/* ---- the encoder layer's fan-ins folded into the LayerNorm kernels (ABI 11) ----
 * Forward with a second output q = y + pos (all (rows,256)), written in the same pass from the y in registers: the next
 * encoder layer's query (reference models/deformable_encoder.py:88-90, with_pos_embed), otherwise an element-wise add
 * over the tensor this kernel has just written.  sum / y / stats are bit for bit those of clipops_add_layer_norm_fwd_f32,
 * q is the fp32 sum y + pos. */
int clipops_add_layer_norm_pos_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta,
                                       const float *pos, long rows, float eps, float *sum, float *y, float *q,
                                       float *stats, void *stream);
/* Backward for an output with up to three consumers: grad_y = (g0 + g1) + g2 over the NON-NULL slots in slot order (at
 * least one), summed in registers -- the sum is never written.  grad_sum and partial as above.  colsum_partial
 * (2 * ceil(rows/chunk_rows), 256) receives the per-chunk column sums of grad_sum (the bias gradient of the Linear that
 * produced `res`), accumulated in fp64 and stored as two float rows per chunk (the fp32 value and its remainder);
 * clipops_colsum_f32 over it yields the column sums rounded once.  No atomics: the results do not vary between runs. */
int clipops_add_layer_norm_fanin_bwd_f32(const float *g0, const float *g1, const float *g2, const float *sum,
                                         const float *stats, const float *gamma, long rows, int chunk_rows,
                                         float *grad_sum, float *partial, float *colsum_partial, void *stream);

/* Linear sum assignment of `n_problems` cost matrices of one shape (n_rows, n_cols) on the device -- what the
 * reference's matcher does on the host with scipy.optimize.linear_sum_assignment after a `.cpu()` copy
 * (models/matcher.py:122-124).  Same algorithm as scipy's (shortest augmenting paths, Crouse 2016, float64 arithmetic
 * on the float32 costs) with the same scan order and tie rule, so the PAIRS are scipy's, not just the cost
 * (memotr_amd/csrc/assign_core.h; held to scipy on 1000 random matrices with ties on the CPU and on the GPU).
 * Element (p, r, c) of `cost` is at cost[p*stride_problem + r*stride_row + c*stride_col] (element strides: a
 * (layers, Q, T) cost tensor and its transpose are both addressable without a copy).  One 64-lane wavefront per
 * problem, all state in LDS, max(n_rows, n_cols) <= CLIPOPS_ASSIGN_MAX_DIM.  Outputs, k = min(n_rows, n_cols):
 * row_ind, col_ind (n_problems, k) int32 -- pairs ordered by row like scipy's result; status (n_problems) int32,
 * may be NULL: k, or -1 for an infeasible matrix (every completion costs +inf: scipy raises ValueError).
 * NOT checked: NaN or -inf entries (scipy raises ValueError on them; this kernel returns some pairing) -- a caller
 * that cannot rule them out tests the matrix first.  Dynamic LDS is 13 n_r + 29 n_c bytes: past 64 KB (n ~ 1560) the
 * launcher raises the kernel's limit itself (round 4).
 * The solver and its parity tests; the model's criterion consumes scipy's result on the host (shelved). */
#define CLIPOPS_ASSIGN_MAX_DIM 2048
int clipops_assign_f32(const float *cost, long stride_problem, long stride_row, long stride_col, int n_problems,
                       int n_rows, int n_cols, int32_t *row_ind, int32_t *col_ind, int32_t *status, void *stream);

/* ---- the backbone's element-wise tail (round 4, ABI 9) ----
 * x = relu(x + shift[c] (+ res)) in place on a convolution's output, NCHW contiguous, `planes` = N * C planes of HW
 * elements; `res` (same shape) may be NULL.  Replaces, in ONE pass, what torchvision's Bottleneck.forward does with a
 * frozen batch norm folded into the convolution (reference models/backbone.py:70-76, FrozenBatchNorm2d :20-60): the
 * per-channel bias add, `out += identity` and the ReLU -- three passes over up to 344 MB per layer and clip.  The bf16
 * form rounds after the bias add and after the residual add like the kernels it replaces.  NaN propagates (x < 0 ? 0 : x). */
int clipops_shift_relu_f32(float *x, const float *shift, const float *res, long planes, int C, long HW, void *stream);
int clipops_shift_relu_bf16(uint16_t *x, const float *shift, const uint16_t *res, long planes, int C, long HW,
                            void *stream);

/* Backward of a query-sized Linear y = x W^T + b (x (rows, in), W (out, in), all contiguous fp32) in one launch:
 * grad_x (rows, in) = G' W, grad_w (out, in) = G'^T x, grad_b (out) = column sums of G', with G' = grad_y or, when the
 * forward fused a ReLU (`y_relu` = its output), grad_y masked by y > 0 -- torch.nn.functional.linear's backward as the
 * reference's decoder / heads / query updater run it a few hundred times per train step on 300-odd rows
 * (models/deformable_decoder.py, models/mlp.py, models/query_updater.py), where it is four dependent launches.  fp32 MFMA
 * (exact fp32 products and sums; the contraction order differs from a library GEMM's).  grad_x / grad_w / grad_b may be
 * NULL (grad_b needs grad_w). */
int clipops_linear_bwd_f32(const float *grad_y, const float *y_relu, const float *x, const float *w, int rows,
                           int in_features, int out_features, float *grad_x, float *grad_w, float *grad_b,
                           void *stream);

/* ... and its forward, y (rows, out) = [relu](x W^T + b) (`bias` may be NULL; in_features a multiple of 4): the same
 * 32 x 32 MFMA tiles with both operands read as 16-byte loads along the contraction. */
int clipops_linear_fwd_f32(const float *x, const float *w, const float *bias, int rows, int in_features,
                           int out_features, int relu, float *y, void *stream);

/* g2 = y > 0 ? g : 0 (the ReLU mask of a Linear whose forward fused the activation; torch's threshold_backward) AND
 * the per-chunk column sums of g2 (first pass of the bias gradient, finished by clipops_colsum_f32 over `partial`
 * (chunks, cols)) in one pass over (rows, cols) contiguous matrices: the encoder FFN's first linear
 * (models/deformable_encoder.py:100-103 of the reference) otherwise re-reads its 914 MB gradient for the sum: 522 vs
 * 637 us.  fp32 only: with 2-byte elements this tile shape loses to the two torch passes (546 vs 358 us, measured). */
int clipops_relu_bwd_colsum_partial_f32(const float *g, const float *y, long rows, int cols, int chunk_rows, float *g2,
                                        float *partial, void *stream);

/* ---- result rows of a tracked sequence, kept on the device (ABI 12) ----
 * The reportable tracks of one frame (reference submit_engine.py:95-112: score and area filters, xyxy pixel boxes),
 * appended to a table that stays on the device until the sequence ends.  For row i of the n live tracks, in float32
 * with every operation rounded once:
 *   s = max_k scores[i,k];  area = ((w * ori_w) * h) * ori_h;  kept when s > score_thresh and area > area_thresh
 *   (both strict; a NaN score or area is dropped, as torch's max and > drop it);
 *   kept rows store x1 = (cx - 0.5 w) ori_w, y1 = (cy - 0.5 h) ori_h, x2 = (cx + 0.5 w) ori_w, y2 = (cy + 0.5 h) ori_h
 *   and s in rows_f (capacity,5), and frame, ids[i], labels[i] in rows_i (capacity,3).
 * Kept rows keep the order of the input and start at row counters[0] as it was when the call began; afterwards
 * counters[0] has grown by the number stored.  A row that would land at or past `capacity` is not stored but counted
 * in counters[1]; nothing is written past the tables.  One 256-thread workgroup (n is tens to hundreds): ballot and
 * population count inside a wavefront, wave totals through LDS, no atomics -- the same inputs give the same table.
 * Calls on one table are issued on one stream.  n == 0 launches nothing.  Returns 1 for a bad argument (negative
 * size, K < 1, null pointer with n > 0), 3 when the launch failed. */
int clipops_result_rows_f32(const float *boxes, const float *scores, const int64_t *ids, const int64_t *labels, int n,
                            int K, int64_t frame, float ori_w, float ori_h, float score_thresh, float area_thresh,
                            float *rows_f, int64_t *rows_i, int32_t *counters, int capacity, void *stream);

/* ---- track hand-over between two frames of a training clip: one gather, one scatter ----
 * The active track set of frame t + 1 is a row-by-row copy of the decoder's outputs of frame t and of the tracks carried
 * into it (reference models/criterion.py:166-194 + :354-367, models/query_updater.py:160-200 without drop / insert
 * augmentation): which output row comes from where is known to the host once the assignment is solved, so it uploads a
 * table and these two launches replace the per-field gathers, concatenations, the row selection and their ~40 backward
 * nodes.  (Added without a new CLIPOPS_ABI_VERSION, like clipops_refine_boxes_split_fwd_f32: no entry point changed.)
 *
 * Sources: row r of source i is src.ptr[i] + r * src.row_stride[i] (element strides; the columns of a row are dense --
 * the decoder's outputs are views of padded graph buffers).  Widths: K logits, 4 box / reference columns, C embedding
 * columns, QW = C (use_dab) or 2C query columns. */
enum {
    CLIPOPS_HO_LOGITS = 0,   /* (n_det + n_tracks, K)   model output: pred_logits */
    CLIPOPS_HO_BOXES,        /* (n_det + n_tracks, 4)   pred_bboxes, cxcywh */
    CLIPOPS_HO_OUTPUTS,      /* (n_det + n_tracks, C)   last decoder layer's output */
    CLIPOPS_HO_QUERIES,      /* (n_det, C)              the queries entering the last decoder layer */
    CLIPOPS_HO_LAST_REF,     /* (n_det, 4)              last_ref_pts */
    CLIPOPS_HO_INIT_REF,     /* (n_det, 4)              init_ref_pts */
    CLIPOPS_HO_DET_EMBED,    /* (n_det, >= C)           det_query_embed; read (and required) only when !use_dab */
    CLIPOPS_HO_PREV_REF,     /* (n_tracks, 4)           the carried tracks' ref_pts */
    CLIPOPS_HO_PREV_LONG,    /* (n_tracks, C)           long_memory */
    CLIPOPS_HO_PREV_LAST,    /* (n_tracks, C)           last_output */
    CLIPOPS_HO_PREV_QUERY,   /* (n_tracks, QW)          query_embed */
    CLIPOPS_HO_PREV_IOU,     /* (n_tracks, 1)           iou */
    CLIPOPS_HO_N_SOURCES
};
typedef struct {
    const float *ptr[CLIPOPS_HO_N_SOURCES];
    long row_stride[CLIPOPS_HO_N_SOURCES];
} clipops_handover_sources;
typedef struct {
    float *ptr[CLIPOPS_HO_N_SOURCES];
} clipops_handover_grads;

/* Forward: base (n_keep, W) contiguous, W = K + 8 + 3C + QW + 1, columns
 *   logits | boxes | ref_pts | output_embed | long_memory | last_output | query_embed | iou,
 * and the int64 fields ids, matched_idx (n_keep each).  Output row o is described by table[3o .. 3o+2] = (kind, s, g):
 *   kind 0, carried track s:  logits, boxes, output_embed = model row n_det + s;  ref_pts, long_memory, last_output,
 *           query_embed = the previous set's row s;  m = prev_matched[s] (the ground truth it owns, -1: none);
 *           iou = m >= 0 ? IoU(box, gt_boxes[m]) : previous iou;  ids = prev_ids[s];  matched_idx = m.
 *   kind 1, new track from detect query s matched to ground truth g:  logits, boxes, output_embed = model row s;
 *           ref_pts = last_ref[s];  last_output = outputs[s];  long_memory = queries[s];
 *           query_embed = queries[s] (use_dab) or det_embed[s][:C] | queries[s];
 *           iou = IoU(box, gt_boxes[g]);  ids = gt_ids[g];  matched_idx = g.
 *   kind 2, unclaimed detection s:  as kind 1 with ref_pts = init_ref[s];  iou = 0;  ids = matched_idx = -1.
 * Then ids = iou < 0.5 ? -1 : ids on every row.  The IoU is the arithmetic of clipops_pair_iou_f32 (one device function);
 * everything else is a copy, bit for bit.  One workgroup per output row.  A table row that points outside its source
 * (s, g or prev_matched[s] out of range, unknown kind) yields a row of zeros with ids = matched_idx = -1: nothing is read
 * or written out of bounds.  prev_* may be NULL when n_tracks == 0.  n_keep == 0 launches nothing. */
int clipops_handover_fwd_f32(const clipops_handover_sources *src, const int64_t *prev_ids, const int64_t *prev_matched,
                             const float *gt_boxes, const int64_t *gt_ids, const int64_t *table, int n_keep, int n_det,
                             int n_tracks, int n_gt, int K, int C, int use_dab, float *base, int64_t *ids,
                             int64_t *matched_idx, void *stream);

/* Backward: from grad_base (n_keep, W) contiguous, the WHOLE gradient tensor of every differentiable source, each
 * contiguous, NULL = not wanted:
 *   grad.ptr[OUTPUTS], [QUERIES] (n_q, C);  [LAST_REF], [INIT_REF] (n_q, 4);  [DET_EMBED] (n_det, det_cols), !use_dab;
 *   [PREV_REF] (n_tracks, 4);  [PREV_LONG], [PREV_LAST] (n_tracks, C);  [PREV_QUERY] (n_tracks, QW).
 * (logits, boxes and iou take no gradient: grad.ptr of these must be NULL.)
 * n_q >= n_det + n_tracks is the row count of the model-output tensors (padded query slots behind the live ones).
 * A source row feeds at most one output row, so the kernel walks the SOURCE rows -- one workgroup per model row r < n_q,
 * then one per previous-set row -- through the inverse tables: inv_q[r] / inv_prev[j] = the output row that reads model
 * row r / previous row j, or -1.  It writes the sum of the columns that came from that row (output_embed + last_output
 * and query_embed + long_memory of a new or unclaimed row: two terms, order-free) and zeros everywhere else: no atomics,
 * no zero-fill beforehand, the same bits every time.  An inverse entry outside [0, n_keep), or one whose table row does
 * not point back at the source row, counts as -1. */
int clipops_handover_bwd_f32(const float *grad_base, const int64_t *table, const int64_t *inv_q, const int64_t *inv_prev,
                             int n_keep, int n_q, int n_det, int n_tracks, int K, int C, int use_dab, int det_cols,
                             const clipops_handover_grads *grad, void *stream);

/* ---- track bank: the online tracker's bookkeeping for B sequences on fixed-size device tables ----
 * (Added without a new CLIPOPS_ABI_VERSION, like the hand-over entries: no entry point changed.)
 * The tracks of stream b live in `cap` slots; a track keeps its slot for life, ids[b][s] = -1 marks a free slot and a
 * free slot holds zeros in every field.  All bank tensors are contiguous: ids, labels, disappear_time int64 (B, cap);
 * boxes, ref_pts (B, cap, 4); logits, scores (B, cap, K); output_embed, long_memory, last_output (B, cap, C);
 * query_embed (B, cap, QW), QW = C (use_dab) or 2C; next_id int64 (B,); counters int32 (B, 2) = live tracks after the
 * last update, births that found no free slot (accumulated); free_list int32 (B, cap): workspace of the update. */
typedef struct {
    int64_t *ids, *labels, *disappear_time;
    float *boxes, *ref_pts, *logits, *scores, *output_embed, *long_memory, *last_output, *query_embed;
    int64_t *next_id;
    int32_t *counters;
    int32_t *free_list;
} clipops_bank;

/* The decoder's outputs for the B streams, each (B, n_det + cap, width) with a dense last axis: element (b, r, c) of
 * source i is ptr[i][b * batch_stride[i] + r * row_stride[i] + c].  det_embed (n_det, >= C) with its row stride is read
 * (and required) only when !use_dab. */
enum {
    CLIPOPS_BK_LOGITS = 0,   /* K   pred_logits */
    CLIPOPS_BK_BOXES,        /* 4   pred_bboxes, cxcywh */
    CLIPOPS_BK_OUTPUTS,      /* C   last decoder layer's output */
    CLIPOPS_BK_LAST_REF,     /* 4   last_ref_pts */
    CLIPOPS_BK_QUERIES,      /* C   the queries entering the last decoder layer */
    CLIPOPS_BK_N_MODEL
};
typedef struct {
    const float *ptr[CLIPOPS_BK_N_MODEL];
    long batch_stride[CLIPOPS_BK_N_MODEL];
    long row_stride[CLIPOPS_BK_N_MODEL];
    const float *det_embed;
    long det_row_stride;
} clipops_bank_model;

/* One frame of track management for every stream (reference models/runtime_tracker.py:36-101 and the inference branch
 * of models/query_updater.py:160-166), one workgroup per stream, sigmoid(x) = 1 / (1 + expf(-x)) in float32:
 *   live slot s (ids >= 0), from model row n_det + s:  boxes, logits, output_embed = the row;  scores = sigmoid(logits);
 *     own = scores[labels];  disappear_time = own < track_score_thresh ? disappear_time + 1 : 0 (a NaN does not age);
 *     disappear_time >= miss_tolerance: the slot is freed -- ids = -1 and every field of the row zero.
 *   detect row r < n_det is born when max_k sigmoid(logits[r,k]) >= det_score_thresh and no score of the row is NaN; its
 *     label is the lowest index of the maximum.  The j-th born row in row order takes the j-th slot in slot order that
 *     was free WHEN THE CALL BEGAN (a slot freed by this call is reused from the next call on):  ids = next_id + j;
 *     logits, boxes, output_embed = the row;  scores = sigmoid(logits);  ref_pts = last_ref row;  disappear_time = 0;
 *     last_output = output_embed;  long_memory = queries row;  query_embed = queries row (use_dab) or
 *     det_embed[r][:C] | queries row.
 *   next_id grows by the births placed; births beyond the free slots are not placed and are added to counters[b][1];
 *   counters[b][0] = live slots afterwards.
 * n_det and cap of any size (chunks of 1024).  No atomics: ranks come from ballots and prefix sums, the same inputs give
 * the same bits.  Calls on one bank are issued on one stream.  B == 0 launches nothing.  Returns 1 for a bad argument
 * (negative size or stride, cap < 1, K < 1, C < 1, null pointer), 3 when the launch failed. */
int clipops_bank_update_f32(const clipops_bank_model *model, const clipops_bank *bank, int B, int n_det, int cap, int K,
                            int C, int use_dab, float det_score_thresh, float track_score_thresh,
                            int64_t miss_tolerance, void *stream);

/* clipops_result_rows_f32 for every stream of a bank in one launch, into one table: the same filters, float32 roundings
 * and capacity rule; slot (b, s) is offered when ids[b][s] >= 0, streams in order, slots in order.  rows_i is
 * (capacity, 4): sequence, frame, id, label.  seq_frame int64 (B, 2) = (sequence, frame) and ori_wh float32 (B, 2) =
 * (ori_w, ori_h) of stream b are device arrays, so the launch is the same every frame.  B * cap == 0 launches nothing.
 * Returns 1 for a bad argument (negative size, K < 1, null pointer), 3 when the launch failed. */
int clipops_bank_result_rows_f32(const float *boxes, const float *scores, const int64_t *ids, const int64_t *labels,
                                 int B, int cap, int K, const int64_t *seq_frame, const float *ori_wh,
                                 float score_thresh, float area_thresh, float *rows_f, int64_t *rows_i,
                                 int32_t *counters, int capacity, void *stream);

/* ---- the bank entries with one threshold per stream: one sequence tracked under B settings at once ----
 * (Added without a new CLIPOPS_ABI_VERSION, like the bank entries: no entry point changed.)
 * clipops_bank_update_f32 / clipops_bank_result_rows_f32 with every threshold a device array of B values (float32;
 * miss_tolerance int64), stream b applying element b.  Stream b of a _streams call equals, bit for bit, stream b of the
 * scalar call made with that stream's values -- every bank field, next_id, counters, free_list, the rows and their order
 * in the table: the same kernels read the value from the array where the scalar entries take it from the argument, and
 * make the same float32 comparisons in the same order (>= for a birth, < for a miss, strict > in the result filter, a
 * NaN score as before).  In the update one workgroup is one stream and loads its three values once; the result rows
 * read the two values of slot / cap per slot.  The arrays are read on `stream`; no atomics.  Arguments are checked as
 * the scalar entries check theirs, then: returns 1 for a null threshold array.  B == 0 launches nothing. */
int clipops_bank_update_streams_f32(const clipops_bank_model *model, const clipops_bank *bank, int B, int n_det, int cap,
                                    int K, int C, int use_dab, const float *det_score_thresh,
                                    const float *track_score_thresh, const int64_t *miss_tolerance, void *stream);
int clipops_bank_result_rows_streams_f32(const float *boxes, const float *scores, const int64_t *ids,
                                         const int64_t *labels, int B, int cap, int K, const int64_t *seq_frame,
                                         const float *ori_wh, const float *score_thresh, const float *area_thresh,
                                         float *rows_f, int64_t *rows_i, int32_t *counters, int capacity, void *stream);

/* ---- the overlay's draw table, made on the device from the tracks where they live ----
 * (Added without a new CLIPOPS_ABI_VERSION, like the bank entries: no entry point changed.)
 * The int32 table trackdraw_draw_u8 draws from (include/track_draw_hip.h: 16 words a row), for every stream of a bank
 * in one launch, so that an annotated frame needs no result on the host.  boxes (B, cap, 4) cxcywh normalised, scores
 * (B, cap, K), ids int64 (B, cap) with -1 a free slot, ori_wh float32 (B, 2) = (ori_w, ori_h) on the device (integers
 * of at most 65535, which float32 carries exactly); table int32 (B, cap, 16).  One sequence's TrackInstances pass as
 * B = 1, cap = the number of tracks.
 *   kept    slot (b, s) is kept when ids >= 0 and it passes clipops_result_rows_f32's filters, the same float32
 *           operations, each rounded once, in the same order: s = max_k scores > score_thresh and
 *           ((w * ori_w) * h) * ori_h > area_thresh, both strict, a NaN failing either.  Ids are 0 .. 2^31 - 1: a slot
 *           with a larger id is NOT kept (the host statement, render.track_table, raises there; a kernel cannot).
 *   order   the kept slots of a stream fill the first rows of table[b] in ascending id order -- the one-sequence
 *           tracker's birth order, and the order a pixel's last covering primitive depends on.  Ids are unique within a
 *           stream; equal ids would keep their slot order.
 *   row     what render.track_table writes for that id and clipops_result_rows_f32's xyxy box: corners floor(v + 0.5)
 *           in float32 with NaN -> 0 and a clamp to +-2^24; the colour render.palette_entry(id % 64) from its integer
 *           formula (bytes swapped for bgr); the text colour by the integer luma rule; the glyph count and the packed
 *           decimal digits; the tab (6 n - 1) font_scale + 2 wide and 7 font_scale + 2 high above the box, inside it
 *           when it would leave the frame at the top, shifted left to end at column ori_w - 1 on the right.
 *   padding every other row of table[b] is 0, 0, -1, -1 and twelve zeros: x2 < x1 draws nothing, tab included, so
 *           trackdraw_draw_u8(..., table[b], n = cap, ...) is launched with a row count the host knows.
 * One workgroup per stream; the row of a kept slot is the number of kept slots of its stream with a smaller id, counted
 * by all-pairs compares over chunks of 1024 slots through LDS.  No atomics: the same inputs give the same bits.  cap of
 * any size.  B * cap == 0 launches nothing.  Arguments are checked on the host without touching a device: returns 1 for
 * a negative size, more than 2^31 - 1 slots, K < 1, font_scale outside 1 .. 64 or a null pointer with B * cap > 0; 3 when
 * the launch failed. */
int clipops_draw_table_f32(const float *boxes, const float *scores, const int64_t *ids, int B, int cap, int K,
                           const float *ori_wh, float score_thresh, float area_thresh, int bgr, int font_scale,
                           int32_t *table, void *stream);

/* ---- gap filling and short-track removal on a result table, where the rows live ----
 * (Added without a new CLIPOPS_ABI_VERSION, like the bank entries: no entry point changed.)
 * The offline pass over the rows of finished sequences that memotr_amd/postprocess.py states on the host (fill_gaps):
 * a track that was not reported for 1 .. max_gap frames and came back under its id gets the missing rows by linear
 * interpolation between the two rows around the hole, and a track with fewer than min_length rows is removed whole
 * (and fills nothing).  Input: a table as clipops_result_rows_f32 (W = 3: frame, id, label) or
 * clipops_bank_result_rows_f32 (W = 4: sequence, frame, id, label) leaves it -- rows_f (>= n, 5), rows_i (>= n, W), and
 * its device counters: the rows read are the first min(counters[0], n), so the host passes a bound it knows (the rows
 * offered) and the stored count never leaves the device.  Rows address a cell table [n_seq][n_ids][n_frames]; with
 * W = 3 every row is of sequence 0 and n_seq is 1.
 *   new row   for two rows of an id at frames f0 < f1 without a row between them and m = f1 - f0 - 1, 1 <= m <= max_gap:
 *             frame f0 + k for k = 1 .. m, the id and the label of the row at f0, and each of x1, y1, x2, y2, score as
 *             a + (b - a) * t,  t = float(k) / float(m + 1),  a and b the values at f0 and f1: a quotient, a difference,
 *             a product and a sum in float32, each rounded once, never fused.
 *   output    the rows of the surviving tracks bit-unchanged and the new rows, sorted by (sequence, frame, id), written
 *             behind row out_counters[0] as it was when the call began, by clipops_result_rows_f32's capacity rule:
 *             out_counters[0] grows by the rows stored, a row that would land at or past `capacity` is counted in
 *             out_counters[1], and nothing is written past out_f (capacity, 5) / out_i (capacity, W).
 *   status    a sticky word, OR-ed with CLIPOPS_FG_DUPLICATE when two rows share (sequence, frame, id), with
 *             CLIPOPS_FG_ID / _FRAME / _SEQUENCE when a row's id, frame or sequence lies outside 0 .. n_ids - 1,
 *             0 .. n_frames - 1, 0 .. n_seq - 1.  Such a row addresses no cell and is left out; of two rows in one
 *             cell one is left out.  The caller zeroes the word and must not use the output when it is not 0.
 *   workspace clipops_fill_gaps_workspace(n_seq, n_ids, n_frames) int32 words: two tables of n_seq * n_ids * n_frames
 *             cells and n_seq * n_frames offsets; -1 for a negative size, -2 when the cells exceed 2^31 - 1.  No device
 *             is touched.  Contents need no preparation and mean nothing afterwards.
 * Five launches on `stream`, nothing synchronises: clear the cells; each row writes its index into its cell (integer
 * compare-and-swap: the second writer sets the status bit); one workgroup per track finds, for every empty cell, the
 * nearest occupied frame on either side -- a suffix minimum and a prefix maximum by wavefront shuffles, chunks of 1024
 * frames carried through LDS -- counts the track's rows, marks the cells to fill or empties a short track; per
 * (sequence, frame) the surviving cells are counted and the counts scanned; one workgroup per (sequence, frame) ranks
 * its ids by ballots and writes the rows.  No float atomics: a table without duplicates gives the same bits every time.
 * n == 0 launches nothing.  Arguments are checked on the host without touching a device: returns 1 for a negative size,
 * max_gap or min_length, W not 3 or 4, W = 3 with n_seq > 1, or a null pointer with n > 0; 2 when the cells exceed
 * 2^31 - 1; 3 when a launch failed. */
#define CLIPOPS_FG_DUPLICATE 1
#define CLIPOPS_FG_ID 2
#define CLIPOPS_FG_FRAME 4
#define CLIPOPS_FG_SEQUENCE 8
long clipops_fill_gaps_workspace(int n_seq, int n_ids, int n_frames);
int clipops_fill_gaps_f32(const float *rows_f, const int64_t *rows_i, const int32_t *counters, int n, int W, int n_seq,
                          int n_ids, int n_frames, int max_gap, int min_length, int32_t *workspace, float *out_f,
                          int64_t *out_i, int32_t *out_counters, int32_t *status, int capacity, void *stream);

/* ---- error analysis: the match events of CLEAR, and the overlay's draw table coloured by event ----
 * (Added without a new CLIPOPS_ABI_VERSION, like the bank entries: no entry point changed.)
 * clipops_clear_events_f64 walks every sequence as CLEAR does (memotr_amd/evaluation.py: _clear_host; the same walk as
 * trackeval_clear of include/track_eval_hip.h, which keeps only the counts) and keeps the decision of every row.  It
 * works on the preprocessed, compacted arrays trackeval_clear is launched on, with the same meaning: sim float64, the
 * similarity of every frame row-major (ground truth x tracker) behind sim_off int64 [F + 1]; gt_off / tr_off int32
 * [F + 1]; gt_ids / tr_ids int32, relabelled 0 .. n - 1 per sequence; seq_off int32 [S + 1] in frames; n_gt_ids int32 [S];
 * max_gt / max_tr the largest frame, max_gt_ids the largest n_gt_ids, each at most CLIPOPS_EVENTS_MAX_DIM.
 *   frame     a frame without ground truth counts its tracker rows as false positives, one without tracker rows its
 *             ground truth as misses, and neither touches the per-id state.  Otherwise the assignment maximises
 *             1000 * [tracker id == the id's match in the previous evaluated frame] + similarity, entries with
 *             similarity < 0.5 - eps set to 0; pairs are scipy.optimize.linear_sum_assignment's (assign_core.h) and a
 *             pair counts when its similarity is at least 0.5 - eps.
 *   output    gt_partner int32 [NG']: the matched tracker row's index within its frame, -1 for a miss; gt_flags int32
 *             [NG']: bit 0 (CLIPOPS_EVENT_SWITCH) the id's last match ever was another tracker id, bit 1
 *             (CLIPOPS_EVENT_FRAG) the id was matched before but not in the previous evaluated frame; tr_partner int32
 *             [NT']: the matched ground-truth row's index within its frame, -1 for a false positive; counts int32
 *             [S, 5] = CLR_TP, CLR_FN, CLR_FP, IDSW, Frag; status int32 [S]: 0, -1 no feasible assignment, -2 a frame
 *             or an id count above what the launch was made for (the sequence's events are then all -1 / 0 and its
 *             counts 0).  Every entry of the five arrays is written; the caller zeroes nothing.
 * One wavefront per sequence; per ground-truth id the tracker id of its last match and the evaluated frame it happened
 * in live in LDS (dynamic, above 64 KiB by opt-in).  Integer results only: the same inputs give the same bits.
 * n_seqs == 0 launches nothing.  Arguments are checked on the host without touching a device: returns 1 for a negative
 * size or a null pointer with n_seqs > 0, 2 for a size above CLIPOPS_EVENTS_MAX_DIM, 3 when the launch failed. */
#define CLIPOPS_EVENTS_MAX_DIM 2048
#define CLIPOPS_EVENT_SWITCH 1
#define CLIPOPS_EVENT_FRAG 2
int clipops_clear_events_f64(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                             const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *seq_off, int n_seqs,
                             const int32_t *n_gt_ids, int max_gt, int max_tr, int max_gt_ids, int32_t *gt_partner,
                             int32_t *gt_flags, int32_t *tr_partner, int32_t *counts, int32_t *status, void *stream);

/* clipops_error_table_f64: the draw tables (include/track_draw_hip.h: 16 words a row) of all frames of a sequence in
 * one launch, from the rows as the files give them: gt_boxes / tr_boxes float64 (n, 4) xywh, gt_off / tr_off int32
 * [F + 1], gt_ids / tr_ids int32 (0 .. 2^31 - 1), gt_kind / tr_kind int32 the CLIPOPS_KIND_* of every row; table int32
 * (F, max_rows, 16).
 *   rows     of frame f: first its ground-truth rows of kind MISS in input order, labelled with the ground-truth id, then
 *            its tracker rows of kind MATCH, SWITCH and FP in input order, labelled with the tracker id.  Any other kind
 *            is not drawn.  A row that would land at or past max_rows is left out; every remaining row up to max_rows
 *            is clipops_draw_table_f32's padding row (0, 0, -1, -1 and twelve zeros).
 *   row      what render.track_table writes for that id and the box (x, y, x + w, y + h), each sum formed in float64
 *            and rounded once to float32, with `width` the frame's width -- except the colour (word 4): MATCH
 *            (0, 200, 0), FP (255, 0, 0), MISS (255, 200, 0), SWITCH (255, 0, 255) as r | g << 8 | b << 16, bytes 0 and
 *            2 swapped for bgr, and the text colour (word 9), which follows from it by the same luma rule.
 * One workgroup per frame, rows ranked by ballots.  n_frames * max_rows == 0 launches nothing.  Arguments are checked on
 * the host without touching a device: returns 1 for a negative size, width or height below 1 or above 65535, font_scale
 * outside 1 .. 64, more than 2^31 - 1 table rows or a null pointer; 3 when the launch failed. */
#define CLIPOPS_KIND_IGNORED 0
#define CLIPOPS_KIND_MATCH 1
#define CLIPOPS_KIND_SWITCH 2
#define CLIPOPS_KIND_MISS 3
#define CLIPOPS_KIND_FP 4
int clipops_error_table_f64(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_off, const int32_t *tr_off,
                            const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *gt_kind, const int32_t *tr_kind,
                            int n_frames, int max_rows, int width, int height, int bgr, int font_scale, int32_t *table,
                            void *stream);

/* ---- BDD100K error analysis: the cross-class pairs of a frame ----
 * (Added without a new CLIPOPS_ABI_VERSION, like the error-analysis entries: no entry point changed.)
 * BDD100K scores every class on its own, so a car labelled truck is a MISS of `car` and an FP of `truck`.
 * clipops_bdd_cross_class_f64 finds such boxes (memotr_amd/diagnose_bdd100k.py: _cross_host).  It reads the rows as
 * evaluation_bdd100k.PackedBDD gives them, frame-major: gt_boxes / tr_boxes float64 (n, 4) x0, y0, x1, y1; gt_classes /
 * tr_classes int32 TrackEval's class ids (include/track_eval_bdd_hip.h); gt_off / tr_off int32 [F + 1]; gt_kind / tr_kind
 * int32 the CLIPOPS_KIND_* of every row.
 *   frame     the candidates are the ground-truth rows of kind MISS and the tracker rows of kind FP whose class is one of
 *             the 8 evaluated, each side in input order.  score(i, j) is 0 for two rows of one class, else their IoU
 *             (bddeval_similarity's operation order: the same bits) with values < 0.5 - eps set to 0.  The pairs are
 *             scipy.optimize.linear_sum_assignment(-score)'s (assign_core.h); a pair counts when its score is > eps.
 *   output    per row of either side: partner int32 the paired row's index within its frame, -1; class int32 the paired
 *             row's class index 0 .. 7, -1; iou float64 the pair's IoU, 0.  status int32 [F]: 0, -1 no feasible
 *             assignment, -2 more candidates on a side than max_gt / max_tr (the frame's rows are then all -1 / -1 / 0).
 *             Every entry of the seven arrays is written.
 * One wavefront per frame; candidates and solver state in LDS (dynamic, above 64 KiB by opt-in).  max_gt / max_tr at most
 * CLIPOPS_EVENTS_MAX_DIM.  n_frames == 0 launches nothing.  Arguments are checked on the host without touching a device:
 * returns 1 for a negative size or a null pointer with n_frames > 0, 2 for a size above CLIPOPS_EVENTS_MAX_DIM, 3 when the
 * launch failed. */
int clipops_bdd_cross_class_f64(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_classes,
                                const int32_t *tr_classes, const int32_t *gt_off, const int32_t *tr_off,
                                const int32_t *gt_kind, const int32_t *tr_kind, int n_frames, int max_gt, int max_tr,
                                int32_t *gt_partner, int32_t *gt_class, double *gt_iou, int32_t *tr_partner,
                                int32_t *tr_class, double *tr_iou, int32_t *status, void *stream);

/* ---- association analysis: HOTA's and Identity's matches kept, reduced per identity, drawn as a timeline ----
 * (Added without a new CLIPOPS_ABI_VERSION, like the error-analysis entries: no entry point changed.)
 * The four entries work on the preprocessed, compacted arrays and the per-sequence tables of include/track_eval_hip.h
 * (trackeval_accumulate's outputs: alignment float64 and id_matches int32 behind cell_off int64 [S + 1], gt_count /
 * tr_count int32 behind gid_off / tid_off int32 [S + 1]; n_gt_ids / n_tr_ids int32 [S] = G, K of a sequence).  All of
 * them check their arguments on the host without touching a device: 1 for a negative size, an index out of range or a
 * null pointer, 2 for a size above its limit, 3 when the launch failed.
 *
 * clipops_hota_events_f64: one wavefront per frame (frame_seq int32 [F]: the frame's sequence) solves
 * linear_sum_assignment(-(alignment[gt id, tracker id] * sim)) as trackeval_hota_match does (assign_core.h) and keeps the
 * pairs.  `level` of a pair is the number of thresholds a with sim >= alphas[a] - eps (alphas: CLIPOPS_ASSOC_ALPHAS
 * ascending float64 in host memory, read during the call), so the pair is a true positive at threshold a exactly when
 * a < level.  gt_partner / tr_partner int32 [NG'] / [NT']: the partner row's index within its frame, -1; gt_level /
 * tr_level int32: the pair's level, 0.  A pair of level 0 is reported as no pair.  status int32 [F]: 0, -1 no feasible
 * assignment, -2 a frame above max_gt / max_tr (the frame's rows are then all -1 / 0).  Every entry of the five arrays is
 * written.  matches int32 [19 * cells], or null: behind 19 * cell_off[s], [a][gt id][tracker id] is incremented for every
 * pair and every a < level -- trackeval_hota_match's table; the caller zeroes it.  max_gt / max_tr at most
 * CLIPOPS_EVENTS_MAX_DIM.  n_frames == 0 launches nothing. */
#define CLIPOPS_ASSOC_ALPHAS 19
int clipops_hota_events_f64(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                            const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *frame_seq, int n_frames,
                            const int32_t *n_tr_ids, const int64_t *cell_off, const double *alignment,
                            const double *alphas, int max_gt, int max_tr, int32_t *gt_partner, int32_t *gt_level,
                            int32_t *tr_partner, int32_t *tr_level, int32_t *matches, int32_t *status, void *stream);

/* clipops_identity_pairs_i32: one wavefront per sequence solves the Identity metric's (G + K) x (G + K) problem
 * (memotr_amd/evaluation.py: _identity_host; the cost is a function of gt_count, tr_count and id_matches, never a
 * matrix) as trackeval_identity does and keeps the map: gt_id_partner int32 [sum G] the tracker id a ground-truth id is
 * credited to, -1; gt_idtp int32 its id_matches entry, 0; tr_id_partner / tr_idtp int32 [sum K] the same pairs read from
 * the tracker side.  status int32 [S]: 0, -1, -2 for G + K above max_ids (at most CLIPOPS_EVENTS_MAX_DIM); the
 * sequence's ids are then all -1 / 0.  Every entry is written.  n_seqs == 0 launches nothing. */
int clipops_identity_pairs_i32(int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                               const int32_t *gid_off, const int32_t *tid_off, const int32_t *gt_count,
                               const int32_t *tr_count, const int32_t *id_matches, int max_ids, int32_t *gt_id_partner,
                               int32_t *gt_idtp, int32_t *tr_id_partner, int32_t *tr_idtp, int32_t *status,
                               void *stream);

/* clipops_assoc_reduce_f64: HOTA's association sums per identity, one wavefront per (id, sequence, side), from
 * matches (m = matches[a][g][k]), gt_count (gc) and tr_count (tc).  For a ground-truth id g: gt_tp int32 [sum G, 19] =
 * sum_k m; gt_num float64 [sum G, 2, 19] = sum_k m * (m / max(1, gc[g] + tc[k] - m)) and sum_k m * (m / max(1, gc[g]));
 * gt_top int32 [sum G, 3] at threshold alpha_index: the number of k with m > 0, the k of the largest m (ties: the lowest
 * k; -1 without any) and that m.  For a tracker id k the mirror image over g, with max(1, tc[k]) in the second sum.
 * Every product and quotient is rounded once (no contraction); a lane adds its terms in ascending id order and the 64
 * partial sums meet in a fixed xor tree, so the same inputs give the same bits.  max_side_ids: the largest G or K, at most
 * CLIPOPS_EVENTS_MAX_DIM; at most 65535 sequences.  Every entry is written.  n_seqs * max_side_ids == 0 launches nothing. */
int clipops_assoc_reduce_f64(int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                             const int32_t *gid_off, const int32_t *tid_off, const int32_t *gt_count,
                             const int32_t *tr_count, const int32_t *matches, int max_side_ids, int alpha_index,
                             int32_t *gt_tp, double *gt_num, int32_t *gt_top, int32_t *tr_tp, double *tr_num,
                             int32_t *tr_top, void *stream);

/* clipops_timeline_u8: the identity timeline of one sequence, image uint8 (n_ids * cell_h, n_frames * cell_w, 3): one row
 * of cells per ground-truth identity, one column per frame.  gt_off int32 [F + 1] the kept ground-truth rows of every
 * frame; per row gt_ids int32 (0 .. n_ids - 1, unique within a frame), partner_id int32 (the partner's tracker id as the
 * files name it, -1) and level int32.  Cell (g, f) is (0, 0, 0) when g has no row in frame f, (96, 96, 96) when its row
 * has level <= alpha_index, else render.PALETTE[partner_id % 64], bytes 0 and 2 swapped for bgr.  One workgroup per
 * frame; integers only; every byte of the image is written.  Returns 2 when a side of the image exceeds 65535 pixels.
 * n_ids * n_frames == 0 launches nothing. */
int clipops_timeline_u8(const int32_t *gt_off, const int32_t *gt_ids, const int32_t *partner_id, const int32_t *level,
                        int n_ids, int n_frames, int alpha_index, int cell_w, int cell_h, int bgr, uint8_t *image,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIP_OPS_HIP_H */
