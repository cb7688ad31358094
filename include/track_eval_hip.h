/* track_eval_hip.h -- C ABI of libtrack_eval_hip.so: multi-object-tracking evaluation (HOTA, CLEAR, Identity with the
 * definitions of TrackEval's metrics/{hota,clear,identity}.py and the MOT-challenge preprocessing of
 * datasets/mot_challenge_2d_box.py) for one class, as gfx950 kernels.  The definition, stated once more on the host:
 * memotr_amd/evaluation.py; the cut of the work: DESIGN.md, "Evaluation".
 *
 * PACKED INPUT of one call: S sequences, F frames in all, frames of a sequence consecutive.
 *   seq_off  int32 [S + 1]  frames seq_off[s] .. seq_off[s + 1] - 1 belong to sequence s
 *   gt_off   int32 [F + 1]  ground-truth detections gt_off[f] .. gt_off[f + 1] - 1 belong to frame f; tr_off likewise
 *   boxes    float64 [N, 4] x, y, w, h
 *   sim_off  int64 [F + 1]  the similarity of frame f is a row-major (g_f x k_f) matrix at sim + sim_off[f]
 *                           (g_f = gt_off[f + 1] - gt_off[f], k_f likewise; sim_off[f + 1] = sim_off[f] + g_f * k_f)
 * After preprocessing ids are contiguous per sequence (0 .. G_s - 1 ground truth, 0 .. K_s - 1 tracker; unique within
 * a frame) and every sequence owns
 *   n_gt_ids, n_tr_ids  int32 [S]      G_s, K_s
 *   cell_off            int64 [S + 1]  its G_s x K_s tables start at cell_off[s] (cell_off[s + 1] - cell_off[s] = G_s K_s)
 *   gid_off, tid_off    int32 [S + 1]  its per-id tables start there
 *
 * All arithmetic is float64 with contraction off; the assignments are assign_core.h, scipy's pairs, one 64-lane
 * wavefront per problem.  No call uses a float atomic: every float sum has a fixed order, results are bit-reproducible.
 *
 * All pointers are device pointers unless marked HOST; nothing is kept between calls except the text of the calling
 * thread's last error.  Returns 0 or a non-zero code (trackeval_last_error() has the text); launches on `stream`
 * (hipStream_t as void*; NULL = default stream) and does not synchronise.  Arguments are validated on the host without
 * touching a device.  `max_gt` / `max_tr` (largest g_f / k_f of the call) and `max_ids` (largest G_s + K_s) size the
 * LDS of a launch; each is capped at TRACKEVAL_MAX_DIM (error 2), and a frame or sequence that exceeds the value
 * passed is not evaluated: its `status` entry is -2 (the caller raises).  status 0 = ok, -1 = infeasible assignment.
 * LDS of a launch: an assignment takes 21 bytes per entry of its shorter side and 29 per entry of its longer one
 * (pairs + assign::work_bytes), 102,400 bytes at 2048 x 2048; trackeval_clear keeps 24 bytes per ground-truth id of the
 * sequence beside it, 151,552 bytes with 2048 ids.  So every problem within TRACKEVAL_MAX_DIM fits the 163,840 bytes
 * of a gfx950 CU; the "does not fit the LDS of a CU" error (2) guards the arithmetic and is not reachable below the cap.
 */
#ifndef TRACK_EVAL_HIP_H
#define TRACK_EVAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRACKEVAL_ABI_VERSION 1
#define TRACKEVAL_MAX_DIM 2048      /* largest side of one assignment problem (CLIPOPS_ASSIGN_MAX_DIM) */
#define TRACKEVAL_N_ALPHA 19        /* HOTA's localisation thresholds */
#define TRACKEVAL_CLEAR_INTS 8      /* CLR_TP, CLR_FN, CLR_FP, IDSW, MT, PT, ML, Frag */

int trackeval_abi_version(void);
const char *trackeval_last_error(void);

/* sim[sim_off[f] + i * k_f + j] = IoU of ground-truth box i and tracker box j of frame f, in the operation order of
 * TrackEval's _calculate_box_ious(box_format='xywh').  One workgroup per frame. */
int trackeval_similarity(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_off, const int32_t *tr_off,
                         const int64_t *sim_off, int n_frames, double *sim, void *stream);

/* MOT-challenge preprocessing, the matching step: per frame one assignment on the similarity with entries below
 * 0.5 - eps set to 0; tr_remove[tr_off[f] + j] = 1 where tracker detection j is matched (score > eps) to a ground
 * truth of a distractor class (2, 7, 8, 12).  tr_remove (int32 [NT]) must be zeroed by the caller; status int32 [F]. */
int trackeval_preproc_match(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                            const int32_t *gt_classes, int n_frames, int max_gt, int max_tr, int32_t *tr_remove,
                            int32_t *status, void *stream);

/* HOTA pass 1 and Identity's counts.  One workgroup per sequence walks its frames in order (the sums of a table cell
 * are formed in frame order, as the definition's loop does).  Writes, per sequence:
 *   potential float64 [cells]  sum over frames of sim / (rowsum + colsum - sim) at (gt id, tracker id)
 *   id_matches int32 [cells]   number of frames with sim >= 0.5 at (gt id, tracker id)
 *   gt_count, tr_count int32   detections per id
 *   alignment float64 [cells]  potential / (gt_count + tr_count - potential)
 * All outputs are written in full (no zeroing needed). */
int trackeval_accumulate(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                         const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *seq_off, int n_seqs,
                         const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                         const int32_t *gid_off, const int32_t *tid_off, int max_gt, int max_tr,
                         double *potential, int32_t *id_matches, int32_t *gt_count, int32_t *tr_count,
                         double *alignment, void *stream);

/* HOTA pass 2, one wavefront per frame: assignment on -(alignment[gt id, tracker id] * sim), then per threshold a
 *   tp int32 [F, 19]            matched pairs with sim >= alpha_a - eps
 *   loc float64 [F, 19]         sum of their sim, in pair order
 *   matches int32 [19 * cells]  (integer atomics) at 19 * cell_off[s] + a * G_s K_s + gid * K_s + tid; zeroed by caller
 * frame_seq int32 [F]: the sequence of each frame.  alphas: HOST pointer to 19 doubles. */
int trackeval_hota_match(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                         const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *frame_seq, int n_frames,
                         const int32_t *n_tr_ids, const int64_t *cell_off, const double *alignment,
                         const double *alphas, int max_gt, int max_tr, int32_t *matches, int32_t *tp, double *loc,
                         int32_t *status, void *stream);

/* HOTA reduction, one wavefront per (threshold, sequence), fixed order:
 *   out_tp int64 [S, 19]       sum of tp over the sequence's frames
 *   out_sums float64 [S, 4, 19] sum over cells of m * m / max(1, gc + tc - m), m * m / max(1, gc), m * m / max(1, tc)
 *                              (m = matches), and the sum of loc over frames */
int trackeval_hota_reduce(const int32_t *seq_off, int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids,
                          const int64_t *cell_off, const int32_t *gid_off, const int32_t *tid_off,
                          const int32_t *gt_count, const int32_t *tr_count, const int32_t *matches, const int32_t *tp,
                          const double *loc, int64_t *out_tp, double *out_sums, void *stream);

/* CLEAR, one wavefront per sequence walking its frames (the match of a frame depends on the previous frame's); the
 * per-id state lives in LDS.  Per frame an assignment on -(1000 * [tracker id == id matched in the previous frame]
 * + sim), entries with sim < 0.5 - eps set to 0.  out_ints int32 [S, 8] (TRACKEVAL_CLEAR_INTS order), motp_sum
 * float64 [S], status int32 [S].  max_gt_ids: largest G_s. */
int trackeval_clear(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                    const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *seq_off, int n_seqs,
                    const int32_t *n_gt_ids, int max_gt, int max_tr, int max_gt_ids, int32_t *out_ints,
                    double *motp_sum, int32_t *status, void *stream);

/* Identity, one wavefront per sequence: the (G + K) x (G + K) assignment whose cost is fn + fp of identity.py as a
 * function of the counts (never a matrix in memory).  out int64 [S, 2]: IDFN and IDFP, each summed over the pairs
 * found.  status int32 [S].  max_ids: largest G_s + K_s. */
int trackeval_identity(int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                       const int32_t *gid_off, const int32_t *tid_off, const int32_t *gt_count,
                       const int32_t *tr_count, const int32_t *id_matches, int max_ids, int64_t *out, int32_t *status,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRACK_EVAL_HIP_H */
