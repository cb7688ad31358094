/* track_eval_bdd_hip.h -- C ABI of libtrack_eval_bdd_hip.so: what BDD100K's evaluation needs in front of the metric
 * kernels of libtrack_eval_hip.so (include/track_eval_hip.h): the cut of every frame into its 8 evaluated classes, box
 * IoU on corner boxes, and the preprocessing of TrackEval's datasets/bdd100k.py (unmatched detections inside
 * crowd-ignore regions are dropped), as gfx950 kernels.  The definition, stated once more on the host:
 * memotr_amd/evaluation_bdd100k.py; the cut of the work: DESIGN.md, "Evaluation".
 *
 * PACKED INPUT of one call: S sequences, F frames in all, frames of a sequence consecutive (frame-major).
 *   seq_off    int32 [S + 1]  frames seq_off[s] .. seq_off[s + 1] - 1 belong to sequence s (T_s of them)
 *   frame_seq  int32 [F]      the sequence of each frame
 *   gt_off     int32 [F + 1]  ground-truth rows gt_off[f] .. gt_off[f + 1] - 1 belong to frame f; tr_off, ig_off likewise
 *   boxes      float64 [N, 4] x0, y0, x1, y1 (ground truth, tracker detections, ignore regions)
 *   classes    int32 [N]      TrackEval's class id of each ground-truth / tracker row: 1 pedestrian, 2 rider, 4 car,
 *                             5 bus, 6 truck, 7 train, 10 motorcycle, 11 bicycle are evaluated (class index c = 0 .. 7
 *                             in that order); a row of any other id belongs to no problem
 * PROBLEM-MAJOR LAYOUT, what the class split produces and every later call reads: a problem is a (sequence, class)
 * pair, p = s * 8 + c; its T_s frames are consecutive, so frame t of sequence s and class c is the split frame
 *   q = 8 * seq_off[s] + c * T_s + t                                    (F * 8 split frames in all)
 *   split gt_off / tr_off  int32 [8 F + 1]  rows of split frame q, in the order they had in the packed frame (stable)
 *   sim_off                int64 [8 F + 1]  as in track_eval_hip.h: a row-major (g_q x k_q) matrix per split frame
 *   frame_src              int32 [8 F]      the packed frame a split frame was cut from (its ignore regions)
 * With seq_off' = (8 * seq_off[s] + c * T_s) the split arrays are the "S * 8 sequences" the trackeval_* calls take.
 *
 * Conventions are those of track_eval_hip.h: float64 with contraction off, no float atomics, fixed orders, the same
 * bits on every run; the assignment is assign_core.h (scipy's pairs), one 64-lane wavefront per problem.  All pointers
 * are device pointers; nothing is kept between calls except the text of the calling thread's last error.  Returns 0
 * or a non-zero code (bddeval_last_error() has the text); launches on `stream` (hipStream_t as void*; NULL = default
 * stream) and does not synchronise.  Arguments are validated on the host without touching a device.  `max_gt` /
 * `max_tr` (largest g_q / k_q of the call) size the LDS of a launch; each is capped at BDDEVAL_MAX_DIM (error 2), and
 * a split frame that exceeds the value passed is not evaluated: its `status` entry is -2.  status 0 = ok,
 * -1 = infeasible assignment.
 */
#ifndef TRACK_EVAL_BDD_HIP_H
#define TRACK_EVAL_BDD_HIP_H

#include <stdint.h>

#include "track_eval_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDDEVAL_ABI_VERSION 1
#define BDDEVAL_N_CLASSES 8
#define BDDEVAL_MAX_DIM TRACKEVAL_MAX_DIM       /* largest side of one assignment problem */

int bddeval_abi_version(void);
const char *bddeval_last_error(void);

/* Class split, step 1: gt_count[q] / tr_count[q] (int32 [8 F] each) = rows of class c in packed frame f, for every
 * split frame q of (f, c).  One wavefront per (frame, side).  The caller forms the exclusive running sums (the split
 * gt_off / tr_off) from them. */
int bddeval_class_count(const int32_t *gt_classes, const int32_t *tr_classes, const int32_t *gt_off,
                        const int32_t *tr_off, const int32_t *seq_off, const int32_t *frame_seq, int n_frames,
                        int32_t *gt_count, int32_t *tr_count, void *stream);

/* Class split, step 2: the stable scatter.  Row i of packed frame f with class index c goes to
 * split_off[q] + (number of rows of class c before i in the frame): boxes and ids of both sides.  One wavefront per
 * (frame, side) walks the frame 64 rows at a time; a row's rank is the ballot's prefix count plus the running base. */
int bddeval_class_split(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_ids, const int32_t *tr_ids,
                        const int32_t *gt_classes, const int32_t *tr_classes, const int32_t *gt_off,
                        const int32_t *tr_off, const int32_t *seq_off, const int32_t *frame_seq, int n_frames,
                        const int32_t *split_gt_off, const int32_t *split_tr_off, double *out_gt_boxes,
                        double *out_tr_boxes, int32_t *out_gt_ids, int32_t *out_tr_ids, void *stream);

/* sim[sim_off[q] + i * k_q + j] = IoU of ground-truth box i and tracker box j of split frame q, in the operation order
 * of TrackEval's _calculate_box_ious(box_format='x0y0x1y1'): areas (x1 - x0) * (y1 - y0) from the corners as they are.
 * One workgroup per split frame ((frame, class)); n_frames counts split frames. */
int bddeval_similarity(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_off, const int32_t *tr_off,
                       const int64_t *sim_off, int n_frames, double *sim, void *stream);

/* BDD100K's preprocessing, one wavefront per split frame: one assignment on the similarity with entries below
 * 0.5 - eps set to 0; a detection is matched where its pair's score is > eps.  Every UNMATCHED detection (all of them
 * where the split frame has no ground truth) walks the ignore regions ig_off[f] .. ig_off[f + 1] - 1 of its packed
 * frame f = frame_src[q]: tr_remove[tr_off[q] + j] = 1 where intersection / (area of the detection) > 0.5 + eps for
 * any region (a detection with area <= eps stays).  tr_remove (int32, one per split tracker row) must be zeroed by
 * the caller; status int32 [n_frames]; n_frames counts split frames. */
int bddeval_preproc(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                    const double *tr_boxes, const int32_t *ig_off, const double *ig_boxes, const int32_t *frame_src,
                    int n_frames, int max_gt, int max_tr, int32_t *tr_remove, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRACK_EVAL_BDD_HIP_H */
