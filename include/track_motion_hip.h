/* track_motion_hip.h -- C ABI of libtrack_motion_hip.so: the motion post-process of the online tracker (the
 * reference's USE_MOTION: models/motion.py, models/runtime_tracker.py:43-54,81-94, submit_engine.py:78-87) as three
 * small gfx950 kernels on a device-resident table keyed by track id.  The definition, stated once more on the host:
 * memotr_amd/models/motion.py (MotionState); the cut of the work: DESIGN.md, "Motion post-process".
 *
 * THE TABLE: ids are dense (the tracker hands them out from 0 upward), so the history of track `id` is row `id`.
 *   table_boxes  float32 [capacity, L, 4]  the last count[id] boxes (cx, cy, w, h) the track was seen with, oldest
 *                                          first; entries at and past count[id] are stale and never read
 *   table_count  int32   [capacity]        0 .. L
 *   status       int32   [1]               sticky bits, set with an atomic OR and never read by these calls:
 *                                          TRACKMOTION_STATUS_NEGATIVE_ID / _ID_PAST_CAPACITY / _BAD_LABEL
 * PER-ROW STATE of one call, n rows as TrackInstances holds them: ids, labels, disappear_time int64 [n]; boxes,
 * last_appear_boxes, ref_pts float32 [n, 4]; scores float32 [n, K] (sigmoid of the logits, as torch computed them).
 *
 * Layout of a launch: four adjacent lanes per row, one per box coordinate, 256-thread blocks.  A table row is touched
 * only by the lanes of its id, so there are no float atomics and the same inputs give the same bits.  PRECONDITIONS:
 * ids are unique within a call; calls on one table are issued on one stream; input and output arrays do not overlap.
 * float32 arithmetic with contraction off (the build passes -ffp-contract=off): add, mul and div are the host's bits.
 *
 * All pointers are device pointers; nothing is kept between calls except the text of the calling thread's last error.
 * Returns 0 or a non-zero code (trackmotion_last_error() has the text): 1 = bad argument (negative size, L outside
 * 2 .. TRACKMOTION_MAX_LENGTH, min_length < 2, K < 1, null pointer with n > 0, rows outside the table), 2 = a size
 * the 32-bit indexing does not cover, 3 = the launch failed.  Arguments are validated on the host without touching a
 * device; n == 0 is a successful no-op without a launch.  Launches on `stream` (hipStream_t as void*; NULL = default
 * stream) and does not synchronise.
 */
#ifndef TRACK_MOTION_HIP_H
#define TRACK_MOTION_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRACKMOTION_ABI_VERSION 1
#define TRACKMOTION_MAX_LENGTH 16               /* largest L (boxes kept per track) */
#define TRACKMOTION_STATUS_NEGATIVE_ID 1
#define TRACKMOTION_STATUS_ID_PAST_CAPACITY 2
#define TRACKMOTION_STATUS_BAD_LABEL 4

int trackmotion_abi_version(void);
const char *trackmotion_last_error(void);

/* The existing-track loop of runtime_tracker.py:43-54.  Per row i, own = scores[i, labels[i]]:
 *   own < track_score_thresh (strict, float32):  disappear_time_out = disappear_time + 1, history untouched;
 *   otherwise: the history of ids[i] is cleared when disappear_time > 0, boxes[i] is appended (the last L are kept),
 *              disappear_time_out = 0 and last_appear_boxes_out[i] = boxes[i];
 *   then disappear_time_out >= miss_tolerance gives ids_out[i] = -1 (the history row is the id's before that).
 * A row with ids[i] < 0 or >= capacity touches no table row: ids and last_appear_boxes are copied, disappear_time
 * still follows the score rule, a status bit is set.  A row whose label is outside 0 .. K - 1 is copied as it is
 * (status bit). */
int trackmotion_observe(const float *scores, const int64_t *labels, const float *boxes, const int64_t *ids,
                        const int64_t *disappear_time, const float *last_appear_boxes, int n, int K,
                        float track_score_thresh, int64_t miss_tolerance, float *table_boxes, int32_t *table_count,
                        int capacity, int L, int64_t *ids_out, int64_t *disappear_time_out,
                        float *last_appear_boxes_out, int32_t *status, void *stream);

/* Newborn tracks first_id .. first_id + n - 1 (inside the table: error 1 otherwise): count = 1 and
 * table_boxes[id, 0] = new_boxes[id - first_id]. */
int trackmotion_register(const float *new_boxes, int n, int64_t first_id, float *table_boxes, int32_t *table_count,
                         int capacity, int L, void *stream);

/* submit_engine.py:78-87, out of place.  A row is changed when disappear_time > 0, its id is inside the table and
 * count[id] >= min_length; then, b being the id's history,
 *   delta          = motion_lambda * (float((double)disappear_time / (double)(count - 1)) * sum_k (b[k + 1] - b[k]))
 *   ref_pts_out[i] = inverse_sigmoid(last_appear_boxes[i]) + delta        (eps 1e-5: log(clamp(x) / clamp(1 - x)))
 * with the sum taken in float32 from zero, oldest pair first.  Every other row: ref_pts_out[i] = ref_pts[i].
 * delta_out (float32 [n, 4], may be NULL): delta of the changed rows, 0 elsewhere. */
int trackmotion_extrapolate(const int64_t *ids, const int64_t *disappear_time, const float *last_appear_boxes,
                            const float *ref_pts, int n, float motion_lambda, int min_length,
                            const float *table_boxes, const int32_t *table_count, int capacity, int L,
                            float *ref_pts_out, float *delta_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRACK_MOTION_HIP_H */
