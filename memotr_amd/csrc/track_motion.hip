// track_motion.hip -- the motion post-process of the online tracker (the reference's USE_MOTION) on a device-resident
// table keyed by track id (C ABI, table layout and preconditions: include/track_motion_hip.h; the same definition on
// the host: memotr_amd/models/motion.py; why it is cut this way: DESIGN.md, "Motion post-process").
//
//   observe_kernel       the existing-track loop of runtime_tracker.py:43-54: age or refresh every track, push the box
//                        of a seen track into its history (cleared first after a miss), retire at miss_tolerance
//   register_kernel      newborn ids: count = 1, first box
//   extrapolate_kernel   submit_engine.py:78-87: a missed track's reference point moves along its mean box velocity
// Every kernel gives a row four adjacent lanes, one per box coordinate (a 256-thread block holds 64 rows; the four
// lanes of a row share a wavefront).  Lane 0 of a row is the only one that touches the row's count: it reads it once
// and the other three get it by a shuffle, so nothing is read that another lane of the launch writes.  A few hundred
// rows at most: the cost of a call is its launch, and the kernels are kept plain.  float32, contraction off.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/track_motion_hip.h"

namespace {

thread_local char g_err[256] = {0};      // text of this thread's last error; read by trackmotion_last_error() only

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

constexpr int BLOCK = 256;
constexpr int MAX_ROWS = INT32_MAX / 4;          // 4 n threads, 4 n floats: int indices throughout
constexpr float INV_SIGMOID_EPS = 1e-5f;         // utils.inverse_sigmoid's eps, as torch's clamp casts it

// torch.clamp(x, lo, hi): NaN goes through
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ float inverse_sigmoid(float x) {
    const float x1 = clampf(x, INV_SIGMOID_EPS, 1.0f);
    const float x2 = clampf(1.0f - x, INV_SIGMOID_EPS, 1.0f);
    return logf(x1 / x2);
}

// what lane 0 of this row's four lanes holds (every lane of the wavefront calls it)
__device__ __forceinline__ int from_row_lane0(int v) { return __shfl(v, 0, 4); }

__global__ __launch_bounds__(BLOCK) void observe_kernel(
        const float *__restrict__ scores, const int64_t *__restrict__ labels, const float *__restrict__ boxes,
        const int64_t *__restrict__ ids, const int64_t *__restrict__ disappear_time,
        const float *__restrict__ last_appear_boxes, int n, int K, float thresh, int64_t miss_tolerance,
        float *__restrict__ table_boxes, int32_t *__restrict__ table_count, int capacity, int L,
        int64_t *__restrict__ ids_out, int64_t *__restrict__ disappear_time_out,
        float *__restrict__ last_appear_boxes_out, int32_t *__restrict__ status) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int i = t >> 2, c = t & 3;
    const bool live = i < n;                                  // (no early return: the shuffle below wants every lane)
    const int64_t id = live ? ids[i] : -1;
    const int64_t label = live ? labels[i] : 0;
    const int64_t dt = live ? disappear_time[i] : 0;
    const bool label_ok = label >= 0 && label < K;
    const bool in_table = id >= 0 && id < capacity;
    int count = 0;
    if (live && label_ok && in_table && c == 0) count = table_count[id];
    count = from_row_lane0(count);
    if (!live) return;
    const float lab = last_appear_boxes[(size_t)i * 4 + c];
    if (!label_ok) {                                          // no score to judge the row by: it stays as it is
        if (c == 0) {
            atomicOr(status, TRACKMOTION_STATUS_BAD_LABEL);
            ids_out[i] = id;
            disappear_time_out[i] = dt;
        }
        last_appear_boxes_out[(size_t)i * 4 + c] = lab;
        return;
    }
    const float own = scores[(size_t)i * K + label];
    const bool missed = own < thresh;                         // (NaN: not missed, as the reference's `if`)
    const int64_t dt_new = missed ? dt + 1 : 0;
    if (!in_table) {
        if (c == 0) {
            atomicOr(status, id < 0 ? TRACKMOTION_STATUS_NEGATIVE_ID : TRACKMOTION_STATUS_ID_PAST_CAPACITY);
            ids_out[i] = id;
            disappear_time_out[i] = dt_new;
        }
        last_appear_boxes_out[(size_t)i * 4 + c] = lab;
        return;
    }
    float out_lab = lab;
    if (!missed) {
        const float b = boxes[(size_t)i * 4 + c];
        float *row = table_boxes + (size_t)id * L * 4 + c;    // this lane's coordinate of the id's history
        if (dt > 0) count = 0;                                // seen again after a miss: the history starts over
        count = count < 0 ? 0 : (count > L ? L : count);      // (a table nobody else wrote holds 0 .. L)
        if (count == L) {                                     // full: drop the oldest
            for (int k = 0; k + 1 < L; ++k) row[(size_t)k * 4] = row[(size_t)(k + 1) * 4];
            count = L - 1;
        }
        row[(size_t)count * 4] = b;
        if (c == 0) table_count[id] = count + 1;
        out_lab = b;
    }
    last_appear_boxes_out[(size_t)i * 4 + c] = out_lab;
    if (c == 0) {
        disappear_time_out[i] = dt_new;
        ids_out[i] = dt_new >= miss_tolerance ? -1 : id;
    }
}

__global__ __launch_bounds__(BLOCK) void register_kernel(const float *__restrict__ new_boxes, int n, int64_t first_id,
                                                          float *__restrict__ table_boxes,
                                                          int32_t *__restrict__ table_count, int L) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int j = t >> 2, c = t & 3;
    if (j >= n) return;
    const size_t id = (size_t)first_id + j;                   // (inside the table: checked on the host)
    table_boxes[id * L * 4 + c] = new_boxes[(size_t)j * 4 + c];
    if (c == 0) table_count[id] = 1;
}

__global__ __launch_bounds__(BLOCK) void extrapolate_kernel(
        const int64_t *__restrict__ ids, const int64_t *__restrict__ disappear_time,
        const float *__restrict__ last_appear_boxes, const float *__restrict__ ref_pts, int n, float motion_lambda,
        int min_length, const float *__restrict__ table_boxes, const int32_t *__restrict__ table_count, int capacity,
        int L, float *__restrict__ ref_pts_out, float *__restrict__ delta_out) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int i = t >> 2, c = t & 3;
    if (i >= n) return;
    const int64_t id = ids[i], dt = disappear_time[i];
    const size_t at = (size_t)i * 4 + c;
    float out = ref_pts[at], delta = 0.0f;
    if (dt > 0 && id >= 0 && id < capacity) {
        int count = table_count[id];                          // (read-only in this launch: every lane may read it)
        count = count > L ? L : count;
        if (count >= min_length) {                            // min_length >= 2: count - 1 >= 1
            const float *row = table_boxes + (size_t)id * L * 4 + c;
            float sum = 0.0f;                                 // Motion.get_box_delta: sequential, not telescoped
            for (int k = 0; k + 1 < count; ++k) sum = sum + (row[(size_t)(k + 1) * 4] - row[(size_t)k * 4]);
            const float factor = (float)((double)dt / (double)(count - 1));
            delta = motion_lambda * (factor * sum);
            out = inverse_sigmoid(last_appear_boxes[at]) + delta;
        }
    }
    ref_pts_out[at] = out;
    if (delta_out) delta_out[at] = delta;
}

// ------------------------------------------------------------------------------------------------------ host side
int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return 3;
    }
    g_err[0] = 0;
    return 0;
}

int check_rows(int n, const char *who) {
    char msg[200];
    if (n < 0) {
        snprintf(msg, sizeof(msg), "%s: negative row count %d", who, n);
        return fail(1, msg);
    }
    if (n > MAX_ROWS) {
        snprintf(msg, sizeof(msg), "%s: %d rows exceed the %d the 32-bit indexing covers", who, n, MAX_ROWS);
        return fail(2, msg);
    }
    return 0;
}

int check_table(int capacity, int L, const char *who) {
    char msg[200];
    if (capacity < 0) {
        snprintf(msg, sizeof(msg), "%s: negative capacity %d", who, capacity);
        return fail(1, msg);
    }
    if (L < 2 || L > TRACKMOTION_MAX_LENGTH) {
        snprintf(msg, sizeof(msg), "%s: L = %d is outside 2 .. %d", who, L, TRACKMOTION_MAX_LENGTH);
        return fail(1, msg);
    }
    return 0;
}

inline int blocks_for(int n) { return (int)(((int64_t)n * 4 + BLOCK - 1) / BLOCK); }

}  // namespace

extern "C" {

int trackmotion_abi_version(void) { return TRACKMOTION_ABI_VERSION; }

const char *trackmotion_last_error(void) { return g_err; }

int trackmotion_observe(const float *scores, const int64_t *labels, const float *boxes, const int64_t *ids,
                        const int64_t *disappear_time, const float *last_appear_boxes, int n, int K,
                        float track_score_thresh, int64_t miss_tolerance, float *table_boxes, int32_t *table_count,
                        int capacity, int L, int64_t *ids_out, int64_t *disappear_time_out,
                        float *last_appear_boxes_out, int32_t *status, void *stream) {
    if (const int rc = check_rows(n, "trackmotion_observe")) return rc;
    if (const int rc = check_table(capacity, L, "trackmotion_observe")) return rc;
    if (K < 0) return fail(1, "trackmotion_observe: negative class count K");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (K < 1) return fail(1, "trackmotion_observe: K < 1 with rows to judge");
    if ((int64_t)n * K > INT32_MAX) return fail(2, "trackmotion_observe: n * K exceeds the 32-bit indexing");
    if (!scores || !labels || !boxes || !ids || !disappear_time || !last_appear_boxes || !ids_out ||
        !disappear_time_out || !last_appear_boxes_out || !status || (capacity > 0 && (!table_boxes || !table_count)))
        return fail(1, "trackmotion_observe: null pointer");
    hipLaunchKernelGGL(observe_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, scores, labels, boxes,
                       ids, disappear_time, last_appear_boxes, n, K, track_score_thresh, miss_tolerance, table_boxes,
                       table_count, capacity, L, ids_out, disappear_time_out, last_appear_boxes_out, status);
    return check_launch("observe_kernel");
}

int trackmotion_register(const float *new_boxes, int n, int64_t first_id, float *table_boxes, int32_t *table_count,
                         int capacity, int L, void *stream) {
    if (const int rc = check_rows(n, "trackmotion_register")) return rc;
    if (const int rc = check_table(capacity, L, "trackmotion_register")) return rc;
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!new_boxes || !table_boxes || !table_count) return fail(1, "trackmotion_register: null pointer");
    if (first_id < 0 || first_id + n > capacity) {
        char msg[200];
        snprintf(msg, sizeof(msg), "trackmotion_register: ids %lld .. %lld are outside the table (capacity %d)",
                 (long long)first_id, (long long)first_id + n - 1, capacity);
        return fail(1, msg);
    }
    hipLaunchKernelGGL(register_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, new_boxes, n,
                       first_id, table_boxes, table_count, L);
    return check_launch("register_kernel");
}

int trackmotion_extrapolate(const int64_t *ids, const int64_t *disappear_time, const float *last_appear_boxes,
                            const float *ref_pts, int n, float motion_lambda, int min_length,
                            const float *table_boxes, const int32_t *table_count, int capacity, int L,
                            float *ref_pts_out, float *delta_out, void *stream) {
    if (const int rc = check_rows(n, "trackmotion_extrapolate")) return rc;
    if (const int rc = check_table(capacity, L, "trackmotion_extrapolate")) return rc;
    if (min_length < 2) return fail(1, "trackmotion_extrapolate: min_length < 2 (the mean is over count - 1 steps)");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!ids || !disappear_time || !last_appear_boxes || !ref_pts || !ref_pts_out ||
        (capacity > 0 && (!table_boxes || !table_count)))
        return fail(1, "trackmotion_extrapolate: null pointer");
    hipLaunchKernelGGL(extrapolate_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, ids,
                       disappear_time, last_appear_boxes, ref_pts, n, motion_lambda, min_length, table_boxes,
                       table_count, capacity, L, ref_pts_out, delta_out);
    return check_launch("extrapolate_kernel");
}

}  // extern "C"
