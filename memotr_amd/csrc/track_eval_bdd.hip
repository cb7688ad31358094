// track_eval_bdd.hip -- BDD100K's evaluation in front of the metric kernels of track_eval.hip: the cut of every frame
// into its 8 evaluated classes, box IoU on corner boxes, and the preprocessing of TrackEval's datasets/bdd100k.py
// (C ABI and data layout: include/track_eval_bdd_hip.h; the same definition on the host:
// memotr_amd/evaluation_bdd100k.py; how the work is cut: DESIGN.md, "Evaluation").
//
//   class_count_kernel   one wavefront per (frame, side): rows per class, 64 rows per ballot
//   class_split_kernel   one wavefront per (frame, side): the stable scatter into the problem-major layout; a row's
//                        place is the running count of its class plus the ballot's prefix count below its lane
//   similarity_kernel    one workgroup per split frame, one thread per matrix entry
//   preproc_kernel       one wavefront per split frame: assignment on the thresholded similarity marks the matched
//                        detections (LDS flags); every other detection walks the frame's ignore regions
// The assignment is assign_core.h with a cost view.  All arithmetic is float64, contraction off (the build passes
// -ffp-contract=off for this file as well); no atomics at all: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/track_eval_bdd_hip.h"
#include "assign_core.h"

namespace {

thread_local char g_err[256] = {0};      // text of this thread's last error; read by bddeval_last_error() only

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

constexpr double EPS = DBL_EPSILON;              // np.finfo('float').eps
constexpr double MATCH_THRESHOLD = 0.5;
constexpr double IGNORE_THRESHOLD = 0.5;
constexpr int N_CLASSES = BDDEVAL_N_CLASSES;
constexpr int LDS_OPT_IN = 160 * 1024;           // LDS of a gfx950 CU; above 64 KiB a kernel has to ask

using assign::WaveLanes;

__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
__host__ __device__ inline size_t pairs_bytes(int mn) { return align16((size_t)2 * mn * 4); }

// TrackEval's class id -> class index in its order of evaluation, -1: not evaluated
__device__ __forceinline__ int class_index(int id) {
    switch (id) {
        case 1: return 0;       // pedestrian
        case 2: return 1;       // rider
        case 4: return 2;       // car
        case 5: return 3;       // bus
        case 6: return 4;       // truck
        case 7: return 5;       // train
        case 10: return 6;      // motorcycle
        case 11: return 7;      // bicycle
        default: return -1;
    }
}

// ---------------------------------------------------------------------------------------------------- class split
struct Sides {
    const int32_t *classes[2], *off[2];
};

__global__ __launch_bounds__(64) void class_count_kernel(const Sides in, const int32_t *__restrict__ seq_off,
                                                          const int32_t *__restrict__ frame_seq,
                                                          int32_t *__restrict__ gt_count,
                                                          int32_t *__restrict__ tr_count) {
    const int f = blockIdx.x, side = blockIdx.y, lane = threadIdx.x;
    const int32_t *classes = in.classes[side];
    const int r0 = in.off[side][f], n = in.off[side][f + 1] - r0;
    int total[N_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < n; base += 64) {              // (wave-uniform trip count: every lane votes)
        const int i = base + lane;
        const int ci = i < n ? class_index(classes[r0 + i]) : -1;
#pragma unroll
        for (int c = 0; c < N_CLASSES; ++c) total[c] += __popcll(__ballot(ci == c));
    }
    const int s = frame_seq[f], f0 = seq_off[s], T = seq_off[s + 1] - f0;
    int32_t *out = side == 0 ? gt_count : tr_count;
    int mine = 0;
#pragma unroll
    for (int c = 0; c < N_CLASSES; ++c) mine = lane == c ? total[c] : mine;
    if (lane < N_CLASSES) out[(size_t)N_CLASSES * f0 + (size_t)lane * T + (f - f0)] = mine;
}

struct SplitIo {
    const double *boxes[2];
    const int32_t *ids[2], *split_off[2];
    double *out_boxes[2];
    int32_t *out_ids[2];
};

__global__ __launch_bounds__(64) void class_split_kernel(const Sides in, const SplitIo io,
                                                          const int32_t *__restrict__ seq_off,
                                                          const int32_t *__restrict__ frame_seq) {
    const int f = blockIdx.x, side = blockIdx.y, lane = threadIdx.x;
    const int32_t *classes = in.classes[side], *split_off = io.split_off[side];
    const int r0 = in.off[side][f], n = in.off[side][f + 1] - r0;
    const int s = frame_seq[f], f0 = seq_off[s], T = seq_off[s + 1] - f0;
    const size_t q0 = (size_t)N_CLASSES * f0 + (f - f0);    // split frame of class c: q0 + c * T
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int seen[N_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0};         // rows of each class in the chunks before this one
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const int ci = i < n ? class_index(classes[r0 + i]) : -1;
        int rank = 0;
#pragma unroll
        for (int c = 0; c < N_CLASSES; ++c) {
            const unsigned long long votes = __ballot(ci == c);
            if (ci == c) rank = seen[c] + __popcll(votes & below);
            seen[c] += __popcll(votes);
        }
        if (ci >= 0) {
            const size_t q = q0 + (size_t)ci * T;
            const int dst = split_off[q] + rank;
            if (dst < split_off[q + 1]) {                    // (offsets that do not belong to these classes: no write)
                const double *b = io.boxes[side] + (size_t)(r0 + i) * 4;
                double *o = io.out_boxes[side] + (size_t)dst * 4;
                o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
                io.out_ids[side][dst] = io.ids[side][r0 + i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- similarity
__global__ __launch_bounds__(256) void similarity_kernel(const double *__restrict__ gt_boxes,
                                                          const double *__restrict__ tr_boxes,
                                                          const int32_t *__restrict__ gt_off,
                                                          const int32_t *__restrict__ tr_off,
                                                          const int64_t *__restrict__ sim_off,
                                                          double *__restrict__ sim) {
#pragma clang fp contract(off)
    const int f = blockIdx.x;
    const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
    double *out = sim + sim_off[f];
    const int n = g * k;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int i = e / k, j = e - i * k;
        const double *a = gt_boxes + (size_t)(g0 + i) * 4, *b = tr_boxes + (size_t)(k0 + j) * 4;
        const double ax0 = a[0], ay0 = a[1], ax1 = a[2], ay1 = a[3];
        const double bx0 = b[0], by0 = b[1], bx1 = b[2], by1 = b[3];
        const double w = (ax1 < bx1 ? ax1 : bx1) - (ax0 > bx0 ? ax0 : bx0);
        const double h = (ay1 < by1 ? ay1 : by1) - (ay0 > by0 ? ay0 : by0);
        double inter = (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
        const double area1 = (ax1 - ax0) * (ay1 - ay0), area2 = (bx1 - bx0) * (by1 - by0);
        double uni = area1 + area2 - inter;
        if (area1 <= EPS || area2 <= EPS || uni <= EPS) inter = 0.0;
        if (uni <= EPS) uni = 1.0;
        out[e] = inter / uni;
    }
}

// ------------------------------------------------------------------------------------------------- preprocessing
struct PreprocView {
    const double *s;
    int k;
    __device__ __forceinline__ double score(int i, int j) const {
        const double v = s[(size_t)i * k + j];
        return v < MATCH_THRESHOLD - EPS ? 0.0 : v;
    }
    __device__ __forceinline__ double at(int i, int j) const { return -score(i, j); }
};

__global__ __launch_bounds__(64) void preproc_kernel(const double *__restrict__ sim,
                                                      const int64_t *__restrict__ sim_off,
                                                      const int32_t *__restrict__ gt_off,
                                                      const int32_t *__restrict__ tr_off,
                                                      const double *__restrict__ tr_boxes,
                                                      const int32_t *__restrict__ ig_off,
                                                      const double *__restrict__ ig_boxes,
                                                      const int32_t *__restrict__ frame_src, int max_gt, int max_tr,
                                                      int mn, int32_t *__restrict__ tr_remove,
                                                      int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int q = blockIdx.x;
    const int g0 = gt_off[q], g = gt_off[q + 1] - g0, k0 = tr_off[q], k = tr_off[q + 1] - k0;
    int32_t *rows = reinterpret_cast<int32_t *>(smem), *cols = rows + mn;
    unsigned char *matched = smem + pairs_bytes(mn);                         // [max_tr] 1: the detection has a pair
    unsigned char *work = matched + align16((size_t)max_tr);
    const WaveLanes lanes{(int)threadIdx.x};
    int rc = 0;
    if (g > max_gt || k > max_tr) {
        rc = -2;
    } else if (k > 0) {
        lanes.each(k, [&](int j) { matched[j] = 0; });
        lanes.sync();
        if (g > 0) {
            const PreprocView view{sim + sim_off[q], k};
            const int n = assign::solve_view(lanes, view, g, k, work, rows, cols);
            rc = n < 0 ? -1 : 0;
            lanes.each(n, [&](int p) {
                if (view.score(rows[p], cols[p]) > EPS) matched[cols[p]] = 1;
            });
            lanes.sync();
        }
        if (rc == 0) {
            const int f = frame_src[q];
            const int r0 = ig_off[f], r1 = ig_off[f + 1];
            lanes.each(k, [&](int j) {
                if (matched[j]) return;
                const double *a = tr_boxes + (size_t)(k0 + j) * 4;
                const double ax0 = a[0], ay0 = a[1], ax1 = a[2], ay1 = a[3];
                const double area = (ax1 - ax0) * (ay1 - ay0);
                if (!(area > 0.0 + EPS)) return;                             // (its intersection over area counts as 0)
                bool inside = false;
                for (int r = r0; r < r1 && !inside; ++r) {
                    const double *b = ig_boxes + (size_t)r * 4;
                    const double w = (ax1 < b[2] ? ax1 : b[2]) - (ax0 > b[0] ? ax0 : b[0]);
                    const double h = (ay1 < b[3] ? ay1 : b[3]) - (ay0 > b[1] ? ay0 : b[1]);
                    const double inter = (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
                    inside = inter / area > IGNORE_THRESHOLD + EPS;
                }
                if (inside) tr_remove[k0 + j] = 1;
            });
        }
    }
    if (threadIdx.x == 0) status[q] = rc;
}

// ------------------------------------------------------------------------------------------------------ host side
int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    g_err[0] = 0;
    return 0;
}

// dynamic LDS beyond the default limit of a launch: opt in once per kernel and device (as track_eval.hip)
int allow_lds(const void *kernel, size_t lds, std::atomic<unsigned long long> &done, const char *who) {
    if (lds <= 64 * 1024) return 0;
    if (lds > (size_t)LDS_OPT_IN) {
        snprintf(g_err, sizeof(g_err), "%s: problem does not fit the LDS of a CU", who);
        return 2;
    }
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_OPT_IN) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(g_err, sizeof(g_err), "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed", who);
        return 3;
    }
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

int check_frames(int n_frames, int limit, const char *who) {
    if (n_frames < 0) {
        snprintf(g_err, sizeof(g_err), "%s: negative frame count", who);
        return 1;
    }
    if (n_frames > limit) {
        snprintf(g_err, sizeof(g_err), "%s: %d frames in one call exceed %d", who, n_frames, limit);
        return 2;
    }
    return 0;
}

}  // namespace

extern "C" {

int bddeval_abi_version(void) { return BDDEVAL_ABI_VERSION; }
const char *bddeval_last_error(void) { return g_err; }

int bddeval_class_count(const int32_t *gt_classes, const int32_t *tr_classes, const int32_t *gt_off,
                        const int32_t *tr_off, const int32_t *seq_off, const int32_t *frame_seq, int n_frames,
                        int32_t *gt_count, int32_t *tr_count, void *stream) {
    if (const int rc = check_frames(n_frames, INT32_MAX / N_CLASSES, "bddeval_class_count")) return rc;
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!gt_classes || !tr_classes || !gt_off || !tr_off || !seq_off || !frame_seq || !gt_count || !tr_count)
        return fail(1, "bddeval_class_count: null pointer");
    const Sides in{{gt_classes, tr_classes}, {gt_off, tr_off}};
    hipLaunchKernelGGL(class_count_kernel, dim3(n_frames, 2), dim3(64), 0, (hipStream_t)stream, in, seq_off,
                       frame_seq, gt_count, tr_count);
    return check_launch("class_count_kernel");
}

int bddeval_class_split(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_ids, const int32_t *tr_ids,
                        const int32_t *gt_classes, const int32_t *tr_classes, const int32_t *gt_off,
                        const int32_t *tr_off, const int32_t *seq_off, const int32_t *frame_seq, int n_frames,
                        const int32_t *split_gt_off, const int32_t *split_tr_off, double *out_gt_boxes,
                        double *out_tr_boxes, int32_t *out_gt_ids, int32_t *out_tr_ids, void *stream) {
    if (const int rc = check_frames(n_frames, INT32_MAX / N_CLASSES, "bddeval_class_split")) return rc;
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!gt_boxes || !tr_boxes || !gt_ids || !tr_ids || !gt_classes || !tr_classes || !gt_off || !tr_off ||
        !seq_off || !frame_seq || !split_gt_off || !split_tr_off || !out_gt_boxes || !out_tr_boxes || !out_gt_ids ||
        !out_tr_ids)
        return fail(1, "bddeval_class_split: null pointer");
    const Sides in{{gt_classes, tr_classes}, {gt_off, tr_off}};
    const SplitIo io{{gt_boxes, tr_boxes}, {gt_ids, tr_ids}, {split_gt_off, split_tr_off},
                     {out_gt_boxes, out_tr_boxes}, {out_gt_ids, out_tr_ids}};
    hipLaunchKernelGGL(class_split_kernel, dim3(n_frames, 2), dim3(64), 0, (hipStream_t)stream, in, io, seq_off,
                       frame_seq);
    return check_launch("class_split_kernel");
}

int bddeval_similarity(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_off, const int32_t *tr_off,
                       const int64_t *sim_off, int n_frames, double *sim, void *stream) {
    if (const int rc = check_frames(n_frames, INT32_MAX, "bddeval_similarity")) return rc;
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!gt_boxes || !tr_boxes || !gt_off || !tr_off || !sim_off || !sim)
        return fail(1, "bddeval_similarity: null pointer");
    hipLaunchKernelGGL(similarity_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, gt_boxes, tr_boxes,
                       gt_off, tr_off, sim_off, sim);
    return check_launch("similarity_kernel");
}

int bddeval_preproc(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                    const double *tr_boxes, const int32_t *ig_off, const double *ig_boxes, const int32_t *frame_src,
                    int n_frames, int max_gt, int max_tr, int32_t *tr_remove, int32_t *status, void *stream) {
    if (const int rc = check_frames(n_frames, INT32_MAX, "bddeval_preproc")) return rc;
    if (max_gt < 0 || max_tr < 0) return fail(1, "bddeval_preproc: negative frame size");
    if (max_gt > BDDEVAL_MAX_DIM || max_tr > BDDEVAL_MAX_DIM) {
        snprintf(g_err, sizeof(g_err), "bddeval_preproc: a frame with %d ground-truth and %d tracker detections of "
                 "one class exceeds BDDEVAL_MAX_DIM = %d", max_gt, max_tr, BDDEVAL_MAX_DIM);
        return 2;
    }
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!sim || !sim_off || !gt_off || !tr_off || !tr_boxes || !ig_off || !ig_boxes || !frame_src || !tr_remove ||
        !status)
        return fail(1, "bddeval_preproc: null pointer");
    static std::atomic<unsigned long long> allowed{0};
    const int mn = max_gt < max_tr ? max_gt : max_tr, mx = max_gt < max_tr ? max_tr : max_gt;
    const size_t lds = pairs_bytes(mn) + align16((size_t)max_tr) + align16(assign::work_bytes(mn, mx));
    if (const int rc = allow_lds(reinterpret_cast<const void *>(preproc_kernel), lds, allowed, "bddeval_preproc"))
        return rc;
    hipLaunchKernelGGL(preproc_kernel, dim3(n_frames), dim3(64), lds, (hipStream_t)stream, sim, sim_off, gt_off,
                       tr_off, tr_boxes, ig_off, ig_boxes, frame_src, max_gt, max_tr, mn, tr_remove, status);
    return check_launch("preproc_kernel");
}

}  // extern "C"
