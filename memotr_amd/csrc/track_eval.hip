// track_eval.hip -- tracking evaluation on the device: box IoU, the MOT-challenge preprocessing match, and the HOTA,
// CLEAR and Identity metrics with TrackEval's definitions (C ABI and data layout: include/track_eval_hip.h; the same
// definition on the host: memotr_amd/evaluation.py; how the work is cut and what it costs: DESIGN.md, "Evaluation").
//
//   similarity_kernel     one workgroup per frame, one thread per matrix entry
//   preproc_match_kernel  one wavefront per frame: assignment on the thresholded similarity, flags tracker detections
//                         matched to a distractor
//   accumulate_kernel     one workgroup per sequence walks the frames: a table cell (gt id, tracker id) is touched at
//                         most once per frame (ids are unique in a frame), so its float sum is formed in frame order
//                         without an atomic; ends with the global alignment score
//   hota_match_kernel     one wavefront per frame: assignment on -(alignment * similarity), then lane a counts the
//                         matches of threshold a (integer atomics into the per-threshold match tables)
//   hota_reduce_kernel    one wavefront per (threshold, sequence): lane-strided partial sums, xor butterfly
//   clear_kernel          one wavefront per sequence walks the frames (each match depends on the previous frame's);
//                         the per-id state lives in LDS
//   identity_kernel       one wavefront per sequence: the (G + K) x (G + K) problem, cost computed from the counts
// Every assignment is assign_core.h with a cost view that computes the entry where the solver asks for it.  All
// arithmetic is float64, contraction off (the build passes -ffp-contract=off for this file as well); no float atomics:
// the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/track_eval_hip.h"
#include "assign_core.h"

namespace {

thread_local char g_err[256] = {0};      // text of this thread's last error; read by trackeval_last_error() only

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

constexpr double EPS = DBL_EPSILON;              // np.finfo('float').eps
constexpr double MATCH_THRESHOLD = 0.5;          // CLEAR's, Identity's and the preprocessing's
constexpr int N_ALPHA = TRACKEVAL_N_ALPHA;
constexpr int LDS_OPT_IN = 160 * 1024;           // LDS of a gfx950 CU; above 64 KiB a kernel has to ask

using assign::WaveLanes;

struct Alphas {
    double v[N_ALPHA];
};

__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// LDS of one assignment of a launch: the pair lists (2 * mn int32), then the solver's scratch for (mn x mx)
__host__ __device__ inline size_t pairs_bytes(int mn) { return align16((size_t)2 * mn * 4); }
__host__ inline size_t solve_bytes(int a, int b) {
    const int mn = a < b ? a : b, mx = a < b ? b : a;
    return pairs_bytes(mn) + align16(assign::work_bytes(mn, mx));
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
        const double ax0 = a[0], ay0 = a[1], ax1 = a[0] + a[2], ay1 = a[1] + a[3];
        const double bx0 = b[0], by0 = b[1], bx1 = b[0] + b[2], by1 = b[1] + b[3];
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

__device__ __forceinline__ bool is_distractor(int cls) { return cls == 2 || cls == 7 || cls == 8 || cls == 12; }

__global__ __launch_bounds__(64) void preproc_match_kernel(const double *__restrict__ sim,
                                                            const int64_t *__restrict__ sim_off,
                                                            const int32_t *__restrict__ gt_off,
                                                            const int32_t *__restrict__ tr_off,
                                                            const int32_t *__restrict__ gt_classes, int max_gt,
                                                            int max_tr, int mn, int32_t *__restrict__ tr_remove,
                                                            int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x;
    const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
    int32_t *rows = reinterpret_cast<int32_t *>(smem), *cols = rows + mn;
    const WaveLanes lanes{(int)threadIdx.x};
    int rc = 0;
    if (g > max_gt || k > max_tr) {
        rc = -2;
    } else if (g > 0 && k > 0) {
        const PreprocView view{sim + sim_off[f], k};
        const int n = assign::solve_view(lanes, view, g, k, smem + pairs_bytes(mn), rows, cols);
        rc = n < 0 ? -1 : 0;
        lanes.each(n, [&](int p) {
            if (view.score(rows[p], cols[p]) > EPS && is_distractor(gt_classes[g0 + rows[p]]))
                tr_remove[k0 + cols[p]] = 1;
        });
    }
    if (threadIdx.x == 0) status[f] = rc;
}

// ----------------------------------------------------------------------------- HOTA pass 1 and Identity's counts
struct SeqTables {
    const int32_t *n_gt_ids, *n_tr_ids;
    const int64_t *cell_off;
    const int32_t *gid_off, *tid_off;
};

__global__ __launch_bounds__(256) void accumulate_kernel(const double *__restrict__ sim,
                                                          const int64_t *__restrict__ sim_off,
                                                          const int32_t *__restrict__ gt_off,
                                                          const int32_t *__restrict__ tr_off,
                                                          const int32_t *__restrict__ gt_ids,
                                                          const int32_t *__restrict__ tr_ids,
                                                          const int32_t *__restrict__ seq_off, const SeqTables t,
                                                          int max_gt, int max_tr, double *__restrict__ potential,
                                                          int32_t *__restrict__ id_matches,
                                                          int32_t *__restrict__ gt_count,
                                                          int32_t *__restrict__ tr_count,
                                                          double *__restrict__ alignment) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *rowsum = reinterpret_cast<double *>(smem), *colsum = rowsum + max_gt;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int G = t.n_gt_ids[s], K = t.n_tr_ids[s];
    const long cells = (long)G * K;
    double *pot = potential + t.cell_off[s];
    int32_t *idm = id_matches + t.cell_off[s];
    int32_t *gc = gt_count + t.gid_off[s], *tc = tr_count + t.tid_off[s];
    for (long c = tid; c < cells; c += 256) {
        pot[c] = 0.0;
        idm[c] = 0;
    }
    for (int i = tid; i < G; i += 256) gc[i] = 0;
    for (int j = tid; j < K; j += 256) tc[j] = 0;
    __syncthreads();
    for (int f = seq_off[s]; f < seq_off[s + 1]; ++f) {
        const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
        if (g > max_gt || k > max_tr) continue;             // (reported by hota_match_kernel's status)
        const double *sm = sim + sim_off[f];
        for (int x = tid; x < g + k; x += 256) {            // one thread per row or column: its sum, its id's count
            double acc = 0.0;
            if (x < g) {
                for (int j = 0; j < k; ++j) acc += sm[(size_t)x * k + j];
                rowsum[x] = acc;
                const int id = gt_ids[g0 + x];
                if (id >= 0 && id < G) gc[id] += 1;
            } else {
                const int j = x - g;
                for (int i = 0; i < g; ++i) acc += sm[(size_t)i * k + j];
                colsum[j] = acc;
                const int id = tr_ids[k0 + j];
                if (id >= 0 && id < K) tc[id] += 1;
            }
        }
        __syncthreads();
        for (int e = tid; e < g * k; e += 256) {
            const int i = e / k, j = e - i * k;
            const int gi = gt_ids[g0 + i], tj = tr_ids[k0 + j];
            if (gi < 0 || gi >= G || tj < 0 || tj >= K) continue;
            const double v = sm[e];
            const double denom = colsum[j] + rowsum[i] - v;
            if (denom > 0.0 + EPS) pot[(long)gi * K + tj] += v / denom;
            if (v >= MATCH_THRESHOLD) idm[(long)gi * K + tj] += 1;
        }
        __syncthreads();
    }
    for (long c = tid; c < cells; c += 256) {
        const int gi = (int)(c / K), tj = (int)(c - (long)gi * K);
        alignment[t.cell_off[s] + c] = pot[c] / ((double)gc[gi] + (double)tc[tj] - pot[c]);
    }
}

// ---------------------------------------------------------------------------------------------------- HOTA pass 2
struct HotaView {
    const double *s, *align;        // the frame's similarity; the sequence's alignment table
    const int32_t *gid, *tid;       // the frame's ids
    int k, K;
    __device__ __forceinline__ double at(int i, int j) const {
        return -(align[(long)gid[i] * K + tid[j]] * s[(size_t)i * k + j]);
    }
};

__global__ __launch_bounds__(64) void hota_match_kernel(const double *__restrict__ sim,
                                                         const int64_t *__restrict__ sim_off,
                                                         const int32_t *__restrict__ gt_off,
                                                         const int32_t *__restrict__ tr_off,
                                                         const int32_t *__restrict__ gt_ids,
                                                         const int32_t *__restrict__ tr_ids,
                                                         const int32_t *__restrict__ frame_seq,
                                                         const int32_t *__restrict__ n_tr_ids,
                                                         const int64_t *__restrict__ cell_off,
                                                         const double *__restrict__ alignment, const Alphas alphas,
                                                         int max_gt, int max_tr, int mn, int32_t *__restrict__ matches,
                                                         int32_t *__restrict__ tp, double *__restrict__ loc,
                                                         int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
    int32_t *rows = reinterpret_cast<int32_t *>(smem), *cols = rows + mn;
    const WaveLanes lanes{lane};
    int rc = 0, n = 0;
    const int s = frame_seq[f];
    const int K = n_tr_ids[s];
    const long c0 = cell_off[s], cells = cell_off[s + 1] - c0;
    const double *sm = sim + sim_off[f];
    if (g > max_gt || k > max_tr) {
        rc = -2;
    } else if (g > 0 && k > 0) {
        const HotaView view{sm, alignment + c0, gt_ids + g0, tr_ids + k0, k, K};
        n = assign::solve_view(lanes, view, g, k, smem + pairs_bytes(mn), rows, cols);
        if (n < 0) {
            rc = -1;
            n = 0;
        }
    }
    if (lane < N_ALPHA) {                                   // lane a: threshold a, the pairs in scipy's order
        const double thr = alphas.v[lane] - EPS;
        int32_t *mc = matches + N_ALPHA * c0 + (long)lane * cells;
        int count = 0;
        double sum = 0.0;
        for (int p = 0; p < n; ++p) {
            const double v = sm[(size_t)rows[p] * k + cols[p]];
            if (v >= thr) {
                ++count;
                sum += v;
                atomicAdd(mc + (long)gt_ids[g0 + rows[p]] * K + tr_ids[k0 + cols[p]], 1);
            }
        }
        tp[(size_t)f * N_ALPHA + lane] = count;
        loc[(size_t)f * N_ALPHA + lane] = sum;
    }
    if (lane == 0) status[f] = rc;
}

__device__ __forceinline__ double wave_sum(double v) {      // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void hota_reduce_kernel(const int32_t *__restrict__ seq_off, const SeqTables t,
                                                          const int32_t *__restrict__ gt_count,
                                                          const int32_t *__restrict__ tr_count,
                                                          const int32_t *__restrict__ matches,
                                                          const int32_t *__restrict__ tp,
                                                          const double *__restrict__ loc,
                                                          int64_t *__restrict__ out_tp,
                                                          double *__restrict__ out_sums) {
#pragma clang fp contract(off)
    const int a = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const int K = t.n_tr_ids[s];
    const long c0 = t.cell_off[s], cells = t.cell_off[s + 1] - c0;
    const int32_t *mc = matches + N_ALPHA * c0 + (long)a * cells;
    const int32_t *gc = gt_count + t.gid_off[s], *tc = tr_count + t.tid_off[s];
    double ass_a = 0.0, ass_re = 0.0, ass_pr = 0.0, loc_sum = 0.0;
    for (long c = lane; c < cells; c += 64) {
        const int gi = (int)(c / K), tj = (int)(c - (long)gi * K);
        const double m = (double)mc[c], cg = (double)gc[gi], ct = (double)tc[tj];
        const double d = cg + ct - m;
        ass_a += m * (m / (d > 1.0 ? d : 1.0));
        ass_re += m * (m / (cg > 1.0 ? cg : 1.0));
        ass_pr += m * (m / (ct > 1.0 ? ct : 1.0));
    }
    long long count = 0;
    for (int f = seq_off[s] + lane; f < seq_off[s + 1]; f += 64) {
        count += tp[(size_t)f * N_ALPHA + a];
        loc_sum += loc[(size_t)f * N_ALPHA + a];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) count += __shfl_xor(count, off, 64);
    ass_a = wave_sum(ass_a);
    ass_re = wave_sum(ass_re);
    ass_pr = wave_sum(ass_pr);
    loc_sum = wave_sum(loc_sum);
    if (lane == 0) {
        out_tp[(size_t)s * N_ALPHA + a] = count;
        double *o = out_sums + (size_t)s * 4 * N_ALPHA + a;
        o[0] = ass_a;
        o[N_ALPHA] = ass_re;
        o[2 * N_ALPHA] = ass_pr;
        o[3 * N_ALPHA] = loc_sum;
    }
}

// ---------------------------------------------------------------------------------------------------------- CLEAR
struct ClearView {
    const double *s;
    const int32_t *gid, *tid;       // the frame's ids
    const int32_t *prev_step;       // [G] tracker id matched in the previous evaluated frame, -1: none
    int k;
    __device__ __forceinline__ double at(int i, int j) const {
        const double v = s[(size_t)i * k + j];
        if (v < MATCH_THRESHOLD - EPS) return -0.0;
        return -((tid[j] == prev_step[gid[i]] ? 1000.0 : 0.0) + v);
    }
};

__global__ __launch_bounds__(64) void clear_kernel(const double *__restrict__ sim, const int64_t *__restrict__ sim_off,
                                                    const int32_t *__restrict__ gt_off,
                                                    const int32_t *__restrict__ tr_off,
                                                    const int32_t *__restrict__ gt_ids,
                                                    const int32_t *__restrict__ tr_ids,
                                                    const int32_t *__restrict__ seq_off,
                                                    const int32_t *__restrict__ n_gt_ids, int max_gt, int max_tr,
                                                    int max_gt_ids, int mn, int32_t *__restrict__ out_ints,
                                                    double *__restrict__ motp_sum, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int G = n_gt_ids[s];
    int32_t *rows = reinterpret_cast<int32_t *>(smem), *cols = rows + mn;
    int32_t *seen = reinterpret_cast<int32_t *>(smem + pairs_bytes(mn));     // [G] frames the id is present in
    int32_t *matched = seen + max_gt_ids, *frag = matched + max_gt_ids;      // [G] frames matched; track starts
    int32_t *prev = frag + max_gt_ids, *prev_step = prev + max_gt_ids;       // [G] last match ever / in the last frame
    int32_t *was_free = prev_step + max_gt_ids;                              // [G] prev_step before this frame
    unsigned char *work = smem + pairs_bytes(mn) + align16((size_t)6 * max_gt_ids * 4);
    const WaveLanes lanes{lane};
    int rc = G > max_gt_ids ? -2 : 0;
    int n_tp = 0, n_fn = 0, n_fp = 0, n_idsw = 0;           // lane 0's are the result
    double motp = 0.0;
    if (rc == 0) {
        lanes.each(G, [&](int i) { seen[i] = matched[i] = frag[i] = 0; prev[i] = prev_step[i] = -1; });
        lanes.sync();
    }
    for (int f = seq_off[s]; rc == 0 && f < seq_off[s + 1]; ++f) {
        const int g0 = gt_off[f], g = gt_off[f + 1] - g0, k0 = tr_off[f], k = tr_off[f + 1] - k0;
        if (g > max_gt || k > max_tr) {
            rc = -2;
            break;
        }
        if (g == 0) {
            n_fp += k;
            continue;
        }
        const int32_t *gid = gt_ids + g0, *tid = tr_ids + k0;
        if (k == 0) {
            n_fn += g;
            lanes.each(g, [&](int i) { seen[gid[i]] += 1; });
            lanes.sync();
            continue;
        }
        const double *sm = sim + sim_off[f];
        const ClearView view{sm, gid, tid, prev_step, k};
        const int n = assign::solve_view(lanes, view, g, k, work, rows, cols);
        if (n < 0) {
            rc = -1;
            break;
        }
        lanes.each(G, [&](int i) { was_free[i] = prev_step[i] < 0; prev_step[i] = -1; });
        lanes.each(g, [&](int i) { seen[gid[i]] += 1; });
        lanes.sync();
        int n_match = 0;
        if (lane == 0) {                                    // the pairs in scipy's order: the order MOTP is summed in
            double frame_sum = 0.0;
            for (int p = 0; p < n; ++p) {
                const double v = sm[(size_t)rows[p] * k + cols[p]];
                if (v < MATCH_THRESHOLD - EPS) continue;    // (a kept score is >= 0.5 - eps > eps)
                const int gi = gid[rows[p]], tj = tid[cols[p]];
                if (prev[gi] >= 0 && prev[gi] != tj) ++n_idsw;
                matched[gi] += 1;
                prev[gi] = tj;
                prev_step[gi] = tj;
                frame_sum += v;
                ++n_match;
            }
            if (n_match > 0) motp += frame_sum;
        }
        lanes.sync();
        lanes.each(G, [&](int i) { frag[i] += (was_free[i] && prev_step[i] >= 0) ? 1 : 0; });
        lanes.sync();
        n_tp += n_match;
        n_fn += g - n_match;
        n_fp += k - n_match;
    }
    if (lane == 0) {
        int mt = 0, pt = 0, n_frag = 0;
        if (rc == 0)
            for (int i = 0; i < G; ++i) {
                if (seen[i] > 0) {
                    const double ratio = (double)matched[i] / (double)seen[i];
                    if (ratio > 0.8) ++mt;
                    if (ratio >= 0.2) ++pt;
                }
                if (frag[i] > 0) n_frag += frag[i] - 1;
            }
        pt -= mt;
        int32_t *o = out_ints + (size_t)s * TRACKEVAL_CLEAR_INTS;
        o[0] = n_tp; o[1] = n_fn; o[2] = n_fp; o[3] = n_idsw;
        o[4] = mt; o[5] = pt; o[6] = G - mt - pt; o[7] = n_frag;
        motp_sum[s] = motp;
        status[s] = rc;
    }
}

// ------------------------------------------------------------------------------------------------------- Identity
struct IdentityView {
    const int32_t *gc, *tc, *idm;   // detections per gt id, per tracker id; frames with sim >= 0.5 per (gt id, tracker id)
    int G, K;
    __device__ __forceinline__ double fn(int i, int j) const {
        if (i >= G) return 0.0;
        if (j < K) return (double)gc[i] - (double)idm[(long)i * K + j];
        return j - K == i ? (double)gc[i] : 1e10;
    }
    __device__ __forceinline__ double fp(int i, int j) const {
        if (j >= K) return 0.0;
        if (i < G) return (double)tc[j] - (double)idm[(long)i * K + j];
        return i - G == j ? (double)tc[j] : 1e10;
    }
    __device__ __forceinline__ double at(int i, int j) const { return fn(i, j) + fp(i, j); }
};

__global__ __launch_bounds__(64) void identity_kernel(const SeqTables t, const int32_t *__restrict__ gt_count,
                                                       const int32_t *__restrict__ tr_count,
                                                       const int32_t *__restrict__ id_matches, int max_ids,
                                                       int64_t *__restrict__ out, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int G = t.n_gt_ids[s], K = t.n_tr_ids[s], N = G + K;
    int32_t *rows = reinterpret_cast<int32_t *>(smem), *cols = rows + max_ids;
    const WaveLanes lanes{lane};
    int rc = 0;
    double sum_fn = 0.0, sum_fp = 0.0;
    if (N > max_ids) {
        rc = -2;
    } else if (N > 0) {
        const IdentityView view{gt_count + t.gid_off[s], tr_count + t.tid_off[s], id_matches + t.cell_off[s], G, K};
        const int n = assign::solve_view(lanes, view, N, N, smem + pairs_bytes(max_ids), rows, cols);
        if (n < 0) rc = -1;
        else if (lane == 0)
            for (int p = 0; p < n; ++p) {
                sum_fn += view.fn(rows[p], cols[p]);
                sum_fp += view.fp(rows[p], cols[p]);
            }
    }
    if (lane == 0) {
        out[2 * (size_t)s] = (int64_t)sum_fn;
        out[2 * (size_t)s + 1] = (int64_t)sum_fp;
        status[s] = rc;
    }
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

// dynamic LDS beyond the default limit of a launch: opt in once per kernel and device (gfx950 has 160 KiB per CU;
// the attribute belongs to the current device, so `done` keeps one bit per device ordinal)
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

int check_dims(int max_gt, int max_tr, const char *who) {
    if (max_gt < 0 || max_tr < 0) {
        snprintf(g_err, sizeof(g_err), "%s: negative frame size", who);
        return 1;
    }
    if (max_gt > TRACKEVAL_MAX_DIM || max_tr > TRACKEVAL_MAX_DIM) {
        snprintf(g_err, sizeof(g_err), "%s: a frame with %d ground-truth and %d tracker detections exceeds "
                 "TRACKEVAL_MAX_DIM = %d", who, max_gt, max_tr, TRACKEVAL_MAX_DIM);
        return 2;
    }
    return 0;
}

}  // namespace

extern "C" {

int trackeval_abi_version(void) { return TRACKEVAL_ABI_VERSION; }
const char *trackeval_last_error(void) { return g_err; }

int trackeval_similarity(const double *gt_boxes, const double *tr_boxes, const int32_t *gt_off, const int32_t *tr_off,
                         const int64_t *sim_off, int n_frames, double *sim, void *stream) {
    if (n_frames < 0) return fail(1, "trackeval_similarity: negative frame count");
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!gt_boxes || !tr_boxes || !gt_off || !tr_off || !sim_off || !sim)
        return fail(1, "trackeval_similarity: null pointer");
    hipLaunchKernelGGL(similarity_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, gt_boxes, tr_boxes,
                       gt_off, tr_off, sim_off, sim);
    return check_launch("similarity_kernel");
}

int trackeval_preproc_match(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                            const int32_t *gt_classes, int n_frames, int max_gt, int max_tr, int32_t *tr_remove,
                            int32_t *status, void *stream) {
    if (n_frames < 0) return fail(1, "trackeval_preproc_match: negative frame count");
    if (const int rc = check_dims(max_gt, max_tr, "trackeval_preproc_match")) return rc;
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!sim || !sim_off || !gt_off || !tr_off || !gt_classes || !tr_remove || !status)
        return fail(1, "trackeval_preproc_match: null pointer");
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = solve_bytes(max_gt, max_tr);
    if (const int rc = allow_lds(reinterpret_cast<const void *>(preproc_match_kernel), lds, allowed,
                                 "trackeval_preproc_match"))
        return rc;
    hipLaunchKernelGGL(preproc_match_kernel, dim3(n_frames), dim3(64), lds, (hipStream_t)stream, sim, sim_off, gt_off,
                       tr_off, gt_classes, max_gt, max_tr, max_gt < max_tr ? max_gt : max_tr, tr_remove, status);
    return check_launch("preproc_match_kernel");
}

int trackeval_accumulate(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                         const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *seq_off, int n_seqs,
                         const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                         const int32_t *gid_off, const int32_t *tid_off, int max_gt, int max_tr,
                         double *potential, int32_t *id_matches, int32_t *gt_count, int32_t *tr_count,
                         double *alignment, void *stream) {
    if (n_seqs < 0) return fail(1, "trackeval_accumulate: negative sequence count");
    if (const int rc = check_dims(max_gt, max_tr, "trackeval_accumulate")) return rc;
    if (n_seqs == 0) { g_err[0] = 0; return 0; }
    if (!sim || !sim_off || !gt_off || !tr_off || !gt_ids || !tr_ids || !seq_off || !n_gt_ids || !n_tr_ids ||
        !cell_off || !gid_off || !tid_off || !potential || !id_matches || !gt_count || !tr_count || !alignment)
        return fail(1, "trackeval_accumulate: null pointer");
    const SeqTables t{n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off};
    const size_t lds = align16((size_t)(max_gt + max_tr) * 8);
    hipLaunchKernelGGL(accumulate_kernel, dim3(n_seqs), dim3(256), lds, (hipStream_t)stream, sim, sim_off, gt_off,
                       tr_off, gt_ids, tr_ids, seq_off, t, max_gt, max_tr, potential, id_matches, gt_count, tr_count,
                       alignment);
    return check_launch("accumulate_kernel");
}

int trackeval_hota_match(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                         const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *frame_seq, int n_frames,
                         const int32_t *n_tr_ids, const int64_t *cell_off, const double *alignment,
                         const double *alphas, int max_gt, int max_tr, int32_t *matches, int32_t *tp, double *loc,
                         int32_t *status, void *stream) {
    if (n_frames < 0) return fail(1, "trackeval_hota_match: negative frame count");
    if (const int rc = check_dims(max_gt, max_tr, "trackeval_hota_match")) return rc;
    if (n_frames == 0) { g_err[0] = 0; return 0; }
    if (!sim || !sim_off || !gt_off || !tr_off || !gt_ids || !tr_ids || !frame_seq || !n_tr_ids || !cell_off ||
        !alignment || !alphas || !matches || !tp || !loc || !status)
        return fail(1, "trackeval_hota_match: null pointer");
    Alphas a;
    for (int i = 0; i < N_ALPHA; ++i) a.v[i] = alphas[i];
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = solve_bytes(max_gt, max_tr);
    if (const int rc = allow_lds(reinterpret_cast<const void *>(hota_match_kernel), lds, allowed,
                                 "trackeval_hota_match"))
        return rc;
    hipLaunchKernelGGL(hota_match_kernel, dim3(n_frames), dim3(64), lds, (hipStream_t)stream, sim, sim_off, gt_off,
                       tr_off, gt_ids, tr_ids, frame_seq, n_tr_ids, cell_off, alignment, a, max_gt, max_tr,
                       max_gt < max_tr ? max_gt : max_tr, matches, tp, loc, status);
    return check_launch("hota_match_kernel");
}

int trackeval_hota_reduce(const int32_t *seq_off, int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids,
                          const int64_t *cell_off, const int32_t *gid_off, const int32_t *tid_off,
                          const int32_t *gt_count, const int32_t *tr_count, const int32_t *matches, const int32_t *tp,
                          const double *loc, int64_t *out_tp, double *out_sums, void *stream) {
    if (n_seqs < 0) return fail(1, "trackeval_hota_reduce: negative sequence count");
    if (n_seqs > 65535) return fail(2, "trackeval_hota_reduce: more than 65535 sequences in one call");
    if (n_seqs == 0) { g_err[0] = 0; return 0; }
    if (!seq_off || !n_gt_ids || !n_tr_ids || !cell_off || !gid_off || !tid_off || !gt_count || !tr_count ||
        !matches || !tp || !loc || !out_tp || !out_sums)
        return fail(1, "trackeval_hota_reduce: null pointer");
    const SeqTables t{n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off};
    hipLaunchKernelGGL(hota_reduce_kernel, dim3(N_ALPHA, n_seqs), dim3(64), 0, (hipStream_t)stream, seq_off, t,
                       gt_count, tr_count, matches, tp, loc, out_tp, out_sums);
    return check_launch("hota_reduce_kernel");
}

int trackeval_clear(const double *sim, const int64_t *sim_off, const int32_t *gt_off, const int32_t *tr_off,
                    const int32_t *gt_ids, const int32_t *tr_ids, const int32_t *seq_off, int n_seqs,
                    const int32_t *n_gt_ids, int max_gt, int max_tr, int max_gt_ids, int32_t *out_ints,
                    double *motp_sum, int32_t *status, void *stream) {
    if (n_seqs < 0) return fail(1, "trackeval_clear: negative sequence count");
    if (const int rc = check_dims(max_gt, max_tr, "trackeval_clear")) return rc;
    if (max_gt_ids < 0) return fail(1, "trackeval_clear: negative id count");
    if (max_gt_ids > TRACKEVAL_MAX_DIM)
        return fail(2, "trackeval_clear: a sequence has more ground-truth ids than TRACKEVAL_MAX_DIM");
    if (n_seqs == 0) { g_err[0] = 0; return 0; }
    if (!sim || !sim_off || !gt_off || !tr_off || !gt_ids || !tr_ids || !seq_off || !n_gt_ids || !out_ints ||
        !motp_sum || !status)
        return fail(1, "trackeval_clear: null pointer");
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = solve_bytes(max_gt, max_tr) + align16((size_t)6 * max_gt_ids * 4);
    if (const int rc = allow_lds(reinterpret_cast<const void *>(clear_kernel), lds, allowed, "trackeval_clear"))
        return rc;
    hipLaunchKernelGGL(clear_kernel, dim3(n_seqs), dim3(64), lds, (hipStream_t)stream, sim, sim_off, gt_off, tr_off,
                       gt_ids, tr_ids, seq_off, n_gt_ids, max_gt, max_tr, max_gt_ids,
                       max_gt < max_tr ? max_gt : max_tr, out_ints, motp_sum, status);
    return check_launch("clear_kernel");
}

int trackeval_identity(int n_seqs, const int32_t *n_gt_ids, const int32_t *n_tr_ids, const int64_t *cell_off,
                       const int32_t *gid_off, const int32_t *tid_off, const int32_t *gt_count,
                       const int32_t *tr_count, const int32_t *id_matches, int max_ids, int64_t *out, int32_t *status,
                       void *stream) {
    if (n_seqs < 0 || max_ids < 0) return fail(1, "trackeval_identity: negative count");
    if (max_ids > TRACKEVAL_MAX_DIM) {
        snprintf(g_err, sizeof(g_err), "trackeval_identity: a sequence with %d ground-truth plus tracker ids exceeds "
                 "TRACKEVAL_MAX_DIM = %d", max_ids, TRACKEVAL_MAX_DIM);
        return 2;
    }
    if (n_seqs == 0) { g_err[0] = 0; return 0; }
    if (!n_gt_ids || !n_tr_ids || !cell_off || !gid_off || !tid_off || !gt_count || !tr_count || !id_matches ||
        !out || !status)
        return fail(1, "trackeval_identity: null pointer");
    const SeqTables t{n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off};
    static std::atomic<unsigned long long> allowed{0};
    const size_t lds = solve_bytes(max_ids, max_ids);
    if (const int rc = allow_lds(reinterpret_cast<const void *>(identity_kernel), lds, allowed, "trackeval_identity"))
        return rc;
    hipLaunchKernelGGL(identity_kernel, dim3(n_seqs), dim3(64), lds, (hipStream_t)stream, t, gt_count, tr_count,
                       id_matches, max_ids, out, status);
    return check_launch("identity_kernel");
}

}  // extern "C"
