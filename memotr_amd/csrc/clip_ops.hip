// clip_ops.hip -- the small-tensor chains of the clip train step as single gfx950 kernels (C ABI: include/clip_ops_hip.h).
//
// Everything here works on a few thousand elements: the cost is the launch, not the arithmetic.  One thread per
// output element, straight-line fp32 code following the reference formulas (operation order kept where it is
// cheap to do so; `#pragma clang fp contract(off)` so that a product rounds before it is added, as in torch's
// separate kernels), fixed-order reductions where a sum is needed.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "../../include/clip_ops_hip.h"
#include "assign_core.h"

namespace {

thread_local char g_err[256] = {0};

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    g_err[0] = 0;
    return 0;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x4_t __attribute__((ext_vector_type(4)));

struct Box {
    float x1, y1, x2, y2;
};

// cxcywh -> xyxy (reference utils/box_ops.py:16-20)
__device__ __forceinline__ Box to_xyxy(float cx, float cy, float w, float h) {
#pragma clang fp contract(off)
    Box b;
    b.x1 = cx - 0.5f * w;
    b.y1 = cy - 0.5f * h;
    b.x2 = cx + 0.5f * w;
    b.y2 = cy + 0.5f * h;
    return b;
}

// generalised IoU of two xyxy boxes (reference utils/box_ops.py:49-70, one pair)
__device__ __forceinline__ float giou_pair(const Box a, const Box b) {
#pragma clang fp contract(off)
    const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.f);
    const float ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.f);
    const float inter = iw * ih;
    const float area_a = (a.x2 - a.x1) * (a.y2 - a.y1);
    const float area_b = (b.x2 - b.x1) * (b.y2 - b.y1);
    const float uni = area_a + area_b - inter;
    const float iou = inter / uni;
    const float hw = fmaxf(fmaxf(a.x2, b.x2) - fminf(a.x1, b.x1), 0.f);
    const float hh = fmaxf(fmaxf(a.y2, b.y2) - fminf(a.y1, b.y1), 0.f);
    const float hull = hw * hh;
    return iou - (hull - uni) / hull;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float powg(float x, float gamma) { return gamma == 2.f ? x * x : powf(x, gamma); }

// ----------------------------------------------------------------------------------------
// matching cost
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void match_cost_kernel(const float *__restrict__ logits, long lsl, long lsq,
                                                        const float *__restrict__ boxes, long bsl, long bsq,
                                                        const int64_t *__restrict__ gt_labels,
                                                        const float *__restrict__ gt_boxes, int n_layers, int Q,
                                                        int K, int T, float w_class, float w_bbox, float w_giou,
                                                        float *__restrict__ cost) {
#pragma clang fp contract(off)
    const long total = (long)n_layers * Q * T;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        const long lq = i / T;
        const int q = (int)(lq % Q), l = (int)(lq / Q);
        long lab = gt_labels[t];
        lab = lab < 0 ? 0 : (lab >= K ? K - 1 : lab);
        const float prob = sigmoidf(logits[l * lsl + q * lsq + lab]);
        const float alpha = 0.25f, gamma = 2.f;
        const float neg = ((1.f - alpha) * powg(prob, gamma)) * (-logf(1.f - prob + 1e-8f));
        const float pos = (alpha * powg(1.f - prob, gamma)) * (-logf(prob + 1e-8f));
        const float c_class = pos - neg;
        const float *pb = boxes + l * bsl + q * bsq;
        const float *tb = gt_boxes + (long)t * 4;
        const float p0 = pb[0], p1 = pb[1], p2 = pb[2], p3 = pb[3];
        const float t0 = tb[0], t1 = tb[1], t2 = tb[2], t3 = tb[3];
        const float c_bbox = ((fabsf(p0 - t0) + fabsf(p1 - t1)) + fabsf(p2 - t2)) + fabsf(p3 - t3);
        const float giou = giou_pair(to_xyxy(p0, p1, p2, p3), to_xyxy(t0, t1, t2, t3));
        cost[i] = (w_bbox * c_bbox + w_class * c_class) + w_giou * (-giou);
    }
}

// ----------------------------------------------------------------------------------------
// paired box losses
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_box_loss_fwd_kernel(const float *__restrict__ boxes,
                                                               const int64_t *__restrict__ lay,
                                                               const int64_t *__restrict__ qidx, long row_mul,
                                                               long row_add, const float *__restrict__ tgt,
                                                               const int64_t *__restrict__ gidx,
                                                               const float *__restrict__ weight, int n,
                                                               float *__restrict__ l1, float *__restrict__ gl) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *pb = boxes + (lay[i] * row_mul + row_add + qidx[i]) * 4;
    const float *tb = tgt + (gidx ? gidx[i] : (long)i) * 4;
    const float p0 = pb[0], p1 = pb[1], p2 = pb[2], p3 = pb[3];
    const float t0 = tb[0], t1 = tb[1], t2 = tb[2], t3 = tb[3];
    float a = ((fabsf(p0 - t0) + fabsf(p1 - t1)) + fabsf(p2 - t2)) + fabsf(p3 - t3);
    float g = 1.f - giou_pair(to_xyxy(p0, p1, p2, p3), to_xyxy(t0, t1, t2, t3));
    if (weight) {
        a *= weight[i];
        g *= weight[i];
    }
    l1[i] = a;
    gl[i] = g;
}

// IoU of two xyxy boxes (reference utils/box_ops.py:23-46, one pair): pair_iou_kernel and the track hand-over share it
__device__ __forceinline__ float iou_pair(const Box a, const Box b) {
#pragma clang fp contract(off)
    const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.f);
    const float ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.f);
    const float inter = iw * ih;
    const float uni = (a.x2 - a.x1) * (a.y2 - a.y1) + (b.x2 - b.x1) * (b.y2 - b.y1) - inter;
    return inter / uni;
}

__global__ __launch_bounds__(256) void pair_iou_kernel(const float *__restrict__ boxes, const float *__restrict__ tgt,
                                                      const int64_t *__restrict__ gidx, int n,
                                                      float *__restrict__ iou) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *pb = boxes + (long)i * 4;
    const float *tb = tgt + (gidx ? gidx[i] : (long)i) * 4;
    iou[i] = iou_pair(to_xyxy(pb[0], pb[1], pb[2], pb[3]), to_xyxy(tb[0], tb[1], tb[2], tb[3]));
}

// ----------------------------------------------------------------------------------------
// track hand-over between two frames (include/clip_ops_hip.h: clipops_handover_*)
// ----------------------------------------------------------------------------------------
// column offsets of the packed row: logits | boxes | ref_pts | output_embed | long_memory | last_output | query_embed | iou
struct HandoverCols {
    int K, C, QW, oB, oR, oO, oM, oS, oQ, oI, W;
};

HandoverCols handover_cols(int K, int C, int use_dab) {
    HandoverCols c;
    c.K = K;
    c.C = C;
    c.QW = use_dab ? C : 2 * C;
    c.oB = K;
    c.oR = K + 4;
    c.oO = K + 8;
    c.oM = c.oO + C;
    c.oS = c.oM + C;
    c.oQ = c.oS + C;
    c.oI = c.oQ + c.QW;
    c.W = c.oI + 1;
    return c;
}

// n consecutive floats by the whole workgroup (column offsets of the packed row are not 16-byte aligned: scalar lanes)
__device__ __forceinline__ void row_copy(float *__restrict__ dst, const float *__restrict__ src, int n) {
    for (int c = threadIdx.x; c < n; c += blockDim.x) dst[c] = src[c];
}
__device__ __forceinline__ void row_sum(float *__restrict__ dst, const float *__restrict__ a,
                                        const float *__restrict__ b, int n) {
    for (int c = threadIdx.x; c < n; c += blockDim.x) dst[c] = a[c] + b[c];
}
__device__ __forceinline__ void row_zero(float *__restrict__ dst, int n) {
    for (int c = threadIdx.x; c < n; c += blockDim.x) dst[c] = 0.f;
}

__global__ __launch_bounds__(256) void handover_fwd_kernel(clipops_handover_sources src,
                                                          const int64_t *__restrict__ prev_ids,
                                                          const int64_t *__restrict__ prev_matched,
                                                          const float *__restrict__ gt_boxes,
                                                          const int64_t *__restrict__ gt_ids,
                                                          const int64_t *__restrict__ table, int n_det, int n_tracks,
                                                          int n_gt, int use_dab, HandoverCols cols,
                                                          float *__restrict__ base, int64_t *__restrict__ ids,
                                                          int64_t *__restrict__ matched_idx) {
    const int o = blockIdx.x;
    const int64_t kind = table[3 * (long)o], s = table[3 * (long)o + 1];
    int64_t g = table[3 * (long)o + 2];
    float *row = base + (long)o * cols.W;
    bool ok;
    if (kind == 0) {
        ok = s >= 0 && s < n_tracks;
        if (ok) {
            g = prev_matched[s];
            ok = g >= -1 && g < n_gt;
        }
    } else {
        ok = (kind == 1 || kind == 2) && s >= 0 && s < n_det && (kind == 2 || (g >= 0 && g < n_gt));
    }
    if (!ok) {                                   // a table row that points nowhere: zeros, no identity
        row_zero(row, cols.W);
        if (threadIdx.x == 0) ids[o] = matched_idx[o] = -1;
        return;
    }
    const long m = kind == 0 ? (long)n_det + s : s;           // row of the model's outputs
#define HO_ROW(i, r) (src.ptr[i] + (r) * src.row_stride[i])
    const float *box = HO_ROW(CLIPOPS_HO_BOXES, m);
    row_copy(row, HO_ROW(CLIPOPS_HO_LOGITS, m), cols.K);
    row_copy(row + cols.oB, box, 4);
    row_copy(row + cols.oO, HO_ROW(CLIPOPS_HO_OUTPUTS, m), cols.C);
    if (kind == 0) {
        row_copy(row + cols.oR, HO_ROW(CLIPOPS_HO_PREV_REF, s), 4);
        row_copy(row + cols.oM, HO_ROW(CLIPOPS_HO_PREV_LONG, s), cols.C);
        row_copy(row + cols.oS, HO_ROW(CLIPOPS_HO_PREV_LAST, s), cols.C);
        row_copy(row + cols.oQ, HO_ROW(CLIPOPS_HO_PREV_QUERY, s), cols.QW);
    } else {
        row_copy(row + cols.oR, HO_ROW(kind == 1 ? CLIPOPS_HO_LAST_REF : CLIPOPS_HO_INIT_REF, s), 4);
        row_copy(row + cols.oM, HO_ROW(CLIPOPS_HO_QUERIES, s), cols.C);
        row_copy(row + cols.oS, HO_ROW(CLIPOPS_HO_OUTPUTS, s), cols.C);
        if (use_dab) {
            row_copy(row + cols.oQ, HO_ROW(CLIPOPS_HO_QUERIES, s), cols.C);
        } else {
            row_copy(row + cols.oQ, HO_ROW(CLIPOPS_HO_DET_EMBED, s), cols.C);
            row_copy(row + cols.oQ + cols.C, HO_ROW(CLIPOPS_HO_QUERIES, s), cols.C);
        }
    }
    if (threadIdx.x == 0) {
        float iou = 0.f;
        int64_t id = -1;
        if (kind == 2) {
            g = -1;
        } else {
            if (g >= 0) {
                const float *tb = gt_boxes + g * 4;
                iou = iou_pair(to_xyxy(box[0], box[1], box[2], box[3]), to_xyxy(tb[0], tb[1], tb[2], tb[3]));
            } else {
                iou = HO_ROW(CLIPOPS_HO_PREV_IOU, s)[0];       // kind 0 only: a track whose ground truth is gone
            }
            id = kind == 0 ? prev_ids[s] : gt_ids[g];
        }
        row[cols.oI] = iou;
        ids[o] = iou < 0.5f ? (int64_t)-1 : id;
        matched_idx[o] = g;
    }
#undef HO_ROW
}

__global__ __launch_bounds__(256) void handover_bwd_kernel(const float *__restrict__ grad_base,
                                                          const int64_t *__restrict__ table,
                                                          const int64_t *__restrict__ inv_q,
                                                          const int64_t *__restrict__ inv_prev, int n_keep, int n_q,
                                                          int n_det, int n_tracks, int use_dab, int det_cols,
                                                          HandoverCols cols, clipops_handover_grads grad) {
    const int C = cols.C;
    if ((int)blockIdx.x < n_q) {                             // a row of the model's outputs
        const long r = blockIdx.x;
        int64_t o = inv_q[r], kind = -1;
        if (o >= 0 && o < n_keep) {
            kind = table[3 * o];
            const int64_t s = table[3 * o + 1];
            const bool back = kind == 0 ? (s >= 0 && s < n_tracks && n_det + s == r)
                                        : ((kind == 1 || kind == 2) && s == r && r < n_det);
            if (!back) kind = -1;
        }
        const float *gr = kind >= 0 ? grad_base + o * cols.W : nullptr;
        float *g_out = grad.ptr[CLIPOPS_HO_OUTPUTS], *g_qry = grad.ptr[CLIPOPS_HO_QUERIES];
        float *g_last = grad.ptr[CLIPOPS_HO_LAST_REF], *g_init = grad.ptr[CLIPOPS_HO_INIT_REF];
        float *g_det = grad.ptr[CLIPOPS_HO_DET_EMBED];
        if (g_out) {
            if (kind == 0) row_copy(g_out + r * C, gr + cols.oO, C);
            else if (kind > 0) row_sum(g_out + r * C, gr + cols.oO, gr + cols.oS, C);
            else row_zero(g_out + r * C, C);
        }
        if (g_qry) {
            if (kind > 0) row_sum(g_qry + r * C, gr + cols.oQ + (use_dab ? 0 : C), gr + cols.oM, C);
            else row_zero(g_qry + r * C, C);
        }
        if (g_last) {
            if (kind == 1) row_copy(g_last + r * 4, gr + cols.oR, 4);
            else row_zero(g_last + r * 4, 4);
        }
        if (g_init) {
            if (kind == 2) row_copy(g_init + r * 4, gr + cols.oR, 4);
            else row_zero(g_init + r * 4, 4);
        }
        if (g_det && !use_dab && r < n_det) {
            if (kind > 0) {
                row_copy(g_det + r * det_cols, gr + cols.oQ, C);
                row_zero(g_det + r * det_cols + C, det_cols - C);
            } else {
                row_zero(g_det + r * det_cols, det_cols);
            }
        }
        return;
    }
    const long j = (long)blockIdx.x - n_q;                   // a row of the previous track set
    if (j >= n_tracks) return;
    int64_t o = inv_prev[j];
    if (!(o >= 0 && o < n_keep && table[3 * o] == 0 && table[3 * o + 1] == j)) o = -1;
    const float *gr = o >= 0 ? grad_base + o * cols.W : nullptr;
    float *g_ref = grad.ptr[CLIPOPS_HO_PREV_REF], *g_long = grad.ptr[CLIPOPS_HO_PREV_LONG];
    float *g_lo = grad.ptr[CLIPOPS_HO_PREV_LAST], *g_qe = grad.ptr[CLIPOPS_HO_PREV_QUERY];
    if (g_ref) { if (gr) row_copy(g_ref + j * 4, gr + cols.oR, 4); else row_zero(g_ref + j * 4, 4); }
    if (g_long) { if (gr) row_copy(g_long + j * C, gr + cols.oM, C); else row_zero(g_long + j * C, C); }
    if (g_lo) { if (gr) row_copy(g_lo + j * C, gr + cols.oS, C); else row_zero(g_lo + j * C, C); }
    if (g_qe) {
        if (gr) row_copy(g_qe + j * cols.QW, gr + cols.oQ, cols.QW);
        else row_zero(g_qe + j * cols.QW, cols.QW);
    }
}

// d max(a,b)/da and d min(a,b)/da with torch's tie rule (half each)
__device__ __forceinline__ float dmax_a(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float dmin_a(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void pair_box_loss_bwd_kernel(const float *__restrict__ boxes,
                                                               const int64_t *__restrict__ lay,
                                                               const int64_t *__restrict__ qidx, long row_mul,
                                                               long row_add, const float *__restrict__ tgt,
                                                               const int64_t *__restrict__ gidx,
                                                               const float *__restrict__ weight, int n,
                                                               const float *__restrict__ g_l1,
                                                               const float *__restrict__ g_gl,
                                                               float *__restrict__ grad_boxes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long row = lay[i] * row_mul + row_add + qidx[i];
    const float *pb = boxes + row * 4;
    const float *tb = tgt + (gidx ? gidx[i] : (long)i) * 4;
    const float p0 = pb[0], p1 = pb[1], p2 = pb[2], p3 = pb[3];
    const float t0 = tb[0], t1 = tb[1], t2 = tb[2], t3 = tb[3];
    const float w = weight ? weight[i] : 1.f;
    const float ga = g_l1[i] * w;         // d/d(l1 sum)
    const float gg = -g_gl[i] * w;        // d/d(giou): the loss is 1 - giou
    const Box a = to_xyxy(p0, p1, p2, p3), b = to_xyxy(t0, t1, t2, t3);
    // forward values
    const float ltx = fmaxf(a.x1, b.x1), lty = fmaxf(a.y1, b.y1), rbx = fminf(a.x2, b.x2), rby = fminf(a.y2, b.y2);
    const float dw = rbx - ltx, dh = rby - lty;
    const float iw = fmaxf(dw, 0.f), ih = fmaxf(dh, 0.f);
    const float inter = iw * ih;
    const float aw = a.x2 - a.x1, ah = a.y2 - a.y1;
    const float area_a = aw * ah, area_b = (b.x2 - b.x1) * (b.y2 - b.y1);
    const float uni = area_a + area_b - inter;
    const float hx1 = fminf(a.x1, b.x1), hy1 = fminf(a.y1, b.y1), hx2 = fmaxf(a.x2, b.x2), hy2 = fmaxf(a.y2, b.y2);
    const float ew = hx2 - hx1, eh = hy2 - hy1;
    const float hw = fmaxf(ew, 0.f), hh = fmaxf(eh, 0.f);
    const float hull = hw * hh;
    // giou = inter/uni - (hull - uni)/hull
    const float g_inter0 = gg / uni;                                          // via iou
    const float g_uni = gg * (-inter / (uni * uni)) + gg / hull;              // via iou and via -(hull-uni)/hull
    const float g_hull = gg * (-(uni / (hull * hull)));                       // d[-(hull-uni)/hull]/d hull = -uni/hull^2
    const float g_inter = g_inter0 - g_uni;                                   // uni = area_a + area_b - inter
    const float g_area_a = g_uni;
    // inter = clamp(dw) * clamp(dh)   (clamp(min=0) passes the gradient where x >= 0)
    const float g_dw = g_inter * ih * (dw >= 0.f ? 1.f : 0.f), g_dh = g_inter * iw * (dh >= 0.f ? 1.f : 0.f);
    const float g_ew = g_hull * hh * (ew >= 0.f ? 1.f : 0.f), g_eh = g_hull * hw * (eh >= 0.f ? 1.f : 0.f);
    // xyxy gradients of box a
    float gx1 = -g_dw * dmax_a(a.x1, b.x1) - g_ew * dmin_a(a.x1, b.x1) - g_area_a * ah;
    float gy1 = -g_dh * dmax_a(a.y1, b.y1) - g_eh * dmin_a(a.y1, b.y1) - g_area_a * aw;
    float gx2 = g_dw * dmin_a(a.x2, b.x2) + g_ew * dmax_a(a.x2, b.x2) + g_area_a * ah;
    float gy2 = g_dh * dmin_a(a.y2, b.y2) + g_eh * dmax_a(a.y2, b.y2) + g_area_a * aw;
    // cxcywh: x1 = cx - w/2, x2 = cx + w/2
    float *go = grad_boxes + row * 4;
    go[0] = (gx1 + gx2) + ga * sgn(p0 - t0);
    go[1] = (gy1 + gy2) + ga * sgn(p1 - t1);
    go[2] = 0.5f * (gx2 - gx1) + ga * sgn(p2 - t2);
    go[3] = 0.5f * (gy2 - gy1) + ga * sgn(p3 - t3);
}

// ----------------------------------------------------------------------------------------
// focal loss of stacked layers
// ----------------------------------------------------------------------------------------
struct Focal {
    float loss, dloss;
};

// one element: logit x, binary target (t == 1 when is_pos)
__device__ __forceinline__ Focal focal_elem(float x, bool is_pos, float alpha, float gamma) {
    const float p = sigmoidf(x);
    // binary_cross_entropy_with_logits: max(x,0) - x*t + log(1 + exp(-|x|))
    const float ce = fmaxf(x, 0.f) - (is_pos ? x : 0.f) + log1pf(expf(-fabsf(x)));
    const float p_t = is_pos ? p : 1.f - p;
    const float q = 1.f - p_t;
    const float a_t = alpha >= 0.f ? (is_pos ? alpha : 1.f - alpha) : 1.f;
    const float mod = powg(q, gamma);
    Focal f;
    f.loss = a_t * (ce * mod);
    // d/dx: -s a_t [gamma q^(gamma-1) (p_t q) ce + q^gamma q],  s = +1 (positive) / -1
    // (gamma == 0: the modulating factor is the constant 1 and has no derivative -- torch's pow backward returns zero
    //  there; q^(gamma-1) would be 1/q, infinite once p_t saturates at 1, and 0 * inf a NaN)
    const float qg1 = gamma == 2.f ? q : (gamma == 0.f ? 0.f : powf(q, gamma - 1.f));
    const float d = a_t * (gamma * qg1 * (p_t * q) * ce + mod * q);
    f.dloss = is_pos ? -d : d;
    return f;
}

__global__ __launch_bounds__(256) void focal_fwd_kernel(const float *__restrict__ logits, long sl, long sq,
                                                       const int64_t *__restrict__ labels, int Nq, int K, float alpha,
                                                       float gamma, float *__restrict__ loss) {
    __shared__ float s_part[256];
    const int l = blockIdx.x;
    const int total = Nq * K;
    float acc = 0.f;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int q = i / K, k = i - q * K;
        const float x = logits[l * sl + q * sq + k];
        acc += focal_elem(x, labels[(long)l * Nq + q] == k, alpha, gamma).loss;
    }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_part[threadIdx.x] += s_part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[l] = s_part[0] / (float)K;      // mean over the classes, sum over the queries
}

__global__ __launch_bounds__(256) void focal_bwd_kernel(const float *__restrict__ logits, long sl, long sq,
                                                       const int64_t *__restrict__ labels, int n_layers, int Nq,
                                                       int K, float alpha, float gamma,
                                                       const float *__restrict__ g_loss,
                                                       float *__restrict__ grad_logits) {
    const long total = (long)n_layers * Nq * K;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const long lq = i / K;
        const int q = (int)(lq % Nq), l = (int)(lq / Nq);
        const float x = logits[l * sl + q * sq + k];
        const Focal f = focal_elem(x, labels[lq] == k, alpha, gamma);
        grad_logits[i] = (g_loss[l] / (float)K) * f.dloss;
    }
}

// ----------------------------------------------------------------------------------------
// decoder glue: sine embedding of the anchors, clamped logit, box refinement
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sine_embed_fwd_kernel(const float *__restrict__ pos,
                                                            const float *__restrict__ dim_t, long n, int K, int F,
                                                            float scale, float *__restrict__ out) {
#pragma clang fp contract(off)
    const long total = n * K * F;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % F);
        const long ik = i / F;                      // = row * K + k
        const float e = (pos[ik] * scale) / dim_t[j];
        out[i] = (j & 1) ? cosf(e) : sinf(e);
    }
}

// one wavefront per (row, coordinate): the F terms of its gradient, summed in a fixed order
__global__ __launch_bounds__(256) void sine_embed_bwd_kernel(const float *__restrict__ pos,
                                                            const float *__restrict__ dim_t, long n, int K, int F,
                                                            float scale, const float *__restrict__ g,
                                                            float *__restrict__ gpos) {
    const int lane = threadIdx.x & 63;
    const long waves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long ik = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; ik < n * K; ik += waves) {
        const float ps = pos[ik] * scale;
        float acc = 0.f;
        for (int j = lane; j < F; j += 64) {
            const float e = ps / dim_t[j];
            const float d = (j & 1) ? -sinf(e) : cosf(e);
            acc += (g[ik * F + j] * d) / dim_t[j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) gpos[ik] = acc * scale;
    }
}

__device__ __forceinline__ float clamp_keep_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ float inv_sigmoid(float x, float eps) {
    return logf(clamp_keep_nan(x, eps, 1.f) / clamp_keep_nan(1.f - x, eps, 1.f));
}

// d inverse_sigmoid / dx with torch's clamp(min, max) masks (the gradient passes where min <= v <= max)
__device__ __forceinline__ float inv_sigmoid_grad(float x, float eps) {
    const float u = 1.f - x;
    const float x1 = clamp_keep_nan(x, eps, 1.f), x2 = clamp_keep_nan(u, eps, 1.f);
    const float a = (x >= eps && x <= 1.f) ? 1.f / x1 : 0.f;
    const float b = (u >= eps && u <= 1.f) ? 1.f / x2 : 0.f;
    return a + b;
}

__global__ __launch_bounds__(256) void inverse_sigmoid_fwd_kernel(const float *__restrict__ x, long n, float eps,
                                                                 float *__restrict__ y) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = inv_sigmoid(x[i], eps);
}

__global__ __launch_bounds__(256) void inverse_sigmoid_bwd_kernel(const float *__restrict__ x,
                                                                 const float *__restrict__ g, long n, float eps,
                                                                 float *__restrict__ gx) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        gx[i] = g[i] * inv_sigmoid_grad(x[i], eps);
}

__global__ __launch_bounds__(256) void refine_boxes_fwd_kernel(const float *__restrict__ delta,
                                                              const float *__restrict__ ref, long n, float eps,
                                                              float *__restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = sigmoidf(delta[i] + inv_sigmoid(ref[i], eps));
}

// Layer 0 of the Deformable-DETR variant (reference models/deformable_decoder.py:141-149 and memotr.py:148-158): the box
// head refines all four coordinates of the 4-d reference, the decoder only xy and takes sigmoid(delta) for wh.  Both boxes
// from one read of `delta`, one thread per row of four; element for element the arithmetic of refine_boxes_fwd_kernel
// (`dec` wh: the same sigmoid with inverse_sigmoid(0.5) == 0 added).  VEC: all four pointers are 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void refine_boxes_split_fwd_kernel(const float *__restrict__ delta,
                                                                    const float *__restrict__ ref, long n_rows,
                                                                    float eps, float *__restrict__ head,
                                                                    float *__restrict__ dec) {
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (long)gridDim.x * blockDim.x) {
        float4 d, f;
        if (VEC) {
            d = reinterpret_cast<const float4 *>(delta)[r];
            f = reinterpret_cast<const float4 *>(ref)[r];
        } else {
            d = make_float4(delta[4 * r], delta[4 * r + 1], delta[4 * r + 2], delta[4 * r + 3]);
            f = make_float4(ref[4 * r], ref[4 * r + 1], ref[4 * r + 2], ref[4 * r + 3]);
        }
        float4 h, c;
        h.x = sigmoidf(d.x + inv_sigmoid(f.x, eps));
        h.y = sigmoidf(d.y + inv_sigmoid(f.y, eps));
        h.z = sigmoidf(d.z + inv_sigmoid(f.z, eps));
        h.w = sigmoidf(d.w + inv_sigmoid(f.w, eps));
        c.x = h.x;
        c.y = h.y;
        c.z = sigmoidf(d.z);
        c.w = sigmoidf(d.w);
        if (VEC) {
            reinterpret_cast<float4 *>(head)[r] = h;
            reinterpret_cast<float4 *>(dec)[r] = c;
        } else {
            head[4 * r] = h.x; head[4 * r + 1] = h.y; head[4 * r + 2] = h.z; head[4 * r + 3] = h.w;
            dec[4 * r] = c.x; dec[4 * r + 1] = c.y; dec[4 * r + 2] = c.z; dec[4 * r + 3] = c.w;
        }
    }
}

__global__ __launch_bounds__(256) void refine_boxes_bwd_kernel(const float *__restrict__ out,
                                                              const float *__restrict__ ref,
                                                              const float *__restrict__ g, long n, float eps,
                                                              float *__restrict__ gdelta, float *__restrict__ gref) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float y = out[i];
        const float gs = (g[i] * (1.f - y)) * y;          // sigmoid backward
        gdelta[i] = gs;
        if (gref) gref[i] = gs * inv_sigmoid_grad(ref[i], eps);
    }
}

// 32 columns x 8 row lanes per workgroup; lane (ty, tx) sums rows ty, ty + 8, ... of column tile tx.
// The sums of all column-sum kernels are kept in fp64 and rounded once: a lane's rows are a strided subset, so an fp32
// partial sum grows to (rows / lanes) * max|x| even where neighbouring rows cancel, and its rounding error with it
// (alternating +-1e4 over 2048 rows: 0.3 absolute against a true sum of ~50).  The kernels are bound by their loads.
__global__ __launch_bounds__(256) void colsum_kernel(const float *__restrict__ x, long rows, int cols,
                                                    float *__restrict__ out) {
    __shared__ double s_part[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (c < cols) {
        long r = ty;
        for (; r + 24 < rows; r += 32) {          // four independent loads in flight
            a0 += x[r * cols + c];
            a1 += x[(r + 8) * cols + c];
            a2 += x[(r + 16) * cols + c];
            a3 += x[(r + 24) * cols + c];
        }
        for (; r < rows; r += 8) a0 += x[r * cols + c];
    }
    s_part[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && c < cols) {
        double t = s_part[0][tx];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += s_part[i][tx];
        out[c] = (float)t;
    }
}

// Short matrices (a few hundred rows) are latency-bound, not bandwidth-bound: one workgroup per FOUR columns, thread t
// takes rows t, t + 256, ... as 16-byte loads (one or two per thread at 310 rows), then a wavefront shuffle reduction
// and one LDS step over the four wavefronts.  6.0 -> ~3 us at 310 x 256 against the 32 x 8 tile above.
__global__ __launch_bounds__(256) void colsum_quad_kernel(const float *__restrict__ x, long rows, int cols,
                                                         float *__restrict__ out) {
    __shared__ f64x4_t s_w[4];
    const int c = blockIdx.x * 4;
    f64x4_t a = {0., 0., 0., 0.};
    for (long r = threadIdx.x; r < rows; r += 256) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(x + r * cols + c);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.x += __shfl_xor(a.x, o, 64);
        a.y += __shfl_xor(a.y, o, 64);
        a.z += __shfl_xor(a.z, o, 64);
        a.w += __shfl_xor(a.w, o, 64);
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const f64x4_t t = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        const f32x4_t r = {(float)t.x, (float)t.y, (float)t.z, (float)t.w};
        *reinterpret_cast<f32x4_t *>(out + c) = r;
    }
}

// the same tile over one chunk of rows per workgroup row (blockIdx.y): partial sums for tall matrices
__device__ __forceinline__ float colsum_ld(const float *x, long i) { return x[i]; }
__device__ __forceinline__ float colsum_ld(const uint16_t *x, long i) {      // bf16 storage, fp32 sums
    return __uint_as_float(((unsigned)x[i]) << 16);
}

template <typename TX>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const TX *__restrict__ x, long rows, int cols,
                                                            int chunk_rows, float *__restrict__ partial) {
    __shared__ double s_part[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    const long r0 = (long)blockIdx.y * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (c < cols) {
        long r = r0 + ty;
        for (; r + 24 < r1; r += 32) {
            a0 += colsum_ld(x, r * cols + c);
            a1 += colsum_ld(x, (r + 8) * cols + c);
            a2 += colsum_ld(x, (r + 16) * cols + c);
            a3 += colsum_ld(x, (r + 24) * cols + c);
        }
        for (; r < r1; r += 8) a0 += colsum_ld(x, r * cols + c);
    }
    s_part[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && c < cols) {
        double t = s_part[0][tx];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += s_part[i][tx];
        partial[(long)blockIdx.y * cols + c] = (float)t;
    }
}

// The ReLU mask of a fused-ReLU Linear's backward and the first pass of its bias gradient in ONE pass over the
// gradient: g2 = y > 0 ? g : 0 is written and summed per (32-column tile, row chunk) on the way.  For the encoder
// FFN's first linear (111,615 x 2048 floats per layer of a 5-frame clip) the separate column sum re-read 914 MB.
__device__ __forceinline__ void colsum_st(float *x, long i, float v) { x[i] = v; }

template <typename TX>
__global__ __launch_bounds__(256) void relu_bwd_colsum_partial_kernel(const TX *__restrict__ g, const TX *__restrict__ y,
                                                                     long rows, int cols, int chunk_rows,
                                                                     TX *__restrict__ g2, float *__restrict__ partial) {
    __shared__ double s_part[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    const long r0 = (long)blockIdx.y * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (c < cols) {
        long r = r0 + ty;
        for (; r + 24 < r1; r += 32) {
            const long i0 = r * cols + c, i1 = (r + 8) * cols + c, i2 = (r + 16) * cols + c, i3 = (r + 24) * cols + c;
            const float v0 = colsum_ld(y, i0) <= 0.f ? 0.f : colsum_ld(g, i0);
            const float v1 = colsum_ld(y, i1) <= 0.f ? 0.f : colsum_ld(g, i1);
            const float v2 = colsum_ld(y, i2) <= 0.f ? 0.f : colsum_ld(g, i2);
            const float v3 = colsum_ld(y, i3) <= 0.f ? 0.f : colsum_ld(g, i3);
            colsum_st(g2, i0, v0); colsum_st(g2, i1, v1); colsum_st(g2, i2, v2); colsum_st(g2, i3, v3);
            a0 += v0; a1 += v1; a2 += v2; a3 += v3;
        }
        for (; r < r1; r += 8) {
            const long i0 = r * cols + c;
            const float v0 = colsum_ld(y, i0) <= 0.f ? 0.f : colsum_ld(g, i0);
            colsum_st(g2, i0, v0);
            a0 += v0;
        }
    }
    s_part[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && c < cols) {
        double t = s_part[0][tx];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += s_part[i][tx];
        partial[(long)blockIdx.y * cols + c] = (float)t;
    }
}

// ----------------------------------------------------------------------------------------
// multi-head self-attention over the decoder queries (head_dim 32, L <= 512): forward and backward
// ----------------------------------------------------------------------------------------
// One workgroup = kRows rows x kLanes lanes (256 threads) of one (batch, head).  A lane of a row visits the rows of
// the OTHER axis j = lane, lane + kLanes, ... : 32-float dot products against rows staged in LDS (pitch 36 floats: the
// sixteen lanes of a row cover all 64 banks exactly once per ds_read_b128, the four rows of a wavefront read the same
// addresses = broadcast).  16 lanes per row: a decoder call is only ~2,500 rows x 320 keys, so the per-lane chain
// (20 keys) sets the kernel's latency, not throughput.
constexpr int kLanes = 16;         // lanes per row
constexpr int kRows = 256 / kLanes;  // rows per workgroup
constexpr int kHd = 32;            // head dimension
constexpr int kPitch = 36;         // LDS row pitch in floats

__device__ __forceinline__ void load_row32(const float *p, float *r) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(p + 4 * i);
        r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
}

__device__ __forceinline__ float dot32(const float *a, const float *lds_row) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(lds_row + 4 * i);
        s0 = fmaf(a[4 * i], v.x, s0);
        s1 = fmaf(a[4 * i + 1], v.y, s1);
        s0 = fmaf(a[4 * i + 2], v.z, s0);
        s1 = fmaf(a[4 * i + 3], v.w, s1);
    }
    return s0 + s1;
}

// the same sum from two register rows.  D = dO . O of the backward uses the association of dot32 on purpose: where a
// row attends to ONE key (L = 1, a single live key) O is that key's V bit for bit, and dO . V_j - D must be exactly zero
__device__ __forceinline__ float dot32r(const float *a, const float *b) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s0 = fmaf(a[4 * i], b[4 * i], s0);
        s1 = fmaf(a[4 * i + 1], b[4 * i + 1], s1);
        s0 = fmaf(a[4 * i + 2], b[4 * i + 2], s0);
        s1 = fmaf(a[4 * i + 3], b[4 * i + 3], s1);
    }
    return s0 + s1;
}

__device__ __forceinline__ void axpy32(float *acc, float w, const float *lds_row) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(lds_row + 4 * i);
        acc[4 * i] = fmaf(w, v.x, acc[4 * i]);
        acc[4 * i + 1] = fmaf(w, v.y, acc[4 * i + 1]);
        acc[4 * i + 2] = fmaf(w, v.z, acc[4 * i + 2]);
        acc[4 * i + 3] = fmaf(w, v.w, acc[4 * i + 3]);
    }
}

// sum / max over the kLanes lanes of a row (they differ in the low bits of the lane id)
__device__ __forceinline__ float sum8l(float x) {
#pragma unroll
    for (int o = 1; o < kLanes; o <<= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ float max8l(float x) {
#pragma unroll
    for (int o = 1; o < kLanes; o <<= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}

// cooperative copy of L rows (32 floats each, `rs` apart) into LDS at pitch kPitch
__device__ __forceinline__ void stage_rows(float *dst, const float *src, long rs, int L) {
    for (int i = threadIdx.x; i < L * 8; i += blockDim.x) {
        const int r = i >> 3, c = (i & 7) * 4;
        *reinterpret_cast<f32x4_t *>(dst + r * kPitch + c) = *reinterpret_cast<const f32x4_t *>(src + r * rs + c);
    }
}

__global__ __launch_bounds__(256) void mha_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                     const float *__restrict__ v, long q_bs, long q_rs, long k_bs,
                                                     long k_rs, long v_bs, long v_rs,
                                                     const uint8_t *__restrict__ key_mask, int H, int L, float scale,
                                                     float *__restrict__ out, float *__restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float *Ks = s_mem, *Vs = s_mem + (size_t)L * kPitch;
    const int h = blockIdx.y, b = blockIdx.z;
    stage_rows(Ks, k + b * k_bs + h * kHd, k_rs, L);
    stage_rows(Vs, v + b * v_bs + h * kHd, v_rs, L);
    __syncthreads();
    const int row = blockIdx.x * kRows + threadIdx.x / kLanes, sub = threadIdx.x % kLanes;
    const bool row_ok = row < L;
    const int rowc = row_ok ? row : L - 1;
    float qr[kHd];
    load_row32(q + b * q_bs + rowc * q_rs + h * kHd, qr);
#pragma unroll
    for (int i = 0; i < kHd; ++i) qr[i] *= scale;
    const uint8_t *mk = key_mask ? key_mask + (long)b * L : nullptr;
    float m = -INFINITY, l = 0.f, acc[kHd];
#pragma unroll
    for (int i = 0; i < kHd; ++i) acc[i] = 0.f;
    for (int j = sub; j < L; j += kLanes) {
        if (mk && mk[j]) continue;
        const float s = dot32(qr, Ks + j * kPitch);
        const float m_new = fmaxf(m, s);
        const float corr = expf(m - m_new), p = expf(s - m_new);      // exp(-inf) = 0 on the first key
        l = l * corr + p;
#pragma unroll
        for (int i = 0; i < kHd; ++i) acc[i] *= corr;
        axpy32(acc, p, Vs + j * kPitch);
        m = m_new;
    }
    // merge the lanes of the row
    const float M = max8l(m);
    const float w = (m == -INFINITY) ? 0.f : expf(m - M);          // a lane may have seen no key at all
    const float Lsum = sum8l(l * w);
    const float inv = 1.f / Lsum;
    float *o = out + ((long)b * L + rowc) * (H * kHd) + h * kHd;
#pragma unroll
    for (int i = 0; i < kHd; ++i) {
        const float t = sum8l(acc[i] * w) * inv;
        if (row_ok && (i >> 2) == sub) o[i] = t;                   // lane `sub` stores floats 4*sub .. 4*sub+3
    }
    if (row_ok && sub == 0) lse[((long)b * H + h) * L + row] = M + logf(Lsum);
}

// grad_q: same decomposition as the forward (a workgroup = kRows query rows; K and V of the head in LDS)
__global__ __launch_bounds__(256) void mha_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                       const float *__restrict__ v, long q_bs, long q_rs, long k_bs,
                                                       long k_rs, long v_bs, long v_rs,
                                                       const uint8_t *__restrict__ key_mask,
                                                       const float *__restrict__ out, const float *__restrict__ lse,
                                                       const float *__restrict__ go, int H, int L, float scale,
                                                       float *__restrict__ gq, long gq_bs, long gq_rs) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float *Ks = s_mem, *Vs = s_mem + (size_t)L * kPitch;
    const int h = blockIdx.y, b = blockIdx.z;
    stage_rows(Ks, k + b * k_bs + h * kHd, k_rs, L);
    stage_rows(Vs, v + b * v_bs + h * kHd, v_rs, L);
    __syncthreads();
    const int row = blockIdx.x * kRows + threadIdx.x / kLanes, sub = threadIdx.x % kLanes;
    const bool row_ok = row < L;
    const int rowc = row_ok ? row : L - 1;
    float qr[kHd], gr[kHd], acc[kHd];
    load_row32(q + b * q_bs + rowc * q_rs + h * kHd, qr);
    const long orow = ((long)b * L + rowc) * (H * kHd) + h * kHd;
    load_row32(go + orow, gr);
    float D = 0.f;                                                  // rowsum(dP o P) = dO . O
    {
        float orr[kHd];
        load_row32(out + orow, orr);
        D = dot32r(gr, orr);
    }
#pragma unroll
    for (int i = 0; i < kHd; ++i) { qr[i] *= scale; acc[i] = 0.f; }
    const float ls = lse[((long)b * H + h) * L + rowc];
    const uint8_t *mk = key_mask ? key_mask + (long)b * L : nullptr;
    for (int j = sub; j < L; j += kLanes) {
        if (mk && mk[j]) continue;
        const float p = expf(dot32(qr, Ks + j * kPitch) - ls);
        const float ds = p * (dot32(gr, Vs + j * kPitch) - D);
        axpy32(acc, ds, Ks + j * kPitch);
    }
    float *g = gq + b * gq_bs + rowc * gq_rs + h * kHd;
#pragma unroll
    for (int i = 0; i < kHd; ++i) {
        const float t = sum8l(acc[i]) * scale;
        if (row_ok && (i >> 2) == sub) g[i] = t;
    }
}

// grad_k, grad_v: a workgroup = kRows KEY rows; Q and dO of the head in LDS, lse and D = dO . O per query too
__global__ __launch_bounds__(256) void mha_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                        const float *__restrict__ v, long q_bs, long q_rs, long k_bs,
                                                        long k_rs, long v_bs, long v_rs,
                                                        const uint8_t *__restrict__ key_mask,
                                                        const float *__restrict__ out, const float *__restrict__ lse,
                                                        const float *__restrict__ go, int H, int L, float scale,
                                                        float *__restrict__ gk, long gk_bs, long gk_rs,
                                                        float *__restrict__ gv, long gv_bs, long gv_rs) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float *Qs = s_mem, *Gs = s_mem + (size_t)L * kPitch;
    float *s_lse = Gs + (size_t)L * kPitch, *s_D = s_lse + L;
    const int h = blockIdx.y, b = blockIdx.z;
    stage_rows(Qs, q + b * q_bs + h * kHd, q_rs, L);
    // Q is kept SCALED, as the forward and grad_q hold it: (q * scale) . k is then the forward's score bit for bit and
    // exp(s - lse) the forward's probability (scaling k instead moved s by an ulp: p = 1 +- 5e-7 where it is exactly 1).
    // Each thread scales the float4s it staged itself, so no barrier is needed in between.
    for (int i = threadIdx.x; i < L * 8; i += blockDim.x) {
        f32x4_t *p4 = reinterpret_cast<f32x4_t *>(Qs + (i >> 3) * kPitch + (i & 7) * 4);
        *p4 = *p4 * scale;
    }
    stage_rows(Gs, go + (long)b * L * (H * kHd) + h * kHd, (long)H * kHd, L);
    for (int i = threadIdx.x; i < L; i += blockDim.x) s_lse[i] = lse[((long)b * H + h) * L + i];
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += blockDim.x) {             // D_i = dO_i . O_i
        const float *o = out + ((long)b * L + i) * (H * kHd) + h * kHd;
        float orr[kHd];
        load_row32(o, orr);
        s_D[i] = dot32(orr, Gs + i * kPitch);
    }
    __syncthreads();
    const int row = blockIdx.x * kRows + threadIdx.x / kLanes, sub = threadIdx.x % kLanes;
    const bool row_ok = row < L;
    const int rowc = row_ok ? row : L - 1;
    const bool dead = key_mask && key_mask[(long)b * L + rowc];     // a masked key receives no gradient
    float kr[kHd], vr[kHd], ak[kHd], av[kHd];
    load_row32(k + b * k_bs + rowc * k_rs + h * kHd, kr);
    load_row32(v + b * v_bs + rowc * v_rs + h * kHd, vr);
#pragma unroll
    for (int i = 0; i < kHd; ++i) { ak[i] = 0.f; av[i] = 0.f; }
    if (!dead) {
        for (int i = sub; i < L; i += kLanes) {
            const float p = expf(dot32(kr, Qs + i * kPitch) - s_lse[i]);
            const float ds = p * (dot32(vr, Gs + i * kPitch) - s_D[i]);
            axpy32(av, p, Gs + i * kPitch);
            axpy32(ak, ds, Qs + i * kPitch);
        }
    }
    float *pk = gk + b * gk_bs + rowc * gk_rs + h * kHd, *pv = gv + b * gv_bs + rowc * gv_rs + h * kHd;
#pragma unroll
    for (int i = 0; i < kHd; ++i) {
        const float tk = sum8l(ak[i]), tv = sum8l(av[i]);           // (ak sums ds * (q * scale) already)
        if (row_ok && (i >> 2) == sub) {
            pk[i] = tk;
            pv[i] = tv;
        }
    }
}

// dynamic LDS above 64 KiB has to be allowed once per kernel and device (one bit per device ordinal in `done`)
int allow_lds(const void *kernel, size_t lds, std::atomic<unsigned long long> &done) {
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "hipFuncSetAttribute: %s", hipGetErrorString(e));
        return (int)e;
    }
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

std::atomic<unsigned long long> g_lds_fwd{0}, g_lds_bq{0}, g_lds_bkv{0};

int mha_check(const void *q, const void *k, const void *v, int B, int H, int L) {
    if (B < 0 || H <= 0 || L < 0) return fail(1, "clipops_mha: bad dimension");
    if (L > CLIPOPS_MHA_MAX_L) return fail(2, "clipops_mha: L exceeds CLIPOPS_MHA_MAX_L");
    if ((long)B * L > 0 && (!q || !k || !v)) return fail(1, "clipops_mha: null pointer");
    return 0;
}

// ----------------------------------------------------------------------------------------
// residual add + LayerNorm over rows of 256 floats: one wavefront per row, 4 floats per lane
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum64(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// WITH_Q (ABI 11): q = y + pos is written in the same pass from the y still in registers -- the next encoder layer's
// query, which was a torch add (read 2, write 1 tensor) right after this kernel.  y is the same expression either way.
template <bool WITH_Q>
__global__ __launch_bounds__(256) void add_layer_norm_fwd_kernel(const float *__restrict__ x,
                                                                const float *__restrict__ res,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ beta,
                                                                const float *__restrict__ pos, long rows, float eps,
                                                                float *__restrict__ sum, float *__restrict__ y,
                                                                float *__restrict__ q, float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long off = row * CLIPOPS_LN_COLS + lane * 4;
    const f32x4_t a = *reinterpret_cast<const f32x4_t *>(x + off);
    const f32x4_t b = *reinterpret_cast<const f32x4_t *>(res + off);
    const f32x4_t s = a + b;
    *reinterpret_cast<f32x4_t *>(sum + off) = s;
    const float mean = wave_sum64((s.x + s.y) + (s.z + s.w)) * (1.f / CLIPOPS_LN_COLS);
    const f32x4_t d = s - mean;
    const float var = wave_sum64((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * (1.f / CLIPOPS_LN_COLS);
    const float rstd = rsqrtf(var + eps);
    const f32x4_t g = *reinterpret_cast<const f32x4_t *>(gamma + lane * 4);
    const f32x4_t be = *reinterpret_cast<const f32x4_t *>(beta + lane * 4);
    const f32x4_t yv = (d * rstd) * g + be;
    *reinterpret_cast<f32x4_t *>(y + off) = yv;
    if (WITH_Q) *reinterpret_cast<f32x4_t *>(q + off) = yv + *reinterpret_cast<const f32x4_t *>(pos + off);
    if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
}

// a workgroup walks chunk_rows rows (4 at a time, one per wavefront) and keeps the column sums of its rows
__global__ __launch_bounds__(256) void add_layer_norm_bwd_kernel(const float *__restrict__ gy,
                                                                const float *__restrict__ sum,
                                                                const float *__restrict__ stats,
                                                                const float *__restrict__ gamma, long rows,
                                                                int chunk_rows, float *__restrict__ gsum,
                                                                float *__restrict__ partial) {
    __shared__ f32x4_t s_acc[4][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4_t gm = *reinterpret_cast<const f32x4_t *>(gamma + lane * 4);
    f32x4_t acc_g = {0.f, 0.f, 0.f, 0.f}, acc_b = {0.f, 0.f, 0.f, 0.f};
    const long r0 = (long)blockIdx.x * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    for (long row = r0 + wave; row < r1; row += 4) {
        const long off = row * CLIPOPS_LN_COLS + lane * 4;
        const f32x4_t g = *reinterpret_cast<const f32x4_t *>(gy + off);
        const f32x4_t s = *reinterpret_cast<const f32x4_t *>(sum + off);
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        const f32x4_t xh = (s - mean) * rstd;
        const f32x4_t gh = g * gm;
        const float c1 = wave_sum64((gh.x + gh.y) + (gh.z + gh.w)) * (1.f / CLIPOPS_LN_COLS);
        const float c2 = wave_sum64((gh.x * xh.x + gh.y * xh.y) + (gh.z * xh.z + gh.w * xh.w)) * (1.f / CLIPOPS_LN_COLS);
        *reinterpret_cast<f32x4_t *>(gsum + off) = (gh - c1 - xh * c2) * rstd;
        acc_g += g * xh;
        acc_b += g;
    }
    s_acc[wave][0][lane] = acc_g;
    s_acc[wave][1][lane] = acc_b;
    __syncthreads();
    if (wave < 2) {                       // wave 0: gamma part, wave 1: beta part
        const f32x4_t t = (s_acc[0][wave][lane] + s_acc[1][wave][lane]) + (s_acc[2][wave][lane] + s_acc[3][wave][lane]);
        *reinterpret_cast<f32x4_t *>(partial + (long)blockIdx.x * 2 * CLIPOPS_LN_COLS + wave * CLIPOPS_LN_COLS + lane * 4) = t;
    }
}

// The same backward for a LayerNorm whose output has up to three consumers (ABI 11): the incoming gradient is
// (ga + gb) + gc, summed in registers (gb / gc may be null: skipped) and never written out, and the column sums of
// grad_sum -- the bias gradient of the Linear that produced `res` -- ride along.  Those are kept in fp64 like every
// column sum here and leave the workgroup as a float pair (hi, lo = the rounding remainder) in rows 2 * chunk and
// 2 * chunk + 1 of `zpartial`: the finishing colsum adds both in fp64, so a chunk's sum is not rounded to fp32 on the way.
__global__ __launch_bounds__(256) void add_layer_norm_bwd_fanin_kernel(const float *__restrict__ ga,
                                                                      const float *__restrict__ gb,
                                                                      const float *__restrict__ gc,
                                                                      const float *__restrict__ sum,
                                                                      const float *__restrict__ stats,
                                                                      const float *__restrict__ gamma, long rows,
                                                                      int chunk_rows, float *__restrict__ gsum,
                                                                      float *__restrict__ partial,
                                                                      float *__restrict__ zpartial) {
    __shared__ f32x4_t s_acc[4][2][64];
    __shared__ f64x4_t s_z[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4_t gm = *reinterpret_cast<const f32x4_t *>(gamma + lane * 4);
    f32x4_t acc_g = {0.f, 0.f, 0.f, 0.f}, acc_b = {0.f, 0.f, 0.f, 0.f};
    f64x4_t acc_z = {0., 0., 0., 0.};
    const long r0 = (long)blockIdx.x * chunk_rows;
    const long r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    for (long row = r0 + wave; row < r1; row += 4) {
        const long off = row * CLIPOPS_LN_COLS + lane * 4;
        f32x4_t g = *reinterpret_cast<const f32x4_t *>(ga + off);
        if (gb) g += *reinterpret_cast<const f32x4_t *>(gb + off);
        if (gc) g += *reinterpret_cast<const f32x4_t *>(gc + off);
        const f32x4_t s = *reinterpret_cast<const f32x4_t *>(sum + off);
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        const f32x4_t xh = (s - mean) * rstd;
        const f32x4_t gh = g * gm;
        const float c1 = wave_sum64((gh.x + gh.y) + (gh.z + gh.w)) * (1.f / CLIPOPS_LN_COLS);
        const float c2 = wave_sum64((gh.x * xh.x + gh.y * xh.y) + (gh.z * xh.z + gh.w * xh.w)) * (1.f / CLIPOPS_LN_COLS);
        const f32x4_t dz = (gh - c1 - xh * c2) * rstd;
        *reinterpret_cast<f32x4_t *>(gsum + off) = dz;
        acc_g += g * xh;
        acc_b += g;
        acc_z.x += dz.x; acc_z.y += dz.y; acc_z.z += dz.z; acc_z.w += dz.w;
    }
    s_acc[wave][0][lane] = acc_g;
    s_acc[wave][1][lane] = acc_b;
    s_z[wave][lane] = acc_z;
    __syncthreads();
    if (wave < 2) {                       // wave 0: gamma part, wave 1: beta part
        const f32x4_t t = (s_acc[0][wave][lane] + s_acc[1][wave][lane]) + (s_acc[2][wave][lane] + s_acc[3][wave][lane]);
        *reinterpret_cast<f32x4_t *>(partial + (long)blockIdx.x * 2 * CLIPOPS_LN_COLS + wave * CLIPOPS_LN_COLS + lane * 4) = t;
    } else if (wave == 2) {               // wave 2: the column sums of grad_sum
        const f64x4_t t = (s_z[0][lane] + s_z[1][lane]) + (s_z[2][lane] + s_z[3][lane]);
        const f32x4_t hi = {(float)t.x, (float)t.y, (float)t.z, (float)t.w};
        const f32x4_t lo = {(float)(t.x - (double)hi.x), (float)(t.y - (double)hi.y), (float)(t.z - (double)hi.z),
                            (float)(t.w - (double)hi.w)};
        float *zp = zpartial + (long)blockIdx.x * 2 * CLIPOPS_LN_COLS + lane * 4;
        *reinterpret_cast<f32x4_t *>(zp) = hi;
        *reinterpret_cast<f32x4_t *>(zp + CLIPOPS_LN_COLS) = lo;
    }
}

// ---- linear sum assignment on the device (assign_core.h; one wavefront per problem) ----------------------------
// (assign::WaveLanes, the wavefront's side of the solver, lives with it in assign_core.h)
using assign::WaveLanes;

__global__ __launch_bounds__(64) void assign_kernel(const float *__restrict__ cost, long stride_p, long stride_r,
                                                    long stride_c, int n_rows, int n_cols,
                                                    int32_t *__restrict__ row_ind, int32_t *__restrict__ col_ind,
                                                    int32_t *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_assign[];
    const long p = blockIdx.x;
    const int k = n_rows < n_cols ? n_rows : n_cols;
    const WaveLanes lanes{(int)threadIdx.x};
    const int rc = assign::solve_problem(lanes, cost + p * stride_p, stride_r, stride_c, n_rows, n_cols, s_assign,
                                         row_ind + p * k, col_ind + p * k);
    if (threadIdx.x == 0 && status != nullptr) status[p] = rc;
}

int grid_for(long total) {
    long g = (total + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g > 4096 ? 4096 : g);
}


// ---------------------------------------------------------------------------------------------------------------
// Frozen-BN shift + (residual) + ReLU of a ResNet bottleneck in ONE pass over the convolution's output, in place.
// The backbone (reference models/backbone.py:70-76: torchvision's resnet50 with FrozenBatchNorm2d) does this as three
// element-wise passes over activations of up to 344 MB each (5 frames x 256 x 200 x 336): conv bias, `out += identity`,
// ReLU.  NCHW: one (image, channel) plane per blockIdx.y, so the shift is a scalar of the block.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sr_bf16(uint16_t h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ uint16_t sr_to_bf16(float f) {          // round to nearest even (NaN stays NaN)
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <bool RES>
__global__ __launch_bounds__(256) void shift_relu_f32_kernel(float *__restrict__ x, const float *__restrict__ shift,
                                                             const float *__restrict__ res, long planes, int C, long HW,
                                                             int vec) {
    for (long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const float b = shift[plane % C];
        float *xp = x + plane * HW;
        const float *rp = RES ? res + plane * HW : nullptr;
        if (vec) {
            const long n4 = HW >> 2;
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
                float4 v = reinterpret_cast<float4 *>(xp)[i];
                if (RES) {
                    const float4 r = reinterpret_cast<const float4 *>(rp)[i];
                    v.x = (v.x + b) + r.x; v.y = (v.y + b) + r.y; v.z = (v.z + b) + r.z; v.w = (v.w + b) + r.w;
                } else {
                    v.x += b; v.y += b; v.z += b; v.w += b;
                }
                // (max(v, 0) would turn NaN into 0; torch's relu keeps it: v < 0 ? 0 : v)
                v.x = v.x < 0.f ? 0.f : v.x; v.y = v.y < 0.f ? 0.f : v.y;
                v.z = v.z < 0.f ? 0.f : v.z; v.w = v.w < 0.f ? 0.f : v.w;
                reinterpret_cast<float4 *>(xp)[i] = v;
            }
        } else {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (long)gridDim.x * blockDim.x) {
                float v = xp[i] + b;
                if (RES) v += rp[i];
                xp[i] = v < 0.f ? 0.f : v;
            }
        }
    }
}

// bf16 storage (the autocast step): the bias add and the residual add round to bf16 one after the other, like the two
// torch kernels they replace
template <bool RES>
__global__ __launch_bounds__(256) void shift_relu_bf16_kernel(uint16_t *__restrict__ x, const float *__restrict__ shift,
                                                              const uint16_t *__restrict__ res, long planes, int C,
                                                              long HW, int vec) {
    for (long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const float b = sr_bf16(sr_to_bf16(shift[plane % C]));          // autocast hands the convolution a bf16 bias
        uint16_t *xp = x + plane * HW;
        const uint16_t *rp = RES ? res + plane * HW : nullptr;
        if (vec) {
            const long n8 = HW >> 3;
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
                uint4 v = reinterpret_cast<uint4 *>(xp)[i];
                uint4 r = {0u, 0u, 0u, 0u};
                if (RES) r = reinterpret_cast<const uint4 *>(rp)[i];
                unsigned *vw = reinterpret_cast<unsigned *>(&v);
                const unsigned *rw = reinterpret_cast<const unsigned *>(&r);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float lo = sr_bf16((uint16_t)(vw[k] & 0xffffu)) + b, hi = sr_bf16((uint16_t)(vw[k] >> 16)) + b;
                    if (RES) {
                        lo = sr_bf16(sr_to_bf16(lo)) + sr_bf16((uint16_t)(rw[k] & 0xffffu));
                        hi = sr_bf16(sr_to_bf16(hi)) + sr_bf16((uint16_t)(rw[k] >> 16));
                    }
                    lo = lo < 0.f ? 0.f : lo;
                    hi = hi < 0.f ? 0.f : hi;
                    vw[k] = (unsigned)sr_to_bf16(lo) | ((unsigned)sr_to_bf16(hi) << 16);
                }
                reinterpret_cast<uint4 *>(xp)[i] = v;
            }
        } else {
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (long)gridDim.x * blockDim.x) {
                float v = sr_bf16(xp[i]) + b;
                if (RES) v = sr_bf16(sr_to_bf16(v)) + sr_bf16(rp[i]);
                xp[i] = sr_to_bf16(v < 0.f ? 0.f : v);
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------
// Backward of a query-sized Linear (a few hundred rows) in ONE launch: grad_x = G' W, grad_w = G'^T X, grad_b = colsum G',
// G' = grad_y (masked by y > 0 when the forward fused a ReLU).  torch issues [threshold_backward,] two GEMMs and a
// reduction -- four dependent launches of ~5 us each inside the decoder's hipGraphs for ~0.1 GFLOP; the three results
// depend on the same inputs only, so they are tiles of one grid here.
//   * one 32 x 32 output tile per workgroup, fp32 MFMA 32x32x2 (bit-for-bit a k-ordered fmaf chain), the contraction
//     split over the four wavefronts and added up through LDS;
//   * lane l feeds A[i = l & 31][k] and B[k][j = l & 31] for k = 8 c + 4 (l >> 5) + {0..3}: four MFMAs per 8 k;
//   * operands straight from global memory (the whole problem sits in L2), zero-filled past the edges.
// ---------------------------------------------------------------------------------------------------------------
typedef float lb_f32x16 __attribute__((ext_vector_type(16)));

// One workgroup's tile.  GX: C = G' W (A rows are rows of G: one 16-byte load per lane and chunk when OUT % 4 == 0);
// else C = G'^T X (A columns are rows of G: coalesced dwords).  LB_U chunks of 8 k are requested before the first MFMA
// of the group -- without that every chunk waits a memory round trip and the kernel takes 40 us at K = 1024.
#ifndef MSDA_LB_U
#define MSDA_LB_U 4
#endif
constexpr int LB_U = MSDA_LB_U;

template <bool GX, bool RELU>
__device__ __forceinline__ void linear_bwd_tile(const float *__restrict__ g, const float *__restrict__ y,
                                                const float *__restrict__ Bp, int M, int N, int K, int OUT, int i0, int j0,
                                                float *__restrict__ C, float *__restrict__ gb, float (*s_c)[16][64],
                                                float (*s_b)[32]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = i0 + (lane & 31), j = j0 + (lane & 31), kq = (lane >> 5) * 4;
    const bool iok = i < M, jok = j < N;
    const int chunks = (K + 7) / 8, per = (chunks + 3) / 4;
    const int c_lo = wave * per, c_hi = (c_lo + per) < chunks ? (c_lo + per) : chunks;
    const bool vec = GX && (OUT % 4 == 0);
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int c = c_lo; c < c_hi; c += LB_U) {
        float a[LB_U][4], b[LB_U][4], m[LB_U][4];
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            const int k0 = (c + u) * 8 + kq;
            const bool cok = c + u < c_hi;
            if (vec) {
                float4 av = {0.f, 0.f, 0.f, 0.f}, mv = {1.f, 1.f, 1.f, 1.f};
                if (cok && iok && k0 < K) {          // (K = OUT is a multiple of 4 and k0 one too: all four or none)
                    av = *reinterpret_cast<const float4 *>(g + (long)i * OUT + k0);
                    if (RELU) mv = *reinterpret_cast<const float4 *>(y + (long)i * OUT + k0);
                }
                a[u][0] = av.x; a[u][1] = av.y; a[u][2] = av.z; a[u][3] = av.w;
                m[u][0] = mv.x; m[u][1] = mv.y; m[u][2] = mv.z; m[u][3] = mv.w;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + q;
                const bool kok = cok && k < K;
                if (!vec) {
                    const long idx = GX ? (long)i * OUT + k : (long)k * OUT + i;
                    a[u][q] = (iok && kok) ? g[idx] : 0.f;
                    m[u][q] = (RELU && iok && kok) ? y[idx] : 1.f;
                }
                b[u][q] = (jok && kok) ? Bp[(long)k * N + j] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float av = RELU ? (m[u][q] <= 0.f ? 0.f : a[u][q]) : a[u][q];      // (y <= 0 ? 0 : g -- aten's threshold_backward: a NaN activation passes g)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][q], acc, 0, 0, 0);
                bsum += av;
            }
        }
    }
    // add the four partial tiles (and bias sums) up; wavefront v finishes accumulator registers 4v .. 4v + 3
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    bsum += __shfl_xor(bsum, 32, 64);
    if (lane < 32) s_b[wave][lane] = bsum;
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const float v = (s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane]);
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M && jok) C[(long)row * N + j] = v;
    }
    if (!GX && gb != nullptr && j0 == 0 && wave == 0 && lane < 32 && i0 + lane < M)
        gb[i0 + lane] = (s_b[0][lane] + s_b[1][lane]) + (s_b[2][lane] + s_b[3][lane]);
}

template <bool RELU>
__global__ __launch_bounds__(256) void linear_bwd_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                         const float *__restrict__ x, const float *__restrict__ w,
                                                         int R, int IN, int OUT, float *__restrict__ gx,
                                                         float *__restrict__ gw, float *__restrict__ gb, int n_gx,
                                                         int gx_tj, int gw_tj) {
    __shared__ float s_c[4][16][64];
    __shared__ float s_b[4][32];
    const int tile = blockIdx.x;
    // C (M x N) = A (M x K) B (K x N):   gx: A = G' (R x OUT), B = W (OUT x IN)     gw: A = G'^T (OUT x R), B = X (R x IN)
    if (tile < n_gx) {
        linear_bwd_tile<true, RELU>(g, y, w, R, IN, OUT, OUT, (tile / gx_tj) * 32, (tile % gx_tj) * 32, gx, nullptr, s_c, s_b);
    } else {
        const int t = tile - n_gx;
        linear_bwd_tile<false, RELU>(g, y, x, OUT, IN, R, OUT, (t / gw_tj) * 32, (t % gw_tj) * 32, gw, gb, s_c, s_b);
    }
}

// Forward of the same linears: y = [relu](x W^T + b), one 32 x 32 tile per workgroup.  Both operands are contiguous
// along the contraction (x rows, W rows), so a lane's four k of a chunk are ONE 16-byte load each.
template <bool RELU>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         const float *__restrict__ bias, int R, int IN, int OUT,
                                                         float *__restrict__ yout, int tj) {
    __shared__ float s_c[4][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = (blockIdx.x / tj) * 32, j0 = (blockIdx.x % tj) * 32;
    const int i = i0 + (lane & 31), j = j0 + (lane & 31), kq = (lane >> 5) * 4;
    const bool iok = i < R, jok = j < OUT;
    const int chunks = (IN + 7) / 8, per = (chunks + 3) / 4;
    const int c_lo = wave * per, c_hi = (c_lo + per) < chunks ? (c_lo + per) : chunks;
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = c_lo; c < c_hi; c += LB_U) {
        float4 a[LB_U], b[LB_U];
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            const int k0 = (c + u) * 8 + kq;
            const bool kok = c + u < c_hi && k0 < IN;          // (IN is a multiple of 4: the launcher checks)
            a[u] = (iok && kok) ? *reinterpret_cast<const float4 *>(x + (long)i * IN + k0) : float4{0.f, 0.f, 0.f, 0.f};
            b[u] = (jok && kok) ? *reinterpret_cast<const float4 *>(w + (long)j * IN + k0) : float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b[u].w, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    __syncthreads();
    const float bj = (bias != nullptr && jok) ? bias[j] : 0.f;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        float v = ((s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane])) + bj;
        if (RELU) v = v < 0.f ? 0.f : v;
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < R && jok) yout[(long)row * OUT + j] = v;
    }
}

// ---- the same tiles with their operands staged through LDS (the shipped form; MEMOTR_LINEAR_STAGED=0 launches the
//      kernels above) ----
// The arithmetic is the kernels' above, MFMA for MFMA: the same lane -> (i, j, k) mapping, the same quarter of the
// chunks per wavefront in the same k order, the same reduction.  Only where an operand comes from differs: the workgroup
// first brings the A and B tile of the whole contraction into LDS -- every thread issues its 16-byte loads of both
// operands (and of the ReLU mask, applied on the way in) back to back, so the tile costs ONE memory round trip where the
// direct form pays one per LB_U chunks with four dwords per lane and chunk for every operand that is not contiguous along k.
// Two LDS images, both read without bank conflicts by lanes l & 31 along i / j with the half-waves 4 k apart:
//   ROW  the operand is contiguous along k (G for grad_x; x and W forward): [32 rows][pitch 32 S + 4]; a lane's four k
//        are one ds_read_b128 (pitch / 4 is odd: the 16 lanes of a b128 group hit 16 distinct bank quads);
//   COL  the operand is contiguous along i / j (W and X backward, G for grad_w): [k][32]; four ds_read_b32.
// LDS holds LS_S chunks of 8 k per wavefront; a longer contraction goes in K blocks (OUT > 512 or rows > 512 backward,
// IN > 512 forward), block b holding chunks b S .. b S + S - 1 of EVERY wavefront's quarter.  A launch asks for exactly
// its largest tile's images (66 KB at K = 256, 80 KB for the weight-gradient tiles of 320 rows: two workgroups per CU);
// the 16.5 KB of the reduction lie over the images once every wavefront is done with them.
// `VEC`: every operand base is 16-byte aligned and every pitch a multiple of 4; otherwise the same pieces come in as
// dwords.  Pieces past an edge are zero (their loads are redirected to the operand's first element and discarded, so
// that the loads stay unconditional and issue together).
constexpr int LS_S = 16;
constexpr int LS_RED_FLOATS = 4 * 16 * 64 + 4 * 32;          // s_c and s_b of the reduction, over the images once they are spent

__host__ __device__ constexpr int ls_pitch(int S) { return 32 * S + 4; }
// chunks of 8 k per wavefront that LDS holds of a contraction of length K, and the floats of an image of that many
__host__ __device__ constexpr int ls_chunks(int K) { return (((K + 7) / 8 + 3) / 4) < LS_S ? (((K + 7) / 8 + 3) / 4) : LS_S; }
__host__ __device__ constexpr int ls_image(bool row, int S) { return row ? 32 * ls_pitch(S) : 8 * 4 * S * 32; }
// dynamic LDS of a launch whose tiles contract over K with these images (the reduction re-uses the images' bytes)
constexpr size_t ls_bytes(bool a_row, bool b_row, int K) {
    const int n = ls_image(a_row, ls_chunks(K)) + ls_image(b_row, ls_chunks(K));
    return sizeof(float) * (size_t)(n > LS_RED_FLOATS ? n : LS_RED_FLOATS);
}

// piece (w, it) of a thread for K block b: `off` where its four floats start in the operand, `n` how many of them are
// real (0 .. 4), `lds` where they go in the image (-1: no such slot, or one past the contraction's last chunk, which no
// MFMA reads).  lim / t0: rows (ROW) or columns (COL) of the operand and the tile's first one.
template <bool ROW>
__device__ __forceinline__ void ls_piece(int w, int it, int b, int S, int per, int K, int lim, int t0, long ld, long &off,
                                         int &n, int &lds) {
    const int g8 = threadIdx.x >> 3, f = threadIdx.x & 7;
    int left;
    if (ROW) {          // 8 threads per row: 8 consecutive 16-byte pieces = 4 chunks of wavefront w's quarter
        const int fi = f + 8 * it, t = fi >> 1, cw = b * S + t;
        const int k0 = 8 * (w * per + cw) + 4 * (fi & 1);
        left = (fi < 2 * S && cw < per && t0 + g8 < lim) ? K - k0 : 0;
        off = (long)(t0 + g8) * ld + k0;
        lds = (fi < 2 * S && cw < per && 8 * (w * per + cw) < K) ? g8 * ls_pitch(S) + 8 * (w * S + t) + 4 * (fi & 1) : -1;
    } else {            // 8 threads per k: the 32 columns of the tile
        const int kr = g8 + 32 * it, cw = b * S + (kr >> 3);
        const int k = 8 * (w * per + b * S) + kr;
        left = (kr < 8 * S && cw < per && k < K) ? lim - (t0 + 4 * f) : 0;
        off = (long)k * ld + t0 + 4 * f;
        lds = (kr < 8 * S && cw < per && 8 * (w * per + cw) < K) ? (8 * w * S + kr) * 32 + 4 * f : -1;
    }
    n = left < 0 ? 0 : (left > 4 ? 4 : left);
}

template <bool VEC>
__device__ __forceinline__ float4 ls_load4(const float *__restrict__ src, long off, int n) {
    float4 v;
    if (VEC) {          // (n is 0 or 4: pitches, K and the tile origins are multiples of 4)
        v = *reinterpret_cast<const float4 *>(src + (n > 0 ? off : 0));
        if (n <= 0) v = float4{0.f, 0.f, 0.f, 0.f};
    } else {
        v.x = src[n > 0 ? off : 0];
        v.y = src[n > 1 ? off + 1 : 0];
        v.z = src[n > 2 ? off + 2 : 0];
        v.w = src[n > 3 ? off + 3 : 0];
        v.x = n > 0 ? v.x : 0.f; v.y = n > 1 ? v.y : 0.f; v.z = n > 2 ? v.z : 0.f; v.w = n > 3 ? v.w : 0.f;
    }
    return v;
}

// K block b of both operands into LDS.  A is masked by y on the way in when RELU: y <= 0 ? 0 : g, aten's
// threshold_backward (a NaN activation passes g); zero-filled pieces stay zero under it.
template <bool AROW, bool BROW, bool RELU, bool VEC>
__device__ __forceinline__ void ls_stage(const float *__restrict__ a_src, const float *__restrict__ y_src, long a_ld,
                                         int a_lim, int a_t0, const float *__restrict__ b_src, long b_ld, int b_lim,
                                         int b_t0, int K, int per, int S, int b, float *__restrict__ As,
                                         float *__restrict__ Bs) {
    const int n_it = (S + 3) / 4;
    for (int it0 = 0; it0 < n_it; it0 += 2) {
        float4 va[2][4], vy[2][4], vb[2][4];
        int la[2][4], lb[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                long off;
                int n;
                ls_piece<AROW>(w, it0 + u, b, S, per, K, a_lim, a_t0, a_ld, off, n, la[u][w]);
                va[u][w] = ls_load4<VEC>(a_src, off, n);
                if (RELU) vy[u][w] = ls_load4<VEC>(y_src, off, n);
                ls_piece<BROW>(w, it0 + u, b, S, per, K, b_lim, b_t0, b_ld, off, n, lb[u][w]);
                vb[u][w] = ls_load4<VEC>(b_src, off, n);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                float4 a = va[u][w];
                if (RELU) {
                    const float4 m = vy[u][w];
                    a.x = m.x <= 0.f ? 0.f : a.x; a.y = m.y <= 0.f ? 0.f : a.y;
                    a.z = m.z <= 0.f ? 0.f : a.z; a.w = m.w <= 0.f ? 0.f : a.w;
                }
                if (la[u][w] >= 0) *reinterpret_cast<float4 *>(As + la[u][w]) = a;
                if (lb[u][w] >= 0) *reinterpret_cast<float4 *>(Bs + lb[u][w]) = vb[u][w];
            }
        }
    }
}

// a wavefront's n_t chunks of the staged block: per chunk the four MFMAs (and bias-sum adds) of the direct form
template <bool AROW, bool BROW>
__device__ __forceinline__ void ls_mfma(const float *__restrict__ As, const float *__restrict__ Bs, int S, int n_t,
                                        lb_f32x16 &acc, float &bsum) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l = lane & 31, kq = (lane >> 5) * 4;
    n_t = __builtin_amdgcn_readfirstlane(n_t);          // (uniform: a scalar trip count)
    const float *ap = AROW ? As + l * ls_pitch(S) + 8 * wave * S + kq : As + (8 * wave * S + kq) * 32 + l;
    const float *bp = BROW ? Bs + l * ls_pitch(S) + 8 * wave * S + kq : Bs + (8 * wave * S + kq) * 32 + l;
    auto read = [&](int t, float *a, float *b) {
        if (AROW) {
            const float4 v = *reinterpret_cast<const float4 *>(ap + 8 * t);
            a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = ap[(8 * t + q) * 32];
        }
        if (BROW) {
            const float4 v = *reinterpret_cast<const float4 *>(bp + 8 * t);
            b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = bp[(8 * t + q) * 32];
        }
    };
    auto mfma4 = [&](const float *a, const float *b) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
            bsum += a[q];
        }
    };
    if (n_t <= 0) return;
    float a0[4], b0[4], a1[4], b1[4];
    read(0, a0, b0);
    int t = 0;
    for (; t + 2 <= n_t; t += 2) {          // the next chunk's LDS reads are in flight under this chunk's MFMAs
        read(t + 1, a1, b1);
        mfma4(a0, b0);
        read(t + 2 < n_t ? t + 2 : t + 1, a0, b0);
        mfma4(a1, b1);
    }
    if (t < n_t) mfma4(a0, b0);
}

// the whole contraction of one tile: C (32 x 32 at i0, j0) += A B over K, this wavefront's quarter in `acc`
template <bool AROW, bool BROW, bool RELU, bool VEC>
__device__ __forceinline__ void ls_contract(const float *__restrict__ a_src, const float *__restrict__ y_src, long a_ld,
                                            int a_lim, int a_t0, const float *__restrict__ b_src, long b_ld, int b_lim,
                                            int b_t0, int K, float *__restrict__ smem, lb_f32x16 &acc, float &bsum) {
    const int wave = threadIdx.x >> 6;
    const int chunks = (K + 7) / 8, per = (chunks + 3) / 4;
    const int mine = (chunks - wave * per) < per ? (chunks - wave * per) : per;          // c_hi - c_lo (may be <= 0)
    const int S = ls_chunks(K);
    float *As = smem, *Bs = As + ls_image(AROW, S);
    for (int b = 0; b * S < per; ++b) {
        if (b) __syncthreads();                    // every wavefront is done with the block before
        ls_stage<AROW, BROW, RELU, VEC>(a_src, y_src, a_ld, a_lim, a_t0, b_src, b_ld, b_lim, b_t0, K, per, S, b, As, Bs);
        __syncthreads();
        const int n_t = (mine - b * S) < S ? (mine - b * S) : S;
        ls_mfma<AROW, BROW>(As, Bs, S, n_t, acc, bsum);
    }
    __syncthreads();          // the caller's reduction buffers lie over the images
}

template <bool GX, bool RELU, bool VEC>
__device__ __forceinline__ void linear_bwd_tile_staged(const float *__restrict__ g, const float *__restrict__ y,
                                                       const float *__restrict__ Bp, int M, int N, int K, int OUT, int i0,
                                                       int j0, float *__restrict__ C, float *__restrict__ gb,
                                                       float *__restrict__ smem) {
    float(*s_c)[16][64] = reinterpret_cast<float(*)[16][64]>(smem);
    float(*s_b)[32] = reinterpret_cast<float(*)[32]>(smem + 4 * 16 * 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = j0 + (lane & 31);
    const bool jok = j < N;
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    // GX: A rows are rows of G (ROW image); else A columns are rows of G (COL image).  B rows are rows of W / X.
    ls_contract<GX, false, RELU, VEC>(g, y, OUT, M, i0, Bp, N, N, j0, K, smem, acc, bsum);
    // add the four partial tiles (and bias sums) up, as linear_bwd_tile does
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    bsum += __shfl_xor(bsum, 32, 64);
    if (lane < 32) s_b[wave][lane] = bsum;
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const float v = (s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane]);
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M && jok) C[(long)row * N + j] = v;
    }
    if (!GX && gb != nullptr && j0 == 0 && wave == 0 && lane < 32 && i0 + lane < M)
        gb[i0 + lane] = (s_b[0][lane] + s_b[1][lane]) + (s_b[2][lane] + s_b[3][lane]);
}

template <bool RELU, bool VEC>
__global__ __launch_bounds__(256) void linear_bwd_staged_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                                const float *__restrict__ x, const float *__restrict__ w,
                                                                int R, int IN, int OUT, float *__restrict__ gx,
                                                                float *__restrict__ gw, float *__restrict__ gb, int n_gx,
                                                                int gx_tj, int gw_tj) {
    extern __shared__ __attribute__((aligned(16))) float s_linear[];
    const int tile = blockIdx.x;
    if (tile < n_gx) {
        linear_bwd_tile_staged<true, RELU, VEC>(g, y, w, R, IN, OUT, OUT, (tile / gx_tj) * 32, (tile % gx_tj) * 32, gx,
                                                nullptr, s_linear);
    } else {
        const int t = tile - n_gx;
        linear_bwd_tile_staged<false, RELU, VEC>(g, y, x, OUT, IN, R, OUT, (t / gw_tj) * 32, (t % gw_tj) * 32, gw, gb,
                                                 s_linear);
    }
}

template <bool RELU, bool VEC>
__global__ __launch_bounds__(256) void linear_fwd_staged_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                const float *__restrict__ bias, int R, int IN, int OUT,
                                                                float *__restrict__ yout, int tj) {
    extern __shared__ __attribute__((aligned(16))) float s_linear[];
    float(*s_c)[16][64] = reinterpret_cast<float(*)[16][64]>(s_linear);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = (blockIdx.x / tj) * 32, j0 = (blockIdx.x % tj) * 32;
    const int j = j0 + (lane & 31);
    const bool jok = j < OUT;
    lb_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float unused = 0.f;
    ls_contract<true, true, false, VEC>(x, nullptr, IN, R, i0, w, IN, OUT, j0, IN, s_linear, acc, unused);
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[wave][r][lane] = acc[r];
    __syncthreads();
    const float bj = (bias != nullptr && jok) ? bias[j] : 0.f;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        float v = ((s_c[0][r][lane] + s_c[1][r][lane]) + (s_c[2][r][lane] + s_c[3][r][lane])) + bj;
        if (RELU) v = v < 0.f ? 0.f : v;
        const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < R && jok) yout[(long)row * OUT + j] = v;
    }
}

// MEMOTR_LINEAR_STAGED=0: the direct-from-global kernels (the A/B switch of both entry points, read at every launch)
bool linear_staged() {
    const char *e = getenv("MEMOTR_LINEAR_STAGED");
    return !(e && e[0] == '0' && e[1] == 0);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

// ---- per-frame bookkeeping of the criterion (round 6, ABI 10): index arithmetic on a few hundred elements that took
//      7 and 11 torch launches per frame -- the forward between two decoder graphs is bound by the host's launch rate ----
// one workgroup: thread i < n_tr finds the LAST ground truth carrying track i's id, thread j < n_gt whether any track
// carries ground truth j's id
__global__ __launch_bounds__(256) void track_ownership_kernel(const int64_t *__restrict__ tr_ids, int n_tr,
                                                              const int64_t *__restrict__ gt_ids, int n_gt,
                                                              int64_t *__restrict__ matched, float *__restrict__ free_out) {
    for (int i = threadIdx.x; i < n_tr; i += blockDim.x) {
        const int64_t id = tr_ids[i];
        int64_t m = -1;
        for (int j = 0; j < n_gt; ++j)
            if (gt_ids[j] == id) m = j;
        matched[i] = m;
    }
    for (int j = threadIdx.x; j < n_gt; j += blockDim.x) {
        const int64_t id = gt_ids[j];
        bool owned = false;
        for (int i = 0; i < n_tr; ++i) owned = owned || tr_ids[i] == id;
        free_out[j] = owned ? 0.f : 1.f;
    }
}

// one workgroup: background everywhere, the carried tracks' labels in the late layers, then the matched pairs
__global__ __launch_bounds__(256) void focal_labels_kernel(const int64_t *__restrict__ lay, const int64_t *__restrict__ q,
                                                           const int64_t *__restrict__ g, int n_pairs,
                                                           const int64_t *__restrict__ gt_labels, int n_gt,
                                                           const int64_t *__restrict__ matched, int n_tr,
                                                           const unsigned char *__restrict__ late, int n_layers, int nd,
                                                           int K, int64_t *__restrict__ labels) {
    const int nq = nd + n_tr;
    for (int e = threadIdx.x; e < n_layers * nq; e += blockDim.x) {
        const int l = e / nq, c = e - l * nq;
        int64_t v = K;
        if (c >= nd && late[l]) {
            const int64_t m = matched[c - nd];
            if (m >= 0 && m < n_gt) v = gt_labels[m];
        }
        labels[e] = v;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < n_pairs; p += blockDim.x) {
        const int64_t l = lay[p], c = q[p], t = g[p];
        if (l >= 0 && l < n_layers && c >= 0 && c < nq && t >= 0 && t < n_gt) labels[l * nq + c] = gt_labels[t];
    }
}

// ---- result rows of the submit path (ABI 12): the score / area filter and the pixel boxes of SequenceTracker._report,
//      compacted onto the end of a device-resident table -- one launch per frame, no host read ----
// one workgroup; rows in chunks of 256: a 64-bit ballot and the population count of the lower lanes place a row inside
// its wavefront, the four wave totals go through LDS, `base` runs across chunks.  Both counters are read before
// anything is written and written once, by one lane, with plain stores.  Every float operation rounds once.
__global__ __launch_bounds__(256) void result_rows_kernel(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                          const int64_t *__restrict__ ids,
                                                          const int64_t *__restrict__ labels, int n, int K, int64_t frame,
                                                          float ori_w, float ori_h, float score_thresh, float area_thresh,
                                                          float *__restrict__ rows_f, int64_t *__restrict__ rows_i,
                                                          int32_t *__restrict__ counters, int capacity) {
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stored0 = counters[0], dropped0 = counters[1];
    int base = 0;                                   // rows kept by the chunks before this one
    for (int c0 = 0; c0 < n; c0 += 256) {           // (n is uniform: every thread makes every trip)
        const int i = c0 + (int)threadIdx.x;
        bool keep = false;
        float s = 0.f, cx = 0.f, cy = 0.f, w = 0.f, h = 0.f;
        if (i < n) {
            const float *sc = scores + (long)i * K;
            s = sc[0];
            for (int k = 1; k < K; ++k) {           // torch's max: a NaN wins and stays
                const float v = sc[k];
                if (v > s || v != v) s = v;
            }
            cx = boxes[4 * i], cy = boxes[4 * i + 1], w = boxes[4 * i + 2], h = boxes[4 * i + 3];
            const float area = __fmul_rn(__fmul_rn(__fmul_rn(w, ori_w), h), ori_h);
            keep = s > score_thresh && area > area_thresh;      // false for a NaN on either side
        }
        const unsigned long long m = __ballot(keep);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int v = 0; v < 4; ++v) {
            const int t = wave_total[v];
            before += v < wave ? t : 0;
            total += t;
        }
        if (keep) {
            const long pos = (long)stored0 + base + before + below;
            if (pos >= 0 && pos < capacity) {
                const float hw = __fmul_rn(0.5f, w), hh = __fmul_rn(0.5f, h);
                float *rf = rows_f + pos * 5;
                rf[0] = __fmul_rn(__fsub_rn(cx, hw), ori_w);
                rf[1] = __fmul_rn(__fsub_rn(cy, hh), ori_h);
                rf[2] = __fmul_rn(__fadd_rn(cx, hw), ori_w);
                rf[3] = __fmul_rn(__fadd_rn(cy, hh), ori_h);
                rf[4] = s;
                int64_t *ri = rows_i + pos * 3;
                ri[0] = frame;
                ri[1] = ids[i];
                ri[2] = labels[i];
            }
        }
        base += total;
        __syncthreads();                            // wave_total is written again by the next chunk
    }
    if (threadIdx.x == 0) {
        const int room = stored0 < 0 ? 0 : (capacity > stored0 ? capacity - stored0 : 0);
        const int stored = base < room ? base : room;
        counters[0] = stored0 + stored;
        counters[1] = dropped0 + (base - stored);
    }
}

// ---- track bank (include/clip_ops_hip.h: clipops_bank_*): the online tracker's bookkeeping for B sequences at once,
//      on fixed-size slot tables -- no row count ever reaches the host ----
// One workgroup per stream, three phases separated by barriers:
//   1. the slots that are free when the call begins, in slot order, into the bank's free_list (ballot + population count
//      inside a wavefront, wave totals through LDS, a running base across chunks of 1024 slots);
//   2. one wavefront per live slot: refresh from model row n_det + s, age, retire (the row is zeroed);
//   3. detect rows in chunks of 1024: one thread decides a row's birth and label, the same ballot scheme ranks the born
//      rows, rank j takes free_list[j]; the (row, slot) pairs of the chunk go through LDS and one wavefront copies a pair.
// Phases 2 and 3 write disjoint slots (live / free at the start).  Every counter is read before anything is written and
// written once by one lane with plain stores; no atomics.
template <int NW>
__device__ __forceinline__ void bank_ranks(bool flag, int lane, int wave, int *wave_total, int &before, int &total) {
    const unsigned long long m = __ballot(flag);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    before = below;
    total = 0;
    for (int v = 0; v < NW; ++v) {
        const int t = wave_total[v];
        before += v < wave ? t : 0;
        total += t;
    }
}

// (16 wavefronts: phase 2 is a chain of dependent loads per slot, and a wavefront walks its slots one after another)
constexpr int BANK_THREADS = 1024, BANK_WAVES = BANK_THREADS / 64;

__global__ __launch_bounds__(BANK_THREADS) void bank_update_kernel(clipops_bank_model m, clipops_bank bank, int n_det, int cap,
                                                          int K, int C, int use_dab, float det_thresh,
                                                          float track_thresh, int64_t miss_tolerance) {
#pragma clang fp contract(off)
    __shared__ int wave_total[BANK_WAVES], wave_live[BANK_WAVES], pair_row[BANK_THREADS], pair_slot[BANK_THREADS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int QW = use_dab ? C : 2 * C;
    const long bc = (long)b * cap;
    int64_t *ids = bank.ids + bc, *labels = bank.labels + bc, *dtime = bank.disappear_time + bc;
    int32_t *free_list = bank.free_list + bc;
    float *boxes = bank.boxes + bc * 4, *ref_pts = bank.ref_pts + bc * 4;
    float *logits = bank.logits + bc * K, *scores = bank.scores + bc * K;
    float *out_embed = bank.output_embed + bc * C, *long_mem = bank.long_memory + bc * C;
    float *last_out = bank.last_output + bc * C, *query = bank.query_embed + bc * QW;
    const float *m_logits = m.ptr[CLIPOPS_BK_LOGITS] + b * m.batch_stride[CLIPOPS_BK_LOGITS];
    const float *m_boxes = m.ptr[CLIPOPS_BK_BOXES] + b * m.batch_stride[CLIPOPS_BK_BOXES];
    const float *m_out = m.ptr[CLIPOPS_BK_OUTPUTS] + b * m.batch_stride[CLIPOPS_BK_OUTPUTS];
    const float *m_ref = m.ptr[CLIPOPS_BK_LAST_REF] + b * m.batch_stride[CLIPOPS_BK_LAST_REF];
    const float *m_query = m.ptr[CLIPOPS_BK_QUERIES] + b * m.batch_stride[CLIPOPS_BK_QUERIES];
    const long rs_logits = m.row_stride[CLIPOPS_BK_LOGITS], rs_boxes = m.row_stride[CLIPOPS_BK_BOXES];
    const long rs_out = m.row_stride[CLIPOPS_BK_OUTPUTS], rs_ref = m.row_stride[CLIPOPS_BK_LAST_REF];
    const long rs_query = m.row_stride[CLIPOPS_BK_QUERIES];
    const int64_t next0 = bank.next_id[b];
    const int dropped0 = bank.counters[2 * b + 1];

    // ---- 1. free slots, as they are before this call
    int n_free = 0;
    for (int s0 = 0; s0 < cap; s0 += BANK_THREADS) {
        const int s = s0 + (int)threadIdx.x;
        const bool is_free = s < cap && ids[s] < 0;
        int before, total;
        bank_ranks<BANK_WAVES>(is_free, lane, wave, wave_total, before, total);
        if (is_free) free_list[n_free + before] = s;
        n_free += total;
        __syncthreads();                            // wave_total is written again; ids are written from here on
    }

    // ---- 2. live slots: one wavefront each (s, id, label and the decision are uniform over the wavefront)
    int live = 0;
    for (int s = wave; s < cap; s += BANK_WAVES) {
        const int64_t id = ids[s], d0 = dtime[s];
        int64_t lab = labels[s];
        if (id < 0) continue;
        const long r = (long)n_det + s;
        const float *lg = m_logits + r * rs_logits;
        lab = lab < 0 ? 0 : (lab >= K ? K - 1 : lab);
        const float own = sigmoidf(lg[lab]);
        const int64_t d = own < track_thresh ? d0 + 1 : 0;             // (a NaN score does not age the track)
        if (d >= miss_tolerance) {                                      // retired: the slot holds zeros again
            for (int c = lane; c < K; c += 64) logits[(long)s * K + c] = 0.f, scores[(long)s * K + c] = 0.f;
            if (lane < 4) boxes[s * 4L + lane] = 0.f, ref_pts[s * 4L + lane] = 0.f;
            for (int c = lane; c < C; c += 64)
                out_embed[(long)s * C + c] = 0.f, long_mem[(long)s * C + c] = 0.f, last_out[(long)s * C + c] = 0.f;
            for (int c = lane; c < QW; c += 64) query[(long)s * QW + c] = 0.f;
            if (lane == 0) ids[s] = -1, labels[s] = 0, dtime[s] = 0;
        } else {
            for (int c = lane; c < K; c += 64) {
                const float v = lg[c];
                logits[(long)s * K + c] = v;
                scores[(long)s * K + c] = sigmoidf(v);
            }
            if (lane < 4) boxes[s * 4L + lane] = m_boxes[r * rs_boxes + lane];
            for (int c = lane; c < C; c += 64) out_embed[(long)s * C + c] = m_out[r * rs_out + c];
            if (lane == 0) dtime[s] = d;
            ++live;
        }
    }
    if (lane == 0) wave_live[wave] = live;
    __syncthreads();

    // ---- 3. births
    int born_base = 0;                              // born rows of the chunks before this one
    for (int c0 = 0; c0 < n_det; c0 += BANK_THREADS) {      // (n_det is uniform: every thread makes every trip)
        const int r = c0 + (int)threadIdx.x;
        bool born = false;
        int label = 0;
        if (r < n_det) {
            const float *lg = m_logits + r * rs_logits;
            float best = sigmoidf(lg[0]);
            bool nan = best != best;
            for (int k = 1; k < K; ++k) {           // the lowest index of the maximum
                const float v = sigmoidf(lg[k]);
                nan |= v != v;
                if (v > best) best = v, label = k;
            }
            born = !nan && best >= det_thresh;
        }
        int before, total;
        bank_ranks<BANK_WAVES>(born, lane, wave, wave_total, before, total);
        const int room = n_free > born_base ? n_free - born_base : 0;
        const int n_pairs = total < room ? total : room;
        if (born && before < n_pairs) {
            const int slot = free_list[born_base + before];
            pair_row[before] = r;
            pair_slot[before] = slot;
            ids[slot] = next0 + born_base + before;
            labels[slot] = label;
            dtime[slot] = 0;
        }
        __syncthreads();
        for (int p = wave; p < n_pairs; p += BANK_WAVES) {
            const long row = pair_row[p], s = pair_slot[p];
            const float *lg = m_logits + row * rs_logits;
            for (int c = lane; c < K; c += 64) {
                const float v = lg[c];
                logits[s * K + c] = v;
                scores[s * K + c] = sigmoidf(v);
            }
            if (lane < 4) {
                boxes[s * 4 + lane] = m_boxes[row * rs_boxes + lane];
                ref_pts[s * 4 + lane] = m_ref[row * rs_ref + lane];
            }
            for (int c = lane; c < C; c += 64) {
                const float o = m_out[row * rs_out + c], q = m_query[row * rs_query + c];
                out_embed[s * C + c] = o;
                last_out[s * C + c] = o;
                long_mem[s * C + c] = q;
                if (use_dab) {
                    query[s * QW + c] = q;
                } else {
                    query[s * QW + c] = m.det_embed[row * m.det_row_stride + c];
                    query[s * QW + C + c] = q;
                }
            }
        }
        born_base += total;
        __syncthreads();                            // wave_total and the pairs are written again by the next chunk
    }
    if (threadIdx.x == 0) {
        const int placed = born_base < n_free ? born_base : n_free;
        bank.next_id[b] = next0 + placed;
        int live_after = placed;
        for (int v = 0; v < BANK_WAVES; ++v) live_after += wave_live[v];
        bank.counters[2 * b] = live_after;
        bank.counters[2 * b + 1] = dropped0 + (born_base - placed);
    }
}

// clipops_result_rows_f32's filter and arithmetic over the B * cap slots of a bank, streams in order, free slots skipped:
// one workgroup, so that the rows of all streams land in one table in a fixed order.
__global__ __launch_bounds__(256) void bank_result_rows_kernel(const float *__restrict__ boxes,
                                                               const float *__restrict__ scores,
                                                               const int64_t *__restrict__ ids,
                                                               const int64_t *__restrict__ labels, int n_slots, int cap,
                                                               int K, const int64_t *__restrict__ seq_frame,
                                                               const float *__restrict__ ori_wh, float score_thresh,
                                                               float area_thresh, float *__restrict__ rows_f,
                                                               int64_t *__restrict__ rows_i,
                                                               int32_t *__restrict__ counters, int capacity) {
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stored0 = counters[0], dropped0 = counters[1];
    int base = 0;
    for (int c0 = 0; c0 < n_slots; c0 += 256) {
        const int i = c0 + (int)threadIdx.x;
        bool keep = false;
        int b = 0;
        float s = 0.f, cx = 0.f, cy = 0.f, w = 0.f, h = 0.f, ori_w = 0.f, ori_h = 0.f;
        if (i < n_slots && ids[i] >= 0) {
            b = i / cap;
            ori_w = ori_wh[2 * b], ori_h = ori_wh[2 * b + 1];
            const float *sc = scores + (long)i * K;
            s = sc[0];
            for (int k = 1; k < K; ++k) {           // torch's max: a NaN wins and stays
                const float v = sc[k];
                if (v > s || v != v) s = v;
            }
            cx = boxes[4L * i], cy = boxes[4L * i + 1], w = boxes[4L * i + 2], h = boxes[4L * i + 3];
            const float area = __fmul_rn(__fmul_rn(__fmul_rn(w, ori_w), h), ori_h);
            keep = s > score_thresh && area > area_thresh;
        }
        int before, total;
        bank_ranks<4>(keep, lane, wave, wave_total, before, total);
        if (keep) {
            const long pos = (long)stored0 + base + before;
            if (pos >= 0 && pos < capacity) {
                const float hw = __fmul_rn(0.5f, w), hh = __fmul_rn(0.5f, h);
                float *rf = rows_f + pos * 5;
                rf[0] = __fmul_rn(__fsub_rn(cx, hw), ori_w);
                rf[1] = __fmul_rn(__fsub_rn(cy, hh), ori_h);
                rf[2] = __fmul_rn(__fadd_rn(cx, hw), ori_w);
                rf[3] = __fmul_rn(__fadd_rn(cy, hh), ori_h);
                rf[4] = s;
                int64_t *ri = rows_i + pos * 4;
                ri[0] = seq_frame[2 * b];
                ri[1] = seq_frame[2 * b + 1];
                ri[2] = ids[i];
                ri[3] = labels[i];
            }
        }
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int room = stored0 < 0 ? 0 : (capacity > stored0 ? capacity - stored0 : 0);
        const int stored = base < room ? base : room;
        counters[0] = stored0 + stored;
        counters[1] = dropped0 + (base - stored);
    }
}

// ---- the overlay's draw table from device tracks (include/clip_ops_hip.h: clipops_draw_table_f32) ----
// One workgroup per stream.  A slot's key is its id when the slot is kept (bank_result_rows_kernel's filter, id below
// 2^31) and -1 otherwise; the row of a kept slot is the number of kept slots of the stream with a smaller id (equal ids,
// which a bank never holds, in slot order).  Slots go through in chunks of 1024, one thread each; for every chunk of slots
// the keys of every chunk pass through LDS and each thread counts the ones below its own -- all pairs, no atomics, and
// every thread also counts the kept slots of the stream, so the padding rows are known without another pass.
struct DrawKey {
    int key;                                        // the id of a kept slot, -1 otherwise
    float x1, y1, x2, y2;
};

__device__ __forceinline__ DrawKey draw_table_key(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                  const int64_t *__restrict__ ids, long i, int K, float ori_w,
                                                  float ori_h, float score_thresh, float area_thresh) {
    DrawKey r = {-1, 0.f, 0.f, 0.f, 0.f};
    const int64_t id = ids[i];
    if (id < 0 || id > 0x7fffffffLL) return r;
    const float *sc = scores + i * K;
    float s = sc[0];
    for (int k = 1; k < K; ++k) {                   // torch's max: a NaN wins and stays
        const float v = sc[k];
        if (v > s || v != v) s = v;
    }
    const float cx = boxes[4 * i], cy = boxes[4 * i + 1], w = boxes[4 * i + 2], h = boxes[4 * i + 3];
    const float area = __fmul_rn(__fmul_rn(__fmul_rn(w, ori_w), h), ori_h);
    if (!(s > score_thresh && area > area_thresh)) return r;
    const float hw = __fmul_rn(0.5f, w), hh = __fmul_rn(0.5f, h);
    r.key = (int)id;
    r.x1 = __fmul_rn(__fsub_rn(cx, hw), ori_w);
    r.y1 = __fmul_rn(__fsub_rn(cy, hh), ori_h);
    r.x2 = __fmul_rn(__fadd_rn(cx, hw), ori_w);
    r.y2 = __fmul_rn(__fadd_rn(cy, hh), ori_h);
    return r;
}

// floor(v + 0.5) in float32, NaN -> 0, clamped to +-2^24 (render.track_table)
__device__ __forceinline__ int draw_table_round(float v) {
    const float r = floorf(__fadd_rn(v, 0.5f));
    if (r != r) return 0;
    return (int)fminf(fmaxf(r, -16777216.f), 16777216.f);
}

// render.palette_entry(i), i in 0 .. 63, as r | g << 8 | b << 16
__device__ __forceinline__ int draw_table_palette(int i) {
    const int hue = (i * 13 % 64) * 24, sector = hue >> 8, f = hue & 255;
    const int lo = i % 3 == 0 ? 0 : (i % 3 == 1 ? 64 : 112);
    const int up = lo + (255 - lo) * f / 255, down = lo + (255 - lo) * (255 - f) / 255;
    int r, g, b;
    switch (sector) {
        case 0: r = 255, g = up, b = lo; break;
        case 1: r = down, g = 255, b = lo; break;
        case 2: r = lo, g = 255, b = up; break;
        case 3: r = lo, g = down, b = 255; break;
        case 4: r = up, g = lo, b = 255; break;
        default: r = 255, g = lo, b = down; break;
    }
    return r | g << 8 | b << 16;
}

constexpr int DRAW_ROW_WORDS = 16;                  // TRACKDRAW_ROW_WORDS of include/track_draw_hip.h

__global__ __launch_bounds__(BANK_THREADS) void draw_table_kernel(const float *__restrict__ boxes,
                                                                  const float *__restrict__ scores,
                                                                  const int64_t *__restrict__ ids, int cap, int K,
                                                                  const float *__restrict__ ori_wh, float score_thresh,
                                                                  float area_thresh, int bgr, int font_scale,
                                                                  int32_t *__restrict__ table) {
    __shared__ int4 keys4[BANK_THREADS / 4];
    int *keys = reinterpret_cast<int *>(keys4);
    const int b = blockIdx.x, tid = threadIdx.x;
    const long bc = (long)b * cap;
    const float ori_w = ori_wh[2 * b], ori_h = ori_wh[2 * b + 1];
    int32_t *rows = table + bc * DRAW_ROW_WORDS;
    int total = 0;                                  // kept slots of the stream (every thread counts them all)
    for (int i0 = 0; i0 < cap; i0 += BANK_THREADS) {             // (cap is uniform: every thread makes every trip)
        const int i = i0 + tid;
        DrawKey mine = {-1, 0.f, 0.f, 0.f, 0.f};
        if (i < cap) mine = draw_table_key(boxes, scores, ids, bc + i, K, ori_w, ori_h, score_thresh, area_thresh);
        int rank = 0;
        total = 0;
        for (int j0 = 0; j0 < cap; j0 += BANK_THREADS) {
            int kj = mine.key;
            if (j0 != i0) {
                const int j = j0 + tid;
                kj = j < cap ? draw_table_key(boxes, scores, ids, bc + j, K, ori_w, ori_h, score_thresh, area_thresh).key
                             : -1;
            }
            keys[tid] = kj;
            __syncthreads();
            const int nj4 = (min(BANK_THREADS, cap - j0) + 3) >> 2;     // (every thread wrote a key: -1 past cap)
#pragma unroll 4
            for (int q = 0; q < nj4; ++q) {         // four keys a read: the loop is a chain of LDS latencies otherwise
                const int4 k4 = keys4[q];
                const int k[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    total += k[e] >= 0;
                    rank += k[e] >= 0 && (k[e] < mine.key || (k[e] == mine.key && j0 + 4 * q + e < i));
                }
            }
            __syncthreads();                        // keys is written again by the next chunk
        }
        if (mine.key < 0) continue;
        const int id = mine.key;
        const int x1 = draw_table_round(mine.x1), y1 = draw_table_round(mine.y1);
        const int rgb = draw_table_palette(id & 63);
        const int r = rgb & 255, g = (rgb >> 8) & 255, bl = rgb >> 16;
        int n_digits = 1;
        for (int v = id; v >= 10; v /= 10) ++n_digits;
        unsigned lo_word = 0, hi_word = 0;          // glyph k is the k-th digit from the left
        for (int k = n_digits - 1, v = id; k >= 0; --k, v /= 10) {
            const unsigned d = (unsigned)(v % 10);
            if (k < 8) lo_word |= d << (4 * k);
            else hi_word |= d << (4 * (k - 8));
        }
        const int tab_w = (6 * n_digits - 1) * font_scale + 2, tab_h = 7 * font_scale + 2;
        const int ty1 = y1 - tab_h >= 0 ? y1 - tab_h : y1;
        const int tx1 = min(x1, (int)ori_w - tab_w);
        int32_t *row = rows + (long)rank * DRAW_ROW_WORDS;
        row[0] = x1, row[1] = y1, row[2] = draw_table_round(mine.x2), row[3] = draw_table_round(mine.y2);
        row[4] = bgr ? (bl | g << 8 | r << 16) : rgb;
        row[5] = tx1, row[6] = ty1, row[7] = tx1 + tab_w - 1, row[8] = ty1 + tab_h - 1;
        row[9] = ((77 * r + 150 * g + 29 * bl) >> 8) >= 128 ? 0 : 0xFFFFFF;
        row[10] = n_digits, row[11] = (int32_t)lo_word, row[12] = (int32_t)hi_word;
        row[13] = row[14] = row[15] = 0;
    }
    for (int p = total + tid; p < cap; p += BANK_THREADS) {      // the rows that draw nothing: x2 < x1
        int32_t *row = rows + (long)p * DRAW_ROW_WORDS;
        for (int k = 0; k < DRAW_ROW_WORDS; ++k) row[k] = (k == 2 || k == 3) ? -1 : 0;
    }
}

// ---- gap filling and short-track removal on a result table (include/clip_ops_hip.h: clipops_fill_gaps_f32) ----
// Workspace, int32: cell[n_seq][n_ids][n_frames] | right[the same] | offs[n_seq][n_frames].
//   cell   -1 empty; v >= 0 the table row that sits there; v <= -2 a filled cell whose left neighbour is row -(v + 2)
//   right  pass 1 of the track kernel: the next occupied frame at or after the cell; of a filled cell afterwards: the
//          table row of its right neighbour
//   offs   the surviving cells of a (sequence, frame), then the output row its first survivor goes to
// Five launches in stream order: clear, scatter, one workgroup per track, count + scan over (sequence, frame), write.
// Integer atomics only (who owns a cell, the status bits): a table without duplicates gives the same bits every time.
constexpr int FG_THREADS = 1024, FG_WAVES = FG_THREADS / 64, FG_NONE = 0x7fffffff;

__global__ __launch_bounds__(256) void fg_clear_kernel(int32_t *__restrict__ cell, long cells) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long)gridDim.x * 256) cell[i] = -1;
}

__global__ __launch_bounds__(256) void fg_scatter_kernel(const int64_t *__restrict__ rows_i,
                                                         const int32_t *__restrict__ counters, int n, int W, int n_seq,
                                                         int n_ids, int n_frames, int32_t *__restrict__ cell,
                                                         int32_t *__restrict__ status) {
    const int c0 = counters[0], stored = c0 < 0 ? 0 : (c0 < n ? c0 : n);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < stored; i += (long)gridDim.x * 256) {
        const int64_t *r = rows_i + i * W;
        const int64_t seq = W == 4 ? r[0] : 0, frame = r[W - 3], id = r[W - 2];
        int bad = 0;
        if (seq < 0 || seq >= n_seq) bad |= CLIPOPS_FG_SEQUENCE;
        if (id < 0 || id >= n_ids) bad |= CLIPOPS_FG_ID;
        if (frame < 0 || frame >= n_frames) bad |= CLIPOPS_FG_FRAME;
        if (bad) {
            atomicOr(status, bad);
            continue;
        }
        if (atomicCAS(cell + ((seq * n_ids + id) * n_frames + frame), -1, (int)i) != -1)
            atomicOr(status, CLIPOPS_FG_DUPLICATE);
    }
}

// One workgroup per track, frames in chunks of 1024, one thread a frame.  Pass 1 walks the chunks from the last to the
// first: a suffix minimum of the occupied frames (shuffles inside a wavefront, wave results and the carry of the later
// chunks through LDS) leaves every cell's next occupied frame in `right`, and the ballots count the track's rows.  Pass 2
// walks forward with the prefix maximum: an empty cell with an occupied frame on either side and at most max_gap missing
// frames between them becomes a filled cell.  A thread writes only its own cell, and only empty cells change while the
// occupied ones are read by others; a track shorter than min_length is emptied instead.
__global__ __launch_bounds__(FG_THREADS) void fg_track_kernel(int32_t *__restrict__ cell, int32_t *__restrict__ right,
                                                              int n_frames, int max_gap, int min_length) {
    __shared__ int wave_val[FG_WAVES], wave_cnt[FG_WAVES];
    int32_t *A = cell + (long)blockIdx.x * n_frames, *B = right + (long)blockIdx.x * n_frames;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (int)(((long)n_frames + FG_THREADS - 1) / FG_THREADS);
    int carry = FG_NONE, length = 0;
    for (int c = n_chunks - 1; c >= 0; --c) {
        const long f = (long)c * FG_THREADS + tid;
        const bool occ = f < n_frames && A[f] >= 0;
        int v = occ ? (int)f : FG_NONE;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(v, d);
            if (lane + d < 64) v = min(v, o);
        }
        const unsigned long long m = __ballot(occ);
        if (lane == 0) wave_val[wave] = v, wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int later = carry, all = carry;
        for (int w = 0; w < FG_WAVES; ++w) {
            const int t = wave_val[w];
            if (w > wave) later = min(later, t);
            all = min(all, t);
            length += wave_cnt[w];
        }
        if (f < n_frames) B[f] = min(v, later);
        carry = all;
        __syncthreads();                            // wave_val and wave_cnt are written again by the next chunk
    }
    const bool keep = length >= min_length;
    carry = -1;
    for (int c = 0; c < n_chunks; ++c) {
        const long f = (long)c * FG_THREADS + tid;
        const int a = f < n_frames ? A[f] : -1;
        int v = a >= 0 ? (int)f : -1;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d);
            if (lane >= d) v = max(v, o);
        }
        if (lane == 63) wave_val[wave] = v;
        __syncthreads();
        int earlier = carry, all = carry;
        for (int w = 0; w < FG_WAVES; ++w) {
            const int t = wave_val[w];
            if (w < wave) earlier = max(earlier, t);
            all = max(all, t);
        }
        if (f < n_frames) {
            if (!keep) {
                if (a >= 0) A[f] = -1;
            } else if (a < 0) {
                const int f0 = max(v, earlier), f1 = B[f];
                if (f0 >= 0 && f1 != FG_NONE && f1 - f0 - 1 <= max_gap) {
                    A[f] = -(A[f0] + 2);
                    B[f] = A[f1];
                }
            }
        }
        carry = all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fg_count_kernel(const int32_t *__restrict__ cell, long n_sf, int n_ids, int n_frames,
                                                       int32_t *__restrict__ offs) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sf) return;
    const int32_t *p = cell + (i / n_frames) * n_ids * n_frames + i % n_frames;
    int c = 0;
    for (int id = 0; id < n_ids; ++id) c += p[(long)id * n_frames] != -1;
    offs[i] = c;
}

// offs[i] <- counters[0] + the survivors of all (sequence, frame) before i (clamped to 2^31 - 1: no row lands there), and
// the counters by clipops_result_rows_f32's capacity rule.  One workgroup: an inclusive scan by shuffles inside a
// wavefront, wave totals through LDS, a running base across chunks of 1024.
__global__ __launch_bounds__(FG_THREADS) void fg_scan_kernel(int32_t *__restrict__ offs, long n_sf,
                                                             int32_t *__restrict__ counters, int capacity) {
    __shared__ int wave_val[FG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stored0 = counters[0], dropped0 = counters[1];
    const long start = stored0 < 0 ? 0 : stored0;
    long base = 0;
    for (long i0 = 0; i0 < n_sf; i0 += FG_THREADS) {
        const long i = i0 + tid;
        const int mine = i < n_sf ? offs[i] : 0;
        int v = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d);
            if (lane >= d) v += o;
        }
        if (lane == 63) wave_val[wave] = v;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < FG_WAVES; ++w) {
            const int t = wave_val[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (i < n_sf) {
            const long at = start + base + before + v - mine;
            offs[i] = (int)(at < FG_NONE ? at : FG_NONE);
        }
        base += total;
        __syncthreads();
    }
    __syncthreads();                                // every thread has read the counters
    if (tid == 0) {
        const long room = stored0 < 0 ? 0 : (capacity > stored0 ? capacity - stored0 : 0);
        const long stored = base < room ? base : room;
        counters[0] = (int)(stored0 + stored);
        counters[1] = (int)(dropped0 + (base - stored));
    }
}

// One workgroup per (sequence, frame): the ids in chunks of 256, ranked by ballots (bank_ranks); a survivor's row is its
// source row as it stands, or left + (right - left) * (k / (m + 1)) of the five float columns, every operation rounded
// once, with the id and the label of the left row.
__global__ __launch_bounds__(256) void fg_write_kernel(const float *__restrict__ rows_f, const int64_t *__restrict__ rows_i,
                                                       int W, const int32_t *__restrict__ cell,
                                                       const int32_t *__restrict__ right, const int32_t *__restrict__ offs,
                                                       int n_ids, int n_frames, float *__restrict__ out_f,
                                                       int64_t *__restrict__ out_i, int capacity) {
#pragma clang fp contract(off)
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long sf = blockIdx.x, seq = sf / n_frames, frame = sf % n_frames;
    const long first = seq * n_ids * n_frames + frame, start = offs[sf];
    int base = 0;
    for (int id0 = 0; id0 < n_ids; id0 += 256) {    // (n_ids is uniform: every thread makes every trip)
        const int id = id0 + (int)threadIdx.x;
        const long c = first + (long)id * n_frames;
        const int v = id < n_ids ? cell[c] : -1;
        int before, total;
        bank_ranks<4>(v != -1, lane, wave, wave_total, before, total);
        const long pos = start + base + before;
        if (v != -1 && pos < capacity) {
            float *of = out_f + pos * 5;
            int64_t *oi = out_i + pos * W;
            if (v >= 0) {
                for (int j = 0; j < 5; ++j) of[j] = rows_f[(long)v * 5 + j];
                for (int j = 0; j < W; ++j) oi[j] = rows_i[(long)v * W + j];
            } else {
                const long l = -(v + 2), r = right[c];
                const int64_t *li = rows_i + l * W, *ri = rows_i + r * W;
                const int64_t f0 = li[W - 3], f1 = ri[W - 3];
                const float t = (float)(int)(frame - f0) / (float)(int)(f1 - f0);
                for (int j = 0; j < 5; ++j) {       // (contract(off): the product rounds before the sum)
                    const float a = rows_f[l * 5 + j], b = rows_f[r * 5 + j];
                    of[j] = a + (b - a) * t;
                }
                if (W == 4) oi[0] = seq;
                oi[W - 3] = frame, oi[W - 2] = li[W - 2], oi[W - 1] = li[W - 1];
            }
        }
        base += total;
        __syncthreads();                            // wave_total is written again by the next chunk
    }
}

extern "C" {

int clipops_abi_version(void) { return CLIPOPS_ABI_VERSION; }

long clipops_fill_gaps_workspace(int n_seq, int n_ids, int n_frames) {
    if (n_seq < 0 || n_ids < 0 || n_frames < 0) return -1;
    const __int128 cells = (__int128)n_seq * n_ids * n_frames;
    if (cells > 0x7fffffffL) return -2;
    return 2 * (long)cells + (long)n_seq * n_frames;
}

int clipops_fill_gaps_f32(const float *rows_f, const int64_t *rows_i, const int32_t *counters, int n, int W, int n_seq,
                          int n_ids, int n_frames, int max_gap, int min_length, int32_t *workspace, float *out_f,
                          int64_t *out_i, int32_t *out_counters, int32_t *status, int capacity, void *stream) {
    if (n < 0 || n_seq < 0 || n_ids < 0 || n_frames < 0 || capacity < 0)
        return fail(1, "clipops_fill_gaps_f32: negative size");
    if (max_gap < 0 || min_length < 0) return fail(1, "clipops_fill_gaps_f32: negative max_gap or min_length");
    if (W != 3 && W != 4) return fail(1, "clipops_fill_gaps_f32: W is 3 (frame, id, label) or 4 (sequence, frame, id, label)");
    if (W == 3 && n_seq > 1) return fail(1, "clipops_fill_gaps_f32: rows without a sequence column take n_seq <= 1");
    if (n == 0) { g_err[0] = 0; return 0; }
    const long words = clipops_fill_gaps_workspace(n_seq, n_ids, n_frames);
    if (words == -2) return fail(2, "clipops_fill_gaps_f32: more than 2^31 - 1 cells");
    if (!rows_f || !rows_i || !counters || !out_counters || !status || (words > 0 && !workspace) ||
        (capacity > 0 && (!out_f || !out_i)))
        return fail(1, "clipops_fill_gaps_f32: null pointer");
    const hipStream_t s = (hipStream_t)stream;
    const long n_sf = (long)n_seq * n_frames, cells = n_sf * n_ids;
    int32_t *cell = workspace, *right = workspace + cells, *offs = workspace + 2 * cells;
    if (cells > 0) {
        hipLaunchKernelGGL(fg_clear_kernel, dim3(grid_for(cells)), dim3(256), 0, s, cell, cells);
        if (check_launch("fg_clear_kernel")) return 3;
    }
    // (without a cell every stored row is out of range: the scatter alone says so)
    hipLaunchKernelGGL(fg_scatter_kernel, dim3(grid_for(n)), dim3(256), 0, s, rows_i, counters, n, W, n_seq, n_ids, n_frames,
                       cell, status);
    if (check_launch("fg_scatter_kernel")) return 3;
    if (cells == 0) return 0;
    hipLaunchKernelGGL(fg_track_kernel, dim3((unsigned)(n_seq * (long)n_ids)), dim3(FG_THREADS), 0, s, cell, right, n_frames,
                       max_gap, min_length);
    if (check_launch("fg_track_kernel")) return 3;
    hipLaunchKernelGGL(fg_count_kernel, dim3((unsigned)((n_sf + 255) / 256)), dim3(256), 0, s, cell, n_sf, n_ids, n_frames,
                       offs);
    if (check_launch("fg_count_kernel")) return 3;
    hipLaunchKernelGGL(fg_scan_kernel, dim3(1), dim3(FG_THREADS), 0, s, offs, n_sf, out_counters, capacity);
    if (check_launch("fg_scan_kernel")) return 3;
    hipLaunchKernelGGL(fg_write_kernel, dim3((unsigned)n_sf), dim3(256), 0, s, rows_f, rows_i, W, cell, right, offs, n_ids,
                       n_frames, out_f, out_i, capacity);
    return check_launch("fg_write_kernel") ? 3 : 0;
}

int clipops_draw_table_f32(const float *boxes, const float *scores, const int64_t *ids, int B, int cap, int K,
                           const float *ori_wh, float score_thresh, float area_thresh, int bgr, int font_scale,
                           int32_t *table, void *stream) {
    if (B < 0 || cap < 0) return fail(1, "clipops_draw_table_f32: negative size");
    if (K < 1) return fail(1, "clipops_draw_table_f32: K < 1");
    if (font_scale < 1 || font_scale > 64) return fail(1, "clipops_draw_table_f32: font_scale outside 1 .. 64");
    if ((long)B * cap > 0x7fffffffL) return fail(1, "clipops_draw_table_f32: more than 2^31 - 1 slots");
    if ((long)B * cap == 0) { g_err[0] = 0; return 0; }
    if (!boxes || !scores || !ids || !ori_wh || !table) return fail(1, "clipops_draw_table_f32: null pointer");
    hipLaunchKernelGGL(draw_table_kernel, dim3(B), dim3(BANK_THREADS), 0, (hipStream_t)stream, boxes, scores, ids, cap, K,
                       ori_wh, score_thresh, area_thresh, bgr ? 1 : 0, font_scale, table);
    return check_launch("draw_table_kernel") ? 3 : 0;
}

int clipops_bank_update_f32(const clipops_bank_model *model, const clipops_bank *bank, int B, int n_det, int cap, int K,
                            int C, int use_dab, float det_score_thresh, float track_score_thresh,
                            int64_t miss_tolerance, void *stream) {
    if (B < 0 || n_det < 0 || cap < 0) return fail(1, "clipops_bank_update_f32: negative size");
    if (K < 1 || C < 1) return fail(1, "clipops_bank_update_f32: K < 1 or C < 1");
    if (cap < 1) return fail(1, "clipops_bank_update_f32: a bank without slots");
    if (B == 0) { g_err[0] = 0; return 0; }
    if (!model || !bank) return fail(1, "clipops_bank_update_f32: null pointer");
    for (int i = 0; i < CLIPOPS_BK_N_MODEL; ++i) {
        if (!model->ptr[i]) return fail(1, "clipops_bank_update_f32: null model pointer");
        if (model->row_stride[i] < 0 || model->batch_stride[i] < 0)
            return fail(1, "clipops_bank_update_f32: negative stride");
    }
    if (!use_dab && (!model->det_embed || model->det_row_stride < 0))
        return fail(1, "clipops_bank_update_f32: det_embed is required without DAB");
    if (!bank->ids || !bank->labels || !bank->disappear_time || !bank->boxes || !bank->ref_pts || !bank->logits ||
        !bank->scores || !bank->output_embed || !bank->long_memory || !bank->last_output || !bank->query_embed ||
        !bank->next_id || !bank->counters || !bank->free_list)
        return fail(1, "clipops_bank_update_f32: null bank pointer");
    hipLaunchKernelGGL(bank_update_kernel, dim3(B), dim3(BANK_THREADS), 0, (hipStream_t)stream, *model, *bank, n_det, cap, K, C,
                       use_dab, det_score_thresh, track_score_thresh, miss_tolerance);
    return check_launch("bank_update_kernel") ? 3 : 0;
}

int clipops_bank_result_rows_f32(const float *boxes, const float *scores, const int64_t *ids, const int64_t *labels,
                                 int B, int cap, int K, const int64_t *seq_frame, const float *ori_wh,
                                 float score_thresh, float area_thresh, float *rows_f, int64_t *rows_i,
                                 int32_t *counters, int capacity, void *stream) {
    if (B < 0 || cap < 0 || capacity < 0) return fail(1, "clipops_bank_result_rows_f32: negative size");
    if (K < 1) return fail(1, "clipops_bank_result_rows_f32: K < 1");
    if ((long)B * cap > 0x7fffffffL) return fail(1, "clipops_bank_result_rows_f32: more than 2^31 - 1 slots");
    if ((long)B * cap == 0) { g_err[0] = 0; return 0; }
    if (!boxes || !scores || !ids || !labels || !seq_frame || !ori_wh || !counters ||
        (capacity > 0 && (!rows_f || !rows_i)))
        return fail(1, "clipops_bank_result_rows_f32: null pointer");
    hipLaunchKernelGGL(bank_result_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, boxes, scores, ids, labels,
                       B * cap, cap, K, seq_frame, ori_wh, score_thresh, area_thresh, rows_f, rows_i, counters, capacity);
    return check_launch("bank_result_rows_kernel") ? 3 : 0;
}

int clipops_result_rows_f32(const float *boxes, const float *scores, const int64_t *ids, const int64_t *labels, int n,
                            int K, int64_t frame, float ori_w, float ori_h, float score_thresh, float area_thresh,
                            float *rows_f, int64_t *rows_i, int32_t *counters, int capacity, void *stream) {
    if (n < 0 || capacity < 0) return fail(1, "clipops_result_rows_f32: negative size");
    if (K < 1) return fail(1, "clipops_result_rows_f32: K < 1");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!boxes || !scores || !ids || !labels || !counters || (capacity > 0 && (!rows_f || !rows_i)))
        return fail(1, "clipops_result_rows_f32: null pointer");
    hipLaunchKernelGGL(result_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, boxes, scores, ids, labels, n, K,
                       frame, ori_w, ori_h, score_thresh, area_thresh, rows_f, rows_i, counters, capacity);
    return check_launch("result_rows_kernel") ? 3 : 0;
}

const char *clipops_last_error(void) { return g_err; }

int clipops_match_cost_f32(const float *logits, long logit_sl, long logit_sq, const float *boxes, long box_sl,
                           long box_sq, const int64_t *gt_labels, const float *gt_boxes, int n_layers, int Q, int K,
                           int T, float w_class, float w_bbox, float w_giou, float *cost, void *stream) {
    if (n_layers < 0 || Q < 0 || T < 0 || K <= 0) return fail(1, "clipops_match_cost_f32: bad dimension");
    if ((long)n_layers * Q * T == 0) { g_err[0] = 0; return 0; }
    if (!logits || !boxes || !gt_labels || !gt_boxes || !cost) return fail(1, "clipops_match_cost_f32: null pointer");
    hipLaunchKernelGGL(match_cost_kernel, dim3(grid_for((long)n_layers * Q * T)), dim3(256), 0, (hipStream_t)stream,
                       logits, logit_sl, logit_sq, boxes, box_sl, box_sq, gt_labels, gt_boxes, n_layers, Q, K, T,
                       w_class, w_bbox, w_giou, cost);
    return check_launch("match_cost_kernel");
}

int clipops_pair_box_loss_fwd_f32(const float *boxes, const int64_t *lay, const int64_t *qidx, long row_mul,
                                  long row_add, const float *tgt_boxes, const int64_t *gidx, const float *weight,
                                  int n, float *l1, float *giou_loss, void *stream) {
    if (n < 0) return fail(1, "clipops_pair_box_loss_fwd_f32: negative count");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!boxes || !lay || !qidx || !tgt_boxes || !l1 || !giou_loss)
        return fail(1, "clipops_pair_box_loss_fwd_f32: null pointer");
    hipLaunchKernelGGL(pair_box_loss_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, lay,
                       qidx, row_mul, row_add, tgt_boxes, gidx, weight, n, l1, giou_loss);
    return check_launch("pair_box_loss_fwd_kernel");
}

int clipops_pair_box_loss_bwd_f32(const float *boxes, const int64_t *lay, const int64_t *qidx, long row_mul,
                                  long row_add, const float *tgt_boxes, const int64_t *gidx, const float *weight,
                                  int n, const float *grad_l1, const float *grad_giou, float *grad_boxes,
                                  void *stream) {
    if (n < 0) return fail(1, "clipops_pair_box_loss_bwd_f32: negative count");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!boxes || !lay || !qidx || !tgt_boxes || !grad_l1 || !grad_giou || !grad_boxes)
        return fail(1, "clipops_pair_box_loss_bwd_f32: null pointer");
    hipLaunchKernelGGL(pair_box_loss_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, lay,
                       qidx, row_mul, row_add, tgt_boxes, gidx, weight, n, grad_l1, grad_giou, grad_boxes);
    return check_launch("pair_box_loss_bwd_kernel");
}

int clipops_track_ownership_i64(const int64_t *track_ids, int n_tracks, const int64_t *gt_ids, int n_gt,
                                int64_t *matched_idx, float *gt_free, void *stream) {
    if (n_tracks < 0 || n_gt < 0) return fail(1, "clipops_track_ownership_i64: negative count");
    if (n_tracks + n_gt == 0) { g_err[0] = 0; return 0; }
    if ((n_tracks > 0 && (!track_ids || !matched_idx)) || (n_gt > 0 && (!gt_ids || !gt_free)))
        return fail(1, "clipops_track_ownership_i64: null pointer");
    hipLaunchKernelGGL(track_ownership_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, track_ids, n_tracks, gt_ids,
                       n_gt, matched_idx, gt_free);
    return check_launch("track_ownership_kernel");
}

int clipops_focal_labels_i64(const int64_t *lay, const int64_t *q, const int64_t *g, int n_pairs,
                             const int64_t *gt_labels, int n_gt, const int64_t *matched_idx, int n_tracks,
                             const uint8_t *late, int n_layers, int n_det, int K, int64_t *labels, void *stream) {
    if (n_pairs < 0 || n_gt < 0 || n_tracks < 0 || n_layers < 0 || n_det < 0) return fail(1, "clipops_focal_labels_i64: negative count");
    if ((long)n_layers * (n_det + n_tracks) == 0) { g_err[0] = 0; return 0; }
    if (!labels || !late || (n_pairs > 0 && (!lay || !q || !g || !gt_labels)) || (n_tracks > 0 && !matched_idx) ||
        (n_gt > 0 && !gt_labels))
        return fail(1, "clipops_focal_labels_i64: null pointer");
    hipLaunchKernelGGL(focal_labels_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lay, q, g, n_pairs, gt_labels, n_gt,
                       matched_idx, n_tracks, late, n_layers, n_det, K, labels);
    return check_launch("focal_labels_kernel");
}

int clipops_pair_iou_f32(const float *boxes, const float *tgt_boxes, const int64_t *gidx, int n, float *iou,
                         void *stream) {
    if (n < 0) return fail(1, "clipops_pair_iou_f32: negative count");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!boxes || !tgt_boxes || !iou) return fail(1, "clipops_pair_iou_f32: null pointer");
    hipLaunchKernelGGL(pair_iou_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, tgt_boxes,
                       gidx, n, iou);
    return check_launch("pair_iou_kernel");
}

int clipops_handover_fwd_f32(const clipops_handover_sources *src, const int64_t *prev_ids, const int64_t *prev_matched,
                             const float *gt_boxes, const int64_t *gt_ids, const int64_t *table, int n_keep, int n_det,
                             int n_tracks, int n_gt, int K, int C, int use_dab, float *base, int64_t *ids,
                             int64_t *matched_idx, void *stream) {
    if (n_keep < 0 || n_det < 0 || n_tracks < 0 || n_gt < 0) return fail(1, "clipops_handover_fwd_f32: negative size");
    if (K < 1 || C < 1) return fail(1, "clipops_handover_fwd_f32: K < 1 or C < 1");
    if (n_keep == 0) { g_err[0] = 0; return 0; }
    if (!src || !table || !base || !ids || !matched_idx || (n_gt > 0 && (!gt_boxes || !gt_ids)))
        return fail(1, "clipops_handover_fwd_f32: null pointer");
    for (int i = 0; i < CLIPOPS_HO_N_SOURCES; ++i) {
        const bool prev = i >= CLIPOPS_HO_PREV_REF;
        const bool needed = prev ? n_tracks > 0 : (i == CLIPOPS_HO_DET_EMBED ? (!use_dab && n_det > 0) : n_det + n_tracks > 0);
        if (needed && !src->ptr[i]) return fail(1, "clipops_handover_fwd_f32: null source pointer");
        if (needed && src->row_stride[i] < 0) return fail(1, "clipops_handover_fwd_f32: negative row stride");
    }
    if (n_tracks > 0 && (!prev_ids || !prev_matched)) return fail(1, "clipops_handover_fwd_f32: null pointer");
    hipLaunchKernelGGL(handover_fwd_kernel, dim3(n_keep), dim3(256), 0, (hipStream_t)stream, *src, prev_ids,
                       prev_matched, gt_boxes, gt_ids, table, n_det, n_tracks, n_gt, use_dab,
                       handover_cols(K, C, use_dab), base, ids, matched_idx);
    return check_launch("handover_fwd_kernel");
}

int clipops_handover_bwd_f32(const float *grad_base, const int64_t *table, const int64_t *inv_q, const int64_t *inv_prev,
                             int n_keep, int n_q, int n_det, int n_tracks, int K, int C, int use_dab, int det_cols,
                             const clipops_handover_grads *grad, void *stream) {
    if (n_keep < 0 || n_q < 0 || n_det < 0 || n_tracks < 0) return fail(1, "clipops_handover_bwd_f32: negative size");
    if (K < 1 || C < 1) return fail(1, "clipops_handover_bwd_f32: K < 1 or C < 1");
    if ((long)n_det + n_tracks > n_q) return fail(1, "clipops_handover_bwd_f32: n_q < n_det + n_tracks");
    if (n_q + n_tracks == 0) { g_err[0] = 0; return 0; }
    if (!grad || !inv_q || (n_tracks > 0 && !inv_prev) || (n_keep > 0 && (!grad_base || !table)))
        return fail(1, "clipops_handover_bwd_f32: null pointer");
    if (grad->ptr[CLIPOPS_HO_LOGITS] || grad->ptr[CLIPOPS_HO_BOXES] || grad->ptr[CLIPOPS_HO_PREV_IOU])
        return fail(1, "clipops_handover_bwd_f32: logits, boxes and iou take no gradient");
    if (grad->ptr[CLIPOPS_HO_DET_EMBED] && (use_dab || det_cols < C))
        return fail(1, "clipops_handover_bwd_f32: det_embed gradient under DAB or narrower than C");
    hipLaunchKernelGGL(handover_bwd_kernel, dim3(n_q + n_tracks), dim3(256), 0, (hipStream_t)stream, grad_base, table,
                       inv_q, inv_prev, n_keep, n_q, n_det, n_tracks, use_dab, det_cols, handover_cols(K, C, use_dab),
                       *grad);
    return check_launch("handover_bwd_kernel");
}

int clipops_focal_fwd_f32(const float *logits, long sl, long sq, const int64_t *labels, int n_layers, int Nq, int K,
                          float alpha, float gamma, float *loss, void *stream) {
    if (n_layers < 0 || Nq < 0 || K <= 0) return fail(1, "clipops_focal_fwd_f32: bad dimension");
    if (n_layers == 0) { g_err[0] = 0; return 0; }
    if (!loss || (Nq > 0 && (!logits || !labels))) return fail(1, "clipops_focal_fwd_f32: null pointer");
    hipLaunchKernelGGL(focal_fwd_kernel, dim3(n_layers), dim3(256), 0, (hipStream_t)stream, logits, sl, sq, labels, Nq,
                       K, alpha, gamma, loss);
    return check_launch("focal_fwd_kernel");
}

int clipops_focal_bwd_f32(const float *logits, long sl, long sq, const int64_t *labels, int n_layers, int Nq, int K,
                          float alpha, float gamma, const float *grad_loss, float *grad_logits, void *stream) {
    if (n_layers < 0 || Nq < 0 || K <= 0) return fail(1, "clipops_focal_bwd_f32: bad dimension");
    if ((long)n_layers * Nq == 0) { g_err[0] = 0; return 0; }
    if (!logits || !labels || !grad_loss || !grad_logits) return fail(1, "clipops_focal_bwd_f32: null pointer");
    hipLaunchKernelGGL(focal_bwd_kernel, dim3(grid_for((long)n_layers * Nq * K)), dim3(256), 0, (hipStream_t)stream,
                       logits, sl, sq, labels, n_layers, Nq, K, alpha, gamma, grad_loss, grad_logits);
    return check_launch("focal_bwd_kernel");
}

int clipops_sine_embed_fwd_f32(const float *pos, const float *dim_t, long n, int K, int F, float scale, float *out,
                               void *stream) {
    if (n < 0 || K <= 0 || F <= 0) return fail(1, "clipops_sine_embed_fwd_f32: bad dimension");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!pos || !dim_t || !out) return fail(1, "clipops_sine_embed_fwd_f32: null pointer");
    hipLaunchKernelGGL(sine_embed_fwd_kernel, dim3(grid_for(n * K * F)), dim3(256), 0, (hipStream_t)stream, pos, dim_t,
                       n, K, F, scale, out);
    return check_launch("sine_embed_fwd_kernel");
}

int clipops_sine_embed_bwd_f32(const float *pos, const float *dim_t, long n, int K, int F, float scale,
                               const float *grad_out, float *grad_pos, void *stream) {
    if (n < 0 || K <= 0 || F <= 0) return fail(1, "clipops_sine_embed_bwd_f32: bad dimension");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!pos || !dim_t || !grad_out || !grad_pos) return fail(1, "clipops_sine_embed_bwd_f32: null pointer");
    hipLaunchKernelGGL(sine_embed_bwd_kernel, dim3(grid_for(n * K * 64)), dim3(256), 0, (hipStream_t)stream, pos,
                       dim_t, n, K, F, scale, grad_out, grad_pos);
    return check_launch("sine_embed_bwd_kernel");
}

int clipops_inverse_sigmoid_fwd_f32(const float *x, long n, float eps, float *y, void *stream) {
    if (n < 0) return fail(1, "clipops_inverse_sigmoid_fwd_f32: negative count");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!x || !y) return fail(1, "clipops_inverse_sigmoid_fwd_f32: null pointer");
    hipLaunchKernelGGL(inverse_sigmoid_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, n, eps, y);
    return check_launch("inverse_sigmoid_fwd_kernel");
}

int clipops_inverse_sigmoid_bwd_f32(const float *x, const float *grad_y, long n, float eps, float *grad_x,
                                    void *stream) {
    if (n < 0) return fail(1, "clipops_inverse_sigmoid_bwd_f32: negative count");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!x || !grad_y || !grad_x) return fail(1, "clipops_inverse_sigmoid_bwd_f32: null pointer");
    hipLaunchKernelGGL(inverse_sigmoid_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, grad_y, n,
                       eps, grad_x);
    return check_launch("inverse_sigmoid_bwd_kernel");
}

int clipops_refine_boxes_fwd_f32(const float *delta, const float *ref, long n, float eps, float *out, void *stream) {
    if (n < 0) return fail(1, "clipops_refine_boxes_fwd_f32: negative count");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!delta || !ref || !out) return fail(1, "clipops_refine_boxes_fwd_f32: null pointer");
    hipLaunchKernelGGL(refine_boxes_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, delta, ref, n,
                       eps, out);
    return check_launch("refine_boxes_fwd_kernel");
}

int clipops_refine_boxes_split_fwd_f32(const float *delta, const float *ref, long n_rows, float eps, float *out_head,
                                       float *out_dec, void *stream) {
    if (n_rows < 0) return fail(1, "clipops_refine_boxes_split_fwd_f32: negative count");
    if (n_rows == 0) { g_err[0] = 0; return 0; }
    if (!delta || !ref || !out_head || !out_dec) return fail(1, "clipops_refine_boxes_split_fwd_f32: null pointer");
    if (out_head == out_dec) return fail(1, "clipops_refine_boxes_split_fwd_f32: the two outputs alias");
    const bool vec = (((uintptr_t)delta | (uintptr_t)ref | (uintptr_t)out_head | (uintptr_t)out_dec) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(refine_boxes_split_fwd_kernel<true>, dim3(grid_for(n_rows)), dim3(256), 0,
                           (hipStream_t)stream, delta, ref, n_rows, eps, out_head, out_dec);
    else
        hipLaunchKernelGGL(refine_boxes_split_fwd_kernel<false>, dim3(grid_for(n_rows)), dim3(256), 0,
                           (hipStream_t)stream, delta, ref, n_rows, eps, out_head, out_dec);
    return check_launch("refine_boxes_split_fwd_kernel");
}

int clipops_refine_boxes_bwd_f32(const float *out, const float *ref, const float *grad_out, long n, float eps,
                                 float *grad_delta, float *grad_ref, void *stream) {
    if (n < 0) return fail(1, "clipops_refine_boxes_bwd_f32: negative count");
    if (n == 0) { g_err[0] = 0; return 0; }
    if (!out || !ref || !grad_out || !grad_delta) return fail(1, "clipops_refine_boxes_bwd_f32: null pointer");
    hipLaunchKernelGGL(refine_boxes_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, out, ref,
                       grad_out, n, eps, grad_delta, grad_ref);
    return check_launch("refine_boxes_bwd_kernel");
}

int clipops_colsum_f32(const float *x, long rows, int cols, float *out, void *stream) {
    if (rows < 0 || cols < 0) return fail(1, "clipops_colsum_f32: bad dimension");
    if (cols == 0) { g_err[0] = 0; return 0; }
    if (!out || (rows > 0 && !x)) return fail(1, "clipops_colsum_f32: null pointer");
    if (cols % 4 == 0 && rows <= 2048 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(colsum_quad_kernel, dim3(cols / 4), dim3(256), 0, (hipStream_t)stream, x, rows, cols, out);
        return check_launch("colsum_quad_kernel");
    }
    hipLaunchKernelGGL(colsum_kernel, dim3((cols + 31) / 32), dim3(256), 0, (hipStream_t)stream, x, rows, cols, out);
    return check_launch("colsum_kernel");
}

int clipops_colsum_partial_f32(const float *x, long rows, int cols, int chunk_rows, float *partial, void *stream) {
    if (rows < 0 || cols < 0 || chunk_rows <= 0) return fail(1, "clipops_colsum_partial_f32: bad dimension");
    if (cols == 0 || rows == 0) { g_err[0] = 0; return 0; }
    if (!x || !partial) return fail(1, "clipops_colsum_partial_f32: null pointer");
    const long chunks = (rows + chunk_rows - 1) / chunk_rows;
    if (chunks > 65535) return fail(1, "clipops_colsum_partial_f32: too many chunks");
    hipLaunchKernelGGL(colsum_partial_kernel<float>, dim3((cols + 31) / 32, (unsigned)chunks), dim3(256), 0,
                       (hipStream_t)stream, x, rows, cols, chunk_rows, partial);
    return check_launch("colsum_partial_kernel");
}

int clipops_colsum_partial_bf16(const uint16_t *x, long rows, int cols, int chunk_rows, float *partial, void *stream) {
    if (rows < 0 || cols < 0 || chunk_rows <= 0) return fail(1, "clipops_colsum_partial_bf16: bad dimension");
    if (cols == 0 || rows == 0) { g_err[0] = 0; return 0; }
    if (!x || !partial) return fail(1, "clipops_colsum_partial_bf16: null pointer");
    const long chunks = (rows + chunk_rows - 1) / chunk_rows;
    if (chunks > 65535) return fail(1, "clipops_colsum_partial_bf16: too many chunks");
    hipLaunchKernelGGL(colsum_partial_kernel<uint16_t>, dim3((cols + 31) / 32, (unsigned)chunks), dim3(256), 0,
                       (hipStream_t)stream, x, rows, cols, chunk_rows, partial);
    return check_launch("colsum_partial_kernel<bf16>");
}

static int relu_bwd_colsum_check(const void *g, const void *y, const void *g2, const void *partial, long rows, int cols,
                                 int chunk_rows, long *chunks) {
    if (rows < 0 || cols < 0 || chunk_rows <= 0) return fail(1, "clipops_relu_bwd_colsum_partial: bad dimension");
    *chunks = (rows + chunk_rows - 1) / chunk_rows;
    if (cols == 0 || rows == 0) return 0;
    if (!g || !y || !g2 || !partial) return fail(1, "clipops_relu_bwd_colsum_partial: null pointer");
    if (*chunks > 65535) return fail(1, "clipops_relu_bwd_colsum_partial: too many chunks");
    return 0;
}

int clipops_relu_bwd_colsum_partial_f32(const float *g, const float *y, long rows, int cols, int chunk_rows, float *g2,
                                        float *partial, void *stream) {
    long chunks = 0;
    if (relu_bwd_colsum_check(g, y, g2, partial, rows, cols, chunk_rows, &chunks)) return 1;
    if (cols == 0 || rows == 0) { g_err[0] = 0; return 0; }
    hipLaunchKernelGGL(relu_bwd_colsum_partial_kernel<float>, dim3((cols + 31) / 32, (unsigned)chunks), dim3(256), 0,
                       (hipStream_t)stream, g, y, rows, cols, chunk_rows, g2, partial);
    return check_launch("relu_bwd_colsum_partial_kernel");
}

int clipops_mha_fwd_f32(const float *q, const float *k, const float *v, long q_bs, long q_rs, long k_bs, long k_rs,
                        long v_bs, long v_rs, const uint8_t *key_mask, int B, int H, int L, float scale, float *out,
                        float *lse, void *stream) {
    int rc = mha_check(q, k, v, B, H, L);
    if (rc) return rc;
    if ((long)B * L == 0) { g_err[0] = 0; return 0; }
    if (!out || !lse) return fail(1, "clipops_mha_fwd_f32: null pointer");
    const size_t lds = (size_t)2 * L * kPitch * sizeof(float);
    if ((rc = allow_lds(reinterpret_cast<const void *>(mha_fwd_kernel), lds, g_lds_fwd))) return rc;
    hipLaunchKernelGGL(mha_fwd_kernel, dim3((L + kRows - 1) / kRows, H, B), dim3(256), lds, (hipStream_t)stream, q, k, v, q_bs,
                       q_rs, k_bs, k_rs, v_bs, v_rs, key_mask, H, L, scale, out, lse);
    return check_launch("mha_fwd_kernel");
}

int clipops_mha_bwd_f32(const float *q, const float *k, const float *v, long q_bs, long q_rs, long k_bs, long k_rs,
                        long v_bs, long v_rs, const uint8_t *key_mask, const float *out, const float *lse,
                        const float *grad_out, int B, int H, int L, float scale, float *grad_q, long gq_bs, long gq_rs,
                        float *grad_k, long gk_bs, long gk_rs, float *grad_v, long gv_bs, long gv_rs, void *stream) {
    int rc = mha_check(q, k, v, B, H, L);
    if (rc) return rc;
    if ((long)B * L == 0) { g_err[0] = 0; return 0; }
    if (!out || !lse || !grad_out || !grad_q || !grad_k || !grad_v) return fail(1, "clipops_mha_bwd_f32: null pointer");
    const size_t lds_q = (size_t)2 * L * kPitch * sizeof(float);
    const size_t lds_kv = lds_q + (size_t)2 * L * sizeof(float);
    if ((rc = allow_lds(reinterpret_cast<const void *>(mha_bwd_q_kernel), lds_q, g_lds_bq))) return rc;
    if ((rc = allow_lds(reinterpret_cast<const void *>(mha_bwd_kv_kernel), lds_kv, g_lds_bkv))) return rc;
    const dim3 grid((L + kRows - 1) / kRows, H, B);
    hipLaunchKernelGGL(mha_bwd_q_kernel, grid, dim3(256), lds_q, (hipStream_t)stream, q, k, v, q_bs, q_rs, k_bs, k_rs,
                       v_bs, v_rs, key_mask, out, lse, grad_out, H, L, scale, grad_q, gq_bs, gq_rs);
    if ((rc = check_launch("mha_bwd_q_kernel"))) return rc;
    hipLaunchKernelGGL(mha_bwd_kv_kernel, grid, dim3(256), lds_kv, (hipStream_t)stream, q, k, v, q_bs, q_rs, k_bs, k_rs,
                       v_bs, v_rs, key_mask, out, lse, grad_out, H, L, scale, grad_k, gk_bs, gk_rs, grad_v, gv_bs, gv_rs);
    return check_launch("mha_bwd_kv_kernel");
}

int clipops_add_layer_norm_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta, long rows,
                                   float eps, float *sum, float *y, float *stats, void *stream) {
    if (rows < 0) return fail(1, "clipops_add_layer_norm_fwd_f32: negative row count");
    if (rows == 0) { g_err[0] = 0; return 0; }
    if (!x || !res || !gamma || !beta || !sum || !y || !stats) return fail(1, "clipops_add_layer_norm_fwd_f32: null pointer");
    hipLaunchKernelGGL(add_layer_norm_fwd_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       x, res, gamma, beta, nullptr, rows, eps, sum, y, nullptr, stats);
    return check_launch("add_layer_norm_fwd_kernel");
}

int clipops_add_layer_norm_pos_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta,
                                       const float *pos, long rows, float eps, float *sum, float *y, float *q,
                                       float *stats, void *stream) {
    if (rows < 0) return fail(1, "clipops_add_layer_norm_pos_fwd_f32: negative row count");
    if (rows == 0) { g_err[0] = 0; return 0; }
    if (!x || !res || !gamma || !beta || !pos || !sum || !y || !q || !stats)
        return fail(1, "clipops_add_layer_norm_pos_fwd_f32: null pointer");
    hipLaunchKernelGGL(add_layer_norm_fwd_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       x, res, gamma, beta, pos, rows, eps, sum, y, q, stats);
    return check_launch("add_layer_norm_fwd_kernel<pos>");
}

int clipops_add_layer_norm_bwd_f32(const float *grad_y, const float *sum, const float *stats, const float *gamma,
                                   long rows, int chunk_rows, float *grad_sum, float *partial, void *stream) {
    if (rows < 0 || chunk_rows <= 0) return fail(1, "clipops_add_layer_norm_bwd_f32: bad dimension");
    if (rows == 0) { g_err[0] = 0; return 0; }
    if (!grad_y || !sum || !stats || !gamma || !grad_sum || !partial)
        return fail(1, "clipops_add_layer_norm_bwd_f32: null pointer");
    hipLaunchKernelGGL(add_layer_norm_bwd_kernel, dim3((unsigned)((rows + chunk_rows - 1) / chunk_rows)), dim3(256), 0,
                       (hipStream_t)stream, grad_y, sum, stats, gamma, rows, chunk_rows, grad_sum, partial);
    return check_launch("add_layer_norm_bwd_kernel");
}

int clipops_add_layer_norm_fanin_bwd_f32(const float *g0, const float *g1, const float *g2, const float *sum,
                                         const float *stats, const float *gamma, long rows, int chunk_rows,
                                         float *grad_sum, float *partial, float *colsum_partial, void *stream) {
    if (rows < 0 || chunk_rows <= 0) return fail(1, "clipops_add_layer_norm_fanin_bwd_f32: bad dimension");
    if (rows == 0) { g_err[0] = 0; return 0; }
    const float *g[3] = {nullptr, nullptr, nullptr};      // the non-null slots, in slot order
    int n = 0;
    if (g0) g[n++] = g0;
    if (g1) g[n++] = g1;
    if (g2) g[n++] = g2;
    if (n == 0) return fail(1, "clipops_add_layer_norm_fanin_bwd_f32: no gradient input");
    if (!sum || !stats || !gamma || !grad_sum || !partial || !colsum_partial)
        return fail(1, "clipops_add_layer_norm_fanin_bwd_f32: null pointer");
    hipLaunchKernelGGL(add_layer_norm_bwd_fanin_kernel, dim3((unsigned)((rows + chunk_rows - 1) / chunk_rows)), dim3(256), 0,
                       (hipStream_t)stream, g[0], g[1], g[2], sum, stats, gamma, rows, chunk_rows, grad_sum, partial,
                       colsum_partial);
    return check_launch("add_layer_norm_bwd_fanin_kernel");
}

int clipops_assign_f32(const float *cost, long stride_problem, long stride_row, long stride_col, int n_problems,
                       int n_rows, int n_cols, int32_t *row_ind, int32_t *col_ind, int32_t *status, void *stream) {
    if (n_problems < 0 || n_rows < 0 || n_cols < 0) return fail(1, "clipops_assign_f32: bad dimension");
    if (n_problems == 0 || n_rows == 0 || n_cols == 0) { g_err[0] = 0; return 0; }
    if (!cost || !row_ind || !col_ind) return fail(1, "clipops_assign_f32: null pointer");
    const int nr = n_rows < n_cols ? n_rows : n_cols, nc = n_rows < n_cols ? n_cols : n_rows;
    if (nc > CLIPOPS_ASSIGN_MAX_DIM) return fail(2, "clipops_assign_f32: problem exceeds CLIPOPS_ASSIGN_MAX_DIM");
    const size_t lds = (assign::work_bytes(nr, nc) + 15) & ~(size_t)15;
    if (lds > 64 * 1024) {       // beyond the default limit of a launch: opt in (gfx950 has 160 KB per CU), once per process
        static std::atomic<size_t> allowed{0};
        if (lds > 160 * 1024) return fail(2, "clipops_assign_f32: problem does not fit the LDS of a CU");
        if (lds > allowed.load()) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(assign_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
                (void)hipGetLastError();
                return fail(3, "clipops_assign_f32: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
            }
            allowed.store(160 * 1024);
        }
    }
    hipLaunchKernelGGL(assign_kernel, dim3(n_problems), dim3(64), lds, (hipStream_t)stream, cost, stride_problem,
                       stride_row, stride_col, n_rows, n_cols, row_ind, col_ind, status);
    return check_launch("assign_kernel");
}

static int shift_relu_check(const void *x, const void *shift, long planes, int C, long HW, const char *who) {
    if (planes < 0 || C <= 0 || HW < 0) return fail(1, who);
    if (planes && HW && (!x || !shift)) return fail(1, who);
    return 0;
}

int clipops_shift_relu_f32(float *x, const float *shift, const float *res, long planes, int C, long HW, void *stream) {
    if (shift_relu_check(x, shift, planes, C, HW, "clipops_shift_relu_f32: bad argument")) return 1;
    if (planes == 0 || HW == 0) { g_err[0] = 0; return 0; }
    const int vec = (HW % 4 == 0) && ((uintptr_t)x % 16 == 0) && (!res || (uintptr_t)res % 16 == 0);
    const long per = vec ? HW / 4 : HW;
    const dim3 grid((unsigned)((per + 1023) / 1024 > 64 ? 64 : (per + 1023) / 1024 < 1 ? 1 : (per + 1023) / 1024),
                    (unsigned)(planes > 65535 ? 65535 : planes));
    if (res) hipLaunchKernelGGL(shift_relu_f32_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, shift, res, planes, C, HW, vec);
    else hipLaunchKernelGGL(shift_relu_f32_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, shift, res, planes, C, HW, vec);
    return check_launch("shift_relu_f32_kernel");
}

int clipops_shift_relu_bf16(uint16_t *x, const float *shift, const uint16_t *res, long planes, int C, long HW, void *stream) {
    if (shift_relu_check(x, shift, planes, C, HW, "clipops_shift_relu_bf16: bad argument")) return 1;
    if (planes == 0 || HW == 0) { g_err[0] = 0; return 0; }
    const int vec = (HW % 8 == 0) && ((uintptr_t)x % 16 == 0) && (!res || (uintptr_t)res % 16 == 0);
    const long per = vec ? HW / 8 : HW;
    const dim3 grid((unsigned)((per + 1023) / 1024 > 64 ? 64 : (per + 1023) / 1024 < 1 ? 1 : (per + 1023) / 1024),
                    (unsigned)(planes > 65535 ? 65535 : planes));
    if (res) hipLaunchKernelGGL(shift_relu_bf16_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, shift, res, planes, C, HW, vec);
    else hipLaunchKernelGGL(shift_relu_bf16_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, shift, res, planes, C, HW, vec);
    return check_launch("shift_relu_bf16_kernel");
}

int clipops_linear_bwd_f32(const float *grad_y, const float *y_relu, const float *x, const float *w, int rows,
                           int in_features, int out_features, float *grad_x, float *grad_w, float *grad_b,
                           void *stream) {
    if (rows < 0 || in_features <= 0 || out_features <= 0) return fail(1, "clipops_linear_bwd_f32: bad dimension");
    if (!grad_y || !x || !w) return fail(1, "clipops_linear_bwd_f32: null pointer");
    if (grad_b && !grad_w) return fail(1, "clipops_linear_bwd_f32: grad_b is computed with grad_w");
    const int gx_ti = (rows + 31) / 32, gx_tj = (in_features + 31) / 32;
    const int gw_ti = (out_features + 31) / 32, gw_tj = gx_tj;
    const int n_gx = grad_x ? gx_ti * gx_tj : 0, n_gw = grad_w ? gw_ti * gw_tj : 0;
    if (n_gx + n_gw == 0) { g_err[0] = 0; return 0; }
    if (rows == 0) {          // nothing to contract over: the weight and bias gradients are zero
        if (grad_w && hipMemsetAsync(grad_w, 0, sizeof(float) * (size_t)out_features * in_features, (hipStream_t)stream) != hipSuccess)
            return fail(3, "clipops_linear_bwd_f32: memset failed");
        if (grad_b && hipMemsetAsync(grad_b, 0, sizeof(float) * (size_t)out_features, (hipStream_t)stream) != hipSuccess)
            return fail(3, "clipops_linear_bwd_f32: memset failed");
        g_err[0] = 0;
        return 0;
    }
    if (linear_staged()) {
        static std::atomic<unsigned long long> done[4];
        const size_t lds = std::max(grad_x ? ls_bytes(true, false, out_features) : 0, grad_w ? ls_bytes(false, false, rows) : 0);
        const bool vec = in_features % 4 == 0 && out_features % 4 == 0 && aligned16(grad_y) && aligned16(x) &&
                         aligned16(w) && (!y_relu || aligned16(y_relu));
        const int which = (y_relu ? 2 : 0) + (vec ? 1 : 0);
        auto kernel = which == 3 ? linear_bwd_staged_kernel<true, true> : which == 2 ? linear_bwd_staged_kernel<true, false>
                      : which == 1 ? linear_bwd_staged_kernel<false, true> : linear_bwd_staged_kernel<false, false>;
        int rc;
        if ((rc = allow_lds(reinterpret_cast<const void *>(kernel), lds, done[which]))) return rc;
        hipLaunchKernelGGL(kernel, dim3(n_gx + n_gw), dim3(256), lds, (hipStream_t)stream, grad_y, y_relu, x, w, rows, in_features, out_features, grad_x, grad_w, grad_b, n_gx, gx_tj, gw_tj);
        return check_launch("linear_bwd_staged_kernel");
    }
    if (y_relu) hipLaunchKernelGGL(linear_bwd_kernel<true>, dim3(n_gx + n_gw), dim3(256), 0, (hipStream_t)stream, grad_y, y_relu, x, w, rows, in_features, out_features, grad_x, grad_w, grad_b, n_gx, gx_tj, gw_tj);
    else hipLaunchKernelGGL(linear_bwd_kernel<false>, dim3(n_gx + n_gw), dim3(256), 0, (hipStream_t)stream, grad_y, y_relu, x, w, rows, in_features, out_features, grad_x, grad_w, grad_b, n_gx, gx_tj, gw_tj);
    return check_launch("linear_bwd_kernel");
}

int clipops_linear_fwd_f32(const float *x, const float *w, const float *bias, int rows, int in_features,
                           int out_features, int relu, float *y, void *stream) {
    if (rows < 0 || in_features <= 0 || out_features <= 0) return fail(1, "clipops_linear_fwd_f32: bad dimension");
    if (in_features % 4) return fail(2, "clipops_linear_fwd_f32: in_features must be a multiple of 4");
    if (rows == 0) { g_err[0] = 0; return 0; }
    if (!x || !w || !y) return fail(1, "clipops_linear_fwd_f32: null pointer");
    const int ti = (rows + 31) / 32, tj = (out_features + 31) / 32;
    if (linear_staged()) {
        static std::atomic<unsigned long long> done[4];
        const size_t lds = ls_bytes(true, true, in_features);
        const bool vec = aligned16(x) && aligned16(w);
        const int which = (relu ? 2 : 0) + (vec ? 1 : 0);
        auto kernel = which == 3 ? linear_fwd_staged_kernel<true, true> : which == 2 ? linear_fwd_staged_kernel<true, false>
                      : which == 1 ? linear_fwd_staged_kernel<false, true> : linear_fwd_staged_kernel<false, false>;
        int rc;
        if ((rc = allow_lds(reinterpret_cast<const void *>(kernel), lds, done[which]))) return rc;
        hipLaunchKernelGGL(kernel, dim3(ti * tj), dim3(256), lds, (hipStream_t)stream, x, w, bias, rows, in_features, out_features, y, tj);
        return check_launch("linear_fwd_staged_kernel");
    }
    if (relu) hipLaunchKernelGGL(linear_fwd_kernel<true>, dim3(ti * tj), dim3(256), 0, (hipStream_t)stream, x, w, bias, rows, in_features, out_features, y, tj);
    else hipLaunchKernelGGL(linear_fwd_kernel<false>, dim3(ti * tj), dim3(256), 0, (hipStream_t)stream, x, w, bias, rows, in_features, out_features, y, tj);
    return check_launch("linear_fwd_kernel");
}

}  // extern "C"
