// clip_handover.h -- track hand-over between two frames: one gather kernel, one scatter kernel for its gradient.
// Included by clip_ops.hip after clip_common.h.
#pragma once

namespace {
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
}  // namespace

extern "C" {
int clipops_handover_fwd_f32(const clipops_handover_sources *src, const int64_t *prev_ids, const int64_t *prev_matched,
                             const float *gt_boxes, const int64_t *gt_ids, const int64_t *table, int n_keep, int n_det,
                             int n_tracks, int n_gt, int K, int C, int use_dab, float *base, int64_t *ids,
                             int64_t *matched_idx, void *stream) {
    if (n_keep < 0 || n_det < 0 || n_tracks < 0 || n_gt < 0) return fail(1, "clipops_handover_fwd_f32: negative size");
    if (K < 1 || C < 1) return fail(1, "clipops_handover_fwd_f32: K < 1 or C < 1");
    if (n_keep == 0) return ok();
    if (!src || !table || !base || !ids || !matched_idx || (n_gt > 0 && (!gt_boxes || !gt_ids)))
        return fail(1, "clipops_handover_fwd_f32: null pointer");
    for (int i = 0; i < CLIPOPS_HO_N_SOURCES; ++i) {
        const bool prev = i >= CLIPOPS_HO_PREV_REF;
        const bool needed = prev ? n_tracks > 0 : (i == CLIPOPS_HO_DET_EMBED ? (!use_dab && n_det > 0) : n_det + n_tracks > 0);
        if (needed && !src->ptr[i]) return fail(1, "clipops_handover_fwd_f32: null source pointer");
        if (needed && src->row_stride[i] < 0) return fail(1, "clipops_handover_fwd_f32: negative row stride");
    }
    if (n_tracks > 0 && (!prev_ids || !prev_matched)) return fail(1, "clipops_handover_fwd_f32: null pointer");
    return launch("handover_fwd_kernel", handover_fwd_kernel, dim3(n_keep), dim3(256), 0, stream, *src, prev_ids,
                  prev_matched, gt_boxes, gt_ids, table, n_det, n_tracks, n_gt, use_dab, handover_cols(K, C, use_dab), base,
                  ids, matched_idx);
}

int clipops_handover_bwd_f32(const float *grad_base, const int64_t *table, const int64_t *inv_q, const int64_t *inv_prev,
                             int n_keep, int n_q, int n_det, int n_tracks, int K, int C, int use_dab, int det_cols,
                             const clipops_handover_grads *grad, void *stream) {
    if (n_keep < 0 || n_q < 0 || n_det < 0 || n_tracks < 0) return fail(1, "clipops_handover_bwd_f32: negative size");
    if (K < 1 || C < 1) return fail(1, "clipops_handover_bwd_f32: K < 1 or C < 1");
    if ((long)n_det + n_tracks > n_q) return fail(1, "clipops_handover_bwd_f32: n_q < n_det + n_tracks");
    if (n_q + n_tracks == 0) return ok();
    if (!grad || !inv_q || (n_tracks > 0 && !inv_prev) || (n_keep > 0 && (!grad_base || !table)))
        return fail(1, "clipops_handover_bwd_f32: null pointer");
    if (grad->ptr[CLIPOPS_HO_LOGITS] || grad->ptr[CLIPOPS_HO_BOXES] || grad->ptr[CLIPOPS_HO_PREV_IOU])
        return fail(1, "clipops_handover_bwd_f32: logits, boxes and iou take no gradient");
    if (grad->ptr[CLIPOPS_HO_DET_EMBED] && (use_dab || det_cols < C))
        return fail(1, "clipops_handover_bwd_f32: det_embed gradient under DAB or narrower than C");
    return launch("handover_bwd_kernel", handover_bwd_kernel, dim3(n_q + n_tracks), dim3(256), 0, stream, grad_base, table,
                  inv_q, inv_prev, n_keep, n_q, n_det, n_tracks, use_dab, det_cols, handover_cols(K, C, use_dab), *grad);
}
}  // extern "C"
