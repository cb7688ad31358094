// clip_criterion.h -- the criterion and the matcher: matching cost, paired box losses and IoU, the focal loss of stacked
// layers, the per-frame bookkeeping (track ownership, focal labels) and the device assignment solver.
// Included by clip_ops.hip after clip_common.h and assign_core.h.
#pragma once

namespace {
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

std::atomic<unsigned long long> g_lds_assign{0};
}  // namespace

extern "C" {
int clipops_match_cost_f32(const float *logits, long logit_sl, long logit_sq, const float *boxes, long box_sl,
                           long box_sq, const int64_t *gt_labels, const float *gt_boxes, int n_layers, int Q, int K,
                           int T, float w_class, float w_bbox, float w_giou, float *cost, void *stream) {
    if (n_layers < 0 || Q < 0 || T < 0 || K <= 0) return fail(1, "clipops_match_cost_f32: bad dimension");
    if ((long)n_layers * Q * T == 0) return ok();
    if (!logits || !boxes || !gt_labels || !gt_boxes || !cost) return fail(1, "clipops_match_cost_f32: null pointer");
    return launch("match_cost_kernel", match_cost_kernel, dim3(grid_for((long)n_layers * Q * T)), dim3(256), 0, stream,
                  logits, logit_sl, logit_sq, boxes, box_sl, box_sq, gt_labels, gt_boxes, n_layers, Q, K, T, w_class,
                  w_bbox, w_giou, cost);
}

int clipops_pair_box_loss_fwd_f32(const float *boxes, const int64_t *lay, const int64_t *qidx, long row_mul,
                                  long row_add, const float *tgt_boxes, const int64_t *gidx, const float *weight,
                                  int n, float *l1, float *giou_loss, void *stream) {
    if (n < 0) return fail(1, "clipops_pair_box_loss_fwd_f32: negative count");
    if (n == 0) return ok();
    if (!boxes || !lay || !qidx || !tgt_boxes || !l1 || !giou_loss)
        return fail(1, "clipops_pair_box_loss_fwd_f32: null pointer");
    return launch("pair_box_loss_fwd_kernel", pair_box_loss_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, boxes,
                  lay, qidx, row_mul, row_add, tgt_boxes, gidx, weight, n, l1, giou_loss);
}

int clipops_pair_box_loss_bwd_f32(const float *boxes, const int64_t *lay, const int64_t *qidx, long row_mul,
                                  long row_add, const float *tgt_boxes, const int64_t *gidx, const float *weight,
                                  int n, const float *grad_l1, const float *grad_giou, float *grad_boxes,
                                  void *stream) {
    if (n < 0) return fail(1, "clipops_pair_box_loss_bwd_f32: negative count");
    if (n == 0) return ok();
    if (!boxes || !lay || !qidx || !tgt_boxes || !grad_l1 || !grad_giou || !grad_boxes)
        return fail(1, "clipops_pair_box_loss_bwd_f32: null pointer");
    return launch("pair_box_loss_bwd_kernel", pair_box_loss_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, boxes,
                  lay, qidx, row_mul, row_add, tgt_boxes, gidx, weight, n, grad_l1, grad_giou, grad_boxes);
}

int clipops_pair_iou_f32(const float *boxes, const float *tgt_boxes, const int64_t *gidx, int n, float *iou,
                         void *stream) {
    if (n < 0) return fail(1, "clipops_pair_iou_f32: negative count");
    if (n == 0) return ok();
    if (!boxes || !tgt_boxes || !iou) return fail(1, "clipops_pair_iou_f32: null pointer");
    return launch("pair_iou_kernel", pair_iou_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, boxes, tgt_boxes, gidx,
                  n, iou);
}

int clipops_focal_fwd_f32(const float *logits, long sl, long sq, const int64_t *labels, int n_layers, int Nq, int K,
                          float alpha, float gamma, float *loss, void *stream) {
    if (n_layers < 0 || Nq < 0 || K <= 0) return fail(1, "clipops_focal_fwd_f32: bad dimension");
    if (n_layers == 0) return ok();
    if (!loss || (Nq > 0 && (!logits || !labels))) return fail(1, "clipops_focal_fwd_f32: null pointer");
    return launch("focal_fwd_kernel", focal_fwd_kernel, dim3(n_layers), dim3(256), 0, stream, logits, sl, sq, labels, Nq, K,
                  alpha, gamma, loss);
}

int clipops_focal_bwd_f32(const float *logits, long sl, long sq, const int64_t *labels, int n_layers, int Nq, int K,
                          float alpha, float gamma, const float *grad_loss, float *grad_logits, void *stream) {
    if (n_layers < 0 || Nq < 0 || K <= 0) return fail(1, "clipops_focal_bwd_f32: bad dimension");
    if ((long)n_layers * Nq == 0) return ok();
    if (!logits || !labels || !grad_loss || !grad_logits) return fail(1, "clipops_focal_bwd_f32: null pointer");
    return launch("focal_bwd_kernel", focal_bwd_kernel, dim3(grid_for((long)n_layers * Nq * K)), dim3(256), 0, stream,
                  logits, sl, sq, labels, n_layers, Nq, K, alpha, gamma, grad_loss, grad_logits);
}

int clipops_track_ownership_i64(const int64_t *track_ids, int n_tracks, const int64_t *gt_ids, int n_gt,
                                int64_t *matched_idx, float *gt_free, void *stream) {
    if (n_tracks < 0 || n_gt < 0) return fail(1, "clipops_track_ownership_i64: negative count");
    if (n_tracks + n_gt == 0) return ok();
    if ((n_tracks > 0 && (!track_ids || !matched_idx)) || (n_gt > 0 && (!gt_ids || !gt_free)))
        return fail(1, "clipops_track_ownership_i64: null pointer");
    return launch("track_ownership_kernel", track_ownership_kernel, dim3(1), dim3(256), 0, stream, track_ids, n_tracks,
                  gt_ids, n_gt, matched_idx, gt_free);
}

int clipops_focal_labels_i64(const int64_t *lay, const int64_t *q, const int64_t *g, int n_pairs,
                             const int64_t *gt_labels, int n_gt, const int64_t *matched_idx, int n_tracks,
                             const uint8_t *late, int n_layers, int n_det, int K, int64_t *labels, void *stream) {
    if (n_pairs < 0 || n_gt < 0 || n_tracks < 0 || n_layers < 0 || n_det < 0) return fail(1, "clipops_focal_labels_i64: negative count");
    if ((long)n_layers * (n_det + n_tracks) == 0) return ok();
    if (!labels || !late || (n_pairs > 0 && (!lay || !q || !g || !gt_labels)) || (n_tracks > 0 && !matched_idx) ||
        (n_gt > 0 && !gt_labels))
        return fail(1, "clipops_focal_labels_i64: null pointer");
    return launch("focal_labels_kernel", focal_labels_kernel, dim3(1), dim3(256), 0, stream, lay, q, g, n_pairs, gt_labels,
                  n_gt, matched_idx, n_tracks, late, n_layers, n_det, K, labels);
}

int clipops_assign_f32(const float *cost, long stride_problem, long stride_row, long stride_col, int n_problems,
                       int n_rows, int n_cols, int32_t *row_ind, int32_t *col_ind, int32_t *status, void *stream) {
    if (n_problems < 0 || n_rows < 0 || n_cols < 0) return fail(1, "clipops_assign_f32: bad dimension");
    if (n_problems == 0 || n_rows == 0 || n_cols == 0) return ok();
    if (!cost || !row_ind || !col_ind) return fail(1, "clipops_assign_f32: null pointer");
    const int nr = n_rows < n_cols ? n_rows : n_cols, nc = n_rows < n_cols ? n_cols : n_rows;
    if (nc > CLIPOPS_ASSIGN_MAX_DIM) return fail(2, "clipops_assign_f32: problem exceeds CLIPOPS_ASSIGN_MAX_DIM");
    // (86,016 bytes at CLIPOPS_ASSIGN_MAX_DIM x CLIPOPS_ASSIGN_MAX_DIM: every admitted problem fits what allow_lds asks for)
    const size_t lds = (assign::work_bytes(nr, nc) + 15) & ~(size_t)15;
    if (lds > 160 * 1024) return fail(2, "clipops_assign_f32: problem does not fit the LDS of a CU");
    if (allow_lds(reinterpret_cast<const void *>(assign_kernel), lds, g_lds_assign)) {
        (void)hipGetLastError();
        return fail(3, "clipops_assign_f32: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    }
    return launch("assign_kernel", assign_kernel, dim3(n_problems), dim3(64), lds, stream, cost, stride_problem, stride_row,
                  stride_col, n_rows, n_cols, row_ind, col_ind, status);
}
}  // extern "C"
