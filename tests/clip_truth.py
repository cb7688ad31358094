"""Test infrastructure: float64 CPU truth of the clip-step kernels (include/clip_ops_hip.h), the inputs that reach their
lane, tile and tie edges, and the two rules every bound of tests/test_clip_ops_truth_gpu.py comes from.

Each ``*_truth`` function is plain torch in float64, written from the formula in the header comment of its entry point
(and the reference lines cited there), not from the kernel.  They are called on the fp32 inputs cast up, so truth is
the exact function of the bits the kernel saw; gradients are autograd's on the float64 graph.
tests/test_clip_truth_cpu.py pins them against the project's own ``*_reference`` formulations and evaluates every
input generator once.

Bounds.  ``analytic_*``: fp32 round-off of a K-term sum, c * 2^-24 * sqrt(K) * scale.  ``measured_bound``: 4 x the
error of the fp32 torch formulation on the same inputs + one fp32 ulp of the output scale (two correct fp32
evaluations in different operation orders differ by a few ulps per step; a wrong kernel is off by orders of magnitude).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ bounds and errors
def f64(t):
    return t.detach().cpu().double()


def f32_scalar(v: float) -> float:
    """The value a float argument has after the C ABI took it as a 32-bit float."""
    return float(np.float32(v))


def max_err(got, truth) -> float:
    got, truth = f64(got), f64(truth)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    if truth.numel() == 0:
        return 0.0
    d = (got - truth).abs()
    return float("inf") if not bool(torch.isfinite(got).all()) else float(d.max())


def out_scale(truth) -> float:
    return float(f64(truth).abs().max()) if truth.numel() else 0.0


def ulp32(scale: float) -> float:
    """Spacing of fp32 numbers at ``scale`` (0 for a zero scale: an exactly-zero truth with an exact baseline asks for
    an exact kernel)."""
    if scale == 0.0:
        return 0.0
    return 2.0 ** (math.frexp(scale)[1] - 24)        # scale = m * 2^e, 0.5 <= m < 1: ulp = 2^(e - 1 - 23)


def measured_bound(ref_err: float, scale: float) -> float:
    return 4.0 * ref_err + ulp32(scale)


def colsum_bound(rows: int, max_abs: float) -> float:
    return U24 * rows ** 0.5 * max_abs


# ------------------------------------------------------------------------------------------------ attention
def attention_truth(q, k, v, n_heads: int, key_mask=None, scale: float = None):
    """out[b,i,h,:] = sum_j softmax_j(scale * q[b,i,h,:] . k[b,j,h,:] | key_mask[b,j] == 0) * v[b,j,h,:]; (B, L, E) in
    and out, heads concatenated.  ``scale``: what the kernel receives, 1/sqrt(head_dim) rounded to fp32."""
    B, L, E = q.shape
    d = E // n_heads
    if scale is None:
        scale = f32_scalar(1.0 / d ** 0.5)
    qh, kh, vh = (t.reshape(B, L, n_heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.einsum("bhid,bhjd->bhij", qh, kh) * scale
    if key_mask is not None:
        s = s.masked_fill(key_mask.reshape(B, 1, 1, L), float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("bhij,bhjd->bhid", p, vh).permute(0, 2, 1, 3).reshape(B, L, E)


def attention_lse_truth(q, k, n_heads: int, key_mask=None, scale: float = None):
    B, L, E = q.shape
    d = E // n_heads
    if scale is None:
        scale = f32_scalar(1.0 / d ** 0.5)
    qh, kh = (t.reshape(B, L, n_heads, d).permute(0, 2, 1, 3) for t in (q, k))
    s = torch.einsum("bhid,bhjd->bhij", qh, kh) * scale
    if key_mask is not None:
        s = s.masked_fill(key_mask.reshape(B, 1, 1, L), float("-inf"))
    return torch.logsumexp(s, -1), s


def attention_truth_with_grads(q, k, v, up, n_heads, key_mask=None):
    """(out, grad q, grad k, grad v) in float64 for fp32 (or any) CPU/GPU inputs."""
    a, b, c = (f64(t).requires_grad_(True) for t in (q, k, v))
    mask = None if key_mask is None else key_mask.detach().cpu()
    out = attention_truth(a, b, c, n_heads, mask)
    (out * f64(up)).sum().backward()
    return out.detach(), a.grad, b.grad, c.grad


ATTN_LENGTHS = (1, 15, 16, 17, 31, 33, 255, 257, 511, 512)     # 16 rows x 16 lanes per workgroup; 512 = the LDS limit
ATTN_HEADS = (1, 3, 8)
ATTN_BATCHES = (1, 2)


def attn_inputs(B, L, H, seed=None):
    g = torch.Generator().manual_seed(1000 * L + 10 * H + B if seed is None else seed)
    E = 32 * H
    q = torch.randn(B, L, E, generator=g) * 1.5
    k = torch.randn(B, L, E, generator=g) * 1.5
    v = torch.randn(B, L, E, generator=g)
    up = torch.randn(B, L, E, generator=g)
    return q, k, v, up


def attn_mask_case(name):
    """(B, L, mask (B, L) bool) of the four mask cases; True = that key takes no part."""
    if name == "starved_lane":          # keys 5, 21, 37 of 40: lane 5 of every row (j = 5 mod 16) sees no key
        m = torch.zeros(1, 40, dtype=torch.bool)
        m[0, [5, 21, 37]] = True
    elif name == "single_live_key":     # every key but key 17 of 33
        m = torch.ones(1, 33, dtype=torch.bool)
        m[0, 17] = False
    elif name == "even_keys":           # interior mask: every second key of 64
        m = torch.zeros(1, 64, dtype=torch.bool)
        m[0, 0::2] = True
    elif name == "dead_batch":          # batch 1 has no live key at all, batch 0 is healthy
        m = torch.zeros(2, 40, dtype=torch.bool)
        m[1] = True
    else:
        raise KeyError(name)
    return m.shape[0], m.shape[1], m


ATTN_MASK_CASES = ("starved_lane", "single_live_key", "even_keys", "dead_batch")

# q and k ~ N(0, ATTN_LARGE_SIGMA^2) per element: the score q . k / sqrt(32) then has a standard deviation of sigma^2 =
# 19.4, and the extremes of the 2 x 48 x 48 scores sit near +-4.1 sigma^2 = +-80 (asserted on the CPU, with the
# fp32-rounded lse of every row finite).
ATTN_LARGE_SIGMA = 4.4
ATTN_LARGE_L = 48
ATTN_LARGE_H = 2


def attn_large_logit_inputs(order):
    """Keys ordered by the score of query row 0, per head: 'ascending' makes every key of row 0's lanes a new running
    maximum of the online softmax, 'descending' none after the first, 'shuffled' is the control."""
    g = torch.Generator().manual_seed(77)
    L, H = ATTN_LARGE_L, ATTN_LARGE_H
    q = torch.randn(1, L, 32 * H, generator=g) * ATTN_LARGE_SIGMA
    k = torch.randn(1, L, 32 * H, generator=g) * ATTN_LARGE_SIGMA
    v = torch.randn(1, L, 32 * H, generator=g)
    up = torch.randn(1, L, 32 * H, generator=g)
    if order != "shuffled":
        kh = k.reshape(1, L, H, 32)
        s0 = torch.einsum("hd,jhd->hj", q.reshape(1, L, H, 32)[0, 0].double(), kh[0].double())      # (H, L)
        idx = s0.argsort(1, descending=(order == "descending"))
        kh = torch.stack([kh[0, idx[h], h] for h in range(H)], 1)[None]
        k = kh.reshape(1, L, 32 * H).contiguous()
    return q, k, v, up


# ------------------------------------------------------------------------------------------------ add + LayerNorm
LN_COLS = 256


def add_layer_norm_truth(x, res, gamma, beta, eps: float):
    """sum = x + res;  y = (sum - mean) * rstd * gamma + beta, mean / biased variance over the 256 columns, eps inside
    the square root."""
    s = x + res
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    return (s - mean) / torch.sqrt(var + eps) * gamma + beta


LN_DATA = ("randn", "large_mean", "constant_rows")


def ln_inputs(kind, rows, seed=0):
    """x, res, gamma, beta, up (fp32).  In every kind x + res is exact in fp32 for the rows the kind is about, so truth
    (which adds in float64) normalises the very numbers the kernel normalises."""
    g = torch.Generator().manual_seed(seed * 7919 + rows)
    gamma = torch.rand(LN_COLS, generator=g) + 0.5
    beta = torch.randn(LN_COLS, generator=g) * 0.2
    up = torch.randn(rows, LN_COLS, generator=g)
    if kind == "randn":
        x, res = torch.randn(rows, LN_COLS, generator=g), torch.randn(rows, LN_COLS, generator=g)
    elif kind == "large_mean":
        # x + res = 1000 + 0.01 randn: variance 1e-4 against a mean of 1e3.  res = fl(1000 + n) - 1000 is exact and
        # so is 1000 + res.  A one-pass variance E[s^2] - mean^2 loses all of it: 1e6 * 2^-24 = 0.06 >> 1e-4.
        x = torch.full((rows, LN_COLS), 1000.0)
        res = (x + 0.01 * torch.randn(rows, LN_COLS, generator=g)) - x
    elif kind == "constant_rows":
        x, res = torch.randn(rows, LN_COLS, generator=g), torch.randn(rows, LN_COLS, generator=g)
        for r, (a, b) in zip(sorted({0, rows // 2}), ((3.0, -1.25), (-0.5, 0.5))):      # var = 0: y == beta exactly
            x[r], res[r] = a, b
    else:
        raise KeyError(kind)
    return x, res, gamma, beta, up


def ln_constant_rows(rows):
    return sorted({0, rows // 2})


# ------------------------------------------------------------------------------------------------ boxes
def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), -1)


def _iou_union(a, b):
    lt = torch.maximum(a[..., :2], b[..., :2])
    rb = torch.minimum(a[..., 2:], b[..., 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter
    return inter / union, union


def giou_truth(a, b):
    """GIoU of xyxy boxes, broadcasting: iou - (hull - union) / hull."""
    iou, union = _iou_union(a, b)
    wh = (torch.maximum(a[..., 2:], b[..., 2:]) - torch.minimum(a[..., :2], b[..., :2])).clamp(min=0)
    hull = wh[..., 0] * wh[..., 1]
    return iou - (hull - union) / hull


def pair_box_loss_truth(pred, tgt, weight=None):
    """(l1, giou loss) of n cxcywh pairs: |pred - tgt|_1 summed over the 4 coordinates and 1 - GIoU(xyxy, xyxy)."""
    l1 = (pred - tgt).abs().sum(-1)
    gl = 1 - giou_truth(xyxy(pred), xyxy(tgt))
    if weight is not None:
        l1, gl = l1 * weight, gl * weight
    return l1, gl


def pair_iou_truth(pred, tgt):
    return _iou_union(xyxy(pred), xyxy(tgt))[0]


def match_cost_truth(logits, boxes, gt_labels, gt_boxes, w_class, w_bbox, w_giou):
    """cost[l,q,t] = w_bbox |box - gt|_1 + w_class (pos - neg)(sigmoid(logit[l,q,label_t])) + w_giou (-GIoU), focal
    class cost with alpha 0.25, gamma 2 (matcher.py:83-121); a label outside [0, K) is clamped into it."""
    K = logits.shape[-1]
    prob = torch.sigmoid(logits)[..., gt_labels.clamp(0, K - 1)]
    neg = 0.75 * prob ** 2 * (-(1 - prob + 1e-8).log())
    pos = 0.25 * (1 - prob) ** 2 * (-(prob + 1e-8).log())
    c_bbox = (boxes[:, :, None, :] - gt_boxes[None, None]).abs().sum(-1)
    giou = giou_truth(xyxy(boxes)[:, :, None, :], xyxy(gt_boxes)[None, None])
    return w_bbox * c_bbox + w_class * (pos - neg) + w_giou * (-giou)


def grid_boxes(n, gen):
    """cxcywh with every coordinate a multiple of 1/64 in [1/8, 7/8]: the corners are multiples of 1/128, exact in fp32
    and float64 alike, so every max / min / >= 0 decision is the same in both."""
    return torch.randint(8, 57, (n, 4), generator=gen).float() / 64


# (prediction, target) pairs that sit exactly on the decisions of the GIoU backward
BOX_EDGE_PAIRS = (
    ("identical", (0.5, 0.5, 0.25, 0.25), (0.5, 0.5, 0.25, 0.25)),                    # every max / min is a tie
    ("shared_vertical_edge", (0.375, 0.375, 0.25, 0.25), (0.625, 0.375, 0.25, 0.25)),  # dw == 0, dh > 0
    ("shared_edge_swapped", (0.625, 0.375, 0.25, 0.25), (0.375, 0.375, 0.25, 0.25)),
    ("shared_corner", (0.375, 0.375, 0.25, 0.25), (0.625, 0.625, 0.25, 0.25)),         # dw == 0 and dh == 0
    ("nested_common_side", (0.5, 0.5, 0.5, 0.5), (0.375, 0.5, 0.25, 0.25)),            # x1 ties, the rest nests
    ("nested_inside", (0.375, 0.5, 0.25, 0.25), (0.5, 0.5, 0.5, 0.5)),
    ("disjoint", (0.25, 0.25, 0.125, 0.125), (0.75, 0.75, 0.125, 0.125)),              # dw < 0: the clamp is off
)
N_RANDOM_BOX_PAIRS = 64


def box_pairs():
    """pred (n, 4), tgt (n, 4), up (2, n): the edge pairs, then 64 random grid boxes (ties happen among them too)."""
    g = torch.Generator().manual_seed(64)
    pred = torch.cat((torch.tensor([p for _, p, _ in BOX_EDGE_PAIRS]), grid_boxes(N_RANDOM_BOX_PAIRS, g)))
    tgt = torch.cat((torch.tensor([t for _, _, t in BOX_EDGE_PAIRS]), grid_boxes(N_RANDOM_BOX_PAIRS, g)))
    up = torch.randn(2, pred.shape[0], generator=g)
    return pred, tgt, up


def box_decisions(pred, tgt):
    """Every comparison the GIoU forward and backward take, as one tensor of {-1, 0, 1}: sign(a - b) of the four corner
    pairs and the signs of the intersection / hull extents (>= 0 is sign != -1)."""
    a, b = xyxy(pred), xyxy(tgt)
    lt, rb = torch.maximum(a[..., :2], b[..., :2]), torch.minimum(a[..., 2:], b[..., 2:])
    lt_h, rb_h = torch.minimum(a[..., :2], b[..., :2]), torch.maximum(a[..., 2:], b[..., 2:])
    return torch.cat((torch.sign(a - b), torch.sign(rb - lt), torch.sign(rb_h - lt_h), torch.sign(pred - tgt)), -1)


MATCH_COST_MAX_LOGIT = 12.0     # beyond it the reference's +1e-8 is absorbed in fp32 but not in float64


def match_cost_inputs(n_layers, B, Q, Nq, K, T, labels="random"):
    g = torch.Generator().manual_seed(n_layers * 1000 + Q * 10 + K + T)
    logits = (torch.rand(n_layers, B, Nq, K, generator=g) * 2 - 1) * MATCH_COST_MAX_LOGIT
    logits[0, 0, 0, 0], logits[-1, -1, -1, -1] = MATCH_COST_MAX_LOGIT, -MATCH_COST_MAX_LOGIT
    boxes = grid_boxes(n_layers * B * Nq, g).reshape(n_layers, B, Nq, 4)
    gt_boxes = grid_boxes(T, g)
    gt_labels = torch.randint(0, K, (T,), generator=g)
    if labels == "out_of_range" and T >= 2:
        gt_labels[0], gt_labels[1] = -1, K
    return logits, boxes, gt_labels, gt_boxes


# ------------------------------------------------------------------------------------------------ focal loss
def focal_truth(logits, labels, alpha: float, gamma: float):
    """loss[l] = sum_q mean_k a_t * ce * (1 - p_t)^gamma, target the one-hot of labels[l,q] (label == K: background);
    a_t = alpha for the target class, 1 - alpha otherwise, 1 when alpha < 0.  1 - p_t is taken as the sigmoid of the
    mirrored logit, which it equals exactly, instead of the subtraction that cancels."""
    K = logits.shape[-1]
    t = F.one_hot(labels, K + 1)[..., :-1].to(logits.dtype)
    ce = F.binary_cross_entropy_with_logits(logits, t, reduction="none")
    one_minus_pt = torch.sigmoid(torch.where(t > 0, -logits, logits))
    loss = ce * one_minus_pt ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss.mean(2).sum(1)


FOCAL_GRID = torch.linspace(-90.0, 90.0, 181)           # step 1: contains 0, +-88, +-89; expf(-x) overflows at 88.72
FOCAL_SHAPES = ((1, 5), (1, 255), (1, 256), (1, 257), (1, 2479), (3, 85), (8, 32))       # (K, Nq): Nq*K as asked
FOCAL_PARAMS = ((0.25, 2.0), (0.25, 1.5), (-1.0, 2.0), (0.5, 0.0))
FOCAL_LABELS = ("background", "class0", "random")


def focal_inputs(K, Nq, label_kind, n_layers=2):
    """logits (n_layers, 2, Nq + 3, K) to be viewed as [:, 1, :Nq] (strided), labels (n_layers, Nq), up (n_layers)."""
    g = torch.Generator().manual_seed(K * 10000 + Nq)
    total = n_layers * Nq * K
    if Nq * K == 5:
        vals = torch.tensor([-89.0, -88.0, 0.0, 88.0, 89.0]).repeat(n_layers)
    else:
        reps = -(-total // FOCAL_GRID.numel())
        vals = FOCAL_GRID.repeat(reps)[torch.randperm(reps * FOCAL_GRID.numel(), generator=g)[:total]]
    buf = torch.randn(n_layers, 2, Nq + 3, K, generator=g)
    buf[:, 1, :Nq] = vals.reshape(n_layers, Nq, K)
    labels = {"background": torch.full((n_layers, Nq), K), "class0": torch.zeros(n_layers, Nq, dtype=torch.long),
              "random": torch.randint(0, K + 1, (n_layers, Nq), generator=g)}[label_kind]
    up = torch.randn(n_layers, generator=g)
    return buf, labels, up


# ------------------------------------------------------------------------------------------------ sine embedding
def sine_embed_truth(pos, dim_t, scale: float):
    """out[..., k*F + j] = (j even ? sin : cos)((pos[..., k] * scale) / dim_t[j])."""
    e = (pos * scale)[..., None] / dim_t
    j = torch.arange(dim_t.shape[0])
    out = torch.where(j % 2 == 0, e.sin(), e.cos())
    return out.flatten(-2)


def sine_positions():
    g = torch.Generator().manual_seed(3)
    special = torch.tensor([0.0, 1.0, -0.25, 1.0 - 2.0 ** -24])
    return torch.cat((special, torch.rand(40, generator=g))).reshape(11, 4)


# ------------------------------------------------------------------------------------------------ sums and linears
def colsum_truth(x):
    return x.sum(0)


def colsum_inputs(rows, cols):
    """Alternating +-1e4 by row plus randn: neighbouring rows cancel, a strided partial sum does not."""
    g = torch.Generator().manual_seed(rows * 64 + cols)
    sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
    return sign[:, None] * 1e4 + torch.randn(rows, cols, generator=g)


def linear_truth(x, w, b, relu: bool):
    y = x @ w.t() + b
    return torch.relu(y) if relu else y


LINEAR_SHAPES = ((1, 4, 1), (31, 8, 31), (32, 12, 32), (33, 36, 33), (1, 36, 36), (31, 4, 32), (32, 8, 33), (33, 12, 36),
                 (1, 12, 31), (31, 36, 1), (32, 4, 36), (33, 8, 1))        # rows x in x out: every value of each axis


def linear_inputs(rows, in_f, out_f):
    g = torch.Generator().manual_seed(rows * 10000 + in_f * 100 + out_f)
    x = torch.randn(rows, in_f, generator=g)
    w = torch.randn(out_f, in_f, generator=g) / in_f ** 0.5
    b = torch.randn(out_f, generator=g)
    gy = torch.randn(rows, out_f, generator=g)
    return x, w, b, gy


def linear_integer_inputs(rows=33, in_f=36, out_f=36):
    """Small-integer operands: every product and partial sum is exact in fp32 in any order, so results can be compared
    bit for bit.  y_relu holds a NaN, a -0.0, zeros, negatives and positives."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (rows, in_f), generator=g).float()
    w = torch.randint(-4, 5, (out_f, in_f), generator=g).float()
    gy = torch.randint(-8, 9, (rows, out_f), generator=g).float()
    y = torch.randint(-2, 3, (rows, out_f), generator=g).float()
    y[0, 0], y[1, 1], y[rows - 1, out_f - 1] = float("nan"), -0.0, float("nan")
    gy[0, 0], gy[1, 1] = 7.0, 5.0
    return x, w, gy, y
