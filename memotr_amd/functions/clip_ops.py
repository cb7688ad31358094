"""Fused small-tensor chains of the clip train step: one gfx950 kernel per chain (include/clip_ops_hip.h) where the
reference issues a string of element-wise torch kernels.

Every function takes CUDA fp32 tensors and launches through the C ABI; ``*_reference`` are the element-wise torch
formulations of the same arithmetic (the reference's formulas) -- what CPU tensors run and what the GPU tests
compare the kernels with.  ``fused(t)`` decides: CUDA fp32 tensors use the kernels unless MEMOTR_FUSED_CLIP_OPS=0.
"""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn.functional as F


def fused(*tensors) -> bool:
    return (os.environ.get("MEMOTR_FUSED_CLIP_OPS", "1") != "0"
            and all(t.is_cuda and (t.dtype == torch.float32 or not t.is_floating_point()) for t in tensors))


def config_key() -> tuple:
    """The environment switches that change which kernels a captured graph contains."""
    return (os.environ.get("MEMOTR_FUSED_CLIP_OPS", "1"), os.environ.get("MEMOTR_COLSUM_TALL", "1"),
            os.environ.get("MEMOTR_ATTN_KERNELS", "1"), os.environ.get("MEMOTR_FUSED_LN", "1"),
            os.environ.get("MEMOTR_FUSED_SHIFT_RELU", "1"), os.environ.get("MEMOTR_FUSED_LINEAR_BWD", "1"),
            os.environ.get("MEMOTR_FUSED_LINEAR_FWD", "1"), os.environ.get("MEMOTR_LINEAR_STAGED", "1"))


def _lib():
    from .. import _clip_lib        # raises ImportError when the library is missing: no silent substitute
    return _clip_lib


def _stream(t: torch.Tensor) -> int:
    """Launch stream of ``t``'s device.  The kernels launch on the CURRENT device (one device per process, as under
    DistributedDataParallel); tensors of another device would get that device's stream handle with the wrong device
    current, so that case is refused loudly instead of launching somewhere else."""
    idx = t.device.index
    if idx is not None and idx != torch.cuda.current_device():
        raise RuntimeError(f"clip_ops: tensor on cuda:{idx} but cuda:{torch.cuda.current_device()} is current; "
                           "call torch.cuda.set_device(tensor.device) (one device per process)")
    return torch.cuda.current_stream(t.device).cuda_stream


def _strides3(t: torch.Tensor):
    """(layer stride, row stride) in elements of a (n_layers, rows, C) view whose last axis is dense."""
    if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
        raise RuntimeError("expected a (layers, rows, C) tensor with a dense last axis")
    return t.stride(0), t.stride(1)


# --------------------------------------------------------------------------------------------------------------
# matching cost (models/matcher.py of the reference, :83-121)
# --------------------------------------------------------------------------------------------------------------
def match_cost(logits: torch.Tensor, boxes: torch.Tensor, gt_labels: torch.Tensor, gt_boxes: torch.Tensor,
               w_class: float, w_bbox: float, w_giou: float, out: torch.Tensor = None) -> torch.Tensor:
    """(n_layers, Q, K) logits and (n_layers, Q, 4) cxcywh boxes (views allowed) against (T,) labels / (T, 4) boxes
    -> (n_layers, Q, T) cost.  ``out``: a contiguous float32 destination of n_layers * Q * T elements (any shape: the
    tail of the buffer that travels to the host)."""
    n_layers, Q, K = logits.shape
    T = gt_labels.shape[0]
    if out is not None:
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n_layers * Q * T
        cost = out.view(n_layers, Q, T)
    else:
        cost = torch.empty((n_layers, Q, T), dtype=torch.float32, device=logits.device)
    lsl, lsq = _strides3(logits)
    bsl, bsq = _strides3(boxes)
    gt_labels, gt_boxes = gt_labels.contiguous(), gt_boxes.contiguous()
    L = _lib()
    L.check(L.lib.clipops_match_cost_f32(logits.data_ptr(), lsl, lsq, boxes.data_ptr(), bsl, bsq, gt_labels.data_ptr(),
                                         gt_boxes.data_ptr(), n_layers, Q, K, T, float(w_class), float(w_bbox),
                                         float(w_giou), cost.data_ptr(), _stream(logits)), "clipops_match_cost_f32")
    return cost


# --------------------------------------------------------------------------------------------------------------
# per-frame bookkeeping (include/clip_ops_hip.h, ABI 10): ownership of the ground truths, focal-loss targets
# --------------------------------------------------------------------------------------------------------------
def track_ownership(track_ids: torch.Tensor, gt_ids: torch.Tensor, free_out: torch.Tensor = None):
    """-> (matched_idx (n_tracks,) int64: index of the LAST ground truth carrying the track's id or -1,
    free (n_gt,) float32: 1 where no track carries the ground truth's id).  ``free_out``: where to write ``free``."""
    n_tr, n_gt = track_ids.shape[0], gt_ids.shape[0]
    matched = torch.empty((n_tr,), dtype=torch.int64, device=gt_ids.device)
    free = free_out if free_out is not None else torch.empty((n_gt,), dtype=torch.float32, device=gt_ids.device)
    assert free.is_contiguous() and free.dtype == torch.float32 and free.numel() == n_gt
    track_ids, gt_ids = track_ids.contiguous(), gt_ids.contiguous()
    L = _lib()
    L.check(L.lib.clipops_track_ownership_i64(track_ids.data_ptr(), n_tr, gt_ids.data_ptr(), n_gt, matched.data_ptr(),
                                              free.data_ptr(), _stream(gt_ids)), "clipops_track_ownership_i64")
    return matched, free


def track_ownership_reference(track_ids, gt_ids):
    n_gt = gt_ids.shape[0]
    eq = track_ids[:, None] == gt_ids[None, :]
    order = torch.arange(1, n_gt + 1, device=eq.device)
    return (eq * order).amax(1) - 1 if n_gt > 0 else torch.full_like(track_ids, -1), (~eq.any(0)).to(torch.float32)


def focal_labels(lay: torch.Tensor, q: torch.Tensor, g: torch.Tensor, gt_labels: torch.Tensor, matched_idx,
                 late: torch.Tensor, n_det: int, n_tracks: int, num_classes: int) -> torch.Tensor:
    """(n_layers, n_det + n_tracks) int64 focal-loss targets: background, the carried tracks' labels in the layers with
    ``late`` set, the matched (layer, query, ground truth) triples -- ``focal_labels_reference`` in one launch."""
    n_layers = late.shape[0]
    labels = torch.empty((n_layers, n_det + n_tracks), dtype=torch.int64, device=late.device)
    lay, q, g, gt_labels = lay.contiguous(), q.contiguous(), g.contiguous(), gt_labels.contiguous()
    L = _lib()
    L.check(L.lib.clipops_focal_labels_i64(lay.data_ptr(), q.data_ptr(), g.data_ptr(), lay.shape[0], gt_labels.data_ptr(),
                                           gt_labels.shape[0], None if matched_idx is None else matched_idx.contiguous().data_ptr(),
                                           n_tracks, late.contiguous().data_ptr(), n_layers, n_det, num_classes,
                                           labels.data_ptr(), _stream(late)), "clipops_focal_labels_i64")
    return labels


def focal_labels_reference(lay, q, g, gt_labels, matched_idx, late, n_det, n_tracks, num_classes):
    n_layers = late.shape[0]
    labels = torch.full((n_layers, n_det + n_tracks), num_classes, dtype=torch.int64, device=late.device)
    labels[lay, q] = gt_labels[g]
    if n_tracks > 0:
        has = matched_idx >= 0
        tr_lab = torch.where(has, gt_labels[matched_idx.clamp(min=0)] if gt_labels.shape[0] > 0
                             else torch.full_like(matched_idx, num_classes), torch.full_like(matched_idx, num_classes))
        labels[:, n_det:] = torch.where(late[:, None], tr_lab[None, :], labels[:, n_det:])
    return labels


# --------------------------------------------------------------------------------------------------------------
# paired L1 + GIoU box losses (models/criterion.py of the reference, :417-440)
# --------------------------------------------------------------------------------------------------------------
class _PairBoxLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, boxes_all, lay, qidx, b, tgt_boxes, gidx, weight):
        n_layers, B, Nq, _ = boxes_all.shape
        n = lay.shape[0]
        l1 = torch.empty((n,), dtype=torch.float32, device=boxes_all.device)
        gl = torch.empty_like(l1)
        L = _lib()
        L.check(L.lib.clipops_pair_box_loss_fwd_f32(
            boxes_all.data_ptr(), lay.data_ptr(), qidx.data_ptr(), B * Nq, b * Nq, tgt_boxes.data_ptr(),
            None if gidx is None else gidx.data_ptr(), None if weight is None else weight.data_ptr(), n,
            l1.data_ptr(), gl.data_ptr(), _stream(boxes_all)), "clipops_pair_box_loss_fwd_f32")
        ctx.save_for_backward(boxes_all, lay, qidx, tgt_boxes, gidx, weight)
        ctx.b = b
        return l1, gl

    @staticmethod
    def backward(ctx, g_l1, g_gl):
        boxes_all, lay, qidx, tgt_boxes, gidx, weight = ctx.saved_tensors
        n_layers, B, Nq, _ = boxes_all.shape
        grad = torch.zeros_like(boxes_all)
        L = _lib()
        L.check(L.lib.clipops_pair_box_loss_bwd_f32(
            boxes_all.data_ptr(), lay.data_ptr(), qidx.data_ptr(), B * Nq, ctx.b * Nq, tgt_boxes.data_ptr(),
            None if gidx is None else gidx.data_ptr(), None if weight is None else weight.data_ptr(), lay.shape[0],
            g_l1.contiguous().data_ptr(), g_gl.contiguous().data_ptr(), grad.data_ptr(), _stream(boxes_all)),
            "clipops_pair_box_loss_bwd_f32")
        return grad, None, None, None, None, None, None


def pair_box_loss(boxes_all: torch.Tensor, lay: torch.Tensor, qidx: torch.Tensor, b: int, tgt_boxes: torch.Tensor,
                  gidx: torch.Tensor = None, weight: torch.Tensor = None):
    """L1 (summed over the 4 coordinates) and 1 - GIoU of the pairs (boxes_all[lay[i], b, qidx[i]], tgt_boxes[gidx[i]]
    or tgt_boxes[i]), each optionally times weight[i].  boxes_all: (n_layers, B, Nq, 4) contiguous, cxcywh; the
    (lay, qidx) pairs of one call must be distinct.  Returns two (n,) tensors; gradients flow to boxes_all."""
    if not boxes_all.is_contiguous():
        boxes_all = boxes_all.contiguous()
    return _PairBoxLoss.apply(boxes_all, lay.contiguous(), qidx.contiguous(), int(b), tgt_boxes.contiguous(),
                              None if gidx is None else gidx.contiguous(),
                              None if weight is None else weight.contiguous())


def pair_box_loss_reference(boxes_all, lay, qidx, b, tgt_boxes, gidx=None, weight=None):
    from ..models.criterion import paired_giou
    from ..utils.box_ops import box_cxcywh_to_xyxy
    pb = boxes_all[lay, b, qidx]
    tb = tgt_boxes if gidx is None else tgt_boxes[gidx]
    l1 = F.l1_loss(pb, tb, reduction="none").sum(-1)
    gl = 1 - paired_giou(box_cxcywh_to_xyxy(pb), box_cxcywh_to_xyxy(tb))
    if weight is not None:
        l1, gl = l1 * weight, gl * weight
    return l1, gl


def pair_iou(boxes: torch.Tensor, tgt_boxes: torch.Tensor, gidx: torch.Tensor = None) -> torch.Tensor:
    """IoU of cxcywh boxes[i] with tgt_boxes[gidx[i]] (or tgt_boxes[i]); no gradient (the tracks' ``iou`` field only
    feeds threshold comparisons in the query updater)."""
    boxes, tgt_boxes = boxes.detach().contiguous(), tgt_boxes.contiguous()
    n = boxes.shape[0]
    out = torch.empty((n,), dtype=torch.float32, device=boxes.device)
    L = _lib()
    L.check(L.lib.clipops_pair_iou_f32(boxes.data_ptr(), tgt_boxes.data_ptr(), None if gidx is None else
                                       gidx.contiguous().data_ptr(), n, out.data_ptr(), _stream(boxes)),
            "clipops_pair_iou_f32")
    return out


def assign(cost: torch.Tensor):
    """Linear sum assignment of a batch of cost matrices (P, R, C) (any strides) on the device:
    (row_ind (P, k) int32, col_ind (P, k) int32, status (P,) int32), k = min(R, C) -- per problem the pairs
    ``scipy.optimize.linear_sum_assignment`` returns (same algorithm, scan order and tie rule:
    csrc/assign_core.h), status k, or -1 where scipy would raise "cost matrix is infeasible".  No synchronisation."""
    if cost.dim() != 3 or cost.dtype != torch.float32 or not cost.is_cuda:
        raise RuntimeError("assign expects a float32 CUDA tensor of shape (problems, rows, cols)")
    P, R, C = cost.shape
    k = min(R, C)
    row = torch.empty((P, k), dtype=torch.int32, device=cost.device)
    col = torch.empty((P, k), dtype=torch.int32, device=cost.device)
    status = torch.empty((P,), dtype=torch.int32, device=cost.device)
    L = _lib()
    L.check(L.lib.clipops_assign_f32(cost.data_ptr(), cost.stride(0), cost.stride(1), cost.stride(2), P, R, C,
                                     row.data_ptr(), col.data_ptr(), status.data_ptr(), _stream(cost)),
            "clipops_assign_f32")
    return row, col, status


def pair_iou_reference(boxes, tgt_boxes, gidx=None):
    from ..models.criterion import paired_iou
    from ..utils.box_ops import box_cxcywh_to_xyxy
    tb = tgt_boxes if gidx is None else tgt_boxes[gidx]
    return paired_iou(box_cxcywh_to_xyxy(boxes), box_cxcywh_to_xyxy(tb))


# --------------------------------------------------------------------------------------------------------------
# track hand-over between two frames (include/clip_ops_hip.h: clipops_handover_*)
# --------------------------------------------------------------------------------------------------------------
HANDOVER_CARRIED, HANDOVER_NEW, HANDOVER_UNCLAIMED = 0, 1, 2
# the differentiable sources, in the order ``handover`` takes them (det_embed: None under DAB)
HANDOVER_DIFF = ("outputs", "queries", "last_ref", "init_ref", "det_embed", "prev_ref", "prev_long", "prev_last",
                 "prev_query")


def handover_tables(n_det: int, n_q: int, n_tracks: int, new_q, new_g, free_q, keep):
    """Host side of the hand-over (numpy in, one int64 numpy vector out): the row table of the active set and its
    inverse.  Rows of (carried tracks; new tracks; unclaimed detections) are numbered as the composed path concatenates
    them; ``keep`` picks the active ones, in order.  Returns ``[table (n_keep, 3) | inv_q (n_q) | inv_prev (n_tracks)]``
    flattened: table row o = (kind, source row, ground truth); inv_q[r] / inv_prev[j] = the output row that reads model
    row r / previous-set row j, or -1."""
    import numpy as np
    n_new, n_free = len(new_q), len(free_q)
    kind = np.concatenate((np.full((n_tracks,), HANDOVER_CARRIED, dtype=np.int64),
                           np.full((n_new,), HANDOVER_NEW, dtype=np.int64),
                           np.full((n_free,), HANDOVER_UNCLAIMED, dtype=np.int64)))
    src = np.concatenate((np.arange(n_tracks, dtype=np.int64), np.asarray(new_q, dtype=np.int64),
                          np.asarray(free_q, dtype=np.int64)))
    gt = np.concatenate((np.full((n_tracks,), -1, dtype=np.int64), np.asarray(new_g, dtype=np.int64),
                         np.full((n_free,), -1, dtype=np.int64)))
    keep = np.asarray(keep, dtype=np.int64)
    table = np.stack((kind[keep], src[keep], gt[keep]), axis=1)
    rows = np.arange(len(keep), dtype=np.int64)
    carried = table[:, 0] == HANDOVER_CARRIED
    inv_q = np.full((n_q,), -1, dtype=np.int64)
    inv_q[np.where(carried, n_det + table[:, 1], table[:, 1])] = rows
    inv_prev = np.full((n_tracks,), -1, dtype=np.int64)
    inv_prev[table[carried, 1]] = rows[carried]
    return np.concatenate((table.reshape(-1), inv_q, inv_prev))


def _handover_views(tables, n_keep, n_q, n_tracks):
    table = tables[:3 * n_keep]
    inv_q = tables[3 * n_keep:3 * n_keep + n_q]
    inv_prev = tables[3 * n_keep + n_q:3 * n_keep + n_q + n_tracks]
    return table, inv_q, inv_prev


def _rows_dense(t):
    """A 2-d view the kernels can address as base + row * stride (dense columns), else a contiguous copy."""
    return t if t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1) and t.stride(0) >= 0 else t.contiguous()


class _Handover(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, queries, last_ref, init_ref, det_embed, prev_ref, prev_long, prev_last, prev_query,
                logits, boxes, prev_iou, prev_ids, prev_matched, gt_boxes, gt_ids, tables, n_keep, n_det):
        L = _lib()
        use_dab = det_embed is None
        n_q, C, K = outputs.shape[0], outputs.shape[1], logits.shape[1]
        n_tracks, n_gt = prev_ref.shape[0], gt_boxes.shape[0]
        QW = C if use_dab else 2 * C
        named = dict(logits=logits, boxes=boxes, outputs=outputs, queries=queries, last_ref=last_ref, init_ref=init_ref,
                     det_embed=det_embed, prev_ref=prev_ref, prev_long=prev_long, prev_last=prev_last,
                     prev_query=prev_query, prev_iou=prev_iou.reshape(-1, 1))
        widths = dict(logits=K, boxes=4, outputs=C, queries=C, last_ref=4, init_ref=4, det_embed=C, prev_ref=4,
                      prev_long=C, prev_last=C, prev_query=QW, prev_iou=1)
        src, keep = L.HandoverSources(), []
        for i, name in enumerate(L.HANDOVER_SOURCES):
            t = named[name]
            if t is None or t.shape[0] == 0:
                continue
            lead = n_tracks if name.startswith("prev_") else (n_det if name == "det_embed" else n_det + n_tracks)
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < lead or (
                    t.shape[1] != widths[name] and not (name == "det_embed" and t.shape[1] >= C)):
                raise RuntimeError(f"handover: source {name} has shape {tuple(t.shape)} ({t.dtype})")
            t = _rows_dense(t.detach())
            keep.append(t)
            src.ptr[i], src.row_stride[i] = t.data_ptr(), t.stride(0)
        if n_q != queries.shape[0] or n_q != last_ref.shape[0] or n_q != init_ref.shape[0]:
            raise RuntimeError("handover: the model-output sources differ in their row counts")
        if tables.dtype != torch.int64 or tables.numel() != 3 * n_keep + n_q + n_tracks:
            raise RuntimeError("handover: the table does not have 3 * n_keep + n_q + n_tracks int64 entries")
        tables = tables.contiguous()
        prev_ids, prev_matched, gt_boxes, gt_ids = (t.contiguous() for t in (prev_ids, prev_matched, gt_boxes, gt_ids))
        if n_tracks and (prev_ids.shape[0] != n_tracks or prev_matched.shape[0] != n_tracks):
            raise RuntimeError("handover: ids / matched_idx of the previous set do not have one entry per track")
        dev = outputs.device
        base = torch.empty((n_keep, K + 8 + 3 * C + QW + 1), dtype=torch.float32, device=dev)
        ints = torch.empty((2, n_keep), dtype=torch.int64, device=dev)
        L.check(L.lib.clipops_handover_fwd_f32(
            ctypes.byref(src), prev_ids.data_ptr() if n_tracks else None, prev_matched.data_ptr() if n_tracks else None,
            gt_boxes.data_ptr(), gt_ids.data_ptr(), tables.data_ptr(), n_keep, n_det, n_tracks, n_gt, K, C,
            int(use_dab), base.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), _stream(outputs)),
            "clipops_handover_fwd_f32")
        ctx.save_for_backward(tables)
        ctx.dims = (n_keep, n_q, n_det, n_tracks, K, C, use_dab, 0 if det_embed is None else det_embed.shape[1], QW)
        ctx.mark_non_differentiable(ints)
        return base, ints

    @staticmethod
    def backward(ctx, g_base, _g_ints):
        L = _lib()
        (tables,) = ctx.saved_tensors
        n_keep, n_q, n_det, n_tracks, K, C, use_dab, det_cols, QW = ctx.dims
        table, inv_q, inv_prev = _handover_views(tables, n_keep, n_q, n_tracks)
        g_base = g_base.contiguous()
        shapes = dict(outputs=(n_q, C), queries=(n_q, C), last_ref=(n_q, 4), init_ref=(n_q, 4),
                      det_embed=(n_det, det_cols), prev_ref=(n_tracks, 4), prev_long=(n_tracks, C),
                      prev_last=(n_tracks, C), prev_query=(n_tracks, QW))
        wanted = [name for i, name in enumerate(HANDOVER_DIFF) if ctx.needs_input_grad[i]]
        # every gradient is a slice of ONE allocation, written in full by the one launch (no zero-fill)
        flat = torch.empty((sum(shapes[n][0] * shapes[n][1] for n in wanted),), dtype=torch.float32, device=g_base.device)
        grads, out, pos = L.HandoverGrads(), {}, 0
        for name in wanted:
            r, c = shapes[name]
            out[name] = flat[pos:pos + r * c].view(r, c)
            pos += r * c
            if r * c:
                grads.ptr[L.HANDOVER_SOURCES.index(name)] = out[name].data_ptr()
        if flat.numel():
            L.check(L.lib.clipops_handover_bwd_f32(
                g_base.data_ptr(), table.data_ptr(), inv_q.data_ptr(), inv_prev.data_ptr() if n_tracks else None,
                n_keep, n_q, n_det, n_tracks, K, C, int(use_dab), det_cols, ctypes.byref(grads), _stream(g_base)),
                "clipops_handover_bwd_f32")
        return tuple(out.get(name) for name in HANDOVER_DIFF) + (None,) * 10


def handover(outputs, queries, last_ref, init_ref, det_embed, prev_ref, prev_long, prev_last, prev_query, logits, boxes,
             prev_iou, prev_ids, prev_matched, gt_boxes, gt_ids, tables, n_keep: int, n_det: int):
    """The active track set of the next frame as ONE gather (and one scatter backward): -> (base (n_keep, W) with the
    columns of ``TrackInstances.PACKED_FLOAT``, ids (n_keep,), matched_idx (n_keep,)).  The nine leading arguments are
    the differentiable sources (``HANDOVER_DIFF``; ``det_embed`` None: DAB queries of width C); ``logits``, ``boxes``
    and ``prev_iou`` are copied without a gradient (the composed path's gradient for them is exactly zero: the query
    updater reads the logits through a comparison and the boxes detached).  All 2-d with dense columns, any row stride;
    ``tables`` from ``handover_tables``, on the device.  See include/clip_ops_hip.h for the row kinds."""
    base, ints = _Handover.apply(outputs, queries, last_ref, init_ref, det_embed, prev_ref, prev_long, prev_last,
                                 prev_query, logits, boxes, prev_iou, prev_ids, prev_matched, gt_boxes, gt_ids, tables,
                                 n_keep, n_det)
    return base, ints[0], ints[1]


def handover_reference(outputs, queries, last_ref, init_ref, det_embed, prev_ref, prev_long, prev_last, prev_query,
                       logits, boxes, prev_iou, prev_ids, prev_matched, gt_boxes, gt_ids, tables, n_keep: int,
                       n_det: int):
    """``handover`` as torch gathers and selects (differentiable through autograd; what CPU tensors run)."""
    n_q, C = outputs.shape
    n_tracks = prev_ref.shape[0]
    table, _, _ = _handover_views(tables, n_keep, n_q, n_tracks)
    kind, s, g = table.view(n_keep, 3).unbind(1)
    carried, new = (kind == HANDOVER_CARRIED), (kind == HANDOVER_NEW)
    m = torch.where(carried, n_det + s, s)                     # row of the model's outputs
    q = torch.where(carried, torch.zeros_like(s), s)           # detect query (any valid row where it is not read)

    def prev(t):
        width = 1 if t.dim() == 1 else t.shape[1]
        if n_tracks == 0:
            return t.new_zeros((n_keep, width))
        return t.reshape(n_tracks, width)[torch.where(carried, s, torch.zeros_like(s))]

    col = carried[:, None]
    det_q = queries[q] if det_embed is None else torch.cat((det_embed[q][:, :C], queries[q]), dim=-1)
    box = boxes[m]
    ref = torch.where(col, prev(prev_ref), torch.where(new[:, None], last_ref[q], init_ref[q]))
    g_own = torch.where(carried, prev(prev_matched).reshape(-1), g)
    iou_gt = pair_iou_reference(box.detach(), gt_boxes, g_own.clamp(min=0))
    iou = torch.where(carried, torch.where(g_own >= 0, iou_gt, prev(prev_iou).reshape(-1)),
                      torch.where(new, iou_gt, torch.zeros_like(iou_gt)))
    ids = torch.where(carried, prev(prev_ids).reshape(-1), torch.where(new, gt_ids[g.clamp(min=0)], torch.full_like(g, -1)))
    base = torch.cat((logits[m].detach(), box.detach(), ref, outputs[m], torch.where(col, prev(prev_long), queries[q]),
                      torch.where(col, prev(prev_last), outputs[q]), torch.where(col, prev(prev_query), det_q),
                      iou[:, None]), dim=1)
    ids = torch.where(iou < 0.5, torch.full_like(ids, -1), ids)
    matched = torch.where(carried, g_own, torch.where(new, g, torch.full_like(g, -1)))
    return base, ids, matched


# --------------------------------------------------------------------------------------------------------------
# focal loss of stacked layers (models/criterion.py of the reference, :442-467)
# --------------------------------------------------------------------------------------------------------------
class _FocalPerLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, alpha, gamma):
        n_layers, Nq, K = logits.shape
        sl, sq = _strides3(logits)
        loss = torch.empty((n_layers,), dtype=torch.float32, device=logits.device)
        L = _lib()
        L.check(L.lib.clipops_focal_fwd_f32(logits.data_ptr(), sl, sq, labels.data_ptr(), n_layers, Nq, K, alpha, gamma,
                                            loss.data_ptr(), _stream(logits)), "clipops_focal_fwd_f32")
        ctx.save_for_backward(logits, labels)
        ctx.alpha, ctx.gamma = alpha, gamma
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels = ctx.saved_tensors
        n_layers, Nq, K = logits.shape
        sl, sq = _strides3(logits)
        grad = torch.empty((n_layers, Nq, K), dtype=torch.float32, device=logits.device)
        L = _lib()
        L.check(L.lib.clipops_focal_bwd_f32(logits.data_ptr(), sl, sq, labels.data_ptr(), n_layers, Nq, K, ctx.alpha,
                                            ctx.gamma, g.contiguous().data_ptr(), grad.data_ptr(), _stream(logits)),
                "clipops_focal_bwd_f32")
        return grad, None, None, None


def focal_loss_per_layer(logits: torch.Tensor, labels: torch.Tensor, alpha: float = 0.25, gamma: float = 2.0):
    """(n_layers, Nq, K) logits (a view is fine), (n_layers, Nq) int64 labels with K = background -> (n_layers,)
    sigmoid focal loss, mean over classes and sum over queries."""
    return _FocalPerLayer.apply(logits, labels.contiguous(), float(alpha), float(gamma))


def focal_loss_per_layer_reference(logits, labels, alpha: float = 0.25, gamma: float = 2.0):
    from ..models.criterion import sigmoid_focal_loss_per_layer
    K = logits.shape[-1]
    one_hot = F.one_hot(labels, K + 1)[..., :-1].to(logits.dtype)
    return sigmoid_focal_loss_per_layer(logits, one_hot, alpha, gamma)


# --------------------------------------------------------------------------------------------------------------
# decoder glue: sine embedding of the anchors, clamped logit, box refinement
# --------------------------------------------------------------------------------------------------------------
class _SineEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, dim_t, scale):
        K, F_ = pos.shape[-1], dim_t.shape[0]
        n = pos.numel() // K
        out = torch.empty(pos.shape[:-1] + (K * F_,), dtype=torch.float32, device=pos.device)
        L = _lib()
        L.check(L.lib.clipops_sine_embed_fwd_f32(pos.data_ptr(), dim_t.data_ptr(), n, K, F_, scale, out.data_ptr(),
                                                 _stream(pos)), "clipops_sine_embed_fwd_f32")
        ctx.save_for_backward(pos, dim_t)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        pos, dim_t = ctx.saved_tensors
        K, F_ = pos.shape[-1], dim_t.shape[0]
        grad = torch.empty_like(pos)
        L = _lib()
        L.check(L.lib.clipops_sine_embed_bwd_f32(pos.data_ptr(), dim_t.data_ptr(), pos.numel() // K, K, F_, ctx.scale,
                                                 g.contiguous().data_ptr(), grad.data_ptr(), _stream(pos)),
                "clipops_sine_embed_bwd_f32")
        return grad, None, None


def sine_embed(pos: torch.Tensor, dim_t: torch.Tensor, scale: float) -> torch.Tensor:
    """(..., K) -> (..., K * F): out[..., k*F + j] = (sin | cos)(pos[..., k] * scale / dim_t[j]), even j sin, odd j cos."""
    return _SineEmbed.apply(pos.contiguous(), dim_t, float(scale))


class _InverseSigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        y = torch.empty_like(x)
        L = _lib()
        L.check(L.lib.clipops_inverse_sigmoid_fwd_f32(x.data_ptr(), x.numel(), eps, y.data_ptr(), _stream(x)),
                "clipops_inverse_sigmoid_fwd_f32")
        ctx.save_for_backward(x)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        gx = torch.empty_like(x)
        L = _lib()
        L.check(L.lib.clipops_inverse_sigmoid_bwd_f32(x.data_ptr(), g.contiguous().data_ptr(), x.numel(), ctx.eps,
                                                      gx.data_ptr(), _stream(x)), "clipops_inverse_sigmoid_bwd_f32")
        return gx, None


def inverse_sigmoid(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return _InverseSigmoid.apply(x.contiguous(), float(eps))


class _RefineBoxes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, delta, ref, eps):
        out = torch.empty_like(delta)
        L = _lib()
        L.check(L.lib.clipops_refine_boxes_fwd_f32(delta.data_ptr(), ref.data_ptr(), delta.numel(), eps, out.data_ptr(),
                                                   _stream(delta)), "clipops_refine_boxes_fwd_f32")
        ctx.save_for_backward(out, ref)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, g):
        out, ref = ctx.saved_tensors
        gd = torch.empty_like(out)
        gr = torch.empty_like(out) if ctx.needs_input_grad[1] else None
        L = _lib()
        L.check(L.lib.clipops_refine_boxes_bwd_f32(out.data_ptr(), ref.data_ptr(), g.contiguous().data_ptr(),
                                                   out.numel(), ctx.eps, gd.data_ptr(),
                                                   None if gr is None else gr.data_ptr(), _stream(out)),
                "clipops_refine_boxes_bwd_f32")
        return gd, gr, None


def refine_boxes(delta: torch.Tensor, ref: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """sigmoid(delta + inverse_sigmoid(ref)) for same-shaped tensors."""
    if delta.shape != ref.shape:
        raise RuntimeError("refine_boxes: delta and ref must have the same shape")
    return _RefineBoxes.apply(delta.contiguous(), ref.contiguous(), float(eps))


class _RefineBoxesSplit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, delta, ref, eps):
        head, dec = torch.empty_like(delta), torch.empty_like(delta)
        L = _lib()
        L.check(L.lib.clipops_refine_boxes_split_fwd_f32(delta.data_ptr(), ref.data_ptr(), delta.numel() // 4, eps,
                                                         head.data_ptr(), dec.data_ptr(), _stream(delta)),
                "clipops_refine_boxes_split_fwd_f32")
        ctx.save_for_backward(head, ref)
        ctx.eps = eps
        ctx.mark_non_differentiable(dec)
        return head, dec

    @staticmethod
    def backward(ctx, g, _g_dec):
        return _RefineBoxes.backward(ctx, g)         # the refine backward on `head`: `dec` carries no gradient


def refine_boxes_split_reference(delta: torch.Tensor, ref: torch.Tensor, eps: float = 1e-5):
    """The host statement of ``refine_boxes_split``: the model's box head at level 0 (reference models/memotr.py:148-158)
    and the decoder's own refinement from the 2-d slice of the reference (models/deformable_decoder.py:141-149)."""
    from ..utils.utils import inverse_sigmoid_reference
    head = (delta + inverse_sigmoid_reference(ref, eps)).sigmoid()
    with torch.no_grad():
        xy = delta[..., :2] + inverse_sigmoid_reference(ref[..., :2], eps)
        dec = torch.cat((xy, delta[..., 2:]), -1).sigmoid()
    return head, dec


def refine_boxes_split(delta: torch.Tensor, ref: torch.Tensor, eps: float = 1e-5):
    """Layer 0 of the Deformable-DETR variant, (..., 4) tensors of one shape -> (head, dec):
    head = sigmoid(delta + inverse_sigmoid(ref)), differentiable; dec = (head xy, sigmoid(delta wh)), no gradient.
    One kernel for CUDA fp32 tensors, the torch composition for everything else."""
    if delta.shape != ref.shape or delta.shape[-1] != 4:
        raise RuntimeError("refine_boxes_split: delta and ref must have the same (..., 4) shape")
    if fused(delta, ref) and delta.dtype == torch.float32 and ref.dtype == torch.float32:
        return _RefineBoxesSplit.apply(delta.contiguous(), ref.contiguous(), float(eps))
    return refine_boxes_split_reference(delta, ref, eps)


# --------------------------------------------------------------------------------------------------------------
# bias gradients of the query-sized linears
# --------------------------------------------------------------------------------------------------------------
COLSUM_MAX_ROWS = 2048          # one pass of the tile kernel
COLSUM_CHUNK_ROWS = 256         # tall matrices: partial sums per 256 rows, then one pass over the partials


def colsum(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """x.sum(0) of a contiguous 2-d CUDA matrix through the tiled kernels (fixed summation order, fp32 sums and result):
    fp32 input -- one pass up to COLSUM_MAX_ROWS rows, two passes (per-chunk partial sums, then the partials) above;
    bf16 input -- always the two-pass form.  Anything else takes torch's reduction.  ``out`` may be a contiguous
    fp32 (cols,) destination."""
    b16 = x.dtype == torch.bfloat16
    ok = (x.dim() == 2 and x.is_contiguous() and x.is_cuda and (x.dtype == torch.float32 or b16)
          and os.environ.get("MEMOTR_FUSED_CLIP_OPS", "1") != "0"
          and (out is None or (out.is_contiguous() and out.dtype == torch.float32))
          and 0 < x.shape[0] <= COLSUM_MAX_ROWS * COLSUM_CHUNK_ROWS)
    if not ok:
        return torch.sum(x, 0, out=out) if out is not None else x.sum(0)
    if x.shape[0] > COLSUM_MAX_ROWS and not b16 and os.environ.get("MEMOTR_COLSUM_TALL", "1") == "0":
        return torch.sum(x, 0, out=out) if out is not None else x.sum(0)
    L = _lib()
    if x.shape[0] > COLSUM_MAX_ROWS or b16:
        chunks = -(-x.shape[0] // COLSUM_CHUNK_ROWS)
        partial = torch.empty((chunks, x.shape[1]), dtype=torch.float32, device=x.device)
        fn = L.lib.clipops_colsum_partial_bf16 if b16 else L.lib.clipops_colsum_partial_f32
        L.check(fn(x.data_ptr(), x.shape[0], x.shape[1], COLSUM_CHUNK_ROWS, partial.data_ptr(), _stream(x)),
                "clipops_colsum_partial")
        x = partial
    if out is None:
        out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    L.check(L.lib.clipops_colsum_f32(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), _stream(x)),
            "clipops_colsum_f32")
    return out


def relu_bwd_colsum_usable(g: torch.Tensor, y: torch.Tensor) -> bool:
    return (os.environ.get("MEMOTR_FUSED_CLIP_OPS", "1") != "0" and os.environ.get("MEMOTR_FUSED_RELU_COLSUM", "1") != "0"
            and g.is_cuda and g.dim() == 2 and g.is_contiguous() and y.is_contiguous() and y.shape == g.shape
            and g.dtype == y.dtype and g.dtype == torch.float32        # (bf16: 546 vs 358 us for the two torch passes)
            and COLSUM_MAX_ROWS < g.shape[0] <= COLSUM_MAX_ROWS * COLSUM_CHUNK_ROWS)


def relu_bwd_colsum(g: torch.Tensor, y: torch.Tensor):
    """(g * (y > 0), its column sums in fp32) for tall contiguous (rows, cols) matrices: the ReLU mask of a fused-ReLU
    Linear's backward and its bias gradient with ONE pass over the gradient instead of two."""
    rows, cols = g.shape
    chunks = -(-rows // COLSUM_CHUNK_ROWS)
    g2 = torch.empty_like(g)
    partial = torch.empty((chunks, cols), dtype=torch.float32, device=g.device)
    out = torch.empty((cols,), dtype=torch.float32, device=g.device)
    L = _lib()
    fn = L.lib.clipops_relu_bwd_colsum_partial_f32
    L.check(fn(g.data_ptr(), y.data_ptr(), rows, cols, COLSUM_CHUNK_ROWS, g2.data_ptr(), partial.data_ptr(), _stream(g)),
            "clipops_relu_bwd_colsum_partial")
    L.check(L.lib.clipops_colsum_f32(partial.data_ptr(), chunks, cols, out.data_ptr(), _stream(g)), "clipops_colsum_f32")
    return g2, out


class _AddRowBias(torch.autograd.Function):
    """x (..., C) + bias (C,): the bias gradient through the tiled column sums instead of torch's reduction."""

    @staticmethod
    def forward(ctx, x, bias):
        return x + bias

    @staticmethod
    def backward(ctx, g):
        gb = None
        if ctx.needs_input_grad[1]:
            g2 = g.reshape(-1, g.shape[-1])
            gb = colsum(g2 if g2.is_contiguous() else g2.contiguous())
        return (g if ctx.needs_input_grad[0] else None), gb


def add_row_bias(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    if x.is_cuda and bias.requires_grad and torch.is_grad_enabled() and bias.dim() == 1:
        return _AddRowBias.apply(x, bias)
    return x + bias


# --------------------------------------------------------------------------------------------------------------
# backward of a query-sized Linear in one launch (include/clip_ops_hip.h: clipops_linear_bwd_f32)
# --------------------------------------------------------------------------------------------------------------
LINEAR_BWD_MAX_ROWS = 1024          # beyond a few hundred rows the library GEMMs win
LINEAR_BWD_MAX_OUT = 512            # ... and for wide outputs too: 32 x 32 tiles re-read their operands from L2 (measured
                                    # inside a graph at 320 rows, tools/linear_bwd_probe.py: 256 -> 256: 6.5 vs 14.5 us for
                                    # the chain, with ReLU 10.5 vs 18.4; 256 -> 768: 12.7 vs 11.5; 256 -> 1024: 18.4 vs 17.9)


def linear_bwd_usable(g2: torch.Tensor, x2: torch.Tensor, weight: torch.Tensor) -> bool:
    return (os.environ.get("MEMOTR_FUSED_LINEAR_BWD", "1") != "0" and fused(g2, x2, weight)
            and g2.dtype == torch.float32 and x2.dtype == torch.float32 and weight.dtype == torch.float32
            and 0 < g2.shape[0] <= LINEAR_BWD_MAX_ROWS and g2.shape[1] <= LINEAR_BWD_MAX_OUT
            and x2.is_contiguous() and weight.is_contiguous())


def linear_bwd(g2: torch.Tensor, y_relu, x2: torch.Tensor, weight: torch.Tensor, need_x=True, need_w=True, need_b=True,
               gw_out: torch.Tensor = None, gb_out: torch.Tensor = None):
    """(grad_x, grad_w, grad_b) of y = x2 @ weight.T + b for g2 = d/dy (rows, out); ``y_relu``: the forward's output
    when it applied a ReLU (the mask y > 0 is then part of the kernel).  ``gw_out`` / ``gb_out``: contiguous buffers
    to write into (row slices of a packed parameter's gradient)."""
    g2 = g2.contiguous()
    rows, out_f = g2.shape
    in_f = x2.shape[1]
    need_w = need_w or need_b
    gx = torch.empty((rows, in_f), dtype=torch.float32, device=g2.device) if need_x else None
    gw = (gw_out if gw_out is not None else torch.empty((out_f, in_f), dtype=torch.float32, device=g2.device)) if need_w else None
    gb = (gb_out if gb_out is not None else torch.empty((out_f,), dtype=torch.float32, device=g2.device)) if need_b else None
    assert gw is None or (gw.is_contiguous() and gw.shape == (out_f, in_f)), "gw_out must be a contiguous (out, in) buffer"
    assert gb is None or (gb.is_contiguous() and gb.shape == (out_f,)), "gb_out must be a contiguous (out,) buffer"
    L_ = _lib()
    L_.check(L_.lib.clipops_linear_bwd_f32(g2.data_ptr(), None if y_relu is None else y_relu.data_ptr(), x2.data_ptr(),
                                           weight.data_ptr(), rows, in_f, out_f,
                                           None if gx is None else gx.data_ptr(), None if gw is None else gw.data_ptr(),
                                           None if gb is None else gb.data_ptr(), _stream(g2)), "clipops_linear_bwd_f32")
    return gx, gw, gb


LINEAR_FWD_MAX_IN = 256             # (inside a graph, 320 rows: 256 -> 256 5.0 vs 5.4 us for the library, 512 -> 256 7.4 vs 6.0)


def linear_fwd_usable(x2: torch.Tensor, weight: torch.Tensor, bias) -> bool:
    return (os.environ.get("MEMOTR_FUSED_LINEAR_FWD", "1") != "0" and fused(x2, weight)
            and x2.dtype == torch.float32 and weight.dtype == torch.float32
            and 0 < x2.shape[0] <= LINEAR_BWD_MAX_ROWS and weight.shape[0] <= LINEAR_BWD_MAX_OUT
            and x2.shape[1] % 4 == 0 and x2.shape[1] <= LINEAR_FWD_MAX_IN and x2.is_contiguous() and weight.is_contiguous()
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous())))


def linear_fwd(x2: torch.Tensor, weight: torch.Tensor, bias, relu: bool) -> torch.Tensor:
    """[relu](x2 @ weight.T + bias) for a few hundred rows: one 5 us launch where the library GEMM takes 7-8."""
    rows, in_f = x2.shape
    out_f = weight.shape[0]
    y = torch.empty((rows, out_f), dtype=torch.float32, device=x2.device)
    L_ = _lib()
    L_.check(L_.lib.clipops_linear_fwd_f32(x2.data_ptr(), weight.data_ptr(), None if bias is None else bias.data_ptr(),
                                           rows, in_f, out_f, 1 if relu else 0, y.data_ptr(), _stream(x2)),
             "clipops_linear_fwd_f32")
    return y


def linear_bwd_reference(g2, y_relu, x2, weight):
    if y_relu is not None:
        g2 = g2 * (y_relu > 0).to(g2.dtype)
    return g2 @ weight, g2.t() @ x2, g2.sum(0)


# --------------------------------------------------------------------------------------------------------------
# the backbone's element-wise tail: frozen-BN shift (+ residual) + ReLU in one pass (include/clip_ops_hip.h, ABI 9)
# --------------------------------------------------------------------------------------------------------------
class _ShiftRelu(torch.autograd.Function):
    """y = relu(x + shift[None, :, None, None] (+ res)), written over ``x`` (a convolution's fresh output)."""

    @staticmethod
    def forward(ctx, x, shift, res):
        N, C, H, W = x.shape
        L_ = _lib()
        fn = L_.lib.clipops_shift_relu_bf16 if x.dtype == torch.bfloat16 else L_.lib.clipops_shift_relu_f32
        L_.check(fn(x.data_ptr(), shift.data_ptr(), None if res is None else res.data_ptr(), N * C, C, H * W,
                    _stream(x)), "clipops_shift_relu")
        ctx.mark_dirty(x)
        ctx.save_for_backward(x)
        ctx.has_res = res is not None
        return x

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        gx = torch.ops.aten.threshold_backward(g, y, 0)      # (the ReLU's own backward kernel; the shift is a constant)
        return gx, None, (gx if ctx.has_res else None)


def shift_relu_reference(x: torch.Tensor, shift: torch.Tensor, res: torch.Tensor = None) -> torch.Tensor:
    y = x + shift.to(x.dtype)[None, :, None, None]
    if res is not None:
        y = y + res
    return F.relu(y)


def shift_relu_(x: torch.Tensor, shift: torch.Tensor, res: torch.Tensor = None) -> torch.Tensor:
    """relu(x + per-channel shift (+ res)) over an NCHW tensor; in place on CUDA fp32 / bf16 (``x`` must be a tensor
    nothing else reads: the output of the convolution in front), the element-wise torch chain elsewhere."""
    ok = (os.environ.get("MEMOTR_FUSED_CLIP_OPS", "1") != "0" and os.environ.get("MEMOTR_FUSED_SHIFT_RELU", "1") != "0"
          and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous()
          and not x._is_view() and shift.dtype == torch.float32 and shift.is_contiguous() and not shift.requires_grad
          and (res is None or (res.dtype == x.dtype and res.shape == x.shape and res.is_contiguous())))
    if not ok:
        return shift_relu_reference(x, shift, res)
    return _ShiftRelu.apply(x, shift, res)


# --------------------------------------------------------------------------------------------------------------
# self-attention over the decoder queries (head_dim 32)
# --------------------------------------------------------------------------------------------------------------
MHA_MAX_L = 512
MHA_HEAD_DIM = 32


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qk_p, v_p, key_mask, n_heads):
        B, L, E2 = qk_p.shape
        E = E2 // 2
        out = torch.empty((B, L, E), dtype=torch.float32, device=qk_p.device)
        lse = torch.empty((B, n_heads, L), dtype=torch.float32, device=qk_p.device)
        scale = 1.0 / (E // n_heads) ** 0.5
        mk = None if key_mask is None else key_mask.data_ptr()
        L_ = _lib()
        L_.check(L_.lib.clipops_mha_fwd_f32(qk_p.data_ptr(), qk_p.data_ptr() + 4 * E, v_p.data_ptr(), L * E2, E2, L * E2,
                                            E2, L * E, E, mk, B, n_heads, L, scale, out.data_ptr(), lse.data_ptr(),
                                            _stream(qk_p)), "clipops_mha_fwd_f32")
        ctx.save_for_backward(qk_p, v_p, key_mask, out, lse)
        ctx.n_heads, ctx.scale = n_heads, scale
        return out

    @staticmethod
    def backward(ctx, g):
        qk_p, v_p, key_mask, out, lse = ctx.saved_tensors
        B, L, E2 = qk_p.shape
        E = E2 // 2
        g = g.contiguous()
        g_qk, g_v = torch.empty_like(qk_p), torch.empty_like(v_p)
        mk = None if key_mask is None else key_mask.data_ptr()
        L_ = _lib()
        L_.check(L_.lib.clipops_mha_bwd_f32(qk_p.data_ptr(), qk_p.data_ptr() + 4 * E, v_p.data_ptr(), L * E2, E2, L * E2,
                                            E2, L * E, E, mk, out.data_ptr(), lse.data_ptr(), g.data_ptr(), B, ctx.n_heads,
                                            L, ctx.scale, g_qk.data_ptr(), L * E2, E2, g_qk.data_ptr() + 4 * E, L * E2,
                                            E2, g_v.data_ptr(), L * E, E, _stream(qk_p)), "clipops_mha_bwd_f32")
        return g_qk, g_v, None, None


class _Attention3(torch.autograd.Function):
    """The same kernels for separately projected q, k, v (B, L, E) -- the query updater's memory attention, whose
    queries and keys come from different inputs.  ``key_mask`` (B, L) bool, True = ignore that key (the padded slots of
    the captured update, models/updater_graphs.py), or None."""

    @staticmethod
    def forward(ctx, q_p, k_p, v_p, key_mask, n_heads):
        B, L, E = q_p.shape
        out = torch.empty((B, L, E), dtype=torch.float32, device=q_p.device)
        lse = torch.empty((B, n_heads, L), dtype=torch.float32, device=q_p.device)
        scale = 1.0 / (E // n_heads) ** 0.5
        mk = None if key_mask is None else key_mask.data_ptr()
        L_ = _lib()
        L_.check(L_.lib.clipops_mha_fwd_f32(q_p.data_ptr(), k_p.data_ptr(), v_p.data_ptr(), L * E, E, L * E, E, L * E, E,
                                            mk, B, n_heads, L, scale, out.data_ptr(), lse.data_ptr(), _stream(q_p)),
                 "clipops_mha_fwd_f32")
        ctx.save_for_backward(q_p, k_p, v_p, key_mask, out, lse)
        ctx.n_heads, ctx.scale = n_heads, scale
        return out

    @staticmethod
    def backward(ctx, g):
        q_p, k_p, v_p, key_mask, out, lse = ctx.saved_tensors
        B, L, E = q_p.shape
        g = g.contiguous()
        g_q, g_k, g_v = torch.empty_like(q_p), torch.empty_like(k_p), torch.empty_like(v_p)
        mk = None if key_mask is None else key_mask.data_ptr()
        L_ = _lib()
        L_.check(L_.lib.clipops_mha_bwd_f32(q_p.data_ptr(), k_p.data_ptr(), v_p.data_ptr(), L * E, E, L * E, E, L * E, E,
                                            mk, out.data_ptr(), lse.data_ptr(), g.data_ptr(), B, ctx.n_heads, L,
                                            ctx.scale, g_q.data_ptr(), L * E, E, g_k.data_ptr(), L * E, E,
                                            g_v.data_ptr(), L * E, E, _stream(q_p)), "clipops_mha_bwd_f32")
        return g_q, g_k, g_v, None, None


def attention(q_p: torch.Tensor, k_p: torch.Tensor, v_p: torch.Tensor, n_heads: int, key_padding_mask=None) -> torch.Tensor:
    """softmax(q k^T / sqrt(d)) v per head for projected (B, L, E) inputs of one common length; (B, L, E) out.
    ``key_padding_mask`` (B, L) bool: True = that key takes no part."""
    mask = None if key_padding_mask is None else key_padding_mask.contiguous()
    return _Attention3.apply(q_p.contiguous(), k_p.contiguous(), v_p.contiguous(), mask, int(n_heads))


def attention_supported(q_p: torch.Tensor, k_p: torch.Tensor, n_heads: int) -> bool:
    return (os.environ.get("MEMOTR_ATTN_KERNELS", "1") != "0" and q_p.dim() == 3 and q_p.shape == k_p.shape
            and fused(q_p, k_p) and q_p.dtype == torch.float32
            and q_p.shape[2] % n_heads == 0 and q_p.shape[2] // n_heads == MHA_HEAD_DIM and 0 < q_p.shape[1] <= MHA_MAX_L)


def self_attention_supported(qk_p: torch.Tensor, n_heads: int, any_float: bool = False) -> bool:
    """``any_float``: the caller casts a bf16 / fp16 projection to float32 first (autocast island)."""
    B, L, E2 = qk_p.shape
    dtype_ok = qk_p.is_floating_point() if any_float else qk_p.dtype == torch.float32
    return (os.environ.get("MEMOTR_ATTN_KERNELS", "1") != "0" and os.environ.get("MEMOTR_FUSED_CLIP_OPS", "1") != "0"
            and qk_p.is_cuda and dtype_ok and E2 % (2 * n_heads) == 0
            and E2 // 2 // n_heads == MHA_HEAD_DIM and 0 < L <= MHA_MAX_L)


def self_attention(qk_p: torch.Tensor, v_p: torch.Tensor, key_padding_mask, n_heads: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(d)) v per head from the packed projections: qk_p (B, L, 2E) = [q | k], v_p (B, L, E);
    key_padding_mask (B, L) bool (True = ignore that key) or None.  Returns (B, L, E), heads concatenated -- the
    layout the output projection takes, no transposes or copies either side."""
    mask = None if key_padding_mask is None else key_padding_mask.contiguous()
    return _SelfAttention.apply(qk_p.contiguous(), v_p.contiguous(), mask, int(n_heads))


def self_attention_reference(qk_p, v_p, key_padding_mask, n_heads):
    B, L, E2 = qk_p.shape
    E, d = E2 // 2, E2 // 2 // n_heads
    q, k = (t.transpose(1, 2) for t in qk_p.view(B, L, 2, n_heads, d).unbind(2))
    v = v_p.view(B, L, n_heads, d).transpose(1, 2)
    att = (q @ k.transpose(-1, -2)) / d ** 0.5
    if key_padding_mask is not None:
        att = att.masked_fill(key_padding_mask.view(B, 1, 1, L), float("-inf"))
    return (att.softmax(-1) @ v).transpose(1, 2).reshape(B, L, E)


# --------------------------------------------------------------------------------------------------------------
# residual add + LayerNorm (rows of 256)
# --------------------------------------------------------------------------------------------------------------
LN_COLS = 256


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        s, y, _, stats = add_layer_norm_fwd(x, res, weight, bias, eps)
        ctx.save_for_backward(s, stats, weight)
        return y

    @staticmethod
    def backward(ctx, g):
        s, stats, weight = ctx.saved_tensors
        rows = s.numel() // LN_COLS
        g = g.contiguous()
        gs = torch.empty_like(s)
        chunk = 16 if rows <= 4096 else 64
        partial = torch.empty((-(-rows // chunk), 2 * LN_COLS), dtype=torch.float32, device=s.device)
        L = _lib()
        L.check(L.lib.clipops_add_layer_norm_bwd_f32(g.data_ptr(), s.data_ptr(), stats.data_ptr(), weight.data_ptr(), rows,
                                                     chunk, gs.data_ptr(), partial.data_ptr(), _stream(s)),
                "clipops_add_layer_norm_bwd_f32")
        gwb = colsum(partial)                       # [grad_gamma | grad_beta]
        return gs, gs, gwb[:LN_COLS], gwb[LN_COLS:], None


def add_layer_norm_fwd(x: torch.Tensor, res: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                       pos: torch.Tensor = None):
    """The forward kernel on contiguous fp32 (..., 256) tensors, outside autograd: (sum, y, q, stats) with
    q = y + pos from the same pass when ``pos`` is given (None otherwise); sum / stats are what the backward takes."""
    rows = x.numel() // LN_COLS
    s, y = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    L = _lib()
    if pos is None:
        L.check(L.lib.clipops_add_layer_norm_fwd_f32(x.data_ptr(), res.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                                     rows, eps, s.data_ptr(), y.data_ptr(), stats.data_ptr(), _stream(x)),
                "clipops_add_layer_norm_fwd_f32")
        return s, y, None, stats
    assert pos.shape == x.shape and pos.is_contiguous() and pos.dtype == torch.float32
    q = torch.empty_like(x)
    L.check(L.lib.clipops_add_layer_norm_pos_fwd_f32(x.data_ptr(), res.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                                     pos.data_ptr(), rows, eps, s.data_ptr(), y.data_ptr(), q.data_ptr(),
                                                     stats.data_ptr(), _stream(x)), "clipops_add_layer_norm_pos_fwd_f32")
    return s, y, q, stats


def _fanin_chunk_rows(rows: int) -> int:
    """Rows per workgroup of the fan-in backward: as the plain backward for short inputs; for long ones at most 1024
    chunks, so that the 2 rows per chunk of the column-sum partials stay within one pass of the finishing kernel."""
    if rows <= 4096:
        return 16
    per_chunk = -(-rows // 1024)
    return max(64, (per_chunk + 3) // 4 * 4)


def add_layer_norm_bwd_fanin(grads, s: torch.Tensor, stats: torch.Tensor, weight: torch.Tensor):
    """Backward of add_layer_norm for an output with up to three consumers: ``grads`` = (g0, g1, g2), contiguous fp32
    tensors shaped like ``s`` or None; the kernel sums the given ones in slot order in registers.  Returns
    (grad_sum, grad_gamma, grad_beta, column sums of grad_sum) -- the last is the bias gradient of the Linear whose
    output was the residual branch, from the same pass (fp64 sums, rounded once; no atomics)."""
    g0, g1, g2 = grads
    for g in grads:
        assert g is None or (g.is_contiguous() and g.dtype == torch.float32 and g.numel() == s.numel())
    rows = s.numel() // LN_COLS
    chunk = _fanin_chunk_rows(rows)
    chunks = -(-rows // chunk)
    gs = torch.empty_like(s)
    partial = torch.empty((chunks, 2 * LN_COLS), dtype=torch.float32, device=s.device)
    zpartial = torch.empty((2 * chunks, LN_COLS), dtype=torch.float32, device=s.device)
    out = torch.empty((3 * LN_COLS,), dtype=torch.float32, device=s.device)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    L = _lib()
    st = _stream(s)
    L.check(L.lib.clipops_add_layer_norm_fanin_bwd_f32(ptr(g0), ptr(g1), ptr(g2), s.data_ptr(), stats.data_ptr(),
                                                       weight.data_ptr(), rows, chunk, gs.data_ptr(), partial.data_ptr(),
                                                       zpartial.data_ptr(), st), "clipops_add_layer_norm_fanin_bwd_f32")
    L.check(L.lib.clipops_colsum_f32(partial.data_ptr(), chunks, 2 * LN_COLS, out.data_ptr(), st), "clipops_colsum_f32")
    L.check(L.lib.clipops_colsum_f32(zpartial.data_ptr(), 2 * chunks, LN_COLS, out.data_ptr() + 8 * LN_COLS, st),
            "clipops_colsum_f32")
    return gs, out[:LN_COLS], out[LN_COLS:2 * LN_COLS], out[2 * LN_COLS:]


def add_layer_norm_supported(x: torch.Tensor, res: torch.Tensor, norm) -> bool:
    """fp32 CUDA tensors; under autocast also bf16 / fp16 ones (see add_layer_norm)."""
    island = torch.is_autocast_enabled()
    ok_dtype = (lambda t: t.is_floating_point()) if island else (lambda t: t.dtype == torch.float32)
    return (isinstance(norm, torch.nn.LayerNorm) and norm.elementwise_affine and norm.bias is not None
            and tuple(norm.normalized_shape) == (LN_COLS,) and x.shape == res.shape and x.shape[-1] == LN_COLS
            and x.is_cuda and res.is_cuda and ok_dtype(x) and ok_dtype(res) and norm.weight.dtype == torch.float32
            and os.environ.get("MEMOTR_FUSED_CLIP_OPS", "1") != "0" and os.environ.get("MEMOTR_FUSED_LN", "1") != "0")


def add_layer_norm(x: torch.Tensor, res: torch.Tensor, norm) -> torch.Tensor:
    """norm(x + res) for an nn.LayerNorm over 256 features: one kernel forward (sum, statistics and output in one
    pass), one + a column sum backward; other shapes / dtypes / devices go through the module.

    Under autocast the kernel runs as an fp32 island: autocast itself evaluates layer_norm in float32 (and the sum
    ``x + res`` promotes to float32 as soon as one operand is), so casting the low-precision operand up front gives the
    values autocast would have produced -- through one kernel instead of add + native_layer_norm (+ their backward)."""
    if add_layer_norm_supported(x, res, norm):
        return _AddLayerNorm.apply(x.float().contiguous(), res.float().contiguous(), norm.weight, norm.bias,
                                   float(norm.eps))
    return norm(x + res)


# --------------------------------------------------------------------------------------------------------------
# track bank (models/track_bank.py; include/clip_ops_hip.h: clipops_bank_*): the online tracker's bookkeeping for B
# sequences on fixed-size slot tables
# --------------------------------------------------------------------------------------------------------------
def _bank_model_tensors(res: dict, bank, use_dab: bool):
    """The five decoder outputs the bank update reads, (B, n_det + cap, width) each, and det_query_embed (or None)."""
    named = dict(pred_logits=res["pred_logits"], pred_bboxes=res["pred_bboxes"], outputs=res["outputs"],
                 last_ref_pts=res["last_ref_pts"], queries=res["aux_outputs"][-1]["queries"])
    B, cap, K, C = bank.n_streams, bank.cap, bank.num_classes, bank.hidden_dim
    widths = dict(pred_logits=K, pred_bboxes=4, outputs=C, last_ref_pts=4, queries=C)
    rows = named["pred_logits"].shape[1] if named["pred_logits"].dim() == 3 else -1
    n_det = rows - cap
    if n_det < 0:
        raise ValueError(f"bank update: {rows} model rows for a bank of {cap} slots")
    for name, t in named.items():
        if t.dtype != torch.float32 or tuple(t.shape) != (B, rows, widths[name]) or t.device != bank.ids.device:
            raise ValueError(f"bank update: {name} has shape {tuple(t.shape)} ({t.dtype}, {t.device}); expected "
                             f"{(B, rows, widths[name])} float32 on {bank.ids.device}")
    det = None
    if not use_dab:
        det = res["det_query_embed"]
        if det.dtype != torch.float32 or det.dim() != 2 or det.shape[0] < n_det or det.shape[1] < C:
            raise ValueError(f"bank update: det_query_embed has shape {tuple(det.shape)} ({det.dtype})")
    return named, det, n_det


def _bank_update_structs(L, named, det, bank):
    """``(clipops_bank_model, clipops_bank, tensors to keep alive)`` of a bank update's launch."""
    model, keep = L.BankModel(), []
    for i, name in enumerate(L.BANK_MODEL):
        t = named[name].detach()
        if t.shape[2] > 1 and t.stride(2) != 1 or t.stride(0) < 0 or t.stride(1) < 0:
            t = t.contiguous()
        keep.append(t)
        model.ptr[i], model.batch_stride[i], model.row_stride[i] = t.data_ptr(), t.stride(0), t.stride(1)
    if det is not None:
        det = _rows_dense(det.detach())
        keep.append(det)
        model.det_embed, model.det_row_stride = det.data_ptr(), det.stride(0)
    table = L.Bank()
    for name in L.BANK_FIELDS:
        t = getattr(bank, name)
        if not t.is_contiguous():
            raise RuntimeError(f"bank update: the bank's {name} is not contiguous")
        setattr(table, name, t.data_ptr())
    return model, table, keep


def bank_update(res: dict, bank, det_score_thresh: float, track_score_thresh: float, miss_tolerance: int) -> None:
    """One frame of track management for every stream of ``bank`` (a ``TrackBank``), in place and without a read-back:
    ``RuntimeTracker.update`` plus the inference branch of ``QueryUpdater.select_active_tracks`` on slot tables (see
    include/clip_ops_hip.h: clipops_bank_update_f32).  ``res``: the model's outputs for queries ``cat(det, bank slots)``
    -- pred_logits, pred_bboxes, outputs, last_ref_pts, aux_outputs[-1]["queries"], each (B, n_det + cap, width) with a
    dense last axis, and det_query_embed without DAB.  CUDA tensors take one launch; CPU tensors run
    ``bank_update_reference``."""
    named, det, n_det = _bank_model_tensors(res, bank, bank.use_dab)
    if not bank.ids.is_cuda:
        return bank_update_reference(res, bank, det_score_thresh, track_score_thresh, miss_tolerance)
    L = _lib()
    model, table, keep = _bank_update_structs(L, named, det, bank)
    L.check(L.lib.clipops_bank_update_f32(
        ctypes.byref(model), ctypes.byref(table), bank.n_streams, n_det, bank.cap, bank.num_classes, bank.hidden_dim,
        int(bank.use_dab), float(det_score_thresh), float(track_score_thresh), int(miss_tolerance), _stream(bank.ids)),
        "clipops_bank_update_f32")


@torch.no_grad()
def bank_update_reference(res: dict, bank, det_score_thresh: float, track_score_thresh: float,
                          miss_tolerance: int) -> None:
    """``bank_update`` as torch selects and index copies, stream by stream (what CPU tensors run; reads row counts)."""
    named, det, n_det = _bank_model_tensors(res, bank, bank.use_dab)
    K, C = bank.num_classes, bank.hidden_dim
    for b in range(bank.n_streams):
        logits_all, boxes_all, out_all = named["pred_logits"][b], named["pred_bboxes"][b], named["outputs"][b]
        live = bank.ids[b] >= 0
        free_slots = (~live).nonzero().squeeze(1)                       # as they are before this call
        # live slots: refresh, age, retire
        logits = logits_all[n_det:]
        scores = logits.sigmoid()
        own = scores.gather(1, bank.labels[b].clamp(0, K - 1)[:, None]).squeeze(1)
        aged = torch.where(own < track_score_thresh, bank.disappear_time[b] + 1, torch.zeros_like(bank.disappear_time[b]))
        keep = live & ~(aged >= miss_tolerance)
        retire = live & ~keep
        col, gone = keep[:, None], retire[:, None]
        bank.disappear_time[b] = torch.where(keep, aged, torch.zeros_like(aged))
        bank.ids[b] = torch.where(retire, torch.full_like(bank.ids[b], -1), bank.ids[b])
        bank.labels[b] = torch.where(retire, torch.zeros_like(bank.labels[b]), bank.labels[b])
        for name, new in (("boxes", boxes_all[n_det:]), ("logits", logits), ("scores", scores),
                          ("output_embed", out_all[n_det:])):
            old = getattr(bank, name)[b]
            getattr(bank, name)[b] = torch.where(col, new, torch.where(gone, torch.zeros_like(old), old))
        for name in ("ref_pts", "long_memory", "last_output", "query_embed"):
            old = getattr(bank, name)[b]
            getattr(bank, name)[b] = torch.where(gone, torch.zeros_like(old), old)
        # births: the j-th born row takes the j-th free slot
        det_scores = logits_all[:n_det].sigmoid()
        if n_det > 0:
            top = torch.max(det_scores, dim=-1)
            born = (top.values >= det_score_thresh).nonzero().squeeze(1)
            label = top.indices
        else:
            born, label = free_slots[:0], free_slots[:0]
        placed = min(int(born.shape[0]), int(free_slots.shape[0]))
        rows, slots = born[:placed], free_slots[:placed]
        queries = named["queries"][b][rows]
        bank.ids[b][slots] = bank.next_id[b] + torch.arange(placed, dtype=torch.int64, device=rows.device)
        bank.labels[b][slots] = label[rows]
        bank.disappear_time[b][slots] = 0
        bank.logits[b][slots] = logits_all[rows]
        bank.scores[b][slots] = det_scores[rows]
        bank.boxes[b][slots] = boxes_all[rows]
        bank.ref_pts[b][slots] = named["last_ref_pts"][b][rows]
        bank.output_embed[b][slots] = out_all[rows]
        bank.last_output[b][slots] = out_all[rows]
        bank.long_memory[b][slots] = queries
        bank.query_embed[b][slots] = queries if det is None else torch.cat((det[rows][:, :C], queries), dim=-1)
        bank.next_id[b] += placed
        bank.counters[b, 0] = int(keep.sum()) + placed
        bank.counters[b, 1] += int(born.shape[0]) - placed


class StreamThresholds:
    """One setting per stream of a bank, as the device arrays the ``_streams`` entry points read: ``det``, ``track``,
    ``result``, ``area`` float32 (S,) and ``miss`` int64 (S,).  Built once per sweep; ``settings`` keeps the host values
    (``det_score_thresh``, ``track_score_thresh``, ``result_score_thresh``, ``miss_tolerance``, ``area_thresh``), which
    the host statements and the per-frame report read, so that nothing is read back from the arrays."""

    KEYS = ("det_score_thresh", "track_score_thresh", "result_score_thresh", "miss_tolerance")

    def __init__(self, settings, device, area_thresh: float = 100):
        settings = [dict(s) for s in settings]
        if not settings:
            raise ValueError("stream thresholds: at least one setting")
        for k, s in enumerate(settings):
            s.setdefault("area_thresh", area_thresh)
            unknown = sorted(set(s) - set(self.KEYS) - {"area_thresh"})
            missing = [key for key in self.KEYS if key not in s]
            if unknown or missing:
                raise ValueError(f"stream thresholds: setting {k} " + (f"has unknown keys {unknown}" if unknown else
                                                                        f"lacks {missing}"))
        self.settings = settings
        self.device = torch.device(device)
        col = lambda key, dtype: torch.tensor([s[key] for s in settings], dtype=dtype).to(self.device)   # noqa: E731
        self.det, self.track = col("det_score_thresh", torch.float32), col("track_score_thresh", torch.float32)
        self.result, self.area = col("result_score_thresh", torch.float32), col("area_thresh", torch.float32)
        self.miss = col("miss_tolerance", torch.int64)
        self.device = self.det.device                   # ("cuda" -> the current device, by name)

    def __len__(self) -> int:
        return len(self.settings)

    def _check(self, bank, what: str) -> None:
        if len(self) != bank.n_streams or self.device != bank.ids.device:
            raise ValueError(f"{what}: {len(self)} settings on {self.device} for a bank of {bank.n_streams} streams on "
                             f"{bank.ids.device}")


def _one_stream(res: dict, bank, b: int):
    """Stream ``b`` of a bank and of the model's outputs as a bank of one stream: views, so writes land in ``bank``."""
    import copy
    from ..models.track_bank import STREAM_FIELDS
    one = copy.copy(bank)
    for name in STREAM_FIELDS:
        setattr(one, name, getattr(bank, name)[b:b + 1])
    one.n_streams = 1
    if res is None:
        return None, one
    part = {name: res[name][b:b + 1] for name in ("pred_logits", "pred_bboxes", "outputs", "last_ref_pts")}
    part["aux_outputs"] = [{"queries": res["aux_outputs"][-1]["queries"][b:b + 1]}]
    if "det_query_embed" in res:
        part["det_query_embed"] = res["det_query_embed"]
    return part, one


def bank_update_streams(res: dict, bank, thresholds: StreamThresholds) -> None:
    """``bank_update`` with stream b under setting b of ``thresholds``: one launch of clipops_bank_update_streams_f32,
    whose stream b has the bits of ``bank_update`` made with that stream's values.  CPU tensors run
    ``bank_update_streams_reference``."""
    thresholds._check(bank, "bank update")
    named, det, n_det = _bank_model_tensors(res, bank, bank.use_dab)
    if not bank.ids.is_cuda:
        return bank_update_streams_reference(res, bank, thresholds)
    L = _lib()
    model, table, keep = _bank_update_structs(L, named, det, bank)
    L.check(L.lib.clipops_bank_update_streams_f32(
        ctypes.byref(model), ctypes.byref(table), bank.n_streams, n_det, bank.cap, bank.num_classes, bank.hidden_dim,
        int(bank.use_dab), thresholds.det.data_ptr(), thresholds.track.data_ptr(), thresholds.miss.data_ptr(),
        _stream(bank.ids)), "clipops_bank_update_streams_f32")


@torch.no_grad()
def bank_update_streams_reference(res: dict, bank, thresholds: StreamThresholds) -> None:
    """``bank_update_reference`` stream by stream, each with its own setting (what CPU tensors run)."""
    thresholds._check(bank, "bank update")
    for b, s in enumerate(thresholds.settings):
        part, one = _one_stream(res, bank, b)
        bank_update_reference(part, one, s["det_score_thresh"], s["track_score_thresh"], s["miss_tolerance"])


def _bank_rows_args(bank, seq_frame, ori_wh, rows_f, rows_i, counters) -> None:
    B, capacity = bank.n_streams, rows_f.shape[0]
    if (seq_frame.dtype != torch.int64 or tuple(seq_frame.shape) != (B, 2) or ori_wh.dtype != torch.float32
            or tuple(ori_wh.shape) != (B, 2)):
        raise ValueError(f"bank result rows: seq_frame {tuple(seq_frame.shape)} {seq_frame.dtype} / ori_wh "
                         f"{tuple(ori_wh.shape)} {ori_wh.dtype}; expected int64 and float32 of shape {(B, 2)}")
    if (rows_f.dtype != torch.float32 or rows_i.dtype != torch.int64 or tuple(rows_f.shape) != (capacity, 5)
            or tuple(rows_i.shape) != (capacity, 4) or counters.dtype != torch.int32 or counters.numel() != 2):
        raise ValueError("bank result rows: the table is rows_f (capacity, 5) float32, rows_i (capacity, 4) int64, "
                         "counters (2,) int32")


def bank_result_rows_streams(bank, seq_frame: torch.Tensor, ori_wh: torch.Tensor, thresholds: StreamThresholds,
                             rows_f: torch.Tensor, rows_i: torch.Tensor, counters: torch.Tensor) -> None:
    """``bank_result_rows`` with stream b filtered by ``thresholds.result[b]`` and ``thresholds.area[b]``: one launch of
    clipops_bank_result_rows_streams_f32.  CPU tensors run ``bank_result_rows_streams_reference``."""
    thresholds._check(bank, "bank result rows")
    _bank_rows_args(bank, seq_frame, ori_wh, rows_f, rows_i, counters)
    if not bank.ids.is_cuda:
        return bank_result_rows_streams_reference(bank, seq_frame, ori_wh, thresholds, rows_f, rows_i, counters)
    for t in (bank.boxes, bank.scores, bank.ids, bank.labels, seq_frame, ori_wh, rows_f, rows_i, counters,
              thresholds.result, thresholds.area):
        if not t.is_contiguous() or t.device != bank.ids.device:
            raise RuntimeError("bank result rows: every tensor is contiguous and on the bank's device")
    L = _lib()
    L.check(L.lib.clipops_bank_result_rows_streams_f32(
        bank.boxes.data_ptr(), bank.scores.data_ptr(), bank.ids.data_ptr(), bank.labels.data_ptr(), bank.n_streams,
        bank.cap, bank.num_classes, seq_frame.data_ptr(), ori_wh.data_ptr(), thresholds.result.data_ptr(),
        thresholds.area.data_ptr(), rows_f.data_ptr(), rows_i.data_ptr(), counters.data_ptr(), rows_f.shape[0],
        _stream(bank.ids)), "clipops_bank_result_rows_streams_f32")


@torch.no_grad()
def bank_result_rows_streams_reference(bank, seq_frame, ori_wh, thresholds, rows_f, rows_i, counters) -> None:
    """``bank_result_rows_reference`` stream by stream, each with its own setting (what CPU tensors run)."""
    thresholds._check(bank, "bank result rows")
    for b, s in enumerate(thresholds.settings):
        _, one = _one_stream(None, bank, b)
        bank_result_rows_reference(one, seq_frame[b:b + 1], ori_wh[b:b + 1], s["result_score_thresh"], s["area_thresh"],
                                   rows_f, rows_i, counters)


def bank_result_rows(bank, seq_frame: torch.Tensor, ori_wh: torch.Tensor, score_thresh: float, area_thresh: float,
                     rows_f: torch.Tensor, rows_i: torch.Tensor, counters: torch.Tensor) -> None:
    """The reportable rows of every stream's live tracks behind the rows already in the table (``rows_f`` (capacity, 5)
    float32, ``rows_i`` (capacity, 4) int64: sequence, frame, id, label; ``counters`` (2,) int32: stored, dropped) -- one
    launch, nothing read back.  ``seq_frame`` int64 (B, 2) and ``ori_wh`` float32 (B, 2) = (ori_w, ori_h) per stream,
    on the bank's device.  CPU tensors run ``bank_result_rows_reference``."""
    B, capacity = bank.n_streams, rows_f.shape[0]
    _bank_rows_args(bank, seq_frame, ori_wh, rows_f, rows_i, counters)
    if not bank.ids.is_cuda:
        return bank_result_rows_reference(bank, seq_frame, ori_wh, score_thresh, area_thresh, rows_f, rows_i, counters)
    for t in (bank.boxes, bank.scores, bank.ids, bank.labels, seq_frame, ori_wh, rows_f, rows_i, counters):
        if not t.is_contiguous() or t.device != bank.ids.device:
            raise RuntimeError("bank result rows: every tensor is contiguous and on the bank's device")
    L = _lib()
    L.check(L.lib.clipops_bank_result_rows_f32(
        bank.boxes.data_ptr(), bank.scores.data_ptr(), bank.ids.data_ptr(), bank.labels.data_ptr(), B, bank.cap,
        bank.num_classes, seq_frame.data_ptr(), ori_wh.data_ptr(), float(score_thresh), float(area_thresh),
        rows_f.data_ptr(), rows_i.data_ptr(), counters.data_ptr(), capacity, _stream(bank.ids)),
        "clipops_bank_result_rows_f32")


@torch.no_grad()
def bank_result_rows_reference(bank, seq_frame, ori_wh, score_thresh, area_thresh, rows_f, rows_i, counters) -> None:
    """``bank_result_rows`` through ``results.host_rows``, stream by stream (what CPU tensors run)."""
    from ..results import host_rows
    capacity = rows_f.shape[0]
    for b in range(bank.n_streams):
        live = bank.ids[b] >= 0
        seq, frame = (int(v) for v in seq_frame[b])
        f, i = host_rows(bank.boxes[b][live], bank.scores[b][live], bank.ids[b][live], bank.labels[b][live], frame,
                         ori_wh[b, 1], ori_wh[b, 0], score_thresh, area_thresh)
        at, m = int(counters[0]), int(f.shape[0])
        stored = max(0, min(m, capacity - at))
        rows_f[at:at + stored] = f[:stored]
        rows_i[at:at + stored, 0] = seq
        rows_i[at:at + stored, 1:] = i[:stored]
        counters[0] += stored
        counters[1] += m - stored


def _draw_table_args(boxes, scores, ids, ori_wh, font_scale):
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise ValueError(f"draw table: boxes {tuple(boxes.shape)}; expected (B, cap, 4)")
    B, cap = int(boxes.shape[0]), int(boxes.shape[1])
    scores = scores[:, :, None] if scores.dim() == 2 else scores
    if scores.dim() != 3 or tuple(scores.shape[:2]) != (B, cap):
        raise ValueError(f"draw table: scores {tuple(scores.shape)}; expected {(B, cap, 'K')}")
    if tuple(ids.shape) != (B, cap) or ids.dtype != torch.int64 or scores.shape[2] < 1:
        raise ValueError(f"draw table: ids {tuple(ids.shape)} {ids.dtype} / scores {tuple(scores.shape)}; expected int64 "
                         f"{(B, cap)} and {(B, cap, 'K')}")
    if tuple(ori_wh.shape) != (B, 2) or ori_wh.dtype != torch.float32:
        raise ValueError(f"draw table: ori_wh {tuple(ori_wh.shape)} {ori_wh.dtype}; expected float32 {(B, 2)}")
    if isinstance(font_scale, bool) or not isinstance(font_scale, int) or not 1 <= font_scale <= 64:
        raise ValueError(f"font_scale {font_scale!r} is not an integer in 1 .. 64")
    return B, cap, scores


@torch.no_grad()
def draw_table(boxes: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor, ori_wh: torch.Tensor, score_thresh: float,
               area_thresh: float, *, bgr: bool = False, font_scale: int = 1, out: torch.Tensor = None) -> torch.Tensor:
    """The overlay's int32 draw table (B, cap, 16) from tracks on the device (include/clip_ops_hip.h:
    clipops_draw_table_f32): the reportable slots of every stream in ascending id order as ``render.track_table`` rows,
    then padding rows that draw nothing -- one launch, nothing read back.  ``boxes`` (B, cap, 4) cxcywh normalised,
    ``scores`` (B, cap, K), ``ids`` int64 (B, cap) with -1 a free slot (a ``TrackBank``'s fields, or one sequence's
    ``TrackInstances`` fields with a leading axis of 1), ``ori_wh`` float32 (B, 2) = (ori_w, ori_h).  ``out``: an int32
    (B, cap, 16) tensor to write.  CPU tensors run ``draw_table_reference``."""
    B, cap, scores = _draw_table_args(boxes, scores, ids, ori_wh, font_scale)
    if out is None:
        out = torch.empty((B, cap, 16), dtype=torch.int32, device=boxes.device)
    elif tuple(out.shape) != (B, cap, 16) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f"draw table: out must be a contiguous int32 {(B, cap, 16)} tensor")
    if not boxes.is_cuda:
        out.copy_(draw_table_reference(boxes, scores, ids, ori_wh, score_thresh, area_thresh, bgr=bgr,
                                       font_scale=font_scale))
        return out
    boxes, scores = boxes.detach().float().contiguous(), scores.detach().float().contiguous()
    ids, ori_wh = ids.contiguous(), ori_wh.contiguous()
    for t in (scores, ids, ori_wh, out):
        if t.device != boxes.device:
            raise RuntimeError("draw table: every tensor is on the tracks' device")
    L = _lib()
    L.check(L.lib.clipops_draw_table_f32(
        boxes.data_ptr(), scores.data_ptr(), ids.data_ptr(), B, cap, scores.shape[2], ori_wh.data_ptr(),
        float(score_thresh), float(area_thresh), int(bool(bgr)), font_scale, out.data_ptr(), _stream(boxes)),
        "clipops_draw_table_f32")
    return out


@torch.no_grad()
def draw_table_reference(boxes, scores, ids, ori_wh, score_thresh, area_thresh, *, bgr: bool = False,
                         font_scale: int = 1) -> torch.Tensor:
    """``draw_table`` as a composition of what exists (what CPU tensors run): ``results.host_rows`` of a stream's live
    slots, sorted by id, through ``render.track_table``, then the padding rows 0, 0, -1, -1."""
    import numpy as np

    from ..render import ROW_WORDS, track_table
    from ..results import host_rows
    B, cap, scores = _draw_table_args(boxes, scores, ids, ori_wh, font_scale)
    boxes, scores, ids, ori_wh = boxes.detach().cpu(), scores.detach().cpu(), ids.cpu(), ori_wh.cpu()
    table = np.zeros((B, cap, ROW_WORDS), dtype=np.int32)
    table[:, :, 2:4] = -1
    for b in range(B):
        live = ids[b] >= 0
        ori_w, ori_h = float(ori_wh[b, 0]), float(ori_wh[b, 1])
        rows_f, rows_i = host_rows(boxes[b][live], scores[b][live], ids[b][live], torch.zeros_like(ids[b][live]), 0,
                                   ori_h, ori_w, score_thresh, area_thresh)
        order = torch.argsort(rows_i[:, 1], stable=True)
        m = int(order.shape[0])
        table[b, :m] = track_table(rows_i[order, 1], rows_f[order, :4], int(ori_w), int(ori_h), bgr=bgr,
                                   font_scale=font_scale)
    return torch.from_numpy(table)
