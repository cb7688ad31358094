"""Shared by tests/test_handover_cpu.py and tests/test_handover_gpu.py: one synthetic frame of a training clip in front of
the track hand-over -- model outputs, carried tracks and ground truths built so that every kind of row occurs -- and the
two routes from it to the next frame's active track set:

    composed:  ClipCriterion.finish_tracks -> QueryUpdater.select_active_tracks   (gathers, concatenations, a selection)
    fused:     ClipCriterion.finish_tracks, state["handover"]                       (one gather: clip_ops.handover)

Both start from ``build_frame`` with the same arguments (it is deterministic), since a route consumes its inputs.
"""
import torch

from memotr_amd.models.criterion import ClipCriterion
from memotr_amd.models.matcher import HungarianMatcher
from memotr_amd.models.query_updater import QueryUpdater
from memotr_amd.structures.track_instances import TrackInstances

C = 256
THRESHOLD = 0.5
# (nd, carried tracks, ground truths, K, use_dab, padded views): every value the kernels branch on occurs at least once
CASES = [
    (8, 0, 1, 1, True, False),
    (8, 1, 3, 8, False, True),
    (8, 7, 10, 1, True, True),
    (300, 7, 3, 1, True, False),
    (300, 1, 10, 8, False, True),
    (300, 0, 3, 1, False, False),
    (300, 7, 10, 8, True, True),
]
CASE_IDS = [f"nd{c[0]}-tr{c[1]}-gt{c[2]}-K{c[3]}-{'dab' if c[4] else 'detr'}-{'padded' if c[5] else 'dense'}" for c in CASES]

_UPDATERS = {}


def updater(use_dab: bool) -> QueryUpdater:
    """Only its selection of active tracks is used (no parameter takes part): one instance per variant."""
    if use_dab not in _UPDATERS:
        u = QueryUpdater(hidden_dim=C, ffn_dim=32, tp_drop_ratio=0.0, fp_insert_ratio=0.0, dropout=0.0,
                         use_checkpoint=False, use_dab=use_dab, update_threshold=THRESHOLD, long_memory_lambda=0.01)
        u.train()
        u.__dict__["_keep_rows_ok"] = True
        _UPDATERS[use_dab] = u
    return _UPDATERS[use_dab]


def _boxes(gen, n):
    return torch.cat((0.3 + 0.4 * torch.rand(n, 2, generator=gen), 0.1 + 0.2 * torch.rand(n, 2, generator=gen)), dim=1)


def build_frame(nd, n_tr, n_gt, K, use_dab, padded, device, empty_active=False):
    """-> (criterion, model_outputs, [tracks], leaves): ``leaves`` name -> the leaf tensor (requires_grad) behind every
    differentiable source, i.e. the buffers the padded views are cut from and the previous set's fields.

    Carried tracks (n_tr == 7): 0..2 own a ground truth (track 1's box is far from it: IoU < 0.5, the identity goes),
    3 and 4 carry an identity whose ground truth is gone (previous IoU 0.8: kept; 0.2: the identity goes), 5 and 6 are
    dead (id -1) with a score above / below the threshold (6 leaves the active set).  Detect queries: scores on both
    sides of the threshold, every other ground truth has a detect query right on top of it (IoU > 0.5: a new identity).
    ``empty_active``: no identity anywhere and every score below the threshold."""
    gen = torch.Generator().manual_seed(1000 * nd + 100 * n_tr + 10 * n_gt + K + (5 if use_dab else 0))
    QW = C if use_dab else 2 * C
    n_q = nd + n_tr
    gt_boxes = _boxes(gen, n_gt)
    gt_ids = 10 + torch.arange(n_gt)
    if empty_active:
        gt_ids = torch.full((n_gt,), -1, dtype=torch.long)
    logits = torch.randn(n_q, K, generator=gen) - (0.0 if K == 1 else 1.2)
    boxes = _boxes(gen, n_q)
    for i in range(0, min(n_gt, nd // 2), 2):
        boxes[2 * i + 1] = gt_boxes[i] + 0.004 * torch.rand(4, generator=gen)
    ids = torch.full((n_tr,), -1, dtype=torch.long)
    prev_iou = torch.rand(n_tr, generator=gen)
    for j in range(n_tr):
        if j < min(n_gt, 3):
            ids[j] = gt_ids[n_gt - 1 - j]
            boxes[nd + j] = gt_boxes[n_gt - 1 - j] + (0.3 if j == 1 else 0.004) * torch.rand(4, generator=gen)
        elif j in (3, 4):
            ids[j] = 900 + j
            prev_iou[j] = 0.8 if j == 3 else 0.2
        else:
            logits[nd + j] = 1.0 if j == 5 else -1.0
    if empty_active:
        logits = -logits.abs() - 0.1

    leaves = {}

    def source(name, value):
        """(1, rows, width) model output: a leaf, or -- padded -- a view of a larger leaf (rows and columns to spare)."""
        rows, width = value.shape
        if padded:
            buf = torch.zeros(1, rows + 3, width + 5)
            buf[0, :rows, :width] = value
            buf = buf.to(device).requires_grad_(True)
            leaves[name] = buf
            return buf[:, :rows, :width]
        leaves[name] = value[None].to(device).requires_grad_(True)
        return leaves[name]

    outputs = source("outputs", torch.randn(n_q, C, generator=gen))
    queries = source("queries", torch.randn(n_q, C, generator=gen))
    pred_logits = source("pred_logits", logits)
    pred_boxes = source("pred_bboxes", boxes)
    aux_logits = source("aux_logits", torch.randn(n_q, K, generator=gen))
    aux_boxes = source("aux_bboxes", _boxes(gen, n_q))
    last_ref = source("last_ref_pts", torch.randn(n_q, 4, generator=gen))
    init_ref = source("init_ref_pts", torch.randn(n_q, 4, generator=gen))
    leaves["det_query_embed"] = torch.randn(nd, QW, generator=gen).to(device).requires_grad_(True)
    model_outputs = {
        "pred_logits": pred_logits, "pred_bboxes": pred_boxes, "last_ref_pts": last_ref, "init_ref_pts": init_ref,
        "det_query_embed": leaves["det_query_embed"], "outputs": outputs,
        "query_mask": torch.zeros(1, n_q, dtype=torch.bool, device=device),
        "aux_outputs": [{"pred_logits": aux_logits, "pred_bboxes": aux_boxes, "queries": queries}],
    }

    tr = TrackInstances(hidden_dim=C, num_classes=K, use_dab=use_dab, device=device)
    if n_tr > 0:
        # as the query updater leaves them: column views of one packed tensor (row stride W, iou the last column)
        widths = [K, 4, 4, C, C, C, QW, 1]
        names = TrackInstances.PACKED_FLOAT
        cols = []
        for name, w in zip(names, widths):
            v = (prev_iou[:, None] if name == "iou" else torch.randn(n_tr, w, generator=gen)).to(device)
            if name in ("ref_pts", "long_memory", "last_output", "query_embed"):
                leaves["prev_" + name] = v.requires_grad_(True)
            cols.append(v)
        tr._set_packed(torch.cat(cols, dim=1), names, widths)
        tr.ids = ids.to(device)
        tr.matched_idx = torch.full((n_tr,), -1, dtype=torch.long, device=device)

    criterion = ClipCriterion(num_classes=K, matcher=HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2),
                              n_det_queries=nd, aux_loss=True, weight={"box_l1_loss": 5, "box_giou_loss": 2,
                                                                       "label_focal_loss": 2},
                              max_frame_length=2, n_aux=1, aux_weights=[1.0], hidden_dim=C, use_dab=use_dab)
    gt = TrackInstances(hidden_dim=C, num_classes=K, device=device)
    gt.ids, gt.labels, gt.boxes = gt_ids.to(device), (torch.arange(n_gt) % K).to(device), gt_boxes.to(device)
    criterion.device = torch.device(device)
    criterion.gt_trackinstances_list = [[gt]]
    criterion.n_gts, criterion.log = [], {}
    criterion.keep_threshold = THRESHOLD
    return criterion, model_outputs, [tr], leaves


def active_set(case, device, fused, empty_active=False):
    """The next frame's active tracks by one of the two routes: -> (TrackInstances, leaves, fused route taken?)."""
    nd, n_tr, n_gt, K, use_dab, padded = case
    criterion, model_outputs, tracks, leaves = build_frame(nd, n_tr, n_gt, K, use_dab, padded, device, empty_active)
    state = criterion.begin_frame(model_outputs, tracks, 0)
    state["handover"] = fused
    previous, new, unmatched = criterion.finish_tracks(state)
    assert "per_clip" in state and criterion.n_gts == [n_gt]
    handed = unmatched[0].__dict__.get("_keep_rows", (None,))[0]
    took_fused = isinstance(handed, TrackInstances)
    if took_fused:      # new / unmatched only count their rows
        assert new[0].query_embed.numel() == 0 and unmatched[0].query_embed.numel() == 0
    active = updater(use_dab).select_active_tracks(previous, new, unmatched)[0]
    assert not took_fused or active is handed
    return active, leaves, took_fused


def tensor_fields(t: TrackInstances):
    return {k: v for k, v in vars(t).items() if type(v) is torch.Tensor}


def assert_same_tracks(a: TrackInstances, b: TrackInstances):
    fa, fb = tensor_fields(a), tensor_fields(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        assert fa[k].shape == fb[k].shape and fa[k].dtype == fb[k].dtype and fa[k].device == fb[k].device, k
        assert torch.equal(fa[k], fb[k]), k
    assert (a.frame_height, a.frame_width, a.hidden_dim, a.num_classes) == \
        (b.frame_height, b.frame_width, b.hidden_dim, b.num_classes)


# what QueryUpdater.update_fields differentiates: it reads the logits through a comparison and the boxes detached, and
# nothing reads iou but thresholds
DIFFERENTIATED = ("ref_pts", "output_embed", "long_memory", "last_output", "query_embed")


def backward_through(t: TrackInstances, leaves):
    """d(sum of the differentiated fields x fixed weights) / d(leaves): name -> gradient (None: the leaf is not reached)."""
    gen = torch.Generator().manual_seed(7)
    total = 0
    for name in DIFFERENTIATED:
        v = getattr(t, name)
        total = total + (v * torch.randn(v.shape, generator=gen).to(v.device)).sum()
    names = list(leaves)
    grads = torch.autograd.grad(total, [leaves[n] for n in names], allow_unused=True)
    return dict(zip(names, grads))


def assert_same_grads(ga, gb):
    """Bit-equal gradients; a leaf one route does not reach must get exact zeros from the other."""
    assert ga.keys() == gb.keys()
    for k in ga:
        a, b = ga[k], gb[k]
        if a is None and b is None:
            continue
        if a is None or b is None:
            assert not bool((b if a is None else a).any()), k
            continue
        assert torch.equal(a, b), k
