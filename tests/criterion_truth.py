"""Test infrastructure: the clip criterion (models/criterion.py: ``begin_frame``, ``finish_tracks``, ``_handover``,
``finish_losses``, ``get_mean_by_n_gts``) against float64 truth on scripted multi-frame clips.  Shared by
tests/test_criterion_truth_cpu.py, tests/test_criterion_truth_gpu.py and tests/golden/gen_golden_criterion.py.

The criterion's inputs are plain tensors, so nothing here needs a model: ``frame_inputs`` scripts the decoder outputs of
every layer as leaves and puts every kind of row where it wants it (the constructions of tests/handover_cases.py:
detect queries on every other ground truth, tracks that stay on / drift off their ground truth, identities whose ground
truth is gone, dead tracks on both sides of the score threshold, padded slots behind the clip with fewer tracks).  The
number of track rows of frame t is only known once frame t - 1 has been processed, so the drivers materialise the recipe
frame by frame from the identities the active set carries.  Every draw is float32 from a seeded generator with the
dtype spelled out (under a float64 default dtype ``torch.rand`` without one draws another stream) and cast up.

Truth, in two forms.
  1. ``run_clip(case, "cpu", torch.float64, COMPOSED)``: the module itself under a float64 default dtype on the CPU
     (no kernel takes part there), on the float32 leaves cast up -- the rule of tests/decoder_truth.py.
  2. ``statement(case)``: a plain float64 statement of the operation that shares no code with ``ClipCriterion``: loops
     over frame, clip, layer and pair, scipy's ``linear_sum_assignment`` on float64 costs, and the primitives of
     tests/clip_truth.py (``match_cost_truth``, ``pair_box_loss_truth``, ``pair_iou_truth``, ``focal_truth``);
     gradients by autograd through the statement.  It catches bookkeeping errors both paths of the module share;
     form 1 makes a disagreement attributable.  The CPU test holds the two to each other at ``FORMS_AGREE`` and form 2
     to a fixture written by the reference's own criterion (tests/golden/criterion_clip.npz).
What form 2 states where the reference is silent or differs: a ground truth is free when no track carries its id (the
reference frees the earlier copies of an id that a frame repeats and a track carries; its dict then maps their matches
back onto the last copy); the updater's fake track (an empty active set) takes scripted fields instead of random ones.

The rule.  Per output, error = max |got - truth| against scale = max |truth|.  A path passes when its error is at most
``clip_truth.measured_bound(reference error, scale)``: 4 x the error the float32 torch composition
(MEMOTR_FUSED_CLIP_OPS=0, boolean-mask selection) makes on the same inputs on the same device, plus one float32 ulp
of the scale.  Integer decisions are compared exactly.

The margins.  A float32 decision that falls the other way in float64 puts a path 1e-3 .. 1 from truth and inflates every
bound until it hides what the test is for, so ``statement`` measures, in float64, how far each decision sits from its
edge, and a case must keep (they are conditions on the inputs; a case that misses one gets another seed, never a
smaller margin):
  * ``ASSIGN_MARGIN`` = 1e-4 between the optimum of every assignment problem and the best assignment that differs
    from it (re-solved with each matched pair forbidden in turn).  A sum of ten costs of size up to 20 carries about
    10 x 20 x 2^-24 = 1e-5 of float32 round-off.
  * ``THRESHOLD_MARGIN`` = 1e-5 between every IoU of a carried or new track and 0.5, and between every score and the
    update threshold: both are quotients of a handful of float32 operations on numbers below 1, i.e. a few 1e-7.
  * no max / min tie inside the GIoU of a loss pair, and the same signs in float32 (``clip_truth.box_decisions``).
``REF_ERROR_CAP`` = 1e-5 of scale caps the float32 composition's own error: 25 x the 4.1e-7 a float32 CPU run of the
first case was measured to make on its worst gradient.  It is a condition that keeps a flipped decision from widening
the bound, not a tolerance for the kernels; the CPU test holds the CPU composition to a quarter of it.
"""
import contextlib
import functools
from typing import NamedTuple, Tuple

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from clip_truth import (box_decisions, focal_truth, match_cost_truth, max_err, measured_bound, out_scale,
                        pair_box_loss_truth, pair_iou_truth)
from handover_cases import DIFFERENTIATED, THRESHOLD

C = 256
POOL = 24                                 # identities a clip can show; a frame shows those with (i + t + b) % 4 != 0
ASSIGN_MARGIN = 1e-4
THRESHOLD_MARGIN = 1e-5
REF_ERROR_CAP = 1e-5
FORMS_AGREE = 1e-12      # of scale: two float64 sums of a few thousand terms of like sign, formed in different orders,
#                          differ by about sqrt(terms) x 2^-53 = 1e-14 of the sum; 1e-12 leaves two decades
COST_WEIGHTS = (2.0, 5.0, 2.0)            # class, L1, GIoU of the matching cost
LOSS_WEIGHT = {"box_l1_loss": 5.0, "box_giou_loss": 2.0, "label_focal_loss": 2.0}
# different for every frame and layer, so that a weight in the wrong column or frame changes the sums
FRAME_WEIGHTS = (1.0, 0.5, 2.0, 1.5)
AUX_WEIGHTS = (0.5, 0.75, 1.25)
LOSS_KEYS = ("box_l1_loss", "box_giou_loss", "label_focal_loss")
F32 = torch.float32


class Case(NamedTuple):
    name: str
    nd: int
    K: int
    layers: int                           # decoder layers: the main one and layers - 1 auxiliary ones
    merge: int                            # merge_det_track_layer
    gts: Tuple[Tuple[int, ...], ...]      # [frame][clip] ground-truth count
    seed: int = 1
    use_dab: bool = True
    repeat: Tuple[int, int] = None        # (frame, clip) whose last ground truth repeats an id that a track carries
    miss: Tuple[Tuple[int, int], ...] = ()   # (frame, clip): no detect query sits on a ground truth (new IoUs < 0.5)
    kill: Tuple[Tuple[int, int], ...] = ()   # (frame, clip): every score below the threshold

    @property
    def T(self):
        return len(self.gts)

    @property
    def B(self):
        return len(self.gts[0])


CASES = (
    Case("probe", 20, 8, 3, 1, ((10, 3), (9, 0), (7, 4))),
    Case("repeat-lose", 20, 1, 3, 0, ((6, 2), (7, 0), (5, 3)), repeat=(1, 0), miss=((0, 1),), kill=((1, 1),)),
    Case("crowded", 8, 8, 2, 0, ((10,), (10,))),
    Case("return", 20, 1, 4, 2, ((0, 0), (6, 3), (4, 5), (7, 2))),
    Case("model-nd", 300, 1, 3, 1, ((17,), (17,))),
    Case("plain", 20, 8, 3, 1, ((10, 3), (9, 0), (7, 4)), use_dab=False),
)
CASE_IDS = [c.name for c in CASES]
GOLDEN_CASE = CASES[0]                    # tests/golden/criterion_clip.npz


class Path(NamedTuple):
    keep_rows: bool = True                # criterion.keep_threshold set: the selection by row index
    handover: bool = True                 # state["handover"]: the active set gathered by one kernel (device only)
    deferred: bool = True                 # losses of frame t issued after the tracks of frame t + 1
    stacks: bool = False                  # pred_logits_all / pred_bboxes_all (main layer last) instead of the list


DEFAULT = Path()
COMPOSED = Path(keep_rows=False, handover=False)


# ------------------------------------------------------------------------------------------------ scripted clips
def _gen(case, *key):
    seed = case.seed
    for k in key:
        seed = seed * 1009 + k + 1
    return torch.Generator().manual_seed(seed)


def _rand_boxes(g, n):
    """tests/handover_cases.py: _boxes, with the dtype on every draw."""
    return torch.cat((0.3 + 0.4 * torch.rand(n, 2, generator=g, dtype=F32),
                      0.1 + 0.2 * torch.rand(n, 2, generator=g, dtype=F32)), dim=1)


def _present(case, t, b):
    return [i for i in range(POOL) if (i + t + b) % 4 != 0][:case.gts[t][b]]


def ground_truths(case, t, b):
    """-> (ids (n,) int64, labels (n,) int64, boxes (n, 4) float32) of frame t of clip b.  Identity i sits in cell i of a
    5 x 5 grid (ground truths that do not overlap keep the assignment problems away from ties), drifts a little from
    frame to frame, and is out of sight in every fourth frame: ids leave and return."""
    g = _gen(case, 1, b)
    i = torch.arange(POOL)
    centre = 0.12 + 0.19 * torch.stack((i % 5, i // 5), 1).to(F32) + 0.03 * torch.rand(POOL, 2, generator=g, dtype=F32)
    size = 0.08 + 0.06 * torch.rand(POOL, 2, generator=g, dtype=F32)
    drift = 0.02 * (torch.rand(POOL, 2, generator=g, dtype=F32) - 0.5)
    boxes = torch.cat((centre + t * drift, size), 1)
    present = _present(case, t, b)
    ids = [100 * b + 10 + p for p in present]
    if case.repeat == (t, b):
        # an identity that sat under a detect query in the previous frame (an even place there), so a track carries it
        before = _present(case, t - 1, b)
        again = next(p for p in present[:-1] if p in before and before.index(p) % 2 == 0
                     and before.index(p) < min(len(before), case.nd // 2))
        ids[-1] = 100 * b + 10 + again
    idx = torch.as_tensor(present, dtype=torch.long)
    return torch.as_tensor(ids, dtype=torch.long), idx % case.K, boxes[idx].reshape(-1, 4)


def script(case):
    """-> per frame {"gts": per clip (ids, labels, boxes), "recipe": track ids of every clip -> the model's outputs}."""
    return [{"gts": [ground_truths(case, t, b) for b in range(case.B)],
             "recipe": functools.partial(frame_inputs, case, t)} for t in range(case.T)]


def frame_inputs(case, t, track_ids):
    """The model's outputs of frame t as float32 CPU tensors, given the ids of the tracks every clip carries into it:
    ``logits`` (layers, B, Nq, K) and ``boxes`` (layers, B, Nq, 4) with the MAIN layer at index 0, ``outputs``,
    ``queries`` (B, Nq, C), ``last_ref_pts``, ``init_ref_pts`` (B, Nq, 4), ``det_query_embed`` (nd, C or 2C),
    ``query_mask`` (B, Nq).  Nq = nd + the largest track count; the slots behind a clip's own tracks are padding and
    hold numbers like any other row."""
    nd, K, L, B = case.nd, case.K, case.layers, case.B
    n_q = nd + max(len(ids) for ids in track_ids)
    g = _gen(case, 2, t)
    logits = torch.randn(L, B, n_q, K, generator=g, dtype=F32) - (0.0 if K == 1 else 1.2)
    logits -= 0.6 * torch.arange(B, dtype=F32).reshape(1, B, 1, 1)      # fewer live detections, so fewer tracks, in clip 1
    boxes = _rand_boxes(g, L * B * n_q).reshape(L, B, n_q, 4)
    mask = torch.zeros(B, n_q, dtype=torch.bool)
    for b in range(B):
        gt_ids, _, gt_boxes = ground_truths(case, t, b)
        n_gt, n_tr = len(gt_ids), len(track_ids[b])
        mask[b, nd + n_tr:] = True
        if (t, b) not in case.miss:
            for li in range(L):
                for i in range(0, min(n_gt, nd // 2), 2):
                    boxes[li, b, 2 * i + 1] = gt_boxes[i] + 0.004 * torch.rand(4, generator=g, dtype=F32)
        for j, tid in enumerate(track_ids[b]):
            own = [k for k in range(n_gt) if int(gt_ids[k]) == tid]
            if tid >= 0 and own:              # on its ground truth (the last one with the id), or drifting off it
                for li in range(L):
                    boxes[li, b, nd + j] = gt_boxes[own[-1]] + (0.3 if j % 4 == 1 else 0.004) * torch.rand(
                        4, generator=g, dtype=F32)
            elif tid < 0:                     # dead: one class on either side of the threshold, the others far below
                logits[0, b, nd + j] = -3.0
                logits[0, b, nd + j, j % K] = (1.0 if j % 2 == 0 else -1.0) + 0.1 * torch.rand((), generator=g, dtype=F32)
        if (t, b) in case.kill:
            logits[0, b] = -logits[0, b].abs() - 0.1
    QW = C if case.use_dab else 2 * C
    return {"logits": logits, "boxes": boxes, "query_mask": mask,
            "outputs": torch.randn(B, n_q, C, generator=g, dtype=F32),
            "queries": torch.randn(B, n_q, C, generator=g, dtype=F32),
            "last_ref_pts": torch.randn(B, n_q, 4, generator=g, dtype=F32),
            "init_ref_pts": torch.randn(B, n_q, 4, generator=g, dtype=F32),
            "det_query_embed": torch.randn(nd, QW, generator=g, dtype=F32)}


FIELDS = ("logits", "boxes", "ref_pts", "output_embed", "long_memory", "last_output", "query_embed")
SOURCES = ("outputs", "queries", "last_ref_pts", "init_ref_pts", "det_query_embed")


def fake_fields(case, t, b):
    """The one row the query updater puts in place of an empty active set: scripted, where the module draws it."""
    g = _gen(case, 3, t, b)
    width = {"logits": case.K, "boxes": 4, "ref_pts": 4, "query_embed": C if case.use_dab else 2 * C}
    return {f: torch.randn(1, width.get(f, C), generator=g, dtype=F32) for f in FIELDS}


def handover_weights(case, b, field, shape):
    """Fixed weights of the sum over the last active set that joins the loss in the one backward
    (tests/handover_cases.py: backward_through)."""
    g = _gen(case, 4, b, DIFFERENTIATED.index(field))
    return torch.randn(tuple(shape), generator=g, dtype=F32)


def leaf_names(case, t):
    return [f"f{t}.{n}{li}" for li in range(case.layers) for n in ("logits", "boxes")] + [f"f{t}.{n}" for n in SOURCES]


# ------------------------------------------------------------------------------------------------ form 1: the module
@contextlib.contextmanager
def default_dtype(dtype):
    before = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


_UPDATERS = {}


def _updater(use_dab, device):
    """Only its selection of active tracks is used (no parameter takes part); it lives on ``device`` because its fake
    track does."""
    from memotr_amd.models.query_updater import QueryUpdater
    key = (use_dab, str(device))
    if key not in _UPDATERS:
        with default_dtype(torch.float32):
            u = QueryUpdater(hidden_dim=C, ffn_dim=32, tp_drop_ratio=0.0, fp_insert_ratio=0.0, dropout=0.0,
                             use_checkpoint=False, use_dab=use_dab, update_threshold=THRESHOLD, long_memory_lambda=0.01)
        _UPDATERS[key] = u.to(device).train()
    return _UPDATERS[key]


def run_clip(case, device, dtype, path=DEFAULT):
    """The criterion's part of ``engine.clip_forward_backward`` on the scripted clip: begin_frame, finish_tracks,
    (deferred) finish_losses, QueryUpdater.select_active_tracks, get_mean_by_n_gts(with_log=False), get_sum_loss_dict,
    and ONE backward of the loss plus the weighted sum over the last active set.  The next frame's track fields come
    from that frame's leaves.  -> the result dict ``decisions_of`` / ``floats_of`` read."""
    from memotr_amd.models.criterion import ClipCriterion
    from memotr_amd.models.matcher import HungarianMatcher
    from memotr_amd.structures.track_instances import TrackInstances
    device = torch.device(device)
    with default_dtype(dtype):
        crit = ClipCriterion(num_classes=case.K, matcher=HungarianMatcher(*COST_WEIGHTS), n_det_queries=case.nd,
                             aux_loss=True, weight=dict(LOSS_WEIGHT), max_frame_length=case.T, n_aux=case.layers - 1,
                             merge_det_track_layer=case.merge, aux_weights=list(AUX_WEIGHTS[:case.layers - 1]),
                             hidden_dim=C, use_dab=case.use_dab)
        crit.frame_weights = list(FRAME_WEIGHTS[:case.T])
        crit.device = device
        crit.gt_trackinstances_list = []
        for t in range(case.T):
            per_clip = []
            for b in range(case.B):
                gt = TrackInstances(hidden_dim=C, num_classes=case.K, device=device)
                ids, labels, boxes = ground_truths(case, t, b)
                gt.ids, gt.labels, gt.boxes = ids.to(device), labels.to(device), boxes.to(device, dtype)
                per_clip.append(gt)
            crit.gt_trackinstances_list.append(per_clip)
        crit.n_gts, crit.log = [], {}
        crit._acc = torch.zeros((3, 2), device=device)
        crit.keep_threshold = THRESHOLD if path.keep_rows else None
        upd = _updater(case.use_dab, device)
        upd.__dict__["_keep_rows_ok"] = path.keep_rows
        tracks = [TrackInstances(hidden_dim=C, num_classes=case.K, use_dab=case.use_dab, device=device)
                  for _ in range(case.B)]
        leaves, frames, owed = {}, [], None
        for t in range(case.T):
            track_ids = [tr.ids.tolist() if len(tr) else [] for tr in tracks]
            rec = frame_inputs(case, t, track_ids)

            def leaf(name, value):
                leaves[f"f{t}.{name}"] = value.to(device, dtype).requires_grad_(True)
                return leaves[f"f{t}.{name}"]

            lg = [leaf(f"logits{li}", rec["logits"][li]) for li in range(case.layers)]
            bx = [leaf(f"boxes{li}", rec["boxes"][li]) for li in range(case.layers)]
            src = {n: leaf(n, rec[n]) for n in SOURCES}
            aux = [{"pred_logits": lg[li], "pred_bboxes": bx[li]} for li in range(1, case.layers)]
            aux[-1]["queries"] = src["queries"]
            res = {"pred_logits": lg[0], "pred_bboxes": bx[0], "outputs": src["outputs"],
                   "last_ref_pts": src["last_ref_pts"], "init_ref_pts": src["init_ref_pts"],
                   "det_query_embed": src["det_query_embed"], "query_mask": rec["query_mask"].to(device),
                   "aux_outputs": aux}
            if path.stacks:                 # decoder order: the auxiliary layers, then the main one
                res["pred_logits_all"] = torch.stack(lg[1:] + lg[:1])
                res["pred_bboxes_all"] = torch.stack(bx[1:] + bx[:1])
            state = crit.begin_frame(res, tracks, t)
            state["handover"], state["gather"] = path.handover and device.type == "cuda", True
            if path.deferred:
                if owed is not None:
                    crit.finish_losses(owed)
                previous, new, unmatched = crit.finish_tracks(state)
                owed = state
                pairs = state["per_clip"]
            else:
                seen, issue = [], crit.finish_losses        # finish_frame in one piece; its losses half consumes the pairs
                crit.finish_losses = lambda s: (seen.append(list(s["per_clip"])), issue(s))[1]
                try:
                    previous, new, unmatched = crit.finish_frame(state)
                finally:
                    del crit.finish_losses
                pairs = seen[0]
            frame = {"pairs": [], "n_tr": [len(x) for x in track_ids], "fused": [], "fake": []}
            for b in range(case.B):
                lay, q, g = (x.tolist() for x in pairs[b]["idx"])
                frame["pairs"].append([([qq for ll, qq in zip(lay, q) if ll == li], [gg for ll, gg in zip(lay, g) if ll == li])
                                       for li in range(case.layers)])
                frame["fused"].append(isinstance(unmatched[b].__dict__.get("_keep_rows", (None,))[0], TrackInstances))
            frame["matched_idx"] = [previous[b].matched_idx.tolist() if frame["n_tr"][b] else [] for b in range(case.B)]
            frame["new_ids"] = [new[b].ids.tolist() if new[b].ids.shape[0] == len(new[b]) else None
                                for b in range(case.B)]
            tracks = upd.select_active_tracks(previous, new, unmatched)
            for b, act in enumerate(tracks):
                fake = len(act) == 1 and int(act.ids[0]) == -2
                frame["fake"].append(fake)
                if fake:
                    for f, v in fake_fields(case, t, b).items():
                        setattr(act, f, v.to(device, dtype))
                    act.iou = act.iou.to(dtype)
            frame["active_ids"] = [act.ids.tolist() for act in tracks]
            frame["active_matched"] = [act.matched_idx.tolist() for act in tracks]
            frame["iou"] = [act.iou.detach().clone() for act in tracks]
            frame["fields"] = [{f: getattr(act, f).detach().clone() for f in FIELDS} for act in tracks]
            frames.append(frame)
        if owed is not None:
            crit.finish_losses(owed)
        loss_dict, _ = crit.get_mean_by_n_gts(with_log=False)
        loss = crit.get_sum_loss_dict(loss_dict)
        extra = 0
        for b, act in enumerate(tracks):
            for f in DIFFERENTIATED:
                v = getattr(act, f)
                extra = extra + (v * handover_weights(case, b, f, v.shape).to(device, dtype)).sum()
        names = list(leaves)
        grads = torch.autograd.grad(loss + extra, [leaves[n] for n in names], allow_unused=True)
        grads = {n: (torch.zeros_like(leaves[n]) if gr is None else gr) for n, gr in zip(names, grads)}
        return {"loss": loss.detach(), "losses": {k: v.detach() for k, v in loss_dict.items()},
                "log": {k: v.detach().clone() for k, v in crit.log.items()}, "frames": frames, "grads": grads,
                "n_gts": list(crit.n_gts)}


# ------------------------------------------------------------------------------------------------ form 2: the statement
VARIANTS = {"a": "late layers matched against all ground truths instead of the free ones",
            "b": "the first ground truth with a repeated id owns it",
            "c": "the sums divided per frame instead of by the clip's total",
            "d": "auxiliary weight applied to the main column",
            "e": "track pairs counted on early layers",
            "f": "a padded slot included in the focal sum",
            "g": "track IoU not refreshed where the track owns a ground truth"}


def _solve(cost):
    """-> (rows, cols, gap): the optimum and how much the best assignment that differs from it costs more (each matched
    pair forbidden in turn; inf where there is no other assignment)."""
    if cost.size == 0:
        return [], [], float("inf")
    r, c = linear_sum_assignment(cost)
    best, gap = cost[r, c].sum(), float("inf")
    for i, j in zip(r, c):
        other = cost.copy()
        other[i, j] = 1e6
        r2, c2 = linear_sum_assignment(other)
        if other[r2, c2].sum() < 1e5:
            gap = min(gap, other[r2, c2].sum() - best)
    return r.tolist(), c.tolist(), gap


def statement(case, variant=None):
    """Form 2 (see the module docstring); ``variant``: one of the wrong criteria of ``VARIANTS``.  -> a result dict like
    ``run_clip``'s, plus "margins" and "rows" (how often each kind of row occurred)."""
    nd, K, L, B, T = case.nd, case.K, case.layers, case.B, case.T
    f64 = torch.float64
    margins = {"assign": float("inf"), "iou": float("inf"), "score": float("inf"), "giou_ties": 0, "giou_signs": 0}
    # (an identity whose ground truth is gone always stays: it kept its id because its last IoU was at least 0.5)
    rows = {k: 0 for k in ("stays", "drifts_off", "gone_kept", "gone_dropped", "dead_kept", "dead_dropped", "padded",
                           "repeated_owned", "no_gt", "fake", "returns", "late_restricted", "early_with_tracks")}
    # a track: its identity, previous iou and the four fields that travel from frame to frame
    tracks = [[] for _ in range(B)]
    leaves, frames, log = {}, [], {}
    acc = {k: 0.0 for k in LOSS_KEYS + tuple("aux_" + k for k in LOSS_KEYS)}
    n_gts = []

    def note(kind, value):
        margins[kind] = min(margins[kind], float(value))

    def box_loss(pred, tgt):
        d64, d32 = box_decisions(pred.detach(), tgt), box_decisions(pred.detach().float(), tgt.float())
        margins["giou_ties"] += int((d64 == 0).sum())
        margins["giou_signs"] += int((d64 != d32.double()).sum())
        l1, gl = pair_box_loss_truth(pred, tgt)
        return l1.sum(), gl.sum()

    for t in range(T):
        rec = frame_inputs(case, t, [[tr["id"] for tr in tracks[b]] for b in range(B)])
        lg = [rec["logits"][li].to(f64).requires_grad_(True) for li in range(L)]
        bx = [rec["boxes"][li].to(f64).requires_grad_(True) for li in range(L)]
        src = {n: rec[n].to(f64).requires_grad_(True) for n in SOURCES}
        for li in range(L):
            leaves[f"f{t}.logits{li}"], leaves[f"f{t}.boxes{li}"] = lg[li], bx[li]
        for n in SOURCES:
            leaves[f"f{t}.{n}"] = src[n]
        n_q_all = lg[0].shape[1]
        per_layer = {k: [0.0] * L for k in LOSS_KEYS}
        frame = {"pairs": [], "n_tr": [len(tr) for tr in tracks], "matched_idx": [], "new_ids": [], "active_ids": [],
                 "active_matched": [], "iou": [], "fields": [], "fake": []}
        n_gts.append(sum(case.gts[t]))
        for b in range(B):
            gt_ids, gt_labels, gt_boxes = ground_truths(case, t, b)
            gt_boxes = gt_boxes.to(f64)
            n_gt, n_tr = len(gt_ids), len(tracks[b])
            id_list = gt_ids.tolist()
            rows["padded"] += n_q_all - nd - n_tr
            rows["no_gt"] += n_gt == 0
            # ---- who owns which ground truth
            owner = []
            for tr in tracks[b]:
                own = [k for k in range(n_gt) if id_list[k] == tr["id"]]
                owner.append(-1 if not own else (own[0] if variant == "b" else own[-1]))
                rows["repeated_owned"] += len(own) > 1
            carried = {tr["id"] for tr in tracks[b]}
            free = [k for k in range(n_gt) if id_list[k] not in carried]
            # ---- one assignment problem per layer
            pairs = []
            for li in range(L):
                early = li > 0 and li - 1 < case.merge
                cols = list(range(n_gt)) if (early or variant == "a") else free
                if n_gt:
                    cost = match_cost_truth(lg[li].detach()[None, b, :nd], bx[li].detach()[None, b, :nd], gt_labels,
                                            gt_boxes, *COST_WEIGHTS)[0].numpy()
                    q, c, gap = _solve(cost[:, cols])
                else:
                    q, c, gap = [], [], float("inf")
                note("assign", gap)
                rows["late_restricted"] += (not early) and len(free) < n_gt
                rows["early_with_tracks"] += early and any(o >= 0 for o in owner)
                pairs.append((q, [cols[j] for j in c]))
                # ---- losses of the layer: matched detect queries, and (late layers) the tracks that own a ground truth
                pq, pg = list(q), [cols[j] for j in c]
                if not early or variant == "e":
                    pq += [nd + j for j in range(n_tr) if owner[j] >= 0]
                    pg += [owner[j] for j in range(n_tr) if owner[j] >= 0]
                n_rows = n_q_all if variant == "f" else nd + n_tr
                labels = torch.full((n_rows,), K, dtype=torch.long)
                labels[pq] = gt_labels[pg]
                per_layer["label_focal_loss"][li] = per_layer["label_focal_loss"][li] + focal_truth(
                    lg[li][None, b, :n_rows], labels[None], 0.25, 2.0)[0]
                if pq:
                    l1, gl = box_loss(bx[li][b, pq], gt_boxes[pg])
                    per_layer["box_l1_loss"][li] = per_layer["box_l1_loss"][li] + l1
                    per_layer["box_giou_loss"][li] = per_layer["box_giou_loss"][li] + gl
            frame["pairs"].append(pairs)
            frame["matched_idx"].append(owner)
            # ---- the next frame's candidates: carried tracks, new tracks, unclaimed detections; who stays active
            score = torch.sigmoid(lg[0].detach()[b, :nd + n_tr]).max(1).values
            note("score", (score - THRESHOLD).abs().min())
            above = (score > THRESHOLD).tolist()
            mq, mg = pairs[0]
            cand = []
            for j, tr in enumerate(tracks[b]):
                iou = tr["iou"]
                if owner[j] >= 0 and variant != "g":
                    iou = pair_iou_truth(bx[0].detach()[b, nd + j], gt_boxes[owner[j]])
                    note("iou", (iou - 0.5).abs())
                if tr["id"] >= 0 or above[nd + j]:
                    cand.append({"id": tr["id"], "iou": iou, "matched": owner[j], "row": nd + j,
                                 "ref_pts": tr["ref_pts"], "long_memory": tr["long_memory"],
                                 "last_output": tr["last_output"], "query_embed": tr["query_embed"]})
                    if tr["id"] >= 0:
                        rows["returns"] += owner[j] >= 0 and tr["matched"] == -1
                        kind = ("stays" if iou >= 0.5 else "drifts_off") if owner[j] >= 0 else \
                            ("gone_kept" if iou >= 0.5 else "gone_dropped")
                        rows[kind] += 1
                    else:
                        rows["dead_kept"] += 1
                else:
                    rows["dead_dropped"] += 1

            def detect(q):
                query = src["queries"][b, q]
                return {"row": q, "long_memory": query, "last_output": src["outputs"][b, q],
                        "query_embed": query if case.use_dab else torch.cat((src["det_query_embed"][q, :C], query))}

            new_ids = []
            for q, k in zip(mq, mg):
                iou = pair_iou_truth(bx[0].detach()[b, q], gt_boxes[k])
                note("iou", (iou - 0.5).abs())
                new_ids.append(id_list[k])
                cand.append(dict(detect(q), id=id_list[k], iou=iou, matched=k, ref_pts=src["last_ref_pts"][b, q]))
            for q in range(nd):
                if q not in mq and above[q]:
                    cand.append(dict(detect(q), id=-1, iou=torch.zeros((), dtype=f64), matched=-1,
                                     ref_pts=src["init_ref_pts"][b, q]))
            frame["new_ids"].append(new_ids)
            for c in cand:
                c["fields"] = {"logits": lg[0].detach()[b, c["row"]], "boxes": bx[0].detach()[b, c["row"]],
                               "output_embed": src["outputs"][b, c["row"]], "ref_pts": c["ref_pts"],
                               "long_memory": c["long_memory"], "last_output": c["last_output"],
                               "query_embed": c["query_embed"]}
                if c["iou"] < 0.5:
                    c["id"] = -1
            frame["fake"].append(not cand)
            if not cand:
                rows["fake"] += 1
                ff = {f: v[0].to(f64) for f, v in fake_fields(case, t, b).items()}
                cand = [dict(ff, id=-2, iou=torch.zeros((), dtype=f64), matched=-2, fields=ff)]
            tracks[b] = cand
            frame["active_ids"].append([c["id"] for c in cand])
            frame["active_matched"].append([c["matched"] for c in cand])
            frame["iou"].append(torch.stack([c["iou"] for c in cand]))
            frame["fields"].append({f: torch.stack([c["fields"][f] for c in cand]).detach() for f in FIELDS})
        frames.append(frame)
        # ---- the frame's sums into the clip's: main layer x frame weight, auxiliary layers x their weights as well
        fw = FRAME_WEIGHTS[t]
        div = max(float(n_gts[t]), 1.0) if variant == "c" else 1.0
        for k in LOSS_KEYS:
            log[f"frame{t}_{k}"] = torch.as_tensor(per_layer[k][0], dtype=f64).detach()
            acc[k] = acc[k] + (AUX_WEIGHTS[0] if variant == "d" else 1.0) * fw * per_layer[k][0] / div
            for li in range(1, L):
                acc["aux_" + k] = acc["aux_" + k] + AUX_WEIGHTS[li - 1] * fw * per_layer[k][li] / div
    total = 1.0 if variant == "c" else max(float(sum(n_gts)), 1.0)
    losses = {k: torch.as_tensor(v, dtype=f64) / total for k, v in acc.items()}
    loss = sum(LOSS_WEIGHT[k.replace("aux_", "")] * v for k, v in losses.items())
    extra = 0
    for b in range(B):
        for f in DIFFERENTIATED:
            v = torch.stack([c["fields"][f] for c in tracks[b]])
            extra = extra + (v * handover_weights(case, b, f, v.shape).to(f64)).sum()
    names = list(leaves)
    grads = torch.autograd.grad(loss + extra, [leaves[n] for n in names], allow_unused=True)
    grads = {n: (torch.zeros_like(leaves[n]) if gr is None else gr) for n, gr in zip(names, grads)}
    return {"loss": loss.detach(), "losses": {k: v.detach() for k, v in losses.items()}, "log": log, "frames": frames,
            "grads": grads, "n_gts": n_gts, "margins": margins, "rows": rows}


@functools.lru_cache(maxsize=None)
def truth(case):
    """Form 2 of ``case``, computed once and shared; nobody modifies it."""
    return statement(case)


@functools.lru_cache(maxsize=None)
def module_truth(case):
    """Form 1 of ``case``."""
    return run_clip(case, "cpu", torch.float64, COMPOSED)


def decisions(case):
    """How far every decision of ``case`` sits from its edge, in float64 (see the module docstring)."""
    return truth(case)["margins"]


def margins_hold(m):
    return (m["assign"] >= ASSIGN_MARGIN and m["iou"] >= THRESHOLD_MARGIN and m["score"] >= THRESHOLD_MARGIN
            and m["giou_ties"] == 0 and m["giou_signs"] == 0)


# ------------------------------------------------------------------------------------------------ comparisons
def decisions_of(result):
    """Every integer decision of a run, as nested lists: per frame the matched (query, ground truth) pairs of every
    clip and layer, the ground truth every carried track owns, and ids and ground truths of the active set."""
    return [{"pairs": [[(list(q), list(g)) for q, g in clip] for clip in f["pairs"]], "n_tr": list(f["n_tr"]),
             "matched_idx": [list(x) for x in f["matched_idx"]], "active_ids": [list(x) for x in f["active_ids"]],
             "active_matched": [list(x) for x in f["active_matched"]], "fake": [bool(x) for x in f["fake"]]}
            for f in result["frames"]]


def new_ids_agree(result, other):
    """ids of the new tracks, where a path materialises them (the fused hand-over only counts its new tracks)."""
    return all(a is None or b is None or list(a) == list(b)
               for fa, fb in zip(result["frames"], other["frames"]) for a, b in zip(fa["new_ids"], fb["new_ids"]))


def floats_of(result):
    """what -> tensor: the loss, the six entries, the three log values per frame, the iou of every active set and the
    gradient of every leaf."""
    out = {"loss": result["loss"]}
    out.update({f"loss.{k}": v for k, v in result["losses"].items()})
    out.update({f"log.{k}": v for k, v in result["log"].items()})
    for t, f in enumerate(result["frames"]):
        out[f"f{t}.iou"] = torch.cat([x.reshape(-1) for x in f["iou"]])
    out.update({f"grad.{k}": v for k, v in result["grads"].items()})
    return out


def errors(got, want):
    """what -> (max |got - want|, max |want|)"""
    a, b = floats_of(got), floats_of(want)
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    return {k: (max_err(a[k], b[k]) if a[k].shape == b[k].shape else float("inf"), out_scale(b[k])) for k in a}


def check(case, got, ref_errors, want, failures, label="kernel"):
    """One TRUTH line per output of ``got``; appends what lies outside ``measured_bound`` to ``failures``."""
    worst = {}
    for what, (err, scale) in errors(got, want).items():
        ref = ref_errors[what][0]
        bound = measured_bound(ref, scale)
        print(f"TRUTH {case.name} {what} ref={ref:.3e} {label}={err:.3e} bound={bound:.3e} scale={scale:.3e}")
        worst[what] = err / bound if bound else (0.0 if err == 0 else float("inf"))
        if not err <= bound:
            failures.append(f"{case.name} {what}: {label} {err:.3e} > bound {bound:.3e} (ref {ref:.3e}, scale {scale:.3e})")
    return worst


def same_bits(got, want):
    """-> the outputs of ``got`` that are not bit copies of ``want``'s (decisions, active-set fields, floats)."""
    bad = []
    if decisions_of(got) != decisions_of(want):
        bad.append("decisions")
    a, b = floats_of(got), floats_of(want)
    bad += [k for k in a if not torch.equal(a[k], b[k])]
    for t, (fa, fb) in enumerate(zip(got["frames"], want["frames"])):
        for clip, (xa, xb) in enumerate(zip(fa["fields"], fb["fields"])):
            bad += [f"f{t}.clip{clip}.{f}" for f in FIELDS if not torch.equal(xa[f], xb[f])]
    return bad


def fields_are_copies(got, want):
    """-> the float fields of the active sets of ``got`` that are not bit copies of the leaf rows truth takes them from
    (``want``'s fields are float64 casts of float32 leaves, so the comparison in float64 is exact)."""
    bad = []
    for t, (fa, fb) in enumerate(zip(got["frames"], want["frames"])):
        for clip, (xa, xb) in enumerate(zip(fa["fields"], fb["fields"])):
            for f in FIELDS:
                a, b = xa[f].detach().cpu().double(), xb[f]
                if a.shape != b.shape or not torch.equal(a, b):
                    bad.append(f"f{t}.clip{clip}.{f}")
    return bad


def to_numpy(result):
    return {k: v.detach().cpu().numpy() for k, v in floats_of(result).items()}


def flat_pairs(result):
    """name -> int64 array: the matched pairs of every frame, clip and layer (for the fixture)."""
    out = {}
    for t, f in enumerate(result["frames"]):
        for b, clip in enumerate(f["pairs"]):
            for li, (q, g) in enumerate(clip):
                out[f"pairs.f{t}.clip{b}.layer{li}"] = np.asarray([q, g], dtype=np.int64).reshape(2, -1)
    return out
