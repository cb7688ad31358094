"""Golden clip for the criterion's truth tests, produced by importing the REFERENCE (build container only):

    python tests/golden/gen_golden_criterion.py        ->  tests/golden/criterion_clip.npz

The first scripted clip of tests/criterion_truth.py (3 frames, 2 clips, 20 detect queries, 8 classes, 3 decoder layers,
merge_det_track_layer 1; ground truths (10, 3), (9, 0), (7, 4)) through the reference's own
``models/criterion.py`` ClipCriterion (``process_single_frame`` :138-370, ``get_mean_by_n_gts`` :118-136,
``get_sum_loss_dict`` :104-116) and the selection of ``models/query_updater.py`` (:168-242), in float32 (the reference
writes its float32 ``iou`` field by index, so it does not run under a float64 default dtype).  Written: the inputs the
losses depend on (logits and boxes of every layer, ground truths, the ids of the tracks carried into every frame), the
matched pairs of every frame, clip and layer (what the reference's matcher returned, its column indices mapped back to
ground truths by id), the six normalised losses and the gradients of the logits and box leaves.  Only data is
written; no reference source is copied.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_model import install_stubs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz, criterion_truth (the script)
from conftest import save_npz  # noqa: E402


def main():
    install_stubs()
    torch.set_grad_enabled(True)
    import criterion_truth as ct
    from models.criterion import ClipCriterion
    from models.matcher import HungarianMatcher
    from models.query_updater import QueryUpdater
    from structures.track_instances import TrackInstances

    case = ct.GOLDEN_CASE
    out = {}
    matcher = HungarianMatcher(*ct.COST_WEIGHTS)
    crit = ClipCriterion(num_classes=case.K, matcher=matcher, n_det_queries=case.nd, aux_loss=True,
                         weight=dict(ct.LOSS_WEIGHT), max_frame_length=case.T, n_aux=case.layers - 1,
                         merge_det_track_layer=case.merge, aux_weights=list(ct.AUX_WEIGHTS[:case.layers - 1]),
                         hidden_dim=ct.C, use_dab=case.use_dab)
    crit.frame_weights = list(ct.FRAME_WEIGHTS[:case.T])
    crit.device = torch.device("cpu")
    crit.gt_trackinstances_list = []
    for t in range(case.T):
        per_clip = []
        for b in range(case.B):
            gt = TrackInstances(hidden_dim=ct.C, num_classes=case.K)
            ids, labels, boxes = ct.ground_truths(case, t, b)
            gt.ids, gt.labels, gt.boxes = ids, labels, boxes
            out[f"in.f{t}.clip{b}.gt_ids"], out[f"in.f{t}.clip{b}.gt_labels"] = ids.numpy(), labels.numpy()
            out[f"in.f{t}.clip{b}.gt_boxes"] = boxes.numpy()
            per_clip.append(gt)
        crit.gt_trackinstances_list.append(per_clip)
    crit.n_gts, crit.log = [], {}
    crit.loss = {k: torch.zeros(()) for k in ct.LOSS_KEYS + tuple("aux_" + k for k in ct.LOSS_KEYS)}
    updater = QueryUpdater(hidden_dim=ct.C, ffn_dim=32, tp_drop_ratio=0.0, fp_insert_ratio=0.0, dropout=0.0,
                           use_checkpoint=False, use_dab=case.use_dab, update_threshold=ct.THRESHOLD,
                           long_memory_lambda=0.01).train()

    calls = []

    def spy(outputs, targets, use_focal=True):
        res = matcher(outputs=outputs, targets=targets, use_focal=use_focal)
        calls.append([(i.tolist(), targets[b].ids[j].tolist()) for b, (i, j) in enumerate(res)])
        return res

    crit.matcher = spy
    tracks = [TrackInstances(hidden_dim=ct.C, num_classes=case.K, use_dab=case.use_dab) for _ in range(case.B)]
    leaves = {}
    for t in range(case.T):
        track_ids = [tr.ids.tolist() if len(tr) else [] for tr in tracks]
        rec = ct.frame_inputs(case, t, track_ids)
        out[f"in.f{t}.logits"], out[f"in.f{t}.boxes"] = rec["logits"].numpy(), rec["boxes"].numpy()
        for b in range(case.B):
            out[f"track_ids.f{t}.clip{b}"] = np.asarray(track_ids[b], dtype=np.int64)

        def leaf(name, value):
            leaves[f"f{t}.{name}"] = value.clone().requires_grad_(True)
            return leaves[f"f{t}.{name}"]

        lg = [leaf(f"logits{li}", rec["logits"][li]) for li in range(case.layers)]
        bx = [leaf(f"boxes{li}", rec["boxes"][li]) for li in range(case.layers)]
        src = {n: rec[n] for n in ct.SOURCES}
        aux = [{"pred_logits": lg[li], "pred_bboxes": bx[li], "query_mask": rec["query_mask"]}
               for li in range(1, case.layers)]
        aux[-1]["queries"] = src["queries"]
        res = {"pred_logits": lg[0], "pred_bboxes": bx[0], "outputs": src["outputs"], "last_ref_pts": src["last_ref_pts"],
               "init_ref_pts": src["init_ref_pts"], "det_query_embed": src["det_query_embed"],
               "query_mask": rec["query_mask"], "aux_outputs": aux}
        calls.clear()
        previous, new, unmatched = crit.process_single_frame(model_outputs=res, tracked_instances=tracks, frame_idx=t)
        assert len(calls) == case.layers           # the main layer, then the auxiliary ones in order
        for li, call in enumerate(calls):
            for b, (q, ids) in enumerate(call):
                gt_ids = crit.gt_trackinstances_list[t][b].ids.tolist()
                out[f"pairs.f{t}.clip{b}.layer{li}"] = np.asarray([q, [gt_ids.index(i) for i in ids]],
                                                                  dtype=np.int64).reshape(2, -1)
        tracks = updater.select_active_tracks(previous, new, unmatched)
    loss_dict, _ = crit.get_mean_by_n_gts()
    loss = crit.get_sum_loss_dict(loss_dict)
    loss.backward()
    out["loss"] = loss.detach().numpy()
    out.update({f"loss.{k}": v.detach().numpy() for k, v in loss_dict.items()})
    out.update({f"grad.{k}": v.grad.numpy() for k, v in leaves.items()})
    save_npz(os.path.join(OUT, "criterion_clip.npz"), **out)
    print("criterion_clip:", float(loss), {k: float(v) for k, v in loss_dict.items()})


if __name__ == "__main__":
    main()
