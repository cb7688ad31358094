"""Golden vectors for the BDD100K tracking evaluation (memotr_amd/evaluation_bdd100k.py,
memotr_amd/csrc/track_eval_bdd.hip), produced by TrackEval's own code from a checkout of the reference (the tests that
read the fixture need neither):

    python tests/golden/gen_golden_track_eval_bdd.py --reference /path/to/reference  ->  tests/golden/trackeval_bdd100k.npz

``trackeval`` is imported from ``<reference>/TrackEval`` as it is.  No files are read: a ``BDD100K`` dataset is made
without its constructor (only ``class_name_to_class_id`` set), ``raw_data`` dictionaries are built directly from the
sequences below (similarities by the dataset's own ``_calculate_similarities``), and ``get_preprocessed_seq_data`` per
class, the ``eval_sequence`` of HOTA, CLEAR, Identity and Count, their ``combine_sequences``,
``combine_classes_class_averaged`` / ``combine_classes_det_averaged`` in the order of ``eval.py`` and
``utils.write_summary_results`` produce what is stored: only arrays --

    the packed inputs (PackedBDD's arrays, ``names``),
    ``raw_similarity`` / ``pre::similarity``: per (sequence, class) p = s * 8 + c, frame by frame, concatenated,
    the preprocessed ``pre::gt_off / tr_off / gt_ids / tr_ids / n_gt_ids / n_tr_ids / n_gt_dets / n_tr_dets``,
    ``res::<field>`` with one row per entry of ``res_rows``: "<seq>/<class>" for every p, then "COMBINED_SEQ/<class>",
    then "COMBINED_SEQ/<key>" for cls_comb_cls_av, cls_comb_det_av, HUMAN, VEHICLE, BIKE,
    ``summary_keys``, ``summary_names``, ``summary_values``: the two lines of <key>_summary.txt for four keys.

Robustness check, as in gen_golden_track_eval.py: the reference alone evaluates every (sequence, class) a second time
with the frames REVERSED; HOTA_TP, HOTA_FN and HOTA_FP must be identical at all 19 thresholds, else the run stops
without writing anything and the sequence gets another seed.

The sequences, each named for the edge it is there for: ``edges`` (hand-made: intersection over area exactly 0.5 and
1, a matched detection inside a region, IoU exactly 0.5, a detection without area, frames without regions / ground
truth / detections, exact duplicates, a trailer and a Crowd row as regions, an id labelled car then truck, classes on
one side only), ``wide_65x7`` and ``tall_70x9`` (more rows of one class than a wavefront has lanes), ``regions_70``
(70 regions, only the last covers the unmatched detection), two random walks over all 8 classes, ``one_frame``,
``no_tracker``, ``no_gt``.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from conftest import save_npz  # noqa: E402
from memotr_amd import evaluation as E  # noqa: E402
from memotr_amd import evaluation_bdd100k as B  # noqa: E402

SUMMARY_KEYS = ("cls_comb_cls_av", "cls_comb_det_av", "car", "HUMAN")


def from_rows(frames):
    """Per-frame lists from hand-made frames ``(ground-truth rows, tracker rows)``, a ground-truth row being
    ``(id, box, category[, crowd])`` and a tracker row ``(id, box, category)``, through the evaluator: rows of a
    distractor category or with crowd set become the frame's ignore regions."""
    ev = B.BDD100KEvaluator()
    for t, (gt, tr) in enumerate(frames):
        ev.add_ground_truth("x", t, [r[0] for r in gt], [r[1] for r in gt], [r[2] for r in gt],
                            [len(r) > 3 and r[3] for r in gt])
        ev.add_tracker_rows("x", t, [r[0] for r in tr], [r[1] for r in tr], [r[2] for r in tr])
    ev.set_length("x", len(frames))
    return ev.sequences()["x"]


def edge_sequence():
    big, half, far = [0.0, 0, 10, 10], [0.0, 0, 10, 5], [100.0, 100, 120, 140]
    at = lambda x: [x, 0.0, x + 10, 10]                                                   # noqa: E731
    return from_rows([
        # IoU exactly 0.5 is a match (pedestrian); a car inside a Crowd row: unmatched, removed (IoA 1)
        ([(1, big, "pedestrian"), (2, far, "pedestrian"), (90, at(200), "car", True)],
         [(7, half, "pedestrian"), (8, far, "pedestrian"), (30, at(200), "car")]),
        # IoA exactly 0.5 against a trailer: kept; the same box under a region that covers a little more: removed
        ([(1, big, "pedestrian"), (91, half, "trailer"), (92, [300.0, 0, 310, 5.5], "other vehicle")],
         [(7, big, "pedestrian"), (31, big, "car"), (32, at(300), "car")]),
        # a MATCHED detection wholly inside a region: kept; a detection without area inside a region: kept
        ([(3, at(400), "car"), (93, [390.0, -10, 420, 20], "other person"), (94, [500.0, 0, 520, 20], "car", True)],
         [(33, at(400), "car"), (34, [505.0, 5, 505, 15], "car")]),
        ([(1, big, "pedestrian"), (2, far, "pedestrian")], []),                            # no detections, no regions
        ([], [(7, half, "pedestrian"), (8, far, "pedestrian")]),                           # no ground truth
        ([(95, [0.0, 0, 10, 6], "trailer")], [(7, half, "pedestrian"), (8, far, "rider")]),   # regions only: 7 goes
        ([(1, big, "pedestrian"), (2, big, "pedestrian")], [(7, big, "pedestrian"), (8, big, "pedestrian")]),  # ties
        # tracker id 40 is a car here and a truck in the next frame; the ground truth keeps it a car
        ([(3, at(400), "car"), (4, at(600), "truck")], [(40, at(400), "car"), (41, at(600), "truck")]),
        ([(3, at(400), "car"), (4, at(600), "truck")], [(40, at(400), "truck"), (41, at(600), "truck")]),
        # bus: ground truth only; motorcycle: tracker only; train and bicycle: nowhere
        ([(5, at(700), "bus"), (1, big, "pedestrian")], [(50, at(800), "motorcycle"), (9, big, "pedestrian")]),
    ])


def regions_sequence():
    """A frame with 70 ignore regions of which only the last covers the unmatched detection; the next frame has them
    in the opposite order."""
    box = [1000.0, 1000, 1040, 1060]
    elsewhere = [(100 + i, [20.0 * i, 0, 20.0 * i + 15, 15], "other person") for i in range(69)]
    cover = (99, [995.0, 990, 1050, 1070], "trailer")
    gt = [(1, [0.0, 500, 50, 600], "rider")]
    tr = [(7, [2.0, 500, 50, 600], "rider"), (8, box, "rider"), (9, [3.0, 2, 14, 13], "bicycle")]
    return from_rows([(gt + elsewhere + [cover], tr), (gt + [cover] + elsewhere, tr), (gt + elsewhere, tr)])


def blank(seq, frames, side):
    keys = ("gt_ids", "gt_boxes", "gt_classes") if side == "gt" else ("tracker_ids", "tracker_boxes", "tracker_classes")
    for t in frames:
        for k in keys:
            seq[k][t] = seq[k][t][:0]
    return seq


def sequences():
    S = B.synthetic_bdd_sequence
    return {
        "edges": edge_sequence(),
        "wide_65x7": S(4, 4, 7, n_classes=1, n_false=58, miss=0.0, gap=0.0),                # 65 detections, 7 ground truths
        "tall_70x9": S(5, 4, 70, n_classes=1, n_false=0, miss=0.0, gap=0.0, track=list(range(9))),
        "regions_70": regions_sequence(),
        "walk37": blank(blank(S(2, 37, 19, n_false=3, gap=0.08, n_regions=3), [5], "gt"), [11, 12], "tracker"),
        "walk41": S(3, 41, 26, n_false=4, switch=0.05, gap=0.05, n_regions=4),
        "one_frame": S(1, 1, 9, n_false=2),
        "no_tracker": blank(S(7, 6, 10), range(6), "tracker"),
        "no_gt": blank(S(8, 6, 10, n_false=3), range(6), "gt"),
    }


def reference_eval(trackeval, seqs):
    ds = trackeval.datasets.BDD100K.__new__(trackeval.datasets.BDD100K)
    ds.class_name_to_class_id = dict(B.CLASS_NAME_TO_CLASS_ID)
    metrics = [trackeval.metrics.HOTA(), trackeval.metrics.CLEAR({"PRINT_CONFIG": False}),
               trackeval.metrics.Identity({"PRINT_CONFIG": False}), trackeval.metrics.Count()]

    def run(name, seq, order, cls):
        raw = {"num_timesteps": len(order), "seq": name,
               "gt_ids": [seq["gt_ids"][t].astype(int) for t in order],
               "gt_dets": [seq["gt_boxes"][t].astype(np.float64).reshape(-1, 4) for t in order],
               "gt_classes": [seq["gt_classes"][t].astype(int) for t in order],
               "gt_crowd_ignore_regions": [seq["ignore_regions"][t].astype(np.float64).reshape(-1, 4) for t in order],
               "tracker_ids": [seq["tracker_ids"][t].astype(int) for t in order],
               "tracker_dets": [seq["tracker_boxes"][t].astype(np.float64).reshape(-1, 4) for t in order],
               "tracker_classes": [seq["tracker_classes"][t].astype(int) for t in order]}
        raw["similarity_scores"] = [ds._calculate_similarities(g, k) for g, k in zip(raw["gt_dets"], raw["tracker_dets"])]
        data = ds.get_preprocessed_seq_data(raw, cls)
        cls_id = ds.class_name_to_class_id[cls]
        raw_sim = [s[g == cls_id][:, k == cls_id] for s, g, k in
                   zip(raw["similarity_scores"], raw["gt_classes"], raw["tracker_classes"])]
        return raw_sim, data, {m.get_name(): m.eval_sequence(data) for m in metrics}

    raws, datas, results = {}, {}, {}
    for name, seq in seqs.items():
        T = len(seq["gt_ids"])
        results[name] = {}
        for cls in B.CLASSES:
            raw_sim, data, res = run(name, seq, list(range(T)), cls)
            _, _, rev = run(name, seq, list(range(T))[::-1], cls)
            if any(not np.array_equal(res["HOTA"][k], rev["HOTA"][k]) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP")):
                raise SystemExit(f"{name}, {cls}: HOTA's integer fields change with the frame order; it cannot be a "
                                 "fixture (give it another seed), nothing written")
            raws[name, cls], datas[name, cls], results[name][cls] = raw_sim, data, res
    # eval.py: sequences per class, then the classes, then the super-categories
    comb = {cls: {m.get_name(): m.combine_sequences({n: results[n][cls][m.get_name()] for n in seqs}) for m in metrics}
            for cls in B.CLASSES}
    per_class = dict(comb)
    comb["cls_comb_cls_av"] = {m.get_name(): m.combine_classes_class_averaged(
        {c: per_class[c][m.get_name()] for c in B.CLASSES}) for m in metrics}
    comb["cls_comb_det_av"] = {m.get_name(): m.combine_classes_det_averaged(
        {c: per_class[c][m.get_name()] for c in B.CLASSES}) for m in metrics}
    for cat, members in B.SUPER_CATEGORIES.items():
        comb[cat] = {m.get_name(): m.combine_classes_det_averaged(
            {c: per_class[c][m.get_name()] for c in B.CLASSES if c in members}) for m in metrics}
    lines = {}
    with tempfile.TemporaryDirectory() as tmp:
        for key in SUMMARY_KEYS:
            table = [m.summary_results({"COMBINED_SEQ": comb[key][m.get_name()]}) for m in metrics]
            trackeval.utils.write_summary_results(table, key, tmp)
            with open(os.path.join(tmp, key + "_summary.txt")) as f:
                lines[key] = f.readline().split(), f.readline().split()
    return raws, datas, results, comb, metrics, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "TrackEval"))
    import trackeval
    seqs = sequences()
    raws, datas, results, comb, metrics, lines = reference_eval(trackeval, seqs)
    p = B.pack_bdd(seqs)
    arrays = {k: getattr(p, k) for k in p.ARRAYS}
    arrays["names"] = np.array(p.names)
    problems = [(n, c) for n in p.names for c in B.CLASSES]
    arrays["raw_similarity"] = np.concatenate([s.reshape(-1) for key in problems for s in raws[key]])
    cat = lambda field, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for key in problems                 # noqa
                                            for x in datas[key][field]] + [np.zeros(0, dt)])
    count = lambda field: np.concatenate(([0], np.cumsum([len(x) for key in problems                          # noqa
                                                          for x in datas[key][field]]))).astype(np.int32)
    arrays.update({"pre::gt_off": count("gt_ids"), "pre::tr_off": count("tracker_ids"),
                   "pre::gt_ids": cat("gt_ids", np.int32), "pre::tr_ids": cat("tracker_ids", np.int32),
                   "pre::similarity": cat("similarity_scores", np.float64)})
    for key, field in (("n_gt_ids", "num_gt_ids"), ("n_tr_ids", "num_tracker_ids"), ("n_gt_dets", "num_gt_dets"),
                       ("n_tr_dets", "num_tracker_dets")):
        arrays["pre::" + key] = np.array([datas[k][field] for k in problems], np.int64)
    combined_rows = list(B.CLASSES) + list(B.COMBINED_KEYS)
    arrays["res_rows"] = np.array([f"{n}/{c}" for n, c in problems] + ["COMBINED_SEQ/" + k for k in combined_rows])
    for m in metrics:
        for field in comb["car"][m.get_name()]:
            rows = [results[n][c][m.get_name()][field] for n, c in problems] + \
                   [comb[k][m.get_name()][field] for k in combined_rows]
            arrays["res::" + field] = np.array(rows, np.int64 if field in E.INT_FIELDS else np.float64)
    arrays["summary_keys"] = np.array(SUMMARY_KEYS)
    arrays["summary_names"] = np.array([lines[k][0] for k in SUMMARY_KEYS])
    arrays["summary_values"] = np.array([lines[k][1] for k in SUMMARY_KEYS])
    path = os.path.join(OUT, "trackeval_bdd100k.npz")
    save_npz(path, **arrays)
    print(path, f"{os.path.getsize(path)} bytes, sequences:", ", ".join(p.names))


if __name__ == "__main__":
    main()
