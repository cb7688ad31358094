"""Golden vectors for the tracking evaluation (memotr_amd/evaluation.py, memotr_amd/csrc/track_eval.hip), produced by
TrackEval's own code from a checkout of the reference (the tests that read the fixtures need neither):

    python tests/golden/gen_golden_track_eval.py --reference /path/to/reference   ->  tests/golden/trackeval_*.npz

``trackeval`` is imported from ``<reference>/TrackEval`` as it is.  No files are read: a ``MotChallenge2DBox`` is made
without its constructor (``benchmark``, ``do_preproc``, ``class_name_to_class_id`` and ``valid_class_numbers`` set by
hand), ``raw_data`` dictionaries are built directly from the sequences below (similarities by the dataset's own
``_calculate_similarities``), and ``get_preprocessed_seq_data``, the ``eval_sequence`` of HOTA, CLEAR, Identity and
Count, their ``combine_sequences`` and ``utils.write_summary_results`` produce what is stored: only arrays --

    the packed inputs (PackedSequences' arrays, ``names``), ``raw_similarity`` (all frames, concatenated),
    the preprocessed ``pre::gt_off / tr_off / gt_ids / tr_ids / n_gt_ids / n_tr_ids / n_gt_dets / n_tr_dets``,
    ``res::<field>`` with one row per sequence and COMBINED_SEQ as the last row,
    ``summary_names`` / ``summary_values``: the two lines of pedestrian_summary.txt.

Robustness check.  HOTA's per-frame assignments depend on the global alignment score, float sums over the frames
that an implementation may form in another order.  A fixture must not depend on that order: every sequence is
evaluated a second time, by the reference alone, with its frames in REVERSED order (HOTA does not look at the order
of frames except through the order of those sums), and is kept only if HOTA_TP, HOTA_FN and HOTA_FP are identical at
all 19 thresholds.  Every sequence below is there for an edge the tests name, so one that fails is not dropped
quietly: the run stops without writing anything, and the sequence gets another seed.

The sequences are small synthetic random walks (``evaluation.synthetic_sequence``: noise, misses, false positives,
id switches, exact copies, gaps after which ids return) plus hand-made frames for the edges: no ground truth / no
detections in a frame and in a whole sequence, one frame, 65 detections against 7 ground truths and 70 ground truths
against 9 detections, about 150 ids in the identity problem, distractors overlapping detections above and below
IoU 0.5, zero-marked rows, IoU exactly 0.5 and exactly 1.
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

CLASS_IDS = {"pedestrian": 1, "person_on_vehicle": 2, "car": 3, "bicycle": 4, "motorbike": 5, "non_mot_vehicle": 6,
             "static_person": 7, "distractor": 8, "occluder": 9, "occluder_on_ground": 10, "occluder_full": 11,
             "reflection": 12, "crowd": 13}


def edge_sequence():
    """Hand-made frames: thresholds hit exactly, distractors on both sides of 0.5, empty frames, a returning id."""
    big, half = [0.0, 0.0, 10.0, 10.0], [0.0, 0.0, 10.0, 5.0]           # IoU exactly 0.5
    far = [100.0, 100.0, 20.0, 40.0]
    f = lambda ids, boxes, cls=None, zm=None: (np.array(ids, np.int64), np.array(boxes, np.float64).reshape(-1, 4),   # noqa
                                               np.array(cls if cls is not None else [1] * len(ids), np.int64),
                                               np.array(zm if zm is not None else [1] * len(ids), np.int64))
    t = lambda ids, boxes: (np.array(ids, np.int64), np.array(boxes, np.float64).reshape(-1, 4))    # noqa: E731
    frames = [
        (f([1, 2], [big, far]), t([7, 8], [half, far])),                               # 0.5 and 1.0
        (f([1, 2], [big, far]), t([], [])),                                            # no detections
        (f([], []), t([7, 8], [half, far])),                                           # no ground truth
        (f([1, 2], [big, far]), t([8, 7], [half, far])),                               # ids swapped: switches
        (f([2], [far]), t([8], [far])),                                                # 1 away ...
        (f([2], [far]), t([8], [far])),
        (f([1, 2], [big, far]), t([9, 8], [big, far])),                                # ... and back under a new id
        # a distractor well matched (its detection goes), one badly matched (IoU 1/3: stays), a zero-marked pedestrian
        (f([1, 3, 4, 5], [big, [200, 0, 10, 10], [300, 0, 10, 10], [400, 0, 10, 10]], [1, 8, 12, 1], [1, 1, 1, 0]),
         t([7, 20, 21, 22], [big, [200, 0, 10, 9], [300, 0, 10, 30], [400, 0, 10, 10]])),
        (f([1, 6, 7], [big, [500, 0, 10, 10], [600, 0, 10, 10]], [1, 2, 7]),
         t([7, 23, 24], [big, [500, 0, 10, 10], [600, 0, 10, 4]])),
        (f([1, 2], [big, big]), t([7, 8], [big, big])),                                # two exact duplicates: ties
    ]
    seq = {k: [] for k in ("gt_ids", "gt_boxes", "gt_classes", "gt_zero_marked", "tracker_ids", "tracker_boxes")}
    for (gi, gb, gc, gz), (ti, tb) in frames:
        for k, v in zip(seq, (gi, gb, gc, gz, ti, tb)):
            seq[k].append(v)
    return seq


def blank(seq, frames, side):
    keys = ("gt_ids", "gt_boxes", "gt_classes", "gt_zero_marked") if side == "gt" else ("tracker_ids", "tracker_boxes")
    for t in frames:
        for k in keys:
            seq[k][t] = seq[k][t][:0]
    return seq


def sequences():
    S = E.synthetic_sequence
    every = lambda s: range(len(s["gt_ids"]))                                          # noqa: E731
    return {
        "edges": edge_sequence(),
        "one_frame": S(1, 1, 5, n_distractors=1),
        "walk37": blank(blank(S(2, 37, 9, n_distractors=3, zero_marked=0.1, gap=0.08), [5], "gt"), [11, 12], "tracker"),
        "walk130": S(3, 130, 12, n_distractors=2, switch=0.03, gap=0.05),
        "wide_65x7": S(4, 6, 7, n_false=58, miss=0.0, gap=0.0),                         # 65 detections, 7 ground truths
        "tall_70x9": S(5, 6, 70, n_false=0, miss=0.0, gap=0.0, track=list(range(9))),   # 70 ground truths, 9 detections
        "ids150": S(6, 37, 60, n_false=1, switch=0.04, gap=0.04),                       # G + K about 150
        "no_tracker": blank(S(7, 8, 4), range(8), "tracker"),
        "no_gt": blank(S(8, 8, 4), range(8), "gt"),
        "all_distractors": S(9, 5, 0, n_distractors=4, n_false=2),                      # ground truth empty AFTER preprocessing
    }


def reference_eval(trackeval, seqs, benchmark):
    ds = trackeval.datasets.MotChallenge2DBox.__new__(trackeval.datasets.MotChallenge2DBox)
    ds.benchmark, ds.do_preproc = benchmark, True
    ds.class_name_to_class_id = CLASS_IDS
    ds.valid_class_numbers = list(CLASS_IDS.values())
    metrics = [trackeval.metrics.HOTA(), trackeval.metrics.CLEAR({"PRINT_CONFIG": False}),
               trackeval.metrics.Identity({"PRINT_CONFIG": False}), trackeval.metrics.Count()]

    def run(name, seq, order):
        raw = {"num_timesteps": len(order), "seq": name,
               "gt_ids": [seq["gt_ids"][t].astype(int) for t in order],
               "gt_dets": [seq["gt_boxes"][t].astype(np.float64).reshape(-1, 4) for t in order],
               "gt_classes": [seq["gt_classes"][t].astype(int) for t in order],
               "gt_extras": [{"zero_marked": seq["gt_zero_marked"][t].astype(int)} for t in order],
               "tracker_ids": [seq["tracker_ids"][t].astype(int) for t in order],
               "tracker_dets": [seq["tracker_boxes"][t].astype(np.float64).reshape(-1, 4) for t in order],
               "tracker_classes": [np.ones(len(seq["tracker_ids"][t]), int) for t in order],
               "tracker_confidences": [np.ones(len(seq["tracker_ids"][t])) for t in order]}
        raw["similarity_scores"] = [ds._calculate_similarities(g, k) for g, k in zip(raw["gt_dets"], raw["tracker_dets"])]
        data = ds.get_preprocessed_seq_data(raw, "pedestrian")
        return raw, data, {m.get_name(): m.eval_sequence(data) for m in metrics}

    kept, raws, datas, results = {}, {}, {}, {}
    for name, seq in seqs.items():
        T = len(seq["gt_ids"])
        raw, data, res = run(name, seq, list(range(T)))
        _, _, rev = run(name, seq, list(range(T))[::-1])
        if any(not np.array_equal(res["HOTA"][k], rev["HOTA"][k]) for k in ("HOTA_TP", "HOTA_FN", "HOTA_FP")):
            raise SystemExit(f"{name}: HOTA's integer fields change with the frame order; it cannot be a fixture "
                             "(give it another seed), nothing written")
        kept[name], raws[name], datas[name], results[name] = seq, raw, data, res
    combined = {m.get_name(): m.combine_sequences({n: r[m.get_name()] for n, r in results.items()}) for m in metrics}
    with tempfile.TemporaryDirectory() as tmp:
        table = [m.summary_results({"COMBINED_SEQ": combined[m.get_name()]}) for m in metrics]
        trackeval.utils.write_summary_results(table, "pedestrian", tmp)
        with open(os.path.join(tmp, "pedestrian_summary.txt")) as f:
            header, values = f.readline().split(), f.readline().split()
    return kept, raws, datas, results, combined, header, values


def store(path, trackeval, seqs, benchmark):
    kept, raws, datas, results, combined, header, values = reference_eval(trackeval, seqs, benchmark)
    p = E.pack_sequences(kept)
    arrays = {k: getattr(p, k) for k in p.ARRAYS}
    arrays["names"] = np.array(p.names)
    arrays["raw_similarity"] = np.concatenate([s.reshape(-1) for n in p.names for s in raws[n]["similarity_scores"]])
    cat = lambda key, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for n in p.names for x in datas[n][key]] +     # noqa
                                         [np.zeros(0, dt)])
    count = lambda key: np.concatenate(([0], np.cumsum([len(x) for n in p.names for x in datas[n][key]]))).astype(np.int32)  # noqa
    arrays.update({"pre::gt_off": count("gt_ids"), "pre::tr_off": count("tracker_ids"),
                   "pre::gt_ids": cat("gt_ids", np.int32), "pre::tr_ids": cat("tracker_ids", np.int32),
                   "pre::similarity": cat("similarity_scores", np.float64)})
    for key, field in (("n_gt_ids", "num_gt_ids"), ("n_tr_ids", "num_tracker_ids"), ("n_gt_dets", "num_gt_dets"),
                       ("n_tr_dets", "num_tracker_dets")):
        arrays["pre::" + key] = np.array([datas[n][field] for n in p.names], np.int64)
    for metric in combined:
        for field in combined[metric]:
            rows = [results[n][metric][field] for n in p.names] + [combined[metric][field]]
            is_int = field in E.INT_FIELDS
            arrays["res::" + field] = np.array(rows, np.int64 if is_int else np.float64)
    arrays["summary_names"], arrays["summary_values"] = np.array(header), np.array(values)
    save_npz(path, **arrays)
    print(path, f"{os.path.getsize(path)} bytes, sequences:", ", ".join(p.names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "TrackEval"))
    import trackeval
    seqs = sequences()
    store(os.path.join(OUT, "trackeval_mot17.npz"), trackeval, seqs, "MOT17")
    store(os.path.join(OUT, "trackeval_mot15.npz"), trackeval,
          {k: seqs[k] for k in ("edges", "walk37", "no_tracker")}, "MOT15")


if __name__ == "__main__":
    main()
