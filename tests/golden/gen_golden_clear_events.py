"""Golden vectors for the error analysis (memotr_amd/diagnose.py, clipops_clear_events_f64), produced by TrackEval's own
code from a checkout of the reference (the tests that read the fixture need neither):

    python tests/golden/gen_golden_clear_events.py --reference /path/to/reference   ->  tests/golden/clear_events.npz

``trackeval`` is imported from ``<reference>/TrackEval`` as it is.  The sequences, the dataset object and the
preprocessing are ``gen_golden_track_eval.py``'s (the edge frames, 65 detections against 7 ground truths and 70 ground
truths against 9 detections, empty frames and empty sequences, exact ties, distractors and zero-marked rows).  TrackEval
never returns CLEAR's decisions, so they are taken where they pass by:

  * ``trackeval.metrics.clear.linear_sum_assignment`` is wrapped with a recorder.  ``CLEAR.eval_sequence`` calls it once
    per timestep that has both ground truth and detections, in order, with ``-score_mat``; the pairs it keeps are the
    returned ones whose score exceeds the float64 epsilon (its ``actually_matched_mask``).
  * the IDSW increment of a timestep is ``IDSW`` of ``eval_sequence`` on the first t + 1 timesteps minus ``IDSW`` on the
    first t (the preprocessed data cut to a prefix, its detection counts formed again).

Stored, under ``mot17::`` and ``mot15::``, arrays only: the packed inputs (PackedSequences' arrays, ``names``); the
preprocessed ``pre::gt_off / tr_off / gt_ids / tr_ids`` (TrackEval's relabelled ids, all frames concatenated);
``pair_off`` int32 [F + 1] with ``pair_gt`` / ``pair_tr``, the kept pairs of every frame as relabelled ids, sorted by
ground-truth id; ``idsw`` int32 [F], the per-frame IDSW increments.
"""
import argparse
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)                               # gen_golden_track_eval (which puts tests/ and the root on the path)

import gen_golden_track_eval as G  # noqa: E402
from conftest import save_npz  # noqa: E402
from memotr_amd import evaluation as E  # noqa: E402

EPS = np.finfo("float").eps


def record(trackeval, seqs, benchmark):
    ds = trackeval.datasets.MotChallenge2DBox.__new__(trackeval.datasets.MotChallenge2DBox)
    ds.benchmark, ds.do_preproc = benchmark, True
    ds.class_name_to_class_id = G.CLASS_IDS
    ds.valid_class_numbers = list(G.CLASS_IDS.values())
    clear = trackeval.metrics.CLEAR({"PRINT_CONFIG": False})
    module = trackeval.metrics.clear
    solver, calls = module.linear_sum_assignment, []

    def recorder(cost):
        rows, cols = solver(cost)
        calls.append((np.array(cost), rows, cols))
        return rows, cols

    def prefix(data, t):
        cut = dict(data)
        for k in ("gt_ids", "tracker_ids", "similarity_scores"):
            cut[k] = data[k][:t]
        cut["num_timesteps"] = t
        cut["num_gt_dets"] = sum(len(x) for x in cut["gt_ids"])
        cut["num_tracker_dets"] = sum(len(x) for x in cut["tracker_ids"])
        return cut

    pre = {k: [] for k in ("gt_ids", "tracker_ids")}
    pairs, idsw = [], []
    for name, seq in seqs.items():
        T = len(seq["gt_ids"])
        raw = {"num_timesteps": T, "seq": name,
               "gt_ids": [x.astype(int) for x in seq["gt_ids"]],
               "gt_dets": [x.astype(np.float64).reshape(-1, 4) for x in seq["gt_boxes"]],
               "gt_classes": [x.astype(int) for x in seq["gt_classes"]],
               "gt_extras": [{"zero_marked": x.astype(int)} for x in seq["gt_zero_marked"]],
               "tracker_ids": [x.astype(int) for x in seq["tracker_ids"]],
               "tracker_dets": [x.astype(np.float64).reshape(-1, 4) for x in seq["tracker_boxes"]],
               "tracker_classes": [np.ones(len(x), int) for x in seq["tracker_ids"]],
               "tracker_confidences": [np.ones(len(x)) for x in seq["tracker_ids"]]}
        raw["similarity_scores"] = [ds._calculate_similarities(g, k) for g, k in zip(raw["gt_dets"], raw["tracker_dets"])]
        data = ds.get_preprocessed_seq_data(raw, "pedestrian")
        module.linear_sum_assignment = recorder
        try:
            del calls[:]
            total = clear.eval_sequence(data)["IDSW"]
            seen = list(calls)
        finally:
            module.linear_sum_assignment = solver
        solved = [t for t in range(T) if len(data["gt_ids"][t]) and len(data["tracker_ids"][t])]
        if data["num_gt_dets"] == 0 or data["num_tracker_dets"] == 0:
            solved = []                                # (eval_sequence returns before its loop)
        assert len(seen) == len(solved), name
        kept = {t: None for t in range(T)}
        for t, (cost, rows, cols) in zip(solved, seen):
            hit = -cost[rows, cols] > 0 + EPS
            g, k = data["gt_ids"][t][rows[hit]], data["tracker_ids"][t][cols[hit]]
            order = np.argsort(g)
            kept[t] = np.stack([g[order], k[order]], 1)
        running = [clear.eval_sequence(prefix(data, t))["IDSW"] for t in range(T + 1)]
        assert running[-1] == total, name
        for t in range(T):
            pairs.append(kept[t] if kept[t] is not None else np.zeros((0, 2), int))
            idsw.append(running[t + 1] - running[t])
            for k in pre:
                pre[k].append(np.asarray(data[k][t], int))
    return pre, pairs, idsw


def arrays_of(trackeval, seqs, benchmark):
    pre, pairs, idsw = record(trackeval, seqs, benchmark)
    p = E.pack_sequences(seqs)
    off = lambda parts: np.concatenate(([0], np.cumsum([len(x) for x in parts]))).astype(np.int32)        # noqa: E731
    cat = lambda parts: np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in parts] + [np.zeros(0, np.int32)])  # noqa
    out = {k: getattr(p, k) for k in p.ARRAYS}
    out["names"] = np.array(p.names)
    out.update({"pre::gt_off": off(pre["gt_ids"]), "pre::tr_off": off(pre["tracker_ids"]),
                "pre::gt_ids": cat(pre["gt_ids"]), "pre::tr_ids": cat(pre["tracker_ids"]),
                "pair_off": off(pairs), "pair_gt": cat([x[:, 0] for x in pairs]), "pair_tr": cat([x[:, 1] for x in pairs]),
                "idsw": np.asarray(idsw, np.int32)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "TrackEval"))
    import trackeval
    seqs = G.sequences()
    arrays = {"mot17::" + k: v for k, v in arrays_of(trackeval, seqs, "MOT17").items()}
    arrays.update({"mot15::" + k: v for k, v in
                   arrays_of(trackeval, {k: seqs[k] for k in ("edges", "walk37", "no_tracker")}, "MOT15").items()})
    path = os.path.join(OUT, "clear_events.npz")
    save_npz(path, **arrays)
    print(path, f"{os.path.getsize(path)} bytes, {int(arrays['mot17::idsw'].sum())} + {int(arrays['mot15::idsw'].sum())} "
          "switches")


if __name__ == "__main__":
    main()
