"""Golden vectors for the association analysis (memotr_amd/association.py, clipops_hota_events_f64,
clipops_identity_pairs_i32), produced by TrackEval's own code from a checkout of the reference (the tests that read the
fixture need neither):

    python tests/golden/gen_golden_association.py --reference /path/to/reference   ->  tests/golden/association.npz

``trackeval`` is imported from ``<reference>/TrackEval`` as it is.  The sequences, the dataset object and the
preprocessing are ``gen_golden_clear_events.py``'s (and so ``gen_golden_track_eval.py``'s): MOT17 rules on all of
``sequences()``, MOT15 on ``edges`` / ``walk37`` / ``no_tracker``.  TrackEval returns sums, so the matches are taken
where they pass by:

  * ``trackeval.metrics.hota.linear_sum_assignment`` is wrapped with a recorder.  ``HOTA.eval_sequence`` calls it once
    per timestep that has both ground truth and detections, in order, with ``-score_mat``; every returned pair is kept,
    with its entry of the timestep's similarity (what the 19 thresholds are then applied to).
  * ``trackeval.metrics.identity.linear_sum_assignment`` is wrapped likewise.  ``Identity.eval_sequence`` calls it once
    per sequence that has both ground truth and detections, on the (G + K) x (G + K) matrix ``fn_mat + fp_mat``.

Stored, under ``mot17::`` and ``mot15::``, arrays only (the inputs are the ``mot17::`` / ``mot15::`` arrays of
clear_events.npz): ``names``; ``pair_off`` int32 [F + 1] with ``pair_gt`` / ``pair_tr`` int32, the pairs of every frame as
relabelled ids sorted by ground-truth id, and ``pair_sim`` float64, their similarity; ``hota_calls`` int32 [S], the
solver calls of every sequence; ``id_off`` int32 [S + 1] with ``id_rows`` / ``id_cols`` int32, the Identity metric's
assignment of every sequence, and ``id_shape`` int32 [S, 2], its G and K.
"""
import argparse
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)                               # gen_golden_track_eval (which puts tests/ and the root on the path)

import gen_golden_track_eval as G  # noqa: E402
from conftest import save_npz  # noqa: E402


def record(trackeval, seqs, benchmark):
    ds = trackeval.datasets.MotChallenge2DBox.__new__(trackeval.datasets.MotChallenge2DBox)
    ds.benchmark, ds.do_preproc = benchmark, True
    ds.class_name_to_class_id = G.CLASS_IDS
    ds.valid_class_numbers = list(G.CLASS_IDS.values())
    hota = trackeval.metrics.HOTA({"PRINT_CONFIG": False})
    identity = trackeval.metrics.Identity({"PRINT_CONFIG": False})
    calls = []

    def recorded(module, run):
        solver = module.linear_sum_assignment

        def recorder(cost):
            rows, cols = solver(cost)
            calls.append((np.array(cost).shape, np.array(rows), np.array(cols)))
            return rows, cols

        module.linear_sum_assignment = recorder
        try:
            del calls[:]
            run()
            return list(calls)
        finally:
            module.linear_sum_assignment = solver

    pairs, hota_calls, id_pairs, id_shape = [], [], [], []
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
        seen = recorded(trackeval.metrics.hota, lambda: hota.eval_sequence(data))     # noqa: B023
        solved = [t for t in range(T) if len(data["gt_ids"][t]) and len(data["tracker_ids"][t])]
        if data["num_gt_dets"] == 0 or data["num_tracker_dets"] == 0:
            solved = []                                # (eval_sequence returns before its loop)
        assert len(seen) == len(solved), name
        kept = {t: np.zeros((0, 3)) for t in range(T)}
        for t, (shape, rows, cols) in zip(solved, seen):
            assert shape == data["similarity_scores"][t].shape, name
            g, k = data["gt_ids"][t][rows], data["tracker_ids"][t][cols]
            order = np.argsort(g)
            kept[t] = np.stack([g[order], k[order], data["similarity_scores"][t][rows, cols][order]], 1)
        pairs += [kept[t] for t in range(T)]
        hota_calls.append(len(seen))
        seen = recorded(trackeval.metrics.identity, lambda: identity.eval_sequence(data))     # noqa: B023
        n = data["num_gt_ids"] + data["num_tracker_ids"]
        assert len(seen) == (0 if not solved and (data["num_gt_dets"] == 0 or data["num_tracker_dets"] == 0) else 1), name
        assert all(shape == (n, n) for shape, _, _ in seen), name
        id_pairs.append(np.stack([seen[0][1], seen[0][2]], 1) if seen else np.zeros((0, 2), int))
        id_shape.append((data["num_gt_ids"], data["num_tracker_ids"]))
    off = lambda parts: np.concatenate(([0], np.cumsum([len(x) for x in parts]))).astype(np.int32)        # noqa: E731
    col = lambda parts, c, dt: np.concatenate([x[:, c] for x in parts] + [np.zeros(0)]).astype(dt)        # noqa: E731
    return {"names": np.array(list(seqs)), "pair_off": off(pairs), "pair_gt": col(pairs, 0, np.int32),
            "pair_tr": col(pairs, 1, np.int32), "pair_sim": col(pairs, 2, np.float64),
            "hota_calls": np.asarray(hota_calls, np.int32), "id_off": off(id_pairs),
            "id_rows": col(id_pairs, 0, np.int32), "id_cols": col(id_pairs, 1, np.int32),
            "id_shape": np.asarray(id_shape, np.int32).reshape(-1, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "TrackEval"))
    import trackeval
    seqs = G.sequences()
    arrays = {"mot17::" + k: v for k, v in record(trackeval, seqs, "MOT17").items()}
    arrays.update({"mot15::" + k: v for k, v in
                   record(trackeval, {k: seqs[k] for k in ("edges", "walk37", "no_tracker")}, "MOT15").items()})
    path = os.path.join(OUT, "association.npz")
    save_npz(path, **arrays)
    print(path, f"{os.path.getsize(path)} bytes; HOTA solver calls {arrays['mot17::hota_calls'].tolist()} + "
          f"{arrays['mot15::hota_calls'].tolist()}, {len(arrays['mot17::pair_gt'])} + {len(arrays['mot15::pair_gt'])} pairs")


if __name__ == "__main__":
    main()
