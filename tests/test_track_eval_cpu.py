"""CPU: the host statement of the tracking evaluation (memotr_amd/evaluation.py) against what TrackEval produced
(tests/golden/trackeval_*.npz, tests/golden/gen_golden_track_eval.py): similarities bit for bit, preprocessed ids and
every integer field exactly, float fields within 1e-9 (float64 sums of fewer than 1e5 terms of size at most 1 differ
by about 1e-11 between summation orders); the summary, the evaluator fed from tracker results and from text files,
and the C ABI of libtrack_eval_hip.so without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header
from track_eval_helpers import SETS, check_results, check_tables, golden

from memotr_amd import evaluation as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def track_eval_lib():
    from memotr_amd.build import build_track_eval_lib
    build_track_eval_lib()
    from memotr_amd import _track_eval_lib
    return _track_eval_lib


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_statement_equals_trackeval(name):
    g, packed = golden(name)
    check_tables(E.host_tables(packed, SETS[name]), g)
    res = E.evaluate_packed(packed, SETS[name], device="cpu")
    assert list(res) == packed.names + ["COMBINED_SEQ"]
    print("largest float difference", check_results(res, g, packed.names))


def test_fixture_covers_the_edges():
    g, p = golden("trackeval_mot17")
    n_gt, n_tr, frames = np.diff(p.gt_off), np.diff(p.tr_off), np.diff(p.seq_off)
    assert {1, 37, 130} <= set(frames.tolist()) and len(frames) >= 3
    assert ((n_gt == 0) & (n_tr > 0)).any() and ((n_tr == 0) & (n_gt > 0)).any()
    assert ((n_tr == 65) & (n_gt == 7)).any() and ((n_gt == 70) & (n_tr == 9)).any()
    assert (g["pre::n_gt_ids"] + g["pre::n_tr_ids"]).max() >= 140
    assert (g["pre::n_tr_dets"] == 0).any() and (g["pre::n_gt_dets"] == 0).any()
    assert set(E.DISTRACTOR_CLASSES) <= set(p.gt_classes.tolist()) and (p.gt_zero_marked == 0).any()
    assert (g["raw_similarity"] == 0.5).any() and (g["raw_similarity"] == 1.0).any()
    assert len(g["pre::tr_ids"]) < len(p.tr_ids)                 # preprocessing removed detections on distractors
    # every sequence the generator names is there (it stops when one fails its frame-order check)
    assert p.names == ["edges", "one_frame", "walk37", "walk130", "wide_65x7", "tall_70x9", "ids150", "no_tracker",
                       "no_gt", "all_distractors"]
    # a distractor whose best detection overlaps it above 0.5 and one whose best stays below; an id that returns
    sim_off = np.concatenate(([0], np.cumsum(n_gt.astype(np.int64) * n_tr)))
    above = below = returns = False
    for f in np.flatnonzero((n_gt > 0) & (n_tr > 0)):
        sim = g["raw_similarity"][sim_off[f]:sim_off[f + 1]].reshape(n_gt[f], n_tr[f])
        best = sim[np.isin(p.gt_classes[p.gt_off[f]:p.gt_off[f + 1]], E.DISTRACTOR_CLASSES)].max(1)
        above, below = above or bool((best >= 0.5).any()), below or bool(((best > 0) & (best < 0.5)).any())
    for s in range(len(p.names)):
        last = {}
        for t, f in enumerate(range(p.seq_off[s], p.seq_off[s + 1])):
            for i in p.gt_ids[p.gt_off[f]:p.gt_off[f + 1]].tolist():
                returns = returns or t - last.get(i, t) > 1
                last[i] = t
    assert above and below and returns


def test_mot15_switch_skips_matching_and_class_filter():
    g, packed = golden("trackeval_mot15")
    t15, t17 = E.host_tables(packed, "MOT15"), E.host_tables(packed, "MOT17")
    assert len(t15["tr_ids"]) == len(packed.tr_ids) > len(t17["tr_ids"])          # no detection removed
    assert len(t15["gt_ids"]) == int((packed.gt_zero_marked != 0).sum()) > len(t17["gt_ids"])
    with pytest.raises(ValueError, match="not supported"):
        E.evaluate_packed(packed, "MOT20", device="cpu")


def test_summary_has_the_names_order_and_values_of_the_summary_file():
    g, packed = golden("trackeval_mot17")
    s = E.summary(E.evaluate_packed(packed, "MOT17", device="cpu")["COMBINED_SEQ"])
    assert list(s) == [str(n) for n in g["summary_names"]] == list(E.SUMMARY_FIELDS)
    for k, v in zip(s, g["summary_values"]):
        assert s[k] == float(v), (k, s[k], v)
        assert isinstance(s[k], int) == (k in E.INT_FIELDS)


class Result:
    """What SequenceTracker reports: ids and xyxy boxes (float32, as ``_report`` makes them)."""

    def __init__(self, ids, boxes):
        self.ids, self.boxes = torch.as_tensor(ids), torch.as_tensor(boxes, dtype=torch.float32)


def tracked(seed, n_frames=6):
    rng = np.random.RandomState(seed)
    out = []
    for t in range(n_frames):
        n = rng.randint(0 if t + 1 < n_frames else 1, 5)         # (a result file ends with the last frame that has a row)
        xy = rng.uniform(0, 500, (n, 2)).astype(np.float32)
        out.append(Result(rng.permutation(9)[:n], np.concatenate([xy, xy + rng.uniform(20, 90, (n, 2)).astype(np.float32)], 1)))
    return out


def write_layout(tmp_path, results_by_seq, with_ini):
    """The directory layout eval_engine.py gives TrackEval, the tracker files written by ``mot_lines``."""
    from memotr_amd.inference import SequenceTracker
    writer = SequenceTracker.__new__(SequenceTracker)
    writer.dataset_name = "DanceTrack"
    gt_root, tracker_dir = tmp_path / "val", tmp_path / "tracker"
    tracker_dir.mkdir()
    for seq, results in results_by_seq.items():
        (gt_root / seq / "gt").mkdir(parents=True)
        rng = np.random.RandomState(len(seq))
        with open(gt_root / seq / "gt" / "gt.txt", "w") as f:
            for t, r in enumerate(results):                       # ground truth: the boxes, moved a little, other ids
                for i, (x1, y1, x2, y2) in zip(r.ids.tolist(), r.boxes.tolist()):
                    f.write(f"{t + 1},{i + 100},{x1 + rng.uniform(-4, 4)},{y1},{x2 - x1},{y2 - y1},1,1,1\n")
        if with_ini:
            (gt_root / seq / "seqinfo.ini").write_text(f"[Sequence]\nname={seq}\nseqLength={len(results) + 2}\n")
        with open(tracker_dir / f"{seq}.txt", "w") as f:
            for t, r in enumerate(results):
                f.writelines(writer.mot_lines(t, r))
    seqmap = tmp_path / "val_seqmap.txt"
    seqmap.write_text("name\n" + "\n".join(results_by_seq) + "\n")
    return str(gt_root), str(tracker_dir), str(seqmap)


def test_add_frame_forms_the_doubles_mot_lines_prints(tmp_path):
    results = tracked(3)
    _, tracker_dir, _ = write_layout(tmp_path, {"a": results}, with_ini=False)
    rows = E.read_mot_txt(os.path.join(tracker_dir, "a.txt"))
    ev = E.TrackingEvaluator()
    for t, r in enumerate(results):
        ev.add_frame("a", t, r)
    seq = ev.sequences()["a"]
    assert sum(len(x) for x in seq["tracker_ids"]) == len(rows) > 0
    for t in range(len(results)):
        mine = rows[rows[:, 0] == t + 1]
        assert np.array_equal(seq["tracker_ids"][t], mine[:, 1].astype(np.int64))
        assert np.array_equal(seq["tracker_boxes"][t], mine[:, 2:6])          # bit for bit: repr round-trips
    assert (rows[:, 6] == 1).all() and (rows[:, 7:10] == -1).all()


@pytest.mark.parametrize("with_ini", [False, True])
def test_evaluate_files_equals_the_evaluator_fed_in_memory(tmp_path, with_ini):
    by_seq = {"seq_a": tracked(5, 7), "seq_b": tracked(6, 4)}
    gt_root, tracker_dir, seqmap = write_layout(tmp_path, by_seq, with_ini)
    res = E.evaluate_files(gt_root, tracker_dir, seqmap)
    assert list(res) == ["seq_a", "seq_b", "COMBINED_SEQ"]
    ev = E.TrackingEvaluator()
    for seq, results in by_seq.items():
        gt = E.read_mot_txt(os.path.join(gt_root, seq, "gt", "gt.txt"))
        for t, r in enumerate(results):
            ev.add_frame(seq, t, r)
            mine = gt[gt[:, 0] == t + 1]
            ev.add_ground_truth(seq, t + 1, mine[:, 1].astype(int), mine[:, 2:6])
        if with_ini:                                              # (else: up to the last frame anything was added for)
            ev.set_length(seq, len(results) + 2)
    want = ev.evaluate()
    for name in res:
        for k in res[name]:
            assert np.array_equal(res[name][k], want[name][k]), (name, k)
    c = res["COMBINED_SEQ"]
    assert c["CLR_Frames"] == (15 if with_ini else 11) and c["CLR_TP"] == c["GT_Dets"] == c["Dets"] > 0
    assert c["IDSW"] == 0 and c["MOTA"] == 1.0 and 0.5 < c["MOTP"] < 1.0


def test_evaluator_rejects_what_trackeval_rejects():
    ev = E.TrackingEvaluator()
    ev.add_ground_truth("s", 1, [4, 4], [[0, 0, 1, 1], [2, 2, 1, 1]])
    with pytest.raises(ValueError, match="more than once"):
        ev.evaluate()
    ev = E.TrackingEvaluator()
    ev.add_ground_truth("s", 3, [4], [[0, 0, 1, 1]])
    ev.set_length("s", 2)
    with pytest.raises(ValueError, match="outside"):
        ev.evaluate()


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_every_declared_symbol(track_eval_lib):
    syms = assert_binding_matches_header(track_eval_lib, "track_eval_hip.h", "trackeval", "TRACKEVAL_ABI_VERSION")
    assert len(syms) == 9
    header = open(os.path.join(ROOT, "include", "track_eval_hip.h")).read()
    assert int(re.search(r"#define TRACKEVAL_MAX_DIM (\d+)", header).group(1)) == track_eval_lib.MAX_DIM == 2048
    assert int(re.search(r"#define TRACKEVAL_N_ALPHA (\d+)", header).group(1)) == track_eval_lib.N_ALPHA == len(E.ALPHAS)
    assert track_eval_lib.CLEAR_INTS == E.CLEAR_INTS[:8]


def test_argument_errors_are_reported_without_a_device(track_eval_lib):
    lib = track_eval_lib.lib
    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch
    err = lib.trackeval_last_error
    calls = {
        "trackeval_similarity": lambda n=3, a=p: lib.trackeval_similarity(a, p, p, p, p, n, p, None),
        "trackeval_preproc_match": lambda n=3, a=p, g=5, k=5: lib.trackeval_preproc_match(a, p, p, p, p, n, g, k, p, p, None),
        "trackeval_accumulate": lambda n=3, a=p, g=5, k=5: lib.trackeval_accumulate(a, p, p, p, p, p, p, n, p, p, p, p, p, g, k,
                                                                                   p, p, p, p, p, None),
        "trackeval_hota_match": lambda n=3, a=p, g=5, k=5: lib.trackeval_hota_match(a, p, p, p, p, p, p, n, p, p, p, p, g, k,
                                                                                   p, p, p, p, None),
        "trackeval_hota_reduce": lambda n=3, a=p: lib.trackeval_hota_reduce(a, n, p, p, p, p, p, p, p, p, p, p, p, p, None),
        "trackeval_clear": lambda n=3, a=p, g=5, k=5: lib.trackeval_clear(a, p, p, p, p, p, p, n, p, g, k, 9, p, p, p, None),
        "trackeval_identity": lambda n=3, a=p, g=5: lib.trackeval_identity(n, a, p, p, p, p, p, p, p, g, p, p, None),
    }
    for name, call in calls.items():
        assert call(a=None) == 1 and b"null pointer" in err() and name.encode() in err(), name
        assert call(n=-1) == 1 and b"negative" in err(), name
        assert call(n=0) == 0 and err() == b"", name             # an empty call launches nothing and clears the text
    # a problem beyond the cap is an error with the numbers in it, never a wrong answer
    for name in ("trackeval_preproc_match", "trackeval_accumulate", "trackeval_hota_match", "trackeval_clear"):
        assert calls[name](g=2049) == 2 and b"exceeds TRACKEVAL_MAX_DIM = 2048" in err() and b"2049" in err(), name
        assert calls[name](k=2049) == 2 and b"TRACKEVAL_MAX_DIM" in err(), name
        assert calls[name](g=-1) == 1 and b"negative" in err(), name
    assert calls["trackeval_identity"](g=2049) == 2
    assert b"2049 ground-truth plus tracker ids exceeds TRACKEVAL_MAX_DIM = 2048" in err()
    assert lib.trackeval_clear(p, p, p, p, p, p, p, 3, p, 5, 5, 2049, p, p, p, None) == 2 and b"ids" in err()
    with pytest.raises(RuntimeError, match="null pointer"):
        track_eval_lib.check(calls["trackeval_similarity"](a=None), "trackeval_similarity")
