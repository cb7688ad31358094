"""CPU: the offline pass over result rows (memotr_amd/postprocess.py ``fill_gaps``) against an independent per-track loop
in float64, its properties and edges, the writers and the evaluator on a filled log, ``submit`` with ``postprocess=``,
and the C ABI of the kernels behind ``filled`` on a device."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dataset_trees as T
import postprocess_cases as C
from cabi_helpers import assert_binding_matches_header

from memotr_amd import submit as S
from memotr_amd.postprocess import fill_gaps, postprocess_options
from memotr_amd.results import BankResultLog, ResultLog, Rows


@pytest.fixture(scope="module", autouse=True)
def libraries(request):
    """The writers and the trackers import the package's models, which bind the operator library."""
    request.getfixturevalue("hip_lib"), request.getfixturevalue("clip_lib")


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("seed, n_ids, n_frames, drop, max_gap, min_length",
                         [(0, 12, 90, 0.3, 5, 4), (1, 5, 200, 0.8, 63, 0), (2, 40, 64, 0.5, 2, 30), (3, 1, 30, 0.5, 30, 1)])
def test_host_statement_against_a_float64_loop(seed, n_ids, n_frames, drop, max_gap, min_length):
    rows = C.rows_from_mask(C.random_mask(n_ids, n_frames, drop, seed), seed)
    got, want = fill_gaps(rows, max_gap, min_length), C.loop_fill(rows, max_gap, min_length)
    assert list(zip(got.frames.tolist(), got.ids.tolist(), got.labels.tolist())) == [r[:3] for r in want]
    assert got.boxes_xyxy.dtype == np.float32 and got.scores.dtype == np.float32
    values, n_new = C.values_of(got), 0
    for v, (_, _, _, exact, ends) in zip(values, want):
        if ends is None:                                    # an input row: bit-equal
            assert v.tolist() == exact
            continue
        n_new += 1
        # the quotient, the difference, the product and the sum are rounded: at most
        # u (3 |b - a| + max(|a|, |b|)) <= 4 u (|a| + |b|), u = 2^-24
        for x, e, (a, b) in zip(v.tolist(), exact, ends):
            assert abs(x - e) <= 2.0 ** -22 * (abs(a) + abs(b))
    assert n_new > 0 and n_new == len(got.frames) - sum(r[4] is None for r in want)


def test_identity_idempotence_and_span():
    rows = C.rows_from_mask(C.random_mask(9, 120, 0.4, 5), 5)
    for min_length in (0, 1):
        C.assert_same_rows(fill_gaps(rows, 0, min_length), rows)
    for max_gap, min_length in ((3, 0), (7, 10), (200, 0)):
        once = fill_gaps(rows, max_gap, min_length)
        C.assert_same_rows(fill_gaps(once, max_gap, min_length), once)
        assert len(once.frames) > len(rows.frames) or min_length
        for tid in np.unique(once.ids):
            src = rows.frames[rows.ids == tid]
            out = once.frames[once.ids == tid]
            assert out.min() == src.min() and out.max() == src.max()
    full = fill_gaps(rows, 200)                              # every hole closed: a row for every frame of every span
    for tid in np.unique(rows.ids):
        src = rows.frames[rows.ids == tid]
        assert full.frames[full.ids == tid].tolist() == list(range(src.min(), src.max() + 1))


def test_edges():
    # holes of exactly max_gap and max_gap + 1 missing frames in one track
    mask = np.zeros((1, 20), bool)
    mask[0, [0, 4, 9, 10]] = True                           # 3 missing, then 4 missing, then none
    rows = C.rows_from_mask(mask, 1)
    assert fill_gaps(rows, 3).frames.tolist() == [0, 1, 2, 3, 4, 9, 10]
    assert fill_gaps(rows, 4).frames.tolist() == list(range(11))
    assert fill_gaps(rows, 2).frames.tolist() == [0, 4, 9, 10]
    # min_length at len - 1, len, len + 1; a removed track changes no other track's rows and fills nothing
    mask = np.zeros((3, 12), bool)
    mask[0, [0, 2, 4, 6]], mask[1, [1, 2, 5]], mask[2, 3:9] = True, True, True
    rows = C.rows_from_mask(mask, 2)
    for min_length, kept in ((2, [0, 1, 2]), (3, [0, 1, 2]), (4, [0, 2]), (5, [2]), (7, [])):
        got = fill_gaps(rows, 5, min_length)
        assert sorted(set(got.ids.tolist())) == kept
        for tid in kept:
            pick = np.flatnonzero(rows.ids == tid)
            alone = fill_gaps(Rows(*(a[pick] for a in rows)), 5, 0)
            C.assert_same_rows(Rows(*(a[got.ids == tid] for a in got)), alone)
    # the label is the left row's when it differs across a hole
    labels = np.zeros((1, 6), np.int64)
    labels[0, 4:] = 5
    mask = np.zeros((1, 6), bool)
    mask[0, [0, 1, 4, 5]] = True
    got = fill_gaps(C.rows_from_mask(mask, 3, labels), 2)
    assert got.frames.tolist() == [0, 1, 2, 3, 4, 5] and got.labels.tolist() == [0, 0, 0, 0, 5, 5]
    # the empty log, duplicates, negative arguments
    empty = fill_gaps(C.empty_rows(), 10, 3)
    assert len(empty.frames) == 0 and empty.boxes_xyxy.shape == (0, 4) and empty.scores.dtype == np.float32
    twice = Rows(*(np.concatenate((a, a[:1])) for a in rows))
    with pytest.raises(ValueError, match="more than once"):
        fill_gaps(twice, 0)
    for bad in ((-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            fill_gaps(rows, *bad)
    # unsorted input gives the sorted output
    perm = np.random.RandomState(0).permutation(len(rows.frames))
    C.assert_same_rows(fill_gaps(Rows(*(a[perm] for a in rows)), 5), fill_gaps(rows, 5))


# ---------------------------------------------------------------------------------------------- logs and writers
def moving_object_log(missed=(3, 4, 5), n_frames=9):
    """One object in every frame, moving linearly; the tracker (id 7) misses ``missed``."""
    gt = [[10.0 + 4 * f, 20.0 + 2 * f, 30.0, 40.0] for f in range(n_frames)]         # xywh
    seen = [f for f in range(n_frames) if f not in missed]
    boxes = np.asarray([[gt[f][0], gt[f][1], gt[f][0] + 30.0, gt[f][1] + 40.0] for f in seen], np.float32)
    rows = Rows(np.asarray(seen, np.int64), np.full(len(seen), 7, np.int64), np.zeros(len(seen), np.int64), boxes,
                np.full(len(seen), 0.9, np.float32))
    return C.log_from_rows(rows, "cpu"), gt


def test_writers_and_evaluator_see_the_new_frames():
    from memotr_amd.evaluation import TrackingEvaluator
    log, gt = moving_object_log()
    filled = log.filled(max_gap=3)
    assert isinstance(filled, ResultLog) and filled.device == log.device and len(filled) == 9 and len(log) == 6
    C.assert_same_rows(filled.read(), fill_gaps(log.read(), 3))
    assert [int(line.split(",")[0]) for line in filled.mot_lines("DanceTrack")] == list(range(1, 10))
    assert [int(line.split(",")[0]) for line in log.mot_lines("DanceTrack")] == [1, 2, 3, 7, 8, 9]
    names = [f"video-{i:07d}.jpg" for i in range(9)]
    assert [len(fr["labels"]) for fr in filled.bdd_frames(names)] == [1] * 9
    assert [len(fr["labels"]) for fr in log.bdd_frames(names)] == [1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert filled.bdd_frames(names)[4]["labels"][0]["id"] == "7"
    scores = {}
    for name, which in (("raw", log), ("filled", filled), ("short", log.filled(max_gap=2))):
        ev = TrackingEvaluator("MOT17")
        for f, box in enumerate(gt):
            ev.add_ground_truth("seq", f + 1, [1], [box])
        which.add_to(ev, "seq", 9)
        scores[name] = ev.evaluate()["seq"]
    assert scores["raw"]["CLR_FN"] == 3 and scores["filled"]["CLR_FN"] == 0 and scores["short"]["CLR_FN"] == 3
    assert scores["raw"]["IDs"] == scores["filled"]["IDs"] == 1 and scores["filled"]["CLR_FP"] == 0
    with pytest.raises(ValueError):
        log.filled(max_gap=-1)
    with pytest.raises(RuntimeError, match="id out of range"):
        log.filled(max_gap=3, n_ids=7)
    with pytest.raises(RuntimeError, match="frame out of range"):
        log.filled(max_gap=3, n_frames=8)
    assert len(log.filled(max_gap=3, n_ids=8, n_frames=9)) == 9


def test_bank_log_fills_every_sequence_on_its_own():
    sequences = {0: C.rows_from_mask(C.random_mask(4, 30, 0.4, 0), 0), 2: C.rows_from_mask(C.random_mask(6, 17, 0.3, 1), 1)}
    log = C.bank_log_from_rows(sequences, "cpu")
    filled = log.filled(max_gap=4, min_length=3)
    assert isinstance(filled, BankResultLog) and filled.dataset_name == log.dataset_name
    assert sorted(filled.read()) == [0, 2]
    for seq, rows in sequences.items():
        C.assert_same_rows(filled.read()[seq], fill_gaps(rows, 4, 3))
        C.assert_same_rows(filled.sequence(seq).read(), fill_gaps(rows, 4, 3))
        assert len(filled.mot_lines(seq)) == len(fill_gaps(rows, 4, 3).frames) > len(rows.frames) - 10
    assert len(filled.sequence(1)) == 0
    assert log.filled(max_gap=0).read()[2].frames.tolist() == sequences[2].frames.tolist()
    assert C.bank_log_from_rows({}, "cpu").filled(max_gap=3).read() == {}


# ---------------------------------------------------------------------------------------------- submit
def test_postprocess_options(monkeypatch):
    monkeypatch.delenv("MEMOTR_POSTPROCESS", raising=False)
    assert postprocess_options(None) is None
    assert postprocess_options(dict(max_gap=4)) == dict(max_gap=4, min_length=0)
    monkeypatch.setenv("MEMOTR_POSTPROCESS", "max_gap=20,min_length=5")
    assert postprocess_options(None) == dict(max_gap=20, min_length=5)
    assert postprocess_options(dict(min_length=2)) == dict(max_gap=0, min_length=2)          # the argument wins
    monkeypatch.setenv("MEMOTR_POSTPROCESS", "max_gap=20,smooth=1")
    with pytest.raises(TypeError, match="smooth"):
        postprocess_options(None)
    with pytest.raises(TypeError, match="window"):
        postprocess_options(dict(max_gap=1, window=3))
    with pytest.raises(ValueError):
        postprocess_options(dict(max_gap=-1))


def scripted_submit(root, out, **kwargs):
    config = dict(C.SCRIPT_THRESHOLDS, SUBMIT_DIR=str(out), SUBMIT_MODEL=None, SUBMIT_DATA_SPLIT="train", DATA_ROOT=root)
    return S.submit(config, model=C.ScriptedModel(), train_config=dict(DATASET="DanceTrack", USE_DAB=True),
                    tracker_options=dict(raw_size=(96, 160), area_thresh=0), **kwargs)


def read_all(files):
    out = []
    for path in files:
        with open(path) as f:
            out.append(f.read())
    return out


def test_submit_writes_the_files_of_the_filled_log(tmp_path, monkeypatch):
    from memotr_amd.inference import SequenceTracker
    monkeypatch.delenv("MEMOTR_POSTPROCESS", raising=False)
    root = T.write_trees(str(tmp_path / "data"), only=("DanceTrack",))
    raw, want_off, want_on = {}, [], []
    for seq in sorted(T.DANCE_SEQS):                        # the rows as tracked, by hand
        paths = S.sequence_frames("DanceTrack", os.path.join(root, "DanceTrack", "train", seq))
        tracker = SequenceTracker(C.ScriptedModel(), dataset_name="DanceTrack", det_score_thresh=0.9,
                                  track_score_thresh=0.2, result_score_thresh=0.5, miss_tolerance=5, use_dab=True,
                                  raw_size=(96, 160), area_thresh=0)
        log = ResultLog("cpu")
        assert tracker.track_logged(paths, log) == len(paths)
        raw[seq] = log.read()
        want_off.append("".join(log.mot_lines("DanceTrack")))
        want_on.append("".join(C.log_from_rows(fill_gaps(raw[seq], 3, 2), "cpu").mot_lines("DanceTrack")))
    rows = raw["dancetrack0007"]                            # the script: two holes, one spurious track of one row
    assert rows.frames[rows.ids == 0].tolist() == [0, 1, 4, 5, 6] and rows.frames[rows.ids == 3].tolist() == [2]
    off = read_all(scripted_submit(root, tmp_path / "off"))
    assert off == want_off                                  # without the pass: today's bytes
    on = read_all(scripted_submit(root, tmp_path / "on", postprocess=dict(max_gap=3, min_length=2)))
    assert on == want_on and on != off
    assert sum(line.split(",")[1] == "0" for line in on[1].splitlines()) == 7
    assert not any(line.split(",")[1] == "3" for line in on[1].splitlines())
    monkeypatch.setenv("MEMOTR_POSTPROCESS", "max_gap=3,min_length=2")
    assert read_all(scripted_submit(root, tmp_path / "env")) == want_on
    assert read_all(scripted_submit(root, tmp_path / "arg", postprocess=dict(max_gap=0))) == want_off
    with pytest.raises(TypeError, match="smooth"):
        scripted_submit(root, tmp_path / "bad", postprocess=dict(max_gap=3, smooth=True))


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_and_argument_errors(clip_lib):
    from memotr_amd import _clip_lib as L
    declared = assert_binding_matches_header(L, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert "clipops_fill_gaps_f32" in declared and "clipops_fill_gaps_workspace" in declared
    assert L.ABI_VERSION == 12
    ws = L.lib.clipops_fill_gaps_workspace
    assert ws(1, 300, 1050) == 2 * 300 * 1050 + 1050 and ws(3, 4, 5) == 2 * 60 + 15 and ws(0, 4, 5) == 0
    assert ws(-1, 1, 1) == -1 and ws(1, 1, -1) == -1 and ws(2, 65536, 16384) == -2 and ws(1, 46341, 46341) == -2
    buf = (ctypes.c_int64 * 64)()                           # host memory: an argument error touches no pointer
    p = ctypes.addressof(buf)

    def call(rows_f=p, rows_i=p, counters=p, n=4, W=3, n_seq=1, n_ids=2, n_frames=5, max_gap=1, min_length=0,
             workspace=p, out_f=p, out_i=p, out_counters=p, status=p, capacity=8):
        return L.lib.clipops_fill_gaps_f32(rows_f, rows_i, counters, n, W, n_seq, n_ids, n_frames, max_gap, min_length,
                                           workspace, out_f, out_i, out_counters, status, capacity, None)

    for bad in (dict(n=-1), dict(n_seq=-1), dict(n_ids=-1), dict(n_frames=-1), dict(capacity=-1), dict(max_gap=-1),
                dict(min_length=-1), dict(W=2), dict(W=5), dict(W=3, n_seq=2), dict(rows_f=None), dict(rows_i=None),
                dict(counters=None), dict(workspace=None), dict(out_f=None), dict(out_i=None),
                dict(out_counters=None), dict(status=None)):
        assert call(**bad) == 1, bad
        assert b"clipops_fill_gaps_f32" in L.lib.clipops_last_error()
    assert call(W=4, n_seq=2, n_ids=65536, n_frames=16384) == 2 and b"cells" in L.lib.clipops_last_error()
    assert call(n=0, rows_f=None, rows_i=None, workspace=None, out_f=None, out_i=None) == 0      # a no-op
    assert call(n=0, W=7) == 1
