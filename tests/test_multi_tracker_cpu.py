"""CPU: ``MultiSequenceTracker`` (memotr_amd/inference_multi.py) with the small model and the oracle's operator.  Three
sequences of 2, 4 and 3 frames on two streams -- a stream refilled when its sequence ends, the batch shrinking when none
is left -- against three ``SequenceTracker`` runs: the same ids, labels and reported rows, boxes and scores to 1e-4; and
``submit(streams=2)`` writes the rows of ``submit(streams=1)``.  No decision score of the one-sequence runs may lie within
1e-3 of its threshold (tests/multi_track_cases.py)."""
import os

import pytest

import dataset_trees as T
import multi_track_cases as M
from model_helpers import patch_operator

from memotr_amd import submit as S
from memotr_amd.inference_multi import MultiSequenceTracker
from memotr_amd.results import BankResultLog


@pytest.fixture(scope="module")
def scenario():
    """The model, the sequences and the three one-sequence runs (computed once, read by every test)."""
    mp = pytest.MonkeyPatch()
    patch_operator(mp)
    try:
        model, seqs = M.scenario_model(64), M.sequences()
        want, margin = M.single_runs(model, seqs)
    finally:
        mp.undo()
    return model, seqs, want, margin


def test_the_scenario_decides_nothing_near_a_threshold(scenario):
    _, _, want, margin = scenario
    assert margin > M.MARGIN, f"a decision score lies {margin} from its threshold: choose another seed"
    assert M.scenario_is_eventful(want)


@pytest.mark.parametrize("n_streams", [2, 1, 3])
def test_lockstep_streams_track_what_one_tracker_per_sequence_tracks(scenario, monkeypatch, n_streams):
    patch_operator(monkeypatch)
    model, seqs, want, margin = scenario
    assert margin > M.MARGIN
    tracker = MultiSequenceTracker(model, n_streams=n_streams, cap=32, **M.OPTIONS)
    got = M.multi_runs(tracker, seqs)
    M.assert_equivalent(want, got)
    assert tracker.frame_counts == list(M.LENGTHS)
    assert tracker.bank.n_streams == 1                      # the batch shrank as the sequences ended


def test_the_order_of_the_sources_does_not_change_a_sequences_results(scenario, monkeypatch):
    patch_operator(monkeypatch)
    model, seqs, want, _ = scenario
    order = [2, 0, 1]
    got = M.multi_runs(MultiSequenceTracker(model, n_streams=2, cap=32, **M.OPTIONS), [seqs[i] for i in order])
    M.assert_equivalent([want[i] for i in order], got)


def test_a_small_bank_grows_and_a_full_one_is_reported(scenario, monkeypatch):
    patch_operator(monkeypatch)
    model, seqs, want, _ = scenario
    most = max(len(r.ids) for seq in want for r in seq)
    assert most > 8
    tracker = MultiSequenceTracker(model, n_streams=2, cap=16, **M.OPTIONS)
    M.assert_equivalent(want, M.multi_runs(tracker, seqs))
    assert tracker.bank.cap > 16
    # without room to grow into: the births that found no slot are counted, and the end of a sequence raises
    tracker = MultiSequenceTracker(model, n_streams=2, cap=16, **dict(M.OPTIONS, det_score_thresh=0.2))
    monkeypatch.setattr(tracker, "_watch_counts", lambda: None)
    with pytest.raises(RuntimeError, match="dropped .* births"):
        M.multi_runs(tracker, seqs)


def test_logged_tracking_gives_the_rows_of_track_many(scenario, monkeypatch):
    patch_operator(monkeypatch)
    model, seqs, want, _ = scenario
    tracker = MultiSequenceTracker(model, n_streams=2, cap=32, **M.OPTIONS)
    got = M.multi_runs(tracker, seqs)
    log = BankResultLog("cpu", capacity=8)
    assert MultiSequenceTracker(model, n_streams=2, cap=32, **M.OPTIONS).track_many_logged(seqs, log) == list(M.LENGTHS)
    for s, results in enumerate(got):
        lines = [line for idx, r in enumerate(results) for line in tracker.mot_lines(idx, r)]
        assert log.mot_lines(s) == lines and lines
    assert log.mot_lines(7) == []


def test_jpeg_sources_and_mixed_frame_sizes(scenario, monkeypatch):
    """Byte streams decode to the pixels ``track_jpeg`` sees; a sequence of another geometry runs in a group of its own.
    (Frames of their own: the codec moves the scenario's scores, and these keep clear of the thresholds.)"""
    from memotr_amd.data import encode_jpeg
    from memotr_amd.inference import SequenceTracker
    patch_operator(monkeypatch)
    model = scenario[0]
    seqs = M.sequences((2, 3, 3), first=11)
    streams = [[bytes(encode_jpeg(f, quality=90, subsampling="4:2:0")) for f in frames] for frames in seqs[:2]]
    wide = [f[:48].contiguous() for f in seqs[2]]            # 48 x 96: resizes to another target size
    want, margin = [], float("inf")
    for src in streams + [wide]:
        t = SequenceTracker(model, **M.OPTIONS)
        d = M.Decisions(t, model.query_updater.update_threshold)
        want.append([r for _, r in (t.track(src) if src is wide else t.track_jpeg(src))])
        margin = min(margin, d.margin())
    assert margin > M.MARGIN
    got = M.multi_runs(MultiSequenceTracker(model, n_streams=2, cap=32, **M.OPTIONS), streams + [wide])
    M.assert_equivalent(want[:2], got[:2])
    M.assert_equivalent(want[2:], got[2:], ori_h=48)


def test_argument_errors(scenario):
    model = scenario[0]
    with pytest.raises(ValueError, match="USE_MOTION"):
        MultiSequenceTracker(model, n_streams=2, use_motion=True)
    with pytest.raises(ValueError, match="multiple of 16"):
        MultiSequenceTracker(model, n_streams=2, cap=20)
    with pytest.raises(ValueError, match="n_streams"):
        MultiSequenceTracker(model, n_streams=0)
    tracker = MultiSequenceTracker(model, n_streams=2, cap=16, **M.OPTIONS)
    tracker.begin(2)
    with pytest.raises(ValueError, match="1 frames for a bank of 2"):
        tracker.step_raw([M.sequences()[0][0]])
    with pytest.raises(ValueError, match="different geometries"):
        tracker.step_raw([M.sequences()[0][0], M.sequences()[0][0][:48].contiguous()])


def test_submit_with_two_streams_writes_the_rows_of_one(scenario, tmp_path, monkeypatch, request):
    request.getfixturevalue("hip_lib"), request.getfixturevalue("clip_lib")
    patch_operator(monkeypatch)
    model = scenario[0]
    root = T.write_trees(str(tmp_path / "data"))
    train_config = dict(DATASET="DanceTrack", USE_DAB=True)
    # (thresholds chosen for the trees' frames as the scenario's are for its own: the margin is asserted below)
    thresholds = dict(DET_SCORE_THRESH=0.7, TRACK_SCORE_THRESH=0.45, RESULT_SCORE_THRESH=0.6, MISS_TOLERANCE=2,
                      USE_MOTION=False)
    options = dict(raw_size=M.RAW_SIZE, area_thresh=10)
    single = dict(M.OPTIONS, det_score_thresh=0.7, track_score_thresh=0.45, result_score_thresh=0.6)

    def run(name, **kwargs):
        config = dict(thresholds, SUBMIT_DIR=str(tmp_path / name), SUBMIT_MODEL=None, SUBMIT_DATA_SPLIT="train",
                      DATA_ROOT=root)
        files = S.submit(config, model=model, train_config=train_config, tracker_options=options, **kwargs)
        assert [os.path.basename(f) for f in files] == [f"{seq}.txt" for seq in sorted(T.DANCE_SEQS)]
        rows = []
        for path in files:
            with open(path) as f:
                rows.append([[float(x) for x in line.split(",")] for line in f.read().splitlines()])
        return rows

    # (the trees' frames through the one-sequence tracker: no decision near a threshold here either)
    from memotr_amd.data.jpeg import decode_jpeg
    directory = S.split_dir(root, "DanceTrack", "train")
    pixels = [[decode_jpeg(p, "cpu") for p in S.sequence_frames("DanceTrack", os.path.join(directory, seq))]
              for seq in sorted(T.DANCE_SEQS)]
    assert M.single_runs(model, pixels, single)[1] > M.MARGIN
    one = run("one", streams=1)
    monkeypatch.setenv("MEMOTR_SUBMIT_STREAMS", "2")            # what `streams=None` reads
    two = run("two")
    monkeypatch.delenv("MEMOTR_SUBMIT_STREAMS")
    assert sum(len(r) for r in one) > 0
    for a, b in zip(one, two):
        assert [r[:2] for r in a] == [r[:2] for r in b]          # frame, id
        for ra, rb in zip(a, b):
            # x, y, w, h in pixels of the 48 x 80 frames; a width or height is the difference of two corners
            for x, y, size in zip(ra[2:6], rb[2:6], (80, 48, 2 * 80, 2 * 48)):
                assert abs(x - y) <= M.TOL * size
            assert ra[6:] == rb[6:]
    with pytest.raises(ValueError, match="USE_MOTION"):
        S.submit(dict(thresholds, USE_MOTION=True, SUBMIT_DIR=str(tmp_path / "m"), SUBMIT_DATA_SPLIT="train",
                      DATA_ROOT=root), model=model, train_config=train_config, tracker_options=options, streams=2)
    with pytest.raises(ValueError, match="streams"):
        S.submit_streams(0)
