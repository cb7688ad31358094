"""CPU: ``SweepTracker`` (memotr_amd/inference_sweep.py) and the sweep engine (memotr_amd/sweep.py) with the small model
and the oracle's operator.  One sequence under the four settings of tests/sweep_cases.py in one pass against a fresh
``SequenceTracker`` per setting and sequence: the same ids, labels and reported rows, boxes and scores to 1e-4 (no decision
score of the one-sequence runs may lie within 1e-3 of its threshold); ``sweep()`` on the dataset trees writes, per
setting, the files ``submit(streams=1)`` writes under that setting and the metrics ``evaluate`` gives for them."""
import json
import os

import pytest

import dataset_trees as T
import multi_track_cases as M
import sweep_cases as C
from model_helpers import patch_operator

from memotr_amd import submit as S
from memotr_amd import sweep as W
from memotr_amd.inference_sweep import SweepTracker
from memotr_amd.results import BankResultLog


@pytest.fixture(scope="module")
def scenario():
    """The model, the sequences and every setting's one-sequence runs (computed once, read by every test)."""
    mp = pytest.MonkeyPatch()
    patch_operator(mp)
    try:
        model, seqs = M.scenario_model(64), M.sequences()
        want, margin = C.single_runs(model, seqs)
    finally:
        mp.undo()
    return model, seqs, want, margin


def test_the_scenario_decides_nothing_near_a_threshold(scenario):
    _, _, want, margin = scenario
    assert margin > M.MARGIN, f"a decision score lies {margin} from its threshold: choose other settings"
    assert all(M.scenario_is_eventful(runs) for runs in want)
    assert C.some_frame_differs(want)
    assert len({tuple(len(r.ids) for seq in runs for r in seq) for runs in want}) == len(want)


def test_every_stream_tracks_what_a_tracker_with_its_setting_tracks(scenario, monkeypatch):
    patch_operator(monkeypatch)
    model, seqs, want, margin = scenario
    assert margin > M.MARGIN
    tracker = SweepTracker(model, C.SETTINGS, cap=32, **C.OPTIONS)
    got = C.sweep_runs(tracker, seqs)                        # (a new sequence starts every stream afresh)
    for k in range(len(C.SETTINGS)):
        M.assert_equivalent(want[k], got[k])
    assert C.some_frame_differs(got)                         # not every stream under setting 0
    assert tracker.bank.n_streams == len(C.SETTINGS)


def test_logged_tracking_gives_the_lines_of_track_and_a_small_bank_grows(scenario, monkeypatch):
    patch_operator(monkeypatch)
    model, seqs, want, margin = scenario
    assert margin > M.MARGIN
    busiest = max(range(len(seqs)), key=lambda s: max(len(r.ids) for runs in want for r in runs[s]))
    frames = seqs[busiest]
    tracker = SweepTracker(model, C.SETTINGS, cap=16, **C.OPTIONS)
    got = [[r for r in results] for results in zip(*[results for _, results in tracker.track(frames)])]
    assert int(tracker.bank.counters[:, 0].max()) > 8 and tracker.bank.cap > 16
    for k in range(len(C.SETTINGS)):
        M.assert_equivalent([want[k][busiest]], [got[k]])
    log = BankResultLog("cpu", capacity=8)
    assert SweepTracker(model, C.SETTINGS, cap=32, **C.OPTIONS).track_logged(frames, log, first_setting=3) == len(frames)
    for k, runs in enumerate(got):
        lines = [line for idx, r in enumerate(runs) for line in tracker.mot_lines(idx, r)]
        assert log.mot_lines(3 + k) == lines and lines
    assert log.mot_lines(0) == []
    # without room to grow into, the end of the sequence names the setting whose births found no slot
    full = SweepTracker(model, [dict(C.SETTINGS[0]), dict(C.SETTINGS[0], det_score_thresh=0.2)], cap=16, **C.OPTIONS)
    monkeypatch.setattr(full, "_watch_counts", lambda: None)
    with pytest.raises(RuntimeError, match=r"setting 1 \{.*\} dropped \d+ births"):
        list(full.track(frames))


def test_from_config_and_argument_errors(scenario):
    model = scenario[0]
    config = dict(DATASET="MOT17", USE_DAB=True, DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.4, RESULT_SCORE_THRESH=0.3,
                  MISS_TOLERANCE=15)
    tracker = SweepTracker.from_config(model, config, [dict(det_score_thresh=0.7), dict(miss_tolerance=30), {}], cap=16)
    assert tracker.dataset_name == "MOT17" and tracker.n_streams == 3
    assert [s["det_score_thresh"] for s in tracker.settings] == [0.7, 0.5, 0.5]
    assert [s["miss_tolerance"] for s in tracker.settings] == [15, 30, 15]
    assert tracker.thresholds.track.tolist() == pytest.approx([0.4] * 3) and tracker.thresholds.area.tolist() == [100] * 3
    with pytest.raises(ValueError, match="USE_MOTION"):
        SweepTracker(model, C.SETTINGS, use_motion=True)
    with pytest.raises(ValueError, match="USE_MOTION"):
        SweepTracker.from_config(model, dict(config, USE_MOTION=True), C.SETTINGS)
    with pytest.raises(ValueError, match="at least one setting"):
        SweepTracker(model, [])
    with pytest.raises(ValueError, match="lacks"):
        SweepTracker(model, [dict(det_score_thresh=0.5)])
    with pytest.raises(ValueError, match="one sequence"):
        SweepTracker(model, C.SETTINGS, cap=16, **C.OPTIONS).step_raw([M.sequences()[0][0]] * 2)
    with pytest.raises(NotImplementedError, match="one sequence"):
        SweepTracker(model, C.SETTINGS, cap=16, **C.OPTIONS).track_many([])


# ---------------------------------------------------------------------------------------------- the engine
def test_the_grid_and_its_command_line_form():
    grid = W.threshold_grid(DET_SCORE_THRESH=[0.5, 0.6, 0.7], TRACK_SCORE_THRESH=[0.5], MISS_TOLERANCE=[15, 30])
    assert len(grid) == 6 and grid[0] == dict(det_score_thresh=0.5, track_score_thresh=0.5, miss_tolerance=15)
    assert grid[1]["miss_tolerance"] == 30 and grid[2]["det_score_thresh"] == 0.6
    assert all("result_score_thresh" not in s for s in grid)
    assert W.parse_grid(["det=0.5,0.6,0.7", "track=0.5", "miss=15,30"]) == grid
    assert W.parse_grid(["result=0.25"]) == [dict(result_score_thresh=0.25)]
    assert isinstance(W.parse_grid(["miss=15"])[0]["miss_tolerance"], int)
    for bad in (["det"], ["update=0.5"], ["det="], ["det=0.5", "det=0.6"], ["miss=1.5"], ["det=high"]):
        with pytest.raises(ValueError, match="--grid"):
            W.parse_grid(bad)
    with pytest.raises(ValueError, match="unknown keys"):
        W.threshold_grid(UPDATE_THRESH=[0.5])
    with pytest.raises(ValueError, match="no value"):
        W.threshold_grid(DET_SCORE_THRESH=[])


def test_the_engine_refuses_bdd100k_and_a_config_without_its_keys(tmp_path):
    base = dict(EVAL_DIR=str(tmp_path), EVAL_MODEL=None, EVAL_DATA_SPLIT="train", DATA_ROOT=str(tmp_path),
                DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.5, RESULT_SCORE_THRESH=0.5, MISS_TOLERANCE=5)
    with pytest.raises(NotImplementedError, match="scores MOT-format datasets only"):
        W.sweep(dict(base, DATASET="BDD100K"), [{}], train_config=dict(DATASET="BDD100K", USE_DAB=True))
    with pytest.raises(ValueError, match="EVAL_DIR"):
        W.sweep(dict(base, EVAL_DIR=None), [{}], train_config=dict(DATASET="DanceTrack", USE_DAB=True))
    with pytest.raises(ValueError, match="EVAL_MODEL"):
        W.sweep(dict(base, DATASET="DanceTrack"), [{}], train_config=dict(DATASET="DanceTrack", USE_DAB=True))


def test_sweep_writes_the_files_of_submit_and_the_metrics_of_evaluate_per_setting(scenario, tmp_path, monkeypatch,
                                                                                   request):
    from memotr_amd.data.jpeg import decode_jpeg
    from memotr_amd.evaluation import evaluate_files, summary
    request.getfixturevalue("hip_lib"), request.getfixturevalue("clip_lib")
    patch_operator(monkeypatch)
    model = scenario[0]
    root = T.write_trees(str(tmp_path / "data"), only=("DanceTrack",))
    seqmap = os.path.join(root, "DanceTrack", "train_seqmap.txt")
    with open(seqmap, "w") as f:
        f.write("name\n" + "".join(seq + "\n" for seq in sorted(T.DANCE_SEQS)))
    train_config = dict(DATASET="DanceTrack", USE_DAB=True)
    # (thresholds chosen for the trees' frames as the scenario's are for its own: the margin is asserted below)
    thresholds = dict(DET_SCORE_THRESH=0.7, TRACK_SCORE_THRESH=0.45, RESULT_SCORE_THRESH=0.6, MISS_TOLERANCE=2,
                      USE_MOTION=False)
    settings = [dict(), dict(det_score_thresh=0.6, result_score_thresh=0.5, miss_tolerance=1), dict(track_score_thresh=0.5)]
    options = dict(raw_size=M.RAW_SIZE, area_thresh=10)
    full = [dict(dict(det_score_thresh=0.7, track_score_thresh=0.45, result_score_thresh=0.6, miss_tolerance=2), **part)
            for part in settings]
    directory = S.split_dir(root, "DanceTrack", "train")
    pixels = [[decode_jpeg(p, "cpu") for p in S.sequence_frames("DanceTrack", os.path.join(directory, seq))]
              for seq in sorted(T.DANCE_SEQS)]
    for s in full:
        assert M.single_runs(model, pixels, dict(C.OPTIONS, **s))[1] > M.MARGIN, s

    def rows_of(path):
        with open(path) as f:
            return [[float(x) for x in line.split(",")] for line in f.read().splitlines()]

    eval_dir = tmp_path / "outputs"
    config = dict(thresholds, EVAL_DIR=str(eval_dir), EVAL_MODEL=None, EVAL_DATA_SPLIT="train", DATA_ROOT=root,
                  DATASET="DanceTrack")
    table = W.sweep(config, settings, model=model, train_config=train_config, tracker_options=dict(options, cap=32),
                    max_streams=2)                               # three settings: a pass of two and a pass of one
    assert [row["index"] for row in table] == [0, 1, 2] and [row["setting"] for row in table] == full
    with open(eval_dir / "train" / "sweep.jsonl") as f:
        assert [json.loads(line) for line in f] == table
    total = []
    for k, s in enumerate(full):
        submit_config = dict(thresholds, SUBMIT_DIR=str(tmp_path / f"submit{k}"), SUBMIT_MODEL=None,
                             SUBMIT_DATA_SPLIT="train", DATA_ROOT=root,
                             **{name: s[key] for key, name in W.CONFIG_KEYS.items()})
        files = S.submit(submit_config, model=model, train_config=train_config, tracker_options=options, streams=1)
        tracker_dir = eval_dir / "train" / "sweep" / str(k) / "tracker"
        assert sorted(os.listdir(tracker_dir)) == sorted([os.path.basename(p) for p in files] + ["pedestrian_summary.txt"])
        n = 0
        for path in files:
            a, b = rows_of(path), rows_of(tracker_dir / os.path.basename(path))
            assert [r[:2] for r in a] == [r[:2] for r in b]          # frame, id
            for ra, rb in zip(a, b):
                # x, y, w, h in pixels of the 48 x 80 frames; a width or height is the difference of two corners
                for x, y, size in zip(ra[2:6], rb[2:6], (80, 48, 2 * 80, 2 * 48)):
                    assert abs(x - y) <= M.TOL * size
                assert ra[6:] == rb[6:]
            n += len(a)
        total.append(n)
        want = summary(evaluate_files(directory, str(tracker_dir), seqmap)["COMBINED_SEQ"])
        assert table[k]["metrics"] == want and {"HOTA", "MOTA", "IDF1"} <= set(want)
    assert min(total) > 0 and len(set(total)) > 1                # the settings do not write the same rows
    # the rows after the offline pass: the files of the filled log
    W.sweep(dict(config, EVAL_DIR=str(tmp_path / "filled")), settings[:1], model=model, train_config=train_config,
            tracker_options=dict(options, cap=32), postprocess=dict(max_gap=2, min_length=2))
    assert os.path.exists(tmp_path / "filled" / "train" / "sweep" / "0" / "tracker" / "dancetrack0002.txt")
