"""CPU: the submit and eval engines (memotr_amd/submit.py, memotr_amd/evaluate.py) on the small dataset trees, with
the small model and the oracle's operator: listings and rank shards, result files against a hand loop of ``track_jpeg``
+ ``mot_lines`` / ``bdd_frame_result``, a PNG frame, the checkpoint sweep with its summary files and states."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import dataset_trees as T
from model_helpers import build_small_memotr, patch_operator

from memotr_amd import evaluate as EV
from memotr_amd import submit as S
from memotr_amd.inference import SequenceTracker
from memotr_amd.results import ResultLog

RAW_SIZE = (96, 160)
THRESHOLDS = dict(DET_SCORE_THRESH=0.0, TRACK_SCORE_THRESH=0.0, RESULT_SCORE_THRESH=0.0, MISS_TOLERANCE=5,
                  USE_MOTION=False)
OPTIONS = dict(raw_size=RAW_SIZE, area_thresh=0)


@pytest.fixture(scope="module")
def root(tmp_path_factory, request):
    request.getfixturevalue("hip_lib"), request.getfixturevalue("clip_lib")
    return T.write_trees(str(tmp_path_factory.mktemp("data")))


def small_model(seed=4):
    torch.manual_seed(seed)
    return build_small_memotr().eval()


def hand_tracker(model, dataset, result_score_thresh=0.0):
    return SequenceTracker(model, dataset_name=dataset, det_score_thresh=0.0, track_score_thresh=0.0,
                           result_score_thresh=result_score_thresh, miss_tolerance=5, use_dab=True, **OPTIONS)


def hand_lines(model, paths, dataset="DanceTrack"):
    t = hand_tracker(model, dataset)
    return [line for idx, result in t.track_jpeg(paths) for line in t.mot_lines(idx, result)]


# ---------------------------------------------------------------------------------------------- listings
def test_split_dirs_frames_and_rank_shards(root):
    assert S.split_dir(root, "DanceTrack", "train") == os.path.join(root, "DanceTrack", "train")
    assert S.split_dir(root, "SportsMOT", "val") == os.path.join(root, "SportsMOT", "val")
    assert S.split_dir(root, "MOT17", "train") == os.path.join(root, "MOT17", "images", "train")
    assert S.split_dir(root, "BDD100K", "train") == os.path.join(root, "BDD100K", "images", "track", "train")
    for dataset, seqs in (("DanceTrack", T.DANCE_SEQS), ("MOT17", T.MOT_SEQS), ("BDD100K", T.BDD_SEQS)):
        directory = S.split_dir(root, dataset, "train")
        names = S.sequence_names(directory)
        assert names == sorted(seqs) and names != list(seqs)                        # sorted, not as written
        for world in (1, 2, 3):
            shards = [S.sequence_names(directory, rank, world) for rank in range(world)]
            assert sorted(sum(shards, [])) == names and sum(len(s) for s in shards) == len(names)
            assert all(s == names[rank::world] for rank, s in enumerate(shards))
        for seq, n in seqs.items():
            frames = S.sequence_frames(dataset, os.path.join(directory, seq))
            assert len(frames) == n and frames == sorted(frames) and all(os.path.isfile(f) for f in frames)
            inside = os.path.join(directory, seq) if dataset == "BDD100K" else os.path.join(directory, seq, "img1")
            assert all(os.path.dirname(f) == inside for f in frames)
    with pytest.raises(ValueError):
        S.sequence_names(S.split_dir(root, "DanceTrack", "train"), 2, 2)


# ---------------------------------------------------------------------------------------------- submit
def test_submit_writes_the_lines_of_the_frame_loop_and_replaces_older_files(root, tmp_path, monkeypatch):
    patch_operator(monkeypatch)
    model = small_model()
    out = tmp_path / "outputs"
    os.makedirs(out / "train")
    with open(out / "train" / "config.yaml", "w") as f:                             # the training run's config
        yaml.dump(dict(DATASET="DanceTrack", USE_DAB=True), f)
    config = dict(THRESHOLDS, SUBMIT_DIR=str(out), SUBMIT_MODEL="unused.pth", SUBMIT_DATA_SPLIT="train", DATA_ROOT=root)
    files = S.submit(config, model=model, tracker_options=OPTIONS)
    assert files == [str(out / "train" / "tracker" / f"{seq}.txt") for seq in sorted(T.DANCE_SEQS)]
    want = {}
    for seq, path in zip(sorted(T.DANCE_SEQS), files):
        frames = S.sequence_frames("DanceTrack", os.path.join(root, "DanceTrack", "train", seq))
        want[seq] = "".join(hand_lines(model, frames))
        with open(path) as f:
            assert f.read() == want[seq] and want[seq].count("\n") >= T.DANCE_SEQS[seq]
    assert want["dancetrack0002"] != want["dancetrack0007"]
    with open(files[0], "a") as f:
        f.write("left over from an older run\n")
    assert S.submit(config, model=model, tracker_options=OPTIONS) == files
    for seq, path in zip(sorted(T.DANCE_SEQS), files):
        with open(path) as f:
            assert f.read() == want[seq]
    with pytest.raises(ValueError, match="DATA_ROOT"):
        S.submit(dict(config, DATA_ROOT=None), model=model)


def test_submit_bdd100k_writes_one_record_per_frame(root, tmp_path, monkeypatch):
    patch_operator(monkeypatch)
    model = small_model()
    train_config = dict(DATASET="BDD100K", USE_DAB=True)
    config = dict(THRESHOLDS, SUBMIT_DIR=str(tmp_path), SUBMIT_MODEL=None, SUBMIT_DATA_SPLIT="train", DATA_ROOT=root)
    files = S.submit(config, model=model, train_config=train_config, tracker_options=OPTIONS)
    assert [os.path.basename(f) for f in files] == [f"{seq}.json" for seq in sorted(T.BDD_SEQS)]
    for seq, path in zip(sorted(T.BDD_SEQS), files):
        frames = S.sequence_frames("BDD100K", os.path.join(S.split_dir(root, "BDD100K", "train"), seq))
        t = hand_tracker(model, "BDD100K")
        want = [SequenceTracker.bdd_frame_result(idx, result, frames[idx]) for idx, result in t.track_jpeg(frames)]
        with open(path) as f:
            got = json.load(f)
        assert got == want and len(got) == T.BDD_SEQS[seq] and all(fr["labels"] for fr in got)
        assert got[1]["videoName"] == seq and got[1]["name"] == os.path.basename(frames[1])
    # no row at all (nothing scores above 2): every frame is there, with an empty list
    files = S.submit(dict(config, RESULT_SCORE_THRESH=2.0), model=model, train_config=train_config,
                     tracker_options=OPTIONS)
    with open(files[0]) as f:
        got = json.load(f)
    assert [fr["frameIndex"] for fr in got] == list(range(T.BDD_SEQS[sorted(T.BDD_SEQS)[0]]))
    assert all(fr["labels"] == [] for fr in got)


def test_a_png_frame_tracks_like_its_pixels(root, tmp_path, monkeypatch):
    from PIL import Image

    from memotr_amd.data import encode_jpeg
    from memotr_amd.data import jpeg as J
    patch_operator(monkeypatch)
    model = small_model()
    img1 = tmp_path / "MOT17" / "images" / "val" / "MOT17-99-SDP" / "img1"
    os.makedirs(img1)
    pixels = []
    for i in range(3):
        px = T.frame_pixels(40 + i)
        if i == 1:
            Image.fromarray(px).save(img1 / f"{i + 1:06d}.png")
            pixels.append(torch.from_numpy(px))
        else:
            data = encode_jpeg(torch.from_numpy(px), quality=90, subsampling="4:2:0")
            (img1 / f"{i + 1:06d}.jpg").write_bytes(bytes(data))
            pixels.append(J.decode_jpeg(data, "cpu"))
    frames = S.sequence_frames("MOT17", str(img1.parent))
    assert [os.path.basename(f) for f in frames] == ["000001.jpg", "000002.png", "000003.jpg"]
    with pytest.raises(J.CorruptJpeg):                     # the JPEG path's Pillow fallback is for JPEG streams only ...
        J.decode_jpeg(frames[1], "cpu")
    log = ResultLog("cpu")                                 # ... so submit decodes such a sequence itself
    path = S.submit_sequence(lambda: hand_tracker(model, "MOT17"), "MOT17", str(img1.parent), str(tmp_path / "out"), log)
    assert path == str(tmp_path / "out" / "tracker" / "MOT17-99-SDP.txt")
    t = hand_tracker(model, "MOT17")
    want = [line for idx, result in t.track(pixels) for line in t.mot_lines(idx, result)]
    with open(path) as f:
        assert f.read() == "".join(want) and len(want) >= 3


# ---------------------------------------------------------------------------------------------- evaluate
def reference_reader(metric_path):
    """eval_engine.py:117-123 of the reference, restated."""
    with open(metric_path) as f:
        metric_names = f.readline()[:-1].split(" ")
        metric_values = f.readline()[:-1].split(" ")
    return {n: float(v) for n, v in zip(metric_names, metric_values)}


def test_evaluate_continue_sweeps_the_checkpoints_once(root, tmp_path, monkeypatch):
    from memotr_amd.evaluation import evaluate_files, summary
    from memotr_amd.models.utils import save_checkpoint
    patch_operator(monkeypatch)
    eval_dir = tmp_path / "outputs"
    os.makedirs(eval_dir)
    models = [small_model(seed) for seed in (4, 5)]
    for i, m in enumerate(models):
        save_checkpoint(m, str(eval_dir / f"checkpoint_{i}.pth"), states={"start_epoch": i + 1})
    seqmap = os.path.join(root, "DanceTrack", "train_seqmap.txt")
    with open(seqmap, "w") as f:
        f.write("name\n" + "".join(seq + "\n" for seq in sorted(T.DANCE_SEQS)))
    config = dict(THRESHOLDS, EVAL_DIR=str(eval_dir), EVAL_MODE="continue", EVAL_MODEL=None, EVAL_DATA_SPLIT="train",
                  DATA_ROOT=root, DATASET="DanceTrack")
    calls, seen, real = [], [], EV.submit
    monkeypatch.setattr(EV, "submit", lambda *a, **k: (calls.append(a[0]["SUBMIT_MODEL"]), real(*a, **k))[1])
    kwargs = dict(model=small_model(9), train_config=dict(DATASET="DanceTrack", USE_DAB=True), tracker_options=OPTIONS)
    got = EV.evaluate(config, on_metrics=lambda i, m: seen.append((i, m)), **kwargs)
    assert calls == ["checkpoint_0.pth", "checkpoint_1.pth"] and sorted(got) == [0, 1] and seen == sorted(got.items())
    gt_root = os.path.join(root, "DanceTrack", "train")
    for i, m in enumerate(models):
        tracker_dir = eval_dir / "train" / f"checkpoint_{i}_tracker"
        for seq in T.DANCE_SEQS:                                 # the checkpoint's weights made these files
            with open(tracker_dir / f"{seq}.txt") as f:
                assert f.read() == "".join(hand_lines(m, S.sequence_frames("DanceTrack", os.path.join(gt_root, seq))))
        want = summary(evaluate_files(gt_root, str(tracker_dir), seqmap)["COMBINED_SEQ"])
        assert got[i] == want and "HOTA" in want and want["Dets"] > 0
        assert reference_reader(tracker_dir / "pedestrian_summary.txt") == want
    assert not os.path.exists(eval_dir / "train" / "tracker")
    with open(eval_dir / "train" / "eval_states.yaml") as f:
        assert yaml.safe_load(f) == {"NEXT_INDEX": 2}
    with open(eval_dir / "train" / "metrics.jsonl") as f:
        lines = [json.loads(line) for line in f]
    assert [(r["index"], r["checkpoint"]) for r in lines] == [(0, "checkpoint_0.pth"), (1, "checkpoint_1.pth")]
    assert lines[1]["metrics"] == got[1]
    # a second call finds nothing to do -- neither from the states file nor, without it, from the summary files
    assert EV.evaluate(config, **kwargs) == {} and len(calls) == 2
    os.remove(eval_dir / "train" / "eval_states.yaml")
    assert EV.evaluate(config, **kwargs) == {} and len(calls) == 2
    with open(eval_dir / "train" / "eval_states.yaml") as f:
        assert yaml.safe_load(f) == {"NEXT_INDEX": 2}


def test_evaluate_rejects_what_the_reference_rejects(root, tmp_path):
    base = dict(THRESHOLDS, EVAL_DIR=str(tmp_path), EVAL_DATA_SPLIT="train", DATA_ROOT=root, DATASET="DanceTrack")
    with pytest.raises(ValueError, match="EVAL_MODEL"):
        EV.evaluate(dict(base, EVAL_MODE="specific", EVAL_MODEL=None))
    with pytest.raises(ValueError, match="not supported"):
        EV.evaluate(dict(base, EVAL_MODE="sometimes"))
    with pytest.raises(NotImplementedError, match="BDD100K"):
        EV.evaluate(dict(base, EVAL_MODE="specific", EVAL_MODEL="checkpoint_0.pth", DATASET="BDD100K"),
                    model=torch.nn.Linear(1, 1), train_config=dict(DATASET="BDD100K", USE_DAB=True))


def test_eval_model_scores_bdd100k_against_a_ground_truth_folder(root, tmp_path, monkeypatch):
    from memotr_amd.evaluation_bdd100k import bdd_summary, evaluate_bdd_files
    from memotr_amd.models.utils import save_checkpoint
    patch_operator(monkeypatch)
    model = small_model()
    save_checkpoint(model, str(tmp_path / "checkpoint_3.pth"))
    gt_dir = tmp_path / "gt"
    os.makedirs(gt_dir)
    for seq, n in T.BDD_SEQS.items():                            # ground truth in the evaluator's layout, from the trees' boxes
        frames = []
        for t in range(1, n + 1):
            labels = [{"id": str(i), "category": "pedestrian", "box2d": {"x1": x, "y1": y, "x2": x + w, "y2": y + h}}
                      for _, i, x, y, w, h in T.boxes_of(seq, t)]
            frames.append({"name": f"{seq}-{t:07d}.jpg", "videoName": seq, "index": t - 1, "labels": labels})
        with open(gt_dir / f"{seq}.json", "w") as f:
            json.dump(frames, f)
    config = dict(THRESHOLDS, EVAL_DIR=str(tmp_path), EVAL_MODE="specific", EVAL_MODEL="checkpoint_3.pth",
                  EVAL_DATA_SPLIT="train", DATA_ROOT=root, DATASET="BDD100K", EVAL_GT_DIR=str(gt_dir))
    got = EV.evaluate(config, model=small_model(7), train_config=dict(DATASET="BDD100K", USE_DAB=True),
                      tracker_options=OPTIONS)
    tracker_dir = tmp_path / "train" / "checkpoint_3_tracker"
    want = bdd_summary(evaluate_bdd_files(str(gt_dir), str(tracker_dir)))
    assert got == want and "pedestrian" in want
    for key, fields in want.items():
        assert reference_reader(tracker_dir / f"{key}_summary.txt") == fields, key
    with open(tmp_path / "train" / "metrics.jsonl") as f:
        (line,) = [json.loads(x) for x in f]
    assert line["index"] is None and line["checkpoint"] == "checkpoint_3.pth"
    assert np.isfinite(want["pedestrian"]["Dets"])
