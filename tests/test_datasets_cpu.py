"""The clip datasets (memotr_amd/data/datasets.py) against the reference's own classes (tests/golden/datasets.npz,
written by tests/golden/gen_golden_datasets.py on the trees of tests/dataset_trees.py), their rejections, and the data
config keys.  No pixels are decoded here: the images are empty files."""
import os
import random

import numpy as np
import pytest
import torch

import dataset_trees as trees
from conftest import load_golden

from memotr_amd import configs
from memotr_amd.data import datasets as D

FIELDS = ("boxes", "ids", "labels", "areas")


def touch(path, index):
    open(path, "wb").close()


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return trees.write_trees(str(tmp_path_factory.mktemp("clip_trees")), write_image=touch)


@pytest.fixture(scope="module")
def golden():
    return load_golden("datasets")


def rel(root, path):
    return os.path.relpath(path, root).replace(os.sep, "/")


def assert_info(info, g, prefix):
    for field in FIELDS:
        want = g[f"{prefix}::{field}"]
        got = info[field].numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (prefix, field, got.dtype, want.dtype)
        assert np.array_equal(got, want), (prefix, field)


@pytest.mark.parametrize("key", ["dance", "bdd"])
def test_sequence_datasets_equal_the_reference(root, golden, key):
    config = dict(trees.DANCE_CONFIG if key == "dance" else trees.BDD_CONFIG, DATA_ROOT=root)
    ds = D.build_dataset(config)
    assert isinstance(ds, D.DanceTrackDataset if key == "dance" else D.BDD100KDataset)
    for epoch in trees.epochs_of(config):
        ds.set_epoch(epoch)
        assert ds.sample_length == int(golden[f"{key}::epoch{epoch}::length"])
        assert [v for v, _ in ds.entries] == golden[f"{key}::epoch{epoch}::begin_vid"].tolist()
        assert [t for _, t in ds.entries] == golden[f"{key}::epoch{epoch}::begin_t"].tolist()
        assert len(ds) == len(ds.entries)
        for seed in trees.SEEDS:
            rng = random.Random(seed)               # == the global generator after random.seed(seed)
            want = golden[f"{key}::epoch{epoch}::seed{seed}::frames"]
            for k, (vid, _) in enumerate(ds.entries):
                sample = ds.sample(k, rng)
                assert [rel(root, p) for p in sample.paths] == [rel(root, ds.frame_path(vid, int(t))) for t in want[k]]
                assert not sample.static and len(sample.infos) == ds.sample_length
                assert sample.overflow_bbox == (key == "bdd")
                for t, info in zip(want[k], sample.infos):
                    assert_info(info, golden, f"{key}::info::{vid}::{int(t)}")
    checked = 0
    for name in golden:
        if name.startswith(f"{key}::info::") and name.endswith("::ids"):
            _, _, vid, t, _ = name.split("::")
            assert_info(ds.frame_info(vid, int(t)), golden, f"{key}::info::{vid}::{t}")
            checked += 1
    assert checked >= 10
    if key == "dance":
        assert list(ds.vid_idx) == golden["dance::vids"].tolist() == sorted(trees.DANCE_SEQS)
        assert ds.frame_path("dancetrack0002", 3).endswith(os.path.join("img1", "00000003.jpg"))
    else:
        vid, t = trees.BDD_EMPTY                     # the reference's fake box for a frame without boxes
        fake = ds.frame_info(vid, t)
        assert fake["boxes"].tolist() == [[0.5, 0.5, 1.0, 1.0]] and fake["ids"].tolist() == [0]
        assert fake["labels"].tolist() == [0] and fake["areas"].tolist() == [0.0]


def test_mot17_and_crowdhuman_equal_the_reference(root, golden):
    config = dict(trees.MOT_CONFIG, DATA_ROOT=root)
    ds = D.build_dataset(config)
    assert isinstance(ds, D.MOT17Dataset) and sorted(ds.mot17_gts) == ["MOT17-02-SDP", "MOT17-04-SDP"]
    frames = golden["mot::frames"].tolist()
    for epoch in trees.epochs_of(config):
        ds.set_epoch(epoch)
        assert ds.sample_length == int(golden[f"mot::epoch{epoch}::length"])
        assert [rel(root, ds.frame_path(*e)) for e in ds.entries] == golden[f"mot::epoch{epoch}::begin"].tolist()
        for seed in trees.SEEDS:
            rng = random.Random(seed)
            want = golden[f"mot::epoch{epoch}::seed{seed}::paths"]
            for k, entry in enumerate(ds.entries):
                sample = ds.sample(k, rng)
                paths = [rel(root, p) for p in sample.paths]
                assert paths == want[k].tolist()
                assert sample.static == (entry[0] == "CrowdHuman") and sample.overflow_bbox
                for p, info in zip(paths, sample.infos):
                    assert_info(info, golden, f"mot::info::{frames.index(p)}")
    ds.set_epoch(0)
    assert all(e[0] == "CrowdHuman" for e in ds.entries) and len(ds) == 3       # MOT17 joins at epoch 1
    empty = ds.frame_info("MOT17", *trees.MOT_NO_GT)                             # a frame without a gt file
    assert empty["boxes"].shape == (0, 4) and empty["areas"].dtype == torch.float32
    plan = ds.sample_plan(48, 80, random.Random(0), np.random.RandomState(0), True)
    assert plan.shift is not None and all(1 <= abs(v) <= 50 for v in plan.shift)
    assert ds.sample_plan(48, 80, random.Random(0), np.random.RandomState(0), False).shift is None
    without = D.build_dataset(dict(config, USE_CROWDHUMAN=None))
    without.set_epoch(1)
    assert all(e[0] == "MOT17" for e in without.entries) and len(without) == 9
    without.set_epoch(0)
    assert len(without) == 0


def test_datasets_are_told_apart_by_structure_not_by_path_substrings(tmp_path, golden):
    root = trees.write_trees(str(tmp_path / "CrowdHuman_MOT17_MOTSynth"), write_image=touch, only=("MOT17",))
    ds = D.build_dataset(dict(trees.MOT_CONFIG, DATA_ROOT=root))
    ds.set_epoch(1)
    rng = random.Random(0)
    got = [[rel(root, p) for p in ds.sample(k, rng).paths] for k in range(len(ds))]
    assert got == golden["mot::epoch1::seed0::paths"].tolist()
    assert ds.sample(5, rng).infos[0]["ids"].max() < 100000


def test_the_plans_follow_the_reference_transform_settings(root):
    def plans(ds, n=200):
        return [ds.sample_plan(1080, 1920, random.Random(s), np.random.RandomState(s), False) for s in range(n)]

    bdd = plans(D.build_dataset(dict(trees.BDD_CONFIG, DATA_ROOT=root)))
    capped = 1333 * 1080 // 1920                     # max_size = 1333 holds the long side: the short one is 749 at most
    assert {p.final[0] for p in bdd if p.first is None} == {s for s in D.COCO_SCALES if s < capped} | {capped}
    assert not any(p.reverse for p in bdd)
    assert {p.first[0] for p in bdd if p.first is not None} == {400, 500, 600}
    assert max(max(p.final) for p in bdd) <= 1333 and max(p.final[0] for p in bdd) > 700
    dance = plans(D.build_dataset(dict(trees.DANCE_CONFIG, DATA_ROOT=root)))
    assert {p.first[0] for p in dance if p.first is not None} == {800, 1000, 1200}
    assert 40 < sum(p.reverse for p in dance) < 160                             # REVERSE_CLIP = 0.5
    assert {p.final[0] for p in dance if p.first is None} <= set(D.SCALES) and max(max(p.final) for p in dance) <= 1536


# ------------------------------------------------------------------------------------------------- rejections
def rewrite(path, text):
    with open(path, "w") as f:
        f.write(text)


def test_malformed_gt_lines_name_file_and_line(tmp_path):
    root = trees.write_trees(str(tmp_path), write_image=touch)
    gt = os.path.join(root, "DanceTrack", "train", "dancetrack0002", "gt", "gt.txt")
    good = open(gt).read()
    rewrite(gt, good + "9,1,2.0,3.0,x,5.0,1,1,1\n")
    with pytest.raises(ValueError, match=r"gt\.txt:%d: " % (good.count("\n") + 1)):
        D.build_dataset(dict(trees.DANCE_CONFIG, DATA_ROOT=root))
    rewrite(gt, "1,1,2.0,3.0,4.0,5.0,1,0,1\n" + good)
    with pytest.raises(ValueError, match=r"gt\.txt:1: the three check digits"):
        D.build_dataset(dict(trees.DANCE_CONFIG, DATA_ROOT=root))
    rewrite(gt, "1,1,2.0,3.0\n" + good)
    with pytest.raises(ValueError, match=r"gt\.txt:1: expected 9 fields"):
        D.build_dataset(dict(trees.DANCE_CONFIG, DATA_ROOT=root))
    rewrite(gt, good)
    D.build_dataset(dict(trees.DANCE_CONFIG, DATA_ROOT=root))

    mot = os.path.join(root, "MOT17", "gts", "train", "MOT17-02-SDP", "img1", "000002.txt")
    mot_good = open(mot).read()
    rewrite(mot, mot_good + "0 1 2 3 4 5\n")
    with pytest.raises(ValueError, match=r"000002\.txt:\d+: expected 7 fields"):
        D.build_dataset(dict(trees.MOT_CONFIG, DATA_ROOT=root))
    rewrite(mot, mot_good)
    ch = os.path.join(root, "CrowdHuman", "gts", "val", trees.CROWDHUMAN[0] + ".txt")
    rewrite(ch, "0 1 2.5 3 4 5\n")
    with pytest.raises(ValueError, match=r"\.txt:1: not a number"):
        D.build_dataset(dict(trees.MOT_CONFIG, DATA_ROOT=root, USE_CROWDHUMAN=True))
    vid = "b1c81faa-3df17267"
    bdd = os.path.join(root, "BDD100K", "filter_labels", "track", "train", vid, f"{vid}-0000002.txt")
    rewrite(bdd, "1 1 2.0 3.0 4.0\n")
    with pytest.raises(ValueError, match=r"-0000002\.txt:1: expected 6 fields"):
        D.build_dataset(dict(trees.BDD_CONFIG, DATA_ROOT=root))


def test_unsupported_settings_raise_as_the_reference_does(root):
    with pytest.raises(NotImplementedError, match="USE_MOTSYNTH"):
        D.build_dataset(dict(trees.MOT_CONFIG, DATA_ROOT=root, USE_MOTSYNTH=True))
    with pytest.raises(ValueError, match="is not supported"):
        D.build_dataset(dict(trees.DANCE_CONFIG, DATA_ROOT=root, DATASET="KITTI"))
    with pytest.raises(ValueError):
        D.build_dataset(dict(trees.DANCE_CONFIG, DATA_ROOT=root), split="test")
    for config, error in ((trees.DANCE_CONFIG, ValueError), (trees.BDD_CONFIG, ValueError),
                          (trees.MOT_CONFIG, NotImplementedError)):
        ds = D.build_dataset(dict(config, DATA_ROOT=root, SAMPLE_MODES=["fixed_interval"]))
        ds.set_epoch(1)
        with pytest.raises(error, match="fixed_interval"):
            ds.sample(len(ds) - 1, random.Random(0))


# ------------------------------------------------------------------------------------------------- config keys
def test_data_config_holds_the_shipped_data_keys():
    dance = configs.data_config("DanceTrack", DATA_ROOT="/data")
    assert dance == dict(DATASET="DanceTrack", DATA_ROOT="/data", NUM_WORKERS=4, COCO_SIZE=False, OVERFLOW_BBOX=False,
                         REVERSE_CLIP=0.0, SAMPLE_STEPS=[6, 10, 14], SAMPLE_LENGTHS=[2, 3, 4, 5],
                         SAMPLE_MODES=["random_interval"], SAMPLE_INTERVALS=[10], USE_CROWDHUMAN=None,
                         USE_MOTSYNTH=None, MOTSYNTH_RATE=None)
    sports = configs.data_config("SportsMOT")
    assert sports["SAMPLE_STEPS"] == [10, 16, 22] and sports["DATASET"] == "SportsMOT" and sports["DATA_ROOT"] is None
    assert {k: v for k, v in sports.items() if k not in ("SAMPLE_STEPS", "DATASET", "DATA_ROOT")} == \
        {k: v for k, v in dance.items() if k not in ("SAMPLE_STEPS", "DATASET", "DATA_ROOT")}
    mot = configs.data_config("MOT17")
    assert mot["SAMPLE_STEPS"] == [60, 100] and mot["SAMPLE_LENGTHS"] == [2, 3, 4] and mot["SAMPLE_MOT17_JOIN"] == 0
    assert mot["USE_CROWDHUMAN"] is True and not mot["USE_MOTSYNTH"] and mot["COCO_SIZE"] and mot["OVERFLOW_BBOX"]
    assert mot["SAMPLE_INTERVALS"] == [10] and mot["REVERSE_CLIP"] == 0.0
    bdd = configs.data_config("BDD100K")
    assert bdd == dict(DATASET="BDD100K", DATA_ROOT=None, NUM_WORKERS=8, SAMPLE_STEPS=[6, 10],
                       SAMPLE_LENGTHS=[2, 3, 4], SAMPLE_MODES=["random_interval"], SAMPLE_INTERVALS=[4, 4, 4])
    configs.data_config("MOT17")["SAMPLE_STEPS"].append(1)                      # a copy each time
    assert configs.data_config("MOT17")["SAMPLE_STEPS"] == [60, 100]
    with pytest.raises(ValueError, match="KITTI"):
        configs.data_config("KITTI")
    merged = dict(configs.mot17_config(), **configs.data_config("MOT17", DATA_ROOT="/d"))
    assert merged["DATASET"] == "MOT17" and merged["SAMPLE_LENGTHS"] == [2, 3, 4] and merged["HIDDEN_DIM"] == 256


DANCETRACK_CONFIG = dict(
    MODE="train", VISUALIZE=False, AVAILABLE_GPUS="0,1,2,3,4,5,6,7", DEVICE="cuda", USE_DISTRIBUTED=False,
    USE_CHECKPOINT=False, CHECKPOINT_LEVEL=2, DATASET="DanceTrack", BATCH_SIZE=1, ACCUMULATION_STEPS=1,
    BACKBONE="resnet50", HIDDEN_DIM=256, FFN_DIM=2048, NUM_FEATURE_LEVELS=4, NUM_HEADS=8, NUM_ENC_POINTS=4,
    NUM_DEC_POINTS=4, NUM_ENC_LAYERS=6, NUM_DEC_LAYERS=6, MERGE_DET_TRACK_LAYER=1, ACTIVATION="ReLU",
    RETURN_INTER_DEC=True, EXTRA_TRACK_ATTN=False, AUX_LOSS=True, USE_DAB=True, UPDATE_THRESH=0.5,
    LONG_MEMORY_LAMBDA=0.01, SAMPLE_STEPS=[6, 10, 14], SAMPLE_LENGTHS=[2, 3, 4, 5], SEED=42, EPOCHS=20,
    ONLY_TRAIN_QUERY_UPDATER_AFTER=20, DROPOUT=0.0, NUM_DET_QUERIES=300, TP_DROP_RATE=0.0, FP_INSERT_RATE=0.0,
    LR=2.0e-4, LR_BACKBONE=2.0e-5, LR_POINTS=1.0e-5, WEIGHT_DECAY=0.0005, CLIP_MAX_NORM=0.1,
    LR_SCHEDULER="MultiStep", LR_DROP_RATE=0.1, LR_DROP_MILESTONES=[12], MATCH_COST_CLASS=2, MATCH_COST_BBOX=5,
    MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5, LOSS_WEIGHT_GIOU=2,
    AUX_LOSS_WEIGHT=[1.0, 1.0, 1.0, 1.0, 1.0], DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.5, RESULT_SCORE_THRESH=0.5,
    MISS_TOLERANCE=30, USE_MOTION=False, MOTION_MIN_LENGTH=3, MOTION_MAX_LENGTH=5, MOTION_LAMBDA=0.5)


def test_the_three_model_configs_return_what_they_returned():
    assert configs.dancetrack_config() == DANCETRACK_CONFIG
    assert configs.mot17_config() == dict(DANCETRACK_CONFIG, DATASET="MOT17", SAMPLE_LENGTHS=[2, 3, 4],
                                          MISS_TOLERANCE=15)
    assert configs.bdd100k_config() == dict(DANCETRACK_CONFIG, DATASET="BDD100K", SAMPLE_LENGTHS=[2, 3, 4],
                                            MISS_TOLERANCE=10)
    assert configs.dancetrack_config(EPOCHS=3, RESUME=None) == dict(DANCETRACK_CONFIG, EPOCHS=3, RESUME=None)


def test_load_yaml_reads_a_reference_format_file(tmp_path):
    pytest.importorskip("yaml")
    path = tmp_path / "train.yaml"
    path.write_text("# a comment\nDATASET: MOT17\nUSE_MOTSYNTH:\nUSE_CROWDHUMAN: True\nDATA_ROOT: /data/sets\n"
                    "SAMPLE_STEPS: [60, 100]\nSAMPLE_MODES: [random_interval]\nREVERSE_CLIP: 0.0\nLR: 2.0e-4\n"
                    "COCO_SIZE: False\nSEED: 42\n")
    cfg = configs.load_yaml(str(path))
    assert cfg == dict(DATASET="MOT17", USE_MOTSYNTH=None, USE_CROWDHUMAN=True, DATA_ROOT="/data/sets",
                       SAMPLE_STEPS=[60, 100], SAMPLE_MODES=["random_interval"], REVERSE_CLIP=0.0, LR=2.0e-4,
                       COCO_SIZE=False, SEED=42)
    (tmp_path / "list.yaml").write_text("- 1\n- 2\n")
    with pytest.raises(ValueError, match="one mapping"):
        configs.load_yaml(str(tmp_path / "list.yaml"))
