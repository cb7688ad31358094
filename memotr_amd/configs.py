"""Model / training hyper-parameters of the reference's shipped configs, as python dicts.

Values transcribed from configs/train_dancetrack.yaml, train_mot17.yaml and train_bdd100k.yaml of the
reference (flat UPPER_CASE keys, read by the ``build(config)`` functions exactly like the reference's).
The three model functions keep only the keys the per-frame path and the train step read; ``data_config`` adds the
data-pipeline keys (``data/datasets.py``, ``data/loader.py``) of the four shipped training configs, and ``load_yaml``
reads a user's file in the reference's format.  ``builtin_config(name)`` is a whole shipped file, every key of it, for
the command line (``main.py``): what ``--config-path dancetrack`` stands for.
"""
from __future__ import annotations


def dancetrack_config(**overrides) -> dict:
    cfg = dict(
        MODE="train", VISUALIZE=False, AVAILABLE_GPUS="0,1,2,3,4,5,6,7", DEVICE="cuda", USE_DISTRIBUTED=False,
        USE_CHECKPOINT=False, CHECKPOINT_LEVEL=2, DATASET="DanceTrack", BATCH_SIZE=1, ACCUMULATION_STEPS=1,
        # model (configs/train_dancetrack.yaml:57-75)
        BACKBONE="resnet50", HIDDEN_DIM=256, FFN_DIM=2048, NUM_FEATURE_LEVELS=4, NUM_HEADS=8, NUM_ENC_POINTS=4,
        NUM_DEC_POINTS=4, NUM_ENC_LAYERS=6, NUM_DEC_LAYERS=6, MERGE_DET_TRACK_LAYER=1, ACTIVATION="ReLU",
        RETURN_INTER_DEC=True, EXTRA_TRACK_ATTN=False, AUX_LOSS=True, USE_DAB=True, UPDATE_THRESH=0.5,
        LONG_MEMORY_LAMBDA=0.01,
        # sampling / training (:78-101)
        SAMPLE_STEPS=[6, 10, 14], SAMPLE_LENGTHS=[2, 3, 4, 5], SEED=42, EPOCHS=20,
        ONLY_TRAIN_QUERY_UPDATER_AFTER=20, DROPOUT=0.0, NUM_DET_QUERIES=300, TP_DROP_RATE=0.0, FP_INSERT_RATE=0.0,
        LR=2.0e-4, LR_BACKBONE=2.0e-5, LR_POINTS=1.0e-5, WEIGHT_DECAY=0.0005, CLIP_MAX_NORM=0.1,
        LR_SCHEDULER="MultiStep", LR_DROP_RATE=0.1, LR_DROP_MILESTONES=[12],
        # matcher / loss (:103-111)
        MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
        LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0, 1.0, 1.0, 1.0, 1.0],
        # inference thresholds (:24-33)
        DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.5, RESULT_SCORE_THRESH=0.5, MISS_TOLERANCE=30, USE_MOTION=False,
        MOTION_MIN_LENGTH=3, MOTION_MAX_LENGTH=5, MOTION_LAMBDA=0.5,
    )
    cfg.update(overrides)
    return cfg


def mot17_config(**overrides) -> dict:
    """configs/train_mot17.yaml: same model; clips of up to 4 frames (:80), MOT17 + CrowdHuman joint training."""
    cfg = dancetrack_config(DATASET="MOT17", SAMPLE_LENGTHS=[2, 3, 4], MISS_TOLERANCE=15)
    cfg.update(overrides)
    return cfg


def bdd100k_config(**overrides) -> dict:
    """configs/train_bdd100k.yaml: 8 classes, 720x1280 inputs, clips of up to 4 frames (:67), MISS_TOLERANCE 10 (:26)."""
    cfg = dancetrack_config(DATASET="BDD100K", SAMPLE_LENGTHS=[2, 3, 4], MISS_TOLERANCE=10)
    cfg.update(overrides)
    return cfg


_DATA_KEYS = {
    # configs/train_dancetrack.yaml:45-56, 80-83 (keys the file leaves empty are None, as yaml reads them)
    "DanceTrack": dict(DATA_ROOT=None, NUM_WORKERS=4, COCO_SIZE=False, OVERFLOW_BBOX=False, REVERSE_CLIP=0.0,
                       SAMPLE_STEPS=[6, 10, 14], SAMPLE_LENGTHS=[2, 3, 4, 5], SAMPLE_MODES=["random_interval"],
                       SAMPLE_INTERVALS=[10], USE_CROWDHUMAN=None, USE_MOTSYNTH=None, MOTSYNTH_RATE=None),
    # configs/train_sportsmot.yaml:44-55, 79-82
    "SportsMOT": dict(DATA_ROOT=None, NUM_WORKERS=4, COCO_SIZE=False, OVERFLOW_BBOX=False, REVERSE_CLIP=0.0,
                      SAMPLE_STEPS=[10, 16, 22], SAMPLE_LENGTHS=[2, 3, 4, 5], SAMPLE_MODES=["random_interval"],
                      SAMPLE_INTERVALS=[10], USE_CROWDHUMAN=None, USE_MOTSYNTH=None, MOTSYNTH_RATE=None),
    # configs/train_mot17.yaml:44-55, 79-83
    "MOT17": dict(DATA_ROOT=None, NUM_WORKERS=4, COCO_SIZE=True, OVERFLOW_BBOX=True, REVERSE_CLIP=0.0,
                  SAMPLE_STEPS=[60, 100], SAMPLE_LENGTHS=[2, 3, 4], SAMPLE_MODES=["random_interval"],
                  SAMPLE_INTERVALS=[10], SAMPLE_MOT17_JOIN=0, USE_CROWDHUMAN=True, USE_MOTSYNTH=None,
                  MOTSYNTH_RATE=None),
    # configs/train_bdd100k.yaml:39-42, 66-69 (the file has no augmentation keys: data/bdd100k.py fixes them)
    "BDD100K": dict(DATA_ROOT=None, NUM_WORKERS=8, SAMPLE_STEPS=[6, 10], SAMPLE_LENGTHS=[2, 3, 4],
                    SAMPLE_MODES=["random_interval"], SAMPLE_INTERVALS=[4, 4, 4]),
}


def data_config(dataset: str, **overrides) -> dict:
    """The data-pipeline keys of the shipped training config for ``dataset`` ("DanceTrack", "SportsMOT", "MOT17",
    "BDD100K"), with ``DATASET`` itself; to be merged over a model config:
    ``dict(dancetrack_config(), **data_config("DanceTrack", DATA_ROOT="/data"))``.  NUM_WORKERS is transcribed and not
    read: the clip loader has one producer thread and no worker processes."""
    if dataset not in _DATA_KEYS:
        raise ValueError(f"no shipped data config for dataset {dataset!r} (one of {sorted(_DATA_KEYS)})")
    cfg = {k: (list(v) if isinstance(v, list) else v) for k, v in _DATA_KEYS[dataset].items()}
    cfg["DATASET"] = dataset
    cfg.update(overrides)
    return cfg


def load_yaml(path: str) -> dict:
    """A training config in the reference's format: one flat mapping of UPPER_CASE keys (utils/utils.py:yaml_to_dict
    there).  Needs PyYAML."""
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: a config is one mapping of keys to values, got {type(cfg).__name__}")
    return cfg


def _train_dancetrack() -> dict:
    """configs/train_dancetrack.yaml, every key in the file's order (keys the file leaves empty are None)."""
    return dict(
        GIT_VERSION=None,
        MODE="train", CONFIG_PATH=None, VISUALIZE=False, AVAILABLE_GPUS="0,1,2,3,4,5,6,7", DEVICE="cuda",
        OUTPUTS_DIR="./outputs/pycharm/", USE_DISTRIBUTED=False, USE_CHECKPOINT=False, CHECKPOINT_LEVEL=2,
        RESUME=None, RESUME_SCHEDULER=True, MULTI_CHECKPOINT=False,
        # submit (:24-34)
        SUBMIT_DIR=None, SUBMIT_MODEL=None, SUBMIT_DATA_SPLIT="test", DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.5,
        RESULT_SCORE_THRESH=0.5, MISS_TOLERANCE=30, USE_MOTION=False, MOTION_MIN_LENGTH=3, MOTION_MAX_LENGTH=5,
        MOTION_LAMBDA=0.5,
        # evaluation (:37-42)
        EVAL_DIR=None, EVAL_MODE="specific", EVAL_MODEL=None, EVAL_PORT=None, EVAL_THREADS=1, EVAL_DATA_SPLIT="val",
        # data (:45-56)
        DATASET="DanceTrack", USE_MOTSYNTH=None, USE_CROWDHUMAN=None, MOTSYNTH_RATE=None, DATA_ROOT=None,
        DATA_PATH=None, NUM_WORKERS=4, BATCH_SIZE=1, ACCUMULATION_STEPS=1, COCO_SIZE=False, OVERFLOW_BBOX=False,
        REVERSE_CLIP=0.0,
        # model (:59-77)
        BACKBONE="resnet50", HIDDEN_DIM=256, FFN_DIM=2048, NUM_FEATURE_LEVELS=4, NUM_HEADS=8, NUM_ENC_POINTS=4,
        NUM_DEC_POINTS=4, NUM_ENC_LAYERS=6, NUM_DEC_LAYERS=6, MERGE_DET_TRACK_LAYER=1, ACTIVATION="ReLU",
        RETURN_INTER_DEC=True, EXTRA_TRACK_ATTN=False, AUX_LOSS=True, USE_DAB=True, UPDATE_THRESH=0.5,
        LONG_MEMORY_LAMBDA=0.01, PRETRAINED_MODEL="dab_deformable_detr.pth",
        # sampling / training (:80-101)
        SAMPLE_STEPS=[6, 10, 14], SAMPLE_LENGTHS=[2, 3, 4, 5], SAMPLE_MODES=["random_interval"],
        SAMPLE_INTERVALS=[10], SEED=42, EPOCHS=20, ONLY_TRAIN_QUERY_UPDATER_AFTER=20, DROPOUT=0.0,
        NUM_DET_QUERIES=300, TP_DROP_RATE=0.0, FP_INSERT_RATE=0.0, LR=2.0e-4, LR_BACKBONE=2.0e-5, LR_POINTS=1.0e-5,
        WEIGHT_DECAY=0.0005, CLIP_MAX_NORM=0.1, LR_SCHEDULER="MultiStep", LR_DROP_RATE=0.1, LR_DROP_MILESTONES=[12],
        # matcher / loss (:103-111)
        MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
        LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0, 1.0, 1.0, 1.0, 1.0],
    )


# What each other shipped file changes against train_dancetrack.yaml (value), and the keys it does not have (drop).
_SPORTSMOT = dict(DATASET="SportsMOT", SAMPLE_STEPS=[10, 16, 22], EPOCHS=28, ONLY_TRAIN_QUERY_UPDATER_AFTER=28,
                  LR_DROP_MILESTONES=[18])
_DEFORMABLE_DETR = dict(FFN_DIM=1024, USE_DAB=False, PRETRAINED_MODEL="deformable_detr.pth")
_BUILTIN = {
    "dancetrack": (dict(), ()),
    "sportsmot": (_SPORTSMOT, ()),
    # configs/train_mot17.yaml (SAMPLE_MOT17_JOIN is the one key only this file has, :83)
    "mot17": (dict(MISS_TOLERANCE=15, DATASET="MOT17", USE_CROWDHUMAN=True, COCO_SIZE=True, OVERFLOW_BBOX=True,
                   SAMPLE_STEPS=[60, 100], SAMPLE_LENGTHS=[2, 3, 4], SAMPLE_MOT17_JOIN=0, EPOCHS=130,
                   ONLY_TRAIN_QUERY_UPDATER_AFTER=130, LR_POINTS=2.0e-5, WEIGHT_DECAY=0.0001,
                   LR_DROP_MILESTONES=[120]), ()),
    # configs/train_bdd100k.yaml (no augmentation and no extra-dataset keys: data/bdd100k.py fixes them)
    "bdd100k": (dict(OUTPUTS_DIR="./outputs/memotr_bdd100k/", RESUME_SCHEDULER=False, SUBMIT_DATA_SPLIT="val",
                     MISS_TOLERANCE=10, DATASET="BDD100K", NUM_WORKERS=8, SAMPLE_STEPS=[6, 10],
                     SAMPLE_LENGTHS=[2, 3, 4], SAMPLE_INTERVALS=[4, 4, 4], EPOCHS=13,
                     ONLY_TRAIN_QUERY_UPDATER_AFTER=1000, WEIGHT_DECAY=0.0002),
                ("USE_MOTSYNTH", "USE_CROWDHUMAN", "MOTSYNTH_RATE", "COCO_SIZE", "OVERFLOW_BBOX", "REVERSE_CLIP")),
    "dancetrack_deformable_detr": (_DEFORMABLE_DETR, ()),
    "sportsmot_deformable_detr": (dict(_SPORTSMOT, **_DEFORMABLE_DETR), ()),
}
BUILTIN_CONFIGS = tuple(_BUILTIN)


def builtin_config(name: str) -> dict:
    """The shipped training config ``name`` (one of ``BUILTIN_CONFIGS``) with every key of its file: equal to
    ``load_yaml`` of configs/train_<name>.yaml of the reference.  A fresh dict on every call."""
    if name not in _BUILTIN:
        raise ValueError(f"no built-in config {name!r} (one of {', '.join(BUILTIN_CONFIGS)})")
    changed, dropped = _BUILTIN[name]
    cfg = _train_dancetrack()
    for k, v in changed.items():
        cfg[k] = list(v) if isinstance(v, list) else v
    for k in dropped:
        del cfg[k]
    return cfg
