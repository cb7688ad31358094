"""The submit engine: a checkpoint and a dataset split in, one result file per sequence out (the reference's
``submit_engine.py:187-252`` and the ``Submitter`` it drives).

    files = submit(dict(SUBMIT_DIR="outputs/dancetrack", SUBMIT_MODEL="checkpoint_19.pth", SUBMIT_DATA_SPLIT="val",
                        DATA_ROOT="/data", DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.5, RESULT_SCORE_THRESH=0.5,
                        MISS_TOLERANCE=30, USE_MOTION=False))
    # outputs/dancetrack/val/tracker/<seq>.txt      (BDD100K: <seq>.json)

Every sequence is tracked by a fresh ``SequenceTracker`` through ``track_logged``: the result rows stay in one reused
device-resident ``ResultLog`` and are read once, when the sequence ends (results.py).  With ``torch.distributed``
initialised each rank takes every ``world_size``-th sequence of the sorted listing; there is no DistributedDataParallel
wrap, since inference needs no collective.
"""
from __future__ import annotations

import json
import os
from typing import Callable, List, Optional

import torch

from .results import ResultLog


def split_dir(data_root: str, dataset: str, split: str) -> str:
    """Where the sequences of ``split`` lie (submit_engine.py:217-222)."""
    if dataset in ("DanceTrack", "SportsMOT"):
        return os.path.join(data_root, dataset, split)
    if dataset == "BDD100K":
        return os.path.join(data_root, dataset, "images", "track", split)
    return os.path.join(data_root, dataset, "images", split)


def sequence_names(directory: str, rank: int = 0, world_size: int = 1) -> List[str]:
    """This rank's share of the sequences: every ``world_size``-th name of the SORTED listing, from ``rank`` (the
    reference shards ``os.listdir``'s order, which need not agree between processes)."""
    if not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} outside 0 .. {world_size - 1}")
    return sorted(os.listdir(directory))[rank::world_size]


def sequence_frames(dataset: str, seq_dir: str) -> List[str]:
    """The frames of a sequence in order (the reference's data/seq_dataset.py:11-19): sorted names containing ``jpg`` or
    ``png``, under ``img1/`` except for BDD100K."""
    image_dir = seq_dir if dataset == "BDD100K" else os.path.join(seq_dir, "img1")
    return [os.path.join(image_dir, n) for n in sorted(os.listdir(image_dir)) if "jpg" in n or "png" in n]


def _is_jpeg(path: str) -> bool:
    with open(path, "rb") as f:
        return f.read(2) == b"\xff\xd8"


def _pixels(paths):
    """Frames as (H, W, 3) uint8 RGB arrays, decoded on the host: JPEG by the package's decoder (the pixels the device
    stage gives), anything else by Pillow -- the JPEG path's own Pillow fallback takes JPEG streams only."""
    import numpy as np
    from PIL import Image

    from .data.jpeg import decode_jpeg
    for p in paths:
        if _is_jpeg(p):
            yield decode_jpeg(p, "cpu")
        else:
            with Image.open(p) as im:
                yield torch.from_numpy(np.array(im.convert("RGB"), order="C"))


def _source(paths):
    """What a tracker is given for the frames at ``paths``: the paths themselves when all are JPEG files (decoded on the
    device), else host-decoded pixels."""
    return paths if all(_is_jpeg(p) for p in paths) else _pixels(paths)


def _write(dataset: str, outputs_dir: str, seq_dir: str, rows, paths) -> str:
    """``<outputs_dir>/tracker/<seq>.txt`` (BDD100K: ``<seq>.json``) from the rows of one sequence (a ``ResultLog``, or
    ``BankResultLog.sequence(i)``), written whole, replacing an older file.  Returns the file's path."""
    seq = os.path.basename(os.path.normpath(seq_dir))
    predict_dir = os.path.join(outputs_dir, "tracker")
    os.makedirs(predict_dir, exist_ok=True)
    if dataset == "BDD100K":
        out = os.path.join(predict_dir, seq + ".json")
        with open(out, "w", encoding="utf-8") as f:
            json.dump(rows.bdd_frames(paths), f)
    else:
        out = os.path.join(predict_dir, seq + ".txt")
        text = "".join(rows.mot_lines(dataset))
        with open(out, "w") as f:
            f.write(text)
    return out


def submit_sequence(tracker_factory: Callable, dataset: str, seq_dir: str, outputs_dir: str, log: ResultLog,
                    annotate=None, postprocess: Optional[dict] = None) -> str:
    """Track the sequence in ``seq_dir`` with a fresh tracker from ``tracker_factory()`` and write its result file
    (``_write``).  ``log`` is emptied first and holds the sequence's rows afterwards.  ``annotate``: ``(writer, i)`` --
    a render.MultiAnnotatedWriter that is also given the annotated frames, as those of its sequence ``i``
    (``track_annotated_logged``).  ``postprocess``: ``dict(max_gap=..., min_length=...)`` -- the file is written from
    ``log.filled(...)`` (results.py), ``log`` itself keeps the rows as tracked.  Returns the file's path."""
    paths = sequence_frames(dataset, seq_dir)
    tracker = tracker_factory()
    log.reset()
    if annotate is None:
        n_frames = tracker.track_logged(_source(paths), log)
    else:
        n_frames = tracker.track_annotated_logged(_source(paths), annotate[0], log, sequence=annotate[1])
    assert n_frames == len(paths)
    rows = log
    if postprocess is not None:         # the host knows both sizes of the cell table: nothing is read for them
        rows = log.filled(n_frames=n_frames, n_ids=tracker.tracker.max_obj_id, **postprocess)
    return _write(dataset, outputs_dir, seq_dir, rows, paths)


def load_model(train_config: dict, checkpoint: str):
    """``build_model(train_config)`` with the weights of ``checkpoint`` -- loaded by every rank: without a
    DistributedDataParallel wrap there is no broadcast to rely on."""
    from .models import build_model
    model = build_model(train_config)
    model.load_state_dict(torch.load(checkpoint, map_location="cpu")["model"])
    return model


def _rank_and_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def submit_streams(streams: Optional[int] = None) -> int:
    """How many sequences ``submit`` tracks side by side: ``streams``, or MEMOTR_SUBMIT_STREAMS, or 1."""
    n = int(os.environ.get("MEMOTR_SUBMIT_STREAMS", "1")) if streams is None else int(streams)
    if n < 1:
        raise ValueError(f"streams must be at least 1, not {n}")
    return n


def submit_sequences(tracker, dataset: str, seq_dirs: List[str], outputs_dir: str, log, writer=None,
                     postprocess: Optional[dict] = None) -> List[str]:
    """``submit_sequence`` for many sequences at once: ``tracker`` (an inference_multi.MultiSequenceTracker) runs them
    in lockstep through ``track_many_logged``, ``log`` (a results.BankResultLog) holds the rows of all of them, and the
    files are written when the last one ends.  ``writer``: a render.MultiAnnotatedWriter that is also given the
    annotated frames (``track_many_annotated_logged``).  ``postprocess``: as for ``submit_sequence``, one
    ``log.filled(...)`` over all sequences (the ids live on the device: one small read finds the largest).  Returns the
    files' paths, in the order of ``seq_dirs``."""
    paths = [sequence_frames(dataset, d) for d in seq_dirs]
    log.reset()
    if writer is None:
        counts = tracker.track_many_logged([_source(p) for p in paths], log)
    else:
        counts = tracker.track_many_annotated_logged([_source(p) for p in paths], writer, log)
    assert counts == [len(p) for p in paths]
    if postprocess is not None:
        log = log.filled(n_frames=max(counts, default=0), n_sequences=len(seq_dirs), **postprocess)
    return [_write(dataset, outputs_dir, d, log.sequence(i), paths[i]) for i, d in enumerate(seq_dirs)]


def submit(config: dict, *, model=None, train_config: Optional[dict] = None,
           tracker_options: Optional[dict] = None, streams: Optional[int] = None,
           annotate_dir: Optional[str] = None, annotate_options: Optional[dict] = None,
           postprocess: Optional[dict] = None) -> List[str]:
    """submit_engine.py:187-252.  ``config``: SUBMIT_DIR, SUBMIT_MODEL, SUBMIT_DATA_SPLIT, DATA_ROOT and the inference
    thresholds (DET_SCORE_THRESH, TRACK_SCORE_THRESH, RESULT_SCORE_THRESH, MISS_TOLERANCE, USE_MOTION and the MOTION_*
    keys).  ``train_config`` (DATASET, USE_DAB and the model's keys) defaults to ``<SUBMIT_DIR>/train/config.yaml``;
    ``model`` defaults to ``load_model(train_config, <SUBMIT_DIR>/<SUBMIT_MODEL>)``.  ``tracker_options``: further
    ``SequenceTracker`` arguments (``raw_size``, ``area_thresh``) for every sequence's tracker.  Returns the files this
    rank wrote, in sequence order.  ``streams`` (default: MEMOTR_SUBMIT_STREAMS, else 1): above 1, that many of the
    rank's sequences are tracked side by side (inference_multi.py) and the files are written from one
    ``BankResultLog``; the rows are those of ``streams=1`` up to float rounding.  ``annotate_dir``: every frame is
    also written with its reported tracks drawn in, as ``<annotate_dir>/<seq>/<frame index, 8 digits>.jpg``, from the
    device (render.MultiAnnotatedWriter: no result is brought to the host for it); ``annotate_options``: ``quality``,
    ``subsampling``, ``thickness``, ``font_scale``, ``fill_alpha`` of that writer.  The result files are the same with
    and without it.  ``postprocess`` (default: MEMOTR_POSTPROCESS="max_gap=20,min_length=5", else off):
    ``dict(max_gap=..., min_length=...)`` -- every file is written from the filled log (postprocess.py: tracks of fewer
    than ``min_length`` rows removed, holes of at most ``max_gap`` frames interpolated), made on the device when the
    sequence ends; unknown keys are a ``TypeError``.  Annotated frames are drawn online, frame by frame, and are not
    affected: they show the tracks as reported, holes included."""
    from .inference import SequenceTracker
    from .postprocess import postprocess_options
    streams = submit_streams(streams)
    postprocess = postprocess_options(postprocess)
    unknown = set(annotate_options or {}) - {"quality", "subsampling", "thickness", "font_scale", "fill_alpha"}
    if unknown:
        raise TypeError(f"unknown annotate options {sorted(unknown)}")
    if annotate_options and annotate_dir is None:
        raise ValueError("annotate_options without annotate_dir")
    for key in ("SUBMIT_DIR", "SUBMIT_DATA_SPLIT", "DATA_ROOT"):
        if config.get(key) is None:
            raise ValueError(f"{key} must not be None for the submit process")
    if train_config is None:
        from .configs import load_yaml
        train_config = load_yaml(os.path.join(config["SUBMIT_DIR"], "train", "config.yaml"))
    dataset, split = train_config["DATASET"], config["SUBMIT_DATA_SPLIT"]
    outputs_dir = os.path.join(config["SUBMIT_DIR"], split)
    if model is None:
        if config.get("SUBMIT_MODEL") is None:
            raise ValueError("SUBMIT_MODEL must not be None for the submit process")
        model = load_model(train_config, os.path.join(config["SUBMIT_DIR"], config["SUBMIT_MODEL"]))
    device = next(model.parameters()).device
    options = dict(
        dataset_name=dataset, use_dab=train_config["USE_DAB"], det_score_thresh=config["DET_SCORE_THRESH"],
        track_score_thresh=config["TRACK_SCORE_THRESH"], result_score_thresh=config["RESULT_SCORE_THRESH"],
        miss_tolerance=config["MISS_TOLERANCE"], use_motion=bool(config.get("USE_MOTION", False)),
        motion_lambda=config.get("MOTION_LAMBDA", 0.5), motion_min_length=config.get("MOTION_MIN_LENGTH", 3),
        motion_max_length=config.get("MOTION_MAX_LENGTH", 5))
    if device.type == "cuda":       # one lookahead stream for the run, not one per sequence (profiles/submit_log.md)
        options["side_stream"] = torch.cuda.Stream(device)
    options.update(tracker_options or {})
    directory = split_dir(config["DATA_ROOT"], dataset, split)
    names = sequence_names(directory, *_rank_and_world())
    writer = None
    if annotate_dir is not None:
        from .render import MultiAnnotatedWriter
        writer = MultiAnnotatedWriter(annotate_dir, names=names, **(annotate_options or {}))
    try:
        if streams > 1:
            from .inference_multi import MultiSequenceTracker
            from .results import BankResultLog
            for key in ("motion_lambda", "motion_min_length", "motion_max_length"):
                options.pop(key)
            tracker = MultiSequenceTracker(model, n_streams=streams, **options)
            files = submit_sequences(tracker, dataset, [os.path.join(directory, seq) for seq in names], outputs_dir,
                                     BankResultLog(device), writer, postprocess)
        else:
            log = ResultLog(device)
            files = [submit_sequence(lambda: SequenceTracker(model, **options), dataset, os.path.join(directory, seq),
                                     outputs_dir, log, None if writer is None else (writer, i), postprocess)
                     for i, seq in enumerate(names)]
    except BaseException:
        if writer is not None:          # an error is already on its way: drain, but do not replace it
            try:
                writer.close()
            except Exception:
                pass
        raise
    if writer is not None:
        writer.close()
    return files
