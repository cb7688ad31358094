"""The eval engine: checkpoints in, HOTA / CLEAR / Identity numbers out (the reference's ``eval_engine.py:12-124``).

    evaluate(dict(EVAL_DIR="outputs/dancetrack", EVAL_MODE="continue", EVAL_DATA_SPLIT="val", DATA_ROOT="/data",
                  DATASET="DanceTrack", DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.5, RESULT_SCORE_THRESH=0.5,
                  MISS_TOLERANCE=30))

``eval_model`` runs ``submit`` in this process (the reference starts ``main.py --mode submit`` and TrackEval as child
processes), moves ``<EVAL_DIR>/<split>/tracker`` to ``<checkpoint stem>_tracker`` and scores it with the package's own
evaluators (evaluation.py, evaluation_bdd100k.py), writing TrackEval's two-line ``<class>_summary.txt``.  ``evaluate``
is the sweep over ``checkpoint_{i}.pth`` with its ``eval_states.yaml``; in place of the reference's TensorBoard scalars
it appends one JSON line per checkpoint to ``<EVAL_DIR>/<split>/metrics.jsonl`` and calls ``on_metrics``.
"""
from __future__ import annotations

import json
import os
import shutil
from typing import Callable, Optional

import torch

from .submit import _rank_and_world, load_model, split_dir, submit


def _barrier() -> None:
    if _rank_and_world()[1] > 1:
        torch.distributed.barrier()


def write_summary(path: str, fields: dict) -> None:
    """TrackEval's summary file: the names on one line, the values on the next, space-separated."""
    with open(path, "w") as f:
        f.write(" ".join(fields) + "\n")
        f.write(" ".join(str(v) for v in fields.values()) + "\n")


def _score(config: dict, dataset: str, split: str, tracker_dir: str, device) -> dict:
    from . import evaluation as E
    device = device if device is not None and device.type == "cuda" else None
    if dataset == "BDD100K":
        from .evaluation_bdd100k import bdd_summary, evaluate_bdd_files
        metrics = bdd_summary(evaluate_bdd_files(config["EVAL_GT_DIR"], tracker_dir, device=device))
        for key, fields in metrics.items():
            write_summary(os.path.join(tracker_dir, f"{key}_summary.txt"), fields)
        return metrics
    data_dir = os.path.join(config["DATA_ROOT"], dataset)
    res = E.evaluate_files(split_dir(config["DATA_ROOT"], dataset, split), tracker_dir,
                           os.path.join(data_dir, f"{split}_seqmap.txt"),
                           benchmark="MOT15" if "mot15" in split else "MOT17", device=device)
    metrics = E.summary(res["COMBINED_SEQ"])
    write_summary(os.path.join(tracker_dir, "pedestrian_summary.txt"), metrics)
    return metrics


def eval_model(config: dict, checkpoint: str, *, model=None, train_config: Optional[dict] = None,
               tracker_options: Optional[dict] = None, streams: Optional[int] = None,
               postprocess: Optional[dict] = None) -> Optional[dict]:
    """Track ``EVAL_DATA_SPLIT`` with ``<EVAL_DIR>/<checkpoint>`` and score the result (eval_engine.py:66-124).
    ``train_config`` defaults to ``<EVAL_DIR>/train/config.yaml``; a ``model`` that is given receives the checkpoint's
    weights.  DanceTrack, SportsMOT and MOT17: ground truth under ``split_dir``, sequence names in
    ``<DATA_ROOT>/<DATASET>/<split>_seqmap.txt``, MOT15 rules for a split named ``*mot15*``; returns
    ``evaluation.summary`` of all sequences.  BDD100K: scored
    against ``EVAL_GT_DIR`` (a folder of ``<seq>.json``) and ``NotImplementedError`` without it, as in the reference;
    returns ``bdd_summary``.  With ``torch.distributed`` initialised every rank tracks its share, all meet at a barrier,
    rank 0 scores and the others return None.  ``streams`` and ``postprocess`` are ``submit``'s: the files that are
    scored are written from the filled log when the pass is on."""
    if train_config is None:
        from .configs import load_yaml
        train_config = load_yaml(os.path.join(config["EVAL_DIR"], "train", "config.yaml"))
    dataset, split = config.get("DATASET") or train_config["DATASET"], config["EVAL_DATA_SPLIT"]
    if dataset == "BDD100K":
        if config.get("EVAL_GT_DIR") is None:
            raise NotImplementedError("Eval Engine DO NOT support dataset 'BDD100K' without EVAL_GT_DIR "
                                      "(a folder of <seq>.json ground truth)")
    elif dataset not in ("DanceTrack", "SportsMOT") and "MOT17" not in dataset:
        raise NotImplementedError(f"Eval Engine DO NOT support dataset '{dataset}'")
    path = os.path.join(config["EVAL_DIR"], checkpoint)
    if model is None:
        model = load_model(train_config, path)
    else:
        from .models.utils import get_model
        get_model(model).load_state_dict(torch.load(path, map_location="cpu")["model"])
    # (``streams`` and ``postprocess``: submit's; handed on only when given, None leaves MEMOTR_SUBMIT_STREAMS / 1 and
    # MEMOTR_POSTPROCESS / off to submit)
    submit(dict(config, SUBMIT_DIR=config["EVAL_DIR"], SUBMIT_MODEL=checkpoint, SUBMIT_DATA_SPLIT=split), model=model,
           train_config=dict(train_config, DATASET=dataset), tracker_options=tracker_options,
           **({} if streams is None else {"streams": streams}),
           **({} if postprocess is None else {"postprocess": postprocess}))
    _barrier()                                      # every rank's files are in tracker/
    metrics = None
    if _rank_and_world()[0] == 0:
        tracker_dir = os.path.join(config["EVAL_DIR"], split, "tracker")
        moved = os.path.join(config["EVAL_DIR"], split, os.path.splitext(checkpoint)[0] + "_tracker")
        if os.path.isdir(moved):
            shutil.rmtree(moved)
        shutil.move(tracker_dir, moved)
        metrics = _score(config, dataset, split, moved, next(model.parameters()).device)
    _barrier()                                      # tracker/ is gone before anyone writes the next checkpoint's
    return metrics


def evaluate(config: dict, on_metrics: Optional[Callable[[int, dict], None]] = None, *, model=None,
             train_config: Optional[dict] = None, tracker_options: Optional[dict] = None,
             streams: Optional[int] = None, postprocess: Optional[dict] = None):
    """eval_engine.py:12-63.  ``EVAL_MODE`` "specific": ``eval_model`` of ``EVAL_MODEL``, returns its metrics.
    "continue": every ``checkpoint_{i}.pth`` of ``EVAL_DIR`` from ``eval_states.yaml``'s ``NEXT_INDEX`` on; an index
    whose ``pedestrian_summary.txt`` exists is not evaluated again; ``eval_states.yaml`` is rewritten after each index,
    ``on_metrics(i, metrics)`` is called and a line appended to ``metrics.jsonl`` for each one evaluated; returns
    ``{i: metrics}`` of those."""
    split, eval_dir = config["EVAL_DATA_SPLIT"], config["EVAL_DIR"]
    outputs_dir = os.path.join(eval_dir, split)
    main = _rank_and_world()[0] == 0
    kwargs = dict(model=model, train_config=train_config, tracker_options=tracker_options, streams=streams,
                  postprocess=postprocess)

    def record(index, checkpoint, metrics):
        if not main:
            return
        with open(os.path.join(outputs_dir, "metrics.jsonl"), "a") as f:
            f.write(json.dumps({"index": index, "checkpoint": checkpoint, "metrics": metrics}) + "\n")
        if on_metrics is not None:
            on_metrics(index, metrics)

    if config["EVAL_MODE"] == "specific":
        if config.get("EVAL_MODEL") is None:
            raise ValueError("EVAL_MODEL should not be None.")
        os.makedirs(outputs_dir, exist_ok=True)
        metrics = eval_model(config, config["EVAL_MODEL"], **kwargs)
        record(None, config["EVAL_MODEL"], metrics)
        return metrics
    if config["EVAL_MODE"] != "continue":
        raise ValueError(f"Eval mode '{config['EVAL_MODE']}' is not supported.")
    import yaml
    os.makedirs(outputs_dir, exist_ok=True)
    states_path = os.path.join(outputs_dir, "eval_states.yaml")
    states = {"NEXT_INDEX": 0}
    if os.path.exists(states_path):
        with open(states_path) as f:
            states = yaml.safe_load(f)
    evaluated = {}
    for i in range(states["NEXT_INDEX"], 10000):
        checkpoint = f"checkpoint_{i}.pth"
        if not os.path.exists(os.path.join(eval_dir, checkpoint)):
            continue
        if not os.path.exists(os.path.join(outputs_dir, f"checkpoint_{i}_tracker", "pedestrian_summary.txt")):
            evaluated[i] = eval_model(config, checkpoint, **kwargs)
            record(i, checkpoint, evaluated[i])
        states["NEXT_INDEX"] = i + 1
        if main:
            with open(states_path, "w") as f:
                yaml.dump(states, f, allow_unicode=True)
    if main:
        with open(states_path, "w") as f:
            yaml.dump(states, f, allow_unicode=True)
    return evaluated
