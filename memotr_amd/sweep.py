"""Threshold sweep: score a checkpoint under many inference settings with ONE tracking pass per sequence.

``DET_SCORE_THRESH`` / ``TRACK_SCORE_THRESH`` / ``RESULT_SCORE_THRESH`` / ``MISS_TOLERANCE`` are tuned per dataset;
``submit`` + ``evaluate`` once per candidate pays for backbone and encoder on every frame of every pass, although neither
depends on them.  Here every sequence is tracked once by an ``inference_sweep.SweepTracker``, whose bank streams apply
one setting each, and every setting is scored from its own result files by the file evaluator ``evaluate`` uses.

    settings = threshold_grid(DET_SCORE_THRESH=[0.5, 0.6, 0.7], MISS_TOLERANCE=[15, 30])
    table = sweep(dict(EVAL_DIR="outputs/dancetrack", EVAL_MODEL="checkpoint_19.pth", EVAL_DATA_SPLIT="val",
                       DATA_ROOT="/data", DET_SCORE_THRESH=0.5, TRACK_SCORE_THRESH=0.5, RESULT_SCORE_THRESH=0.5,
                       MISS_TOLERANCE=30), settings)
    # outputs/dancetrack/val/sweep/<k>/tracker/<seq>.txt, outputs/dancetrack/val/sweep.jsonl
    best = max(table, key=lambda row: row["metrics"]["HOTA"])

    python -m memotr_amd.sweep --config-path outputs/dancetrack/train/config.yaml --data-root /data \\
        --eval-dir outputs/dancetrack --eval-model checkpoint_19.pth --eval-data-split val \\
        --grid det=0.5,0.6,0.7 track=0.5 result=0.5 miss=15,30
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
from typing import List, Optional, Sequence

from .inference_sweep import CONFIG_KEYS

GRID_NAMES = dict(det="DET_SCORE_THRESH", track="TRACK_SCORE_THRESH", result="RESULT_SCORE_THRESH",
                  miss="MISS_TOLERANCE")
_SETTING_KEY = {name: key for key, name in CONFIG_KEYS.items()}      # DET_SCORE_THRESH -> det_score_thresh


def threshold_grid(**axes) -> List[dict]:
    """The cartesian product of the values given per config key (``DET_SCORE_THRESH=[...]``, ``TRACK_SCORE_THRESH``,
    ``RESULT_SCORE_THRESH``, ``MISS_TOLERANCE``) as a list of settings, the first key varying slowest; a key that is not
    given is left out of the settings, and ``sweep`` takes it from the config."""
    unknown = sorted(set(axes) - set(_SETTING_KEY))
    if unknown:
        raise ValueError(f"threshold grid: unknown keys {unknown}; the keys are {sorted(_SETTING_KEY)}")
    names = [name for name in _SETTING_KEY if name in axes]
    values = []
    for name in names:
        axis = list(axes[name]) if isinstance(axes[name], (list, tuple)) else [axes[name]]
        if not axis:
            raise ValueError(f"threshold grid: {name} has no value")
        values.append([int(v) if name == "MISS_TOLERANCE" else float(v) for v in axis])
    return [dict(zip((_SETTING_KEY[n] for n in names), combo)) for combo in itertools.product(*values)]


def parse_grid(words: Sequence[str]) -> List[dict]:
    """``["det=0.5,0.6,0.7", "track=0.5", "miss=15,30"]`` -> ``threshold_grid`` of those axes."""
    axes = {}
    for word in words:
        name, eq, text = word.partition("=")
        if not eq or name not in GRID_NAMES or not text:
            raise ValueError(f"--grid takes {' '.join(k + '=v1,v2' for k in GRID_NAMES)}, not '{word}'")
        if GRID_NAMES[name] in axes:
            raise ValueError(f"--grid names '{name}' twice")
        try:
            axes[GRID_NAMES[name]] = [int(v) if name == "miss" else float(v) for v in text.split(",")]
        except ValueError:
            raise ValueError(f"--grid: '{word}' does not hold numbers") from None
    return threshold_grid(**axes)


def sweep(config: dict, settings, *, model=None, train_config: Optional[dict] = None,
          tracker_options: Optional[dict] = None, postprocess: Optional[dict] = None, max_streams: int = 8):
    """Track ``EVAL_DATA_SPLIT`` once with ``<EVAL_DIR>/<EVAL_MODEL>`` under every setting of ``settings`` and score each.
    ``config``: the keys of ``evaluate``'s "specific" mode (EVAL_DIR, EVAL_MODEL, EVAL_DATA_SPLIT, DATA_ROOT, DATASET) and
    the inference thresholds, which fill what a setting omits.  ``train_config`` and ``model`` as for ``eval_model`` (a
    ``model`` that is given receives the checkpoint's weights when EVAL_MODEL is set).  This rank's sequences (sharded as
    ``submit`` shards them) are each tracked by a ``SweepTracker`` of at most ``max_streams`` settings at a time;
    setting k's rows go to ``<EVAL_DIR>/<split>/sweep/<k>/tracker/<seq>.txt`` through the log's writers -- from
    ``log.filled(...)`` when ``postprocess`` (``dict(max_gap=..., min_length=...)``) is given.  After a barrier rank 0
    scores every setting with the file evaluator, appends ``{"index", "setting", "metrics"}`` per setting to
    ``<EVAL_DIR>/<split>/sweep.jsonl`` and returns the list; the other ranks return None.  ``tracker_options``: further
    ``SweepTracker`` arguments (``raw_size``, ``area_thresh``, ``cap``)."""
    import torch

    from .evaluate import _barrier, _score
    from .inference_sweep import SweepTracker
    from .postprocess import postprocess_options
    from .results import BankResultLog
    from .submit import _rank_and_world, _source, _write, load_model, sequence_frames, sequence_names, split_dir
    for key in ("EVAL_DIR", "EVAL_DATA_SPLIT", "DATA_ROOT"):
        if config.get(key) is None:
            raise ValueError(f"{key} must not be None for a threshold sweep")
    if max_streams < 1:
        raise ValueError(f"max_streams must be at least 1, not {max_streams}")
    if train_config is None:
        from .configs import load_yaml
        train_config = load_yaml(os.path.join(config["EVAL_DIR"], "train", "config.yaml"))
    dataset, split = config.get("DATASET") or train_config["DATASET"], config["EVAL_DATA_SPLIT"]
    if dataset == "BDD100K":
        raise NotImplementedError("the threshold sweep scores MOT-format datasets only (DanceTrack, SportsMOT, MOT17): "
                                  "BDD100K's per-class files are not swept")
    if dataset not in ("DanceTrack", "SportsMOT") and "MOT17" not in dataset:
        raise NotImplementedError(f"Eval Engine DO NOT support dataset '{dataset}'")
    postprocess = None if postprocess is None else postprocess_options(postprocess)
    settings = [dict({key: config[name] for key, name in CONFIG_KEYS.items()}, **s) for s in settings]
    if not settings:
        raise ValueError("a sweep needs at least one setting")
    if model is None:
        if config.get("EVAL_MODEL") is None:
            raise ValueError("EVAL_MODEL should not be None.")
        model = load_model(train_config, os.path.join(config["EVAL_DIR"], config["EVAL_MODEL"]))
    elif config.get("EVAL_MODEL") is not None:
        from .models.utils import get_model
        get_model(model).load_state_dict(torch.load(os.path.join(config["EVAL_DIR"], config["EVAL_MODEL"]),
                                                    map_location="cpu")["model"])
    device = next(model.parameters()).device
    options = dict(dataset_name=dataset, use_dab=train_config["USE_DAB"],
                   use_motion=bool(config.get("USE_MOTION", False)))      # (refused, in MultiSequenceTracker's words)
    if device.type == "cuda":       # one lookahead stream for the run, not one per tracker (profiles/submit_log.md)
        options["side_stream"] = torch.cuda.Stream(device)
    options.update(tracker_options or {})
    sweep_dir = os.path.join(config["EVAL_DIR"], split, "sweep")
    directory = split_dir(config["DATA_ROOT"], dataset, split)
    groups = [(at, settings[at:at + max_streams]) for at in range(0, len(settings), max_streams)]
    trackers = [SweepTracker(model, group, **options) for _, group in groups]
    log = BankResultLog(device, dataset_name=dataset)
    for seq in sequence_names(directory, *_rank_and_world()):
        seq_dir = os.path.join(directory, seq)
        paths = sequence_frames(dataset, seq_dir)
        for (at, group), tracker in zip(groups, trackers):
            log.reset()
            n_frames = tracker.track_logged(_source(paths), log, first_setting=at)
            assert n_frames == len(paths)
            rows = log
            if postprocess is not None:
                rows = log.filled(n_frames=n_frames, n_sequences=at + len(group), **postprocess)
            for k in range(at, at + len(group)):
                _write(dataset, os.path.join(sweep_dir, str(k)), seq_dir, rows.sequence(k), paths)
    _barrier()                                      # every rank's files are in sweep/<k>/tracker/
    table = None
    if _rank_and_world()[0] == 0:
        table = []
        for k, setting in enumerate(settings):
            tracker_dir = os.path.join(sweep_dir, str(k), "tracker")
            os.makedirs(tracker_dir, exist_ok=True)          # (a split without sequences)
            table.append({"index": k, "setting": setting, "metrics": _score(config, dataset, split, tracker_dir, device)})
        with open(os.path.join(config["EVAL_DIR"], split, "sweep.jsonl"), "a") as f:
            for row in table:
                f.write(json.dumps(row) + "\n")
    _barrier()
    return table


def main(argv: Optional[Sequence[str]] = None):
    """``memotr_amd.main``'s options and config loading, ``--grid`` and ``--max-streams`` on top; prints one line per
    setting."""
    from . import main as M
    parser = argparse.ArgumentParser("python -m memotr_amd.sweep", add_help=False)
    parser.add_argument("--grid", nargs="+", required=True, metavar="AXIS=V1,V2",
                        help="det=... track=... result=... miss=...: the values to sweep; an axis left out keeps the "
                             "config's value")
    parser.add_argument("--max-streams", type=int, default=8, help="Settings tracked side by side in one pass.")
    own, rest = parser.parse_known_args(argv)
    settings = parse_grid(own.grid)
    options = M.parse_options(rest)
    config = M.merge_config(M.load_config(options.config_path), options)
    M.check_supported(config)
    M.set_up_process(config)
    try:
        table = sweep(config, settings, max_streams=own.max_streams)
        for row in table or []:
            print(json.dumps(row))
        return table
    finally:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
