"""The command-line entry: train, submit and eval from one config (the reference's ``main.py`` with
``configs/utils.py``).

    python -m memotr_amd --config-path dancetrack --mode train --data-root /data --outputs-dir outputs/dancetrack \\
        --pretrained-model dab_deformable_detr.pth
    python -m memotr_amd --config-path outputs/dancetrack/train/config.yaml --mode submit --data-root /data \\
        --submit-dir outputs/dancetrack --submit-model checkpoint_19.pth --submit-data-split test
    python -m memotr_amd --config-path outputs/dancetrack/train/config.yaml --mode eval --data-root /data \\
        --eval-dir outputs/dancetrack --eval-mode specific --eval-model checkpoint_19.pth --eval-data-split val

``--config-path`` is a YAML file in the reference's format or one of ``configs.BUILTIN_CONFIGS``; every other option
replaces the equally named UPPER_CASE key (``merge_config``).  ``run(config)`` dispatches on ``MODE``.

Keys that nothing here implements fail with a sentence saying why (``check_supported``): ``BATCH_SIZE`` other than 1,
``VISUALIZE`` and ``USE_MOTSYNTH``.  ``EVAL_PORT`` and ``EVAL_THREADS`` (the reference's child processes for submit and
TrackEval: ``evaluate`` runs both in this process) and ``GIT_VERSION`` (a TensorBoard text) are accepted and ignored.
"""
from __future__ import annotations

import argparse
import os
from typing import Optional, Sequence

from .configs import BUILTIN_CONFIGS, builtin_config, load_yaml


def parse_options(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    """The reference's option set, names and types (main.py:15-90); ``--config-path`` also takes a built-in name."""
    parser = argparse.ArgumentParser("python -m memotr_amd", description="Network training and evaluation script.",
                                     add_help=True)
    parser.add_argument("--git-version", type=str)
    # system
    parser.add_argument("--available-gpus", type=str, help="Available GPUs, like '0,1,2,3'.")
    parser.add_argument("--use-distributed", action="store_true", help="Use distributed training.")
    parser.add_argument("--use-checkpoint", action="store_true", help="Use gradient checkpoint to save GPU memory.")
    parser.add_argument("--checkpoint-level", type=int)
    # running mode
    parser.add_argument("--mode", type=str, help="Running mode: train, submit or eval.")
    # submit
    parser.add_argument("--submit-dir", type=str)
    parser.add_argument("--submit-model", type=str)
    parser.add_argument("--submit-data-split", type=str)
    # eval
    parser.add_argument("--eval-dir", type=str)
    parser.add_argument("--eval-mode", type=str)
    parser.add_argument("--eval-model", type=str)
    parser.add_argument("--eval-threads", type=int, help="Accepted and ignored.")
    parser.add_argument("--eval-port", type=int, help="Accepted and ignored.")
    parser.add_argument("--eval-data-split", type=str)
    # weights
    parser.add_argument("--pretrained-model", type=str, help="Pretrained model path.")
    parser.add_argument("--resume", type=str, help="Resume checkpoint path.")
    parser.add_argument("--resume-scheduler", type=str, help="Whether resume the training scheduler.")
    # paths
    parser.add_argument("--config-path", type=str, default="dancetrack",
                        help="Config file path, or one of: " + ", ".join(BUILTIN_CONFIGS) + ".")
    parser.add_argument("--data-root", type=str, help="Dataset root dir.")
    parser.add_argument("--dataset", type=str)
    parser.add_argument("--data-path", type=str)
    parser.add_argument("--outputs-dir", type=str, help="Outputs dir path.")
    # data
    parser.add_argument("--accumulation-steps", type=int, help="Gradient accumulation steps.")
    parser.add_argument("--batch-size", type=int, help="Batch size for training (only 1 is implemented).")
    parser.add_argument("--coco-size", type=str)
    parser.add_argument("--overflow-bbox", type=str)
    parser.add_argument("--reverse-clip", type=float)
    parser.add_argument("--use-motsynth", type=str)
    parser.add_argument("--use-crowdhuman", type=str)
    parser.add_argument("--motsynth-rate", type=float)
    parser.add_argument("--sample-steps", type=int, nargs="*")
    parser.add_argument("--sample-lengths", type=int, nargs="*")
    # training
    parser.add_argument("--weight-decay", type=float)
    parser.add_argument("--lr", type=float)
    parser.add_argument("--lr-points", type=float)
    parser.add_argument("--lr-backbone", type=float)
    parser.add_argument("--epochs", type=int)
    parser.add_argument("--lr-drop-milestones", type=int, nargs="*")
    # submit setting
    parser.add_argument("--miss-tolerance", type=float)
    # model
    parser.add_argument("--num-det-queries", type=int)
    parser.add_argument("--merge-det-track-layer", type=int)
    # training augmentation
    parser.add_argument("--tp-drop-rate", type=float)
    parser.add_argument("--fp-insert-rate", type=float)
    return parser.parse_args(argv)


def _unique(config: dict, seen: set) -> bool:
    for k, v in config.items():
        if k in seen:
            return False
        seen.add(k)
        if isinstance(v, dict) and not _unique(v, seen):
            return False
    return True


def _set(config: dict, key: str, value) -> bool:
    """The first key equal to ``key`` in the file's order, nested mappings searched where they stand."""
    for k in config:
        if isinstance(config[k], dict):
            if _set(config[k], key, value):
                return True
        elif k == key:
            config[k] = {"True": True, "False": False}.get(value, value) if isinstance(value, str) else value
            return True
    return False


def merge_config(config: dict, options: argparse.Namespace, config_path: Optional[str] = None) -> dict:
    """configs/utils.py:update_config and main.py:122-123: every option that is not None (but ``config_path``) replaces
    the key of its name in upper case, the strings "True" / "False" as bools; an option without such a key and a key
    that appears twice (at any depth) are errors; ``CONFIG_PATH`` becomes the path given.  ``config`` is changed and
    returned.  (``--use-distributed`` and ``--use-checkpoint`` are flags: absent they are False, and False replaces the
    file's value, as in the reference.)"""
    if not _unique(config, set()):
        raise RuntimeError("Config's key is not unique, Please check the config file.")
    for name, value in vars(options).items():
        if name != "config_path" and value is not None:
            if not _set(config, name.upper(), value):
                raise RuntimeError("The option '--%s' is not appeared in .yaml config file." % name)
    config["CONFIG_PATH"] = config_path if config_path is not None else getattr(options, "config_path", None)
    return config


def load_config(path: str) -> dict:
    """A built-in name, else a YAML file."""
    return builtin_config(path) if path in BUILTIN_CONFIGS else load_yaml(path)


def check_supported(config: dict) -> None:
    """Fail loudly on keys whose meaning nothing in this package implements."""
    if config.get("BATCH_SIZE", 1) != 1:
        raise NotImplementedError(f"BATCH_SIZE is {config['BATCH_SIZE']}: the clip loader makes one clip per batch and "
                                  f"collating several is not built here; use ACCUMULATION_STEPS for a larger step.")
    if config.get("VISUALIZE"):
        raise NotImplementedError("VISUALIZE is set: the reference's per-frame debug plots are not built here; "
                                  "render.AnnotatedWriter draws tracked sequences.")
    if config.get("USE_MOTSYNTH"):
        raise NotImplementedError("USE_MOTSYNTH is set: MOTSynth is not supported (no shipped config uses it)")


def set_up_process(config: dict):
    """What must happen before anything touches a device (main.py:94-101, train_engine.py:34): the visible GPUs, the
    device, the process group, the seed.  Returns the ``torch.device`` of this process."""
    gpus = config.get("AVAILABLE_GPUS")
    if gpus not in (None, "") and "LOCAL_RANK" not in os.environ:       # a launcher has made that choice already
        os.environ["CUDA_VISIBLE_DEVICES"] = str(gpus)
        os.environ["HIP_VISIBLE_DEVICES"] = str(gpus)
    import torch

    from .utils.utils import set_seed
    kind = config.get("DEVICE", "cuda")
    if kind not in ("cuda", "cpu"):
        raise ValueError(f"DEVICE is '{kind}': 'cuda' or 'cpu'")
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if config.get("USE_DISTRIBUTED"):
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            torch.distributed.init_process_group("nccl" if kind == "cuda" else "gloo")
        device = torch.device("cuda", local_rank) if kind == "cuda" else torch.device("cpu")
    else:
        device = torch.device("cuda", 0) if kind == "cuda" else torch.device("cpu")
    if device.type == "cuda":
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        torch.cuda.set_device(device)
    set_seed(config["SEED"])
    return device


def run(config: dict, *, model=None, dataset=None, tracker_options: Optional[dict] = None, **train_options):
    """Dispatch on ``MODE`` (main.py:93-114).  ``model`` / ``dataset`` / ``tracker_options`` are handed to the engines
    in place of what they would build (tests; ``train_options``: further ``train_from_config`` arguments).  Returns
    what the engine returns."""
    mode = config.get("MODE")
    if mode not in ("train", "submit", "eval"):
        raise ValueError(f"Unsupported mode '{mode}'")
    check_supported(config)
    device = set_up_process(config)
    if mode == "train":
        from .train import train_from_config
        return train_from_config(config, device if model is None else None, model=model, dataset=dataset,
                                 run_log=True, **train_options)
    if mode == "submit":
        from .submit import submit
        return submit(config, model=model, tracker_options=tracker_options)
    from .evaluate import evaluate
    return evaluate(config, model=model, tracker_options=tracker_options)


def main(argv: Optional[Sequence[str]] = None):
    options = parse_options(argv)
    config = merge_config(load_config(options.config_path), options)
    try:
        return run(config)
    finally:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
