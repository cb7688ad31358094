"""The training driver: the epoch loop of the reference's train_engine.py:52-155 around ``engine.clip_forward_backward``
and ``engine.optimizer_step``.

``fit`` is ``train()`` without the data pipeline (``make_batches(epoch)`` yields collate-format batches) and without
the logger; ``train_from_config`` puts the data pipeline in front of it (``data.build_dataset``, ``data.ClipLoader``).
In ``fit``, learning-rate schedule, the epoch policies (ONLY_TRAIN_QUERY_UPDATER_AFTER, the NO_GRAD_STEPS /
NO_GRAD_FRAMES table), RESUME / RESUME_SCHEDULER and the checkpoint cadence are the reference's, line by line.
``train_one_epoch`` keeps the losses on the device and reads them every ``log_every`` iterations in one transfer: the
reference's ``loss.item()`` per iteration is a host synchronisation per clip.
"""
from __future__ import annotations

import os
from typing import Callable, Iterable, Optional

import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, MultiStepLR

from .engine import build_optimizer, clip_forward_backward, optimizer_step
from .models.utils import load_checkpoint, save_checkpoint


def build_scheduler(config: dict, optimizer: torch.optim.Optimizer):
    """train_engine.py:56-68."""
    if config["LR_SCHEDULER"] == "MultiStep":
        return MultiStepLR(optimizer, milestones=config["LR_DROP_MILESTONES"], gamma=config["LR_DROP_RATE"])
    if config["LR_SCHEDULER"] == "Cosine":
        return CosineAnnealingLR(optimizer=optimizer, T_max=config["EPOCHS"])
    raise ValueError(f"Do not support lr scheduler '{config['LR_SCHEDULER']}'")


def apply_epoch_policy(config: dict, optimizer: torch.optim.Optimizer, epoch: int) -> Optional[int]:
    """What the reference decides at the top of an epoch (train_engine.py:104-107, 119-124): from
    ONLY_TRAIN_QUERY_UPDATER_AFTER on, the backbone, sampling-point and default groups (0, 1, 3) stop learning; the
    first NO_GRAD_STEPS[i] <= epoch picks NO_GRAD_FRAMES[i].  Returns no_grad_frames (None: every frame is trained)."""
    if epoch >= config["ONLY_TRAIN_QUERY_UPDATER_AFTER"]:
        for i in (0, 1, 3):
            optimizer.param_groups[i]["lr"] = 0.0
    if "NO_GRAD_FRAMES" in config:
        for i in range(len(config["NO_GRAD_STEPS"])):
            if epoch >= config["NO_GRAD_STEPS"][i]:
                return config["NO_GRAD_FRAMES"][i]
    return None


def train_one_epoch(model, criterion, optimizer, batches: Iterable[dict], *, device, max_norm: float,
                    accumulation_steps: int = 1, use_dab: bool = True, no_grad_frames: Optional[int] = None,
                    states: dict, log_every: int = 100, on_log: Optional[Callable[[dict], None]] = None) -> dict:
    """train_engine.py:183-276: one clip per iteration, an optimizer step every ``accumulation_steps`` clips (gradients
    of a trailing partial group stay for nobody, as in the reference: the next epoch starts with zero_grad()).
    ``on_log({"iter", "global_iters", "loss"})`` is called at iterations 0, log_every, 2 log_every, ... with the mean
    loss since the previous call.  Returns {"iters", "loss"}: the count and the epoch's mean loss (one read at the end)."""
    model.train()
    optimizer.zero_grad()
    pending, total, n = [], 0.0, 0

    def drain():
        nonlocal pending, total
        values = torch.stack(pending).tolist() if pending else []       # the only device -> host read of the loop
        pending = []
        total += sum(values)
        return values

    for i, batch in enumerate(batches):
        loss, _ = clip_forward_backward(model, criterion, batch, device, use_dab=use_dab,
                                        accumulation_steps=accumulation_steps, no_grad_frames=no_grad_frames)
        pending.append(loss.detach())
        if (i + 1) % accumulation_steps == 0:
            optimizer_step(model, optimizer, max_norm)
        n += 1
        if i % log_every == 0:
            values = drain()
            if on_log is not None:
                on_log({"iter": i, "global_iters": states["global_iters"], "loss": sum(values) / len(values)})
        states["global_iters"] += 1
    drain()
    return {"iters": n, "loss": total / n if n else float("nan")}


def fit(config: dict, model, criterion, make_batches: Callable[[int], Iterable[dict]], *, device,
        outputs_dir: Optional[str] = None, impl: Optional[str] = None, log_every: int = 100,
        on_log: Optional[Callable[[dict], None]] = None):
    """train_engine.py:52-155.  ``make_batches(epoch)`` yields the epoch's batches in the collate format of
    ``data.clip_batch`` / ``engine.make_synthetic_clip``.  ``outputs_dir`` (default config["OUTPUTS_DIR"]; None: no
    checkpoints) receives checkpoint_{epoch}.pth in ``save_checkpoint``'s layout on the reference's cadence (:143-153:
    every epoch for DanceTrack or fewer than 100 epochs, else every fifth; none with MULTI_CHECKPOINT).  RESUME loads
    model and states; with RESUME_SCHEDULER also optimizer and scheduler, without it the scheduler is stepped
    start_epoch times.  ``impl`` goes to ``build_optimizer``.  Returns (optimizer, scheduler, states)."""
    if outputs_dir is None:
        outputs_dir = config.get("OUTPUTS_DIR")
    optimizer = build_optimizer(config, model, impl=impl)
    scheduler = build_scheduler(config, optimizer)
    states = {"start_epoch": 0, "global_iters": 0}
    if config.get("RESUME") is not None:
        if config.get("RESUME_SCHEDULER"):
            load_checkpoint(model=model, path=config["RESUME"], states=states, optimizer=optimizer,
                            scheduler=scheduler)
        else:
            load_checkpoint(model=model, path=config["RESUME"], states=states)
            for _ in range(states["start_epoch"]):
                scheduler.step()
    multi_checkpoint = bool(config.get("MULTI_CHECKPOINT"))
    for epoch in range(states["start_epoch"], config["EPOCHS"]):
        no_grad_frames = apply_epoch_policy(config, optimizer, epoch)
        summary = train_one_epoch(model, criterion, optimizer, make_batches(epoch), device=device,
                                  max_norm=config["CLIP_MAX_NORM"],
                                  accumulation_steps=config.get("ACCUMULATION_STEPS", 1),
                                  use_dab=config.get("USE_DAB", True), no_grad_frames=no_grad_frames, states=states,
                                  log_every=log_every, on_log=on_log)
        scheduler.step()
        states["start_epoch"] += 1
        if on_log is not None:
            on_log({"epoch": epoch, "global_iters": states["global_iters"], "loss": summary["loss"]})
        if outputs_dir is not None and not multi_checkpoint:
            if config["DATASET"] == "DanceTrack" or config["EPOCHS"] < 100 or (epoch + 1) % 5 == 0:
                os.makedirs(outputs_dir, exist_ok=True)
                save_checkpoint(model=model, path=os.path.join(outputs_dir, f"checkpoint_{epoch}.pth"),
                                states=states, optimizer=optimizer, scheduler=scheduler)
    return optimizer, scheduler, states


def train_from_config(config: dict, device=None, *, prefetch: int = 2, decode_threads: int = 2, shuffle: bool = True,
                      outputs_dir: Optional[str] = None, impl: Optional[str] = None, log_every: int = 100,
                      on_log: Optional[Callable[[dict], None]] = None):
    """train_engine.py:32-155 from a config alone: ``build_model``, ``build_criterion``, ``build_dataset`` on
    config["DATA_ROOT"], a ``ClipLoader`` seeded with config["SEED"] and ``fit(..., loader.epoch, ...)``.  When
    ``torch.distributed`` is initialised the loader takes this process's rank and the world size, and the model is
    wrapped in ``DistributedDataParallel`` as ``train_bench.py`` wraps it.  ``device`` defaults to the model's.
    Returns (model, optimizer, scheduler, states)."""
    import torch.distributed as dist

    from .data import ClipLoader, build_dataset
    from .models import build_model
    from .models.criterion import build as build_criterion
    model = build_model(config)
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    criterion = build_criterion(config)
    rank, world_size = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() \
        else (0, 1)
    if world_size > 1:
        from torch.nn.parallel import DistributedDataParallel as DDP
        model = DDP(model, device_ids=[device.index] if device.type == "cuda" else None,
                    find_unused_parameters=False, broadcast_buffers=False, gradient_as_bucket_view=True)
    dataset = build_dataset(config, split="train")
    loader = ClipLoader(dataset, device, seed=config["SEED"], shuffle=shuffle, rank=rank, world_size=world_size,
                        prefetch=prefetch, decode_threads=decode_threads)
    optimizer, scheduler, states = fit(config, model, criterion, loader.epoch, device=device, outputs_dir=outputs_dir,
                                       impl=impl, log_every=log_every, on_log=on_log)
    return model, optimizer, scheduler, states
