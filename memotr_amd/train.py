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
import time
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
                    states: dict, log_every: int = 100, on_log: Optional[Callable[[dict], None]] = None,
                    runlog=None, epoch: int = 0, n_iters: Optional[int] = None) -> dict:
    """train_engine.py:183-276: one clip per iteration, an optimizer step every ``accumulation_steps`` clips (gradients
    of a trailing partial group stay for nobody, as in the reference: the next epoch starts with zero_grad()).
    ``on_log({"iter", "global_iters", "loss"})`` is called at iterations 0, log_every, 2 log_every, ... with the mean
    loss since the previous call.  Returns {"iters", "loss"}: the count and the epoch's mean loss (one read at the end).

    ``runlog`` (a ``runlog.RunLog``; None: nothing below happens) turns the component log of train_engine.py:232-286 on:
    every clip's total loss and ``criterion.log_components()`` stay on the device as one vector and travel with the
    losses, in the same single read per log event; a ``MetricWindow`` of this epoch takes them and the host seconds of
    each iteration, and at every log event and at the end of ``epoch`` the reference's lines go to the console,
    ``log.txt`` and ``scalars.jsonl``.  ``n_iters``: the epoch's length for ``Iter=i/N`` and the remaining time."""
    model.train()
    optimizer.zero_grad()
    pending, total, n = [], 0.0, 0
    if runlog is not None:
        from .runlog import TIME, TOTAL, MetricWindow
        metrics, names, seconds, epoch_start = MetricWindow(), [], [], time.time()

    def drain():
        nonlocal pending, total
        if runlog is None:
            values = torch.stack(pending).tolist() if pending else []   # the only device -> host read of the loop
        else:       # the same one read: every clip's vector is (total loss, components ...)
            flat = torch.cat(pending).tolist() if pending else []
            values, at = [], 0
            for clip_names, spent in zip(names, seconds):
                values.append(flat[at])
                metrics.update(TOTAL, flat[at])
                for k, v in zip(clip_names, flat[at + 1:at + 1 + len(clip_names)]):
                    metrics.update(k, v)
                metrics.update(TIME, spent)
                at += 1 + len(clip_names)
            names.clear(), seconds.clear()
        pending = []
        total += sum(values)
        return values

    def report(i):
        metrics.sync(device if torch.device(device).type == "cuda" else None)
        of = "?" if n_iters is None else n_iters
        if i is None:
            head = f"[Epoch: {epoch}, Total Time: {int((time.time() - epoch_start) // 60)}min]"
            runlog.show(head=head, log=metrics)
            runlog.write(head=head, log=metrics)
            runlog.metric_scalars(metrics, step=epoch, mode="epochs")
            return
        per_iter = metrics.avg(TIME)
        rest = "?" if n_iters is None else int(per_iter * (n_iters - i) // 60)
        peak = torch.cuda.max_memory_allocated(device) // (1024 ** 2) if torch.device(device).type == "cuda" else 0
        runlog.show(head=f"[Epoch={epoch}, Iter={i}, {per_iter:.2f}s/iter, {i}/{of} iters, rest time: {rest} min, "
                         f"Max Memory={peak}MB]", log=metrics)
        runlog.write(head=f"[Epoch={epoch}, Iter={i}/{of}]", log=metrics)
        runlog.metric_scalars(metrics, step=states["global_iters"], mode="iters")

    for i, batch in enumerate(batches):
        started = time.time()
        loss, _ = clip_forward_backward(model, criterion, batch, device, use_dab=use_dab,
                                        accumulation_steps=accumulation_steps, no_grad_frames=no_grad_frames)
        if runlog is None:
            pending.append(loss.detach())
        else:
            clip_names, components = criterion.log_components()
            pending.append(torch.cat((loss.detach().reshape(1), components)))
            names.append(clip_names)
        if (i + 1) % accumulation_steps == 0:
            optimizer_step(model, optimizer, max_norm)
        n += 1
        if runlog is not None:
            seconds.append(time.time() - started)
        if i % log_every == 0:
            values = drain()
            if runlog is not None:
                report(i)
            if on_log is not None:
                on_log({"iter": i, "global_iters": states["global_iters"], "loss": sum(values) / len(values)})
        states["global_iters"] += 1
    drain()
    if runlog is not None and n:
        report(None)
    return {"iters": n, "loss": total / n if n else float("nan")}


def fit(config: dict, model, criterion, make_batches: Callable[[int], Iterable[dict]], *, device,
        outputs_dir: Optional[str] = None, impl: Optional[str] = None, log_every: int = 100,
        on_log: Optional[Callable[[dict], None]] = None, runlog=None,
        epoch_len: Optional[Callable[[int], int]] = None):
    """train_engine.py:52-155.  ``make_batches(epoch)`` yields the epoch's batches in the collate format of
    ``data.clip_batch`` / ``engine.make_synthetic_clip``.  ``outputs_dir`` (default config["OUTPUTS_DIR"]; None: no
    checkpoints) receives checkpoint_{epoch}.pth in ``save_checkpoint``'s layout on the reference's cadence (:143-153:
    every epoch for DanceTrack or fewer than 100 epochs, else every fifth; none with MULTI_CHECKPOINT).  RESUME loads
    model and states; with RESUME_SCHEDULER also optimizer and scheduler, without it the scheduler is stepped
    start_epoch times.  ``impl`` goes to ``build_optimizer``.  ``runlog`` (a ``runlog.RunLog``) receives the epoch's
    learning rates by group (:108-117) and goes on to ``train_one_epoch`` with ``epoch_len(epoch)``, the number of
    batches ``make_batches(epoch)`` will yield.  Returns (optimizer, scheduler, states)."""
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
        logging = {}
        if runlog is not None:
            from .runlog import lr_info
            lrs = [g["lr"] for g in optimizer.param_groups]
            runlog.show(head=f"[Epoch {epoch}] lr={lr_info(lrs)}")
            runlog.write(head=f"[Epoch {epoch}] lr={lr_info(lrs)}")
            runlog.scalar("lr", lrs[-1], step=epoch, mode="epochs")
            logging = dict(runlog=runlog, epoch=epoch, n_iters=None if epoch_len is None else epoch_len(epoch))
        summary = train_one_epoch(model, criterion, optimizer, make_batches(epoch), device=device,
                                  max_norm=config["CLIP_MAX_NORM"],
                                  accumulation_steps=config.get("ACCUMULATION_STEPS", 1),
                                  use_dab=config.get("USE_DAB", True), no_grad_frames=no_grad_frames, states=states,
                                  log_every=log_every, on_log=on_log, **logging)
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


def load_pretrained(config: dict, model) -> None:
    """train_engine.py:38-40: ``PRETRAINED_MODEL``, when not None, through ``load_pretrained_model`` (rank 0 loads; the
    DistributedDataParallel wrap broadcasts).  A missing file is an error that names the key."""
    path = config.get("PRETRAINED_MODEL")
    if path is None:
        return
    if not os.path.isfile(path):
        raise FileNotFoundError(f"PRETRAINED_MODEL: no such file '{path}' (the shipped configs start from the COCO "
                                f"weights of DAB-Deformable-DETR; give the file's path or set the key to None)")
    from .models.utils import load_pretrained_model
    load_pretrained_model(model, path, show_details=False)


def train_from_config(config: dict, device=None, *, prefetch: int = 2, decode_threads: int = 2, shuffle: bool = True,
                      outputs_dir: Optional[str] = None, impl: Optional[str] = None, log_every: int = 100,
                      on_log: Optional[Callable[[dict], None]] = None, model=None, dataset=None,
                      run_log: bool = False):
    """train_engine.py:32-155 from a config alone: ``build_model``, ``build_criterion``, ``build_dataset`` on
    config["DATA_ROOT"], a ``ClipLoader`` seeded with config["SEED"] and ``fit(..., loader.epoch, ...)``.  When
    ``torch.distributed`` is initialised the loader takes this process's rank and the world size, and the model is
    wrapped in ``DistributedDataParallel`` as ``train_bench.py`` wraps it.  ``device`` defaults to the model's.
    ``model`` / ``dataset``: used in place of ``build_model(config)`` / ``build_dataset(config)``.

    ``run_log`` (what ``python -m memotr_amd`` sets) makes it the reference's whole ``train()``: ``PRETRAINED_MODEL`` is
    loaded before RESUME is handled, rank 0 writes ``<OUTPUTS_DIR>/train/config.yaml`` (what ``submit`` and ``evaluate``
    read) before the first clip, and ``<OUTPUTS_DIR>/train`` receives ``log.txt`` and ``scalars.jsonl`` (runlog.py).
    Checkpoints stay where ``fit`` puts them.  Returns (model, optimizer, scheduler, states)."""
    import torch.distributed as dist

    from .data import ClipLoader, build_dataset
    from .models.criterion import build as build_criterion
    runlog = None
    if run_log:
        from .runlog import RunLog
        runlog = RunLog(os.path.join(outputs_dir if outputs_dir is not None else config["OUTPUTS_DIR"], "train"))
        runlog.show(head="Configs:", log=config)
        runlog.write_config(config)
    if model is None:
        from .models import build_model
        model = build_model(config)
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    if run_log:
        load_pretrained(config, model)
    criterion = build_criterion(config)
    rank, world_size = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() \
        else (0, 1)
    if world_size > 1:
        from torch.nn.parallel import DistributedDataParallel as DDP
        model = DDP(model, device_ids=[device.index] if device.type == "cuda" else None,
                    find_unused_parameters=False, broadcast_buffers=False, gradient_as_bucket_view=True)
    if dataset is None:
        dataset = build_dataset(config, split="train")
    loader = ClipLoader(dataset, device, seed=config["SEED"], shuffle=shuffle, rank=rank, world_size=world_size,
                        prefetch=prefetch, decode_threads=decode_threads)
    logging = {}
    if run_log:
        def epoch_len(epoch):
            dataset.set_epoch(epoch)
            return len(loader.order(epoch))
        logging = dict(runlog=runlog, epoch_len=epoch_len)
    optimizer, scheduler, states = fit(config, model, criterion, loader.epoch, device=device, outputs_dir=outputs_dir,
                                       impl=impl, log_every=log_every, on_log=on_log, **logging)
    return model, optimizer, scheduler, states
