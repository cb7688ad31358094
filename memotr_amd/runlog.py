"""The run log of a training run: what the reference's ``log/log.py`` (``MetricLog``) and ``log/logger.py``
(``Logger``) keep, without a device-to-host read per clip and without a collective per metric.

``MetricWindow`` holds, per metric name, the last ``window`` values and a running total and count; ``avg`` is the mean
of the window and ``global_avg`` the total over the count (log.py:11-56).  Under ``torch.distributed`` ``sync()`` makes
both the means over all ranks -- the window mean over the union of the ranks' windows, the global mean over the summed
totals and counts -- with ONE all-reduce of a packed float64 vector (four numbers per metric); the reference gathers two
python objects per metric.  Host arithmetic is float64 throughout: the reference's window mean is a float32
``tensor.mean()``, so the last digits of a printed value may differ.

``RunLog`` writes, from rank 0 only, ``config.yaml``, ``log.txt`` (appended, the reference's lines) and
``scalars.jsonl``: one JSON object ``{"mode", "step", "tag", "value"}`` per line wherever the reference adds a
TensorBoard scalar (``mode`` "iters" or "epochs" names the reference's two writers).
"""
from __future__ import annotations

import json
import os
from collections import deque
from typing import Dict, Iterable, List, Optional

import torch
import torch.distributed as dist

TIME = "time per iter"          # log.py:82: recorded like a metric, left out of the printed line
TOTAL = "total_loss"
LR_NAMES = ("lr_backbone", "lr_points", "lr_query_updater", "lr")       # the four groups of engine.get_param_groups


def _distributed() -> bool:
    return dist.is_available() and dist.is_initialized()


class _Series:
    __slots__ = ("values", "total", "count")

    def __init__(self, window: int):
        self.values = deque(maxlen=window)
        self.total = 0.0
        self.count = 0


class MetricWindow:
    def __init__(self, window: int = 100):
        if window < 1:
            raise ValueError("window must be at least 1")
        self.window = int(window)
        self.metrics: Dict[str, _Series] = {}
        self._synced: Optional[Dict[str, tuple]] = None     # name -> (window sum, window length, total, count)

    def update(self, name: str, value: float) -> None:
        s = self.metrics.get(name)
        if s is None:
            s = self.metrics[name] = _Series(self.window)
        value = float(value)
        s.values.append(value)
        s.total += value
        s.count += 1
        self._synced = None

    def sync(self, device=None) -> None:
        """Fix the numbers that ``avg`` / ``global_avg`` report until the next ``update``.  Under ``torch.distributed``
        every rank must call it, with the same metric names in the same order (ranks whose clips have the same number of
        frames: the datasets draw one clip length per epoch); ``device`` is where the all-reduced vector lives (the
        backend's: this rank's GPU for nccl, the host for gloo)."""
        names = list(self.metrics)
        packed = []
        for n in names:
            s = self.metrics[n]
            packed += [sum(s.values), float(len(s.values)), s.total, float(s.count)]
        if _distributed() and dist.get_world_size() > 1 and packed:
            t = torch.tensor(packed, dtype=torch.float64, device=device if device is not None else "cpu")
            dist.all_reduce(t)
            packed = t.tolist()
        self._synced = {n: tuple(packed[4 * i:4 * i + 4]) for i, n in enumerate(names)}

    def _get(self, name: str) -> tuple:
        if self._synced is None:
            raise RuntimeError("Be sure to use .sync() before metric statistic.")
        return self._synced[name]

    def avg(self, name: str) -> float:
        window_sum, window_len, _, _ = self._get(name)
        return window_sum / window_len

    def global_avg(self, name: str) -> float:
        _, _, total, count = self._get(name)
        return total / count

    def get(self, name: str, mode: str) -> float:
        return {"avg": self.avg, "global_avg": self.global_avg}[mode](name)

    def __str__(self) -> str:
        """``MetricLog.__str__`` (log.py:77-87): the total loss first, then every metric but the time, as
        ``name = window mean (global mean); ``."""
        s = ""
        if TOTAL in self.metrics:
            s += f"loss = {self.avg(TOTAL):.4f} ({self.global_avg(TOTAL):.4f}); "
        for name in self.metrics:
            if name in (TIME, TOTAL):
                continue
            s += f"{name} = {self.avg(name):.4f} ({self.global_avg(name):.4f}); "
        return s


def lr_info(lrs: Iterable[float], names: Iterable[str] = LR_NAMES) -> List[dict]:
    """train_engine.py:108-110: one ``{name: lr}`` per parameter group."""
    lrs, names = list(lrs), list(names)
    assert len(lrs) == len(names)
    return [{name: lr} for name, lr in zip(names, lrs)]


class RunLog:
    """``Logger`` of the reference for ``<OUTPUTS_DIR>/train``: nothing is written (and no directory made) on a rank
    other than 0 unless ``only_main`` is False."""

    def __init__(self, logdir: str, only_main: bool = True):
        rank = dist.get_rank() if _distributed() else 0
        self.active = (rank == 0) or not only_main
        self.logdir = logdir if self.active else None
        if self.active:
            os.makedirs(logdir, exist_ok=True)

    def show(self, head: str = "", log="") -> None:
        if self.active:
            print(f"{head} {log}", flush=True)

    def write(self, head: str = "", log="", filename: str = "log.txt") -> None:
        if self.active:
            with open(os.path.join(self.logdir, filename), "a") as f:
                f.write(f"{head} {log}\n")

    def write_config(self, config: dict, filename: str = "config.yaml") -> None:
        """The merged config as ``yaml.dump`` writes it (logger.py:97-108); ``configs.load_yaml`` returns an equal
        dict."""
        if self.active:
            import yaml
            with open(os.path.join(self.logdir, filename), "w") as f:
                yaml.dump(config, f, allow_unicode=True)

    def scalar(self, tag: str, value: float, step: int, mode: str) -> None:
        if self.active:
            with open(os.path.join(self.logdir, "scalars.jsonl"), "a") as f:
                f.write(json.dumps({"mode": mode, "step": int(step), "tag": tag, "value": float(value)}) + "\n")

    def metric_scalars(self, metrics: MetricWindow, step: int, mode: str) -> None:
        """``tb_add_metric_log`` (logger.py:137-182): window means for "iters", global means for "epochs"; the three
        component families as ``<component>/frame<i>`` (``add_scalars``' sub-tags), then ``loss``."""
        if not self.active:
            return
        which = "avg" if mode == "iters" else "global_avg"
        for family in ("box_l1_loss", "box_giou_loss", "label_focal_loss"):
            for name in metrics.metrics:
                if family in name:
                    self.scalar(f"{family}/{name.split('_')[0]}", metrics.get(name, which), step, mode)
        if TOTAL in metrics.metrics:
            self.scalar("loss", metrics.get(TOTAL, which), step, mode)
