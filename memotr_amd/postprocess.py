"""The offline pass over the result rows of a finished sequence: fill the holes of tracks that came back, drop tracks
that lived a few frames.

A track query stays alive for ``MISS_TOLERANCE`` frames after its score falls, but is reported only above
``RESULT_SCORE_THRESH``: a track that re-appears keeps its id and leaves a hole of unreported frames in the result
file.  ``fill_gaps`` is the definition of the pass, in numpy; the kernels behind ``ResultLog.filled`` /
``BankResultLog.filled`` (results.py, ``clipops_fill_gaps_f32`` in include/clip_ops_hip.h) are held to it bit for bit
(tests/test_postprocess_gpu.py).

    rows = fill_gaps(log.read(), max_gap=20, min_length=5)
    filled = log.filled(max_gap=20, min_length=5)           # the same rows, made where the log lives

``postprocess_options`` is what ``submit(..., postprocess=...)`` and MEMOTR_POSTPROCESS are read with.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from .results import Rows

OPTIONS = ("max_gap", "min_length")


def _check(max_gap: int, min_length: int) -> None:
    if int(max_gap) < 0 or int(min_length) < 0:
        raise ValueError(f"max_gap and min_length must not be negative, not {max_gap} and {min_length}")


def fill_gaps(rows: Rows, max_gap: int, min_length: int = 0) -> Rows:
    """The rows of one sequence with short tracks removed and short holes filled.

    1. ``(frame, id)`` pairs are unique (``ValueError`` otherwise).
    2. A track with fewer than ``min_length`` input rows is removed whole, and fills nothing.
    3. Two rows of an id at frames ``f0 < f1`` with no row of it between them and ``m = f1 - f0 - 1``,
       ``1 <= m <= max_gap``: a new row at every frame ``f0 + k``, ``k = 1 .. m``, with the id and the label of the row
       at ``f0`` and each of x1, y1, x2, y2 and the score equal to ``a + (b - a) * t``, ``t = float32(k) /
       float32(m + 1)``: four float32 operations, each rounded once.  Longer holes stay, nothing is extrapolated.
    4. The surviving input rows, bit-unchanged, and the new rows, sorted by (frame, id).
    """
    _check(max_gap, min_length)
    max_gap, min_length = int(max_gap), int(min_length)
    frames, ids, labels = (np.asarray(a, np.int64).reshape(-1) for a in (rows.frames, rows.ids, rows.labels))
    values = np.concatenate((np.asarray(rows.boxes_xyxy, np.float32).reshape(-1, 4),
                             np.asarray(rows.scores, np.float32).reshape(-1, 1)), axis=1)
    order = np.lexsort((frames, ids))                       # by id, then frame: a track's rows are adjacent
    frames, ids, labels, values = frames[order], ids[order], labels[order], values[order]
    same = ids[1:] == ids[:-1]
    if np.any(same & (frames[1:] == frames[:-1])):
        at = int(np.flatnonzero(same & (frames[1:] == frames[:-1]))[0])
        raise ValueError(f"result rows: frame {int(frames[at])} holds id {int(ids[at])} more than once")
    if min_length > 1 and len(ids):
        _, inverse, counts = np.unique(ids, return_inverse=True, return_counts=True)
        keep = counts[inverse] >= min_length
        frames, ids, labels, values = frames[keep], ids[keep], labels[keep], values[keep]
        same = ids[1:] == ids[:-1]
    missing = np.where(same, frames[1:] - frames[:-1] - 1, 0)
    left = np.flatnonzero((missing >= 1) & (missing <= max_gap))       # the row in front of every hole to fill
    if len(left):
        m = missing[left]
        src = np.repeat(left, m)
        k = np.arange(len(src)) - np.repeat(np.cumsum(m) - m, m) + 1
        t = (k.astype(np.float32) / (np.repeat(m, m) + 1).astype(np.float32))[:, None]
        a, b = values[src], values[src + 1]
        with np.errstate(invalid="ignore", over="ignore"):  # (a NaN or an infinite coordinate stays what it is)
            new = a + (b - a) * t                           # float32 throughout: a difference, a product, a sum
        assert new.dtype == np.float32 and t.dtype == np.float32
        frames = np.concatenate((frames, frames[src] + k))
        ids, labels = np.concatenate((ids, ids[src])), np.concatenate((labels, labels[src]))
        values = np.concatenate((values, new))
    order = np.lexsort((ids, frames))
    return Rows(frames[order], ids[order], labels[order], np.ascontiguousarray(values[order, :4]),
                values[order, 4].copy())


def postprocess_options(postprocess: Optional[dict] = None) -> Optional[dict]:
    """``submit``'s post-process setting: ``postprocess`` (a dict with ``max_gap`` and / or ``min_length``), or
    MEMOTR_POSTPROCESS="max_gap=20,min_length=5", or None -- the pass is off.  Returns None or a dict with both keys.
    Unknown keys are a ``TypeError``."""
    if postprocess is None:
        text = os.environ.get("MEMOTR_POSTPROCESS", "").strip()
        if not text:
            return None
        postprocess = {}
        for item in text.split(","):
            key, sep, value = item.partition("=")
            if not sep:
                raise ValueError(f"MEMOTR_POSTPROCESS: '{item}' is not key=value")
            postprocess[key.strip()] = int(value)
    unknown = set(postprocess) - set(OPTIONS)
    if unknown:
        raise TypeError(f"unknown postprocess options {sorted(unknown)}")
    out = dict(max_gap=int(postprocess.get("max_gap", 0)), min_length=int(postprocess.get("min_length", 0)))
    _check(out["max_gap"], out["min_length"])
    return out
