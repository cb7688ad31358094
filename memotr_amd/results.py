"""The result rows of a tracked sequence, kept on the device until the sequence ends.

``SequenceTracker._report`` brings the reportable tracks of every frame to the host: a packed copy through a pinned
buffer and an event wait per frame.  A submit run needs none of them per frame -- it needs the rows of the whole
sequence once.  ``ResultLog`` is that table: ``append`` is one launch of ``clipops_result_rows_f32``
(include/clip_ops_hip.h: score and area filter, xyxy pixel boxes, ballot compaction onto the end of the table),
``read`` one synchronisation and one copy.  ``BankResultLog`` is the same table for sequences tracked side by side;
the tables, their growth, ``reset`` and the packed, validated read are ``_RowTable``'s for both.

    log = ResultLog(device)
    n_frames = tracker.track_logged(paths, log)
    lines = log.mot_lines("DanceTrack")          # what tracker.mot_lines gives frame by frame
    log.reset()                                   # next sequence

On CPU tensors ``append`` runs ``host_rows``, the torch statement the kernel is held to (tests/test_result_log_gpu.py).

``filled`` of either log gives a new log with the offline pass of postprocess.py applied (short tracks removed, holes
of a few frames interpolated), made on the device from the tables as they stand; the writers are the same.
"""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np
import torch

from .utils.host import to_host

ROW_F, ROW_I = 5, 3           # x1, y1, x2, y2, score | frame, id, label
BANK_ROW_I = 4                # sequence, frame, id, label


class Rows(NamedTuple):
    frames: np.ndarray        # (m,) int64, 0-based
    ids: np.ndarray           # (m,) int64
    labels: np.ndarray        # (m,) int64
    boxes_xyxy: np.ndarray    # (m, 4) float32, pixels of the original image
    scores: np.ndarray        # (m,) float32


def host_rows(boxes: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor, labels: torch.Tensor, frame_idx: int,
              ori_h, ori_w, score_thresh: float, area_thresh: float):
    """``_report``'s filter and boxes in float32 (submit_engine.py:95-112): ``(rows_f (m,5), rows_i (m,3))`` of the
    kept rows in input order.  Thresholds and image sizes meet the float32 tensors as Python scalars, so torch rounds
    them to float32 first."""
    n = boxes.shape[0]
    if n == 0:
        return boxes.new_zeros((0, ROW_F), dtype=torch.float32), ids.new_zeros((0, ROW_I), dtype=torch.int64)
    boxes, scores = boxes.float(), scores.float().reshape(n, -1)
    s = torch.max(scores, dim=-1).values
    area = boxes[:, 2] * float(ori_w) * boxes[:, 3] * float(ori_h)
    keep = (s > score_thresh) & (area > area_thresh)
    b, half_w, half_h = boxes[keep], 0.5 * boxes[keep][:, 2], 0.5 * boxes[keep][:, 3]
    rows_f = torch.stack(((b[:, 0] - half_w) * float(ori_w), (b[:, 1] - half_h) * float(ori_h),
                          (b[:, 0] + half_w) * float(ori_w), (b[:, 1] + half_h) * float(ori_h), s[keep]), dim=1)
    rows_i = torch.stack((torch.full_like(ids[keep], int(frame_idx)), ids[keep], labels[keep]), dim=1)
    return rows_f, rows_i


def _raise_for_status(status: int) -> None:
    """The status word of ``clipops_fill_gaps_f32`` (CLIPOPS_FG_* in include/clip_ops_hip.h) as an error."""
    if status == 0:
        return
    said = [text for bit, text in ((1, "a duplicate (frame, id)"), (2, "an id out of range (outside 0 .. n_ids - 1)"),
                                   (4, "a frame out of range (outside 0 .. n_frames - 1)"),
                                   (8, "a sequence out of range (outside 0 .. n_sequences - 1)")) if status & bit]
    raise RuntimeError("result log: the rows cannot be filled: " + "; ".join(said or [f"status {status}"]))


class _RowTable:
    """``rows_f`` (capacity, 5) float32, ``rows_i`` (capacity, ``WIDTH_I``) int64 and ``counters`` (2,) int32 (rows
    stored, rows dropped for lack of room) on ``device``, the bound on the rows in use and the last read.  A log adds
    ``WIDTH_I``, ``append`` and ``_as_rows``.  All calls on one log are made on one stream."""

    def __init__(self, device, capacity: int = 4096):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity = max(1, int(capacity))
        self.rows_f = torch.empty((self.capacity, ROW_F), dtype=torch.float32, device=self.device)
        self.rows_i = torch.empty((self.capacity, self.WIDTH_I), dtype=torch.int64, device=self.device)
        self.counters = torch.zeros((2,), dtype=torch.int32, device=self.device)
        self._bound = 0           # the rows appended can be no more than the rows offered: known without a read
        self._rows = None         # the last read, until the next append / reset
        self.status = None        # of a log made by ``filled`` on the device: (1,) int32, what the kernels objected to

    def _make_room(self, offered: int) -> None:
        """Before an append of at most ``offered`` rows (the caller then adds them to ``_bound``)."""
        self._rows = None
        if self._bound + offered > self.capacity:
            self._grow(self._bound + offered)

    def _grow(self, needed: int) -> None:
        """Larger tables and a stream-ordered device copy of the part that may be in use."""
        capacity = max(2 * self.capacity, needed)
        rows_f = torch.empty((capacity, ROW_F), dtype=torch.float32, device=self.device)
        rows_i = torch.empty((capacity, self.WIDTH_I), dtype=torch.int64, device=self.device)
        rows_f[:self._bound].copy_(self.rows_f[:self._bound])
        rows_i[:self._bound].copy_(self.rows_i[:self._bound])
        if self.device.type == "cuda":        # the old tables are read by that copy on this stream
            stream = torch.cuda.current_stream(self.device)
            self.rows_f.record_stream(stream)
            self.rows_i.record_stream(stream)
        self.rows_f, self.rows_i, self.capacity = rows_f, rows_i, capacity

    def reset(self) -> None:
        """Empty the log for the next sequence (stream-ordered; the tables keep their size)."""
        self.counters.zero_()
        self._bound, self._rows, self.status = 0, None, None

    def read(self):
        """The rows on the host (``_as_rows`` of the stored part of the tables): one packed copy through a pinned buffer
        and one event wait (``utils.host.to_host``)."""
        if self._rows is not None:
            return self._rows
        b, w = self._bound, self.WIDTH_I
        if self.status is not None and b > 0:
            # a filled log: its bound is the room it was given, far above the rows stored, so the counters and the
            # status word come first (a second small read) and the copy below takes the stored rows only
            head = to_host(torch.cat((self.counters, self.status))).numpy()
            _raise_for_status(int(head[2]))
            b = self._bound = min(b, max(int(head[0]), 0))
        if self.device.type == "cuda":
            raw = to_host(torch.cat((self.counters.view(torch.uint8), self.rows_i[:b].reshape(-1).view(torch.uint8),
                                     self.rows_f[:b].reshape(-1).view(torch.uint8)))).numpy()
            counters = raw[:8].view(np.int32)
            rows_i = raw[8:8 + b * w * 8].view(np.int64).reshape(b, w)
            rows_f = raw[8 + b * w * 8:].view(np.float32).reshape(b, ROW_F)
        else:
            counters, rows_i, rows_f = self.counters.numpy(), self.rows_i[:b].numpy(), self.rows_f[:b].numpy()
        stored, dropped = int(counters[0]), int(counters[1])
        if dropped != 0:
            raise RuntimeError(f"result log: {dropped} rows found no room in a table of {self.capacity}")
        if stored > b:
            raise RuntimeError(f"result log: {stored} rows stored, {b} offered (counters written from elsewhere?)")
        self._rows = self._as_rows(rows_i[:stored], rows_f[:stored])
        return self._rows

    def _like(self, capacity: int):
        """An empty log of this class on this device."""
        return type(self)(self.device, capacity)

    def _extent(self):
        """``(n_sequences, n_frames, n_ids)`` of the stored rows -- the largest of each column plus one, 0 without a
        row: one small read (three numbers; the stored count stays on the device)."""
        w = self.WIDTH_I
        if self._bound == 0:
            return 0, 0, 0
        stored = self.counters[0].clamp(0, self._bound)
        valid = torch.arange(self._bound, device=self.device) < stored
        top = to_host(torch.where(valid[:, None], self.rows_i[:self._bound], -1).amax(dim=0)).tolist()
        return (int(top[0]) + 1 if w == BANK_ROW_I else 1), int(top[w - 3]) + 1, int(top[w - 2]) + 1

    def _filled(self, max_gap: int, min_length: int, n_seq, n_frames, n_ids):
        """``filled`` of both logs on a CUDA device: ``clipops_fill_gaps_f32`` (include/clip_ops_hip.h) from these
        tables into those of a new log.  The new log's room is what the pass can give at most -- every cell of the
        ``n_seq * n_ids * n_frames`` table, or every offered row with ``max_gap`` new ones behind it."""
        from . import _clip_lib as L      # no substitute: a missing library is an error
        max_gap, min_length = int(max_gap), int(min_length)
        if max_gap < 0 or min_length < 0:
            raise ValueError(f"max_gap and min_length must not be negative, not {max_gap} and {min_length}")
        if self._bound == 0:
            return self._like(1)
        if n_seq is None or n_frames is None or n_ids is None:
            seen = self._extent()
            n_seq, n_frames, n_ids = (s if given is None else int(given) for s, given in zip(seen, (n_seq, n_frames, n_ids)))
        n_seq, n_frames, n_ids = int(n_seq), int(n_frames), int(n_ids)
        if min(n_seq, n_frames, n_ids) < 0:
            raise ValueError(f"negative table size: {n_seq} sequences, {n_frames} frames, {n_ids} ids")
        words = L.lib.clipops_fill_gaps_workspace(n_seq, n_ids, n_frames)
        if words < 0:
            raise ValueError(f"result log: {n_seq} sequences x {n_ids} ids x {n_frames} frames are more than 2^31 - 1 cells")
        new = self._like(max(1, min(n_seq * n_ids * n_frames, self._bound * (1 + max_gap))))
        new.status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        workspace = torch.empty((max(1, words),), dtype=torch.int32, device=self.device)
        L.check(L.lib.clipops_fill_gaps_f32(
            self.rows_f.data_ptr(), self.rows_i.data_ptr(), self.counters.data_ptr(), self._bound, self.WIDTH_I, n_seq,
            n_ids, n_frames, max_gap, min_length, workspace.data_ptr(), new.rows_f.data_ptr(), new.rows_i.data_ptr(),
            new.counters.data_ptr(), new.status.data_ptr(), new.capacity,
            torch.cuda.current_stream(self.device).cuda_stream), "clipops_fill_gaps_f32")
        new._bound = new.capacity
        return new

    def _store(self, rows_i: np.ndarray, rows_f: np.ndarray) -> None:
        """Host rows into the tables of this (CPU, empty) log."""
        m = rows_i.shape[0]
        self._make_room(m)
        self.rows_i[:m], self.rows_f[:m] = torch.from_numpy(rows_i), torch.from_numpy(rows_f)
        self.counters[0] = m
        self._bound = m


def _check_extent(rows: Rows, n_frames, n_ids) -> None:
    """What the kernels' status word says of rows outside the table a caller named, for a CPU log."""
    status = 0
    if n_ids is not None and len(rows.ids) and (rows.ids.min() < 0 or rows.ids.max() >= int(n_ids)):
        status |= 2
    if n_frames is not None and len(rows.frames) and (rows.frames.min() < 0 or rows.frames.max() >= int(n_frames)):
        status |= 4
    _raise_for_status(status)


class _SequenceRows:
    """The ``Rows`` of one sequence (``read()``) and what is written from them: a sequence of a ``BankResultLog`` as
    it stands, and the writers of ``ResultLog``, whose ``read`` is the table's."""

    def __init__(self, rows: Rows):
        self._rows = rows

    def read(self) -> Rows:
        return self._rows

    def __len__(self) -> int:
        return len(self.read().frames)

    def mot_lines(self, dataset_name: str) -> List[str]:
        """``SequenceTracker.mot_lines`` of every frame, in order: ``frame+1,id,x1,y1,w,h,1,-1,-1,-1`` with ``w`` and
        ``h`` formed in Python floats from the float32 corners."""
        from .inference import MOT_STYLE
        if dataset_name not in MOT_STYLE:
            raise ValueError(f"{dataset_name} dataset is not supported for submit process.")
        r = self.read()
        return [f"{f + 1},{tid},{x1},{y1},{x2 - x1},{y2 - y1},1,-1,-1,-1\n"
                for f, tid, (x1, y1, x2, y2) in zip(r.frames.tolist(), r.ids.tolist(), r.boxes_xyxy.tolist())]

    def _by_frame(self):
        """``{frame: slice of the rows}``: the rows of a frame are adjacent, frames ascend."""
        frames = self.read().frames
        starts = np.flatnonzero(np.diff(frames, prepend=-1))
        ends = list(starts[1:]) + [len(frames)]
        return {int(frames[a]): slice(int(a), int(e)) for a, e in zip(starts, ends)}

    def bdd_frames(self, image_paths) -> List[dict]:
        """``SequenceTracker.bdd_frame_result`` of every frame of the sequence, frames without a row included."""
        from .inference import BDD_CLS2LABEL
        r, where = self.read(), self._by_frame()
        out = []
        for idx, img_path in enumerate(image_paths):
            name = str(img_path).split("/")[-1]
            sl = where.get(idx, slice(0, 0))
            labels = [{"id": str(tid), "category": BDD_CLS2LABEL[lab + 1],
                       "box2d": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}}
                      for tid, lab, (x1, y1, x2, y2) in zip(r.ids[sl].tolist(), r.labels[sl].tolist(),
                                                            r.boxes_xyxy[sl].tolist())]
            out.append({"name": name, "videoName": name[:-12], "frameIndex": idx, "labels": labels})
        return out

    def add_to(self, evaluator, seq: str, n_frames: int = None) -> None:
        """Feed a ``TrackingEvaluator`` what ``add_frame`` would have been given frame by frame: 1-based frames, xywh
        boxes as the doubles ``mot_lines`` prints.  ``n_frames``: frames 0 .. n_frames - 1 are all added (empty ones
        too, as ``add_frame`` adds them); default: up to the last frame with a row."""
        r, where = self.read(), self._by_frame()
        if n_frames is None:
            n_frames = max(where) + 1 if where else 0
        for idx in range(n_frames):
            sl = where.get(idx, slice(0, 0))
            boxes = [[x1, y1, x2 - x1, y2 - y1] for x1, y1, x2, y2 in r.boxes_xyxy[sl].tolist()]
            evaluator.add_tracker_rows(seq, idx + 1, np.asarray(r.ids[sl].tolist(), np.int64),
                                       np.asarray(boxes, np.float64).reshape(-1, 4))


class ResultLog(_RowTable, _SequenceRows):
    """The table of one sequence: ``rows_i`` = frame, id, label; ``read`` gives ``Rows`` in the order appended."""
    WIDTH_I = ROW_I

    @torch.no_grad()
    def append(self, boxes: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor, labels: torch.Tensor,
               frame_idx: int, ori_h, ori_w, score_thresh: float, area_thresh: float) -> None:
        """The reportable rows of one frame's live tracks (``boxes`` (n,4) cxcywh normalised, ``scores`` (n,K) or (n,),
        ``ids`` / ``labels`` (n,)) behind the rows already there.  Nothing is read back."""
        n = int(boxes.shape[0])
        if n == 0:
            return
        if boxes.device != self.device:
            raise ValueError(f"tracks on {boxes.device}, result log on {self.device}")
        self._make_room(n)
        if self.device.type != "cuda":
            rows_f, rows_i = host_rows(boxes, scores, ids, labels, frame_idx, ori_h, ori_w, score_thresh, area_thresh)
            at, m = int(self.counters[0]), rows_f.shape[0]
            self.rows_f[at:at + m], self.rows_i[at:at + m] = rows_f, rows_i
            self.counters[0] += m
            self._bound += n
            return
        from . import _clip_lib as L      # no substitute: a missing library is an error
        boxes = boxes.detach().float().contiguous()
        scores = scores.detach().float().reshape(n, -1).contiguous()
        ids, labels = ids.long().contiguous(), labels.long().contiguous()
        L.check(L.lib.clipops_result_rows_f32(
            boxes.data_ptr(), scores.data_ptr(), ids.data_ptr(), labels.data_ptr(), n, scores.shape[1], int(frame_idx),
            float(ori_w), float(ori_h), float(score_thresh), float(area_thresh), self.rows_f.data_ptr(),
            self.rows_i.data_ptr(), self.counters.data_ptr(), self.capacity,
            torch.cuda.current_stream(self.device).cuda_stream), "clipops_result_rows_f32")
        self._bound += n

    @staticmethod
    def _as_rows(rows_i, rows_f) -> Rows:
        return Rows(rows_i[:, 0].copy(), rows_i[:, 1].copy(), rows_i[:, 2].copy(),
                    np.ascontiguousarray(rows_f[:, :4]), rows_f[:, 4].copy())

    @torch.no_grad()
    def filled(self, max_gap: int, min_length: int = 0, n_frames: int = None, n_ids: int = None) -> "ResultLog":
        """A new log on the same device with the offline pass of postprocess.py applied: tracks of fewer than
        ``min_length`` rows removed, holes of at most ``max_gap`` frames filled by linear interpolation, rows sorted by
        (frame, id).  This log stays as it is.  For a finished sequence: nothing here is called per frame.  On a CUDA
        device the rows never leave it (``clipops_fill_gaps_f32``); ``n_frames`` and ``n_ids`` size its cell table --
        every frame is below ``n_frames`` and every id below ``n_ids`` (``track_logged``'s return value and
        ``tracker.tracker.max_obj_id``).  Where both are passed nothing is read back; otherwise one small read finds
        them.  What the kernels object to (a duplicate (frame, id), an id or a frame out of range) is raised by the new
        log's ``read()``.  A CPU log runs the host statement, ``postprocess.fill_gaps``, at once."""
        if self.device.type == "cuda":
            return self._filled(max_gap, min_length, 1, n_frames, n_ids)
        from .postprocess import fill_gaps
        rows = self.read()
        _check_extent(rows, n_frames, n_ids)
        r = fill_gaps(rows, max_gap, min_length)
        new = self._like(max(1, len(r.frames)))
        new._store(np.stack((r.frames, r.ids, r.labels), axis=1), np.concatenate((r.boxes_xyxy, r.scores[:, None]), axis=1))
        return new


class BankResultLog(_RowTable):
    """The table of sequences tracked side by side (inference_multi.MultiSequenceTracker): one table for all of
    them, ``rows_i`` (capacity, 4) = sequence, frame, id, label.  ``append`` is one launch of
    ``clipops_bank_result_rows_f32`` over every stream of a ``TrackBank``; which sequence and frame a stream is at and
    the size of its images come from two small device arrays, so the launch is the same every frame.  ``read`` gives
    ``{sequence: Rows}``, each sequence's rows sorted by (frame, id) -- the order of the one-sequence tracker, whose
    tracks are in birth order."""

    WIDTH_I = BANK_ROW_I

    def __init__(self, device, capacity: int = 4096, dataset_name: str = "DanceTrack"):
        super().__init__(device, capacity)
        self.dataset_name = dataset_name

    @torch.no_grad()
    def append(self, bank, seq_frame: torch.Tensor, ori_wh: torch.Tensor, score_thresh: float,
               area_thresh: float) -> None:
        """The reportable rows of every stream's live tracks; ``seq_frame`` int64 (B, 2) = (sequence, frame) and
        ``ori_wh`` float32 (B, 2) = (ori_w, ori_h) of each stream, on the device.  Nothing is read back: the table grows
        by the number of slots offered."""
        from .functions.clip_ops import bank_result_rows
        if bank.ids.device != self.device:
            raise ValueError(f"track bank on {bank.ids.device}, result log on {self.device}")
        offered = bank.n_streams * bank.cap
        self._make_room(offered)
        bank_result_rows(bank, seq_frame, ori_wh, score_thresh, area_thresh, self.rows_f, self.rows_i, self.counters)
        self._bound += offered

    @torch.no_grad()
    def append_streams(self, bank, seq_frame: torch.Tensor, ori_wh: torch.Tensor, thresholds) -> None:
        """``append`` with stream b filtered by setting b of ``thresholds`` (clip_ops.StreamThresholds): one launch of
        ``clipops_bank_result_rows_streams_f32``.  In a threshold sweep every stream tracks the same sequence, and the
        "sequence" column of ``seq_frame`` is the setting's index."""
        from .functions.clip_ops import bank_result_rows_streams
        if bank.ids.device != self.device:
            raise ValueError(f"track bank on {bank.ids.device}, result log on {self.device}")
        offered = bank.n_streams * bank.cap
        self._make_room(offered)
        bank_result_rows_streams(bank, seq_frame, ori_wh, thresholds, self.rows_f, self.rows_i, self.counters)
        self._bound += offered

    @staticmethod
    def _as_rows(rows_i, rows_f) -> dict:
        out = {}
        for seq in np.unique(rows_i[:, 0]).tolist():
            pick = np.flatnonzero(rows_i[:, 0] == seq)
            pick = pick[np.lexsort((rows_i[pick, 2], rows_i[pick, 1]))]
            out[int(seq)] = Rows(rows_i[pick, 1].copy(), rows_i[pick, 2].copy(), rows_i[pick, 3].copy(),
                                 np.ascontiguousarray(rows_f[pick, :4]), rows_f[pick, 4].copy())
        return out

    def _like(self, capacity: int):
        return type(self)(self.device, capacity, self.dataset_name)

    @torch.no_grad()
    def filled(self, max_gap: int, min_length: int = 0, n_frames: int = None, n_ids: int = None,
               n_sequences: int = None) -> "BankResultLog":
        """``ResultLog.filled`` for every sequence of the table at once, each sequence on its own: a new log whose
        ``read()`` gives ``postprocess.fill_gaps`` of every sequence's ``Rows`` (a sequence that loses all its tracks
        has no entry).  ``n_frames``: above every frame of every sequence; ``n_ids``: above every id;
        ``n_sequences``: above every sequence number.  Where all three are passed nothing is read back."""
        if self.device.type == "cuda":
            return self._filled(max_gap, min_length, n_sequences, n_frames, n_ids)
        from .postprocess import fill_gaps
        parts_i, parts_f = [np.zeros((0, BANK_ROW_I), np.int64)], [np.zeros((0, ROW_F), np.float32)]
        for seq, rows in sorted(self.read().items()):
            if n_sequences is not None and not 0 <= seq < int(n_sequences):
                _raise_for_status(8)
            _check_extent(rows, n_frames, n_ids)
            r = fill_gaps(rows, max_gap, min_length)
            parts_i.append(np.stack((np.full_like(r.frames, seq), r.frames, r.ids, r.labels), axis=1))
            parts_f.append(np.concatenate((r.boxes_xyxy, r.scores[:, None]), axis=1))
        rows_i, rows_f = np.concatenate(parts_i), np.concatenate(parts_f)
        new = self._like(max(1, rows_i.shape[0]))
        new._store(rows_i, rows_f)
        return new

    def sequence(self, seq: int) -> _SequenceRows:
        """The rows of sequence ``seq`` behind ``ResultLog``'s writers (a sequence without a row: an empty log)."""
        rows = self.read().get(int(seq))
        if rows is None:
            rows = Rows(np.zeros((0,), np.int64), np.zeros((0,), np.int64), np.zeros((0,), np.int64),
                        np.zeros((0, 4), np.float32), np.zeros((0,), np.float32))
        return _SequenceRows(rows)

    def mot_lines(self, seq: int, dataset_name: str = None) -> List[str]:
        return self.sequence(seq).mot_lines(self.dataset_name if dataset_name is None else dataset_name)

    def bdd_frames(self, seq: int, image_paths) -> List[dict]:
        return self.sequence(seq).bdd_frames(image_paths)

    def add_to(self, evaluator, seq: int, name: str, n_frames: int = None) -> None:
        self.sequence(seq).add_to(evaluator, name, n_frames)
