"""Motion post-process of the online tracker (the reference's ``USE_MOTION``: models/motion.py,
models/runtime_tracker.py:43-54,81-94, submit_engine.py:78-87) on device-resident state.

The reference keeps a ``Dict[int, Motion]`` of per-track CPU tensors and reads ``.item()`` / ``.cpu()`` per track and
frame.  Here the whole bookkeeping is a table keyed by track id (ids are dense: the tracker hands them out from 0
upward, so the history of track ``id`` is row ``id``, whatever row order the query updater leaves) and three
operations on it, each ONE launch on CUDA tensors (memotr_amd/csrc/track_motion.hip, C ABI in
include/track_motion_hip.h):

    observe      the existing-track loop: age or refresh every track, push a seen track's box, retire
    register     newborn ids: count = 1, first box
    extrapolate  a missed track's reference point moves along its mean box velocity (out of place)

Nothing in this module synchronises with the device: no ``.item()``, ``.tolist()``, ``.cpu()`` and no boolean
indexing, on either path; the frame loop keeps its one ``nonzero``.  Each operation has a HOST STATEMENT in torch ops,
which runs when the tensors are CPU tensors, is bit-equal to the reference there (tests/test_motion_cpu.py) and is
what the kernels are checked against (tests/test_motion_gpu.py).  CUDA tensors take the kernels; a missing library is
an error.

Preconditions: ids are unique within a call; operations on one ``MotionState`` are issued on one stream; labels are
inside ``0 .. K - 1``.
"""
from __future__ import annotations

import torch

from ..utils.utils import inverse_sigmoid_reference

MAX_LENGTH = 16         # TRACKMOTION_MAX_LENGTH


def _f32(x: torch.Tensor, name: str, cols: int) -> torch.Tensor:
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != cols:
        raise TypeError(f"{name}: expected a float32 (n, {cols}) tensor, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def _i64(x: torch.Tensor, name: str, n: int) -> torch.Tensor:
    if x.dtype != torch.int64 or x.dim() != 1 or x.shape[0] != n:
        raise TypeError(f"{name}: expected an int64 ({n},) tensor, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


class MotionState:
    """The last ``max_length`` boxes of every track id, while the track is seen.

    ``boxes (capacity, L, 4)`` float32, oldest first, and ``count (capacity,)`` int32; entries at and past
    ``count[id]`` are stale.  ``capacity`` doubles (allocate, copy on the current stream) when ``register`` is handed
    ids past it; the host knows ``first_id + n_new`` without a synchronisation.  NOTHING IS EVER PRUNED: a retired id
    keeps its row, 16 L + 4 bytes per id ever handed out (84 B at L = 5; a million ids are 84 MB).

    ``status`` is a device word the kernels OR bits into when a row cannot be served (an id below 0 or past the
    table, a label outside the scores); ``check()`` reads it -- a synchronisation, so the frame loop never calls it.
    """

    def __init__(self, max_length: int, min_length: int, device, capacity: int = 1024):
        if min_length < 2:
            raise ValueError(f"min_length = {min_length}: the mean velocity is over count - 1 >= 1 steps, so >= 2")
        if min_length > max_length:
            raise ValueError(f"min_length = {min_length} > max_length = {max_length}: no track would ever qualify")
        if max_length > MAX_LENGTH:
            raise ValueError(f"max_length = {max_length} > {MAX_LENGTH}")
        if capacity < 1:
            raise ValueError(f"capacity = {capacity}")
        self.max_length, self.min_length = int(max_length), int(min_length)
        self.capacity = int(capacity)
        device = torch.device(device)
        # one row more than the table: where the host statement parks the writes of rows it skips
        self._boxes = torch.zeros((self.capacity + 1, self.max_length, 4), dtype=torch.float32, device=device)
        self.device = self._boxes.device                    # ("cuda" -> "cuda:0": compared with the tensors of a call)
        self._count = torch.zeros((self.capacity + 1,), dtype=torch.int32, device=self.device)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.device)

    @property
    def boxes(self) -> torch.Tensor:
        return self._boxes[:self.capacity]

    @property
    def count(self) -> torch.Tensor:
        return self._count[:self.capacity]

    # ------------------------------------------------------------------ table
    def reserve(self, n_ids: int) -> None:
        """Room for ids ``0 .. n_ids - 1``: the doubled table, copied on the current stream."""
        if n_ids <= self.capacity:
            return
        capacity = self.capacity
        while capacity < n_ids:
            capacity *= 2
        boxes = torch.zeros((capacity + 1, self.max_length, 4), dtype=torch.float32, device=self.device)
        count = torch.zeros((capacity + 1,), dtype=torch.int32, device=self.device)
        boxes[:self.capacity].copy_(self.boxes)
        count[:self.capacity].copy_(self.count)
        self._boxes, self._count, self.capacity = boxes, count, capacity

    def check(self) -> None:
        """Raises when a kernel (or the host statement) met a row it could not serve.  Reads the status word: one
        synchronisation; for the end of a sequence and for tests, not for the frame loop."""
        bits = int(self.status[0])
        if bits:
            from .. import _track_motion_lib as L
            what = [text for bit, text in ((L.STATUS_NEGATIVE_ID, "a negative track id"),
                                           (L.STATUS_ID_PAST_CAPACITY, f"a track id past the table ({self.capacity})"),
                                           (L.STATUS_BAD_LABEL, "a label outside the scores")) if bits & bit]
            raise RuntimeError("MotionState: " + ", ".join(what) + f" (status {bits})")

    def _on_device(self, *tensors) -> bool:
        cuda = [t.is_cuda for t in tensors]
        if any(cuda) != all(cuda) or any(t.device != self.device for t in tensors):
            raise ValueError(f"MotionState on {self.device}: every tensor of a call must live there")
        return all(cuda)

    @staticmethod
    def _stream(t: torch.Tensor):
        return torch.cuda.current_stream(t.device).cuda_stream

    # ------------------------------------------------------------------ observe
    def observe(self, scores, labels, boxes, ids, disappear_time, last_appear_boxes, track_score_thresh: float,
                miss_tolerance: int):
        """The existing-track loop of runtime_tracker.py:43-54; returns new ``(ids, disappear_time,
        last_appear_boxes)``.  ``scores`` (n, K) are the sigmoids torch computed (``logits_to_scores``): the decisions
        are the same bits as without motion."""
        n = ids.shape[0]
        if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[0] != n:
            raise TypeError(f"scores: expected a float32 ({n}, K) tensor, got {scores.dtype} {tuple(scores.shape)}")
        scores = scores.contiguous()
        boxes, last_appear_boxes = _f32(boxes, "boxes", 4), _f32(last_appear_boxes, "last_appear_boxes", 4)
        ids, labels = _i64(ids, "ids", n), _i64(labels, "labels", n)
        disappear_time = _i64(disappear_time, "disappear_time", n)
        if boxes.shape[0] != n or last_appear_boxes.shape[0] != n:
            raise TypeError(f"boxes / last_appear_boxes: expected {n} rows")
        if not self._on_device(scores, labels, boxes, ids, disappear_time, last_appear_boxes):
            return self._observe_host(scores, labels, boxes, ids, disappear_time, last_appear_boxes,
                                      track_score_thresh, miss_tolerance)
        from .. import _track_motion_lib as L
        ids_out, dt_out, lab_out = torch.empty_like(ids), torch.empty_like(disappear_time), torch.empty_like(boxes)
        L.check(L.lib.trackmotion_observe(
            scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), ids.data_ptr(), disappear_time.data_ptr(),
            last_appear_boxes.data_ptr(), n, scores.shape[1], float(track_score_thresh), int(miss_tolerance),
            self._boxes.data_ptr(), self._count.data_ptr(), self.capacity, self.max_length, ids_out.data_ptr(),
            dt_out.data_ptr(), lab_out.data_ptr(), self.status.data_ptr(), self._stream(ids)), "trackmotion_observe")
        return ids_out, dt_out, lab_out

    def _observe_host(self, scores, labels, boxes, ids, disappear_time, last_appear_boxes, track_score_thresh,
                      miss_tolerance):
        n, Lm, cap = ids.shape[0], self.max_length, self.capacity
        if n == 0:
            return ids.clone(), disappear_time.clone(), last_appear_boxes.clone()
        own = scores.gather(1, labels[:, None]).squeeze(1)
        missed = own < track_score_thresh                   # (float32 against the threshold as float32, as today)
        dt_new = torch.where(missed, disappear_time + 1, torch.zeros_like(disappear_time))
        in_table = (ids >= 0) & (ids < cap)
        self.status |= torch.where((ids < 0).any(), 1, 0).to(torch.int32)
        self.status |= torch.where((ids >= cap).any(), 2, 0).to(torch.int32)
        push = in_table & ~missed
        row = torch.where(push, ids, torch.full_like(ids, cap))         # skipped rows write the spare row
        hist = self._boxes.index_select(0, row)                         # (n, L, 4)
        count = self._count.index_select(0, row).long()
        count = torch.where(disappear_time > 0, torch.zeros_like(count), count)      # seen again after a miss
        full = count >= Lm
        hist = torch.where(full[:, None, None], torch.cat((hist[:, 1:], hist[:, -1:]), dim=1), hist)
        at = torch.where(full, torch.full_like(count, Lm - 1), count)
        hist = hist.scatter(1, at[:, None, None].expand(n, 1, 4), boxes[:, None, :])
        self._boxes.index_copy_(0, row, hist)
        self._count.index_copy_(0, row, (at + 1).to(torch.int32))
        lab_out = torch.where(push[:, None], boxes, last_appear_boxes)
        ids_out = torch.where(in_table & (dt_new >= miss_tolerance), torch.full_like(ids, -1), ids)
        return ids_out, dt_new, lab_out

    # ------------------------------------------------------------------ register
    def register(self, first_id: int, new_boxes: torch.Tensor) -> None:
        """Newborn ids ``first_id .. first_id + n_new - 1``: ``count = 1``, ``boxes[:, 0] = new_boxes`` (the caller
        sets ``new.last_appear_boxes = new.boxes``).  Grows the table first when the ids do not fit."""
        new_boxes = _f32(new_boxes, "new_boxes", 4)
        n = new_boxes.shape[0]
        if first_id < 0:
            raise ValueError(f"first_id = {first_id}")
        self.reserve(first_id + n)
        if not self._on_device(new_boxes):
            self._boxes[first_id:first_id + n, 0] = new_boxes
            self._count[first_id:first_id + n] = 1
            return
        from .. import _track_motion_lib as L
        L.check(L.lib.trackmotion_register(new_boxes.data_ptr(), n, int(first_id), self._boxes.data_ptr(),
                                           self._count.data_ptr(), self.capacity, self.max_length,
                                           self._stream(new_boxes)), "trackmotion_register")

    # ------------------------------------------------------------------ extrapolate
    def extrapolate(self, ids, disappear_time, last_appear_boxes, ref_pts, motion_lambda: float,
                    return_delta: bool = False):
        """submit_engine.py:78-87: a NEW ``ref_pts`` (the input may be storage a captured graph owns).  A row with
        ``disappear_time > 0`` and ``count[id] >= min_length`` becomes ``inverse_sigmoid(last_appear_boxes) +
        lambda * (float(disappear_time / (count - 1)) * sum of the box steps)``; the sum runs in float32 from zero,
        oldest step first, as ``Motion.get_box_delta`` does (not the telescoped ``b[last] - b[0]``).  Other rows are
        copied.  ``return_delta``: also the ``lambda * ...`` term, (n, 4), zero for unchanged rows."""
        n = ids.shape[0]
        ids, disappear_time = _i64(ids, "ids", n), _i64(disappear_time, "disappear_time", n)
        last_appear_boxes, ref_pts = _f32(last_appear_boxes, "last_appear_boxes", 4), _f32(ref_pts, "ref_pts", 4)
        if last_appear_boxes.shape[0] != n or ref_pts.shape[0] != n:
            raise TypeError(f"last_appear_boxes / ref_pts: expected {n} rows")
        if not self._on_device(ids, disappear_time, last_appear_boxes, ref_pts):
            out, delta = self._extrapolate_host(ids, disappear_time, last_appear_boxes, ref_pts, motion_lambda)
            return (out, delta) if return_delta else out
        from .. import _track_motion_lib as L
        out = torch.empty_like(ref_pts)
        delta = torch.empty_like(ref_pts) if return_delta else None
        L.check(L.lib.trackmotion_extrapolate(
            ids.data_ptr(), disappear_time.data_ptr(), last_appear_boxes.data_ptr(), ref_pts.data_ptr(), n,
            float(motion_lambda), self.min_length, self._boxes.data_ptr(), self._count.data_ptr(), self.capacity,
            self.max_length, out.data_ptr(), None if delta is None else delta.data_ptr(), self._stream(ids)),
            "trackmotion_extrapolate")
        return (out, delta) if return_delta else out

    def _extrapolate_host(self, ids, disappear_time, last_appear_boxes, ref_pts, motion_lambda):
        n, Lm, cap = ids.shape[0], self.max_length, self.capacity
        if n == 0:
            return ref_pts.clone(), torch.zeros_like(ref_pts)
        in_table = (ids >= 0) & (ids < cap)
        row = torch.where(in_table, ids, torch.full_like(ids, cap))
        hist = self._boxes.index_select(0, row)
        count = self._count.index_select(0, row).long()
        changed = in_table & (disappear_time > 0) & (count >= self.min_length)
        total = torch.zeros_like(ref_pts)
        for k in range(Lm - 1):                             # sequential, from zero, oldest step first
            total = torch.where((count > k + 1)[:, None], total + (hist[:, k + 1] - hist[:, k]), total)
        factor = (disappear_time.double() / (count - 1).clamp(min=1).double()).float()
        lam = torch.tensor(motion_lambda, dtype=torch.float32, device=ref_pts.device)
        delta = torch.where(changed[:, None], lam * (factor[:, None] * total), torch.zeros_like(ref_pts))
        out = torch.where(changed[:, None], inverse_sigmoid_reference(last_appear_boxes) + delta, ref_pts)
        return out, delta
