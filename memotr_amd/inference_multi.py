"""Online tracking of several video sequences in lockstep: one encode and one decoder call per step for B sequences, and
track bookkeeping that never leaves the device.

One sequence is bound by a dependency chain -- the next frame's decoder waits for this frame's tracks -- whose kernels
are too small to fill the device.  Independent sequences have no such dependency, so their chains are run side by side
as one batch: the tracks of every sequence live in the fixed slots of a ``TrackBank`` (models/track_bank.py), and a step
is

    1. one batched upload + resize/normalise            (data/frames.py; utils.host.PinnedUploader)
    2. one batched encode, queued a step ahead on a side stream, two alternating graph slots (lookahead.Lookahead:
       the rules are the one-sequence tracker's, the key is the ``_Step``)
    3. ``MeMOTR.decode_queries`` on cat(detect queries, bank slots), free slots masked as keys
    4. ``clip_ops.bank_update``: refresh, age, retire, births -- one launch for all sequences
    5. ``QueryUpdater.update_bank``
    6. the result: one packed copy for all sequences (``step_raw`` / ``track_many``) or one launch into a
       ``results.BankResultLog`` (``track_many_logged``)

and nothing in 3-6 reads from the device.  The live counts travel to pinned memory with a non-blocking copy and are looked
at one step late; when one passes half the capacity, the bank grows.

    tracker = MultiSequenceTracker.from_config(model, config, n_streams=4)
    for seq, frame_idx, result in tracker.track_many([frames_a, paths_b, frames_c], bgr=False):
        lines[seq] += tracker.mot_lines(frame_idx, result)

    log = BankResultLog(device)
    n_frames = tracker.track_many_logged(sources, log)            # no host result per frame
    lines_b = log.mot_lines(1)

    with MultiAnnotatedWriter("annotated/") as writer:            # render.py: an annotated JPEG per frame and sequence,
        tracker.track_many_annotated_logged(sources, writer, log)  # drawn from a table made on the device

Sequences that share a step share the resized geometry, so they are grouped by ``target_size``; when a sequence ends its
stream takes the next one of that geometry, and when none is left the last stream's tracks move into the hole and the
batch shrinks.  A sequence's results do not depend on which sequences it shared steps with, beyond float rounding.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .data.frames import padded_size, padding_mask, preprocess_frames, target_size
from .functions import clip_ops
from .inference import bdd_frame_result, mot_lines, pack_tracks, reportable
from .lookahead import Lookahead, is_stream_like
from .models.track_bank import TrackBank
from .models.utils import get_model
from .structures.track_instances import TrackInstances
from .utils.host import PinnedUploader, to_host
from .utils.nested_tensor import NestedTensor

_DONE = object()


class _Step:
    """The frames of one lockstep step: ``frames[b]`` for stream b ((H, W, 3) uint8, host or device), ``batch`` the
    same frames as one (B, H, W, 3) device tensor where there is one, ``source`` the caller's own list."""

    def __init__(self, frames, batch=None, source=None):
        self.frames, self.batch, self.source = list(frames), batch, source


class _Sequence:
    """One source being read: ``item`` is the frame of the coming step, ``frame_idx`` its index."""

    def __init__(self, index: int, source):
        self.index, self.it, self.frame_idx = index, iter(source), 0
        self.item = next(self.it, _DONE)
        self.size = None if self.item is _DONE else self._size(self.item)

    @staticmethod
    def _size(item):
        if not is_stream_like(item):
            return int(item.shape[0]), int(item.shape[1])
        from .data import jpeg as J
        try:
            info = J.parse_jpeg(J._as_bytes(item))
            return info.height, info.width
        except J.UnsupportedJpeg:
            px = J.decode_jpeg(item, "cpu")
            return int(px.shape[0]), int(px.shape[1])


class MultiSequenceTracker:
    def __init__(self, model, n_streams: int = 4, cap: int = 128, dataset_name: str = "DanceTrack",
                 det_score_thresh: float = 0.7, track_score_thresh: float = 0.6, result_score_thresh: float = 0.7,
                 miss_tolerance: int = 5, use_dab: bool = True, area_thresh: int = 100, raw_size=(800, 1536),
                 use_motion: bool = False, side_stream=None):
        from .utils.host import respect_cpu_quota
        respect_cpu_quota()
        if n_streams < 1:
            raise ValueError(f"n_streams must be at least 1, not {n_streams}")
        if use_motion:
            raise ValueError("USE_MOTION keeps a box history per track of ONE sequence (models/motion.py): it cannot be "
                             "combined with more than one stream; track with SequenceTracker (streams = 1) instead")
        TrackBank._check_cap(cap)
        self.model = model.eval()
        self.core = get_model(model)
        self.n_streams, self.cap = int(n_streams), int(cap)
        self.dataset_name = dataset_name
        self.det_score_thresh, self.track_score_thresh = det_score_thresh, track_score_thresh
        self.result_score_thresh, self.miss_tolerance = result_score_thresh, miss_tolerance
        self.area_thresh, self.use_dab, self.raw_size = area_thresh, use_dab, raw_size
        self.device = next(self.core.parameters()).device
        self.bank: Optional[TrackBank] = None
        self._lookahead = Lookahead(self.model, self.device, side_stream)     # keyed by the _Step
        self._uploader = PinnedUploader(self.device)      # one pinned buffer per (parity, stream)
        self._parity = 0              # flipped once per batch upload: a buffer comes round every second step
        self._jpeg_staging = None
        self._counts = [None, None]   # two pinned copies of the bank's counters, each with the event of its copy
        self._counts_i = 0
        self._det_parts = {}          # B -> (reference points, query embeddings, mask) of the detect queries
        self._done_step = None        # the _Step whose tracks the bank holds
        self._table = None            # the draw table of the annotated forms, (B, cap, 16) int32: made anew when (B, cap)
        self._table_read = None       # changes; the event behind the writer's draw launches that read it

    @classmethod
    def from_config(cls, model, config: dict, n_streams: int = 4, cap: int = 128, **options):
        return cls(model, n_streams=n_streams, cap=cap, dataset_name=config["DATASET"],
                   det_score_thresh=config["DET_SCORE_THRESH"], track_score_thresh=config["TRACK_SCORE_THRESH"],
                   result_score_thresh=config["RESULT_SCORE_THRESH"], miss_tolerance=config["MISS_TOLERANCE"],
                   use_dab=config["USE_DAB"], use_motion=config.get("USE_MOTION", False), **options)

    def mot_lines(self, frame_idx: int, tracks: TrackInstances) -> List[str]:
        return mot_lines(self.dataset_name, frame_idx, tracks)

    bdd_frame_result = staticmethod(bdd_frame_result)

    # ------------------------------------------------------------------ the bank
    def begin(self, n_streams: int) -> TrackBank:
        """A fresh bank of ``n_streams`` empty streams (what ``track_many`` starts every geometry group with)."""
        if not 1 <= n_streams <= self.n_streams:
            raise ValueError(f"{n_streams} streams asked of a tracker made for {self.n_streams}")
        self._lookahead.forget()
        self._counts = [None, None]
        self.bank = TrackBank(n_streams, self.cap, num_classes=self.core.num_classes, hidden_dim=self.core.hidden_dim,
                              use_dab=self.use_dab, device=self.device)
        return self.bank

    def _watch_counts(self) -> None:
        """Grow the bank when a stream's live count passed half the capacity -- judged from the copy the PREVIOUS step
        queued (long complete), so that this step waits for nothing."""
        bank = self.bank
        if self.device.type != "cuda":
            if int(bank.counters[:, 0].max()) > bank.cap // 2:
                bank.grow(2 * bank.cap)
            return
        i, self._counts_i = self._counts_i, self._counts_i ^ 1
        prev = self._counts[i ^ 1]
        entry = self._counts[i]
        if entry is None:
            entry = self._counts[i] = [torch.zeros((self.n_streams, 2), dtype=torch.int32, pin_memory=True), None, 0]
        elif entry[1] is not None and not entry[1].query():
            entry[1].synchronize()                  # (two steps old)
        entry[0][:bank.n_streams].copy_(bank.counters, non_blocking=True)
        entry[1] = torch.cuda.current_stream(self.device).record_event()
        entry[2] = bank.n_streams
        if prev is not None and prev[1] is not None:
            if not prev[1].query():
                prev[1].synchronize()
            if int(prev[0][:prev[2], 0].max()) > bank.cap // 2:
                bank.grow(2 * bank.cap)

    # ------------------------------------------------------------------ one step
    @torch.no_grad()
    def step_raw(self, frames, next_frames=None, *, bgr: bool = False) -> List[TrackInstances]:
        """One lockstep step: ``frames[b]`` is the (H, W, 3) uint8 frame of stream b (torch or numpy, RGB; ``bgr=True``:
        cv2's order), one per stream of the bank (the first call makes a bank of ``len(frames)`` streams).  Returns the
        reportable tracks of every stream as ``SequenceTracker.step_raw`` reports one stream's.  ``next_frames``: the
        list the next call will pass (the same object), whose upload and encode half are queued on the side stream."""
        if self.bank is None:
            self.begin(len(frames))
        step = self._lookahead.pending_key
        if step is None or step.source is not frames:
            step = _Step(frames, source=frames)
        sizes = [(int(f.shape[0]), int(f.shape[1])) for f in step.frames]
        ahead = None if next_frames is None else (lambda: _Step(next_frames, source=next_frames))
        self._advance(step, ahead, bgr)
        return self._report_all(sizes)

    @torch.no_grad()
    def _advance(self, step: _Step, ahead, bgr: bool) -> Optional[_Step]:
        """Steps 1-5 for the frames of ``step``; ``ahead() -> _Step`` makes the next step's frames once this step's
        decoder is queued (their encode half then goes to the side stream).  Returns that next step."""
        return self._track(self._encoded(step, bgr), ahead, bgr)

    @torch.no_grad()
    def _encoded(self, step: _Step, bgr: bool) -> dict:
        """Steps 1-2: this step's encode result -- the one queued ahead by the previous step, or computed now."""
        if len(step.frames) != self._frames_per_step():
            raise ValueError(f"{len(step.frames)} frames for a bank of {self.bank.n_streams} streams")
        return self._lookahead.take(step, lambda s, after: self._batch_frame(s, bgr, after))

    @torch.no_grad()
    def _track(self, enc: dict, ahead, bgr: bool) -> Optional[_Step]:
        """Steps 3-5 (and the next step's encode half queued behind the decoder): nothing here reads the device."""
        bank = self.bank
        res = self._decode(enc)
        nxt = None
        if ahead is not None:
            nxt = ahead()
            if nxt is not None:             # (uploads on the side stream first, then the wait for main)
                self._lookahead.queue(nxt, lambda s, after: self._batch_frame(s, bgr, after), False,
                                      inputs=[nxt.batch] + nxt.frames)
        self._bank_update(res)
        self.core.query_updater.update_bank(bank)
        self._watch_counts()
        return nxt

    # what a tracker of one sequence under several settings (inference_sweep.SweepTracker) states differently
    def _frames_per_step(self) -> int:
        return self.bank.n_streams

    def _bank_update(self, res: dict) -> None:
        """Step 4."""
        clip_ops.bank_update(res, self.bank, self.det_score_thresh, self.track_score_thresh, self.miss_tolerance)

    def _report_thresholds(self, b: int):
        """``(result_score_thresh, area_thresh)`` of stream ``b``'s report."""
        return self.result_score_thresh, self.area_thresh

    def _decode(self, enc: dict) -> dict:
        core, bank = self.core, self.bank
        B = bank.n_streams
        parts = self._det_parts.get(B)
        if parts is None:
            det_ref = core.get_det_reference_points()
            det_ref = det_ref[None] if det_ref.dim() == 2 else det_ref
            if det_ref.shape[-1] == 2:
                det_ref = torch.cat((det_ref, torch.zeros_like(det_ref)), dim=-1)
            n_det = core.n_det_queries
            parts = self._det_parts[B] = (det_ref.detach().expand(B, -1, -1),
                                          core.det_query_embed.detach()[None].expand(B, -1, -1),
                                          torch.zeros((B, n_det), dtype=torch.bool, device=self.device))
        det_ref, det_embed, det_mask = parts
        return core.decode_queries(enc, torch.cat((det_ref, bank.ref_pts), dim=1),
                                   torch.cat((det_embed, bank.query_embed), dim=1),
                                   torch.cat((det_mask, bank.query_mask()), dim=1))

    # ------------------------------------------------------------------ upload and encode
    def _batch_frame(self, step: _Step, bgr: bool, after=None) -> NestedTensor:
        """Step 1: the frames of ``step`` as the padded normalised batch (``after``: the stream the preprocess kernel
        waits for once the uploads are queued)."""
        frames = [torch.from_numpy(f) if not torch.is_tensor(f) else f for f in step.frames]
        B = len(frames)
        sizes = {target_size(int(f.shape[0]), int(f.shape[1]), *self.raw_size) for f in frames}
        if len(sizes) != 1:
            raise ValueError(f"the frames of one step resize to different geometries {sorted(sizes)}: only sequences of "
                             "one target size share a batch")
        th, tw = sizes.pop()
        cuda = self.device.type == "cuda"
        batch = step.batch
        if batch is None and len({tuple(f.shape) for f in frames}) == 1:
            if cuda and not any(f.is_cuda for f in frames):
                batch = torch.empty((B,) + tuple(frames[0].shape), dtype=torch.uint8, device=self.device)
                self._parity ^= 1
                for b, f in enumerate(frames):
                    self._uploader.into(f, batch[b], (self._parity, b))
            elif not cuda:
                batch = torch.stack(frames)
        if batch is None and cuda:
            self._parity ^= 1
            frames = [self._uploader.upload(f, (self._parity, b)) for b, f in enumerate(frames)]
        if after is not None:                   # (the uploads depend on nothing that stream has queued)
            torch.cuda.current_stream(self.device).wait_stream(after)
        if batch is not None:
            frame = preprocess_frames(batch, bgr=bgr, size=(th, tw))
        else:
            Hp, Wp = padded_size(th, tw)
            out = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=self.device)
            for b, f in enumerate(frames):
                preprocess_frames(f, bgr=bgr, out=out[b:b + 1], size=(th, tw))
            frame = NestedTensor(out, padding_mask(B, th, tw, Hp, Wp, self.device), sizes=((Hp, Wp),) + ((th, tw),) * B)
        step.kept = (batch, frames)             # (device frames stay referenced until the step is done)
        return frame

    def _materialise(self, items, bgr: bool, stream=None) -> _Step:
        """The frames of a step from the sources' items: decoded frames as they are; JPEG paths / byte streams through
        ``decode_jpegs`` (host entropy stage now, upload and pixel kernels on ``stream``)."""
        jpeg = [b for b, x in enumerate(items) if is_stream_like(x)]
        if not jpeg:
            return _Step(items)
        from .data import jpeg as J
        if self.device.type != "cuda":
            decoded = [J.decode_jpeg(items[b], "cpu", bgr=bgr) for b in jpeg]
        else:
            if self._jpeg_staging is None:
                self._jpeg_staging = J._Staging(3)
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                decoded = J.decode_jpegs([items[b] for b in jpeg], self.device, bgr=bgr, staging=self._jpeg_staging)
        whole = torch.is_tensor(decoded) and len(jpeg) == len(items)
        frames = list(items)
        for b, f in zip(jpeg, decoded):
            frames[b] = f
        return _Step(frames, batch=decoded if whole else None)

    # ------------------------------------------------------------------ results
    @torch.no_grad()
    def _report_all(self, sizes) -> List[TrackInstances]:
        """``inference.reportable`` for every stream from ONE packed copy: the live slots of a stream in id order --
        the one-sequence tracker's tracks are in birth order."""
        bank, K = self.bank, self.bank.num_classes
        host = to_host(pack_tracks(bank.boxes, bank.scores, bank.ids, bank.labels, K))
        out = []
        for b, (ori_h, ori_w) in enumerate(sizes):
            rows = host[b]
            ids = rows[:, 4 + K].long()
            slots = (ids >= 0).nonzero().squeeze(1)
            out.append(reportable(rows[slots[torch.argsort(ids[slots])]], K, ori_h, ori_w, *self._report_thresholds(b),
                                  hidden_dim=bank.hidden_dim, num_classes=K, use_dab=self.use_dab))
        return out

    # ------------------------------------------------------------------ many sequences
    def _run(self, sources, bgr: bool, on_step):
        """The lockstep schedule.  ``on_step(meta, sizes)`` is called once per step, after steps 1-5, with
        ``meta[b] = (sequence index, frame index)`` and ``sizes[b] = (ori_h, ori_w)`` of stream b; yields what it returns.
        Returns (through StopIteration) nothing; ``self.frame_counts`` holds the frames read of every source."""
        seqs = [_Sequence(i, src) for i, src in enumerate(sources)]
        self.frame_counts = [0] * len(seqs)
        groups = {}
        for s in seqs:
            if s.item is not _DONE:
                groups.setdefault(target_size(*s.size, *self.raw_size), []).append(s)
        for queue in groups.values():
            yield from self._run_group(queue, bgr, on_step)

    def _run_group(self, queue, bgr: bool, on_step):
        live = [queue.pop(0) for _ in range(min(self.n_streams, len(queue)))]
        bank = self.begin(len(live))
        main = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        side = self._lookahead.side_stream() if main is not None else None
        step = self._materialise([s.item for s in live], bgr, main)
        while live:
            meta = [(s.index, s.frame_idx) for s in live]
            sizes = [s.size for s in live]
            # who goes on, who ends, and what the streams hold at the next step
            nxt_live, ops, ended = list(live), [], False
            for b in range(len(live) - 1, -1, -1):
                s = live[b]
                s.item = next(s.it, _DONE)
                self.frame_counts[s.index] = s.frame_idx + 1
                if s.item is not _DONE:
                    s.frame_idx += 1
                    continue
                ended = True
                if queue:
                    nxt_live[b] = queue.pop(0)
                    ops.append(("reset", b))
                else:
                    last = len(nxt_live) - 1
                    if b != last:
                        nxt_live[b] = nxt_live[last]
                        ops.append(("move", last, b))
                    nxt_live.pop()
                    if nxt_live:
                        ops.append(("shrink", len(nxt_live)))
            for s in nxt_live:               # (a JPEG stream's size shows when it is decoded: _encode_batch checks it)
                if not is_stream_like(s.item) and s.size != (int(s.item.shape[0]), int(s.item.shape[1])):
                    raise ValueError(f"sequence {s.index}: frame {s.frame_idx} has another size than its first frame")
            ahead = (lambda: self._materialise([s.item for s in nxt_live], bgr, side)) if nxt_live else None
            self._done_step = step          # (its device frames: what an annotating on_step draws into)
            step = self._advance(step, ahead, bgr)
            yield on_step(meta, sizes)
            if ended:
                bank.check()                        # the one read of a sequence's end: did every birth find a slot?
            for op in ops:
                if op[0] == "reset":
                    bank.reset_stream(op[1])
                elif op[0] == "move":
                    bank.move_stream(op[1], op[2])
                else:
                    bank.shrink(op[1])
            live = nxt_live

    def track_many(self, sources, *, bgr: bool = False):
        """``sources``: a list of sequences, each an iterable of uint8 frames or of JPEG paths / byte streams.  Yields
        ``(sequence index, frame index, result)`` -- for one sequence, what ``SequenceTracker.track`` yields."""
        for meta, results in self._run(sources, bgr, lambda meta, sizes: (meta, self._report_all(sizes))):
            for (seq, frame_idx), result in zip(meta, results):
                yield seq, frame_idx, result

    def track_many_logged(self, sources, log, *, bgr: bool = False) -> List[int]:
        """``track_many`` with the reportable rows of every step appended to ``log`` (results.BankResultLog) on the
        device instead of being brought to the host: one launch per step.  Returns the frame count of every source."""
        def append(meta, sizes):
            seq_frame, ori_wh = self._step_arrays(meta, sizes)
            log.append(self.bank, seq_frame, ori_wh, self.result_score_thresh, self.area_thresh)

        for _ in self._run(sources, bgr, append):
            pass
        return list(self.frame_counts)

    def _step_arrays(self, meta, sizes):
        """``(seq_frame int64 (B, 2), ori_wh float32 (B, 2))`` of a step on the device: one non-blocking upload."""
        host = torch.tensor([[seq, idx, w, h] for (seq, idx), (h, w) in zip(meta, sizes)], dtype=torch.int64)
        if self.device.type == "cuda":
            host = host.pin_memory()
        dev = host.to(self.device, non_blocking=True)
        return dev[:, :2].contiguous(), dev[:, 2:].float().contiguous()

    # ------------------------------------------------------------------ annotated output
    @torch.no_grad()
    def _annotate(self, writer, meta, ori_wh, bgr: bool) -> None:
        """One ``clip_ops.draw_table`` launch from the bank and the step's device frames (``_batch_frame`` kept them:
        no second upload) to ``writer.add_step``.  The table is rewritten only behind the draw launches that read the
        last one: the current stream waits for their event, the host for nothing."""
        bank = self.bank
        shape = (bank.n_streams, bank.cap, 16)
        if self._table is None or tuple(self._table.shape) != shape:
            self._table = torch.empty(shape, dtype=torch.int32, device=self.device)
        elif self._table_read is not None:
            torch.cuda.current_stream(self.device).wait_event(self._table_read)
        clip_ops.draw_table(bank.boxes, bank.scores, bank.ids, ori_wh, self.result_score_thresh, self.area_thresh,
                            bgr=bgr, font_scale=writer.font_scale, out=self._table)
        batch, frames = self._done_step.kept
        self._table_read = writer.add_step(meta, batch if batch is not None else frames, self._table, bgr=bgr)

    def track_many_annotated(self, sources, writer, *, bgr: bool = False):
        """``track_many`` with an annotated JPEG per frame and sequence on the side (render.MultiAnnotatedWriter):
        yields exactly what ``track_many`` yields.  The overlay does not come from the yielded results: per step one
        launch makes the draw table from the bank, and the writer draws into the device frames the tracker already
        holds.  ``bgr`` is the frames' channel order, for the model and the writer alike.  The caller closes the
        writer."""
        def on_step(meta, sizes):
            self._annotate(writer, meta, self._step_arrays(meta, sizes)[1], bgr)
            return meta, self._report_all(sizes)

        for meta, results in self._run(sources, bgr, on_step):
            for (seq, frame_idx), result in zip(meta, results):
                yield seq, frame_idx, result

    def track_many_annotated_logged(self, sources, writer, log, *, bgr: bool = False) -> List[int]:
        """``track_many_logged`` with the annotated files of ``track_many_annotated``: the rows go to ``log`` and the
        draw table to ``writer`` on the device, and no per-frame result reaches the host.  Returns the frame count of
        every source."""
        def on_step(meta, sizes):
            seq_frame, ori_wh = self._step_arrays(meta, sizes)
            log.append(self.bank, seq_frame, ori_wh, self.result_score_thresh, self.area_thresh)
            self._annotate(writer, meta, ori_wh, bgr)

        for _ in self._run(sources, bgr, on_step):
            pass
        return list(self.frame_counts)
