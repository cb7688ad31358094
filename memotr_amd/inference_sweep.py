"""One sequence tracked under S threshold settings at once, with one encode per frame.

Backbone and encoder do not depend on ``DET_SCORE_THRESH`` / ``TRACK_SCORE_THRESH`` / ``RESULT_SCORE_THRESH`` /
``MISS_TOLERANCE``; only the track queries of the decoder and the bookkeeping behind it do.  A ``SweepTracker`` is a
``MultiSequenceTracker`` whose S bank streams all follow the SAME sequence, stream k under setting k:

    1. one frame is uploaded, preprocessed and encoded (B = 1), a frame ahead on the side stream, as a one-stream bank does
    2. the encode result is broadcast to S: ``memory``, ``valid_ratios`` and ``mask_flatten`` expanded along the batch
       axis and made contiguous (the mask once per geometry, with its masked-rows tag restated for S images)
    3. ``decode_queries`` on cat(detect queries, bank slots) with B = S
    4. ``clip_ops.bank_update_streams``: stream k's births, misses and retirements by setting k -- one launch
    5. ``QueryUpdater.update_bank`` and the live-count watch
    6. the report: one packed copy (``track``) or one launch into a ``BankResultLog`` (``track_logged``), whose
       "sequence" column is the setting's index

and nothing in 3-6 reads from the device.

    settings = [dict(det_score_thresh=0.5, track_score_thresh=0.5, result_score_thresh=0.5, miss_tolerance=30), ...]
    tracker = SweepTracker(model, settings, cap=128, dataset_name="DanceTrack", use_dab=True, area_thresh=100)
    for frame_idx, results in tracker.track(frames_or_jpeg_paths, bgr=False):
        for k, result in enumerate(results):                    # results[k]: what SequenceTracker under setting k reports
            lines[k] += tracker.mot_lines(frame_idx, result)

    log = BankResultLog(device)
    n_frames = tracker.track_logged(source, log)                # no host result per frame
    lines_k = log.mot_lines(k)
"""
from __future__ import annotations

from typing import List

import torch

from .functions import clip_ops
from .inference_multi import _DONE, MultiSequenceTracker, _Sequence, _Step
from .lookahead import is_stream_like
from .modules.ms_deform_attn import MASKED_ROWS_ATTR
from .structures.track_instances import TrackInstances

CONFIG_KEYS = dict(det_score_thresh="DET_SCORE_THRESH", track_score_thresh="TRACK_SCORE_THRESH",
                   result_score_thresh="RESULT_SCORE_THRESH", miss_tolerance="MISS_TOLERANCE")


class SweepTracker(MultiSequenceTracker):
    def __init__(self, model, settings, cap: int = 128, dataset_name: str = "DanceTrack", use_dab: bool = True,
                 area_thresh: int = 100, raw_size=(800, 1536), use_motion: bool = False, side_stream=None):
        settings = [dict(s) for s in settings]
        if not settings:
            raise ValueError("a sweep needs at least one setting")
        super().__init__(model, n_streams=len(settings), cap=cap, dataset_name=dataset_name, use_dab=use_dab,
                         area_thresh=area_thresh, raw_size=raw_size, use_motion=use_motion, side_stream=side_stream)
        self.thresholds = clip_ops.StreamThresholds(settings, self.device, area_thresh=area_thresh)
        self.settings = self.thresholds.settings
        # (the scalar thresholds of the base class decide nothing here)
        self.det_score_thresh = self.track_score_thresh = self.result_score_thresh = self.miss_tolerance = None
        self._wide = None             # the mask-derived tensors of the last geometry, broadcast to S

    @classmethod
    def from_config(cls, model, config: dict, settings, cap: int = 128, **options):
        """``settings``: dicts with any of det_score_thresh, track_score_thresh, result_score_thresh, miss_tolerance;
        what a setting omits comes from ``config``."""
        full = [dict({key: config[name] for key, name in CONFIG_KEYS.items()}, **s) for s in settings]
        return cls(model, full, cap=cap, dataset_name=config["DATASET"], use_dab=config["USE_DAB"],
                   use_motion=config.get("USE_MOTION", False), **options)

    # ------------------------------------------------------------------ what differs from B sequences side by side
    def _frames_per_step(self) -> int:
        return 1

    def _bank_update(self, res: dict) -> None:
        clip_ops.bank_update_streams(res, self.bank, self.thresholds)

    def _report_thresholds(self, b: int):
        s = self.settings[b]
        return s["result_score_thresh"], s["area_thresh"]

    def _decode(self, enc: dict) -> dict:
        return super()._decode(self._broadcast(enc))

    def _broadcast(self, enc: dict) -> dict:
        """Step 2: the one-image encode result as S equal images.  Shapes and level starts are shared; ``memory`` is
        copied every frame; the mask and the valid ratios depend on the geometry alone (``DeformableTransformer.encode``
        hands out the same tensors for the same geometry) and are copied when the mask is another object.  The padded
        rows of image s are those of image 0 shifted by s images: the tag is restated without a read-back."""
        S = self.bank.n_streams
        if S == 1:
            return enc
        mask, ratios = enc["mask_flatten"], enc["valid_ratios"]
        wide = self._wide
        if wide is None or wide[0] is not mask or wide[1] is not ratios or wide[2].shape[0] != S:
            mask_s = mask.expand(S, -1).contiguous()
            rows = getattr(mask, MASKED_ROWS_ATTR, None)
            if rows is not None:
                shift = torch.arange(S, dtype=rows.dtype, device=rows.device)[:, None] * mask.shape[1]
                setattr(mask_s, MASKED_ROWS_ATTR, (rows[None, :] + shift).reshape(-1))
            wide = self._wide = (mask, ratios, mask_s, ratios.expand(S, -1, -1).contiguous())
        return dict(enc, memory=enc["memory"].expand(S, -1, -1).contiguous(), mask_flatten=wide[2], valid_ratios=wide[3])

    def _check(self) -> None:
        """The one read of a sequence's end: did every birth of every setting find a slot?"""
        bad = [(k, n) for k, n in enumerate(self.bank.counters[:, 1].tolist()) if n != 0]
        if bad:
            raise RuntimeError("threshold sweep: " + ", ".join(f"setting {k} {self.settings[k]} dropped {n} births"
                                                                for k, n in bad)
                               + f" for lack of a free slot among {self.bank.cap}")

    # ------------------------------------------------------------------ one sequence
    def _run_one(self, source, bgr: bool, on_step):
        """``on_step(frame_idx, size)`` once per frame, after steps 1-5; yields what it returns.  A new sequence starts
        every stream afresh.  ``self.n_frames`` holds the frames read."""
        seq = _Sequence(0, source)
        self.n_frames = 0
        if seq.item is _DONE:
            return
        self.begin(self.n_streams)
        main = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        side = self._lookahead.side_stream() if main is not None else None
        step = self._materialise([seq.item], bgr, main)
        more = True
        while more:
            frame_idx = seq.frame_idx
            seq.item = next(seq.it, _DONE)
            more = seq.item is not _DONE
            if more:
                seq.frame_idx += 1
                if not is_stream_like(seq.item) and seq.size != (int(seq.item.shape[0]), int(seq.item.shape[1])):
                    raise ValueError(f"frame {seq.frame_idx} has another size than the first frame")
            ahead = (lambda: self._materialise([seq.item], bgr, side)) if more else None
            self._done_step = step
            step = self._advance(step, ahead, bgr)
            self.n_frames = frame_idx + 1
            yield on_step(frame_idx, seq.size)
        self._check()

    def track(self, source, *, bgr: bool = False):
        """``source``: an iterable of uint8 frames or of JPEG paths / byte streams.  Yields ``(frame index, results)``
        with ``results[k]`` what ``SequenceTracker.track`` under setting k reports for the frame."""
        S = self.n_streams
        yield from self._run_one(source, bgr, lambda idx, size: (idx, self._report_all([size] * S)))

    def track_logged(self, source, log, *, bgr: bool = False, first_setting: int = 0) -> int:
        """``track`` with the reportable rows of every frame appended to ``log`` (results.BankResultLog) on the device:
        one launch per frame, nothing per frame on the host.  The log's "sequence" column is ``first_setting + k`` for
        setting k, so ``log.mot_lines(first_setting + k)`` are setting k's lines.  Returns the number of frames."""
        S = self.n_streams

        def append(idx, size):
            seq_frame, ori_wh = self._step_arrays([(first_setting + k, idx) for k in range(S)], [size] * S)
            log.append_streams(self.bank, seq_frame, ori_wh, self.thresholds)

        for _ in self._run_one(source, bgr, append):
            pass
        return self.n_frames

    def step_raw(self, frames, next_frames=None, *, bgr: bool = False) -> List[TrackInstances]:
        """One step on one frame: ``frames`` is a list of ONE (H, W, 3) uint8 frame (``next_frames``: the list the next
        call will pass); returns the S reports."""
        if len(frames) != 1:
            raise ValueError(f"a sweep tracks one sequence: {len(frames)} frames in one step")
        if self.bank is None:
            self.begin(self.n_streams)
        step = self._lookahead.pending_key
        if step is None or step.source is not frames:
            step = _Step(frames, source=frames)
        size = (int(frames[0].shape[0]), int(frames[0].shape[1]))
        ahead = None if next_frames is None else (lambda: _Step(next_frames, source=next_frames))
        self._advance(step, ahead, bgr)
        return self._report_all([size] * self.n_streams)

    def _refuse(self, *args, **kwargs):
        raise NotImplementedError("a SweepTracker tracks one sequence under several settings: use track / track_logged")

    track_many = track_many_logged = track_many_annotated = track_many_annotated_logged = _refuse
