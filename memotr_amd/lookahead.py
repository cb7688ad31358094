"""The stream ordering of the online trackers, stated once: the encode half of the next frame queued a step ahead on a
side stream (``Lookahead``), and the "current / next" loop over a source that feeds it (``frame_pairs``,
``is_stream_like``).  ``SequenceTracker`` (inference.py) and ``MultiSequenceTracker`` (inference_multi.py) each own one
``Lookahead``; the pinned upload and the packed read they pair it with are in utils/host.py.
"""
from __future__ import annotations

import os

import torch


def is_stream_like(item) -> bool:
    """A JPEG path or byte stream, as opposed to a decoded (H, W, 3) frame."""
    return isinstance(item, (str, bytes, bytearray, memoryview, os.PathLike)) or \
        (hasattr(item, "ndim") and item.ndim == 1)


def frame_pairs(source, prepare=None):
    """Yields ``(idx, current, next or None)`` over ``source``.  ``prepare(item, ahead)`` is applied to every item once,
    when it is first read: the first item with ``ahead=False``, every later one -- while the item before it is still
    current -- with ``ahead=True`` (the callers upload or decode it on the main or on the side stream accordingly)."""
    it = iter(source)
    done = object()
    cur, idx = next(it, done), 0
    if cur is not done and prepare is not None:
        cur = prepare(cur, False)
    while cur is not done:
        nxt = next(it, done)
        if nxt is not done and prepare is not None:
            nxt = prepare(nxt, True)
        yield idx, cur, None if nxt is done else nxt
        cur, idx = nxt, idx + 1


class Lookahead:
    """The encode half (backbone + encoder) of a frame, computed now or queued one step ahead on a side stream.

    ``frame_of(key, after)`` turns the caller's key -- an image tensor, a raw frame, a lockstep ``_Step`` -- into the
    padded batch the model encodes.  The rules both trackers rely on:

    * Every encode call goes through ``encode``: it stamps ``encode_slot`` and ``encode_static_ok = True`` on the
      frame and flips the slot (models/infer_graphs.py keeps one static ``memory`` per slot, read in place by the
      decoder: the two alternate so that a queued encode never writes what this frame's decoder still reads).
    * ``take`` waits first: if anything is pending, the current stream waits on its event before anything else is
      encoded or decoded -- also when the key does not match, because the slot buffers may still be written.
    * The key matches by identity (``is``), never by value.
    * ``queue`` is called after this frame's decoder call has been issued on the main stream and before the track
      update (the host blocks there; the device works through the queued half meanwhile).
    * The side stream is the one given as ``side_stream``, else one made when first needed (``side_stream()``).
    * Two orders of waiting: ``wait_first=True`` (inputs already on the device, made on the main stream) is
      ``side.wait_stream(main)`` and then ``frame_of(key, None)``; ``wait_first=False`` is ``frame_of(key, main)``
      on the side stream, which uploads first -- the copies depend on nothing main has queued -- then waits for
      ``main``, then preprocesses.
    * After queueing, device-resident ``inputs`` get ``record_stream(side)``, every tensor of the encode result gets
      ``record_stream(main)``, and the event is recorded on the side stream.
    * On a CPU device nothing is queued.
    * ``forget`` waits on the pending event and drops what was pending.
    """

    def __init__(self, model, device, side_stream=None):
        self.model, self.device = model, device
        self._side = side_stream      # (trackers made one after another can share one: which hardware queue a new stream
        #                               lands on decides whether the lookahead overlaps at all -- profiles/submit_log.md)
        self._pending = None          # (key, encode result, event)
        self._slot = 0

    @property
    def pending_key(self):
        return None if self._pending is None else self._pending[0]

    def side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def encode(self, frame) -> dict:
        frame.encode_slot = self._slot
        frame.encode_static_ok = True
        self._slot ^= 1
        return self.model(frame=frame, stage="encode")

    def forget(self):
        """Wait for what is pending and drop it; returns it (or None)."""
        pending, self._pending = self._pending, None
        if pending is not None:
            torch.cuda.current_stream(self.device).wait_event(pending[2])
        return pending

    def take(self, key, frame_of) -> dict:
        """The encode result of ``key``: the one queued ahead, or computed now."""
        pending = self.forget()
        if pending is not None and pending[0] is key:
            return pending[1]
        return self.encode(frame_of(key, None))

    def queue(self, key, frame_of, wait_first: bool, inputs=None) -> None:
        if self.device.type != "cuda":
            return
        main, side = torch.cuda.current_stream(self.device), self.side_stream()
        if wait_first:
            side.wait_stream(main)
        with torch.cuda.stream(side):
            enc = self.encode(frame_of(key, None if wait_first else main))
            event = side.record_event()
        for t in (key,) if inputs is None else inputs:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(side)
        for v in enc.values():                  # produced on the side stream, consumed on main
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(main)
        self._pending = (key, enc, event)
