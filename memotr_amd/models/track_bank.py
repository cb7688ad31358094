"""The tracks of B sequences as fixed-size device tensors.

``RuntimeTracker`` + ``QueryUpdater.select_active_tracks`` keep one sequence's tracks as a ``TrackInstances`` whose length
changes every frame: each frame pays a ``nonzero()`` and a boolean index, a stream synchronisation apiece.  A
``TrackBank`` holds ``cap`` slots per stream instead.  A track keeps its slot for life; ``ids == -1`` marks a free slot;
holes stay where they are and are masked as attention keys (attention is permutation-equivariant, nothing needs
compacting); free slots hold zeros, so whatever is computed from them stays finite.

    bank = TrackBank(n_streams=4, cap=128, num_classes=1, hidden_dim=256, use_dab=True, device="cuda")
    clip_ops.bank_update(res, bank, det_score_thresh, track_score_thresh, miss_tolerance)    # one launch, no read-back
    updater.update_bank(bank)
    bank.check()                                   # one read: did every birth find a slot?

Fields (B = n_streams, K = num_classes, C = hidden_dim, QW = C with DAB anchors, 2C without):
    ids, labels, disappear_time  int64 (B, cap)        boxes, ref_pts  (B, cap, 4)        logits, scores  (B, cap, K)
    output_embed, long_memory, last_output  (B, cap, C)        query_embed  (B, cap, QW)
    next_id  int64 (B,)        counters  int32 (B, 2): live tracks, births dropped for lack of a free slot (sticky)
    free_list  int32 (B, cap): workspace of the update kernel
"""
from __future__ import annotations

import torch

ROW_FIELDS = ("ids", "labels", "disappear_time", "boxes", "ref_pts", "logits", "scores", "output_embed", "long_memory",
              "last_output", "query_embed")
STREAM_FIELDS = ROW_FIELDS + ("next_id", "counters", "free_list")


class TrackBank:
    def __init__(self, n_streams: int, cap: int = 128, *, num_classes: int = 1, hidden_dim: int = 256,
                 use_dab: bool = True, device="cpu"):
        if n_streams < 1:
            raise ValueError(f"a track bank needs at least one stream, not {n_streams}")
        self._check_cap(cap)
        self.n_streams, self.cap = int(n_streams), int(cap)
        self.num_classes, self.hidden_dim, self.use_dab = int(num_classes), int(hidden_dim), bool(use_dab)
        self.device = torch.device(device)
        for name, t in self._allocate(self.n_streams, self.cap).items():
            setattr(self, name, t)

    @staticmethod
    def _check_cap(cap):
        if cap < 16 or cap % 16 != 0:
            raise ValueError(f"the capacity of a track bank is a positive multiple of 16, not {cap}")

    def _allocate(self, B: int, cap: int) -> dict:
        K, C = self.num_classes, self.hidden_dim
        QW = C if self.use_dab else 2 * C
        f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)      # noqa: E731
        i = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=self.device)        # noqa: E731
        return dict(ids=torch.full((B, cap), -1, dtype=torch.int64, device=self.device), labels=i(B, cap),
                    disappear_time=i(B, cap), boxes=f(B, cap, 4), ref_pts=f(B, cap, 4), logits=f(B, cap, K),
                    scores=f(B, cap, K), output_embed=f(B, cap, C), long_memory=f(B, cap, C), last_output=f(B, cap, C),
                    query_embed=f(B, cap, QW), next_id=i(B),
                    counters=torch.zeros((B, 2), dtype=torch.int32, device=self.device),
                    free_list=torch.zeros((B, cap), dtype=torch.int32, device=self.device))

    # ------------------------------------------------------------------ streams
    def reset_stream(self, b: int) -> None:
        """Stream ``b`` starts a new sequence: no track, ids from 0 (stream-ordered, nothing is read)."""
        self._stream_index(b)
        for name in STREAM_FIELDS:
            getattr(self, name)[b].fill_(-1 if name == "ids" else 0)

    def move_stream(self, src: int, dst: int) -> None:
        """The tracks and counters of stream ``src`` into stream ``dst`` (a device copy of its rows)."""
        self._stream_index(src), self._stream_index(dst)
        if src != dst:
            for name in STREAM_FIELDS:
                getattr(self, name)[dst].copy_(getattr(self, name)[src])

    def shrink(self, n_streams: int) -> None:
        """Keep the first ``n_streams`` streams (views of the same storage)."""
        if not 1 <= n_streams <= self.n_streams:
            raise ValueError(f"cannot shrink a bank of {self.n_streams} streams to {n_streams}")
        for name in STREAM_FIELDS:
            setattr(self, name, getattr(self, name)[:n_streams])
        self.n_streams = int(n_streams)

    def _stream_index(self, b: int) -> None:
        if not 0 <= b < self.n_streams:
            raise IndexError(f"stream {b} of a bank with {self.n_streams}")

    def grow(self, cap: int) -> None:
        """Reallocate with ``cap`` slots per stream and copy: every track keeps its slot, the new slots are free."""
        self._check_cap(cap)
        if cap < self.cap:
            raise ValueError(f"a track bank does not shrink ({self.cap} -> {cap} slots)")
        if cap == self.cap:
            return
        new = self._allocate(self.n_streams, cap)
        for name in ROW_FIELDS:
            new[name][:, :self.cap].copy_(getattr(self, name))
        new["next_id"].copy_(self.next_id)
        new["counters"].copy_(self.counters)
        if self.device.type == "cuda":            # the old tensors are read by those copies on this stream
            stream = torch.cuda.current_stream(self.device)
            for name in STREAM_FIELDS:
                getattr(self, name).record_stream(stream)
        for name, t in new.items():
            setattr(self, name, t)
        self.cap = int(cap)

    # ------------------------------------------------------------------ reads
    def query_mask(self) -> torch.Tensor:
        """(B, cap) bool, True on free slots: the key-padding mask of the track queries."""
        return self.ids < 0

    def check(self) -> None:
        """One read of the counters: raises when a birth found no free slot in some stream (the tracks of that stream
        are then not what the unbounded tracker would hold)."""
        dropped = self.counters[:, 1].tolist()
        bad = [(b, n) for b, n in enumerate(dropped) if n != 0]
        if bad:
            raise RuntimeError("track bank: " + ", ".join(f"stream {b} dropped {n} births" for b, n in bad)
                               + f" for lack of a free slot among {self.cap}")

    def stream_tracks(self, b: int) -> dict:
        """The live tracks of stream ``b`` in id (= birth) order, field by field: what the one-sequence tracker holds as
        a ``TrackInstances``.  Reads the device (tests and debugging)."""
        ids = self.ids[b]
        slots = (ids >= 0).nonzero().squeeze(1)
        slots = slots[torch.argsort(ids[slots])]
        return {name: getattr(self, name)[b][slots] for name in ROW_FIELDS}
