"""``ClipLoader``: a clip dataset (datasets.py) to the batches ``train.fit`` reads, made one or more clips ahead of the
train step on a second thread and a second stream.

    loader = ClipLoader(dataset, device, seed=config["SEED"], shuffle=True, rank=0, world_size=1,
                        prefetch=2, decode_threads=2)
    optimizer, scheduler, states = fit(config, model, criterion, loader.epoch, device=device)

``loader.epoch(e)`` is a generator.  At its first ``next()`` it calls ``dataset.set_epoch(e)``, draws the epoch's
order and starts ONE producer thread (no worker processes: a rank has about two CPUs, and the entropy stage already
runs on ``decode_threads`` threads of its own inside the library).  Per clip the producer reads the files, takes the
frame size from the JPEG headers, asks the dataset for the augmentation plan, runs the host entropy stage into a pinned
ring that belongs to this loader, and queues upload, device decode (data/jpeg.py) and ``augment_clip`` /
``augment_static_clip`` on the loader's own stream.  Ids, labels and boxes of all frames travel in one pinned buffer
and one non-blocking copy, so the engine finds the ground truth on the device (its "resident" path).  The batch is
``clip_batch``'s, plus ``batch["nested"]``, the padded ``NestedTensor`` the frames are views of, and on a CUDA device
``batch["infos_buffer"]``, the one device buffer the ground-truth tensors are views of.

What is drawn ("Clip loader"): the order is ``torch.randperm(n, generator=manual_seed(seed + e))`` (or
``arange``), padded by wrapping to a multiple of ``world_size`` and strided ``rank::world_size`` --
``DistributedSampler``'s rule; the ``random.Random`` and ``np.random.RandomState`` of a sample are derived from
``(seed, e, dataset index)`` alone, the interval is drawn first, then the plan.  So clip k of epoch e is the same bytes
for any ``prefetch``, any ``decode_threads``, on the CPU or the GPU, and after a restart.

Streams: the producer's work is ordered by the loader stream only; it never synchronises the device or the training
stream (the one-time uploads of ``frames.py`` / ``augment.py`` tables and masks wait on the stream they were queued
on, which here is the loader's).  A bounded hand-over of depth ``prefetch`` carries ``(batch, event)``; the consumer
makes its current stream wait for the event and marks every device tensor it is handed with ``record_stream``: they
were allocated on the loader stream and are freed by the consumer.

``device="cpu"`` runs the same code on the host statements of decode and augment: the bit-exact yardstick.

One ``epoch()`` generator of a loader (and of a dataset) is live at a time.  Closing or dropping it stops and joins the
producer; an exception in the producer is raised by the ``next()`` of the clip it belongs to.
"""
from __future__ import annotations

import collections
import random
import threading
import time
from typing import Iterator, List, Optional

import numpy as np
import torch

from . import augment as _augment
from . import jpeg as _jpeg
from . import static_clip as _static_clip
from .datasets import ClipDataset


def epoch_order(n: int, epoch: int, seed: int, shuffle: bool = True, rank: int = 0, world_size: int = 1) -> List[int]:
    """The dataset indices of one rank's epoch, in order (``DistributedSampler``'s rule without ``drop_last``)."""
    if not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} is not in 0 .. {world_size - 1}")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        order = torch.randperm(n, generator=g).tolist()
    else:
        order = list(range(n))
    if world_size > 1 and n:
        total = -(-n // world_size) * world_size
        while len(order) < total:
            order += order[:total - len(order)]
        order = order[rank::world_size]
    return order


def sample_rngs(seed: int, epoch: int, index: int):
    """(``random.Random``, ``np.random.RandomState``) of dataset entry ``index`` in ``epoch``: a function of the three
    numbers only (two children of one ``np.random.SeedSequence``)."""
    a, b = np.random.SeedSequence([int(seed), int(epoch), int(index)]).spawn(2)
    return (random.Random(int.from_bytes(a.generate_state(4).tobytes(), "little")),
            np.random.RandomState(b.generate_state(8)))


class _Handover:
    """A bounded buffer between one producer and one consumer that either side can close."""

    def __init__(self, depth: int):
        self.depth = depth
        self.items = collections.deque()
        self.cond = threading.Condition()
        self.closed = False

    def put(self, item) -> bool:
        """Blocks while the buffer is full; False once the consumer has closed it (the item is dropped)."""
        with self.cond:
            self.cond.wait_for(lambda: self.closed or len(self.items) < self.depth)
            if self.closed:
                return False
            self.items.append(item)
            self.cond.notify_all()
            return True

    def get(self):
        with self.cond:
            self.cond.wait_for(lambda: bool(self.items))
            item = self.items.popleft()
            self.cond.notify_all()
            return item

    def close(self) -> None:
        with self.cond:
            self.closed = True
            self.items.clear()
            self.cond.notify_all()


_END = object()


class _Failure:
    def __init__(self, error: BaseException):
        self.error = error


class ClipLoader:
    def __init__(self, dataset: ClipDataset, device, seed: int = 0, shuffle: bool = True, rank: int = 0,
                 world_size: int = 1, prefetch: int = 2, decode_threads: int = 2, bgr: bool = False):
        """``prefetch``: how many finished clips may wait for the train step (at least 1).  ``decode_threads``: host
        threads of the entropy stage, capped at the library's ``JPEGOPS_MAX_THREADS``; never size it by the machine's
        CPU count.  ``bgr``: decode to B, G, R and let the augmentation swap back (the result is the same bytes)."""
        if prefetch < 1 or decode_threads < 1:
            raise ValueError("prefetch and decode_threads must be at least 1")
        if not 0 <= rank < world_size:
            raise ValueError(f"rank {rank} is not in 0 .. {world_size - 1}")
        self.dataset = dataset
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.seed, self.shuffle, self.rank, self.world_size = int(seed), bool(shuffle), int(rank), int(world_size)
        self.prefetch, self.bgr = int(prefetch), bool(bgr)
        from .. import _jpeg_lib            # no substitute: a missing library is an error
        self.decode_threads = min(int(decode_threads), _jpeg_lib.MAX_THREADS)
        self._staging = _jpeg._Staging(self.prefetch + 1)
        self.timings: Optional[list] = None     # a list: load() appends the host seconds of each clip's stages
        self._stream: Optional[torch.cuda.Stream] = None
        self._thread: Optional[threading.Thread] = None

    # ------------------------------------------------------------------------------------------ what is drawn
    def order(self, epoch: int) -> List[int]:
        """This rank's dataset indices of ``epoch`` (call after ``dataset.set_epoch(epoch)``)."""
        return epoch_order(len(self.dataset), epoch, self.seed, self.shuffle, self.rank, self.world_size)

    # ------------------------------------------------------------------------------------------ one clip
    def _decode(self, streams) -> torch.Tensor:
        frames = _jpeg.decode_jpegs(streams, self.device, threads=self.decode_threads, bgr=self.bgr, fallback=True,
                                    staging=self._staging)
        if isinstance(frames, list):        # mixed sampling factors, or streams only Pillow reads: frame by frame
            if any(f.shape != frames[0].shape for f in frames):
                raise ValueError(f"the frames of a clip differ in size: {[tuple(f.shape[:2]) for f in frames]}")
            frames = torch.stack(frames)
        return frames

    def _pack_infos(self, infos: List[dict]):
        """ids, labels and boxes of every frame as views of ONE device buffer that one non-blocking copy from pinned
        memory fills (int64 ids and labels in front, float32 boxes behind them).  Returns (infos, the buffer)."""
        counts = [int(i["ids"].numel()) for i in infos]
        n = sum(counts)
        host = torch.empty(n * 32, dtype=torch.uint8, pin_memory=True)
        dev = torch.empty(n * 32, dtype=torch.uint8, device=self.device)
        host_long, host_box = host[:n * 16].view(torch.int64), host[n * 16:].view(torch.float32)
        dev_long, dev_box = dev[:n * 16].view(torch.int64), dev[n * 16:].view(torch.float32)
        out, lo = [], 0
        for info, k in zip(infos, counts):
            host_long[2 * lo:2 * lo + k] = info["ids"]
            host_long[2 * lo + k:2 * lo + 2 * k] = info["labels"]
            host_box[4 * lo:4 * (lo + k)] = info["boxes"].reshape(-1)
            out.append({"ids": dev_long[2 * lo:2 * lo + k], "labels": dev_long[2 * lo + k:2 * lo + 2 * k],
                        "boxes": dev_box[4 * lo:4 * (lo + k)].view(k, 4)})
            lo += k
        if n:
            dev.copy_(host, non_blocking=True)
        return out, dev

    def load(self, epoch: int, index: int) -> dict:
        """Dataset entry ``index`` of ``epoch`` (``dataset.set_epoch(epoch)`` done) as a batch, queued on the current
        stream of the loader's device; nothing here waits for the device."""
        t0, cpu0 = time.perf_counter(), time.thread_time()
        rng, np_rng = sample_rngs(self.seed, epoch, index)
        sample = self.dataset.sample(index, rng)
        paths = sample.paths[:1] if sample.static else sample.paths
        streams = []
        for path in paths:
            with open(path, "rb") as f:
                streams.append(np.frombuffer(f.read(), dtype=np.uint8))
        sizes = None
        try:
            sizes = [(f.height, f.width) for f in (_jpeg.parse_jpeg(a) for a in streams)]
        except _jpeg.UnsupportedJpeg:
            pass                            # Pillow reads it below (or the decode raises this again)
        if sizes is not None and any(s != sizes[0] for s in sizes):
            raise ValueError(f"the frames of a clip differ in size: {sizes} ({paths})")
        t1 = time.perf_counter()
        frames = self._decode(streams)
        t2 = time.perf_counter()
        h, w = int(frames.shape[1]), int(frames.shape[2])
        plan = self.dataset.sample_plan(h, w, rng, np_rng, sample.static)
        if sample.static:
            nested, infos = _static_clip.augment_static_clip(frames[0], sample.infos[0], plan, len(sample.paths),
                                                             bgr=self.bgr, overflow_bbox=sample.overflow_bbox)
        else:
            nested, infos = _augment.augment_clip(frames, sample.infos, plan, bgr=self.bgr,
                                                  overflow_bbox=sample.overflow_bbox)
        batch = _augment.clip_batch(nested, infos)
        batch["nested"] = nested
        if self.device.type == "cuda":
            batch["infos"][0], batch["infos_buffer"] = self._pack_infos(infos)
        if self.timings is not None:        # (tools/bench_loader.py) wall seconds per stage, CPU seconds of this thread
            t3 = time.perf_counter()
            self.timings.append({"read": t1 - t0, "decode": t2 - t1, "augment": t3 - t2,
                                 "thread_cpu": time.thread_time() - cpu0})
        return batch

    # ------------------------------------------------------------------------------------------ the epoch
    def _produce(self, epoch: int, order: List[int], handover: _Handover) -> None:
        cuda = self.device.type == "cuda"
        try:
            if cuda:
                torch.cuda.set_device(self.device)
                if self._stream is None:
                    self._stream = torch.cuda.Stream(self.device)
            for index in order:
                try:
                    if cuda:
                        with torch.cuda.stream(self._stream):
                            batch = self.load(epoch, index)
                            event = self._stream.record_event()
                    else:
                        batch, event = self.load(epoch, index), None
                except BaseException as e:      # noqa: B902 -- handed to the consumer, whatever it is
                    handover.put(_Failure(e))
                    return
                if not handover.put((batch, event)):
                    return
                del batch
            handover.put(_END)
        except BaseException as e:              # noqa: B902
            handover.put(_Failure(e))

    def epoch(self, epoch: int) -> Iterator[dict]:
        """The batches of this rank's ``epoch``, in order, each ready for the consumer's current stream (``fit``'s
        ``make_batches``).  The producer thread lives from the first ``next()`` until the generator ends, is closed or
        is dropped."""
        if self._thread is not None and self._thread.is_alive():
            raise RuntimeError("an epoch() generator of this loader is still live: close it first")
        self.dataset.set_epoch(epoch)
        order = self.order(epoch)
        handover = _Handover(self.prefetch)
        thread = threading.Thread(target=self._produce, args=(epoch, order, handover), name="clip-loader",
                                  daemon=True)
        self._thread = thread
        thread.start()
        try:
            while True:
                item = handover.get()
                if item is _END:
                    return
                if isinstance(item, _Failure):
                    raise item.error
                batch, event = item
                if event is not None:
                    current = torch.cuda.current_stream(self.device)
                    current.wait_event(event)
                    nested = batch["nested"]
                    for t in (nested.tensors, nested.masks, batch["infos_buffer"]):
                        t.record_stream(current)
                yield batch
                del item, batch
        finally:
            handover.close()
            thread.join()
            self._thread = None
