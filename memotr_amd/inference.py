"""Online tracking of one video sequence: the frame loop of the reference's ``Submitter.run``
(submit_engine.py:58-120) and its result writers (:133-184), without the dataset / logger plumbing.

    tracker = SequenceTracker(model, dataset_name="DanceTrack", det_score_thresh=0.5, ...)
    for frame_idx, (image, (ori_h, ori_w)) in enumerate(frames):      # image: (3,H,W) normalised tensor
        result = tracker.step(image, ori_h, ori_w)                     # filtered TrackInstances on the CPU
        lines += tracker.mot_lines(frame_idx, result)                  # "frame,id,x,y,w,h,1,-1,-1,-1"

One frame of lookahead (a recorded sequence always has it): ``tracker.step(image, h, w, next_image=frames[i + 1])``
queues the backbone + encoder of the NEXT frame -- the half of a frame that does not depend on the tracks, ~3/4 of
its kernel time -- on a side stream before the host blocks on this frame's scores, so the GPU works through it while
the host does the track bookkeeping and issues the query updater (results are identical; tests/test_model_gpu.py).

From decoded frames (uint8, H x W x 3, e.g. what ``cv2.imread`` returns) instead of normalised tensors:

    for frame_idx, result in tracker.track(frames_u8, bgr=True):       # resize + normalise + pad on the GPU, lookahead
        lines += tracker.mot_lines(frame_idx, result)

``track`` is ``step_raw(frame, next_frame)`` in a loop: upload through pinned memory, one kernel (data/frames.py),
then the same encode / decode path as ``step``.

From JPEG files or byte streams, the decode in front (data/jpeg.py: Huffman stage on one host thread, a frame ahead;
IDCT and colour on the GPU, queued on the side stream with the rest of the next frame's work):

    for frame_idx, result in tracker.track_jpeg(paths, bgr=False):
        lines += tracker.mot_lines(frame_idx, result)

With an annotated JPEG per frame on the side (render.py: boxes and ids drawn and the frame encoded on the GPU, the
Huffman stage and the file a frame behind on one worker thread):

    with AnnotatedWriter("out/") as writer:
        for frame_idx, result in tracker.track_annotated(frames_or_paths, writer): ...

Without a result on the host per frame (a submit run needs the rows of a sequence once; results.py, submit.py):

    log = ResultLog(device)
    n_frames = tracker.track_logged(frames_or_paths, log)              # one launch per frame instead of the read
    lines = log.mot_lines("DanceTrack")

``use_motion=True`` (the reference's ``USE_MOTION``): after the query updater, the reference point of every track that
is being missed is moved along its mean box velocity (models/motion.py: device state, one launch, no synchronisation).
"""
from __future__ import annotations

from typing import List

import torch

from .data.frames import preprocess_frames, target_size
from .models.runtime_tracker import RuntimeTracker
from .models.utils import get_model
from .structures.track_instances import TrackInstances
from .utils.box_ops import box_cxcywh_to_xyxy
from .utils.nested_tensor import tensor_list_to_nested_tensor

BDD_CLS2LABEL = {1: "pedestrian", 2: "rider", 3: "car", 4: "truck", 5: "bus", 6: "train", 7: "motorcycle",
                 8: "bicycle"}
MOT_STYLE = ("DanceTrack", "SportsMOT", "MOT17", "MOT17_SPLIT")


class SequenceTracker:
    def __init__(self, model, dataset_name: str = "DanceTrack", det_score_thresh: float = 0.7,
                 track_score_thresh: float = 0.6, result_score_thresh: float = 0.7, miss_tolerance: int = 5,
                 use_dab: bool = True, area_thresh: int = 100, raw_size=(800, 1536), use_motion: bool = False,
                 motion_lambda: float = 0.5, motion_min_length: int = 3, motion_max_length: int = 5,
                 side_stream=None):
        from .utils.host import respect_cpu_quota
        respect_cpu_quota()           # (a container's CFS quota vs torch's machine-sized thread pool: utils/host.py)
        self.model = model.eval()
        self.core = get_model(model)
        self.dataset_name = dataset_name
        self.result_score_thresh = result_score_thresh
        self.area_thresh = area_thresh
        self.use_dab = use_dab
        self.device = next(self.core.parameters()).device
        self.tracker = RuntimeTracker(det_score_thresh=det_score_thresh, track_score_thresh=track_score_thresh,
                                      miss_tolerance=miss_tolerance, use_dab=use_dab, use_motion=use_motion,
                                      motion_min_length=motion_min_length, motion_max_length=motion_max_length)
        self.use_motion = use_motion  # the reference's USE_MOTION post-process (models/motion.py); off in its configs
        self.motion_lambda = motion_lambda
        self.tracks: List[TrackInstances] = [TrackInstances(hidden_dim=self.core.hidden_dim,
                                                            num_classes=self.core.num_classes,
                                                            use_dab=use_dab).to(self.device)]
        self._pending = None          # (image, encode result, event): the next frame's encode half, queued ahead
        self._slot = 0                # encode calls alternate between two graph slots (one may still be read)
        self._side = side_stream      # the lookahead's stream; None: one of its own, made when first needed.  (Trackers
        #                               made one after another can share one: which hardware queue a new stream lands on
        #                               decides whether the lookahead overlaps at all -- profiles/submit_log.md)
        self.raw_size = raw_size      # step_raw: (short side, longest long side) of the resized frame; the reference's
        self._staging = [None, None]  # step_raw: two pinned upload buffers, each with the event of its last copy
        self._staging_i = 0

    @classmethod
    def from_config(cls, model, config: dict) -> "SequenceTracker":
        return cls(model, dataset_name=config["DATASET"], det_score_thresh=config["DET_SCORE_THRESH"],
                   track_score_thresh=config["TRACK_SCORE_THRESH"], result_score_thresh=config["RESULT_SCORE_THRESH"],
                   miss_tolerance=config["MISS_TOLERANCE"], use_dab=config["USE_DAB"],
                   use_motion=config.get("USE_MOTION", False), motion_lambda=config.get("MOTION_LAMBDA", 0.5),
                   motion_min_length=config.get("MOTION_MIN_LENGTH", 3),
                   motion_max_length=config.get("MOTION_MAX_LENGTH", 5))

    @torch.no_grad()
    def step(self, image: torch.Tensor, ori_h: int, ori_w: int, next_image: torch.Tensor = None) -> TrackInstances:
        """One frame: model -> runtime tracker -> query updater; returns the reportable tracks (CPU, boxes as
        xyxy pixels of the original image, low-score / tiny boxes removed).  ``next_image``: the frame the next call
        will pass (the same tensor object), whose encode half is then queued ahead on a side stream."""
        enc = self._encoded(image)
        res = self.model(tracks=self.tracks, encoded=enc)        # decoder + heads on this frame's encode result
        if next_image is not None:
            self._prefetch(next_image)
        previous, new = self.tracker.update(model_outputs=res, tracks=self.tracks)
        self.tracks = self.core.postprocess_single_frame(previous, new, None)
        if self.use_motion:
            self._extrapolate_missed()
        return self._report(self.tracks[0], ori_h, ori_w)

    def _extrapolate_missed(self) -> None:
        """submit_engine.py:78-87: the reference point of a track that is being missed moves along its mean box
        velocity -- one launch, and a NEW ref_pts tensor (the updater's captured graphs may own the old one)."""
        t = self.tracks[0]
        if len(t) > 0:
            t.ref_pts = self.tracker.motions.extrapolate(t.ids, t.disappear_time, t.last_appear_boxes, t.ref_pts,
                                                         self.motion_lambda)

    def _report(self, t: TrackInstances, ori_h: int, ori_w: int) -> TrackInstances:
        """The reportable tracks on the CPU (submit_engine.py:95-112): score and area filters, xyxy pixel boxes.
        The fields a result needs (ids, boxes, scores, labels) leave the device as ONE packed tensor through a
        pinned buffer and one event wait -- `.to("cpu")` field by field is a blocking copy per field, embeddings
        included."""
        n, K = len(t), t.scores.shape[-1] if t.scores.dim() == 2 else 0
        if n and t.boxes.is_cuda:
            packed = torch.cat((t.boxes.double(), t.scores.double().reshape(n, K), t.ids.double()[:, None],
                                t.labels.double()[:, None]), dim=1)
            host = torch.empty(packed.shape, dtype=packed.dtype, pin_memory=True)
            host.copy_(packed, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            done.synchronize()
        elif n:
            host = torch.cat((t.boxes.double(), t.scores.double().reshape(n, K), t.ids.double()[:, None],
                              t.labels.double()[:, None]), dim=1)
        else:
            host = torch.zeros((0, 6 + K), dtype=torch.float64)
        boxes, scores = host[:, :4].float(), host[:, 4:4 + K].float()
        ids, labels = host[:, 4 + K].long(), host[:, 5 + K].long()
        area = boxes[:, 2] * ori_w * boxes[:, 3] * ori_h
        keep = torch.ones((host.shape[0],), dtype=torch.bool)
        if host.shape[0]:
            keep = torch.max(scores, dim=-1).values > self.result_score_thresh
            keep = keep & (area > self.area_thresh)
        out = TrackInstances(hidden_dim=t.hidden_dim, num_classes=t.num_classes, use_dab=self.use_dab)
        out.ids, out.labels, out.scores, out.area = ids[keep], labels[keep], scores[keep], area[keep]
        out.boxes = box_cxcywh_to_xyxy(boxes[keep]) * torch.as_tensor([ori_w, ori_h, ori_w, ori_h], dtype=torch.float)
        return out

    def _encode(self, image: torch.Tensor) -> dict:
        frame = tensor_list_to_nested_tensor([image]).to(self.device)
        frame.encode_slot = self._slot          # (models/infer_graphs.py: one static `memory` per slot)
        frame.encode_static_ok = True           # ... read in place: this loop alternates the two slots itself
        self._slot ^= 1
        return self.model(frame=frame, stage="encode")

    def _encoded(self, image: torch.Tensor) -> dict:
        """This frame's encode result: the one queued ahead by the previous step, or computed now."""
        pending, self._pending = self._pending, None
        if pending is not None and pending[0] is image:
            torch.cuda.current_stream(self.device).wait_event(pending[2])
            return pending[1]
        if pending is not None:                 # a different frame arrived: nothing may still write the slot buffers
            torch.cuda.current_stream(self.device).wait_event(pending[2])
        return self._encode(image)

    def _prefetch(self, image: torch.Tensor) -> None:
        if self.device.type != "cuda":
            return
        main = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        side = self._side
        side.wait_stream(main)                  # the image (and this frame's decode reading the OTHER slot) are on main
        with torch.cuda.stream(side):
            enc = self._encode(image)
            event = side.record_event()
        if image.is_cuda:
            image.record_stream(side)
        for v in enc.values():                  # produced on the side stream, consumed on main
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(main)
        self._pending = (image, enc, event)

    # ------------------------------------------------------------------ raw uint8 frames
    @torch.no_grad()
    def step_raw(self, frame_u8, next_frame_u8=None, *, bgr: bool = False) -> TrackInstances:
        """``step`` on a decoded frame: (H, W, 3) uint8, torch or numpy, RGB (``bgr=True``: cv2's order); ``ori_h`` and
        ``ori_w`` are the frame's.  The frame is uploaded through a reusable pinned buffer with a non-blocking copy and
        turned into the padded normalised batch by one kernel (data/frames.py), then takes the encode path of ``step``
        (same slot alternation).  ``next_frame_u8``: the frame the next call will pass (the same object, unchanged until
        then); its upload, kernel and encode half are queued on the side stream as ``_prefetch`` does for ``step``."""
        ori_h, ori_w = self._advance_raw(frame_u8, next_frame_u8, bgr=bgr)
        return self._report(self.tracks[0], ori_h, ori_w)

    @torch.no_grad()
    def _advance_raw(self, frame_u8, next_frame_u8=None, *, bgr: bool = False):
        """``step_raw`` up to the report: ``self.tracks`` are this frame's; returns ``(ori_h, ori_w)``."""
        ori_h, ori_w = int(frame_u8.shape[0]), int(frame_u8.shape[1])
        pending, self._pending = self._pending, None
        if pending is not None:
            torch.cuda.current_stream(self.device).wait_event(pending[2])
        enc = pending[1] if pending is not None and pending[0] is frame_u8 else self._encode_raw(frame_u8, bgr)
        res = self.model(tracks=self.tracks, encoded=enc)
        if next_frame_u8 is not None:
            self._prefetch_raw(next_frame_u8, bgr)
        previous, new = self.tracker.update(model_outputs=res, tracks=self.tracks)
        self.tracks = self.core.postprocess_single_frame(previous, new, None)
        if self.use_motion:
            self._extrapolate_missed()
        return ori_h, ori_w

    def track(self, frames, *, bgr: bool = False):
        """Generator over an iterable of uint8 frames: yields ``(frame_idx, result)``, one frame of lookahead."""
        it = iter(frames)
        done = object()
        cur, idx = next(it, done), 0
        while cur is not done:
            nxt = next(it, done)
            yield idx, self.step_raw(cur, None if nxt is done else nxt, bgr=bgr)
            cur, idx = nxt, idx + 1

    def track_jpeg(self, files_or_bytes, *, bgr: bool = False):
        """``track`` with the decode in front: an iterable of JPEG paths or byte streams, yields ``(frame_idx,
        result)``.  ``bgr``: the channel order the frames are decoded to (the model sees the same either way).

        While frame i runs, one worker thread Huffman-decodes frame i + 2 into a pinned buffer (ctypes releases the
        interpreter lock for the call), and frame i + 1's coefficients are uploaded and turned into pixels on the side
        stream, in front of its resize and encode half that ``step_raw`` queues there.  The results are those of
        ``track`` on the same frames decoded by Pillow: the pixels are equal byte for byte."""
        for idx, _, result in self._track_jpeg_frames(files_or_bytes, bgr):
            yield idx, result

    def _track_jpeg_frames(self, files_or_bytes, bgr: bool, step=None):
        """The loop of ``track_jpeg``; yields ``(frame_idx, frame, result)`` with the decoded frame on the device.
        ``step``: what is called per frame in place of ``step_raw`` (``track_logged``: ``_advance_raw``)."""
        step = self.step_raw if step is None else step
        if self.device.type != "cuda":
            from .data.jpeg import decode_jpeg
            yield from self._track_frames((decode_jpeg(x, "cpu", bgr=bgr) for x in files_or_bytes), bgr, step)
            return
        from concurrent.futures import ThreadPoolExecutor
        from .data import jpeg as J
        staging = J._Staging(3)             # written by the worker / being copied / copied a frame ago

        def entropy(item):
            a = J._as_bytes(item)
            try:
                buf, slot = staging.take(J._frame_words(J.parse_jpeg(a)))
                return J.entropy_decode(a, pinned=buf), slot
            except J.UnsupportedJpeg as e:  # a stream only Pillow reads: decoded on the host, uploaded as pixels
                return J._fallback(a, torch.device("cpu"), bgr, e), None

        def pixels(job, stream):
            coefs, slot = job
            with torch.cuda.stream(stream):
                if slot is None:
                    return self._upload(coefs)
                frame = J._device_stage(coefs.flat[None], coefs.info, 1, self.device, bgr)[0]
                staging.copied(slot, stream.record_event())
            return frame

        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        it = iter(files_or_bytes)
        done = object()
        with ThreadPoolExecutor(max_workers=1) as pool:
            ahead = lambda: (lambda x: None if x is done else pool.submit(entropy, x))(next(it, done))  # noqa: E731
            first, job = ahead(), ahead()
            if first is None:
                return
            cur, idx = pixels(first.result(), torch.cuda.current_stream(self.device)), 0
            while cur is not None:
                nxt = None
                if job is not None:
                    decoded, job = job.result(), ahead()
                    nxt = pixels(decoded, self._side)
                yield idx, cur, step(cur, nxt, bgr=bgr)
                cur, idx = nxt, idx + 1

    def _track_frames(self, frames, bgr: bool, step=None):
        """``track`` that keeps hold of the device copy: yields ``(frame_idx, frame on the device, result)``.  The
        upload ``step_raw`` would make is made here, on the stream it would be made on (this frame's on the current
        stream, the next frame's on the side stream), and ``step_raw`` is handed the device tensor: one upload."""
        step = self.step_raw if step is None else step
        cuda = self.device.type == "cuda"
        if cuda and self._side is None:
            self._side = torch.cuda.Stream(self.device)

        def upload(frame, stream):
            if not cuda:
                return torch.from_numpy(frame) if not torch.is_tensor(frame) else frame
            with torch.cuda.stream(stream):
                return self._upload(frame)

        it = iter(frames)
        done = object()
        first = next(it, done)
        if first is done:
            return
        cur, idx = upload(first, torch.cuda.current_stream(self.device) if cuda else None), 0
        while cur is not None:
            nxt = next(it, done)
            nxt = None if nxt is done else upload(nxt, self._side)
            yield idx, cur, step(cur, nxt, bgr=bgr)
            cur, idx = nxt, idx + 1

    def track_annotated(self, source, writer, *, bgr: bool = False):
        """``track`` / ``track_jpeg`` with an annotated JPEG per frame on the side (render.AnnotatedWriter): ``source``
        is an iterable of uint8 frames, or of JPEG paths / byte streams; yields exactly what they yield.  The writer is
        handed the device copy of the frame the tracker already made -- no second upload -- and queues its draw and
        encode launches on its own stream; ``bgr`` is the frames' channel order, for the model and the writer alike.
        The caller closes the writer (it is a context manager)."""
        import itertools
        import os
        it = iter(source)
        done = object()
        first = next(it, done)
        if first is done:
            return
        stream_like = isinstance(first, (str, bytes, bytearray, memoryview, os.PathLike)) or \
            (hasattr(first, "ndim") and first.ndim == 1)
        items = itertools.chain([first], it)
        frames = self._track_jpeg_frames(items, bgr) if stream_like else self._track_frames(items, bgr)
        for idx, frame, result in frames:
            writer.add(idx, frame, result, bgr=bgr)
            yield idx, result

    def track_logged(self, source, log, *, bgr: bool = False) -> int:
        """``track`` / ``track_jpeg`` (``source`` as for ``track_annotated``) with the reportable rows of every frame
        appended to ``log`` (results.ResultLog) on the device instead of being brought to the host: one launch per frame
        in place of ``_report``'s packed copy, event wait and host filter.  Read them once, after the sequence, with
        ``log.read()`` / ``log.mot_lines`` / ``log.bdd_frames``.  Returns the number of frames."""
        import itertools
        import os
        it = iter(source)
        done = object()
        first = next(it, done)
        if first is done:
            return 0

        def append(idx, ori_h, ori_w):
            t = self.tracks[0]
            log.append(t.boxes, t.scores, t.ids, t.labels, idx, ori_h, ori_w, self.result_score_thresh,
                       self.area_thresh)

        stream_like = isinstance(first, (str, bytes, bytearray, memoryview, os.PathLike)) or \
            (hasattr(first, "ndim") and first.ndim == 1)
        if stream_like:
            n = 0
            for idx, _, size in self._track_jpeg_frames(itertools.chain([first], it), bgr, step=self._advance_raw):
                append(idx, *size)
                n = idx + 1
            return n
        cur, idx = first, 0                     # the loop of ``track``
        while cur is not done:
            nxt = next(it, done)
            append(idx, *self._advance_raw(cur, None if nxt is done else nxt, bgr=bgr))
            cur, idx = nxt, idx + 1
        return idx

    def _upload(self, frame_u8) -> torch.Tensor:
        """The frame on the device, copied on the current stream.  Pageable host memory goes through one of two pinned
        buffers (a copy from pageable memory blocks the host); a frame that is pinned already is copied as it is."""
        frame = torch.from_numpy(frame_u8) if not torch.is_tensor(frame_u8) else frame_u8
        if self.device.type != "cuda" or frame.device == self.device:
            return frame
        if frame.is_cuda:
            return frame.to(self.device)
        stream = torch.cuda.current_stream(self.device)
        host, slot = frame, None
        if not (frame.is_pinned() and frame.is_contiguous()):
            slot, self._staging_i = self._staging_i, self._staging_i ^ 1
            entry = self._staging[slot]
            if entry is None or entry[0].shape != frame.shape:
                entry = [torch.empty(frame.shape, dtype=torch.uint8, pin_memory=True), None]
                self._staging[slot] = entry
            elif entry[1] is not None:
                entry[1].synchronize()          # the copy out of this buffer two uploads ago (long done)
            host = entry[0]
            host.copy_(frame)
        dev = torch.empty(host.shape, dtype=torch.uint8, device=self.device)
        dev.copy_(host, non_blocking=True)
        if slot is not None:
            self._staging[slot][1] = stream.record_event()
        return dev

    def _encode_raw(self, frame_u8, bgr: bool, after=None) -> dict:
        dev = self._upload(frame_u8)
        if after is not None:                   # (the upload itself depends on nothing that stream has queued)
            torch.cuda.current_stream(self.device).wait_stream(after)
        frame = preprocess_frames(dev, bgr=bgr, size=target_size(dev.shape[0], dev.shape[1], *self.raw_size))
        frame.encode_slot = self._slot
        frame.encode_static_ok = True
        self._slot ^= 1
        return self.model(frame=frame, stage="encode")

    def _prefetch_raw(self, frame_u8, bgr: bool) -> None:
        if self.device.type != "cuda":
            return
        main = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        side = self._side
        with torch.cuda.stream(side):
            # upload now, kernel and encode behind this frame's decode on main (it reads the OTHER slot)
            enc = self._encode_raw(frame_u8, bgr, after=main)
            event = side.record_event()
        if torch.is_tensor(frame_u8) and frame_u8.is_cuda:
            frame_u8.record_stream(side)
        for v in enc.values():                  # produced on the side stream, consumed on main
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(main)
        self._pending = (frame_u8, enc, event)

    def mot_lines(self, frame_idx: int, tracks: TrackInstances) -> List[str]:
        if self.dataset_name not in MOT_STYLE:
            raise ValueError(f"{self.dataset_name} dataset is not supported for submit process.")
        lines = []
        for box, tid in zip(tracks.boxes.tolist(), tracks.ids.tolist()):
            x1, y1, x2, y2 = box
            lines.append(f"{frame_idx + 1},{tid},{x1},{y1},{x2 - x1},{y2 - y1},1,-1,-1,-1\n")
        return lines

    @staticmethod
    def bdd_frame_result(frame_idx: int, tracks: TrackInstances, img_path: str) -> dict:
        name = img_path.split("/")[-1]
        labels = []
        for box, tid, lab in zip(tracks.boxes.tolist(), tracks.ids.tolist(), tracks.labels.tolist()):
            x1, y1, x2, y2 = box
            labels.append({"id": str(tid), "category": BDD_CLS2LABEL[lab + 1],
                           "box2d": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}})
        return {"name": name, "videoName": name[:-12], "frameIndex": frame_idx, "labels": labels}
