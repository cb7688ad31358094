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
The rules of that queue -- slots, waits, ``record_stream`` -- are ``lookahead.Lookahead``'s.

From decoded frames (uint8, H x W x 3, e.g. what ``cv2.imread`` returns) instead of normalised tensors:

    for frame_idx, result in tracker.track(frames_u8, bgr=True):       # resize + normalise + pad on the GPU, lookahead
        lines += tracker.mot_lines(frame_idx, result)

``track`` is ``step_raw(frame, next_frame)`` in a loop (``lookahead.frame_pairs``): upload through pinned memory
(``utils.host.PinnedUploader``), one kernel (data/frames.py), then the same encode / decode path as ``step``.

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

import itertools
from typing import List

import torch

from .data.frames import preprocess_frames, target_size
from .lookahead import Lookahead, frame_pairs, is_stream_like
from .models.runtime_tracker import RuntimeTracker
from .models.utils import get_model
from .structures.track_instances import TrackInstances
from .utils.box_ops import box_cxcywh_to_xyxy
from .utils.host import PinnedUploader, to_host
from .utils.nested_tensor import tensor_list_to_nested_tensor

BDD_CLS2LABEL = {1: "pedestrian", 2: "rider", 3: "car", 4: "truck", 5: "bus", 6: "train", 7: "motorcycle",
                 8: "bicycle"}
MOT_STYLE = ("DanceTrack", "SportsMOT", "MOT17", "MOT17_SPLIT")


def pack_tracks(boxes, scores, ids, labels, K: int) -> torch.Tensor:
    """The fields a result needs as ONE float64 tensor (..., 6 + K): boxes, scores, id, label."""
    return torch.cat((boxes.double(), scores.double().reshape(*boxes.shape[:-1], K), ids.double()[..., None],
                      labels.double()[..., None]), dim=-1)


def reportable(rows: torch.Tensor, K: int, ori_h: int, ori_w: int, score_thresh: float, area_thresh: float,
               **track_options) -> TrackInstances:
    """The reportable tracks of the packed host ``rows`` (n, 6 + K) (submit_engine.py:95-112): score and area
    filters, xyxy pixel boxes."""
    boxes, scores = rows[:, :4].float(), rows[:, 4:4 + K].float()
    ids, labels = rows[:, 4 + K].long(), rows[:, 5 + K].long()
    area = boxes[:, 2] * ori_w * boxes[:, 3] * ori_h
    keep = torch.ones((rows.shape[0],), dtype=torch.bool)
    if rows.shape[0]:
        keep = torch.max(scores, dim=-1).values > score_thresh
        keep = keep & (area > area_thresh)
    out = TrackInstances(**track_options)
    out.ids, out.labels, out.scores, out.area = ids[keep], labels[keep], scores[keep], area[keep]
    out.boxes = box_cxcywh_to_xyxy(boxes[keep]) * torch.as_tensor([ori_w, ori_h, ori_w, ori_h], dtype=torch.float)
    return out


def mot_lines(dataset_name: str, frame_idx: int, tracks: TrackInstances) -> List[str]:
    if dataset_name not in MOT_STYLE:
        raise ValueError(f"{dataset_name} dataset is not supported for submit process.")
    lines = []
    for box, tid in zip(tracks.boxes.tolist(), tracks.ids.tolist()):
        x1, y1, x2, y2 = box
        lines.append(f"{frame_idx + 1},{tid},{x1},{y1},{x2 - x1},{y2 - y1},1,-1,-1,-1\n")
    return lines


def bdd_frame_result(frame_idx: int, tracks: TrackInstances, img_path: str) -> dict:
    name = img_path.split("/")[-1]
    labels = []
    for box, tid, lab in zip(tracks.boxes.tolist(), tracks.ids.tolist(), tracks.labels.tolist()):
        x1, y1, x2, y2 = box
        labels.append({"id": str(tid), "category": BDD_CLS2LABEL[lab + 1],
                       "box2d": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}})
    return {"name": name, "videoName": name[:-12], "frameIndex": frame_idx, "labels": labels}


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
        self._lookahead = Lookahead(self.model, self.device, side_stream)
        self.raw_size = raw_size      # step_raw: (short side, longest long side) of the resized frame; the reference's
        self._uploader = PinnedUploader(self.device)      # step_raw: two alternating pinned upload buffers

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
        # the image (and this frame's decode reading the OTHER slot) are on main: the side stream waits first
        self._advance(image, next_image, lambda im, after: tensor_list_to_nested_tensor([im]).to(self.device), True)
        return self._report(self.tracks[0], ori_h, ori_w)

    @torch.no_grad()
    def _advance(self, cur, nxt, frame_of, wait_first: bool) -> None:
        """A frame up to the report: ``self.tracks`` are this frame's.  ``frame_of`` and ``wait_first``: how ``cur``
        (and ``nxt``, when there is one) becomes the batch the model encodes -- ``Lookahead``'s arguments."""
        enc = self._lookahead.take(cur, frame_of)
        res = self.model(tracks=self.tracks, encoded=enc)        # decoder + heads on this frame's encode result
        if nxt is not None:
            self._lookahead.queue(nxt, frame_of, wait_first)
        previous, new = self.tracker.update(model_outputs=res, tracks=self.tracks)
        self.tracks = self.core.postprocess_single_frame(previous, new, None)
        if self.use_motion:
            self._extrapolate_missed()

    def _extrapolate_missed(self) -> None:
        """submit_engine.py:78-87: the reference point of a track that is being missed moves along its mean box
        velocity -- one launch, and a NEW ref_pts tensor (the updater's captured graphs may own the old one)."""
        t = self.tracks[0]
        if len(t) > 0:
            t.ref_pts = self.tracker.motions.extrapolate(t.ids, t.disappear_time, t.last_appear_boxes, t.ref_pts,
                                                         self.motion_lambda)

    def _report(self, t: TrackInstances, ori_h: int, ori_w: int) -> TrackInstances:
        """The reportable tracks on the CPU (``reportable``).  The fields a result needs leave the device as ONE packed
        tensor (``utils.host.to_host``), embeddings not included."""
        n, K = len(t), t.scores.shape[-1] if t.scores.dim() == 2 else 0
        rows = to_host(pack_tracks(t.boxes, t.scores, t.ids, t.labels, K)) if n else \
            torch.zeros((0, 6 + K), dtype=torch.float64)
        return reportable(rows, K, ori_h, ori_w, self.result_score_thresh, self.area_thresh,
                          hidden_dim=t.hidden_dim, num_classes=t.num_classes, use_dab=self.use_dab)

    # ------------------------------------------------------------------ raw uint8 frames
    @torch.no_grad()
    def step_raw(self, frame_u8, next_frame_u8=None, *, bgr: bool = False) -> TrackInstances:
        """``step`` on a decoded frame: (H, W, 3) uint8, torch or numpy, RGB (``bgr=True``: cv2's order); ``ori_h`` and
        ``ori_w`` are the frame's.  The frame is uploaded through a reusable pinned buffer with a non-blocking copy and
        turned into the padded normalised batch by one kernel (data/frames.py), then takes the encode path of ``step``
        (same slot alternation).  ``next_frame_u8``: the frame the next call will pass (the same object, unchanged until
        then); its upload, kernel and encode half are queued on the side stream."""
        self._advance_raw(frame_u8, next_frame_u8, bgr)
        return self._report(self.tracks[0], int(frame_u8.shape[0]), int(frame_u8.shape[1]))

    def _advance_raw(self, frame_u8, next_frame_u8, bgr: bool) -> None:
        def frame_of(frame, after):
            # upload now; the kernel and the encode go behind this frame's decode on main (it reads the OTHER slot)
            dev = self._uploader.upload(frame)
            if after is not None:
                torch.cuda.current_stream(self.device).wait_stream(after)
            return preprocess_frames(dev, bgr=bgr, size=target_size(dev.shape[0], dev.shape[1], *self.raw_size))

        self._advance(frame_u8, next_frame_u8, frame_of, False)

    def _frames(self, source, bgr: bool, on_device: bool = False, jpeg=None):
        """The loop of every ``track*``: ``frame_pairs`` over ``source`` -- uint8 frames, or JPEG paths / byte streams
        (``jpeg``; None: told from the first item).  JPEG items are decoded, and with ``on_device`` decoded frames are
        uploaded, where ``step_raw`` would have uploaded them: the current frame on the current stream, the next one
        on the side stream; ``step_raw`` is then handed the device tensor (one upload).  Otherwise the host frames
        are passed on as they are."""
        it = iter(source)
        done = object()
        first = next(it, done)
        if first is done:
            return
        items = itertools.chain([first], it)
        jpeg = is_stream_like(first) if jpeg is None else jpeg
        cuda = self.device.type == "cuda"
        side = self._lookahead.side_stream() if cuda and (jpeg or on_device) else None

        def upload(frame, ahead):
            if not cuda:
                return self._uploader.upload(frame)
            with torch.cuda.stream(side if ahead else torch.cuda.current_stream(self.device)):
                return self._uploader.upload(frame)

        if not jpeg:
            yield from frame_pairs(items, upload if on_device else None)
            return
        from .data import jpeg as J
        if not cuda:
            yield from frame_pairs(items, lambda item, ahead: J.decode_jpeg(item, "cpu", bgr=bgr))
            return
        # While frame i runs, one worker thread Huffman-decodes frame i + 2 into a pinned buffer (ctypes releases the
        # interpreter lock for the call), and frame i + 1's coefficients are uploaded and turned into pixels on the
        # side stream, in front of its resize and encode half that ``step_raw`` queues there.
        from concurrent.futures import ThreadPoolExecutor
        staging = J._Staging(3)             # written by the worker / being copied / copied a frame ago

        def entropy(item):
            a = J._as_bytes(item)
            try:
                buf, slot = staging.take(J._frame_words(J.parse_jpeg(a)))
                return J.entropy_decode(a, pinned=buf), slot
            except J.UnsupportedJpeg as e:  # a stream only Pillow reads: decoded on the host, uploaded as pixels
                return J._fallback(a, torch.device("cpu"), bgr, e), None

        def pixels(job, ahead):
            coefs, slot = job.result()
            if slot is None:
                return upload(coefs, ahead)
            stream = side if ahead else torch.cuda.current_stream(self.device)
            with torch.cuda.stream(stream):
                frame = J._device_stage(coefs.flat[None], coefs.info, 1, self.device, bgr)[0]
                staging.copied(slot, stream.record_event())
            return frame

        with ThreadPoolExecutor(max_workers=1) as pool:
            jobs = (pool.submit(entropy, item) for item in items)
            # (a job is submitted when it is read: the inner frame_pairs has read the job after the one it yields, the
            #  outer one reads a job ahead of the current frame -- the entropy stage runs two frames ahead)
            yield from frame_pairs((job for _, job, _ in frame_pairs(jobs)), pixels)

    def track(self, frames, *, bgr: bool = False):
        """Generator over an iterable of uint8 frames: yields ``(frame_idx, result)``, one frame of lookahead."""
        for idx, cur, nxt in self._frames(frames, bgr, jpeg=False):
            yield idx, self.step_raw(cur, nxt, bgr=bgr)

    def track_jpeg(self, files_or_bytes, *, bgr: bool = False):
        """``track`` with the decode in front: an iterable of JPEG paths or byte streams, yields ``(frame_idx,
        result)``.  ``bgr``: the channel order the frames are decoded to (the model sees the same either way).
        The results are those of ``track`` on the same frames decoded by Pillow: the pixels are equal byte for byte."""
        for idx, cur, nxt in self._frames(files_or_bytes, bgr, jpeg=True):
            yield idx, self.step_raw(cur, nxt, bgr=bgr)

    def track_annotated(self, source, writer, *, bgr: bool = False):
        """``track`` / ``track_jpeg`` with an annotated JPEG per frame on the side (render.AnnotatedWriter): ``source``
        is an iterable of uint8 frames, or of JPEG paths / byte streams; yields exactly what they yield.  The writer is
        handed the device copy of the frame the tracker already made -- no second upload -- and queues its draw and
        encode launches on its own stream; ``bgr`` is the frames' channel order, for the model and the writer alike.
        The caller closes the writer (it is a context manager)."""
        for idx, cur, nxt in self._frames(source, bgr, on_device=True):
            result = self.step_raw(cur, nxt, bgr=bgr)
            writer.add(idx, cur, result, bgr=bgr)
            yield idx, result

    def track_attention(self, source, writer, *, ids=None, layers=None, bgr: bool = False):
        """``track_annotated`` with the attention maps of the tracks under the boxes (attention_maps.py): ``writer`` is
        an ``attention_maps.AttentionWriter``; yields exactly what ``track_annotated`` yields.  ``ids=[...]`` (at most
        16): plane k is the map of track ``ids[k]``, tinted with ``render.palette_entry(id)`` -- the colour is constant,
        the alpha follows the level; ``ids=None``: one plane holding every live track that entered the frame plus the
        newborn, with ``HEAT_LUT``.  ``layers``: the decoder layers that count (default: all).
        The decoder runs under an ``AttentionTap`` (``self.attention_tap`` while the generator is alive), i.e. eagerly:
        the results are those of ``MEMOTR_INFER_GRAPHS=0``.  The row table of a frame is built on the device from the
        ids that entered it and the runtime tracker's newborn rows; nothing is read back per frame beyond
        ``step_raw``'s own report."""
        from . import attention_maps as A
        from .data.frames import padded_size
        from .render import palette_entry
        if ids is not None:
            ids = [int(i) for i in ids]
            if not 1 <= len(ids) <= A.MAX_PLANES:
                raise ValueError(f"ids: 1 .. {A.MAX_PLANES} track ids")
        n_planes = 1 if ids is None else len(ids)
        lut = None if ids is None else A.constant_lut([palette_entry(i) for i in ids])
        want = None if ids is None else torch.as_tensor(ids, dtype=torch.long).to(self.device)
        n_det = self.core.n_det_queries
        tap = A.AttentionTap(self.model)
        n_layers = len(tap.decoder.layers)
        layers = list(range(n_layers)) if layers is None else [int(lid) for lid in layers]
        if not layers or any(not 0 <= lid < n_layers for lid in layers):
            raise ValueError(f"layers: decoder layers 0 .. {n_layers - 1}")
        heat = peak = None
        with torch.no_grad():
            tap.__enter__()
        self.attention_tap = tap
        try:
            for idx, cur, nxt in self._frames(source, bgr, on_device=True):
                ids_before = self.tracks[0].ids
                result = self.step_raw(cur, nxt, bgr=bgr)
                ori_h, ori_w = int(cur.shape[0]), int(cur.shape[1])
                th, tw = target_size(ori_h, ori_w, *self.raw_size)
                Hp, Wp = padded_size(th, tw)
                hc, wc = -(-ori_h // writer.cell), -(-ori_w // writer.cell)
                rows, planes = A.frame_rows(ids_before, self.tracker.last_newborn_rows,
                                            self.tracker.last_newborn_first_id, n_det, want)
                if heat is not None and tuple(heat.shape) != (n_planes, hc, wc):
                    heat = peak = None
                heat, peak = A.tap_heat(tap, layers, rows, planes, n_planes, hc, wc,
                                        A.heat_scale(Wp, ori_w, tw, writer.cell), A.heat_scale(Hp, ori_h, th, writer.cell),
                                        writer.stamp, heat=heat, peak=peak)
                writer.add_attention(idx, cur, result, heat, peak, lut, bgr=bgr)
                yield idx, result
        finally:
            tap.__exit__(None, None, None)
            self.attention_tap = None

    def track_logged(self, source, log, *, bgr: bool = False) -> int:
        """``track`` / ``track_jpeg`` (``source`` as for ``track_annotated``) with the reportable rows of every frame
        appended to ``log`` (results.ResultLog) on the device instead of being brought to the host: one launch per frame
        in place of ``_report``'s packed copy, event wait and host filter.  Read them once, after the sequence, with
        ``log.read()`` / ``log.mot_lines`` / ``log.bdd_frames``.  Returns the number of frames."""
        n = 0
        for idx, cur, nxt in self._frames(source, bgr):
            self._advance_raw(cur, nxt, bgr)
            t = self.tracks[0]
            log.append(t.boxes, t.scores, t.ids, t.labels, idx, int(cur.shape[0]), int(cur.shape[1]),
                       self.result_score_thresh, self.area_thresh)
            n = idx + 1
        return n

    def track_annotated_logged(self, source, writer_or_sink, log, *, bgr: bool = False, sequence: int = 0) -> int:
        """``track_logged`` with the annotated files of ``track_annotated``, and no result on the host: per frame one
        ``clip_ops.draw_table`` launch makes the overlay's table from ``self.tracks[0]`` (a bank of one stream with as
        many slots as there are tracks -- the host knows that number) and a ``render.MultiAnnotatedWriter`` draws and
        encodes behind it.  ``writer_or_sink``: such a writer (the caller closes it; its files are those of sequence
        ``sequence``), or a callable ``sink(frame_idx, data)`` behind a writer of default options made and closed here.
        Returns the number of frames."""
        from .functions.clip_ops import draw_table
        from .render import MultiAnnotatedWriter
        own = None
        if isinstance(writer_or_sink, MultiAnnotatedWriter):
            writer = writer_or_sink
        elif callable(writer_or_sink):
            writer = own = MultiAnnotatedWriter(lambda seq, idx, data: writer_or_sink(idx, data))
        else:
            raise TypeError("track_annotated_logged takes a render.MultiAnnotatedWriter or a sink(frame_idx, data)")
        sizes = {}                    # (ori_w, ori_h) -> the (1, 2) float32 array on the device
        n = 0
        try:
            for idx, cur, nxt in self._frames(source, bgr, on_device=True):
                self._advance_raw(cur, nxt, bgr)
                t = self.tracks[0]
                ori_h, ori_w = int(cur.shape[0]), int(cur.shape[1])
                log.append(t.boxes, t.scores, t.ids, t.labels, idx, ori_h, ori_w, self.result_score_thresh,
                           self.area_thresh)
                ori_wh = sizes.get((ori_w, ori_h))
                if ori_wh is None:
                    host = torch.tensor([[ori_w, ori_h]], dtype=torch.float32)
                    host = host.pin_memory() if self.device.type == "cuda" else host
                    ori_wh = sizes[(ori_w, ori_h)] = host.to(self.device, non_blocking=True)
                table = draw_table(t.boxes[None], t.scores[None], t.ids.long()[None], ori_wh, self.result_score_thresh,
                                   self.area_thresh, bgr=bgr, font_scale=writer.font_scale)
                writer.add_step([(sequence, idx)], [cur], table, bgr=bgr)
                n = idx + 1
        finally:
            if own is not None:
                own.close()
        return n

    def mot_lines(self, frame_idx: int, tracks: TrackInstances) -> List[str]:
        return mot_lines(self.dataset_name, frame_idx, tracks)

    bdd_frame_result = staticmethod(bdd_frame_result)
