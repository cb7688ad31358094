"""Annotated output: the tracks of a frame drawn into it (boxes, translucent fill, id labels), and ``AnnotatedWriter``,
which draws, encodes (data/jpeg_write.py) and writes a JPEG per frame behind the tracker.

    out = draw_tracks(frame_u8, result.ids, result.boxes)            # or draw_tracks(frame_u8, result)
    with AnnotatedWriter("out/", quality=90) as writer:
        for idx, result in tracker.track_annotated(frames, writer): ...
    with MultiAnnotatedWriter("out/", names=["a", "b"]) as writer:   # no result on the host: the table is made on the
        multi_tracker.track_many_annotated_logged(sources, writer, log)  # device (functions/clip_ops.py: draw_table)

The drawing is ONE definition in integers with two statements that agree to the bit: ``draw_tracks_host`` below in
numpy (what a CPU tensor takes) and the kernel of csrc/track_draw.hip (what a CUDA tensor takes, one launch on the
current stream).  No floating point reaches the device: ``track_table`` turns every box into an int32 rectangle with
``floor(v + 0.5)`` in float32, inclusive corners, and the whole frame's tracks travel as one small int32 table.

  colour   ``PALETTE[id % 64]``; ``bgr=True`` swaps the bytes to the frame's channel order.
  outline  every pixel of the rectangle that is not in the rectangle shrunk by ``thickness``, clipped to the frame,
           opaque.  x2 < x1 or y2 < y1 draws nothing, and neither does a rectangle wholly off the frame (its tab
           included); a rectangle thinner than 2 * thickness is filled.
  fill     with ``fill_alpha`` a > 0 the pixels of the shrunk rectangle become (c * a + p * (255 - a) + 127) // 255.
  label    the decimal id in the 5 x 7 digit font ``FONT``, every cell ``font_scale`` pixels square, glyphs 6 *
           font_scale apart, on a tab of the box colour one pixel larger all round: (6 n - 1) * font_scale + 2 wide,
           7 * font_scale + 2 high.  The tab sits above the box with its left edge on x1; when it would leave the
           frame at the top it starts at y1 inside the box; when it would leave the frame on the right it is shifted
           left to end at the last column.  The text is black on colours of integer luma (77 R + 150 G + 29 B) >> 8
           of at least 128, white otherwise.
  order    rows in table order; within a row fill, outline, tab, text; a pixel takes the last primitive covering it.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

ROW_WORDS = 16
MAX_GLYPHS = 10
COORD_MAX = 1 << 24                     # rectangle coordinates are clamped to +-2^24 (exact in float32)

# 5 x 7 digits: 7 rows per glyph, bit 4 the leftmost column
FONT = (
    (0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110),
    (0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),
    (0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111),
    (0b11110, 0b00001, 0b00001, 0b01110, 0b00001, 0b00001, 0b11110),
    (0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010),
    (0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110),
    (0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110),
    (0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000),
    (0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110),
    (0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100),
)


def palette_entry(i: int) -> Tuple[int, int, int]:
    """The integer formula behind ``PALETTE``: a hue wheel of 1536 steps walked in strides of 13 / 64 of a turn (13 is
    coprime to 64: 64 different hues, neighbours far apart), full value, the floor alternating 0 / 64 / 112."""
    hue = (i * 13 % 64) * 24
    sector, f = divmod(hue, 256)
    lo = (0, 64, 112)[i % 3]
    up, down = lo + (255 - lo) * f // 255, lo + (255 - lo) * (255 - f) // 255
    return ((255, up, lo), (down, 255, lo), (lo, 255, up), (lo, down, 255), (up, lo, 255), (255, lo, down))[sector]


PALETTE = (
    (255, 0, 0), (213, 255, 64), (112, 255, 174), (0, 87, 255), (231, 64, 255), (255, 125, 112),
    (175, 255, 0), (64, 255, 165), (112, 147, 255), (248, 0, 255), (255, 99, 64), (196, 255, 112),
    (0, 255, 160), (64, 93, 255), (255, 112, 246), (255, 72, 0), (159, 255, 64), (112, 255, 215),
    (0, 15, 255), (255, 64, 225), (255, 165, 112), (103, 255, 0), (64, 255, 219), (116, 112, 255),
    (255, 0, 191), (255, 153, 64), (156, 255, 112), (0, 255, 232), (87, 64, 255), (255, 112, 205),
    (255, 144, 0), (105, 255, 64), (112, 255, 255), (56, 0, 255), (255, 64, 171), (255, 206, 112),
    (31, 255, 0), (64, 237, 255), (156, 112, 255), (255, 0, 119), (255, 207, 64), (115, 255, 112),
    (0, 207, 255), (141, 64, 255), (255, 112, 165), (255, 216, 0), (64, 255, 75), (112, 214, 255),
    (128, 0, 255), (255, 64, 117), (255, 246, 112), (0, 255, 40), (64, 183, 255), (197, 112, 255),
    (255, 0, 47), (249, 255, 64), (112, 255, 147), (0, 135, 255), (195, 64, 255), (255, 112, 124),
    (223, 255, 0), (64, 255, 129), (112, 174, 255), (200, 0, 255),
)


def _lib():
    from . import _track_draw_lib       # no substitute: a missing library is an error
    return _track_draw_lib


def _ids_boxes(ids, boxes):
    if boxes is None:                   # a TrackInstances (a reported result): its ids and xyxy pixel boxes
        ids, boxes = ids.ids, ids.boxes
    ids = torch.as_tensor(ids).detach().cpu().reshape(-1).to(torch.int64).numpy()
    boxes = torch.as_tensor(boxes).detach().cpu().to(torch.float32).reshape(-1, 4).numpy()
    if ids.shape[0] != boxes.shape[0]:
        raise ValueError(f"{ids.shape[0]} ids for {boxes.shape[0]} boxes")
    if ids.size and (ids.min() < 0 or ids.max() > 2 ** 31 - 1):
        raise ValueError("track ids are 0 .. 2**31 - 1")
    return ids, boxes


def _check_options(thickness, font_scale, fill_alpha):
    for name, v, lo, hi in (("thickness", thickness, 1, 65535), ("font_scale", font_scale, 1, 64),
                            ("fill_alpha", fill_alpha, 0, 255)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} {v!r} is not an integer in {lo} .. {hi}")


def track_table(ids, boxes_xyxy, width: int, height: int, *, bgr: bool = False, font_scale: int = 1) -> np.ndarray:
    """The (n, 16) int32 table both statements draw from (layout: include/track_draw_hip.h).  The only floating point
    of the overlay happens here: ``floor(v + 0.5)`` in float32, clamped to +-2^24."""
    ids, boxes = _ids_boxes(ids, boxes_xyxy)
    n = ids.shape[0]
    table = np.zeros((n, ROW_WORDS), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        rect = np.floor(boxes + np.float32(0.5))
    rect = np.clip(np.nan_to_num(rect, nan=0.0, posinf=COORD_MAX, neginf=-COORD_MAX), -COORD_MAX, COORD_MAX)
    table[:, 0:4] = rect.astype(np.int32)
    s = int(font_scale)
    for i in range(n):
        r, g, b = PALETTE[int(ids[i]) % 64]
        text = 0 if (77 * r + 150 * g + 29 * b) >> 8 >= 128 else 0xFFFFFF
        table[i, 4] = (b | g << 8 | r << 16) if bgr else (r | g << 8 | b << 16)
        digits = [int(ch) for ch in str(int(ids[i]))]
        x1, y1 = int(table[i, 0]), int(table[i, 1])
        tab_w, tab_h = (6 * len(digits) - 1) * s + 2, 7 * s + 2
        ty1 = y1 - tab_h if y1 - tab_h >= 0 else y1
        tx1 = min(x1, width - tab_w)
        table[i, 5:9] = (tx1, ty1, tx1 + tab_w - 1, ty1 + tab_h - 1)
        table[i, 9] = text
        table[i, 10] = len(digits)
        word = sum(d << (4 * k) for k, d in enumerate(digits[:8]))
        table[i, 11] = word - (1 << 32) if word >= 1 << 31 else word        # (the bit pattern, as int32)
        table[i, 12] = sum(d << (4 * k) for k, d in enumerate(digits[8:]))
    return table


def _unpack(word: int) -> np.ndarray:
    return np.array([word & 255, (word >> 8) & 255, (word >> 16) & 255], dtype=np.uint8)


def draw_table_host(frame: np.ndarray, table: np.ndarray, thickness: int = 2, font_scale: int = 1,
                    fill_alpha: int = 0) -> None:
    """The definition: draws ``table`` into the (H, W, 3) uint8 numpy ``frame`` in place."""
    H, W = frame.shape[:2]
    t, s, a = int(thickness), int(font_scale), int(fill_alpha)

    def clip(x1, y1, x2, y2):
        return max(x1, 0), max(y1, 0), min(x2, W - 1), min(y2, H - 1)

    for row in table.tolist():
        x1, y1, x2, y2 = row[0:4]
        if x2 < x1 or y2 < y1 or x2 < 0 or y2 < 0 or x1 >= W or y1 >= H:
            continue
        colour, text = _unpack(row[4]), _unpack(row[9])
        ix1, iy1, ix2, iy2 = clip(x1 + t, y1 + t, x2 - t, y2 - t)
        has_inner = x1 + t <= x2 - t and y1 + t <= y2 - t and ix1 <= ix2 and iy1 <= iy2
        cx1, cy1, cx2, cy2 = clip(x1, y1, x2, y2)
        if cx1 <= cx2 and cy1 <= cy2:
            inner = None
            if has_inner:
                inner = frame[iy1:iy2 + 1, ix1:ix2 + 1].astype(np.int32)
                if a > 0:
                    inner = (colour.astype(np.int32) * a + inner * (255 - a) + 127) // 255
            frame[cy1:cy2 + 1, cx1:cx2 + 1] = colour
            if has_inner:
                frame[iy1:iy2 + 1, ix1:ix2 + 1] = inner.astype(np.uint8)
        bx1, by1, bx2, by2 = row[5:9]
        tx1, ty1, tx2, ty2 = clip(bx1, by1, bx2, by2)
        if tx1 <= tx2 and ty1 <= ty2:
            frame[ty1:ty2 + 1, tx1:tx2 + 1] = colour
        for k in range(row[10]):
            g = (row[11] >> (4 * k)) & 15 if k < 8 else (row[12] >> (4 * (k - 8))) & 15
            for gr in range(7):
                for gc in range(5):
                    if (FONT[g][gr] >> (4 - gc)) & 1:
                        px, py = bx1 + 1 + (6 * k + gc) * s, by1 + 1 + gr * s
                        qx1, qy1, qx2, qy2 = (max(px, tx1), max(py, ty1), min(px + s - 1, tx2), min(py + s - 1, ty2))
                        if qx1 <= qx2 and qy1 <= qy2:
                            frame[qy1:qy2 + 1, qx1:qx2 + 1] = text


def draw_tracks_host(frame_u8, ids, boxes_xyxy=None, labels=None, *, bgr: bool = False, thickness: int = 2,
                     font_scale: int = 1, fill_alpha: int = 0, out=None):
    """``draw_tracks`` for a CPU tensor or a numpy array, in numpy: the statement that is the definition.  Returns
    the same kind it was given."""
    _check_options(thickness, font_scale, fill_alpha)
    is_np = isinstance(frame_u8, np.ndarray)
    src = frame_u8 if is_np else frame_u8.numpy()
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("a frame is (H, W, 3) uint8")
    table = track_table(ids, boxes_xyxy, src.shape[1], src.shape[0], bgr=bgr, font_scale=font_scale)
    if out is None:
        dst = src.copy()
    else:
        dst = out if isinstance(out, np.ndarray) else out.numpy()
        if dst.shape != src.shape or dst.dtype != np.uint8:
            raise ValueError("out must have the frame's shape and dtype")
        if dst is not src and not np.shares_memory(dst, src):
            dst[...] = src
    draw_table_host(dst, table, thickness, font_scale, fill_alpha)
    if out is not None:
        return out
    return dst if is_np else torch.from_numpy(dst)


# ------------------------------------------------------------------------------------ the device statement
class _Tables:
    """Pinned int32 buffers the table is written into and uploaded from, each with the event of its last copy: a
    buffer is written again only after that copy has run."""

    def __init__(self, slots: int):
        self.entries = [None] * slots
        self.i = 0

    def take(self, words: int):
        slot, self.i = self.i, (self.i + 1) % len(self.entries)
        entry = self.entries[slot]
        if entry is None or entry[0].numel() < words:
            entry = [torch.empty(max(words, 64 * ROW_WORDS), dtype=torch.int32, pin_memory=True), None]
            self.entries[slot] = entry
        elif entry[1] is not None:
            entry[1].synchronize()
        return entry[0], slot


_TABLES = _Tables(4)


def _check_device_frame(t: torch.Tensor, name: str) -> None:
    H, W, _ = t.shape
    ok = t.dtype == torch.uint8 and t.stride(2) == 1 and (W == 1 or t.stride(1) == 3)
    ok = ok and (H == 1 or t.stride(0) >= 3 * W)
    if not ok:
        raise ValueError(f"{name} must be uint8 (H, W, 3) with unit channel stride, pixel stride 3 and rows that do "
                         "not overlap (rows may be pitched)")


def draw_table_device(frame: torch.Tensor, table: np.ndarray, thickness: int = 2, font_scale: int = 1,
                      fill_alpha: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One upload of ``table`` and one launch on the current stream of ``frame``'s device; nothing waits."""
    L = _lib()
    H, W, _ = frame.shape
    _check_device_frame(frame, "frame_u8")
    device = frame.device
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
        elif not torch.is_tensor(out) or tuple(out.shape) != (H, W, 3) or out.device != device:
            raise ValueError(f"out must be a (H, W, 3) uint8 tensor on {device}")
        else:
            _check_device_frame(out, "out")
        n = int(table.shape[0])
        stream = torch.cuda.current_stream(device)
        dev_table = None
        if n:
            host, slot = _TABLES.take(n * ROW_WORDS)
            host[:n * ROW_WORDS].copy_(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32).reshape(-1)))
            dev_table = torch.empty(n * ROW_WORDS, dtype=torch.int32, device=device)
            dev_table.copy_(host[:n * ROW_WORDS], non_blocking=True)
            _TABLES.entries[slot][1] = stream.record_event()
        pitch = lambda t: t.stride(0) if H > 1 else 3 * W  # noqa: E731
        L.check(L.lib.trackdraw_draw_u8(frame.data_ptr(), pitch(frame), out.data_ptr(), pitch(out), W, H,
                                        dev_table.data_ptr() if n else None, n, int(thickness), int(font_scale),
                                        int(fill_alpha), stream.cuda_stream), "trackdraw_draw_u8")
    return out


def draw_resident_table(frame: torch.Tensor, table: torch.Tensor, out: torch.Tensor, thickness: int = 2,
                        font_scale: int = 1, fill_alpha: int = 0) -> torch.Tensor:
    """``draw_table_device`` for a table that is already on the device (``clip_ops.draw_table``: (n, 16) int32,
    contiguous, padding rows included): one launch on the current stream, no upload."""
    L = _lib()
    H, W, _ = frame.shape
    _check_device_frame(frame, "frame_u8")
    _check_device_frame(out, "out")
    if (table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != ROW_WORDS or not table.is_contiguous()
            or table.device != frame.device or out.device != frame.device or tuple(out.shape) != (H, W, 3)):
        raise ValueError("a resident table is contiguous int32 (n, 16) on the frame's device, out has the frame's shape")
    n = int(table.shape[0])
    pitch = lambda t: t.stride(0) if H > 1 else 3 * W  # noqa: E731
    with torch.cuda.device(frame.device):
        L.check(L.lib.trackdraw_draw_u8(frame.data_ptr(), pitch(frame), out.data_ptr(), pitch(out), W, H,
                                        table.data_ptr() if n else None, n, int(thickness), int(font_scale),
                                        int(fill_alpha), torch.cuda.current_stream(frame.device).cuda_stream),
                "trackdraw_draw_u8")
    return out


def draw_tracks(frame_u8, ids, boxes_xyxy=None, labels=None, *, bgr: bool = False, thickness: int = 2,
                font_scale: int = 1, fill_alpha: int = 0, out=None):
    """The tracks of a frame drawn into it.  ``frame_u8``: (H, W, 3) uint8, torch on CPU or GPU (rows may be pitched);
    ``ids`` / ``boxes_xyxy``: the fields of a reported ``TrackInstances`` (``result.ids``, ``result.boxes``: xyxy in
    pixels), or ``draw_tracks(frame, result)``.  ``labels`` is accepted so that a result's fields pass straight
    through; the label text is the id.  Returns a new frame, or writes ``out`` (``out=frame_u8`` draws in place; any
    other ``out`` must not overlap the frame).  A CPU tensor takes ``draw_tracks_host``; a CUDA tensor takes one
    kernel launch on the current stream: no allocation beyond the output and the table, no synchronisation."""
    if labels is not None and boxes_xyxy is not None and len(labels) != len(torch.as_tensor(boxes_xyxy).reshape(-1, 4)):
        raise ValueError("labels and boxes differ in length")
    if not torch.is_tensor(frame_u8) or not frame_u8.is_cuda:
        return draw_tracks_host(frame_u8, ids, boxes_xyxy, labels, bgr=bgr, thickness=thickness,
                                font_scale=font_scale, fill_alpha=fill_alpha, out=out)
    _check_options(thickness, font_scale, fill_alpha)
    if frame_u8.dim() != 3 or frame_u8.shape[2] != 3:
        raise ValueError("a frame is (H, W, 3) uint8")
    table = track_table(ids, boxes_xyxy, frame_u8.shape[1], frame_u8.shape[0], bgr=bgr, font_scale=font_scale)
    return draw_table_device(frame_u8, table, thickness, font_scale, fill_alpha, out)


# ------------------------------------------------------------------------------------ the pipeline
class AnnotatedWriter:
    """An annotated JPEG per frame, behind the tracker.

    ``add(frame_idx, frame_u8, result)`` queues, on a side stream of its own behind whatever produced the frame on
    the current stream, the draw launch and the two encode launches and a non-blocking download of the coefficients
    into one of three rotating pinned buffers (a buffer is written again only after its copy's event AND after the
    worker is through with it); one worker thread then waits for that event, Huffman-encodes (the interpreter lock
    is released for the call) and hands the file to the sink, a frame behind.  Nothing in ``add`` waits for the GPU.

    ``out``: a directory (created; files are ``name.format(frame_idx)``) or a callable ``sink(frame_idx, data)``.
    ``draw_options``: ``bgr``, ``thickness``, ``font_scale``, ``fill_alpha`` of ``draw_tracks``; ``bgr`` is also the
    channel order the encoder reads.  A CPU frame is drawn and encoded by the host statements on the worker thread.
    ``close()`` drains the queue and re-raises the worker's first error; it is idempotent."""

    SLOTS = 3

    def __init__(self, out, quality: int = 75, subsampling: str = "4:2:0", name: str = "{:08d}.jpg", **draw_options):
        import os
        from concurrent.futures import ThreadPoolExecutor
        from .data import jpeg_write as JW
        unknown = set(draw_options) - {"bgr", "thickness", "font_scale", "fill_alpha"}
        if unknown:
            raise TypeError(f"unknown draw options {sorted(unknown)}")
        JW.quant_tables(quality), JW._hmax(subsampling)
        _check_options(draw_options.get("thickness", 2), draw_options.get("font_scale", 1),
                       draw_options.get("fill_alpha", 0))
        self.quality, self.subsampling, self.name = quality, subsampling, name
        self.bgr = bool(draw_options.pop("bgr", False))
        self.draw_options = draw_options
        if callable(out):
            self._sink = out
        else:
            os.makedirs(out, exist_ok=True)
            self._sink = lambda idx, data, d=os.fspath(out): self._write(os.path.join(d, self.name.format(idx)), data)
        self.paths = []                 # files written, in order (directory sinks)
        self._pool = ThreadPoolExecutor(max_workers=1)
        self._jobs = []
        self._slots = [None] * self.SLOTS               # per pinned buffer: [tensor, event, job]
        self._i = 0
        self._stream = None
        self._geometry = None           # (H, W, device) the device buffers below were made for
        self._drawn = self._coef = self._planes = None
        self._error = None
        self._closed = False

    def _write(self, path: str, data: bytes) -> None:
        with open(path, "wb") as f:
            f.write(data)
        self.paths.append(path)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                           # an error is already on its way: drain, but do not replace it
            try:
                self.close()
            except Exception:
                pass
        return False

    def _run(self, fn, *args) -> None:
        if self._error is not None:     # after the first error nothing more is written
            return
        try:
            fn(*args)
        except BaseException as e:      # noqa: B902  (kept for close())
            self._error = e

    def _take(self, words: int):
        slot, self._i = self._i, (self._i + 1) % self.SLOTS
        entry = self._slots[slot]
        if entry is not None and entry[2] is not None:
            entry[2].result()           # the worker is through with this buffer (three frames ago: long done)
        if entry is None or entry[0].numel() < words:
            entry = [torch.empty(words, dtype=torch.int16, pin_memory=True), None, None]
            self._slots[slot] = entry
        elif entry[1] is not None:
            entry[1].synchronize()
        return entry

    def add(self, frame_idx: int, frame_u8, result, *, bgr: Optional[bool] = None) -> None:
        if self._closed:
            raise RuntimeError("add() on a closed AnnotatedWriter")
        from .data import jpeg_write as JW
        from .data.jpeg import QT_WORDS, JpegCoefficients
        bgr = self.bgr if bgr is None else bool(bgr)
        ids, boxes = _ids_boxes(result, None) if not isinstance(result, (tuple, list)) else _ids_boxes(*result)
        if not torch.is_tensor(frame_u8):
            frame_u8 = torch.from_numpy(frame_u8)
        if not frame_u8.is_cuda:
            def on_host(frame=frame_u8.clone()):
                drawn = draw_tracks_host(frame, ids, boxes, bgr=bgr, out=frame, **self.draw_options)
                self._sink(frame_idx, JW.encode_jpeg(drawn, self.quality, self.subsampling, bgr))
            self._jobs.append(self._pool.submit(self._run, on_host))
            return
        if frame_u8.dim() != 3 or frame_u8.shape[2] != 3 or frame_u8.dtype != torch.uint8:
            raise ValueError("a frame is (H, W, 3) uint8")
        H, W = int(frame_u8.shape[0]), int(frame_u8.shape[1])
        device = frame_u8.device
        info = JW.frame_info(H, W, self.subsampling)
        n = info.coef_count
        table = track_table(ids, boxes, W, H, bgr=bgr, font_scale=self.draw_options.get("font_scale", 1))
        entry = self._take(n + QT_WORDS)
        host = entry[0][:n + QT_WORDS]
        host[n:] = torch.from_numpy(JW.quant_tables(self.quality).astype(np.int16).reshape(-1))
        with torch.cuda.device(device):
            if self._stream is None or self._stream.device != device:
                self._stream = torch.cuda.Stream(device)
            side = self._stream
            side.wait_stream(torch.cuda.current_stream(device))         # behind the frame's producer
            with torch.cuda.stream(side):
                if self._geometry != (H, W, device):                   # (all used on this one stream, in order)
                    self._drawn = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
                    self._coef = torch.empty((1, n), dtype=torch.int16, device=device)
                    self._planes = torch.empty(n, dtype=torch.uint8, device=device)
                    self._geometry = (H, W, device)
                draw_table_device(frame_u8, table, self.draw_options.get("thickness", 2),
                                  self.draw_options.get("font_scale", 1), self.draw_options.get("fill_alpha", 0),
                                  out=self._drawn)
                JW.forward_coefficients_device(self._drawn[None], self.quality, self.subsampling, bgr, out=self._coef,
                                               planes=self._planes)
                host[:n].copy_(self._coef[0], non_blocking=True)
                event = side.record_event()
            frame_u8.record_stream(side)
        entry[1] = event

        def on_worker():
            event.synchronize()
            self._sink(frame_idx, JW.huffman_encode(JpegCoefficients(info, host)))

        entry[2] = self._pool.submit(self._run, on_worker)
        self._jobs.append(entry[2])

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        for job in self._jobs:
            job.result()
        self._jobs = []
        self._pool.shutdown(wait=True)
        if self._error is not None:
            raise self._error


class MultiAnnotatedWriter(AnnotatedWriter):
    """``AnnotatedWriter`` for sequences tracked side by side, fed from the device: a step's frames and the draw tables
    ``clip_ops.draw_table`` made from the tracks where they live -- no result reaches the host.

    ``add_step(meta, frames, tables)``: ``meta[b] = (sequence, frame_idx)`` of stream b; ``frames`` one (B, H, W, 3)
    uint8 tensor or a list of B (H, W, 3) tensors; ``tables`` int32 (B, cap, 16).  On the writer's side stream, behind
    the current one: a draw launch per stream into one (n, H, W, 3) buffer per frame size (frames of different sizes in
    one step are encoded per size: ``encode_jpegs``' rule), one batched encode and one non-blocking download per size
    into one of three rotating pinned buffers (``AnnotatedWriter``'s rule: written again only after its copy's event and
    its worker job).  One worker then waits for the event, runs the Huffman stage of the step's frames on
    ``min(threads, frames, 16)`` host threads (never sized by the CPU count) and hands every file to the sink.  Nothing
    in ``add_step`` waits for the GPU.  It returns the event behind the draw launches (None on the CPU): whoever rewrites
    ``tables`` makes its stream wait for it first.  CPU frames (with CPU tables) are drawn and encoded by the host
    statements on the worker.

    ``out``: a directory -- files are ``<out>/<names[sequence]>/<name.format(frame_idx)>``, ``names`` defaulting to the
    sequence indices -- or a callable ``sink(sequence, frame_idx, data)``.  ``close()`` drains and re-raises the first
    worker error; it is idempotent, and the writer is a context manager."""

    def __init__(self, out, names=None, quality: int = 75, subsampling: str = "4:2:0", name: str = "{:08d}.jpg",
                 threads: int = 4, **draw_options):
        import os
        from concurrent.futures import ThreadPoolExecutor
        from .data import jpeg_write as JW
        unknown = set(draw_options) - {"bgr", "thickness", "font_scale", "fill_alpha"}
        if unknown:
            raise TypeError(f"unknown draw options {sorted(unknown)}")
        JW.quant_tables(quality), JW._hmax(subsampling)
        if int(threads) < 1:
            raise ValueError("threads must be at least 1")
        self.bgr = bool(draw_options.pop("bgr", False))
        self.thickness, self.font_scale = draw_options.get("thickness", 2), draw_options.get("font_scale", 1)
        self.fill_alpha = draw_options.get("fill_alpha", 0)
        _check_options(self.thickness, self.font_scale, self.fill_alpha)
        self.quality, self.subsampling, self.name, self.threads = quality, subsampling, name, int(threads)
        self.draw_options = draw_options
        self.names = None if names is None else [str(n) for n in names]
        if callable(out):
            self._sink = out
        else:
            self._out, self._made = os.fspath(out), set()
            os.makedirs(self._out, exist_ok=True)
            self._sink = self._to_directory
        self.paths = []                 # files written, in order (directory sinks)
        self._pool = ThreadPoolExecutor(max_workers=1)
        self._jobs = []
        self._slots = [None] * self.SLOTS               # per pinned buffer: [tensor, event, job]
        self._i = 0
        self._stream = None
        self._buffers = {}              # (H, W, n, device) -> (drawn, coef, packed, planes), used on the side stream
        self._error = None
        self._closed = False

    def _to_directory(self, seq: int, frame_idx: int, data: bytes) -> None:
        import os
        d = os.path.join(self._out, str(seq) if self.names is None else self.names[seq])
        if d not in self._made:
            os.makedirs(d, exist_ok=True)
            self._made.add(d)
        self._write(os.path.join(d, self.name.format(frame_idx)), data)

    def add(self, *args, **kwargs):
        raise TypeError("a MultiAnnotatedWriter takes whole steps: add_step(meta, frames, tables)")

    def _step_on_host(self, meta, frames, tables, bgr: bool) -> None:
        from .data import jpeg_write as JW
        if tables.is_cuda:
            raise ValueError("CPU frames are drawn from a CPU table")
        frames = [f.clone() for f in frames]
        tables = tables.clone().numpy()

        def on_host():
            for (seq, idx), frame, table in zip(meta, frames, tables):
                draw_table_host(frame.numpy(), table, self.thickness, self.font_scale, self.fill_alpha)
                self._sink(seq, idx, JW.encode_jpeg(frame, self.quality, self.subsampling, bgr))

        self._jobs.append(self._pool.submit(self._run, on_host))

    def add_step(self, meta, frames, tables, *, bgr: Optional[bool] = None):
        if self._closed:
            raise RuntimeError("add_step() on a closed MultiAnnotatedWriter")
        from .data import jpeg_write as JW
        from .data.jpeg import QT_WORDS
        bgr = self.bgr if bgr is None else bool(bgr)
        meta = [(int(seq), int(idx)) for seq, idx in meta]
        whole = frames if torch.is_tensor(frames) else None
        frames = [f if torch.is_tensor(f) else torch.from_numpy(f) for f in frames]
        B = len(meta)
        if len(frames) != B or tables.dim() != 3 or tables.shape[0] != B or tables.shape[2] != ROW_WORDS \
                or tables.dtype != torch.int32:
            raise ValueError(f"a step is {B} (sequence, frame) pairs, {B} frames and an int32 ({B}, cap, 16) table")
        for f in frames:
            if f.dim() != 3 or f.shape[2] != 3 or f.dtype != torch.uint8:
                raise ValueError("a frame is (H, W, 3) uint8")
        if B == 0:
            return None
        if not any(f.is_cuda for f in frames):
            self._step_on_host(meta, frames, tables, bgr)
            return None
        device = tables.device
        if not all(f.device == device for f in frames) or not tables.is_contiguous():
            raise ValueError("the frames of a step and its contiguous table are on one device")
        groups = {}
        for b, f in enumerate(frames):
            groups.setdefault((int(f.shape[0]), int(f.shape[1])), []).append(b)
        infos = {size: JW.frame_info(size[0], size[1], self.subsampling) for size in groups}
        words = sum(len(idx) * (infos[size].coef_count + QT_WORDS) for size, idx in groups.items())
        entry = self._take(words)
        jobs, at = [], 0
        with torch.cuda.device(device):
            if self._stream is None or self._stream.device != device:
                self._stream = torch.cuda.Stream(device)
            side = self._stream
            side.wait_stream(torch.cuda.current_stream(device))         # behind the frames' and the table's producers
            with torch.cuda.stream(side):
                for (H, W), idx in groups.items():
                    info, n = infos[(H, W)], len(idx)
                    row = info.coef_count + QT_WORDS
                    key = (H, W, n, device)
                    if key not in self._buffers:                        # (all used on this one stream, in order)
                        packed = torch.empty((n, row), dtype=torch.int16, device=device)
                        qt = torch.from_numpy(JW.quant_tables(self.quality).astype(np.int16).reshape(-1))
                        packed[:, info.coef_count:] = qt.to(device)
                        self._buffers[key] = (torch.empty((n, H, W, 3), dtype=torch.uint8, device=device),
                                              torch.empty((n, info.coef_count), dtype=torch.int16, device=device),
                                              packed, torch.empty(n * info.coef_count, dtype=torch.uint8, device=device))
                    drawn, coef, packed, planes = self._buffers[key]
                    for k, b in enumerate(idx):
                        draw_resident_table(frames[b], tables[b], drawn[k], self.thickness, self.font_scale,
                                            self.fill_alpha)
                    jobs.append((idx, info, at))
                    at += n * row
                read = side.record_event()                              # the table may be rewritten behind this
                for (idx, info, start), (H, W) in zip(jobs, groups):
                    n = len(idx)
                    drawn, coef, packed, planes = self._buffers[(H, W, n, device)]
                    JW.forward_coefficients_device(drawn, self.quality, self.subsampling, bgr, out=coef, planes=planes)
                    packed[:, :info.coef_count].copy_(coef)
                    entry[0][start:start + packed.numel()].copy_(packed.reshape(-1), non_blocking=True)
                event = side.record_event()
            for f in ([whole] if whole is not None else frames):
                f.record_stream(side)
            tables.record_stream(side)
        entry[1] = event
        host = entry[0]

        def on_worker():
            event.synchronize()
            for idx, info, start in jobs:
                row = info.coef_count + QT_WORDS
                rows = host[start:start + len(idx) * row].view(len(idx), row)
                for b, data in zip(idx, JW._huffman_batch(rows, info, min(self.threads, len(idx), 16))):
                    self._sink(meta[b][0], meta[b][1], data)

        entry[2] = self._pool.submit(self._run, on_worker)
        self._jobs.append(entry[2])
        return read
