"""JPEG files -> uint8 frames (H x W x 3), the step in front of ``SequenceTracker.track`` and ``augment_clip``.

Two stages ("JPEG decode"):

  * host: marker parsing and Huffman decoding (csrc/jpeg_entropy_core.h through libjpeg_ops_hip.so; plain C++, no
    device, the interpreter lock is released for the call) into int16 coefficient blocks, written straight into
    pinned memory;
  * device: dequantisation, 8x8 IDCT, chroma upsampling, YCbCr -> RGB and interleaving, two launches of
    csrc/jpeg_ops.hip on the current stream.  For 4:2:0 the upload is 3 bytes per pixel, what the RGB frame was.

The arithmetic is ONE definition in 32-bit integers -- libjpeg-turbo's default decode path (accurate integer IDCT,
"fancy" upsampling, 16-bit colour tables) -- with two statements that agree to the bit: the kernels, and
``decode_coefficients_host`` below in numpy.  Both equal Pillow's ``Image.open(...).convert("RGB")`` byte for byte.

    frame = decode_jpeg("000001.jpg", "cuda", bgr=True)            # (H, W, 3) uint8, cv2.imread's channel order
    clip = decode_jpegs(paths, "cuda")                             # (T, H, W, 3), ready for augment_clip
    for idx, result in tracker.track_jpeg(paths): ...              # inference.SequenceTracker

Streams the host stage does not read (progressive, arithmetic, 12-bit, CMYK, ...) raise ``UnsupportedJpeg``, or with
``fallback=True`` are decoded by Pillow on the host when it is installed; corrupt data always raises ``CorruptJpeg``.
"""
from __future__ import annotations

import ctypes
import dataclasses
import io
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

QT_WORDS = 192                          # uint16[3][64] behind the coefficients of a frame


class UnsupportedJpeg(ValueError):
    """A valid stream of a kind the decoder does not read."""


class CorruptJpeg(ValueError):
    """Data that is not a decodable JPEG stream (truncated, malformed, codes outside the tables)."""


@dataclasses.dataclass(frozen=True)
class JpegInfo:
    width: int
    height: int
    ncomp: int
    hmax: int
    vmax: int
    restart_interval: int
    mcus_x: int
    mcus_y: int
    h: Tuple[int, ...]
    v: Tuple[int, ...]
    blocks_w: Tuple[int, ...]
    blocks_h: Tuple[int, ...]
    coef_offset: Tuple[int, ...]
    coef_count: int

    @property
    def geometry(self):
        """What two frames must share to go through one device stage."""
        return self.width, self.height, self.ncomp, self.hmax, self.vmax

    @property
    def sampling(self) -> str:
        return "gray" if self.ncomp == 1 else {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}[(self.hmax, self.vmax)]

    @property
    def chroma_size(self) -> Tuple[int, int]:
        """(rows, columns) of the true chroma plane: ceil(H / vmax), ceil(W / hmax)."""
        return -(-self.height // self.vmax), -(-self.width // self.hmax)


@dataclasses.dataclass
class JpegCoefficients:
    """The host stage's output.  ``flat``: int16, the frame's ``coef_count`` coefficients followed by the 192 words
    of the quantisation tables (uint16 bit patterns): one buffer, one upload.  ``components[c]``: (blocks_h, blocks_w,
    8, 8) int16 view of it, natural order; ``qt``: (ncomp, 64) int32 copy of the tables, natural order."""
    info: JpegInfo
    flat: torch.Tensor

    @property
    def components(self) -> List[torch.Tensor]:
        f = self.info
        return [self.flat[f.coef_offset[c]:f.coef_offset[c] + f.blocks_h[c] * f.blocks_w[c] * 64]
                .view(f.blocks_h[c], f.blocks_w[c], 8, 8) for c in range(f.ncomp)]

    @property
    def qt(self) -> torch.Tensor:
        words = self.flat[self.info.coef_count:self.info.coef_count + QT_WORDS].to(torch.int32) & 0xFFFF
        return words.view(3, 64)[:self.info.ncomp]


def _lib():
    from .. import _jpeg_lib            # no substitute: a missing library is an error
    return _jpeg_lib


def _as_bytes(data) -> np.ndarray:
    if isinstance(data, (str, os.PathLike)):
        with open(data, "rb") as f:
            data = f.read()
    if torch.is_tensor(data):
        data = data.numpy()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    if a.dtype != np.uint8 or a.ndim != 1:
        raise TypeError("a JPEG stream is bytes, a path or a 1-D uint8 array")
    return np.ascontiguousarray(a)


def _raise(rc: int, message: str):
    L = _lib()
    if rc >= L.UNSUPPORTED:
        raise UnsupportedJpeg(message)
    if rc == 1:
        raise ValueError(message)
    raise CorruptJpeg(message)


def _info(c) -> JpegInfo:
    n = c.ncomp
    return JpegInfo(c.width, c.height, n, c.hmax, c.vmax, c.restart_interval, c.mcus_x, c.mcus_y, tuple(c.h[:n]),
                    tuple(c.v[:n]), tuple(c.blocks_w[:n]), tuple(c.blocks_h[:n]), tuple(c.coef_offset[:n]),
                    c.coef_count)


def _cinfo(info: JpegInfo):
    L = _lib()
    c = L.Info()
    for k in ("width", "height", "ncomp", "hmax", "vmax", "restart_interval", "mcus_x", "mcus_y", "coef_count"):
        setattr(c, k, getattr(info, k))
    for k in ("h", "v", "blocks_w", "blocks_h", "coef_offset"):
        for i, x in enumerate(getattr(info, k)):
            getattr(c, k)[i] = x
    off = info.coef_count
    for i in range(info.ncomp, 3):
        c.coef_offset[i] = off
    return c


def parse_jpeg(data) -> JpegInfo:
    """Sizes only (reads the marker segments up to the scan)."""
    L = _lib()
    a = _as_bytes(data)
    c = L.Info()
    rc = L.lib.jpegops_parse_header(a.ctypes.data, a.size, ctypes.byref(c))
    if rc:
        _raise(rc, L.lib.jpegops_last_error().decode())
    return _info(c)


def _frame_words(info: JpegInfo) -> int:
    return info.coef_count + QT_WORDS


def entropy_decode(data, pinned: Optional[torch.Tensor] = None) -> JpegCoefficients:
    """The host stage.  ``pinned``: an int16 tensor of at least ``parse_jpeg(data).coef_count + 192`` elements to write
    into (pinned memory a later upload reads from); a fresh pageable tensor otherwise."""
    L = _lib()
    a = _as_bytes(data)
    info = parse_jpeg(a)
    n = _frame_words(info)
    if pinned is None:
        flat = torch.empty(n, dtype=torch.int16)
    else:
        if pinned.dtype != torch.int16 or pinned.dim() != 1 or pinned.numel() < n or not pinned.is_contiguous() \
                or pinned.device.type != "cpu":
            raise ValueError(f"pinned must be a contiguous 1-D int16 CPU tensor of at least {n} elements")
        flat = pinned[:n]
    c = L.Info()
    rc = L.lib.jpegops_entropy_decode(a.ctypes.data, a.size, ctypes.byref(c), flat.data_ptr(), info.coef_count * 2,
                                      flat.data_ptr() + info.coef_count * 2)
    if rc:
        _raise(rc, L.lib.jpegops_last_error().decode())
    return JpegCoefficients(_info(c), flat)


# ------------------------------------------------------------------------------------ the definition, in numpy
C_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _idct_1d(x, shift: int):
    """One pass of the LL&M IDCT over axis -1 of int32 ``x`` (8 values), descaled by ``shift`` with rounding.  int32
    arithmetic throughout (numpy wraps silently, as the kernel does)."""
    i32 = np.int32
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., k] for k in range(8))
    z1 = (x2 + x6) * i32(F_0_541)
    t2 = z1 + x6 * i32(-F_1_847)
    t3 = z1 + x2 * i32(F_0_765)
    t0 = (x0 + x4) * i32(1 << C_BITS)
    t1 = (x0 - x4) * i32(1 << C_BITS)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x7, x5, x3, x1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * i32(F_1_175)
    o0, o1, o2, o3 = o0 * i32(F_0_298), o1 * i32(F_2_053), o2 * i32(F_3_072), o3 * i32(F_1_501)
    z1, z2 = z1 * i32(-F_0_899), z2 * i32(-F_2_562)
    z3, z4 = z3 * i32(-F_1_961) + z5, z4 * i32(-F_0_390) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    half = i32(1 << (shift - 1))
    out = (t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3)
    return np.stack([(v + half) >> shift for v in out], axis=-1)


def _idct_blocks(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(bh, bw, 8, 8) int16 coefficients and 64 table entries -> (bh * 8, bw * 8) uint8 samples."""
    with np.errstate(over="ignore"):
        d = coef.astype(np.int32) * q.astype(np.int32).reshape(8, 8)
        ws = _idct_1d(d.swapaxes(-1, -2), C_BITS - PASS1_BITS).swapaxes(-1, -2)        # columns first
        px = _idct_1d(ws, C_BITS + PASS1_BITS + 3) + np.int32(128)                     # then rows
    px = np.clip(px, 0, 255).astype(np.uint8)
    bh, bw = coef.shape[:2]
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample_h2v1(c: np.ndarray) -> np.ndarray:
    c = c.astype(np.int32)
    prev = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    nxt = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    even, odd = (3 * c + prev + 1) >> 2, (3 * c + nxt + 2) >> 2
    even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
    return np.stack([even, odd], axis=-1).reshape(c.shape[0], -1)


def _upsample_h2v2(c: np.ndarray) -> np.ndarray:
    c = c.astype(np.int32)
    above = np.concatenate([c[:1], c[:-1]], axis=0)
    below = np.concatenate([c[1:], c[-1:]], axis=0)
    rows = np.stack([3 * c + above, 3 * c + below], axis=1).reshape(-1, c.shape[1])    # output rows 2i, 2i + 1
    prev = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    nxt = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    even, odd = (3 * rows + prev + 8) >> 4, (3 * rows + nxt + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return np.stack([even, odd], axis=-1).reshape(rows.shape[0], -1)


def _upsample(plane: np.ndarray, info: JpegInfo) -> np.ndarray:
    """Chroma plane (padded) -> (H, W) int32 at full resolution: the triangle filter over the TRUE plane, its edge
    samples replicated; plain replication when that plane is at most 2 samples wide (libjpeg's rule)."""
    H, W = info.height, info.width
    ch, cw = info.chroma_size
    c = plane[:ch, :cw]
    if info.hmax == 1:
        return c.astype(np.int32)
    if cw <= 2:
        return np.repeat(np.repeat(c, info.vmax, axis=0), 2, axis=1)[:H, :W].astype(np.int32)
    up = _upsample_h2v1(c) if info.vmax == 1 else _upsample_h2v2(c)
    return up[:H, :W]


def decode_coefficients_host(coefs: JpegCoefficients, bgr: bool = False) -> np.ndarray:
    """The definition the kernels are held to: (H, W, 3) uint8 from the host stage's output, in numpy integers."""
    info = coefs.info
    H, W = info.height, info.width
    qt = coefs.qt.numpy()
    planes = [_idct_blocks(comp.numpy(), qt[c]) for c, comp in enumerate(coefs.components)]
    y = planes[0][:H, :W].astype(np.int32)
    if info.ncomp == 1:
        r = g = b = y
    else:
        cb = _upsample(planes[1], info) - 128
        cr = _upsample(planes[2], info) - 128
        r = y + ((91881 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    out = np.stack([b, g, r] if bgr else [r, g, b], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------ the device stage
class _Staging:
    """Pinned int16 buffers that entropy output is written into and uploaded from, each with the event of its last
    copy: a buffer is written again only after that copy has run."""

    def __init__(self, slots: int):
        self.entries = [None] * slots
        self.i = 0

    def take(self, words: int) -> Tuple[torch.Tensor, int]:
        slot, self.i = self.i, (self.i + 1) % len(self.entries)
        entry = self.entries[slot]
        if entry is None or entry[0].numel() < words:
            entry = [torch.empty(words, dtype=torch.int16, pin_memory=True), None]
            self.entries[slot] = entry
        elif entry[1] is not None:
            entry[1].synchronize()
        return entry[0], slot

    def copied(self, slot: int, event) -> None:
        self.entries[slot][1] = event


_STAGING = _Staging(2)


def _check_out(out: torch.Tensor, shape, device: torch.device) -> None:
    # (the stride of a dimension of size 1 means nothing and torch reports any value for it)
    B, H, W, _ = shape
    ok = tuple(out.shape) == tuple(shape) and out.dtype == torch.uint8 and out.device == device and out.stride(3) == 1
    ok = ok and (W == 1 or out.stride(2) == 3) and (H == 1 or out.stride(1) >= 3 * W)
    ok = ok and (B == 1 or out.stride(0) >= (out.stride(1) if H > 1 else 3 * W) * (H - 1) + 3 * W)
    if not ok:
        raise ValueError(f"out must be a uint8 tensor of shape {tuple(shape)} on {device} with unit channel stride, "
                         "pixel stride 3 and rows and frames that do not overlap")


def _device_stage(host: torch.Tensor, info: JpegInfo, B: int, device: torch.device, bgr: bool,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``host``: (B, coef_count + 192) int16, pinned.  Upload and both launches on the current stream of ``device``;
    returns (B, H, W, 3) uint8."""
    L = _lib()
    words = _frame_words(info)
    shape = (B, info.height, info.width, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    else:
        _check_out(out, shape, device)
    row_pitch = out.stride(1) if info.height > 1 else 3 * info.width
    frame_pitch = out.stride(0) if B > 1 else row_pitch * info.height
    c = _cinfo(info)
    per_frame = L.lib.jpegops_planes_bytes(ctypes.byref(c))
    with torch.cuda.device(device):
        dev = torch.empty((B, words), dtype=torch.int16, device=device)
        dev.copy_(host, non_blocking=True)
        planes = torch.empty(B * per_frame, dtype=torch.uint8, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream
        L.check(L.lib.jpegops_decode_pixels_u8(
            dev.data_ptr(), words, dev.data_ptr() + info.coef_count * 2, words, ctypes.byref(c), planes.data_ptr(),
            planes.numel(), out.data_ptr(), row_pitch, frame_pitch, B, int(bool(bgr)), stream),
            "jpegops_decode_pixels_u8")
    return out


def _pillow_decode(a: np.ndarray, bgr: bool) -> np.ndarray:
    from PIL import Image
    px = np.asarray(Image.open(io.BytesIO(a.tobytes())).convert("RGB"))
    return np.array(px[..., ::-1] if bgr else px, order="C")          # (a writable copy: torch wraps it)


def _fallback(a: np.ndarray, device: torch.device, bgr: bool, error: UnsupportedJpeg) -> torch.Tensor:
    try:
        import PIL  # noqa: F401
    except ImportError:
        raise error from None
    return torch.from_numpy(_pillow_decode(a, bgr)).to(device)


def decode_jpeg(data_or_path, device="cpu", bgr: bool = False, fallback: bool = True,
                out: Optional[torch.Tensor] = None, staging: Optional[_Staging] = None) -> torch.Tensor:
    """One stream (bytes, a 1-D uint8 array or a path) -> (H, W, 3) uint8 on ``device``, RGB (``bgr=True``: B, G, R,
    ``cv2.imread``'s order).  CUDA: entropy stage into a pinned buffer, non-blocking upload and the two kernels on the
    current stream; nothing here waits for them.  ``out``: a (H, W, 3) uint8 CUDA tensor to write into, rows may be
    pitched; bytes outside the pixels are left alone.  ``staging``: the pinned ring to use instead of the module's
    (which is for ONE thread: a second decoding thread brings its own ``_Staging``)."""
    device = torch.device(device)
    staging = _STAGING if staging is None else staging
    a = _as_bytes(data_or_path)
    try:
        info = parse_jpeg(a)
        if device.type != "cuda":
            return torch.from_numpy(decode_coefficients_host(entropy_decode(a), bgr=bgr))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        buf, slot = staging.take(_frame_words(info))
        coefs = entropy_decode(a, pinned=buf)
    except UnsupportedJpeg as e:
        if not fallback:
            raise
        px = _fallback(a, device, bgr, e)
        if out is not None:
            out.copy_(px)
            return out
        return px
    frame = _device_stage(coefs.flat[None], coefs.info, 1, device, bgr, None if out is None else out[None])[0]
    staging.copied(slot, torch.cuda.current_stream(device).record_event())
    return frame


def _entropy_batch(streams: Sequence[np.ndarray], infos: Sequence[JpegInfo], host: torch.Tensor, threads: int) -> None:
    """One library call for a clip: frame i into row i of ``host`` (T, words) on ``threads`` host threads."""
    L = _lib()
    T = len(streams)
    words = host.shape[1]
    ptrs = (ctypes.c_void_p * T)(*[s.ctypes.data for s in streams])
    sizes = (ctypes.c_size_t * T)(*[s.size for s in streams])
    cinfos = (L.Info * T)()
    base = host.data_ptr()
    coef = (ctypes.c_void_p * T)(*[base + i * words * 2 for i in range(T)])
    coef_bytes = (ctypes.c_size_t * T)(*[f.coef_count * 2 for f in infos])
    qts = (ctypes.c_void_p * T)(*[base + (i * words + f.coef_count) * 2 for i, f in enumerate(infos)])
    status = (ctypes.c_int * T)()
    errors = ctypes.create_string_buffer(T * L.ERR_LEN)
    failed = L.lib.jpegops_entropy_decode_batch(ptrs, sizes, T, cinfos, coef, coef_bytes, qts, status, errors,
                                                int(threads))
    if failed < 0:
        raise ValueError(L.lib.jpegops_last_error().decode())
    for i in range(T):
        if status[i]:
            msg = errors.raw[i * L.ERR_LEN:(i + 1) * L.ERR_LEN].split(b"\0", 1)[0].decode()
            _raise(status[i], f"frame {i}: {msg}")


def decode_jpegs(items: Sequence, device="cpu", threads: int = 4, bgr: bool = False, fallback: bool = True,
                 staging: Optional[_Staging] = None) -> Union[torch.Tensor, List[torch.Tensor]]:
    """A clip.  Frames of one geometry: one batched entropy call on ``threads`` host threads (never sized by the
    machine's CPU count), one upload, one device stage, and a (T, H, W, 3) uint8 tensor.  Mixed geometries, or a
    stream only Pillow reads: a list of (H, W, 3) tensors, frame by frame.  ``staging``: as for ``decode_jpeg``."""
    device = torch.device(device)
    staging = _STAGING if staging is None else staging
    streams = [_as_bytes(x) for x in items]
    if not streams:
        return []
    try:
        infos = [parse_jpeg(a) for a in streams]
    except UnsupportedJpeg:
        if not fallback:
            raise
        infos = None
    if infos is None or any(f.geometry != infos[0].geometry for f in infos):
        return [decode_jpeg(a, device, bgr=bgr, fallback=fallback, staging=staging) for a in streams]
    info, T = infos[0], len(streams)
    words = _frame_words(info)
    if device.type != "cuda":
        host = torch.empty((T, words), dtype=torch.int16)
        _entropy_batch(streams, infos, host, threads)
        return torch.from_numpy(np.stack([decode_coefficients_host(JpegCoefficients(info, host[i]), bgr=bgr)
                                          for i in range(T)]))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    buf, slot = staging.take(T * words)
    host = buf[:T * words].view(T, words)
    _entropy_batch(streams, infos, host, threads)
    frames = _device_stage(host, info, T, device, bgr)
    staging.copied(slot, torch.cuda.current_stream(device).record_event())
    return frames
