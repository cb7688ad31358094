"""uint8 frames (H x W x 3) -> baseline JPEG files, the mirror image of ``data/jpeg.py``.

Two stages:

  * device: RGB -> YCbCr, edge replication, 2 x 2 chroma averaging, 8x8 forward DCT and quantisation, two launches
    of csrc/jpeg_enc.hip on the current stream, into int16 coefficient blocks;
  * host: marker segments and the Huffman-coded scan (csrc/jpeg_encode_core.h through libjpeg_enc_hip.so; plain C++,
    no device, the interpreter lock is released for the call).

The arithmetic is ONE definition in 32-bit integers -- libjpeg-turbo's default compress path (16-bit colour tables,
h2v2 box downsampling with alternating bias, the accurate integer FDCT, rounding division by the table) -- with two
statements that agree to the bit: the kernels, and ``forward_coefficients_host`` below in numpy.  The bytes equal
``Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=0 | 2)`` of Pillow (libjpeg-turbo).

    data = encode_jpeg(frame, quality=90)                      # bytes; frame on CPU or GPU
    files = encode_jpegs(list_of_frames, threads=4)

Scope: 8-bit, three components, "4:4:4" and "4:2:0", quality 1 .. 100, the Annex K tables unoptimised, no restart
markers; everything else raises ``ValueError``.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from .jpeg import QT_WORDS, JpegCoefficients, JpegInfo

SAMPLINGS = {"4:4:4": 1, "4:2:0": 2}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K.1 (luma) and K.2 (chroma), natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113,
                      92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def _lib():
    from .. import _jpeg_enc_lib        # no substitute: a missing library is an error
    return _jpeg_enc_lib


def _hmax(subsampling) -> int:
    if subsampling not in SAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r} is not one of {sorted(SAMPLINGS)}")
    return SAMPLINGS[subsampling]


def quant_tables(quality: int) -> np.ndarray:
    """(3, 64) int32, natural order: luma, chroma, chroma.  libjpeg's scaling of the Annex K tables."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"quality {quality!r} is not an integer in 1 .. 100")
    s = 5000 // int(quality) if quality < 50 else 200 - 2 * int(quality)
    luma, chroma = (np.clip((b * s + 50) // 100, 1, 255).astype(np.int32) for b in (BASE_LUMA, BASE_CHROMA))
    return np.stack([luma, chroma, chroma])


def frame_info(height: int, width: int, subsampling="4:2:0") -> JpegInfo:
    """The whole-MCU block geometry the encoder gives a frame (the decoder's ``JpegInfo``)."""
    m = _hmax(subsampling)
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"a JPEG frame is 1 .. 65535 pixels wide and high, not {height} x {width}")
    mx, my = -(-width // (8 * m)), -(-height // (8 * m))
    hv = (m, 1, 1)
    bw, bh = tuple(mx * k for k in hv), tuple(my * k for k in hv)
    counts = [bw[c] * bh[c] * 64 for c in range(3)]
    return JpegInfo(width, height, 3, m, m, 0, mx, my, hv, hv, bw, bh, (0, counts[0], counts[0] + counts[1]),
                    sum(counts))


def _cinfo(info: JpegInfo):
    L = _lib()
    c = L.Info()
    L.check(L.lib.jpegenc_geometry(info.width, info.height, info.hmax, ctypes.byref(c)), "jpegenc_geometry")
    return c


# ------------------------------------------------------------------------------------ the definition, in numpy
def _fdct_1d(d, rows: bool):
    """One pass of the LL&M forward DCT (libjpeg's jfdctint.c) over axis -1 of int32 ``d`` (8 values)."""
    i32 = np.int32
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    shift = 11 if rows else 15
    half = i32(1 << (shift - 1))
    if rows:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = (t10 + t11 + i32(2)) >> 2, (t10 - t11 + i32(2)) >> 2
    z1 = (t12 + t13) * i32(4433)
    o2 = (z1 + t13 * i32(6270) + half) >> shift
    o6 = (z1 + t12 * i32(-15137) + half) >> shift
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * i32(9633)
    m4, m5, m6, m7 = t4 * i32(2446), t5 * i32(16819), t6 * i32(25172), t7 * i32(12299)
    z1, z2 = z1 * i32(-7373), z2 * i32(-20995)
    z3, z4 = z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    o7, o5 = (m4 + z1 + z3 + half) >> shift, (m5 + z2 + z4 + half) >> shift
    o3, o1 = (m6 + z2 + z3 + half) >> shift, (m7 + z1 + z4 + half) >> shift
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)


def _fdct_quant(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(bh * 8, bw * 8) samples and 64 table entries -> (bh, bw, 8, 8) int16 quantised coefficients."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.astype(np.int32).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - np.int32(128)
    ws = _fdct_1d(d, True)                                                           # rows first
    c = _fdct_1d(ws.swapaxes(-1, -2), False).swapaxes(-1, -2)                        # then columns
    dq = q.astype(np.int32).reshape(8, 8) << 3
    a = (np.abs(c) + (dq >> 1)) // dq
    return np.where(c < 0, -a, a).astype(np.int16)


def _check_frame(frame) -> None:
    if not torch.is_tensor(frame) or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError("a frame is a (H, W, 3) uint8 tensor")


def forward_coefficients_host(frame, quality: int = 75, subsampling="4:2:0", bgr: bool = False) -> JpegCoefficients:
    """The definition the kernels are held to: the quantised coefficient blocks of a (H, W, 3) uint8 frame (a CPU
    tensor or a numpy array) in numpy integers, dummy blocks filled, with their tables, in the decoder's layout."""
    if isinstance(frame, np.ndarray):
        frame = torch.from_numpy(np.ascontiguousarray(frame))
    _check_frame(frame)
    qt = quant_tables(quality)
    H, W = int(frame.shape[0]), int(frame.shape[1])
    info = frame_info(H, W, subsampling)
    px = frame.cpu().numpy().astype(np.int32)
    r, g, b = (px[..., 2], px[..., 1], px[..., 0]) if bgr else (px[..., 0], px[..., 1], px[..., 2])
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    PH, PW = info.blocks_h[0] * 8, info.blocks_w[0] * 8

    def pad(p, rows, cols):
        return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")

    if info.hmax == 1:
        blocks = [_fdct_quant(pad(p, PH, PW), qt[c]) for c, p in enumerate((y, cb, cr))]
    else:
        hb, wb = -(-H // 8), -(-W // 8)
        real = _fdct_quant(pad(y, hb * 8, wb * 8), qt[0])
        luma = np.zeros((info.blocks_h[0], info.blocks_w[0], 8, 8), np.int16)
        luma[:hb, :wb] = real
        for by in range(info.blocks_h[0]):
            for bx in range(info.blocks_w[0]):
                if by >= hb or bx >= wb:             # a dummy: the DC of the block it repeats, zero AC
                    src = bx if by < hb else (bx | 1)
                    luma[by, bx, 0, 0] = real[min(by, hb - 1), min(src, wb - 1), 0, 0]
        blocks = [luma]
        for c, p in ((1, cb), (2, cr)):
            p = pad(p, H + (H & 1), PW)              # columns to the MCU width, rows only to an even count
            bias = np.tile(np.array([1, 2], np.int32), PW // 4)
            down = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            blocks.append(_fdct_quant(pad(down, PH // 2, PW // 2), qt[c]))    # then replicas of the last row
    flat = torch.empty(info.coef_count + QT_WORDS, dtype=torch.int16)
    for c in range(3):
        n = blocks[c].size
        flat[info.coef_offset[c]:info.coef_offset[c] + n] = torch.from_numpy(blocks[c].reshape(-1))
    flat[info.coef_count:] = torch.from_numpy(qt.astype(np.int16).reshape(-1))
    return JpegCoefficients(info, flat)


# ------------------------------------------------------------------------------------ the host stage
def _check_coefs(coefs: JpegCoefficients) -> torch.Tensor:
    info, flat = coefs.info, coefs.flat
    if info.ncomp != 3 or (info.hmax, info.vmax) not in ((1, 1), (2, 2)) or info.restart_interval != 0:
        raise ValueError("the encoder writes three components in 4:4:4 or 4:2:0 without restart markers")
    if flat.dtype != torch.int16 or flat.dim() != 1 or flat.device.type != "cpu" or not flat.is_contiguous() \
            or flat.numel() < info.coef_count + QT_WORDS:
        raise ValueError("coefficients are a contiguous 1-D int16 CPU tensor of coef_count + 192 elements")
    return flat


def _encode_error(n: int):
    raise ValueError(_lib().lib.jpegenc_last_error().decode() or f"jpegenc_huffman_encode failed ({n})")


def huffman_encode(coefs: JpegCoefficients) -> bytes:
    """The host stage on its own: the file for these coefficient blocks and tables."""
    L = _lib()
    flat = _check_coefs(coefs)
    info = coefs.info
    c = _cinfo(info)
    coef_ptr, qt_ptr = flat.data_ptr(), flat.data_ptr() + info.coef_count * 2
    out = np.empty(info.coef_count // 2 + 1024, dtype=np.uint8)
    n = L.lib.jpegenc_huffman_encode(coef_ptr, qt_ptr, ctypes.byref(c), out.ctypes.data, out.size)
    if n > out.size:                    # the size needed came back: once more with exactly that
        out = np.empty(n, dtype=np.uint8)
        n = L.lib.jpegenc_huffman_encode(coef_ptr, qt_ptr, ctypes.byref(c), out.ctypes.data, out.size)
    if n < 0:
        _encode_error(n)
    return out[:n].tobytes()


def _huffman_batch(host: torch.Tensor, info: JpegInfo, threads: int) -> List[bytes]:
    """``host``: (T, coef_count + 192) int16 CPU rows; one library call on ``threads`` host threads."""
    L = _lib()
    T, words = host.shape
    c = _cinfo(info)
    base = host.data_ptr()
    coefs = (ctypes.c_void_p * T)(*[base + i * words * 2 for i in range(T)])
    qts = (ctypes.c_void_p * T)(*[base + (i * words + info.coef_count) * 2 for i in range(T)])
    sizes = (ctypes.c_int64 * T)()
    bufs = [np.empty(info.coef_count // 2 + 1024, dtype=np.uint8) for _ in range(T)]
    for _ in range(2):                  # a frame that did not fit reports its size: once more with exactly that
        outs = (ctypes.c_void_p * T)(*[b.ctypes.data for b in bufs])
        caps = (ctypes.c_size_t * T)(*[b.size for b in bufs])
        failed = L.lib.jpegenc_huffman_encode_batch(coefs, qts, ctypes.byref(c), T, outs, caps, sizes, int(threads))
        if failed < 0:
            raise ValueError(L.lib.jpegenc_last_error().decode())
        for i in range(T):
            if sizes[i] < 0:
                raise ValueError(f"frame {i}: jpegenc_huffman_encode failed ({sizes[i]})")
        if failed == 0:
            break
        bufs = [b if sizes[i] <= b.size else np.empty(sizes[i], dtype=np.uint8) for i, b in enumerate(bufs)]
    return [bufs[i][:sizes[i]].tobytes() for i in range(T)]


# ------------------------------------------------------------------------------------ the device stage
def _check_device_frames(frames: torch.Tensor) -> None:
    B, H, W, C = frames.shape
    ok = frames.dtype == torch.uint8 and C == 3 and frames.stride(3) == 1 and (W == 1 or frames.stride(2) == 3)
    ok = ok and (H == 1 or frames.stride(1) >= 3 * W)
    ok = ok and (B <= 1 or frames.stride(0) >= (frames.stride(1) if H > 1 else 3 * W) * (H - 1) + 3 * W)
    if not ok:
        raise ValueError("frames must be uint8 (..., H, W, 3) with unit channel stride, pixel stride 3 and rows and "
                         "frames that do not overlap (rows may be pitched)")


def forward_coefficients_device(frames: torch.Tensor, quality: int = 75, subsampling="4:2:0", bgr: bool = False,
                                out: Optional[torch.Tensor] = None, planes: Optional[torch.Tensor] = None
                                ) -> torch.Tensor:
    """The device stage: (B, H, W, 3) uint8 CUDA frames (rows may be pitched) -> (B, coef_count) int16 on the same
    device, both launches on the current stream, nothing waits.  ``out`` / ``planes``: the result and the uint8
    workspace of ``B * coef_count`` bytes to use instead of fresh ones."""
    L = _lib()
    if not torch.is_tensor(frames) or frames.dim() != 4 or not frames.is_cuda:
        raise ValueError("frames must be a (B, H, W, 3) uint8 CUDA tensor")
    _check_device_frames(frames)
    B, H, W, _ = frames.shape
    qt = np.ascontiguousarray(quant_tables(quality).astype(np.uint16).reshape(-1))
    info = frame_info(H, W, subsampling)
    n = info.coef_count
    device = frames.device
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty((B, n), dtype=torch.int16, device=device)
        elif tuple(out.shape) != (B, n) or out.dtype != torch.int16 or out.device != device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int16 tensor of shape {(B, n)} on {device}")
        if planes is None:
            planes = torch.empty(B * n, dtype=torch.uint8, device=device)
        elif planes.dtype != torch.uint8 or planes.device != device or planes.numel() < B * n \
                or not planes.is_contiguous():
            raise ValueError(f"planes must be a contiguous uint8 tensor of at least {B * n} bytes on {device}")
        if B == 0:
            return out
        c = _cinfo(info)
        row_pitch = frames.stride(1) if H > 1 else 3 * W
        frame_pitch = frames.stride(0) if B > 1 else row_pitch * H
        stream = torch.cuda.current_stream(device).cuda_stream
        L.check(L.lib.jpegenc_forward_u8(frames.data_ptr(), row_pitch, frame_pitch, ctypes.byref(c), qt.ctypes.data,
                                         planes.data_ptr(), planes.numel(), out.data_ptr(), n, B, int(bool(bgr)),
                                         stream), "jpegenc_forward_u8")
    return out


def _host_rows(dev: torch.Tensor, info: JpegInfo, quality: int) -> torch.Tensor:
    """Device coefficients (B, coef_count) -> (B, coef_count + 192) int16 on the host with the tables behind them."""
    B, n = dev.shape
    host = torch.empty((B, n + QT_WORDS), dtype=torch.int16)
    host[:, :n] = dev.cpu()
    host[:, n:] = torch.from_numpy(quant_tables(quality).astype(np.int16).reshape(-1))
    return host


def encode_jpeg(frame_u8: torch.Tensor, quality: int = 75, subsampling="4:2:0", bgr: bool = False) -> bytes:
    """One (H, W, 3) uint8 frame -> the bytes of a baseline JPEG file.  A CPU tensor goes through the numpy statement
    and the host stage, a CUDA tensor through the two kernels, a download and the host stage."""
    _check_frame(frame_u8)
    if not frame_u8.is_cuda:
        return huffman_encode(forward_coefficients_host(frame_u8, quality, subsampling, bgr))
    dev = forward_coefficients_device(frame_u8[None], quality, subsampling, bgr)
    info = frame_info(frame_u8.shape[0], frame_u8.shape[1], subsampling)
    return huffman_encode(JpegCoefficients(info, _host_rows(dev, info, quality)[0]))


def encode_jpegs(frames: Sequence[torch.Tensor], threads: int = 4, quality: int = 75, subsampling="4:2:0",
                 bgr: bool = False) -> List[bytes]:
    """Several frames (a (T, H, W, 3) tensor or a sequence of (H, W, 3) tensors).  CUDA frames of one size go through
    one batched device stage; the host stage runs on ``min(threads, frames, 16)`` threads per size, never sized by
    the machine's CPU count."""
    frames = list(frames)
    for f in frames:
        _check_frame(f)
    quant_tables(quality), _hmax(subsampling)
    if int(threads) < 1:
        raise ValueError("threads must be at least 1")
    result: List[Optional[bytes]] = [None] * len(frames)
    groups = {}
    for i, f in enumerate(frames):
        groups.setdefault((tuple(f.shape), f.device), []).append(i)
    for (shape, device), idx in groups.items():
        info = frame_info(shape[0], shape[1], subsampling)
        if device.type == "cuda":
            dev = forward_coefficients_device(torch.stack([frames[i] for i in idx]), quality, subsampling, bgr)
            host = _host_rows(dev, info, quality)
        else:
            host = torch.stack([forward_coefficients_host(frames[i], quality, subsampling, bgr).flat for i in idx])
        for i, data in zip(idx, _huffman_batch(host, info, threads)):
            result[i] = data
    return result
