"""Raw decoded frames (uint8, H x W x 3) -> the padded, normalised ``NestedTensor`` the model reads.

The reference does this on the CPU (data/seq_dataset.py:33-43, ``SeqDataset.process_image``): a target size with short
side 800 and long side at most 1536, an 8-bit bilinear ``cv2.resize``, torchvision's ``to_tensor`` and ``normalize``;
``tensor_list_to_nested_tensor`` then pads to a multiple of 32 with zeros.  Here the whole chain is ONE definition in
integer arithmetic ("Raw-frame ingestion") with two statements that agree to the bit:

  * CUDA frames: one launch of the gfx950 kernel in csrc/frame_ops.hip (6.2 MB in, 13.8 MB out for a 1080p frame),
    on the current stream;
  * CPU frames: the torch integer restatement below.

    batch = preprocess_frames(frames_u8, bgr=True)        # frames as cv2.imread returns them
"""
from __future__ import annotations

import functools
from typing import Optional, Tuple

import numpy as np
import torch

from ..utils.nested_tensor import NestedTensor

MEAN = (0.485, 0.456, 0.406)            # RGB order (reference data/seq_dataset.py:22-23)
STD = (0.229, 0.224, 0.225)
COEF_BITS = 11                          # interpolation weights in 1/2048
COEF_ONE = 1 << COEF_BITS
SIZE_DIVISIBILITY = 32


def target_size(h: int, w: int, short: int = 800, long: int = 1536) -> Tuple[int, int]:
    """The reference's arithmetic (data/seq_dataset.py:35-40), Python floats and the truncation included."""
    s = short / min(h, w)
    if max(h, w) * s > long:
        s = long / max(h, w)
    return int(h * s), int(w * s)


@functools.lru_cache(maxsize=256)
def resize_tables(src: int, dst: int):
    """Per destination index: ``s0`` (int32), ``s1`` (int32) source indices and ``a1`` (int16), the weight of ``s1``
    in 1/2048 (``a0 = 2048 - a1``).  Half-pixel centres, edge clamp, float64 on the host; cached, do not write to them."""
    d = np.arange(dst, dtype=np.float64)
    f = (d + 0.5) * src / dst - 0.5
    s = np.floor(f)
    f -= s
    lo, hi = s < 0, s >= src - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = src - 1, 0
    s0 = s.astype(np.int32)
    s1 = np.minimum(s0 + 1, src - 1).astype(np.int32)
    a1 = np.rint(f.astype(np.float32) * np.float32(COEF_ONE)).astype(np.int16)
    return torch.from_numpy(s0), torch.from_numpy(s1), torch.from_numpy(a1)


@functools.lru_cache(maxsize=1)
def normalize_table() -> torch.Tensor:
    """(3, 256) fp32: level q of channel c after ``to_tensor`` and ``normalize`` -- built with exactly their three
    torch operations, each rounded to fp32.  Both statements read this table."""
    q = torch.arange(256, dtype=torch.float32)
    mean = torch.as_tensor(MEAN, dtype=torch.float32)[:, None]
    std = torch.as_tensor(STD, dtype=torch.float32)[:, None]
    return q.div(255)[None, :].sub(mean).div(std).contiguous()


def padded_size(th: int, tw: int, d: int = SIZE_DIVISIBILITY) -> Tuple[int, int]:
    return -(-th // d) * d, -(-tw // d) * d


_MASKS = {}             # (B, th, tw, Hp, Wp, device) -> the padding mask, one tensor per geometry
_DEVICE_TABLES = {}     # (h, w, th, tw, device) -> (s0x, s1x, a1x, s0y, s1y, b1y, lut) on the device


def _first_use_done(device: torch.device) -> None:
    # filled on the current stream, read from any stream later: wait once, when the geometry is first seen
    if device.type == "cuda":
        torch.cuda.current_stream(device).synchronize()


def padding_mask(B: int, th: int, tw: int, Hp: int, Wp: int, device: torch.device) -> torch.Tensor:
    key = (B, th, tw, Hp, Wp, str(device))
    m = _MASKS.get(key)
    if m is None:
        if len(_MASKS) >= 64:
            _MASKS.clear()
        m = torch.ones((B, Hp, Wp), dtype=torch.bool, device=device)
        m[:, :th, :tw] = False
        _first_use_done(device)
        _MASKS[key] = m
    return m


def _device_tables(h: int, w: int, th: int, tw: int, device: torch.device):
    key = (h, w, th, tw, str(device))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        if len(_DEVICE_TABLES) >= 64:
            _DEVICE_TABLES.clear()
        t = tuple(x.to(device) for x in resize_tables(w, tw) + resize_tables(h, th) + (normalize_table(),))
        _first_use_done(device)
        _DEVICE_TABLES[key] = t
    return t


def _as_frames(frames_u8) -> torch.Tensor:
    if isinstance(frames_u8, np.ndarray):
        if any(s < 0 for s in frames_u8.strides) or not frames_u8.flags.writeable:      # (torch cannot wrap these)
            frames_u8 = np.array(frames_u8, order="C")
        frames_u8 = torch.from_numpy(frames_u8)
    if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8:
        raise TypeError("frames must be uint8 (torch tensor or numpy array)")
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8[None]
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError(f"frames must be (H, W, 3) or (B, H, W, 3), got {tuple(frames_u8.shape)}")
    if frames_u8.shape[1] < 1 or frames_u8.shape[2] < 1:
        raise ValueError("empty frame")
    return frames_u8


def _resize_levels_cpu(frames: torch.Tensor, th: int, tw: int) -> torch.Tensor:
    """(B, th, tw, 3) int32 levels 0..255: the 8-bit bilinear resize, in the integer arithmetic of the definition."""
    h, w = frames.shape[1:3]
    s0x, s1x, a1x = resize_tables(w, tw)
    s0y, s1y, b1y = resize_tables(h, th)
    s0x, s1x, s0y, s1y = s0x.long(), s1x.long(), s0y.long(), s1y.long()
    a1 = a1x.to(torch.int32)[None, None, :, None]
    a0 = COEF_ONE - a1
    b1 = b1y.to(torch.int32)[None, :, None, None]
    b0 = COEF_ONE - b1

    def row_pass(rows: torch.Tensor) -> torch.Tensor:
        p = frames.index_select(1, rows)
        return p.index_select(2, s0x).to(torch.int32) * a0 + p.index_select(2, s1x).to(torch.int32) * a1

    r0, r1 = row_pass(s0y), row_pass(s1y)
    return (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2


def _check_out(out: torch.Tensor, shape, device) -> None:
    if (tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(shape)} on {device}")


@torch.no_grad()
def preprocess_frames(frames_u8, *, bgr: bool = False, out: Optional[torch.Tensor] = None,
                      size: Optional[Tuple[int, int]] = None) -> NestedTensor:
    """``frames_u8``: (H, W, 3) or (B, H, W, 3) uint8, torch (CPU or CUDA) or numpy, RGB (``bgr=True``: the order
    ``cv2.imread`` gives; channels 0 and 2 are swapped).  Rows and frames may be pitched (any strides with unit pixel
    and channel strides go to the kernel as they are; anything else is made contiguous first).

    Returns the batch as the reference's ``tensor_list_to_nested_tensor`` would build it from ``process_image``
    outputs: ``tensors`` (B, 3, Hp, Wp) fp32 with exact zeros on the padding, ``masks`` (B, Hp, Wp) bool (True on
    padding; ONE cached tensor per geometry, do not write to it) and ``sizes``.  ``out``: a preallocated (B, 3, Hp, Wp)
    fp32 batch that is overwritten in full, padding included.  ``size``: (th, tw) instead of ``target_size(H, W)``.

    CUDA frames run the kernel on the current stream of their device and nothing here waits for it (apart from the
    first call of a geometry, which uploads its tables); the caller orders the source and the result with that stream.
    """
    frames = _as_frames(frames_u8)
    B, h, w = frames.shape[:3]
    th, tw = target_size(h, w) if size is None else (int(size[0]), int(size[1]))
    if th < 1 or tw < 1:
        raise ValueError(f"target size {(th, tw)} of a {(h, w)} frame is empty")
    Hp, Wp = padded_size(th, tw)
    device = frames.device
    shape = (B, 3, Hp, Wp)
    if out is not None:
        _check_out(out, shape, device)
    sizes = ((Hp, Wp),) + ((th, tw),) * B

    if device.type == "cuda":
        from .. import _frame_lib            # no substitute: a missing library is an error
        if frames.stride(3) != 1 or frames.stride(2) != 3 or frames.stride(1) < 3 * w or (B > 1 and frames.stride(0) < 0):
            frames = frames.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=device)
        if B:
            s0x, s1x, a1x, s0y, s1y, b1y, lut = _device_tables(h, w, th, tw, device)
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream(device).cuda_stream
                _frame_lib.check(_frame_lib.lib.frameops_resize_normalize_u8(
                    frames.data_ptr(), frames.stride(1), frames.stride(0), B, h, w, s0x.data_ptr(), s1x.data_ptr(),
                    a1x.data_ptr(), s0y.data_ptr(), s1y.data_ptr(), b1y.data_ptr(), th, tw, Hp, Wp, lut.data_ptr(),
                    int(bool(bgr)), out.data_ptr(), stream), "frameops_resize_normalize_u8")
        return NestedTensor(out, padding_mask(B, th, tw, Hp, Wp, device), sizes=sizes)

    q = _resize_levels_cpu(frames, th, tw).long()
    lut = normalize_table()
    out = torch.zeros(shape, dtype=torch.float32) if out is None else out.zero_()
    for c in range(3):
        out[:, c, :th, :tw] = lut[c][q[..., 2 - c if bgr else c]]
    return NestedTensor(out, padding_mask(B, th, tw, Hp, Wp, device), sizes=sizes)
