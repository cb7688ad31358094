"""Training-clip augmentation: raw uint8 frames + pixel boxes -> the padded, normalised clip the train step reads.

The reference does this on the CPU (data/transforms.py composed by data/dancetrack.py:152-174): horizontal flip, then
either a random resize or resize -> random crop -> resize (PIL bilinear), an HSV jitter (cv2), ``to_tensor``,
``normalize`` and an optional clip reversal, each with its box bookkeeping.  Here the random decisions are drawn once
into a ``ClipAugment`` plan (``sample_clip_augment``), the boxes follow the plan on the host (``augment_infos``) and the
pixels are ONE definition in integer arithmetic ("Training-clip augmentation") with two statements that
agree to the bit:

  * CUDA frames: the gfx950 kernel of csrc/augment_ops.hip on the current stream, one launch for the plain branch and
    two for the crop branch;
  * CPU frames: the torch integer restatement below.

The resize is Pillow's 8-bit fixed-point bilinear resample restated to the bit (tests/test_augment_cpu.py compares with
``Image.resize(..., BILINEAR)`` byte for byte); the HSV round trip is the project's own integer statement of OpenCV's
published 8-bit formulas (cv2 parity is not pinned).

    plan = sample_clip_augment(h, w, random.Random(seed), np.random.RandomState(seed))
    nested, infos = augment_clip(frames_u8, infos, plan)          # (T, H, W, 3) uint8, boxes xyxy in pixels
    loss, _ = clip_forward_backward(model, criterion, clip_batch(nested, infos), device)
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..utils.box_ops import box_xyxy_to_cxcywh
from ..utils.nested_tensor import NestedTensor
from . import frames as _frames

SCALES = (608, 640, 672, 704, 736, 768, 800, 832, 864, 896, 928, 960, 992)     # reference data/dancetrack.py:153
PRECISION_BITS = 32 - 8 - 2             # Pillow's 8-bit resample: coefficients in 1/2**22
HSV_GAINS = (5, 30, 30)                 # reference data/transforms.py:230
HSV_SHIFT = 12
HSV_D = 255 * 30                        # 7650: denominator of the HSV -> RGB sector formulas


# ------------------------------------------------------------------------------------------------- the definition
@functools.lru_cache(maxsize=256)
def resample_tables(n_in: int, n_out: int):
    """``xmin`` (n_out) int32, ``cnt`` (n_out) int32, ``kk`` (n_out, ksize) int32: the taps of Pillow's triangle
    filter (support 1.0) for an axis of ``n_in`` samples resampled to ``n_out``, as ``precompute_coeffs`` and
    ``normalize_coeffs_8bpc`` build them: float64, weights summed in tap order, ``int(0.5 + w * 2**22)``.  (Pillow
    multiplies by ``1 / filterscale`` where one could divide; so does this.)  Cached, do not write to them."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"cannot resample {n_in} samples to {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    c = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((c - support + 0.5).astype(np.int64), 0)          # C truncation; the operand is > -1
    cnt = np.minimum((c + support + 0.5).astype(np.int64), n_in) - xmin
    w = np.zeros((n_out, ksize), dtype=np.float64)
    ww = np.zeros(n_out, dtype=np.float64)
    for x in range(ksize):
        wx = np.maximum(0.0, 1.0 - np.abs((x + xmin - c + 0.5) * ss))
        wx[x >= cnt] = 0.0
        w[:, x] = wx
        ww += wx
    nz = ww != 0.0
    w[nz] /= ww[nz, None]
    kk = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)
    return (torch.from_numpy(xmin.astype(np.int32)), torch.from_numpy(cnt.astype(np.int32)), torch.from_numpy(kk))


def _slice_tables(tables, lo: int, n: int):
    """Output indices lo .. lo+n-1 of a resize's tables: that resize followed by a crop of the axis."""
    xmin, cnt, kk = tables
    if lo < 0 or n < 1 or lo + n > len(xmin):
        raise ValueError(f"window [{lo}, {lo + n}) is not inside the {len(xmin)} resized samples")
    return xmin[lo:lo + n], cnt[lo:lo + n], kk[lo:lo + n]


def new_hw(w: int, h: int, size, max_size: Optional[int] = None) -> Tuple[int, int]:
    """The reference's ``get_new_hw`` (data/transforms.py:80-93) for a ``w`` x ``h`` image: (new_h, new_w), with its
    two roundings kept (``int(round(size * h / w))`` for portrait, the truncating ``int(round(size) * w / h)`` for
    landscape).  A list or tuple ``size`` is (w, h), as there, and comes back as (h, w)."""
    if isinstance(size, (list, tuple)):
        if len(size) != 2:
            raise ValueError(f"size length should be 2, got {len(size)}")
        return int(size[1]), int(size[0])
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(math.floor(max_size * lo / hi))
    if w < h:
        return int(round(size * h / w)), size
    return size, int(round(size) * w / h)


@functools.lru_cache(maxsize=1)
def hsv_tables() -> torch.Tensor:
    """(2, 256) int32: ``sdiv[i] = rint((255 << 12) / i)`` and ``hdiv[i] = rint((180 << 12) / (6 * i))``, 0 at i = 0."""
    i = np.arange(1, 256, dtype=np.float64)
    t = np.zeros((2, 256), dtype=np.int32)
    t[0, 1:] = np.rint((255 << HSV_SHIFT) / i)
    t[1, 1:] = np.rint((180 << HSV_SHIFT) / (6.0 * i))
    return torch.from_numpy(t)


def rgb_to_hsv(rgb: torch.Tensor) -> torch.Tensor:
    """(..., 3) integer RGB levels -> (..., 3) int32 H (0..179), S, V (0..255): OpenCV's 8-bit formulas in integers."""
    sdiv, hdiv = hsv_tables()
    r, g, b = (x.to(torch.int32) for x in rgb.unbind(-1))
    v = torch.maximum(torch.maximum(r, g), b)
    d = v - torch.minimum(torch.minimum(r, g), b)
    half = 1 << (HSV_SHIFT - 1)
    s = (d * sdiv[v.long()] + half) >> HSV_SHIFT
    h0 = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * hdiv[d.long()] + half) >> HSV_SHIFT                   # arithmetic shift
    h = torch.where(h < 0, h + 180, h)
    return torch.stack((h, s, v), -1)


def hsv_to_rgb(hsv: torch.Tensor) -> torch.Tensor:
    """(..., 3) integer H (0..179), S, V (0..255) -> (..., 3) int32 RGB levels."""
    h, s, v = (x.to(torch.int32) for x in hsv.unbind(-1))
    sec = torch.div(h, 30, rounding_mode="floor")
    f = h - sec * 30
    D = HSV_D
    p = torch.div(v * (255 - s) * 30 + D // 2, D, rounding_mode="floor")
    q = torch.div(v * (D - s * f) + D // 2, D, rounding_mode="floor")
    t = torch.div(v * (D - s * (30 - f)) + D // 2, D, rounding_mode="floor")
    order = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = []
    for c in range(3):
        x = order[5][c]
        for k in range(4, -1, -1):
            x = torch.where(sec == k, order[k][c], x)
        out.append(x)
    return torch.stack(out, -1)


def hsv_jitter(rgb: torch.Tensor, dh: int, ds: int, dv: int) -> torch.Tensor:
    """The round trip RGB -> HSV, ``h = (h + dh) mod 180``, ``s``, ``v`` shifted and clamped to 0..255, -> RGB.
    (..., 3) integer levels in, int32 levels out; applied even for zero gains, as the reference does."""
    h, s, v = rgb_to_hsv(rgb).unbind(-1)
    h = torch.remainder(h + int(dh), 180)
    s = (s + int(ds)).clamp(0, 255)
    v = (v + int(dv)).clamp(0, 255)
    return hsv_to_rgb(torch.stack((h, s, v), -1))


def _pass_cpu(p: torch.Tensor, axis: int, tables) -> torch.Tensor:
    """One resample pass over ``axis`` of the uint8 tensor ``p``: ``clamp((2**21 + sum p * kk) >> 22, 0, 255)``."""
    xmin, cnt, kk = tables
    n_in = p.shape[axis]
    shape = [1] * p.dim()
    shape[axis] = -1
    acc = None
    for x in range(int(cnt.max())):
        idx = (xmin.long() + x).clamp_(max=n_in - 1)               # past cnt the coefficient is 0
        term = p.index_select(axis, idx).to(torch.int32) * kk[:, x].reshape(shape)
        acc = term if acc is None else acc.add_(term)
    return ((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS).clamp_(0, 255).to(torch.uint8)


def resample_cpu(frames: torch.Tensor, tables_x, tables_y, flip: bool = False, swap_rb: bool = False) -> torch.Tensor:
    """(T, h, w, 3) uint8 -> (T, oh, ow, 3) uint8: horizontal pass to a uint8 intermediate, then the vertical pass
    over it (Pillow's order).  ``flip``: table column x reads source column w - 1 - x."""
    if flip:
        frames = frames.flip(2)
    if swap_rb:
        frames = frames.flip(3)
    ymin, ycnt, ykk = tables_y
    r0, r1 = int(ymin.min()), int((ymin + ycnt).max())             # the rows the vertical pass reads
    mid = _pass_cpu(frames[:, r0:r1], 2, tables_x)
    return _pass_cpu(mid, 1, (ymin - r0, ycnt, ykk))


# ------------------------------------------------------------------------------------------------- plan and boxes
@dataclasses.dataclass(frozen=True)
class ClipAugment:
    """The random decisions of one clip.  ``first``: (h1, w1) of the crop branch's first resize; ``crop``:
    (i, j, ch, cw), top, left, height, width inside the ``first``-resized frame; ``final``: (th, tw); ``hsv``:
    (dh, ds, dv) or None for no round trip at all; ``reverse``: the clip's frames and infos come out last first.
    ``shift``: (dx, dy) of a clip made from one still image and ``shift_reverse``, that stage's own reversal; read by
    ``static_clip.augment_static_clip`` only."""
    flip: bool
    first: Optional[Tuple[int, int]]
    crop: Optional[Tuple[int, int, int, int]]
    final: Tuple[int, int]
    hsv: Optional[Tuple[int, int, int]] = None
    reverse: bool = False
    shift: Optional[Tuple[int, int]] = None
    shift_reverse: bool = False


def sample_clip_augment(h: int, w: int, rng, np_rng, *, coco_size: bool = False, reverse_clip: float = 0.0,
                        scales: Sequence[int] = SCALES, max_size: int = 1536,
                        max_shift: Optional[int] = None) -> ClipAugment:
    """A plan for ``h`` x ``w`` frames with the decision structure of the reference's ``transfroms_for_train``.
    ``rng``: a ``random.Random``, ``np_rng``: a ``np.random.RandomState``.  (The draws are not the reference's draws:
    it reads the global generators of three libraries.)  ``max_shift`` (the reference's ``MultiRandomShift`` has 50):
    the plan of a clip made from one still image, ``|dx|`` and ``|dy|`` uniform in 1 .. max_shift, fair signs and a
    fair ``shift_reverse``, drawn after everything else; None draws nothing more and gives the plans it always gave."""
    if max_shift is not None and max_shift < 1:
        raise ValueError(f"max_shift must be at least 1, got {max_shift}")
    flip = rng.random() < 0.5
    first = crop = None
    if rng.random() < 0.5:
        final = new_hw(w, h, rng.choice(list(scales)), max_size)
    else:
        h1, w1 = new_hw(w, h, rng.choice([400, 500, 600] if coco_size else [800, 1000, 1200]), None)
        lo, hi = (384, 600) if coco_size else (800, 1200)
        cw = rng.randint(lo, min(w1, hi))
        ch = rng.randint(lo, min(h1, hi))
        i = rng.randint(0, h1 - ch)
        j = rng.randint(0, w1 - cw)
        first, crop = (h1, w1), (i, j, ch, cw)
        final = new_hw(cw, ch, rng.choice(list(scales)), max_size)
    gains = np_rng.uniform(-1, 1, 3) * list(HSV_GAINS)
    gains = gains * np_rng.randint(0, 2, 3)
    hsv = tuple(int(x) for x in gains.astype(np.int16))
    reverse = rng.random() < reverse_clip
    shift, shift_reverse = None, False
    if max_shift is not None:
        dx = rng.randint(1, max_shift) * (1 if rng.random() < 0.5 else -1)
        dy = rng.randint(1, max_shift) * (1 if rng.random() < 0.5 else -1)
        shift, shift_reverse = (dx, dy), rng.random() < 0.5
    return ClipAugment(flip=flip, first=first, crop=crop, final=final, hsv=hsv, reverse=reverse, shift=shift,
                       shift_reverse=shift_reverse)


def _branch(plan: ClipAugment, h: int, w: int):
    """None for the plain branch, else ((h1, w1), (i, j, ch, cw)) with the missing half filled in."""
    if plan.first is None and plan.crop is None:
        return None
    h1, w1 = (int(x) for x in plan.first) if plan.first is not None else (h, w)
    i, j, ch, cw = (int(x) for x in plan.crop) if plan.crop is not None else (0, 0, h1, w1)
    if i < 0 or j < 0 or ch < 1 or cw < 1 or i + ch > h1 or j + cw > w1:
        raise ValueError(f"crop {(i, j, ch, cw)} is not inside the {h1}x{w1} frame")
    return (h1, w1), (i, j, ch, cw)


def augment_infos(plan: ClipAugment, infos: List[dict], h: int, w: int, overflow_bbox: bool = False) -> List[dict]:
    """Per frame {"boxes" (N, 4) xyxy in pixels of the ``h`` x ``w`` frame, "ids", "labels", "areas"} -> what the
    reference's transforms leave: flip (transforms.py:61-62), resize ratios on boxes and areas (:101-107), crop
    shift / clamp / keep filter (:152-167; with ``overflow_bbox`` the kept boxes stay unclamped), then cxcywh divided
    by (tw, th, tw, th) (:130-132); the list reversed if ``plan.reverse``.  The inputs are not modified."""
    branch = _branch(plan, h, w)
    th, tw = (int(x) for x in plan.final)
    out = []
    for info in infos:
        info = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in info.items()}
        for key in ("boxes", "areas"):
            if key not in info:
                raise KeyError(f"info has no key: {key}")
        info["boxes"] = info["boxes"].reshape(-1, 4)
        cw_, ch_ = w, h                                            # the current frame size

        def resize(nh, nw):
            nonlocal cw_, ch_
            rw, rh = float(nw) / float(cw_), float(nh) / float(ch_)
            if len(info["boxes"]) > 0:
                info["boxes"] = info["boxes"] * torch.as_tensor([rw, rh, rw, rh])
                info["areas"] = info["areas"] * rw * rh
            cw_, ch_ = nw, nh

        if plan.flip and len(info["boxes"]) > 0:
            info["boxes"] = (info["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1])
                             + torch.as_tensor([w, 0, w, 0]))
        if branch is not None:
            (h1, w1), (i, j, ch, cw) = branch
            resize(h1, w1)
            if len(info["boxes"]) > 0:
                info["boxes"] = info["boxes"] - torch.as_tensor([j, i, j, i])
                max_wh = torch.as_tensor([cw, ch])
                boxes = torch.min(info["boxes"].reshape(-1, 2, 2), max_wh).clamp(min=0)
                keep = torch.all(boxes[:, 1, :] > boxes[:, 0, :], dim=1)
                if not overflow_bbox:
                    info["boxes"] = boxes.reshape(-1, 4)
                for field in ("labels", "ids", "boxes", "areas"):
                    info[field] = info[field][keep]
            cw_, ch_ = cw, ch
        resize(th, tw)
        if len(info["boxes"]) > 0:
            info["boxes"] = box_xyxy_to_cxcywh(info["boxes"]) / torch.as_tensor([tw, th, tw, th])
        out.append(info)
    if plan.reverse:
        out.reverse()
    return out


# ------------------------------------------------------------------------------------------------- the pixels
_DEVICE_TABLES = {}     # (n_in, n_out, device) -> (xmin, cnt, kk) on the device
_DEVICE_CONSTS = {}     # device -> (normalisation table, hsv tables) on the device


def _device_tables(n_in: int, n_out: int, device: torch.device):
    key = (n_in, n_out, str(device))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        if len(_DEVICE_TABLES) >= 256:
            _DEVICE_TABLES.clear()
        t = tuple(x.to(device) for x in resample_tables(n_in, n_out))
        _frames._first_use_done(device)         # filled on the current stream, read from any stream later
        _DEVICE_TABLES[key] = t
    return t


def _device_consts(device: torch.device):
    t = _DEVICE_CONSTS.get(str(device))
    if t is None:
        t = (_frames.normalize_table().to(device), hsv_tables().to(device))
        _frames._first_use_done(device)
        _DEVICE_CONSTS[str(device)] = t
    return t


def _launch(lib_mod, src, T, h, w, flip, swap_rb, tx, ty, oh, ow, *, out_u8=None, out_f32=None, Hp=0, Wp=0, lut=None,
            hsv_t=None, hsv=None, reverse=False, stream=0):
    xmin_x, cnt_x, kk_x = tx
    xmin_y, cnt_y, kk_y = ty
    dh, ds, dv = hsv if hsv is not None else (0, 0, 0)
    lib_mod.check(lib_mod.lib.augops_resample_u8(
        src.data_ptr(), src.stride(1), src.stride(0), T, h, w, int(bool(flip)), int(bool(swap_rb)),
        xmin_x.data_ptr(), cnt_x.data_ptr(), kk_x.data_ptr(), kk_x.shape[1],
        xmin_y.data_ptr(), cnt_y.data_ptr(), kk_y.data_ptr(), kk_y.shape[1], oh, ow,
        lib_mod.STAGE_U8 if out_f32 is None else lib_mod.STAGE_F32,
        None if out_u8 is None else out_u8.data_ptr(), 0 if out_u8 is None else out_u8.stride(1),
        0 if out_u8 is None else out_u8.stride(0),
        None if out_f32 is None else out_f32.data_ptr(), Hp, Wp, None if lut is None else lut.data_ptr(),
        None if hsv_t is None else hsv_t.data_ptr(), int(hsv is not None), int(dh), int(ds), int(dv),
        int(bool(reverse)), stream), "augops_resample_u8")


def resample_plan_cpu(frames: torch.Tensor, plan: ClipAugment, *, bgr: bool = False) -> torch.Tensor:
    """The resize part of ``plan`` on (T, h, w, 3) uint8 CPU frames -> (T, th, tw, 3) uint8 levels: flip, then one
    resize, or resize -> crop -> resize with the first resize computed on the crop window only."""
    h, w = frames.shape[1:3]
    th, tw = (int(x) for x in plan.final)
    branch = _branch(plan, h, w)
    if branch is None:
        return resample_cpu(frames, resample_tables(w, tw), resample_tables(h, th), plan.flip, bgr)
    (h1, w1), (i, j, ch, cw) = branch
    q = resample_cpu(frames, _slice_tables(resample_tables(w, w1), j, cw),
                     _slice_tables(resample_tables(h, h1), i, ch), plan.flip, bgr)
    return resample_cpu(q, resample_tables(cw, tw), resample_tables(ch, th))


@torch.no_grad()
def augment_clip(frames_u8, infos: List[dict], plan: ClipAugment, *, bgr: bool = False, overflow_bbox: bool = False,
                 out: Optional[torch.Tensor] = None):
    """``frames_u8``: (T, H, W, 3) uint8, torch (CPU or CUDA) or numpy, RGB (``bgr=True``: channels 0 and 2 are
    swapped on the way in), rows and frames may be pitched as for ``preprocess_frames``.  ``infos``: one dict per frame
    for ``augment_infos``.  Returns ``(NestedTensor, infos')``: ``tensors`` (T, 3, Hp, Wp) fp32 with exact zeros on the
    padding (``out``, when given, is overwritten in full), ``masks`` (ONE cached tensor per geometry, do not write to
    it), ``sizes``; frames and infos last first if ``plan.reverse``.

    CUDA frames run the kernel on the current stream of their device and nothing here waits for it (apart from the
    first use of a geometry's tables, which uploads them); CPU frames take the host statement; the two are bit-equal.
    The infos stay on the host."""
    frames = _frames._as_frames(frames_u8)
    T, h, w = frames.shape[:3]
    if len(infos) != T:
        raise ValueError(f"{len(infos)} infos for {T} frames")
    th, tw = (int(x) for x in plan.final)
    if th < 1 or tw < 1:
        raise ValueError(f"final size {(th, tw)} is empty")
    branch = _branch(plan, h, w)
    hsv = None if plan.hsv is None else tuple(int(x) for x in plan.hsv)
    new_infos = augment_infos(plan, infos, h, w, overflow_bbox)
    Hp, Wp = _frames.padded_size(th, tw)
    device = frames.device
    shape = (T, 3, Hp, Wp)
    if out is not None:
        _frames._check_out(out, shape, device)
    sizes = ((Hp, Wp),) + ((th, tw),) * T

    if device.type == "cuda":
        from .. import _augment_lib          # no substitute: a missing library is an error
        if frames.stride(3) != 1 or frames.stride(2) != 3 or frames.stride(1) < 3 * w or (T > 1 and frames.stride(0) < 0):
            frames = frames.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=device)
        if T:
            lut, hsv_t = _device_consts(device)
            last = dict(out_f32=out, Hp=Hp, Wp=Wp, lut=lut, hsv_t=hsv_t, hsv=hsv, reverse=plan.reverse)
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream(device).cuda_stream
                if branch is None:
                    _launch(_augment_lib, frames, T, h, w, plan.flip, bgr, _device_tables(w, tw, device),
                            _device_tables(h, th, device), th, tw, stream=stream, **last)
                else:
                    (h1, w1), (i, j, ch, cw) = branch
                    mid = torch.empty((T, ch, cw, 3), dtype=torch.uint8, device=device)
                    _launch(_augment_lib, frames, T, h, w, plan.flip, bgr,
                            _slice_tables(_device_tables(w, w1, device), j, cw),
                            _slice_tables(_device_tables(h, h1, device), i, ch), ch, cw, out_u8=mid, stream=stream)
                    _launch(_augment_lib, mid, T, ch, cw, False, False, _device_tables(cw, tw, device),
                            _device_tables(ch, th, device), th, tw, stream=stream, **last)
        return NestedTensor(out, _frames.padding_mask(T, th, tw, Hp, Wp, device), sizes=sizes), new_infos

    q = resample_plan_cpu(frames, plan, bgr=bgr)
    if hsv is not None:
        q = hsv_jitter(q, *hsv)
    if plan.reverse:
        q = q.flip(0)
    q = q.long()
    lut = _frames.normalize_table()
    out = torch.zeros(shape, dtype=torch.float32) if out is None else out.zero_()
    for c in range(3):
        out[:, c, :th, :tw] = lut[c][q[..., c]]
    return NestedTensor(out, _frames.padding_mask(T, th, tw, Hp, Wp, device), sizes=sizes), new_infos


def clip_batch(nested: NestedTensor, infos: List[dict]) -> dict:
    """The ``{"imgs": [[...]], "infos": [[...]]}`` batch (one clip) that ``engine.clip_forward_backward`` takes: the
    frames as views ``tensors[t, :, :th, :tw]`` of the padded batch, the infos reduced to ids, labels and boxes."""
    T = nested.tensors.shape[0]
    if len(infos) != T:
        raise ValueError(f"{len(infos)} infos for {T} frames")
    if nested.sizes is None or len(nested.sizes) != T + 1:
        raise ValueError("the NestedTensor carries no frame sizes (it is not the result of augment_clip)")
    imgs = [nested.tensors[t, :, :th, :tw] for t, (th, tw) in enumerate(nested.sizes[1:])]
    keep = [{"ids": i["ids"], "labels": i["labels"], "boxes": i["boxes"]} for i in infos]
    return {"imgs": [imgs], "infos": [keep]}
