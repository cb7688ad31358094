"""Training clips made from ONE still image (CrowdHuman in the MOT17 joint training, reference data/mot17.py:249-269):
flip -> ``MultiRandomShift`` -> the resize / crop branch -> HSV -> normalise -> reverse.

``MultiRandomShift`` (reference data/transforms.py:173-223) makes frame k by cropping a window moved by (dx, dy) out of
frame k - 1 and resizing it back to the image size.  The crop is always ``w`` wide (:211 takes ``max(w, w - x_shift)``;
kept as it is, so ``dx > 0`` moves nothing and ``dx < 0`` pads with black on the right), hence every derived frame is a
vertical Pillow resample of ``hc = h - |dy|`` rows to ``h`` plus a move by ``s = max(0, -dx)`` columns: ONE definition
in integer arithmetic ("Static-image clips") with two statements that agree to the bit:

  * a CUDA image: one launch of the gfx950 kernel of csrc/static_clip_ops.hip for the whole clip, on the current stream;
  * a CPU image: ``shift_chain_cpu`` below, built on ``augment.resample_tables``.

The boxes follow on the host with the reference's float32 operations (``shift_infos``).

    plan = sample_clip_augment(h, w, random.Random(seed), np.random.RandomState(seed), max_shift=50)
    nested, infos = augment_static_clip(image_u8, info, plan, clip_len=5)          # (H, W, 3) uint8, boxes xyxy
    loss, _ = clip_forward_backward(model, criterion, clip_batch(nested, infos), device)
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional

import torch

from . import augment as _augment
from . import frames as _frames


def _geometry(h: int, w: int, T: int, dx: int, dy: int):
    """(s, y0, hc): the column move and the row window y0 .. y0 + hc - 1 of the previous frame (transforms.py:208-214)."""
    dx, dy = int(dx), int(dy)
    if T < 1:
        raise ValueError(f"a clip has at least one frame, got T = {T}")
    if abs(dy) >= h:
        raise ValueError(f"|dy| = {abs(dy)} leaves no row of a {h}-row image")
    return max(0, -dx), max(0, -dy), h - abs(dy)


def _as_image(image_u8) -> torch.Tensor:
    frames = _frames._as_frames(image_u8)
    if frames.shape[0] != 1:
        raise ValueError(f"a static clip is made from one image, got {frames.shape[0]}")
    return frames[0]


def shift_chain_cpu(image, T: int, dx: int, dy: int, flip: bool = False, swap_rb: bool = False) -> torch.Tensor:
    """The host statement: (h, w, 3) uint8 -> the (T, h, w, 3) uint8 clip.  Frame 0 is the image (mirrored if ``flip``,
    channels 0 and 2 swapped if ``swap_rb``); frame k is the window of frame k - 1 at column ``s``, row ``y0``, ``w``
    wide (black where it leaves the image) and ``hc`` tall, through Pillow's 8-bit vertical resample to ``h`` rows."""
    p = _as_image(image).cpu()
    h, w = p.shape[:2]
    s, y0, hc = _geometry(h, w, T, dx, dy)
    if flip:
        p = p.flip(1)
    if swap_rb:
        p = p.flip(2)
    tables = _augment.resample_tables(hc, h)
    frames = [p.contiguous()]
    for _ in range(1, T):
        window = torch.zeros((1, hc, w, 3), dtype=torch.uint8)
        if s < w:
            window[0, :, :w - s] = frames[-1][y0:y0 + hc, s:]
        frames.append(_augment._pass_cpu(window, 1, tables)[0])
    return torch.stack(frames)


@torch.no_grad()
def shift_chain(image_u8, T: int, dx: int, dy: int, flip: bool = False, swap_rb: bool = False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``image_u8``: (H, W, 3) or (1, H, W, 3) uint8, torch (CPU or CUDA) or numpy, rows may be pitched as for
    ``preprocess_frames``.  Returns the (T, H, W, 3) uint8 clip on the image's device.  ``out``: a uint8 tensor of that
    shape and device whose rows and frames may be pitched (unit channel stride, pixel stride 3, frames not
    overlapping); every byte of the T frames is written and nothing between them.

    A CUDA image runs the kernel on the current stream of its device and nothing here waits for it (apart from the
    first use of a geometry's table, which uploads it); a CPU image takes ``shift_chain_cpu``; the two are bit-equal."""
    image = _as_image(image_u8)
    h, w = image.shape[:2]
    T = int(T)
    s, y0, hc = _geometry(h, w, T, dx, dy)
    device = image.device
    if out is not None:
        if (tuple(out.shape) != (T, h, w, 3) or out.dtype != torch.uint8 or out.device != device or out.stride(3) != 1
                or out.stride(2) != 3 or out.stride(1) < 3 * w
                or (T > 1 and out.stride(0) < (h - 1) * out.stride(1) + 3 * w)):
            raise ValueError(f"out must be a uint8 tensor of shape {(T, h, w, 3)} on {device} with unit channel stride, "
                             "pixel stride 3 and frames that do not overlap")
    if device.type != "cuda":
        clip = shift_chain_cpu(image, T, dx, dy, flip, swap_rb)
        return clip if out is None else out.copy_(clip)

    from .. import _static_clip_lib as L     # no substitute: a missing library is an error
    if image.stride(2) != 1 or image.stride(1) != 3 or image.stride(0) < 3 * w:
        image = image.contiguous()
    if out is None:
        out = torch.empty((T, h, w, 3), dtype=torch.uint8, device=device)
    xmin, cnt, kk = _augment._device_tables(hc, h, device)
    with torch.cuda.device(device):
        L.check(L.lib.staticclip_shift_chain(
            image.data_ptr(), image.stride(0), h, w, T, int(bool(flip)), int(bool(swap_rb)), s, y0, hc,
            xmin.data_ptr(), cnt.data_ptr(), kk.data_ptr(), kk.shape[1], out.data_ptr(), out.stride(1), out.stride(0),
            torch.cuda.current_stream(device).cuda_stream), "staticclip_shift_chain")
    return out


def shift_infos(info: dict, T: int, dx: int, dy: int, h: int, w: int) -> List[dict]:
    """The T infos of the clip: ``info`` (a copy), then each from the one before with the reference's float32 torch
    operations in its order (transforms.py:194-204): minus (s, y0, s, y0), times the Python-float ratios
    (w / w, h / hc, w / w, h / hc), pairwise min with (w, h), clamp at 0, keep the boxes with hi > lo in both axes
    (``labels``, ``ids``, ``boxes``, ``areas`` filtered alike).  ``areas`` are not rescaled and a dropped box stays
    dropped.  An info without ``"boxes"`` is copied as it is."""
    s, y0, hc = _geometry(h, w, T, dx, dy)
    out = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in info.items()}]
    for _ in range(1, T):
        nxt = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out[-1].items()}
        if "boxes" in nxt:
            boxes = nxt["boxes"].reshape(-1, 4) - torch.as_tensor([s, y0, s, y0])
            boxes *= torch.as_tensor([w / w, h / hc, w / w, h / hc])
            boxes = torch.min(boxes.reshape(-1, 2, 2), torch.as_tensor([w, h])).clamp(min=0)
            keep = torch.all(boxes[:, 1, :] > boxes[:, 0, :], dim=1)
            nxt["boxes"] = boxes.reshape(-1, 4)
            for field in ("labels", "ids", "boxes", "areas"):
                nxt[field] = nxt[field][keep]
        out.append(nxt)
    return out


@torch.no_grad()
def augment_static_clip(image_u8, info: dict, plan: _augment.ClipAugment, clip_len: int, *, bgr: bool = False,
                        overflow_bbox: bool = False, out: Optional[torch.Tensor] = None):
    """One still image and its info -> what ``augment_clip`` returns for a clip of ``clip_len`` frames,
    ``(NestedTensor, infos)``, in the reference's order of work: the flip (image and boxes), the shift chain with its
    infos, the shift stage's own reversal (``plan.shift_reverse``), then ``augment_clip``'s resize / crop branch, HSV,
    normalisation and ``plan.reverse``.  Frames go through the rest independently of their position, so the two
    reversals are applied as one at the end.  ``plan.shift`` is (dx, dy); a plan without one raises ``ValueError``.
    ``out``: as for ``augment_clip``.  The result goes to ``clip_batch`` unchanged."""
    if plan.shift is None:
        raise ValueError("the plan has no shift: sample it with max_shift, or set ClipAugment.shift")
    dx, dy = (int(x) for x in plan.shift)
    image = _as_image(image_u8)
    h, w = image.shape[:2]
    T = int(clip_len)
    _geometry(h, w, T, dx, dy)
    info = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in info.items()}
    if "boxes" not in info:
        raise KeyError("info has no key: boxes")
    info["boxes"] = info["boxes"].reshape(-1, 4)
    if plan.flip and len(info["boxes"]) > 0:                    # transforms.py:61-62
        info["boxes"] = (info["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1])
                         + torch.as_tensor([w, 0, w, 0]))
    frames = shift_chain(image, T, dx, dy, flip=plan.flip, swap_rb=bgr)
    infos = shift_infos(info, T, dx, dy, h, w)
    rest = dataclasses.replace(plan, flip=False, reverse=plan.reverse != plan.shift_reverse)
    return _augment.augment_clip(frames, infos, rest, overflow_bbox=overflow_bbox, out=out)
