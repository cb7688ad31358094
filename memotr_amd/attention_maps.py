"""Attention maps: where the decoder queries of a track sample, rendered onto the frame.

The reference's ``VISUALIZE`` mode dumps, per decoder layer, the reference points and the deformable-attention sampling
locations of the detect and track queries (models/deformable_decoder.py:97-136, models/ops/modules/ms_deform_attn.py:
124-126).  Here the fused operator forms softmax and locations inside its kernels and the inference decoder is replayed
from a captured graph, so that information never exists -- unless a tap is active:

    with torch.no_grad(), AttentionTap(model) as tap:
        res = model(tracks=tracks, encoded=enc)
        loc, attn = tap.points(5)             # (Lq, M, L, P, 2), (Lq, M, L, P) of batch item 0, last layer
        tap.dump("frame_1/")                  # the reference's files, torch.save

and as pictures, one annotated JPEG per frame with the heat of the tracks' sampling points blended in:

    with AttentionWriter("out/") as writer:
        for frame_idx, result in tracker.track_attention(frames_or_paths, writer, ids=[3, 7]): ...

    python -m memotr_amd.attention_maps --config-path C --model CKPT --frames DIR --out DIR [--ids 3,7] [--layers 4,5]
                                        [--dump-tensors DIR]

The picture is defined by two numpy statements below, ``attention_heat_host`` and ``blend_heat_host``: all integer past
the first float32 multiply, so the HIP kernels behind ``attention_heat`` / ``blend_heat`` (csrc/msda_attn_map.h, in
libmsda_hip.so) equal them bit for bit whatever their order of summation.  On the device a heat plane is an int64 tensor
holding the statement's uint64 bits.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .render import AnnotatedWriter

MAX_RADIUS = 8
MAX_LAYERS = 8              # per launch; more layers go in accumulating launches
MAX_PLANES = 16             # per blend
WEIGHT_ONE = 4096           # an attention weight of 1.0 in heat units
REFERENCE_DET_ROWS = 300    # the reference's dumps split detect / track rows at a literal 300 (deformable_decoder.py:99-102)


def _heat_lut() -> np.ndarray:
    v = np.arange(256, dtype=np.int64)
    ramp = np.stack([np.minimum(255, 3 * v), np.clip(3 * v - 255, 0, 255), np.clip(3 * v - 510, 0, 255)], -1)
    return ramp.astype(np.uint8)


HEAT_LUT = _heat_lut()      # (256, 3) RGB: black -> red -> yellow -> white, an integer ramp


def tent_stamp(radius: int) -> np.ndarray:
    """The (2r+1, 2r+1) uint16 outer product of [1 .. r+1 .. 1]."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"a stamp radius is an integer 0 .. {MAX_RADIUS}, got {radius!r}")
    ramp = np.concatenate([np.arange(1, radius + 2), np.arange(radius, 0, -1)]).astype(np.uint16)
    return np.outer(ramp, ramp).astype(np.uint16)


def constant_lut(colours, bgr: bool = False) -> np.ndarray:
    """(n, 256, 3) uint8 with one colour per plane at every level: the alpha alone follows the level."""
    c = np.asarray(colours, dtype=np.uint8).reshape(-1, 1, 3)
    lut = np.repeat(c, 256, 1)
    return np.ascontiguousarray(lut[..., ::-1] if bgr else lut)


def _check_stamp(stamp) -> Tuple[np.ndarray, int]:
    s = np.ascontiguousarray(np.asarray(stamp), dtype=np.uint16)
    if s.ndim != 2 or s.shape[0] != s.shape[1] or s.shape[0] % 2 != 1 or s.shape[0] > 2 * MAX_RADIUS + 1:
        raise ValueError(f"a stamp is a (2r+1, 2r+1) uint16 table with r <= {MAX_RADIUS}")
    return s, (s.shape[0] - 1) // 2


def _np(x, dtype=None) -> np.ndarray:
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def heat_weights_host(attn) -> np.ndarray:
    """int64 weights in 1/4096: 0 unless ``attn > 0`` (NaN and negatives included), else
    ``rint(min(attn, 1) * 4096)`` in float32, ties to even."""
    a = _np(attn, np.float32)
    w = np.zeros(a.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        pos = a > 0
    w[pos] = np.rint(np.minimum(a[pos], np.float32(1.0)) * np.float32(WEIGHT_ONE)).astype(np.int64)
    return w


# ------------------------------------------------------------------------------------ the two definitions
def attention_heat_host(layers, rows, planes, n_planes: int, hc: int, wc: int, sx, sy, stamp, heat=None):
    """THE DEFINITION of a heat map.  ``layers``: a list of ``(loc (Lq, M, L, P, 2), attn (Lq, M, L, P))`` float32
    arrays, one per decoder layer, each with its own ``Lq``; ``rows`` / ``planes``: int32 [K]; ``stamp``: a
    (2r+1, 2r+1) uint16 table, r <= 8; ``sx`` / ``sy``: float32 scalars from normalised padded-batch coordinates to heat
    cells.  Per entry k, per layer, per point of query row ``q = rows[k]``:

    1. the entry is skipped for the layer if ``q < 0``, ``q >= Lq``, ``planes[k] < 0`` or ``planes[k] >= n_planes``;
    2. ``x = loc_x * sx`` and ``y = loc_y * sy``, one float32 product each;
    3. the point is dropped unless ``-(r+1) <= x < wc + r + 1`` and ``-(r+1) <= y < hc + r + 1`` (NaN and +-inf drop
       here); ``ix = floor(x)``, ``iy = floor(y)``;
    4. ``wq = heat_weights_host(attn)``;
    5. for every stamp cell inside the plane ``heat[p, iy + dy, ix + dx] += wq * stamp[dy + r, dx + r]``.

    Returns ``(heat uint64 [n_planes, hc, wc], peak uint64 [n_planes])`` with ``peak[p] = max(heat[p])``.  A given
    ``heat`` is summed on top of, in place."""
    stamp, r = _check_stamp(stamp)
    rows, planes = _np(rows, np.int32).reshape(-1), _np(planes, np.int32).reshape(-1)
    if rows.shape != planes.shape:
        raise ValueError("rows and planes differ in length")
    if n_planes < 1 or hc < 1 or wc < 1:
        raise ValueError("a heat map has at least one plane and one cell")
    sx, sy = np.float32(sx), np.float32(sy)
    if heat is None:
        heat = np.zeros((n_planes, hc, wc), dtype=np.uint64)
    elif not isinstance(heat, np.ndarray) or heat.dtype != np.uint64 or heat.shape != (n_planes, hc, wc):
        raise ValueError("heat must be a uint64 array (n_planes, hc, wc)")
    stamp64 = stamp.astype(np.uint64)
    lo = np.float32(-(r + 1))
    hi_x, hi_y = np.float32(wc + r + 1), np.float32(hc + r + 1)
    for loc, attn in layers:
        loc, attn = _np(loc, np.float32), _np(attn, np.float32)
        Lq = loc.shape[0]
        for k in range(rows.shape[0]):
            q, p = int(rows[k]), int(planes[k])
            if q < 0 or q >= Lq or p < 0 or p >= n_planes:
                continue
            xy = loc[q].reshape(-1, 2)
            w = heat_weights_host(attn[q].reshape(-1))
            with np.errstate(invalid="ignore", over="ignore"):
                x, y = xy[:, 0] * sx, xy[:, 1] * sy
                ok = (x >= lo) & (x < hi_x) & (y >= lo) & (y < hi_y) & (w > 0)
            for j in np.nonzero(ok)[0]:
                ix, iy = int(math.floor(x[j])), int(math.floor(y[j]))
                y_lo, y_hi, x_lo, x_hi = max(iy - r, 0), min(iy + r, hc - 1), max(ix - r, 0), min(ix + r, wc - 1)
                if y_lo > y_hi or x_lo > x_hi:
                    continue
                heat[p, y_lo:y_hi + 1, x_lo:x_hi + 1] += np.uint64(w[j]) * stamp64[y_lo - iy + r:y_hi - iy + r + 1,
                                                                                   x_lo - ix + r:x_hi - ix + r + 1]
    return heat, heat.reshape(n_planes, -1).max(1)


def blend_heat_host(frame_u8, heat, peak, lut, cell: int, max_alpha: int, full_scale: int = 0, out=None):
    """THE DEFINITION of the overlay.  ``frame_u8`` (H, W, 3) uint8 (numpy or CPU tensor); ``heat`` uint64
    (n_planes, ceil(H / cell), ceil(W / cell)); ``peak`` uint64 (n_planes); ``lut`` uint8 (n_planes, 256, 3).  Per pixel,
    for the planes in order:

    1. ``s = full_scale or peak[p]``;
    2. ``level = 0 if s == 0 else min(255, (heat[p, y // cell, x // cell] * 255 + s // 2) // s)`` (uint64 arithmetic);
    3. ``a = (level * max_alpha + 127) // 255``;
    4. where ``a > 0``: ``px[c] = (lut[p, level, c] * a + px[c] * (255 - a) + 127) // 255`` -- ``track_draw``'s blend.

    Returns a new frame of the kind it was given, or writes ``out`` (``out=frame_u8`` blends in place)."""
    is_np = isinstance(frame_u8, np.ndarray)
    src = frame_u8 if is_np else frame_u8.numpy()
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("a frame is (H, W, 3) uint8")
    _check_blend_options(cell, max_alpha, full_scale)
    H, W = src.shape[:2]
    heat, peak, lut = _np(heat), _np(peak), _np(lut, np.uint8)
    n_planes = heat.shape[0]
    if heat.dtype != np.uint64 or heat.shape != (n_planes, -(-H // cell), -(-W // cell)):
        raise ValueError("heat must be uint64 (n_planes, ceil(H / cell), ceil(W / cell))")
    if peak.dtype != np.uint64 or peak.shape != (n_planes,) or lut.shape != (n_planes, 256, 3):
        raise ValueError("peak is uint64 (n_planes), lut uint8 (n_planes, 256, 3)")
    if out is None:
        dst = src.copy()
    else:
        dst = out if isinstance(out, np.ndarray) else out.numpy()
        if dst.shape != src.shape or dst.dtype != np.uint8:
            raise ValueError("out must have the frame's shape and dtype")
        if dst is not src and not np.shares_memory(dst, src):
            dst[...] = src
    for p in range(n_planes):
        s = np.uint64(full_scale) if full_scale else peak[p]
        if s == 0:          # level 0 everywhere: a = 127 // 255 = 0
            continue
        level = np.minimum((heat[p] * np.uint64(255) + s // np.uint64(2)) // s, np.uint64(255)).astype(np.int32)
        alpha = (level * np.int32(max_alpha) + 127) // 255
        level = np.repeat(np.repeat(level, cell, 0), cell, 1)[:H, :W]
        alpha = np.repeat(np.repeat(alpha, cell, 0), cell, 1)[:H, :W, None]
        colour = lut[p][level].astype(np.int32)
        px = dst.astype(np.int32)
        dst[...] = np.where(alpha > 0, (colour * alpha + px * (255 - alpha) + 127) // 255, px).astype(np.uint8)
    if out is not None:
        return out
    return dst if is_np else torch.from_numpy(dst)


def _check_blend_options(cell, max_alpha, full_scale) -> None:
    for name, v, lo, hi in (("cell", cell, 1, 1 << 16), ("max_alpha", max_alpha, 0, 255),
                            ("full_scale", full_scale, 0, (1 << 64) - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer {lo} .. {hi}, got {v!r}")


# ------------------------------------------------------------------------------------ the device statements
def _lib():
    from . import _lib as L         # no substitute: a missing library is an error
    return L


_CONSTANTS = {}             # (kind, bytes, device) -> the table on the device (stamps and colour tables: a handful)


def _device_constant(kind: str, array: np.ndarray, device) -> torch.Tensor:
    key = (kind, array.shape, array.tobytes(), str(device))
    t = _CONSTANTS.get(key)
    if t is None:
        if len(_CONSTANTS) > 256:
            _CONSTANTS.clear()
        raw = np.ascontiguousarray(array)
        host = torch.from_numpy(raw.view(np.int16) if raw.dtype == np.uint16 else raw)
        t = _CONSTANTS[key] = host.to(device)
    return t


def _check_table(rows, planes, device):
    for name, t in (("rows", rows), ("planes", planes)):
        if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
                and t.device == device):
            raise ValueError(f"{name} must be a contiguous int32 vector on {device}")
    if rows.shape != planes.shape:
        raise ValueError("rows and planes differ in length")


def _heat_buffers(heat, peak, n_planes, hc, wc, device, accumulate):
    if heat is None:
        if accumulate:
            raise ValueError("accumulate=True needs the heat to add to")
        heat = torch.empty((n_planes, hc, wc), dtype=torch.int64, device=device)
    elif not (torch.is_tensor(heat) and heat.dtype == torch.int64 and tuple(heat.shape) == (n_planes, hc, wc)
              and heat.is_contiguous() and heat.device == device):
        raise ValueError(f"heat must be a contiguous int64 tensor (n_planes, hc, wc) on {device}")
    if peak is None:
        peak = torch.empty((n_planes,), dtype=torch.int64, device=device)
    elif not (torch.is_tensor(peak) and peak.dtype == torch.int64 and tuple(peak.shape) == (n_planes,)
              and peak.is_contiguous() and peak.device == device):
        raise ValueError(f"peak must be a contiguous int64 tensor (n_planes) on {device}")
    return heat, peak


def _launch_heat(fused, shapes, pairs, M, L, P, rows, planes, n_planes, hc, wc, sx, sy, stamp, heat, peak, accumulate):
    Lb = _lib()
    device = rows.device
    stamp, r = _check_stamp(stamp)
    _check_table(rows, planes, device)
    with torch.cuda.device(device):
        heat, peak = _heat_buffers(heat, peak, n_planes, hc, wc, device, accumulate)
        stamp_dev = _device_constant("stamp", stamp, device)
        stream = torch.cuda.current_stream(device).cuda_stream
        sx, sy = float(np.float32(sx)), float(np.float32(sy))
        for first in range(0, max(len(pairs), 1), MAX_LAYERS):
            chunk = pairs[first:first + MAX_LAYERS]
            if not chunk:
                raise ValueError("no layers")
            desc = (Lb.HeatLayer * len(chunk))()
            for d, (a, b) in zip(desc, chunk):
                d.a, d.b, d.Lq = a.data_ptr(), b.data_ptr(), int(a.shape[0])
                d.proj_stride, d.ref_dim = (int(a.shape[1]), int(b.shape[2])) if fused else (0, 0)
            acc = 1 if (accumulate or first) else 0
            if fused:
                rc = Lb.lib.msda_attention_heat_f32(shapes.data_ptr(), desc, len(chunk), M, L, P, rows.data_ptr(),
                                                    planes.data_ptr(), int(rows.shape[0]), stamp_dev.data_ptr(), r, sx,
                                                    sy, heat.data_ptr(), peak.data_ptr(), n_planes, hc, wc, acc, stream)
            else:
                rc = Lb.lib.msda_attention_heat_points_f32(desc, len(chunk), M, L, P, rows.data_ptr(),
                                                           planes.data_ptr(), int(rows.shape[0]), stamp_dev.data_ptr(), r,
                                                           sx, sy, heat.data_ptr(), peak.data_ptr(), n_planes, hc, wc,
                                                           acc, stream)
            if rc != 0:
                raise RuntimeError(f"attention heat launch failed (code {rc}): {Lb.last_error()}")
    return heat, peak


def _as_i64_bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))


def attention_heat(layers, rows, planes, n_planes: int, hc: int, wc: int, sx, sy, stamp, *, heat=None, peak=None,
                   accumulate: bool = False):
    """``attention_heat_host`` for torch tensors: ``layers`` a list of ``(loc, attn)`` float32 tensors, ``rows`` /
    ``planes`` int32 tensors, all on one device.  Returns ``(heat, peak)`` as int64 tensors holding the uint64 bits;
    ``heat`` / ``peak`` given: reused (overwritten, or added to with ``accumulate=True``).  CUDA tensors take one kernel
    launch per 8 layers on the current stream -- nothing is allocated beyond missing outputs, nothing synchronises; CPU
    tensors take the host statement."""
    layers = list(layers)
    if not layers:
        raise ValueError("no layers")
    if not rows.is_cuda:
        given = None if heat is None else heat.numpy().view(np.uint64)
        if given is not None and not accumulate:
            given[...] = 0
        h, p = attention_heat_host([(a.numpy(), b.numpy()) for a, b in layers], rows.numpy(), planes.numpy(), n_planes,
                                   hc, wc, sx, sy, stamp, heat=given)
        heat = _as_i64_bits(h) if heat is None else heat
        if peak is None:
            return heat, _as_i64_bits(p)
        peak.copy_(_as_i64_bits(p))
        return heat, peak
    M, L, P = (int(v) for v in layers[0][0].shape[1:4])
    for loc, attn in layers:
        if not (loc.is_cuda and loc.dtype == torch.float32 and loc.is_contiguous() and attn.dtype == torch.float32
                and attn.is_contiguous() and loc.dim() == 5 and tuple(loc.shape[1:]) == (M, L, P, 2)
                and tuple(attn.shape) == tuple(loc.shape[:4]) and loc.device == rows.device == attn.device):
            raise ValueError("a layer is (loc (Lq, M, L, P, 2), attn (Lq, M, L, P)): contiguous float32 on one device")
    return _launch_heat(False, None, layers, M, L, P, rows, planes, n_planes, hc, wc, sx, sy, stamp, heat, peak,
                        accumulate)


def attention_heat_fused(spatial_shapes, layers, n_heads: int, n_points: int, rows, planes, n_planes: int, hc: int,
                         wc: int, sx, sy, stamp, *, heat=None, peak=None, accumulate: bool = False):
    """``attention_heat`` from what the decoder's cross-attention is given instead of materialised points: ``layers`` a
    list of ``(proj (Lq, >= 3*M*L*P), ref (Lq, L, 2|4))`` CUDA float32 tensors of batch item 0.  The kernel forms the
    points with the fused operator's own arithmetic; they never reach memory.  By definition the result is that of
    ``attention_heat`` on ``MultiScaleDeformableAttention.fused_points`` of the same arguments."""
    layers = list(layers)
    M, P, L = int(n_heads), int(n_points), int(spatial_shapes.shape[0])
    for proj, ref in layers:
        if not (proj.is_cuda and proj.dtype == torch.float32 and proj.is_contiguous() and proj.dim() == 2
                and ref.dtype == torch.float32 and ref.is_contiguous() and ref.dim() == 3 and ref.shape[1] == L
                and ref.shape[0] == proj.shape[0] and proj.device == ref.device == rows.device):
            raise ValueError("a fused layer is (proj (Lq, width), ref (Lq, L, 2|4)): contiguous float32 CUDA tensors")
    if not (spatial_shapes.is_cuda and spatial_shapes.dtype == torch.int64 and spatial_shapes.is_contiguous()):
        raise ValueError("spatial_shapes must be a contiguous int64 CUDA tensor (L, 2)")
    return _launch_heat(True, spatial_shapes, layers, M, L, P, rows, planes, n_planes, hc, wc, sx, sy, stamp, heat,
                        peak, accumulate)


def blend_heat(frame_u8, heat, peak, lut=None, *, cell: int = 4, max_alpha: int = 160, full_scale: int = 0, out=None,
               bgr: bool = False):
    """``blend_heat_host`` for torch tensors.  ``lut``: (n_planes, 256, 3) or (256, 3) uint8 in RGB, numpy or tensor
    (default ``HEAT_LUT`` for every plane); ``bgr``: the frame's channel order is BGR, the table is flipped.  A CUDA
    frame (rows may be pitched) takes one launch on the current stream, ``heat`` / ``peak`` being the int64 tensors of
    ``attention_heat``; a CPU frame the host statement.  ``out=frame_u8`` blends in place."""
    n_planes = int(heat.shape[0])
    table = _np(HEAT_LUT if lut is None else lut, np.uint8)
    if table.ndim == 2:
        table = np.repeat(table[None], n_planes, 0)
    if table.shape != (n_planes, 256, 3):
        raise ValueError("lut must be uint8 (n_planes, 256, 3) or (256, 3)")
    table = np.ascontiguousarray(table[..., ::-1] if bgr else table)
    if not torch.is_tensor(frame_u8) or not frame_u8.is_cuda:
        h = _np(heat)
        p = _np(peak)
        return blend_heat_host(frame_u8, h.view(np.uint64) if h.dtype == np.int64 else h,
                               p.view(np.uint64) if p.dtype == np.int64 else p, table, cell, max_alpha, full_scale, out)
    from .render import _check_device_frame
    _check_blend_options(cell, max_alpha, full_scale)
    if frame_u8.dim() != 3 or frame_u8.shape[2] != 3 or not 1 <= n_planes <= MAX_PLANES:
        raise ValueError(f"a frame is (H, W, 3) uint8; 1 .. {MAX_PLANES} planes per blend")
    H, W, _ = frame_u8.shape
    device = frame_u8.device
    _check_device_frame(frame_u8, "frame_u8")
    if not (heat.dtype == torch.int64 and heat.is_contiguous() and heat.device == device
            and tuple(heat.shape) == (n_planes, -(-H // cell), -(-W // cell))
            and peak.dtype == torch.int64 and peak.is_contiguous() and tuple(peak.shape) == (n_planes,)
            and peak.device == device):
        raise ValueError("heat is int64 (n_planes, ceil(H / cell), ceil(W / cell)), peak int64 (n_planes), on the "
                         "frame's device")
    Lb = _lib()
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
        elif not torch.is_tensor(out) or tuple(out.shape) != (H, W, 3) or out.device != device:
            raise ValueError(f"out must be a (H, W, 3) uint8 tensor on {device}")
        else:
            _check_device_frame(out, "out")
        lut_dev = _device_constant("lut", table, device)
        pitch = lambda t: t.stride(0) if H > 1 else 3 * W  # noqa: E731
        rc = Lb.lib.msda_attention_blend_u8(frame_u8.data_ptr(), pitch(frame_u8), out.data_ptr(), pitch(out), W, H,
                                            heat.data_ptr(), peak.data_ptr(), lut_dev.data_ptr(), n_planes, int(cell),
                                            int(max_alpha), int(full_scale),
                                            torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"msda_attention_blend_u8 failed (code {rc}): {Lb.last_error()}")
    return out


# ------------------------------------------------------------------------------------ the tap
class AttentionTap:
    """Context manager that records what the decoder's cross-attention of every layer is given.  Inference only: it
    raises if grad is enabled.

    While it is active ``DeformableDecoder.forward`` skips both graphed branches and runs its eager loop, so results
    under the tap are those of ``MEMOTR_INFER_GRAPHS=0`` (the graphs' results to rounding, not to the bit).  Per layer
    ``lid`` the tap keeps, on the device and without a synchronisation, of the LAST decoder call:

    * ``reference(lid)``: the un-scaled reference points (N, Nq, 4|2) the loop holds;
    * ``cross_reference(lid)``: the cross-attention's ``reference_points`` input (N, Lq_l, L, 2|4), times the valid ratios;
    * ``projection(lid)``: the raw query projection (N, Lq_l, 3*M*L*P) -- ``long_linear(query,
      *cross_attn._fused_query_projection())``, the GEMM the module itself runs.

    Layers below ``merge_det_track_layer`` see the ``n_det_queries`` detect rows only; ``Lq_l`` is recorded as it is.

    ``points(lid)`` -> ``(loc (Lq_l, M, L, P, 2), attn (Lq_l, M, L, P))`` of batch item 0: on CUDA the fused kernels'
    own bits (``MultiScaleDeformableAttention.fused_points``), on CPU -- and for ``sigmoid_attn`` modules on both -- the
    module's unfused torch statement.

    ``dump(dir)`` writes the reference's files with ``torch.save``, with its shapes and slicing (rows split at a literal
    300): ``sampling_locations_layer_{lid}.tensor``, ``detection_ref_pts_layer_{lid}.tensor``,
    ``track_ref_pts_layer_{lid}.tensor``, and ``attention_weights_layer_{lid}.tensor``, which has no reference
    counterpart.  The reference's ``attn_score_layer_{lid}.tensor`` is left out: it is the decoder SELF-attention score
    matrix, which the fused self-attention here never forms."""

    def __init__(self, model):
        from .models.utils import get_model
        core = get_model(model)
        self.decoder = core.transformer.decoder if hasattr(core, "transformer") else core
        self._hooks = []
        self._ref, self._cross, self._proj, self._shapes = {}, {}, {}, None

    @property
    def layers(self) -> List[int]:
        return sorted(self._proj)

    def __enter__(self):
        if torch.is_grad_enabled():
            raise RuntimeError("AttentionTap is for inference: enter it under torch.no_grad()")
        if self.decoder.__dict__.get("_attention_tap") is not None:
            raise RuntimeError("this decoder already has an active AttentionTap")
        self.decoder.__dict__["_attention_tap"] = self
        for lid, layer in enumerate(self.decoder.layers):
            self._hooks.append(layer.cross_attn.register_forward_pre_hook(
                lambda module, args, lid=lid: self._record_cross(lid, module, args)))
        return self

    def __exit__(self, exc_type, exc, tb):
        for h in self._hooks:
            h.remove()
        self._hooks = []
        self.decoder.__dict__.pop("_attention_tap", None)
        return False

    def record_reference(self, lid: int, reference_points: torch.Tensor) -> None:
        """Called by the decoder's eager loop in front of layer ``lid``."""
        if torch.is_grad_enabled():
            raise RuntimeError("AttentionTap is for inference: the decoder ran with grad enabled")
        if lid == 0:
            self._ref, self._cross, self._proj = {}, {}, {}
        self._ref[lid] = reference_points

    def _record_cross(self, lid: int, module, args) -> None:
        from .modules.linear import long_linear
        query, reference_points, spatial_shapes = args[0], args[1], args[3]
        self._cross[lid] = reference_points
        self._proj[lid] = long_linear(query, *module._fused_query_projection())
        self._shapes = spatial_shapes

    def reference(self, lid: int) -> torch.Tensor:
        return self._ref[lid]

    def cross_reference(self, lid: int) -> torch.Tensor:
        return self._cross[lid]

    def projection(self, lid: int) -> torch.Tensor:
        return self._proj[lid]

    @property
    def spatial_shapes(self) -> torch.Tensor:
        return self._shapes

    def module(self, lid: int):
        return self.decoder.layers[lid].cross_attn

    def fusable(self, lid: int) -> bool:
        """The fused kernels' arithmetic applies to layer ``lid``'s record (CUDA float32, softmax weights)."""
        proj, mod = self._proj[lid], self.module(lid)
        return bool(proj.is_cuda and proj.dtype == torch.float32 and not mod.sigmoid_attn
                    and mod.n_levels * mod.n_points <= 64)

    def points(self, lid: int):
        mod = self.module(lid)
        proj, ref = self._proj[lid][:1].float(), self._cross[lid][:1].float()
        M, L, P = mod.n_heads, mod.n_levels, mod.n_points
        if self.fusable(lid):
            from . import MultiScaleDeformableAttention as MSDA
            loc, attn = MSDA.fused_points(self._shapes, proj.contiguous(), ref.contiguous(), M, P)
            return loc[0], attn[0]
        n_off = M * L * P * 2
        Lq = proj.shape[1]
        offsets = proj[..., :n_off].unflatten(-1, (M, L, P, 2))
        logits = proj[..., n_off:n_off + M * L * P].unflatten(-1, (M, L * P))
        attn = logits.sigmoid() if mod.sigmoid_attn else torch.softmax(logits, -1)
        attn = attn.view(1, Lq, M, L, P)
        if ref.shape[-1] == 2:
            wh = self._shapes.flip(-1).to(offsets.dtype)
            loc = ref[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
        else:
            loc = ref[:, :, None, :, None, :2] + offsets / P * ref[:, :, None, :, None, 2:] * 0.5
        return loc[0].contiguous(), attn[0].contiguous()

    def dump(self, directory) -> List[str]:
        os.makedirs(directory, exist_ok=True)
        written = []

        def save(t, name):
            path = os.path.join(os.fspath(directory), name)
            torch.save(t.detach().cpu(), path)
            written.append(path)

        for lid in self.layers:
            loc, attn = self.points(lid)
            save(loc, f"sampling_locations_layer_{lid}.tensor")
            save(attn, f"attention_weights_layer_{lid}.tensor")
            ref = self._ref[lid]
            save(ref[0, :REFERENCE_DET_ROWS, :], f"detection_ref_pts_layer_{lid}.tensor")
            save(ref[0, REFERENCE_DET_ROWS:, :], f"track_ref_pts_layer_{lid}.tensor")
        return written


# ------------------------------------------------------------------------------------ rows of a frame, its heat
def frame_rows(ids_before: torch.Tensor, newborn_rows: torch.Tensor, newborn_first_id: int, n_det: int,
               ids: Optional[Sequence[int]] = None):
    """The (query row, plane) table of a frame, built on the device with torch ops, nothing read back.  Row
    ``n_det + j`` is the track ``ids_before[j]`` that entered the frame, row ``newborn_rows[k]`` the newborn
    ``newborn_first_id + k``.  ``ids=None``: every live track (id >= 0) and every newborn into plane 0; ``ids=[...]``:
    plane k is track ``ids[k]`` (a list, or a long tensor made once), other rows get plane -1.  Returns int32 ``(rows, planes)``."""
    device = ids_before.device
    ids_before = ids_before.long()
    n_tr, n_new = int(ids_before.shape[0]), int(newborn_rows.shape[0])
    rows = torch.cat((torch.arange(n_det, n_det + n_tr, device=device), newborn_rows.long().to(device)))
    all_ids = torch.cat((ids_before, torch.arange(newborn_first_id, newborn_first_id + n_new, device=device)))
    if ids is None:
        planes = torch.where(all_ids >= 0, torch.zeros_like(all_ids), torch.full_like(all_ids, -1))
    else:
        want = ids.to(device) if torch.is_tensor(ids) else torch.as_tensor(list(ids), dtype=torch.long, device=device)
        hit = all_ids[:, None] == want[None, :]
        planes = torch.where(hit.any(1), hit.int().argmax(1), torch.full_like(all_ids, -1))
    return rows.to(torch.int32).contiguous(), planes.to(torch.int32).contiguous()


def heat_scale(padded: int, original: int, resized: int, cell: int) -> np.float32:
    """Normalised padded-batch coordinate -> heat cell of the original frame: ``padded * original / resized / cell`` in
    double, rounded to float32 once."""
    return np.float32(float(padded) * float(original) / float(resized) / float(cell))


def tap_heat(tap: AttentionTap, layers: Sequence[int], rows, planes, n_planes: int, hc: int, wc: int, sx, sy, stamp, *,
             heat=None, peak=None):
    """The heat of the tap's last decoder call over ``layers``: the fused entry where the fused kernels' arithmetic
    applies (the points never reach memory), else ``attention_heat`` on ``tap.points``."""
    layers = list(layers)
    if layers and all(tap.fusable(lid) for lid in layers):
        mod = tap.module(layers[0])
        pairs = [(tap.projection(lid)[0].contiguous(), tap.cross_reference(lid)[0].contiguous()) for lid in layers]
        return attention_heat_fused(tap.spatial_shapes, pairs, mod.n_heads, mod.n_points, rows, planes, n_planes, hc,
                                    wc, sx, sy, stamp, heat=heat, peak=peak)
    return attention_heat([tap.points(lid) for lid in layers], rows, planes, n_planes, hc, wc, sx, sy, stamp,
                          heat=heat, peak=peak)


# ------------------------------------------------------------------------------------ the writer
class AttentionWriter(AnnotatedWriter):
    """``render.AnnotatedWriter`` with the attention heat under the boxes: ``add_attention`` blends the planes into a
    frame copy of its own on the current stream, then hands that to ``AnnotatedWriter.add``, which draws boxes and ids
    and encodes on the writer's side stream.  The blend buffers rotate, and a buffer is blended into again only behind
    the event of the side stream's last read of it.  A CPU frame goes through the host statements on the worker thread.

    ``cell``: frame pixels per heat cell; ``radius``: of the tent stamp; ``max_alpha``: opacity at the hottest cell;
    ``full_scale``: heat value of level 255 (0: each plane's own peak)."""

    BLEND_SLOTS = 2

    def __init__(self, out, quality: int = 85, cell: int = 4, radius: int = 2, max_alpha: int = 160,
                 full_scale: int = 0, **annotated_options):
        _check_blend_options(cell, max_alpha, full_scale)
        self.stamp = tent_stamp(radius)
        self.cell, self.radius, self.max_alpha, self.full_scale = cell, radius, max_alpha, full_scale
        super().__init__(out, quality=quality, **annotated_options)
        self._blend = [[None, None] for _ in range(self.BLEND_SLOTS)]      # [buffer, event of its last read]
        self._bi = 0

    def add_attention(self, frame_idx: int, frame_u8, result, heat, peak, lut=None, *, bgr: Optional[bool] = None):
        if self._closed:
            raise RuntimeError("add_attention() on a closed AttentionWriter")
        bgr = self.bgr if bgr is None else bool(bgr)
        if not torch.is_tensor(frame_u8):
            frame_u8 = torch.from_numpy(frame_u8)
        if not frame_u8.is_cuda:
            from .data import jpeg_write as JW
            from .render import _ids_boxes, draw_tracks_host
            ids, boxes = _ids_boxes(result, None) if not isinstance(result, (tuple, list)) else _ids_boxes(*result)
            table = None if lut is None else _np(lut, np.uint8).copy()

            def on_host(frame=frame_u8.clone(), heat=_np(heat).copy(), peak=_np(peak).copy()):
                blend_heat(frame, heat, peak, table, cell=self.cell, max_alpha=self.max_alpha,
                           full_scale=self.full_scale, out=frame, bgr=bgr)
                drawn = draw_tracks_host(frame, ids, boxes, bgr=bgr, out=frame, **self.draw_options)
                self._sink(frame_idx, JW.encode_jpeg(drawn, self.quality, self.subsampling, bgr))
            self._jobs.append(self._pool.submit(self._run, on_host))
            return
        device = frame_u8.device
        slot = self._blend[self._bi]
        self._bi = (self._bi + 1) % self.BLEND_SLOTS
        with torch.cuda.device(device):
            if slot[0] is None or slot[0].shape != frame_u8.shape or slot[0].device != device:
                slot[0], slot[1] = torch.empty(tuple(frame_u8.shape), dtype=torch.uint8, device=device), None
            if slot[1] is not None:
                torch.cuda.current_stream(device).wait_event(slot[1])
            blend_heat(frame_u8, heat, peak, lut, cell=self.cell, max_alpha=self.max_alpha,
                       full_scale=self.full_scale, out=slot[0], bgr=bgr)
            self.add(frame_idx, slot[0], result, bgr=bgr)
            slot[1] = self._stream.record_event()


# ------------------------------------------------------------------------------------ command line
def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m memotr_amd.attention_maps",
                                 description="Track a folder of frames and write one JPEG per frame with the tracks' "
                                             "boxes over the heat of their decoder queries' sampling points.")
    ap.add_argument("--config-path", required=True, help="a built-in config name or a YAML file")
    ap.add_argument("--model", required=True, help="checkpoint with a 'model' state dict")
    ap.add_argument("--frames", required=True, help="directory of jpg / png frames, tracked in sorted order")
    ap.add_argument("--out", required=True, help="receives one annotated JPEG per frame")
    ap.add_argument("--ids", default=None, help="comma-separated track ids, one tinted plane each (at most 16); "
                                                "default: every track in one heat plane")
    ap.add_argument("--layers", default=None, help="comma-separated decoder layers that count; default: all")
    ap.add_argument("--dump-tensors", default=None, help="also write the reference's VISUALIZE tensors per frame here")
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--cell", type=int, default=4)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--max-alpha", type=int, default=160)
    ap.add_argument("--device", default=None, help="default: cuda when there is one")
    args = ap.parse_args(argv)

    from .inference import SequenceTracker
    from .main import load_config
    from .submit import _source, load_model
    config = load_config(args.config_path)
    device = torch.device(args.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    model = load_model(config, args.model).to(device).eval()
    tracker = SequenceTracker.from_config(model, config)
    paths = [os.path.join(args.frames, n) for n in sorted(os.listdir(args.frames)) if "jpg" in n or "png" in n]
    if not paths:
        raise SystemExit(f"no jpg / png frames in {args.frames}")
    ids = None if args.ids is None else [int(v) for v in args.ids.split(",") if v != ""]
    layers = None if args.layers is None else [int(v) for v in args.layers.split(",") if v != ""]
    with AttentionWriter(args.out, quality=args.quality, cell=args.cell, radius=args.radius,
                         max_alpha=args.max_alpha) as writer:
        for frame_idx, _ in tracker.track_attention(_source(paths), writer, ids=ids, layers=layers):
            if args.dump_tensors is not None:
                tracker.attention_tap.dump(os.path.join(args.dump_tensors, f"frame_{frame_idx + 1}"))
    print(f"{len(paths)} frames -> {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
