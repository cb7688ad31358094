"""Tracking evaluation for BDD100K: HOTA, CLEAR, Identity and Count for the 8 evaluated classes, with crowd-ignore
regions, the per-class combination over sequences and the combination over classes -- what the reference gets from
TrackEval's ``datasets/bdd100k.py`` and ``eval.py`` (``cls_comb_cls_av``, ``cls_comb_det_av``, HUMAN / VEHICLE / BIKE).

    ev = BDD100KEvaluator(device="cuda")
    ev.add_ground_truth("b1c66a42", frame_idx, ids, boxes_xyxy, categories, crowd)     # frame_idx: 0-based
    for frame_idx, result in tracker.track(frames):                  # what SequenceTracker.step / step_raw returns
        ev.add_frame("b1c66a42", frame_idx, result)                  # ids, labels, boxes
    res = ev.evaluate()                            # {"b1c66a42": {"car": {...}, ...}, "COMBINED_SEQ": {"car": ..., "cls_comb_det_av": ...}}
    print(bdd_summary(res)["cls_comb_det_av"])     # names / values of cls_comb_det_av_summary.txt

BDD100K's rules (``BDD100K.get_preprocessed_seq_data``): every class is evaluated on its own; per frame and class the
detections are matched to the ground truth (similarity below 0.5 - eps counts as 0), and an UNMATCHED detection whose
intersection with a crowd-ignore region of the frame covers more than 0.5 + eps of its own area is dropped; nothing is
removed from the ground truth.  Ground-truth rows of the categories ``other person``, ``trailer``, ``other vehicle``
or with the ``Crowd`` attribute are the frame's ignore regions.

A (sequence, class) pair is one "sequence" of ``evaluation.py``: ``host_tables_bdd`` / ``device_tables_bdd`` return
the dictionary of ``host_tables`` with S * 8 rows, ``p = s * 8 + c``, the frames of a pair consecutive (F * 8 frames in
all), and ``evaluation._sequence_result`` / ``combine_sequences`` make the fields.  A detection id the tracker labels
``car`` in one frame and ``truck`` in the next belongs to both classes' problems, relabelled in each.

As in ``evaluation.py`` the definition is stated twice: on the host (numpy, scipy; the default wherever the inputs
live) and on the GPU (memotr_amd/csrc/track_eval_bdd.hip in front of the metric kernels of track_eval.hip), which runs
where a CUDA ``device`` is asked for (``device_front_bdd``, which ``diagnose_bdd100k`` stands on too); a missing library
raises then.  ``tools/bench_eval_bdd.py`` measures both on a synthetic set of BDD100K-val size (200 sequences x 200
frames x 8 classes): on an MI355X the device path took 86 ms from the call to the fields (3 ms of it in the ten library
calls), the host statement 61 s on one core (profiles/track_eval_bdd.md).  No threshold follows from that number; the
host statement stays the default.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from . import evaluation as E
from .evaluation import ALPHAS, EPS, THRESHOLD, _host_array

CLASSES = ("pedestrian", "rider", "car", "bus", "truck", "train", "motorcycle", "bicycle")   # TrackEval's order
CLASS_NAME_TO_CLASS_ID = {"pedestrian": 1, "rider": 2, "other person": 3, "car": 4, "bus": 5, "truck": 6, "train": 7,
                          "trailer": 8, "other vehicle": 9, "motorcycle": 10, "bicycle": 11}
DISTRACTOR_CATEGORIES = ("other person", "trailer", "other vehicle")
SUPER_CATEGORIES = {"HUMAN": ("pedestrian", "rider"), "VEHICLE": ("car", "truck", "bus", "train"),
                    "BIKE": ("motorcycle", "bicycle")}
COMBINED_KEYS = ("cls_comb_cls_av", "cls_comb_det_av") + tuple(SUPER_CATEGORIES)
N_CLASSES = len(CLASSES)
CLASS_IDS = tuple(CLASS_NAME_TO_CLASS_ID[c] for c in CLASSES)                # (1, 2, 4, 5, 6, 7, 10, 11)
IGNORE_THRESHOLD = 0.5


def __getattr__(name):
    """``LABEL_TO_CATEGORY`` and ``LABEL_TO_CLASS_ID``: the model's label index k (argmax over 8 logits) -> category
    (``inference.BDD_CLS2LABEL[k + 1]``) -> TrackEval's class id.  The model's order has truck before bus, TrackEval's
    ids have bus before truck.  Formed on first use: ``inference`` loads the model's libraries, which scoring result
    files does not need."""
    if name not in ("LABEL_TO_CATEGORY", "LABEL_TO_CLASS_ID"):
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    from .inference import BDD_CLS2LABEL
    g = globals()
    g["LABEL_TO_CATEGORY"] = tuple(BDD_CLS2LABEL[k + 1] for k in range(N_CLASSES))
    g["LABEL_TO_CLASS_ID"] = tuple(CLASS_NAME_TO_CLASS_ID[n] for n in g["LABEL_TO_CATEGORY"])
    return g[name]


HOTA_FLOAT_FIELDS = E.HOTA_FLOATS + E.HOTA_FLOAT_ARRAYS
# clear.py: integer_fields are summed over classes, float_fields (MOTP_sum among them) averaged
CLEAR_CLASS_SUMMED, CLEAR_CLASS_AVERAGED = E.CLEAR_INTS, E.CLEAR_FLOATS


# ------------------------------------------------------------------------------------------------------- the input
@dataclass
class PackedBDD:
    """All sequences of one call as ragged arrays (include/track_eval_bdd_hip.h): numpy, or torch tensors on one
    device.  Frames of a sequence are consecutive; boxes are float64 x0, y0, x1, y1; ids and classes (TrackEval's
    class ids) are int32; ``ig_boxes[ig_off[f]:ig_off[f + 1]]`` are the crowd-ignore regions of frame f."""
    names: List[str]
    seq_off: object             # int32 [S + 1]
    gt_off: object              # int32 [F + 1]
    tr_off: object              # int32 [F + 1]
    ig_off: object              # int32 [F + 1]
    gt_boxes: object            # float64 [NG, 4]
    tr_boxes: object            # float64 [NT, 4]
    ig_boxes: object            # float64 [NI, 4]
    gt_ids: object              # int32 [NG]
    tr_ids: object              # int32 [NT]
    gt_classes: object          # int32 [NG]
    tr_classes: object          # int32 [NT]

    ARRAYS = ("seq_off", "gt_off", "tr_off", "ig_off", "gt_boxes", "tr_boxes", "ig_boxes", "gt_ids", "tr_ids",
              "gt_classes", "tr_classes")

    def is_device(self) -> bool:
        return not isinstance(self.gt_boxes, np.ndarray) and self.gt_boxes.is_cuda

    def numpy(self) -> "PackedBDD":
        if isinstance(self.gt_boxes, np.ndarray):
            return self
        return PackedBDD(self.names, *[getattr(self, k).cpu().numpy() for k in self.ARRAYS])

    def to(self, device) -> "PackedBDD":
        import torch
        return PackedBDD(self.names, *[torch.as_tensor(getattr(self, k)).to(device) for k in self.ARRAYS])

    def select(self, index: int) -> "PackedBDD":
        """Sequence ``index`` alone (host arrays)."""
        p = self.numpy()
        f0, f1 = int(p.seq_off[index]), int(p.seq_off[index + 1])
        g0, g1, t0, t1 = int(p.gt_off[f0]), int(p.gt_off[f1]), int(p.tr_off[f0]), int(p.tr_off[f1])
        i0, i1 = int(p.ig_off[f0]), int(p.ig_off[f1])
        return PackedBDD([p.names[index]], np.array([0, f1 - f0], np.int32), p.gt_off[f0:f1 + 1] - g0,
                         p.tr_off[f0:f1 + 1] - t0, p.ig_off[f0:f1 + 1] - i0, p.gt_boxes[g0:g1], p.tr_boxes[t0:t1],
                         p.ig_boxes[i0:i1], p.gt_ids[g0:g1], p.tr_ids[t0:t1], p.gt_classes[g0:g1],
                         p.tr_classes[t0:t1])


def pack_bdd(sequences: Dict[str, dict]) -> PackedBDD:
    """``{name: {"gt_ids", "gt_boxes", "gt_classes", "tracker_ids", "tracker_boxes", "tracker_classes",
    "ignore_regions"}}`` -- every value a list with one array per frame (ids and classes ``(n,)``, boxes and regions
    ``(n, 4)`` x0y0x1y1; ``ignore_regions`` may be left out) -- as host ``PackedBDD``.  An id may occur once per frame
    and class (what TrackEval's ``_check_unique_ids`` sees after the class split) and lies in [0, 2**31)."""
    names, seq_off, n = [], [0], {"gt": [], "tr": [], "ig": []}
    cols = {k: [] for k in ("gt_boxes", "tr_boxes", "ig_boxes", "gt_ids", "tr_ids", "gt_classes", "tr_classes")}
    for name, seq in sequences.items():
        T = len(seq["gt_ids"])
        lists = [seq[k] for k in ("gt_boxes", "gt_classes", "tracker_ids", "tracker_boxes", "tracker_classes")]
        if seq.get("ignore_regions") is not None:
            lists.append(seq["ignore_regions"])
        if any(len(x) != T for x in lists):
            raise ValueError(f"sequence {name}: the per-frame lists differ in length")
        names.append(name)
        seq_off.append(seq_off[-1] + T)
        for t in range(T):
            rows = {}
            for side, key in (("gt", "gt"), ("tr", "tracker")):
                ids = _host_array(seq[key + "_ids"][t], np.int64).reshape(-1)
                boxes = _host_array(seq[key + "_boxes"][t], np.float64).reshape(-1, 4)
                classes = _host_array(seq[key + "_classes"][t], np.int64).reshape(-1)
                which = "ground-truth" if side == "gt" else "tracker"
                if len(boxes) != len(ids) or len(classes) != len(ids):
                    raise ValueError(f"sequence {name}, frame {t}: {which} ids, boxes and classes differ in length")
                if len(ids) and (ids.min() < 0 or ids.max() >= 2 ** 31):
                    raise ValueError(f"sequence {name}, frame {t}: a {which} id is outside [0, 2**31)")
                for c, cls_id in enumerate(CLASS_IDS):
                    mine = ids[classes == cls_id]
                    if len(np.unique(mine)) != len(mine):
                        raise ValueError(f"sequence {name}, frame {t}: a {which} id occurs more than once in class "
                                         f"{CLASSES[c]}")
                rows[side] = ids, boxes, classes
            regions = np.zeros((0, 4)) if seq.get("ignore_regions") is None else \
                _host_array(seq["ignore_regions"][t], np.float64).reshape(-1, 4)
            for side in ("gt", "tr"):
                n[side].append(len(rows[side][0]))
                cols[side + "_ids"].append(rows[side][0].astype(np.int32))
                cols[side + "_boxes"].append(rows[side][1])
                cols[side + "_classes"].append(rows[side][2].astype(np.int32))
            n["ig"].append(len(regions))
            cols["ig_boxes"].append(regions)

    def cat(key, shape, dtype):
        return np.concatenate(cols[key]).astype(dtype) if cols[key] else np.zeros(shape, dtype)

    off = lambda x: np.concatenate(([0], np.cumsum(x))).astype(np.int32)      # noqa: E731
    return PackedBDD(names, np.asarray(seq_off, np.int32), off(n["gt"]), off(n["tr"]), off(n["ig"]),
                     cat("gt_boxes", (0, 4), np.float64), cat("tr_boxes", (0, 4), np.float64),
                     cat("ig_boxes", (0, 4), np.float64), cat("gt_ids", (0,), np.int32), cat("tr_ids", (0,), np.int32),
                     cat("gt_classes", (0,), np.int32), cat("tr_classes", (0,), np.int32))


# --------------------------------------------------------------------------------- the definition, on the host
def _intersection(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    w = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    h = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    return np.maximum(w, 0) * np.maximum(h, 0)


def box_iou_x0y0x1y1(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """IoU of every box of ``a`` (n, 4) with every box of ``b`` (m, 4), corners x0, y0, x1, y1, float64, in the
    operation order of TrackEval's ``_calculate_box_ious(box_format='x0y0x1y1')``: areas from the corners directly,
    union = area + area - intersection; a box or a union without area gives 0."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    inter = _intersection(a, b)
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = area_a[:, None] + area_b[None, :] - inter
    dead = (area_a <= EPS)[:, None] | (area_b <= EPS)[None, :] | (union <= EPS)
    inter = np.where(dead, 0.0, inter)
    union = np.where(union <= EPS, 1.0, union)
    return inter / union


def box_ioa_x0y0x1y1(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Intersection of every box of ``a`` with every box of ``b`` over the area of the box of ``a`` (the FIRST
    argument); 0 where that area is <= eps."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    inter = _intersection(a, b)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    out = np.zeros_like(inter)
    np.divide(inter, area_a[:, None], out=out, where=(area_a > EPS)[:, None])
    return out


def _split_offsets(seq_off):
    """Frame offsets of the S * 8 problems (``p = s * 8 + c`` owns T_s consecutive frames) and, per problem-major
    frame, the packed frame it was cut from."""
    T = np.diff(seq_off).astype(np.int64)
    split_seq_off = np.concatenate(([0], np.cumsum(np.repeat(T, N_CLASSES)))).astype(np.int32)
    src = np.concatenate([np.tile(np.arange(seq_off[s], seq_off[s + 1]), N_CLASSES) for s in range(len(T))] +
                         [np.zeros(0, np.int64)]).astype(np.int32)
    return split_seq_off, src


def class_split_host(p: PackedBDD) -> dict:
    """The problem-major layout: per (sequence, class) the frames of the sequence with the class's detections, in
    their original order.  ``gt_src`` / ``tr_src``: the packed row of every detection."""
    seq_off, src = _split_offsets(p.seq_off)
    cls = np.repeat(np.tile(np.arange(N_CLASSES), len(p.names)), np.repeat(np.diff(p.seq_off), N_CLASSES))
    out = {"seq_off": seq_off, "frame_src": src}
    for side in ("gt", "tr"):
        off, classes = getattr(p, side + "_off"), getattr(p, side + "_classes")
        rows = [off[f] + np.flatnonzero(classes[off[f]:off[f + 1]] == CLASS_IDS[c]) for f, c in zip(src, cls)]
        take = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
        out[side + "_off"] = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
        out[side + "_src"] = take
        out[side + "_boxes"], out[side + "_ids"] = getattr(p, side + "_boxes")[take], getattr(p, side + "_ids")[take]
    return out


def _as_sequences(names, d) -> E.PackedSequences:
    """What ``evaluation._compact`` reads of a class split: offsets and ids."""
    return E.PackedSequences([f"{n}/{c}" for n in names for c in CLASSES], d["seq_off"], d["gt_off"], d["tr_off"],
                             None, None, d["gt_ids"], d["tr_ids"], None, None)


def _preprocess_host(p: PackedBDD):
    d = class_split_host(p)
    F8 = len(d["gt_off"]) - 1
    raw_sim, sims, keep_tr = [], [], np.ones(len(d["tr_ids"]), bool)
    for q in range(F8):
        g0, g1, t0, t1 = d["gt_off"][q], d["gt_off"][q + 1], d["tr_off"][q], d["tr_off"][q + 1]
        sim = box_iou_x0y0x1y1(d["gt_boxes"][g0:g1], d["tr_boxes"][t0:t1])
        raw_sim.append(sim.reshape(-1))
        unmatched = np.ones(t1 - t0, bool)
        if g1 > g0 and t1 > t0:
            score = np.where(sim < THRESHOLD - EPS, 0.0, sim)
            rows, cols = E._assign(-score)
            unmatched[cols[score[rows, cols] > EPS]] = False
        f = d["frame_src"][q]
        ioa = box_ioa_x0y0x1y1(d["tr_boxes"][t0:t1], p.ig_boxes[p.ig_off[f]:p.ig_off[f + 1]])
        keep_tr[t0:t1] = ~(unmatched & np.any(ioa > IGNORE_THRESHOLD + EPS, axis=1))
        sims.append(sim[:, keep_tr[t0:t1]].reshape(-1))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)            # noqa: E731
    return cat(raw_sim), cat(sims), E._compact(_as_sequences(p.names, d), np.ones(len(d["gt_ids"]), bool), keep_tr)


TABLE_KEYS = ("gt_off", "tr_off", "gt_ids", "tr_ids", "n_gt_ids", "n_tr_ids", "n_gt_dets", "n_tr_dets")


def host_tables_bdd(packed: PackedBDD) -> dict:
    """The whole definition on the host: ``evaluation.host_tables``' dictionary with one row per (sequence, class),
    ``p = s * 8 + c``; ``raw_similarity`` and ``similarity`` are those of the problem-major frames, concatenated."""
    p = packed.numpy()
    raw_sim, sim, d = _preprocess_host(p)
    P = len(p.names) * N_CLASSES
    out = {"raw_similarity": raw_sim, "similarity": sim, "hota_tp": np.zeros((P, len(ALPHAS)), np.int64),
           "hota_sums": np.zeros((P, 4, len(ALPHAS))), "clear_ints": np.zeros((P, 8), np.int64),
           "motp_sum": np.zeros(P), "identity": np.zeros((P, 2), np.int64)}
    out.update({k: d[k] for k in TABLE_KEYS})
    for s in range(P):
        G, K = int(d["n_gt_ids"][s]), int(d["n_tr_ids"][s])
        if d["n_gt_dets"][s] == 0 or d["n_tr_dets"][s] == 0:
            continue                    # (an empty side: the fields are fixed by the counts, _sequence_result)
        frames = list(E._frames_of(d, sim, s))
        out["hota_tp"][s], out["hota_sums"][s] = E._hota_host(frames, G, K)
        out["clear_ints"][s], out["motp_sum"][s] = E._clear_host(frames, G)
        out["identity"][s] = E._identity_host(frames, G, K)
    return out


# ------------------------------------------------------------------------------------------------ the device path
def device_front_bdd(packed: PackedBDD, run=None, scatter_rows: bool = False, check_ids: bool = False) -> E.DeviceFront:
    """``_preprocess_host`` by the kernels of libtrack_eval_bdd_hip.so, on the current stream; ``packed`` holds CUDA
    tensors.  The one statement of what ``device_tables_bdd`` and ``diagnose_bdd100k._device_rows`` start with: the
    frames cut into the problem-major layout (``bddeval_class_count``, a cumulative sum, ``bddeval_class_split``), the
    similarity and the unmatched detections inside ignore regions (``bddeval_similarity``, ``bddeval_preproc``), then
    ``evaluation._front_tables`` with the S * 8 (sequence, class) pairs as its sequences.  ``run``: the per-call hook
    every library call goes through.  ``scatter_rows``: the split carries the rows' own numbers in place of their ids,
    which gives ``gt_src`` / ``tr_src``, and the split ids are one gather through them.  ``check_ids``: a pair whose
    identity assignment exceeds the device limit raises.  Beside ``evaluation.DeviceFront``'s attributes the front
    has ``split``: the input's ``seq_off`` and ``frame_src`` on the host; ``gt_off``, ``tr_off``, ``gt_ids``,
    ``tr_ids``, ``gt_boxes``, ``tr_boxes`` of the class split and ``remove`` on the device."""
    import torch
    from . import _track_eval_bdd_lib as B
    from . import _track_eval_lib as L
    fr = E.DeviceFront(packed.gt_boxes.device, run)
    ptr, new, entry = fr.ptr, fr.new, (B, "bddeval_similarity")
    seq_off = packed.seq_off.cpu().numpy()
    S, F = len(seq_off) - 1, len(packed.gt_off) - 1
    F8 = F * N_CLASSES
    fr.tens = tens = {k: getattr(packed, k).contiguous() for k in PackedBDD.ARRAYS}
    split_seq_off, frame_src = _split_offsets(seq_off)
    frame_seq = fr.up(np.repeat(np.arange(S, dtype=np.int32), np.diff(seq_off)))
    d_frame_src = fr.up(frame_src)
    # 1. the class split: counts per (frame, class), their running sum, the stable scatter
    counts = torch.zeros((2, max(F8, 1)), dtype=torch.int32, device=fr.dev)
    if F:
        fr.call(B, "bddeval_class_count", ptr(tens["gt_classes"]), ptr(tens["tr_classes"]), ptr(tens["gt_off"]),
                ptr(tens["tr_off"]), ptr(tens["seq_off"]), ptr(frame_seq), F, ptr(counts[0]), ptr(counts[1]))
    offs = torch.zeros((2, F8 + 1), dtype=torch.int32, device=fr.dev)
    offs[:, 1:] = torch.cumsum(counts[:, :F8], 1, dtype=torch.int32)
    d_gt_off, d_tr_off = offs[0].contiguous(), offs[1].contiguous()
    gt_off, tr_off = d_gt_off.cpu().numpy(), d_tr_off.cpu().numpy()                # (synchronises: sizes the rest)
    n_gt, n_tr = int(gt_off[-1]), int(tr_off[-1])
    gt_boxes, tr_boxes = new(4 * n_gt, torch.float64), new(4 * n_tr, torch.float64)
    gt_ids, tr_ids = new(n_gt, torch.int32), new(n_tr, torch.int32)
    if F:
        carried = (tens["gt_ids"], tens["tr_ids"])
        if scatter_rows:
            carried = (torch.arange(max(tens["gt_ids"].numel(), tens["tr_ids"].numel(), 1), dtype=torch.int32,
                                    device=fr.dev),) * 2
        fr.call(B, "bddeval_class_split", ptr(tens["gt_boxes"]), ptr(tens["tr_boxes"]), ptr(carried[0]),
                ptr(carried[1]), ptr(tens["gt_classes"]), ptr(tens["tr_classes"]), ptr(tens["gt_off"]),
                ptr(tens["tr_off"]), ptr(tens["seq_off"]), ptr(frame_seq), F, ptr(d_gt_off), ptr(d_tr_off),
                ptr(gt_boxes), ptr(tr_boxes), ptr(gt_ids), ptr(tr_ids))
    gt_ids, tr_ids = gt_ids[:n_gt], tr_ids[:n_tr]
    fr.split = {"seq_off": seq_off, "frame_src": frame_src, "gt_off": d_gt_off, "tr_off": d_tr_off}
    if scatter_rows:
        fr.split["gt_src"], fr.split["tr_src"] = gt_ids.long(), tr_ids.long()
        gt_ids, tr_ids = tens["gt_ids"][fr.split["gt_src"]], tens["tr_ids"][fr.split["tr_src"]]
    # 2. raw similarity; one assignment per (frame, class), then the ignore regions for what stayed unmatched
    fr.raw_sim, (_, _, d_sim_off), fr.n_raw = fr.similarity(entry, gt_boxes, tr_boxes, gt_off, tr_off)
    remove = new(n_tr, torch.int32, 0)
    if F8:
        status = new(F8, torch.int32, 0)
        fr.call(B, "bddeval_preproc", ptr(fr.raw_sim), ptr(d_sim_off), ptr(d_gt_off), ptr(d_tr_off), ptr(tr_boxes),
                ptr(tens["ig_off"]), ptr(tens["ig_boxes"]), ptr(d_frame_src), F8, E._frame_max(gt_off),
                E._frame_max(tr_off), ptr(remove), ptr(status))
        E._raise_on_status(status, "preprocessing match", "(frame, class)")
    fr.split.update(gt_ids=gt_ids, tr_ids=tr_ids, gt_boxes=gt_boxes[:4 * n_gt].view(-1, 4),
                    tr_boxes=tr_boxes[:4 * n_tr].view(-1, 4), remove=remove[:n_tr])

    def check(n_ids):
        if check_ids and E._most(n_ids) > L.MAX_DIM:
            p = int(n_ids.argmax())
            raise ValueError(f"sequence {packed.names[p // N_CLASSES]}, class {CLASSES[p % N_CLASSES]}: "
                             f"{int(n_ids[p])} ground-truth plus tracker ids: the identity assignment exceeds the "
                             f"device limit of {L.MAX_DIM} (evaluate it on the host)")

    # 3. the filter and the relabelling on the host, the similarity of what is kept: all ground truth stays
    host = _as_sequences(packed.names, {"seq_off": split_seq_off, "gt_off": gt_off, "tr_off": tr_off,
                                        "gt_ids": gt_ids.cpu().numpy(), "tr_ids": tr_ids.cpu().numpy()})
    return E._front_tables(fr, entry, host, None, fr.split["remove"].cpu().numpy() == 0, gt_boxes,
                           fr.split["tr_boxes"], check)


def device_tables_bdd(packed: PackedBDD, stream=None, timings: dict = None) -> dict:
    """``host_tables_bdd`` on the GPU; ``packed`` holds CUDA tensors.  ``device_front_bdd`` cuts the frames into the
    problem-major layout and preprocesses them; the kept detections then go through ``evaluation._metric_tables``, the
    metric kernels of libtrack_eval_hip.so, with S * 8 sequences.  Launches on ``stream`` (default: the current one);
    returns torch tensors on the device.  ``timings`` as ``device_tables``."""
    with E._on_stream(packed.gt_boxes.device, stream):
        fr = device_front_bdd(packed, E._timed(timings), check_ids=True)
        out = E._metric_tables(fr, "(frame, class)", "(sequence, class)")
        out.update({"split_" + k: fr.split[k] for k in ("gt_off", "tr_off", "gt_ids", "tr_ids", "gt_boxes", "tr_boxes")},
                   tr_remove=fr.split["remove"])
        return out


# ------------------------------------------------------------------------------------------- tables -> the fields
def combine_classes_det_averaged(results: Dict[str, dict]) -> dict:
    """The fields of several classes together, every detection counting the same: what ``combine_sequences`` does
    with sequences (counts and MOTP_sum add up, association scores and LocA averaged with HOTA_TP as weight, ratios
    formed again), as hota.py, clear.py, identity.py and count.py define ``combine_classes_det_averaged``."""
    return E.combine_sequences(results)


def combine_classes_class_averaged(results: Dict[str, dict]) -> dict:
    """The fields of several classes together, every class counting the same (``ignore_empty_classes=False``: a class
    without any detection contributes its fixed values, e.g. LocA 1): integer fields add up, every float field of
    HOTA, CLEAR (clear.py's ``float_fields``, MOTP_sum among them) and Identity is the mean over the classes."""
    classes = list(results.values())
    res = {k: sum([r[k] for r in classes])
           for k in E.HOTA_INT_ARRAYS + CLEAR_CLASS_SUMMED + E.IDENTITY_INTS + E.COUNT_INTS}
    for k in HOTA_FLOAT_FIELDS + CLEAR_CLASS_AVERAGED + E.IDENTITY_FLOATS:
        res[k] = np.mean([r[k] for r in classes], axis=0)
    return res


def results_from_tables(names: List[str], seq_off, t: dict) -> Dict[str, dict]:
    """``{seq: {class: fields}}`` and ``"COMBINED_SEQ": {class: ..., "cls_comb_cls_av": ..., "cls_comb_det_av": ...,
    "HUMAN": ..., "VEHICLE": ..., "BIKE": ...}`` (eval.py's layout; its ``'all'`` key is never produced)."""
    res = {}
    for s, name in enumerate(names):
        res[name] = {}
        for c, cls in enumerate(CLASSES):
            p = s * N_CLASSES + c
            res[name][cls] = E._sequence_result(seq_off[s + 1] - seq_off[s], t["n_gt_dets"][p], t["n_tr_dets"][p],
                                                t["n_gt_ids"][p], t["n_tr_ids"][p], t["hota_tp"][p],
                                                t["hota_sums"][p], t["clear_ints"][p], t["motp_sum"][p],
                                                t["identity"][p])
    comb = {cls: E.combine_sequences({name: res[name][cls] for name in names}) for cls in CLASSES}
    per_class = {cls: comb[cls] for cls in CLASSES}
    comb["cls_comb_cls_av"] = combine_classes_class_averaged(per_class)
    comb["cls_comb_det_av"] = combine_classes_det_averaged(per_class)
    for cat, members in SUPER_CATEGORIES.items():
        comb[cat] = combine_classes_det_averaged({cls: per_class[cls] for cls in CLASSES if cls in members})
    res["COMBINED_SEQ"] = comb
    return res


def bdd_summary(res: Dict[str, dict]) -> Dict[str, Dict[str, float]]:
    """``{key: names and values of <key>_summary.txt}`` for every class and combined key of ``res["COMBINED_SEQ"]``."""
    return {key: E.summary(fields) for key, fields in res["COMBINED_SEQ"].items()}


# ---------------------------------------------------------------------------------------------------- entry points
RESULT_KEYS = ("n_gt_dets", "n_tr_dets", "n_gt_ids", "n_tr_ids", "hota_tp", "hota_sums", "clear_ints", "motp_sum",
               "identity")


def evaluate_packed_bdd(packed: PackedBDD, device=None, stream=None) -> Dict[str, dict]:
    """The result layout of ``results_from_tables``.  ``device``: a CUDA device for the kernels; "cpu" or None (the
    default) for the host statement, to which device tensors are copied."""
    if not packed.names:
        raise ValueError("no sequence to evaluate")
    if "COMBINED_SEQ" in packed.names:
        raise ValueError("a sequence may not be called COMBINED_SEQ")
    if device is not None and str(device).startswith("cuda"):
        t = device_tables_bdd(packed if packed.is_device() else packed.to(device), stream=stream)
        t = {k: t[k].cpu().numpy() for k in RESULT_KEYS}                           # (synchronises)
        seq_off = packed.seq_off.cpu().numpy() if packed.is_device() else packed.seq_off
    else:
        t, seq_off = host_tables_bdd(packed), packed.numpy().seq_off
    return results_from_tables(packed.names, seq_off, t)


def _class_ids(categories, n: int, what: str) -> np.ndarray:
    """Category names or TrackEval class ids -> class ids."""
    out = np.zeros(n, np.int64)
    values = categories.tolist() if hasattr(categories, "tolist") else list(categories)
    if len(values) != n:
        raise ValueError(f"{what}: ids and categories differ in length")
    for i, v in enumerate(values):
        if isinstance(v, str):
            if v not in CLASS_NAME_TO_CLASS_ID:
                raise ValueError(f"{what}: unknown category {v!r}")
            out[i] = CLASS_NAME_TO_CLASS_ID[v]
        else:
            if int(v) not in CLASS_NAME_TO_CLASS_ID.values():
                raise ValueError(f"{what}: unknown class id {v!r}")
            out[i] = int(v)
    return out


class BDD100KEvaluator:
    """Collects ground truth and tracker output frame by frame (0-based frame indices), then evaluates all sequences
    in one call."""

    def __init__(self, device=None):
        self.device = device
        self._gt: Dict[str, dict] = {}
        self._tr: Dict[str, dict] = {}
        self._length: Dict[str, int] = {}

    def set_length(self, seq: str, n_frames: int) -> None:
        """Number of frames of ``seq``; default: one more than the last frame index anything was added for."""
        self._length[seq] = int(n_frames)

    def add_ground_truth(self, seq: str, frame_idx: int, ids, boxes_xyxy, categories, crowd=None) -> None:
        """Ground truth of frame ``frame_idx``.  ``categories``: names or TrackEval's class ids.  Rows of a distractor
        category (other person, trailer, other vehicle) or with ``crowd`` true are the frame's ignore regions and no
        ground truth, as ``BDD100K._load_raw_file`` reads them."""
        ids = _host_array(ids, np.int64).reshape(-1)
        boxes = _host_array(boxes_xyxy, np.float64).reshape(-1, 4)
        classes = _class_ids(categories, len(ids), f"sequence {seq}, frame {frame_idx}")
        region = np.isin(classes, [CLASS_NAME_TO_CLASS_ID[c] for c in DISTRACTOR_CATEGORIES])
        if crowd is not None:
            region |= _host_array(crowd, bool).reshape(-1)
        self._gt.setdefault(seq, {})[int(frame_idx)] = (ids[~region], boxes[~region], classes[~region], boxes[region])

    def add_frame(self, seq: str, frame_idx: int, result) -> None:
        """Tracker output of frame ``frame_idx``: what ``SequenceTracker.step`` / ``step_raw`` / ``track`` return
        (``ids``, ``labels`` as the model's label indices, ``boxes`` as xyxy pixels).  The boxes are the doubles
        ``bdd_frame_result`` would print and TrackEval would read back; the labels go through ``LABEL_TO_CLASS_ID``."""
        to_class_id = __getattr__("LABEL_TO_CLASS_ID")
        self._tr.setdefault(seq, {})[int(frame_idx)] = (
            np.asarray(result.ids.tolist(), np.int64).reshape(-1),
            np.asarray(result.boxes.tolist(), np.float64).reshape(-1, 4),
            np.asarray([to_class_id[k] for k in result.labels.tolist()], np.int64).reshape(-1))

    def add_tracker_rows(self, seq: str, frame_idx: int, ids, boxes_xyxy, categories) -> None:
        """Tracker output of frame ``frame_idx`` as ids, xyxy boxes and categories (names or class ids)."""
        ids = _host_array(ids, np.int64).reshape(-1)
        self._tr.setdefault(seq, {})[int(frame_idx)] = (
            ids, _host_array(boxes_xyxy, np.float64).reshape(-1, 4),
            _class_ids(categories, len(ids), f"sequence {seq}, frame {frame_idx}"))

    def sequences(self) -> Dict[str, dict]:
        out = {}
        none_i, none_b = np.zeros(0, np.int64), np.zeros((0, 4))
        for seq in list(self._gt) + [s for s in self._tr if s not in self._gt]:
            gt, tr = self._gt.get(seq, {}), self._tr.get(seq, {})
            T = self._length.get(seq, max(list(gt) + list(tr) + [-1]) + 1)
            bad = [f for f in list(gt) + list(tr) if f < 0 or f >= T]
            if bad:
                raise ValueError(f"sequence {seq}: frame {bad[0]} is outside 0 .. {T - 1}")
            rows = [gt.get(f, (none_i, none_b, none_i, none_b)) for f in range(T)]
            trk = [tr.get(f, (none_i, none_b, none_i)) for f in range(T)]
            out[seq] = {"gt_ids": [r[0] for r in rows], "gt_boxes": [r[1] for r in rows],
                        "gt_classes": [r[2] for r in rows], "ignore_regions": [r[3] for r in rows],
                        "tracker_ids": [r[0] for r in trk], "tracker_boxes": [r[1] for r in trk],
                        "tracker_classes": [r[2] for r in trk]}
        return out

    def evaluate(self) -> Dict[str, dict]:
        return evaluate_packed_bdd(pack_bdd(self.sequences()), device=self.device if self.device else "cpu")

    def events(self) -> Dict[str, object]:
        """``{name: diagnose_bdd100k.BDDSequenceEvents}`` of what was collected: the decisions behind the per-class
        CLEAR counts, per row, the tracker boxes dropped inside ignore regions and the class confusions."""
        from .diagnose_bdd100k import bdd_events
        return bdd_events(pack_bdd(self.sequences()), device=self.device)


def _read_frames(path: str) -> list:
    with open(path) as f:
        frames = json.load(f)
    key = "index" if frames and all("index" in fr for fr in frames) else "frameIndex"
    return sorted(frames, key=lambda fr: fr[key])


def load_bdd_files(gt_dir: str, tracker_dir: str, device=None) -> BDD100KEvaluator:
    """Result files as a filled ``BDD100KEvaluator`` (``evaluate_bdd_files`` scores it, ``diagnose_bdd100k`` asks it for
    the events): one ``<seq>.json`` per sequence in ``gt_dir`` and in ``tracker_dir``, each a list of frames
    ``{"index" | "frameIndex", "labels": [{"id", "category", "box2d": {"x1", "y1", "x2", "y2"}, "attributes":
    {"Crowd": bool}}]}``.  Frames are sorted by ``index`` where every frame has it, else by ``frameIndex``: TrackEval
    reads the first, the reference's writer (``SequenceTracker.bdd_frame_result``) emits the second, so both are
    accepted.  The t-th frame of one side belongs to the t-th of the other; ids (strings in the writer's files) go
    through ``int()``.  Unequal frame counts on the two sides of a sequence are a ``ValueError``, as in TrackEval."""
    ev = BDD100KEvaluator(device)
    for seq in sorted(f[:-5] for f in os.listdir(gt_dir) if f.endswith(".json")):
        tracker_file = os.path.join(tracker_dir, seq + ".json")
        if not os.path.isfile(tracker_file):
            raise ValueError(f"tracker file not found: {tracker_file}")
        gt, tr = _read_frames(os.path.join(gt_dir, seq + ".json")), _read_frames(tracker_file)
        if len(gt) != len(tr):
            raise ValueError(f"sequence {seq}: the number of ground-truth ({len(gt)}) and tracker ({len(tr)}) frames "
                             "do not match")
        ev.set_length(seq, len(gt))
        box = lambda a: [a["box2d"][k] for k in ("x1", "y1", "x2", "y2")]             # noqa: E731
        for t, (g, r) in enumerate(zip(gt, tr)):
            labels = g.get("labels") or []
            ev.add_ground_truth(seq, t, [int(a["id"]) for a in labels], [box(a) for a in labels],
                                [a["category"] for a in labels],
                                [bool(a.get("attributes", {}).get("Crowd", False)) for a in labels])
            labels = r.get("labels") or []
            ev.add_tracker_rows(seq, t, [int(a["id"]) for a in labels], [box(a) for a in labels],
                                [a["category"] for a in labels])
        ev._gt.setdefault(seq, {})
    return ev


def evaluate_bdd_files(gt_dir: str, tracker_dir: str, device=None) -> Dict[str, dict]:
    """Score result files in ``load_bdd_files``' layout."""
    return load_bdd_files(gt_dir, tracker_dir, device).evaluate()


# ------------------------------------------------------------------------------------------------- synthetic data
def synthetic_bdd_sequence(seed: int, n_frames: int, n_objects: int, *, n_regions: int = 2, n_classes: int = N_CLASSES,
                           **kwargs) -> dict:
    """A sequence of per-frame lists (``pack_bdd``'s input) for tests and ``tools/bench_eval_bdd.py``:
    ``evaluation.synthetic_sequence``'s random walks with the classes assigned by object index (object i has class
    ``CLASSES[i % n_classes]``, and a followed object's detections carry its class), false positives of random
    classes, and ``n_regions`` ignore regions per frame, each laid over one of the frame's false positives or at
    random."""
    seq = E.synthetic_sequence(seed, n_frames, n_objects, **kwargs)
    rng = np.random.RandomState(seed + 7919)
    xyxy = lambda b: np.concatenate([b[:, :2], b[:, :2] + b[:, 2:]], 1) if len(b) else np.zeros((0, 4))   # noqa: E731
    class_of = lambda ids: np.array([CLASS_IDS[(int(i) - 1) % n_classes] for i in ids], np.int64)         # noqa: E731
    out = {k: [] for k in ("gt_ids", "gt_boxes", "gt_classes", "tracker_ids", "tracker_boxes", "tracker_classes",
                           "ignore_regions")}
    names = {}                                         # tracker id -> class id: the class of the object it was first on
    for t in range(n_frames):
        gi, gb = seq["gt_ids"][t], xyxy(seq["gt_boxes"][t])
        ti, tb = seq["tracker_ids"][t], xyxy(seq["tracker_boxes"][t])
        gc, tc = class_of(gi), np.zeros(len(ti), np.int64)
        false = []
        for j, tid in enumerate(ti.tolist()):
            if tid >= 500000:                          # a false positive
                tc[j] = CLASS_IDS[rng.randint(n_classes)]
                false.append(j)
                continue
            if tid not in names:                       # the object this name follows: the nearest ground truth
                centre = (tb[j, :2] + tb[j, 2:]) / 2
                near = np.abs((gb[:, :2] + gb[:, 2:]) / 2 - centre).sum(1).argmin() if len(gb) else -1
                names[tid] = gc[near] if near >= 0 else CLASS_IDS[0]
            tc[j] = names[tid]
        regions = []
        for r in range(n_regions):
            if false and rng.uniform() < 0.5:
                b = tb[false[rng.randint(len(false))]]
                grow = rng.uniform(-10, 30, 4) * np.array([-1, -1, 1, 1])
                regions.append(b + grow)
            else:
                xy = rng.uniform(0, 1500, 2)
                regions.append(np.concatenate([xy, xy + rng.uniform(40, 300, 2)]))
        for k, v in zip(out, (gi, gb, gc, ti, tb, tc, np.array(regions, np.float64).reshape(-1, 4))):
            out[k].append(v)
    return out
