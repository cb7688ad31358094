"""Tracking evaluation: HOTA, CLEAR and Identity for one class (``pedestrian``), the numbers the reference gets from
TrackEval (``eval_engine.py``: ``--METRICS HOTA CLEAR Identity``, MOT-challenge preprocessing) and reads back from
``pedestrian_summary.txt`` -- here from tracker output and ground truth in memory, or from the same text files.

    ev = TrackingEvaluator(benchmark="MOT17", device="cuda")
    ev.add_ground_truth("seq0", frame, ids, boxes_xywh)              # frame: 1-based, as in gt.txt
    for frame_idx, result in tracker.track(frames):                  # what SequenceTracker.step / step_raw returns
        ev.add_frame("seq0", frame_idx, result)                      # frame_idx: 0-based, as for mot_lines
    res = ev.evaluate()                                              # {"seq0": {...}, "COMBINED_SEQ": {...}}
    print(summary(res["COMBINED_SEQ"]))                              # names / values of pedestrian_summary.txt

The definition is stated twice.  ``host_tables`` is numpy and ``scipy.optimize.linear_sum_assignment``, written from
the definitions (Luiten et al., "HOTA", IJCV 2020; Bernardin & Stiefelhagen, CLEAR MOT, 2008; Ristani et al., ID
measures, 2016, and the conventions of TrackEval's implementation of them: thresholds shifted by the float64 epsilon,
the order of the matching, what an empty side returns).  ``device_tables`` is the same on the GPU
(memotr_amd/csrc/track_eval.hip): ``device_front`` preprocesses, and the metric stage, ``diagnose`` and ``association``
stand on what it returns.  Both produce the per-sequence tables that ``_sequence_result`` turns into
TrackEval's fields; integer fields and similarities agree exactly, float fields to float64 summation order.  The
host statement is the default wherever the inputs live; the kernels run where a CUDA ``device`` is asked for, and a
missing library raises then.  (The kernels become the default for device inputs once ``tools/bench_eval.py`` has shown
their whole-set wall time below the host statement's on an MI355X; that measurement has not been made.)

Scope: DanceTrack, SportsMOT, MOT17 (``benchmark="MOT17"``: detections matched to a distractor ground truth -- classes
2, 7, 8, 12 -- are dropped, then ground truth that is not class 1 or is zero-marked) and ``benchmark="MOT15"`` (no
matching, no class filter).  An assignment problem larger than 2048 on a side is an error on the device path.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

ALPHAS = np.arange(0.05, 0.99, 0.05)                    # HOTA's 19 localisation thresholds
EPS = np.finfo("float").eps
THRESHOLD = 0.5
DISTRACTOR_CLASSES = (2, 7, 8, 12)                      # person_on_vehicle, static_person, distractor, reflection
PEDESTRIAN = 1

HOTA_FLOAT_ARRAYS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA", "RHOTA")
HOTA_INT_ARRAYS = ("HOTA_TP", "HOTA_FN", "HOTA_FP")
HOTA_FLOATS = ("HOTA(0)", "LocA(0)", "HOTALocA(0)")
CLEAR_INTS = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag", "CLR_Frames")
CLEAR_FLOATS = ("MOTA", "MOTP", "MODA", "CLR_Re", "CLR_Pr", "MTR", "PTR", "MLR", "sMOTA", "CLR_F1", "FP_per_frame",
                "MOTAL", "MOTP_sum")
IDENTITY_INTS = ("IDTP", "IDFN", "IDFP")
IDENTITY_FLOATS = ("IDF1", "IDR", "IDP")
COUNT_INTS = ("Dets", "GT_Dets", "IDs", "GT_IDs")
INT_FIELDS = CLEAR_INTS + IDENTITY_INTS + COUNT_INTS
FLOAT_FIELDS = HOTA_FLOATS + CLEAR_FLOATS + IDENTITY_FLOATS
# pedestrian_summary.txt: the summary fields of HOTA, CLEAR, Identity and Count in TrackEval's fixed order
SUMMARY_FIELDS = HOTA_FLOAT_ARRAYS + HOTA_FLOATS + (
    "MOTA", "MOTP", "MODA", "CLR_Re", "CLR_Pr", "MTR", "PTR", "MLR", "CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT",
    "ML", "Frag", "sMOTA", "IDF1", "IDR", "IDP", "IDTP", "IDFN", "IDFP") + COUNT_INTS


# ------------------------------------------------------------------------------------------------------- the input
@dataclass
class PackedSequences:
    """All sequences of one call as ragged arrays (include/track_eval_hip.h): numpy, or torch tensors on one device.
    Frames of a sequence are consecutive; boxes are float64 xywh; ids, classes and zero_marked are int32."""
    names: List[str]
    seq_off: object             # int32 [S + 1]
    gt_off: object              # int32 [F + 1]
    tr_off: object              # int32 [F + 1]
    gt_boxes: object            # float64 [NG, 4]
    tr_boxes: object            # float64 [NT, 4]
    gt_ids: object              # int32 [NG]
    tr_ids: object              # int32 [NT]
    gt_classes: object          # int32 [NG]
    gt_zero_marked: object      # int32 [NG]

    ARRAYS = ("seq_off", "gt_off", "tr_off", "gt_boxes", "tr_boxes", "gt_ids", "tr_ids", "gt_classes",
              "gt_zero_marked")

    def is_device(self) -> bool:
        return not isinstance(self.gt_boxes, np.ndarray) and self.gt_boxes.is_cuda

    def numpy(self) -> "PackedSequences":
        if isinstance(self.gt_boxes, np.ndarray):
            return self
        return PackedSequences(self.names, *[getattr(self, k).cpu().numpy() for k in self.ARRAYS])

    def to(self, device) -> "PackedSequences":
        import torch
        return PackedSequences(self.names, *[torch.as_tensor(getattr(self, k)).to(device) for k in self.ARRAYS])

    def select(self, index: int) -> "PackedSequences":
        """Sequence ``index`` alone (host arrays)."""
        p = self.numpy()
        f0, f1 = int(p.seq_off[index]), int(p.seq_off[index + 1])
        g0, g1, t0, t1 = int(p.gt_off[f0]), int(p.gt_off[f1]), int(p.tr_off[f0]), int(p.tr_off[f1])
        return PackedSequences([p.names[index]], np.array([0, f1 - f0], np.int32), p.gt_off[f0:f1 + 1] - g0,
                               p.tr_off[f0:f1 + 1] - t0, p.gt_boxes[g0:g1], p.tr_boxes[t0:t1], p.gt_ids[g0:g1],
                               p.tr_ids[t0:t1], p.gt_classes[g0:g1], p.gt_zero_marked[g0:g1])


def _host_array(x, dtype):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def pack_sequences(sequences: Dict[str, dict]) -> PackedSequences:
    """``{name: {"gt_ids": [...], "gt_boxes": [...], "tracker_ids": [...], "tracker_boxes": [...], "gt_classes":
    [...], "gt_zero_marked": [...]}}`` -- every value a list with one array per frame (ids ``(n,)``, boxes ``(n, 4)``
    xywh); classes default to 1 and zero_marked to 1 -- as host ``PackedSequences``."""
    names, seq_off, gt_n, tr_n = [], [0], [], []
    cols = {k: [] for k in ("gt_boxes", "tr_boxes", "gt_ids", "tr_ids", "gt_classes", "gt_zero_marked")}
    for name, seq in sequences.items():
        T = len(seq["gt_ids"])
        if not (len(seq["gt_boxes"]) == len(seq["tracker_ids"]) == len(seq["tracker_boxes"]) == T):
            raise ValueError(f"sequence {name}: the per-frame lists differ in length")
        names.append(name)
        seq_off.append(seq_off[-1] + T)
        for t in range(T):
            gi = _host_array(seq["gt_ids"][t], np.int64).reshape(-1)
            ti = _host_array(seq["tracker_ids"][t], np.int64).reshape(-1)
            gb = _host_array(seq["gt_boxes"][t], np.float64).reshape(-1, 4)
            tb = _host_array(seq["tracker_boxes"][t], np.float64).reshape(-1, 4)
            if len(gb) != len(gi) or len(tb) != len(ti):
                raise ValueError(f"sequence {name}, frame {t}: ids and boxes differ in length")
            for which, ids in (("ground-truth", gi), ("tracker", ti)):
                if len(np.unique(ids)) != len(ids):
                    raise ValueError(f"sequence {name}, frame {t}: a {which} id occurs more than once")
                if len(ids) and (ids.min() < 0 or ids.max() >= 2 ** 31):
                    raise ValueError(f"sequence {name}, frame {t}: a {which} id is outside [0, 2**31)")
            gc = seq["gt_classes"][t] if seq.get("gt_classes") is not None else np.ones(len(gi))
            gz = seq["gt_zero_marked"][t] if seq.get("gt_zero_marked") is not None else np.ones(len(gi))
            gt_n.append(len(gi))
            tr_n.append(len(ti))
            cols["gt_boxes"].append(gb)
            cols["tr_boxes"].append(tb)
            cols["gt_ids"].append(gi.astype(np.int32))
            cols["tr_ids"].append(ti.astype(np.int32))
            cols["gt_classes"].append(_host_array(gc, np.int32).reshape(-1))
            cols["gt_zero_marked"].append(_host_array(gz, np.int32).reshape(-1))

    def cat(key, shape, dtype):
        return np.concatenate(cols[key]).astype(dtype) if cols[key] else np.zeros(shape, dtype)

    off = lambda n: np.concatenate(([0], np.cumsum(n))).astype(np.int32)      # noqa: E731
    return PackedSequences(names, np.asarray(seq_off, np.int32), off(gt_n), off(tr_n),
                           cat("gt_boxes", (0, 4), np.float64), cat("tr_boxes", (0, 4), np.float64),
                           cat("gt_ids", (0,), np.int32), cat("tr_ids", (0,), np.int32),
                           cat("gt_classes", (0,), np.int32), cat("gt_zero_marked", (0,), np.int32))


def _sim_offsets(gt_off, tr_off):
    g, k = np.diff(gt_off).astype(np.int64), np.diff(tr_off).astype(np.int64)
    return np.concatenate(([0], np.cumsum(g * k))).astype(np.int64)


def _relabel(ids, off, seq_off):
    """Per sequence, ids replaced by their rank among the sequence's distinct ids; the number of ids per sequence."""
    out, n = np.zeros(len(ids), np.int32), np.zeros(len(seq_off) - 1, np.int32)
    for s in range(len(seq_off) - 1):
        a, b = off[seq_off[s]], off[seq_off[s + 1]]
        uniq, inv = np.unique(ids[a:b], return_inverse=True)
        out[a:b], n[s] = inv, len(uniq)
    return out, n


def _id_tables(n_gt_ids, n_tr_ids):
    z = lambda x, t: np.concatenate(([0], np.cumsum(x.astype(np.int64)))).astype(t)       # noqa: E731
    return z(n_gt_ids.astype(np.int64) * n_tr_ids, np.int64), z(n_gt_ids, np.int32), z(n_tr_ids, np.int32)


# --------------------------------------------------------------------------------- the definition, on the host
def box_iou_xywh(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """IoU of every box of ``a`` (n, 4) with every box of ``b`` (m, 4), xywh, float64; a box or a union without area
    gives 0.  (Operation order as TrackEval's: corners by one addition, union = area + area - intersection.)"""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    ax1, ay1, bx1, by1 = a[:, 0] + a[:, 2], a[:, 1] + a[:, 3], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
    w = np.minimum(ax1[:, None], bx1[None, :]) - np.maximum(a[:, 0, None], b[None, :, 0])
    h = np.minimum(ay1[:, None], by1[None, :]) - np.maximum(a[:, 1, None], b[None, :, 1])
    inter = np.maximum(w, 0) * np.maximum(h, 0)
    area_a, area_b = (ax1 - a[:, 0]) * (ay1 - a[:, 1]), (bx1 - b[:, 0]) * (by1 - b[:, 1])
    union = area_a[:, None] + area_b[None, :] - inter
    dead = (area_a <= EPS)[:, None] | (area_b <= EPS)[None, :] | (union <= EPS)
    inter = np.where(dead, 0.0, inter)
    union = np.where(union <= EPS, 1.0, union)
    return inter / union


def _assign(cost):
    from scipy.optimize import linear_sum_assignment
    return linear_sum_assignment(cost)


def _preprocess_host(p: PackedSequences, benchmark: str):
    """Raw and preprocessed similarity (all frames, concatenated) and the preprocessed, relabelled data."""
    F = len(p.gt_off) - 1
    raw_sim, sims, keep_tr = [], [], np.ones(len(p.tr_ids), bool)
    keep_gt = p.gt_zero_marked != 0
    if benchmark != "MOT15":
        keep_gt &= p.gt_classes == PEDESTRIAN
    for f in range(F):
        g0, g1, t0, t1 = p.gt_off[f], p.gt_off[f + 1], p.tr_off[f], p.tr_off[f + 1]
        sim = box_iou_xywh(p.gt_boxes[g0:g1], p.tr_boxes[t0:t1])
        raw_sim.append(sim.reshape(-1))
        if benchmark != "MOT15" and g1 > g0 and t1 > t0:
            score = np.where(sim < THRESHOLD - EPS, 0.0, sim)
            rows, cols = _assign(-score)
            hit = score[rows, cols] > EPS
            rows, cols = rows[hit], cols[hit]
            keep_tr[t0 + cols[np.isin(p.gt_classes[g0:g1][rows], DISTRACTOR_CLASSES)]] = False
        sims.append(sim[keep_gt[g0:g1]][:, keep_tr[t0:t1]].reshape(-1))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)            # noqa: E731
    return cat(raw_sim), cat(sims), _compact(p, keep_gt, keep_tr)


def _compact(p: PackedSequences, keep_gt: np.ndarray, keep_tr: np.ndarray) -> dict:
    """The kept detections with ids relabelled 0 .. n - 1 per sequence, and the per-sequence table offsets."""
    count = lambda keep, off: np.concatenate(([0], np.cumsum(keep)))[off].astype(np.int32)     # noqa: E731
    d = {"seq_off": p.seq_off, "gt_off": count(keep_gt, p.gt_off), "tr_off": count(keep_tr, p.tr_off),
         "keep_gt": np.flatnonzero(keep_gt), "keep_tr": np.flatnonzero(keep_tr)}
    d["gt_ids"], d["n_gt_ids"] = _relabel(p.gt_ids[keep_gt], d["gt_off"], p.seq_off)
    d["tr_ids"], d["n_tr_ids"] = _relabel(p.tr_ids[keep_tr], d["tr_off"], p.seq_off)
    d["cell_off"], d["gid_off"], d["tid_off"] = _id_tables(d["n_gt_ids"], d["n_tr_ids"])
    d["sim_off"] = _sim_offsets(d["gt_off"], d["tr_off"])
    d["n_gt_dets"] = np.diff(d["gt_off"][p.seq_off]).astype(np.int64)
    d["n_tr_dets"] = np.diff(d["tr_off"][p.seq_off]).astype(np.int64)
    return d


def _frames_of(d, sim, s):
    """(gt ids, tracker ids, similarity) of every frame of sequence ``s``."""
    for f in range(d["seq_off"][s], d["seq_off"][s + 1]):
        gi, ti = d["gt_ids"][d["gt_off"][f]:d["gt_off"][f + 1]], d["tr_ids"][d["tr_off"][f]:d["tr_off"][f + 1]]
        yield gi, ti, sim[d["sim_off"][f]:d["sim_off"][f + 1]].reshape(len(gi), len(ti))


def _hota_host(frames, G, K):
    """HOTA_TP (19,) and the sums over id pairs / frames that AssA, AssRe, AssPr and LocA are made of, (4, 19)."""
    potential, gt_count, tr_count = np.zeros((G, K)), np.zeros((G, 1)), np.zeros((1, K))
    for gi, ti, sim in frames:          # how much of each other two ids see, before any matching
        denom = sim.sum(0)[None, :] + sim.sum(1)[:, None] - sim
        share = np.zeros_like(sim)
        np.divide(sim, denom, out=share, where=denom > 0 + EPS)
        potential[gi[:, None], ti[None, :]] += share
        gt_count[gi] += 1
        tr_count[0, ti] += 1
    alignment = potential / (gt_count + tr_count - potential)
    tp, loc, matches = np.zeros(len(ALPHAS)), np.zeros(len(ALPHAS)), np.zeros((len(ALPHAS), G, K))
    for gi, ti, sim in frames:
        if len(gi) == 0 or len(ti) == 0:
            continue
        rows, cols = _assign(-(alignment[gi[:, None], ti[None, :]] * sim))
        for a, alpha in enumerate(ALPHAS):
            hit = sim[rows, cols] >= alpha - EPS
            tp[a] += hit.sum()
            if hit.any():
                loc[a] += sum(sim[rows[hit], cols[hit]])
                matches[a, gi[rows[hit]], ti[cols[hit]]] += 1
    sums = np.stack([(matches * (matches / np.maximum(1, gt_count + tr_count - matches))).sum((1, 2)),
                     (matches * (matches / np.maximum(1, gt_count))).sum((1, 2)),
                     (matches * (matches / np.maximum(1, tr_count))).sum((1, 2)), loc])
    return tp, sums


def _clear_host(frames, G):
    """CLR_TP, CLR_FN, CLR_FP, IDSW, MT, PT, ML, Frag and the sum of the matched similarities."""
    seen, matched, starts = np.zeros(G), np.zeros(G), np.zeros(G)
    last, last_step = np.full(G, -1), np.full(G, -1)    # tracker id of the last match ever / in the previous frame
    tp = fn = fp = idsw = 0
    motp_sum = 0.0
    for gi, ti, sim in frames:
        if len(gi) == 0:
            fp += len(ti)
            continue
        seen[gi] += 1
        if len(ti) == 0:
            fn += len(gi)
            continue
        # keep last frame's pairs where still possible (1000 outweighs any similarity), then maximise similarity
        score = 1000 * (ti[None, :] == last_step[gi[:, None]]) + sim
        score[sim < THRESHOLD - EPS] = 0
        rows, cols = _assign(-score)
        hit = score[rows, cols] > 0 + EPS
        rows, cols = rows[hit], cols[hit]
        mg, mt = gi[rows], ti[cols]
        idsw += int(((last[mg] >= 0) & (last[mg] != mt)).sum())
        matched[mg] += 1
        was_free = last_step < 0
        last[mg] = mt
        last_step[:] = -1
        last_step[mg] = mt
        starts += was_free & (last_step >= 0)
        tp, fn, fp = tp + len(mg), fn + len(gi) - len(mg), fp + len(ti) - len(mg)
        if len(mg):
            motp_sum += sum(sim[rows, cols])
    ratio = matched[seen > 0] / seen[seen > 0]
    mt = int((ratio > 0.8).sum())
    pt = int((ratio >= 0.2).sum()) - mt
    frag = int((starts[starts > 0] - 1).sum())
    return np.array([tp, fn, fp, idsw, mt, pt, G - mt - pt, frag], np.int64), motp_sum


def _identity_host(frames, G, K):
    """IDFN and IDFP: the one-to-one map of whole trajectories (every id may also stay unmatched) with the fewest
    false negatives plus false positives."""
    both, gt_count, tr_count = np.zeros((G, K)), np.zeros(G), np.zeros(K)
    for gi, ti, sim in frames:
        r, c = np.nonzero(sim >= THRESHOLD)
        both[gi[r], ti[c]] += 1
        gt_count[gi] += 1
        tr_count[ti] += 1
    fn, fp = np.zeros((G + K, G + K)), np.zeros((G + K, G + K))
    fn[:G, K:], fp[G:, :K] = 1e10, 1e10                 # an id's "unmatched" slot is its own
    fn[:G, :K] = gt_count[:, None] - both
    fn[np.arange(G), K + np.arange(G)] = gt_count
    fp[:G, :K] = tr_count[None, :] - both
    fp[G + np.arange(K), np.arange(K)] = tr_count
    rows, cols = _assign(fn + fp)
    return np.array([fn[rows, cols].sum().astype(np.int64), fp[rows, cols].sum().astype(np.int64)], np.int64)


def host_tables(packed: PackedSequences, benchmark: str = "MOT17") -> dict:
    """The whole definition on the host: raw similarity, preprocessed ids and, per sequence, the integer counts and
    float sums the metric fields are made of (the same dictionary ``device_tables`` returns, as numpy arrays)."""
    p = packed.numpy()
    raw_sim, sim, d = _preprocess_host(p, benchmark)
    S = len(p.names)
    out = {"raw_similarity": raw_sim, "similarity": sim, "hota_tp": np.zeros((S, len(ALPHAS)), np.int64),
           "hota_sums": np.zeros((S, 4, len(ALPHAS))), "clear_ints": np.zeros((S, 8), np.int64),
           "motp_sum": np.zeros(S), "identity": np.zeros((S, 2), np.int64)}
    out.update({k: d[k] for k in ("gt_off", "tr_off", "gt_ids", "tr_ids", "n_gt_ids", "n_tr_ids", "n_gt_dets",
                                  "n_tr_dets")})
    for s in range(S):
        G, K = int(d["n_gt_ids"][s]), int(d["n_tr_ids"][s])
        if d["n_gt_dets"][s] == 0 or d["n_tr_dets"][s] == 0:
            continue                    # (an empty side: the fields are fixed by the counts, _sequence_result)
        frames = list(_frames_of(d, sim, s))
        tp, out["hota_sums"][s] = _hota_host(frames, G, K)
        out["hota_tp"][s] = tp
        out["clear_ints"][s], out["motp_sum"][s] = _clear_host(frames, G)
        out["identity"][s] = _identity_host(frames, G, K)
    return out


# ------------------------------------------------------------------------------------------------ the device path
def _ptr(t, spare):
    return t.data_ptr() if t.numel() else spare.data_ptr()


def _call(module, name, *args):
    module.check(getattr(module.lib, name)(*args), name)


def _launch(name: str, dev, tensors_and_ints, spare=None) -> None:
    """One entry point of libclip_ops_hip.so on the current stream of ``dev``: tensors become addresses (an empty one the
    address of ``spare``, a two-word array the caller keeps; allocated here when there is none), ``None`` a null pointer,
    everything else is passed as it is."""
    import torch
    from . import _clip_lib as C
    with torch.cuda.device(dev):
        if spare is None:
            spare = torch.zeros(2, dtype=torch.float64, device=dev)
        args = [_ptr(a, spare) if hasattr(a, "data_ptr") else a for a in tensors_and_ints]
        _call(C, name, *args, torch.cuda.current_stream(dev).cuda_stream)


def _timed(timings: dict = None):
    """The per-call hook of the device paths, ``run(name, fn, *args)``: ``fn(*args)``; with a dict, between a pair of
    events that ``timings[name]`` receives."""
    def run(name, fn, *args):
        if timings is None:
            return fn(*args)
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        timings.setdefault(name, []).append((a, b))
    return run


def _on_stream(dev, stream=None):
    import torch
    return torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev)


def _most(a) -> int:
    return int(a.max()) if len(a) else 0


def _frame_max(off) -> int:
    return _most(np.diff(off))


class DeviceFront:
    """What every device path starts from (``device_front``, ``evaluation_bdd100k.device_front_bdd``): the preprocessed
    data on the host and on the device, and the helpers the launches behind it are written with.

    Host: ``d`` (``_compact``'s dictionary), ``host`` (the ``PackedSequences`` it was made from), ``tens`` (the input's
    tensors, contiguous), ``S`` sequences, ``F`` frames, ``cells`` / ``n_gid`` / ``n_tid`` (the lengths of the id-pair
    and the per-id tables), and the launch sizes: ``max_gt`` / ``max_tr`` (kept detections of a frame), ``max_gt_ids`` /
    ``max_side`` / ``max_ids`` (a sequence's ground-truth ids, ids on its larger side, ids of both sides).
    Device: ``raw_sim`` [``n_raw``] of the input's frames; ``sim`` [``n_sim``] of the kept detections behind ``gt_off``,
    ``tr_off``, ``sim_off``; the relabelled ``gt_ids``, ``tr_ids``; ``seq_off``, ``n_gt_ids``; and, once
    ``device_accumulate`` has run, ``n_tr_ids``, ``cell_off``, ``gid_off``, ``tid_off``, ``frame_seq``.  Arrays a launch
    writes are at least one element long."""

    def __init__(self, dev, run=None):
        import torch
        self.dev, self.run = dev, run or _timed(None)
        self.st = torch.cuda.current_stream(dev).cuda_stream
        self.spare = torch.zeros(2, dtype=torch.float64, device=dev)                # an empty array's address

    def ptr(self, t):
        return _ptr(t, self.spare)

    def up(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def new(self, n, dtype, fill=None):
        import torch
        if fill is None:
            return torch.empty(max(int(n), 1), dtype=dtype, device=self.dev)
        return torch.full((max(int(n), 1),), fill, dtype=dtype, device=self.dev)

    def call(self, module, name, *args):
        """``name`` of the library bound in ``module`` on the front's stream, through the per-call hook."""
        self.run(name, _call, module, name, *args, self.st)

    def similarity(self, entry, gt_boxes, tr_boxes, g_off, t_off):
        """``entry``, a (module, name) pair with ``trackeval_similarity``'s arguments, over the frames behind the host
        offsets: (similarity, the uploaded ground-truth, tracker and similarity offsets, the similarity's length)."""
        import torch
        s_off = _sim_offsets(g_off, t_off)
        sim = self.new(s_off[-1], torch.float64)
        offs = self.up(g_off), self.up(t_off), self.up(s_off)
        self.call(*entry, self.ptr(gt_boxes), self.ptr(tr_boxes), self.ptr(offs[0]), self.ptr(offs[1]),
                  self.ptr(offs[2]), len(g_off) - 1, self.ptr(sim))
        return sim, offs, int(s_off[-1])


def _front_tables(fr: DeviceFront, entry, host: PackedSequences, keep_gt, keep_tr, gt_boxes, tr_boxes,
                  check_ids=None) -> DeviceFront:
    """The second half of a front, from the keep masks on: ``_compact`` on the host (small integer arrays; not hot), the
    kept boxes, their similarity by ``entry``, the relabelled ids on the device.  ``keep_gt`` None: all ground truth
    stays and ``gt_boxes`` is taken as it is.  ``check_ids(ids per sequence)`` may raise before anything more is
    launched."""
    gather_gt = keep_gt is not None
    fr.host, fr.d = host, _compact(host, keep_gt if gather_gt else np.ones(len(host.gt_ids), bool), keep_tr)
    d, up = fr.d, fr.up
    if gather_gt:
        gt_boxes = gt_boxes[up(d["keep_gt"])].contiguous()
    tr_boxes = tr_boxes[up(d["keep_tr"])].contiguous()
    fr.S, fr.F = len(host.seq_off) - 1, len(host.gt_off) - 1
    fr.max_gt, fr.max_tr = _frame_max(d["gt_off"]), _frame_max(d["tr_off"])
    n_ids = d["n_gt_ids"].astype(np.int64) + d["n_tr_ids"]
    fr.max_gt_ids, fr.max_side = _most(d["n_gt_ids"]), _most(np.maximum(d["n_gt_ids"], d["n_tr_ids"]))
    fr.max_ids = _most(n_ids)
    if check_ids is not None:
        check_ids(n_ids)
    fr.sim, (fr.gt_off, fr.tr_off, fr.sim_off), fr.n_sim = fr.similarity(entry, gt_boxes, tr_boxes, d["gt_off"],
                                                                         d["tr_off"])
    fr.gt_ids, fr.tr_ids = up(d["gt_ids"]), up(d["tr_ids"])
    fr.seq_off, fr.n_gt_ids = up(host.seq_off), up(d["n_gt_ids"])
    fr.cells, fr.n_gid, fr.n_tid = int(d["cell_off"][-1]), int(d["gid_off"][-1]), int(d["tid_off"][-1])
    return fr


def device_front(packed: PackedSequences, benchmark: str, run=None, on_host: str = None) -> DeviceFront:
    """``_preprocess_host`` by the kernels of libtrack_eval_hip.so, on the current stream; ``packed`` holds CUDA tensors.
    The one statement of what ``device_tables``, ``diagnose._device_rows`` and
    ``association.device_association_tables`` start with: the raw similarity; under MOT17 rules one assignment per frame
    that flags the detections on distractors (``trackeval_preproc_match``); the filters and the relabelling on the host,
    which waits for the device; the similarity of what is kept.  ``run``: the per-call hook (``_timed``) every library
    call goes through.  ``on_host``: what the caller's error advises ("evaluate", "analyse") for a sequence whose
    identity assignment exceeds the device limit; None where no launch behind the front solves one."""
    import torch
    from . import _track_eval_lib as L
    fr = DeviceFront(packed.gt_boxes.device, run)
    ptr, entry = fr.ptr, (L, "trackeval_similarity")
    seq_off, gt_off, tr_off = (getattr(packed, k).cpu().numpy() for k in ("seq_off", "gt_off", "tr_off"))
    F = len(gt_off) - 1
    fr.tens = tens = {k: getattr(packed, k).contiguous() for k in PackedSequences.ARRAYS}
    fr.raw_sim, (d_gt_off, d_tr_off, d_sim_off), fr.n_raw = fr.similarity(entry, tens["gt_boxes"], tens["tr_boxes"],
                                                                          gt_off, tr_off)
    n_tr = tens["tr_ids"].numel()
    remove = fr.new(n_tr, torch.int32, 0)
    if benchmark != "MOT15" and F:
        status = fr.new(F, torch.int32, 0)
        fr.call(L, "trackeval_preproc_match", ptr(fr.raw_sim), ptr(d_sim_off), ptr(d_gt_off), ptr(d_tr_off),
                ptr(tens["gt_classes"]), F, _frame_max(gt_off), _frame_max(tr_off), ptr(remove), ptr(status))
        _raise_on_status(status, "preprocessing match", "frame")
    host = PackedSequences(packed.names, seq_off, gt_off, tr_off, None, None, tens["gt_ids"].cpu().numpy(),
                           tens["tr_ids"].cpu().numpy(), tens["gt_classes"].cpu().numpy(),
                           tens["gt_zero_marked"].cpu().numpy())
    keep_gt = host.gt_zero_marked != 0
    if benchmark != "MOT15":
        keep_gt &= host.gt_classes == PEDESTRIAN

    def check_ids(n_ids):
        if on_host and _most(n_ids) > L.MAX_DIM:
            raise ValueError(f"a sequence has {_most(n_ids)} ground-truth plus tracker ids: the identity assignment "
                             f"exceeds the device limit of {L.MAX_DIM} ({on_host} it on the host)")

    return _front_tables(fr, entry, host, keep_gt, remove[:n_tr].cpu().numpy() == 0, tens["gt_boxes"],
                         tens["tr_boxes"], check_ids)


def device_accumulate(fr: DeviceFront) -> dict:
    """``trackeval_accumulate`` over a front's kept detections, with its set-up: the front gets the id tables on the
    device (``n_tr_ids``, ``cell_off``, ``gid_off``, ``tid_off``, ``frame_seq``), which only the launches behind this one
    read; returned are ``potential``, ``alignment`` float64 and ``id_matches`` int32 [cells], ``gt_count`` [n_gid],
    ``tr_count`` [n_tid] int32.  Unguarded: with no sequence the entry point launches nothing, and the five arrays are
    empty behind their one element."""
    import torch
    from . import _track_eval_lib as L
    d, ptr, up = fr.d, fr.ptr, fr.up
    fr.n_tr_ids = up(d["n_tr_ids"])
    fr.cell_off, fr.gid_off, fr.tid_off = up(d["cell_off"]), up(d["gid_off"]), up(d["tid_off"])
    fr.frame_seq = up(np.repeat(np.arange(fr.S, dtype=np.int32), np.diff(fr.host.seq_off)))
    acc = {"potential": fr.new(fr.cells, torch.float64), "alignment": fr.new(fr.cells, torch.float64),
           "id_matches": fr.new(fr.cells, torch.int32), "gt_count": fr.new(fr.n_gid, torch.int32),
           "tr_count": fr.new(fr.n_tid, torch.int32)}
    fr.call(L, "trackeval_accumulate", ptr(fr.sim), ptr(fr.sim_off), ptr(fr.gt_off), ptr(fr.tr_off), ptr(fr.gt_ids),
            ptr(fr.tr_ids), ptr(fr.seq_off), fr.S, ptr(fr.n_gt_ids), ptr(fr.n_tr_ids), ptr(fr.cell_off),
            ptr(fr.gid_off), ptr(fr.tid_off), fr.max_gt, fr.max_tr, ptr(acc["potential"]), ptr(acc["id_matches"]),
            ptr(acc["gt_count"]), ptr(acc["tr_count"]), ptr(acc["alignment"]))
    return acc


def _metric_tables(fr: DeviceFront, frame: str = "frame", sequence: str = "sequence") -> dict:
    """The metric stage behind a front, its ``S`` sequences being whatever the front made them (BDD100K's are
    (sequence, class) pairs): accumulate, HOTA match and reduce, CLEAR, Identity; ``device_tables``' dictionary.
    ``frame`` / ``sequence``: what an error calls them."""
    import torch
    from . import _track_eval_lib as L
    S, F, dev, d, ptr, new = fr.S, fr.F, fr.dev, fr.d, fr.ptr, fr.new
    n_alpha = len(ALPHAS)
    acc = device_accumulate(fr)
    matches = new(n_alpha * fr.cells, torch.int32, 0)
    tp, loc = new(F * n_alpha, torch.int32), new(F * n_alpha, torch.float64)
    frame_status = new(F, torch.int32, 0)
    alphas = np.ascontiguousarray(ALPHAS, np.float64)
    fr.call(L, "trackeval_hota_match", ptr(fr.sim), ptr(fr.sim_off), ptr(fr.gt_off), ptr(fr.tr_off), ptr(fr.gt_ids),
            ptr(fr.tr_ids), ptr(fr.frame_seq), F, ptr(fr.n_tr_ids), ptr(fr.cell_off), ptr(acc["alignment"]),
            alphas.ctypes.data, fr.max_gt, fr.max_tr, ptr(matches), ptr(tp), ptr(loc), ptr(frame_status))
    hota_tp = torch.zeros((S, n_alpha), dtype=torch.int64, device=dev)
    hota_sums = torch.zeros((S, 4, n_alpha), dtype=torch.float64, device=dev)
    fr.call(L, "trackeval_hota_reduce", ptr(fr.seq_off), S, ptr(fr.n_gt_ids), ptr(fr.n_tr_ids), ptr(fr.cell_off),
            ptr(fr.gid_off), ptr(fr.tid_off), ptr(acc["gt_count"]), ptr(acc["tr_count"]), ptr(matches), ptr(tp),
            ptr(loc), ptr(hota_tp), ptr(hota_sums))
    clear_ints = torch.zeros((S, 8), dtype=torch.int32, device=dev)
    motp_sum = torch.zeros(S, dtype=torch.float64, device=dev)
    clear_status, id_status = new(S, torch.int32, 0), new(S, torch.int32, 0)
    fr.call(L, "trackeval_clear", ptr(fr.sim), ptr(fr.sim_off), ptr(fr.gt_off), ptr(fr.tr_off), ptr(fr.gt_ids),
            ptr(fr.tr_ids), ptr(fr.seq_off), S, ptr(fr.n_gt_ids), fr.max_gt, fr.max_tr, fr.max_gt_ids,
            ptr(clear_ints), ptr(motp_sum), ptr(clear_status))
    identity = torch.zeros((S, 2), dtype=torch.int64, device=dev)
    fr.call(L, "trackeval_identity", S, ptr(fr.n_gt_ids), ptr(fr.n_tr_ids), ptr(fr.cell_off), ptr(fr.gid_off),
            ptr(fr.tid_off), ptr(acc["gt_count"]), ptr(acc["tr_count"]), ptr(acc["id_matches"]), fr.max_ids,
            ptr(identity), ptr(id_status))
    _raise_on_status(frame_status, "HOTA match", frame)
    _raise_on_status(clear_status[:S], "CLEAR", sequence)
    _raise_on_status(id_status[:S], "Identity", sequence)
    return {"raw_similarity": fr.raw_sim[:fr.n_raw], "similarity": fr.sim[:fr.n_sim], "hota_tp": hota_tp,
            "hota_sums": hota_sums, "clear_ints": clear_ints.long(), "motp_sum": motp_sum, "identity": identity,
            "gt_off": fr.gt_off, "tr_off": fr.tr_off, "gt_ids": fr.gt_ids, "tr_ids": fr.tr_ids,
            "n_gt_ids": fr.n_gt_ids, "n_tr_ids": fr.n_tr_ids, "n_gt_dets": fr.up(d["n_gt_dets"]),
            "n_tr_dets": fr.up(d["n_tr_dets"]), "potential": acc["potential"][:fr.cells],
            "alignment": acc["alignment"][:fr.cells], "id_matches": acc["id_matches"][:fr.cells],
            "matches": matches[:n_alpha * fr.cells]}


def device_tables(packed: PackedSequences, benchmark: str = "MOT17", stream=None, timings: dict = None) -> dict:
    """``host_tables`` by the kernels of libtrack_eval_hip.so; ``packed`` holds CUDA tensors.  Launches on ``stream``
    (default: the current one).  Returns torch tensors on the device, plus the intermediate tables (``potential``,
    ``alignment``, ``matches``, ``id_matches``) of the preprocessed data.  ``timings``: a dict that receives, per
    library call, a list of (start, end) event pairs around its launches (tools/bench_eval.py)."""
    with _on_stream(packed.gt_boxes.device, stream):
        return _metric_tables(device_front(packed, benchmark, _timed(timings), on_host="evaluate"))


def _raise_on_status(status, what: str, unit: str) -> None:
    bad = status.nonzero()
    if bad.numel():
        i = int(bad[0])
        code = int(status[i])
        why = "exceeds the size the launch was made for" if code == -2 else "has no feasible assignment"
        raise RuntimeError(f"{what}: {unit} {i} {why} (status {code})")


# ------------------------------------------------------------------------------------------- tables -> the fields
def _hota_final(res: dict) -> dict:
    tp, fn, fp = res["HOTA_TP"], res["HOTA_FN"], res["HOTA_FP"]
    res["DetRe"] = tp / np.maximum(1, tp + fn)
    res["DetPr"] = tp / np.maximum(1, tp + fp)
    res["DetA"] = tp / np.maximum(1, tp + fn + fp)
    res["HOTA"] = np.sqrt(res["DetA"] * res["AssA"])
    res["RHOTA"] = np.sqrt(res["DetRe"] * res["AssA"])
    res["HOTA(0)"], res["LocA(0)"] = res["HOTA"][0], res["LocA"][0]
    res["HOTALocA(0)"] = res["HOTA(0)"] * res["LocA(0)"]
    return res


def _clear_final(res: dict) -> dict:
    tp, fn, fp, idsw = res["CLR_TP"], res["CLR_FN"], res["CLR_FP"], res["IDSW"]
    n_ids = res["MT"] + res["ML"] + res["PT"]
    res["MTR"], res["MLR"], res["PTR"] = (res[k] / np.maximum(1.0, n_ids) for k in ("MT", "ML", "PT"))
    res["CLR_Re"] = tp / np.maximum(1.0, tp + fn)
    res["CLR_Pr"] = tp / np.maximum(1.0, tp + fp)
    res["MODA"] = (tp - fp) / np.maximum(1.0, tp + fn)
    res["MOTA"] = (tp - fp - idsw) / np.maximum(1.0, tp + fn)
    res["MOTP"] = res["MOTP_sum"] / np.maximum(1.0, tp)
    res["sMOTA"] = (res["MOTP_sum"] - fp - idsw) / np.maximum(1.0, tp + fn)
    res["CLR_F1"] = tp / np.maximum(1.0, tp + 0.5 * fn + 0.5 * fp)
    res["FP_per_frame"] = fp / np.maximum(1.0, res["CLR_Frames"])
    res["MOTAL"] = (tp - fp - (np.log10(idsw) if idsw > 0 else idsw)) / np.maximum(1.0, tp + fn)
    return res


def _identity_final(res: dict) -> dict:
    tp, fn, fp = res["IDTP"], res["IDFN"], res["IDFP"]
    res["IDR"] = tp / np.maximum(1.0, tp + fn)
    res["IDP"] = tp / np.maximum(1.0, tp + fp)
    res["IDF1"] = tp / np.maximum(1.0, tp + 0.5 * fp + 0.5 * fn)
    return res


def _sequence_result(n_frames, n_gt_dets, n_tr_dets, n_gt_ids, n_tr_ids, hota_tp, hota_sums, clear_ints, motp_sum,
                     identity) -> dict:
    """TrackEval's fields of one sequence from its tables.  A sequence without tracker detections, or without ground
    truth, gets the fixed values the metrics return for it (everything missed, or everything false; LocA 1, MLR 1)."""
    n = len(ALPHAS)
    n_gt_dets, n_tr_dets, n_gt_ids, n_tr_ids = int(n_gt_dets), int(n_tr_dets), int(n_gt_ids), int(n_tr_ids)
    res = {k: np.zeros(n) for k in HOTA_FLOAT_ARRAYS + HOTA_INT_ARRAYS}
    res.update({k: 0 for k in HOTA_FLOATS + CLEAR_FLOATS + IDENTITY_FLOATS + CLEAR_INTS + IDENTITY_INTS})
    res.update(Dets=n_tr_dets, GT_Dets=n_gt_dets, IDs=n_tr_ids, GT_IDs=n_gt_ids)
    if n_tr_dets == 0 or n_gt_dets == 0:
        res["LocA"], res["LocA(0)"], res["MLR"] = np.ones(n), 1.0, 1.0
        if n_tr_dets == 0:
            res["HOTA_FN"] = n_gt_dets * np.ones(n)
            res["CLR_FN"], res["ML"], res["IDFN"] = n_gt_dets, n_gt_ids, n_gt_dets
        else:
            res["HOTA_FP"] = n_tr_dets * np.ones(n)
            res["CLR_FP"], res["IDFP"] = n_tr_dets, n_tr_dets
        return res
    tp = np.asarray(hota_tp, np.float64)
    res["HOTA_TP"], res["HOTA_FN"], res["HOTA_FP"] = tp, n_gt_dets - tp, n_tr_dets - tp
    res["AssA"], res["AssRe"], res["AssPr"] = (hota_sums[i] / np.maximum(1, tp) for i in range(3))
    res["LocA"] = np.maximum(1e-10, hota_sums[3]) / np.maximum(1e-10, tp)
    _hota_final(res)
    res.update({k: int(v) for k, v in zip(CLEAR_INTS[:8], clear_ints)})
    res["MOTP_sum"], res["CLR_Frames"] = float(motp_sum), int(n_frames)
    _clear_final(res)
    res["IDFN"], res["IDFP"] = int(identity[0]), int(identity[1])
    res["IDTP"] = n_gt_dets - res["IDFN"]
    _identity_final(res)
    return res


def combine_sequences(results: Dict[str, dict]) -> dict:
    """The fields of all sequences together: counts add up, the association scores and LocA are averaged with HOTA_TP
    as weight, and every ratio is formed again from the totals."""
    seqs = list(results.values())
    total = lambda k: sum([r[k] for r in seqs])                                    # noqa: E731
    res = {k: total(k) for k in HOTA_INT_ARRAYS + CLEAR_INTS + IDENTITY_INTS + COUNT_INTS + ("MOTP_sum",)}
    for k in ("AssRe", "AssPr", "AssA"):
        res[k] = sum([r[k] * r["HOTA_TP"] for r in seqs]) / np.maximum(1.0, res["HOTA_TP"])
    res["LocA"] = np.maximum(1e-10, sum([r["LocA"] * r["HOTA_TP"] for r in seqs])) / np.maximum(1e-10, res["HOTA_TP"])
    return _identity_final(_clear_final(_hota_final(res)))


def summary(result: dict) -> Dict[str, float]:
    """Names and values of ``pedestrian_summary.txt`` in its order: float fields in percent with five significant
    digits (HOTA's arrays averaged over the thresholds), integer fields as they are."""
    out = {}
    for k in SUMMARY_FIELDS:
        if k in INT_FIELDS:
            out[k] = int(result[k])
        else:
            out[k] = float("{0:1.5g}".format(100 * float(np.mean(result[k]))))
    return out


# ---------------------------------------------------------------------------------------------------- entry points
def evaluate_packed(packed: PackedSequences, benchmark: str = "MOT17", device=None, stream=None) -> Dict[str, dict]:
    """``{name: fields, ..., "COMBINED_SEQ": fields}``.  ``device``: a CUDA device for the kernels; "cpu" or None (the
    default) for the host statement, to which device tensors are copied."""
    if benchmark not in ("MOT17", "MOT15"):
        raise ValueError(f"benchmark {benchmark!r} is not supported (MOT17 rules, or MOT15 for no preprocessing match)")
    if not packed.names:
        raise ValueError("no sequence to evaluate")
    on_device = device is not None and str(device).startswith("cuda")
    if on_device:
        t = device_tables(packed if packed.is_device() else packed.to(device), benchmark, stream=stream)
        keys = ("n_gt_dets", "n_tr_dets", "n_gt_ids", "n_tr_ids", "hota_tp", "hota_sums", "clear_ints", "motp_sum",
                "identity")
        t = dict(zip(keys, (t[k].cpu().numpy() for k in keys)))                   # (synchronises)
        seq_off = packed.seq_off.cpu().numpy() if packed.is_device() else packed.seq_off
    else:
        t, seq_off = host_tables(packed, benchmark), packed.numpy().seq_off
    res = {name: _sequence_result(seq_off[s + 1] - seq_off[s], t["n_gt_dets"][s], t["n_tr_dets"][s], t["n_gt_ids"][s],
                                  t["n_tr_ids"][s], t["hota_tp"][s], t["hota_sums"][s], t["clear_ints"][s],
                                  t["motp_sum"][s], t["identity"][s]) for s, name in enumerate(packed.names)}
    res["COMBINED_SEQ"] = combine_sequences(res)
    return res


def evaluate_sequences(sequences: Dict[str, dict], benchmark: str = "MOT17", device=None) -> Dict[str, dict]:
    """Evaluate ``{name: per-frame lists}`` (see ``pack_sequences``).  A CUDA ``device`` selects the kernels; the
    default is the host statement."""
    return evaluate_packed(pack_sequences(sequences), benchmark, device=device)


class TrackingEvaluator:
    """Collects ground truth and tracker output frame by frame, then evaluates all sequences in one call."""

    def __init__(self, benchmark: str = "MOT17", device=None):
        self.benchmark, self.device = benchmark, device
        self._gt: Dict[str, dict] = {}
        self._tr: Dict[str, dict] = {}
        self._length: Dict[str, int] = {}

    def set_length(self, seq: str, n_frames: int) -> None:
        """Number of frames of ``seq`` (``seqLength``); default: the last frame anything was added for."""
        self._length[seq] = int(n_frames)

    def add_ground_truth(self, seq: str, frame: int, ids, boxes_xywh, classes=None, zero_marked=None) -> None:
        """Ground truth of the 1-based ``frame`` (the first column of gt.txt).  ``classes`` defaults to pedestrian,
        ``zero_marked`` (the "consider this entry" flag, column 7 of gt.txt) to 1."""
        ids = _host_array(ids, np.int64).reshape(-1)
        self._gt.setdefault(seq, {})[int(frame)] = (
            ids, _host_array(boxes_xywh, np.float64).reshape(-1, 4),
            np.ones(len(ids), np.int32) if classes is None else _host_array(classes, np.int32).reshape(-1),
            np.ones(len(ids), np.int32) if zero_marked is None else _host_array(zero_marked, np.int32).reshape(-1))

    def add_frame(self, seq: str, frame_idx: int, result) -> None:
        """Tracker output of the 0-based ``frame_idx``: what ``SequenceTracker.step`` / ``step_raw`` / ``track`` return
        (``ids``, ``boxes`` as xyxy pixels).  The boxes become the doubles ``mot_lines`` would print and TrackEval
        would read back: ``x1, y1, x2 - x1, y2 - y1`` in Python floats."""
        boxes = [[x1, y1, x2 - x1, y2 - y1] for x1, y1, x2, y2 in result.boxes.tolist()]
        self._tr.setdefault(seq, {})[int(frame_idx) + 1] = (
            np.asarray(result.ids.tolist(), np.int64).reshape(-1), np.asarray(boxes, np.float64).reshape(-1, 4))

    def add_tracker_rows(self, seq: str, frame: int, ids, boxes_xywh) -> None:
        """Tracker output of the 1-based ``frame`` as ids and xywh boxes (a result file's columns)."""
        self._tr.setdefault(seq, {})[int(frame)] = (_host_array(ids, np.int64).reshape(-1),
                                                    _host_array(boxes_xywh, np.float64).reshape(-1, 4))

    def sequences(self) -> Dict[str, dict]:
        out = {}
        none_i, none_b = np.zeros(0, np.int64), np.zeros((0, 4))
        for seq in list(self._gt) + [s for s in self._tr if s not in self._gt]:
            gt, tr = self._gt.get(seq, {}), self._tr.get(seq, {})
            T = self._length.get(seq, max(list(gt) + list(tr) + [0]))
            bad = [f for f in list(gt) + list(tr) if f < 1 or f > T]
            if bad:
                raise ValueError(f"sequence {seq}: frame {bad[0]} is outside 1 .. {T}")
            rows = [gt.get(f, (none_i, none_b, none_i, none_i)) for f in range(1, T + 1)]
            trk = [tr.get(f, (none_i, none_b)) for f in range(1, T + 1)]
            out[seq] = {"gt_ids": [r[0] for r in rows], "gt_boxes": [r[1] for r in rows],
                        "gt_classes": [r[2] for r in rows], "gt_zero_marked": [r[3] for r in rows],
                        "tracker_ids": [r[0] for r in trk], "tracker_boxes": [r[1] for r in trk]}
        return out

    def evaluate(self) -> Dict[str, dict]:
        return evaluate_sequences(self.sequences(), self.benchmark, device=self.device if self.device else "cpu")

    def events(self) -> Dict[str, object]:
        """``{name: diagnose.SequenceEvents}`` of what was collected: the decisions behind CLEAR's counts, per row."""
        from .diagnose import clear_events
        return clear_events(pack_sequences(self.sequences()), self.benchmark, device=self.device)

    def association(self, alpha_index: int = 9) -> Dict[str, object]:
        """``{name: association.SequenceAssociation}`` of what was collected: HOTA's matches per row, the per-identity
        association scores and the Identity metric's map."""
        from .association import association
        return association(pack_sequences(self.sequences()), self.benchmark, device=self.device,
                           alpha_index=alpha_index)


# ------------------------------------------------------------------------------------------------------ text files
def read_mot_txt(path: str) -> np.ndarray:
    """The rows of a MOT-format text file (``frame,id,x,y,w,h,conf,class,visibility...``; gt.txt or a tracker's
    result file) as a float64 array, one row per line; columns missing in the file are filled with -1 up to 8."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line:
                rows.append([float(x) for x in (line.split(",") if "," in line else line.split())])
    width = max([8] + [len(r) for r in rows])
    out = np.full((len(rows), width), -1.0)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _rows_by_frame(rows: np.ndarray):
    frames = rows[:, 0].astype(np.int64)
    return {int(f): rows[frames == f] for f in np.unique(frames)}


def load_files(gt_root: str, tracker_dir: str, seqmap: str, benchmark: str = "MOT17", device=None) -> TrackingEvaluator:
    """A ``TrackingEvaluator`` holding result files in the layout ``eval_engine.py`` hands to TrackEval: ground truth in
    ``<gt_root>/<seq>/gt/gt.txt`` (length from ``<gt_root>/<seq>/seqinfo.ini`` where it exists), results in
    ``<tracker_dir>/<seq>.txt``, sequence names in ``seqmap`` (one per line under a ``name`` header)."""
    with open(seqmap) as f:
        names = [ln.strip() for ln in f if ln.strip()]
    if names and names[0] == "name":
        names = names[1:]
    ev = TrackingEvaluator(benchmark, device)
    for seq in names:
        gt = read_mot_txt(os.path.join(gt_root, seq, "gt", "gt.txt"))
        tr = read_mot_txt(os.path.join(tracker_dir, seq + ".txt"))
        length = _seq_length(os.path.join(gt_root, seq, "seqinfo.ini"))
        ev.set_length(seq, length if length else int(max([0] + list(gt[:, 0]) + list(tr[:, 0]))))
        for f, r in _rows_by_frame(gt).items():
            ev.add_ground_truth(seq, f, r[:, 1].astype(np.int64), r[:, 2:6], r[:, 7].astype(np.int64),
                                r[:, 6].astype(np.int64))
        for f, r in _rows_by_frame(tr).items():
            ev.add_tracker_rows(seq, f, r[:, 1].astype(np.int64), r[:, 2:6])
        ev._gt.setdefault(seq, {})
    return ev


def evaluate_files(gt_root: str, tracker_dir: str, seqmap: str, benchmark: str = "MOT17", device=None) -> Dict[str, dict]:
    """Score the result files ``load_files`` reads."""
    return load_files(gt_root, tracker_dir, seqmap, benchmark, device).evaluate()


def _seq_length(ini_path: str) -> Optional[int]:
    if not os.path.exists(ini_path):
        return None
    import configparser
    ini = configparser.ConfigParser()
    ini.read(ini_path)
    return int(ini["Sequence"]["seqLength"])


# ------------------------------------------------------------------------------------------------- synthetic data
def synthetic_sequence(seed: int, n_frames: int, n_objects: int, *, n_distractors: int = 0, miss: float = 0.1,
                       n_false: int = 1, switch: float = 0.02, noise: float = 0.04, gap: float = 0.03,
                       exact: float = 0.1, zero_marked: float = 0.0, track=None) -> dict:
    """A sequence of per-frame lists (``pack_sequences``' input) for tests and ``tools/bench_eval.py``: ``n_objects``
    pedestrians and ``n_distractors`` objects of the distractor classes on random walks; ground truth leaves for
    stretches of frames (``gap``: chance per frame to start one) and returns; the tracker reports noisy copies
    (``exact``: share of exact copies, IoU 1), misses some (``miss``), adds ``n_false`` boxes per frame that belong to
    nothing, and renames a track now and then (``switch``).  ``track``: indices of the objects the tracker follows at
    all (default: all of them)."""
    rng = np.random.RandomState(seed)
    n = n_objects + n_distractors
    pos = rng.uniform(0, 1500, (n, 2))
    size = rng.uniform(40, 160, (n, 2))
    cls = np.concatenate([np.ones(n_objects, np.int64), rng.choice(DISTRACTOR_CLASSES, n_distractors)]).astype(np.int64)
    name = 1000 + np.arange(n)                         # the tracker's id of each object, renamed on a switch
    next_name, away = 1000 + n, np.zeros(n, np.int64)
    followed = np.ones(n, bool) if track is None else np.isin(np.arange(n), track)
    seq = {k: [] for k in ("gt_ids", "gt_boxes", "gt_classes", "gt_zero_marked", "tracker_ids", "tracker_boxes")}
    for _ in range(n_frames):
        pos += rng.normal(0, 6, (n, 2))
        away = np.where(away > 0, away - 1, np.where(rng.uniform(size=n) < gap, rng.randint(1, 6, n), 0))
        here = away == 0
        boxes = np.concatenate([pos - size / 2, size], 1)
        seq["gt_ids"].append(np.flatnonzero(here) + 1)
        seq["gt_boxes"].append(boxes[here])
        seq["gt_classes"].append(cls[here])
        seq["gt_zero_marked"].append((rng.uniform(size=int(here.sum())) >= zero_marked).astype(np.int64))
        for i in np.flatnonzero(rng.uniform(size=n) < switch):
            name[i], next_name = next_name, next_name + 1
        seen = here & followed & (rng.uniform(size=n) >= miss)
        jitter = rng.normal(0, noise, (n, 4)) * np.concatenate([size, size], 1)
        jitter[rng.uniform(size=n) < exact] = 0
        false = np.concatenate([rng.uniform(0, 1500, (n_false, 2)), rng.uniform(40, 160, (n_false, 2))], 1)
        seq["tracker_ids"].append(np.concatenate([name[seen], 500000 + rng.permutation(4 * n_false + 1)[:n_false]]))
        seq["tracker_boxes"].append(np.concatenate([(boxes + jitter)[seen], false]))
    return seq
