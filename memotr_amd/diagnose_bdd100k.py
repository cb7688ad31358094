"""Error analysis for BDD100K: the decisions behind the per-class CLEAR counts of ``evaluation_bdd100k.py``, per input
row, and the boxes the eight per-class problems cannot see together: a car that is tracked perfectly but labelled
``truck`` costs one CLR_FN in ``car`` and one CLR_FP in ``truck``; here the two rows point at each other.

    events = bdd_events_from_files(gt_dir, tracker_dir, device="cuda")          # evaluate_bdd_files' arguments
    ev = events["b1c66a42"]
    ev.counts()["car"]       # {"CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "Frag"}: evaluate_bdd_files(...)["b1c66a42"]["car"]'s
    ev.confusions(10)        # [("car", "truck", 41), ...]: ground truth of one class under a tracker box of another
    ev.ignored()             # [(frame, tracker_id, class), ...]: the boxes the metric never saw
    ev.switches("car")       # [(frame, gt_id, tracker_id_before, tracker_id_now), ...]
    ev.write_csv("events/b1c66a42.csv")
    write_error_frames(ev.as_sequence_events(), frame_paths, "errors/b1c66a42", device="cuda")     # diagnose.py's

    python -m memotr_amd.diagnose_bdd100k --gt-dir G --tracker-dir T --out DIR [--frames-root R --only-errors]

Frames are numbered from 0 wherever this module names one (``switches``, ``worst_frames``, ``ignored``, the CSV): the
frame index of ``BDD100KEvaluator.add_ground_truth``.  (``as_sequence_events`` hands the rows to ``diagnose.py``, whose
file names count from 1.)

Kinds, per class.  The rows of a frame are cut into the eight evaluated classes (``class_split_host``) and every
(sequence, class) pair is walked as ``diagnose._walk_host`` walks a sequence, after BDD100K's preprocessing
(``evaluation_bdd100k._preprocess_host``).  A ground-truth row is MATCH, SWITCH or MISS; a tracker row TP, SWITCH, FP
or IGNORED.  IGNORED means "the metric never saw this row": a tracker row that was unmatched and lay more than half
inside a crowd or distractor region, or a row of either side whose category is none of the eight.  BDD100K removes
nothing else from the ground truth, and ``BDD100KEvaluator`` turns distractor rows into ignore regions before they are
rows at all, so a ground-truth row is IGNORED only when ``pack_bdd`` was handed a class id outside the eight directly.

Cross-class pairs, per input frame.  The candidates are the MISS rows and the FP rows (never an IGNORED one).  A pair is
admissible when the two classes differ and the box IoU is at least 0.5 (``sim < THRESHOLD - EPS -> 0``, accepted when
the score is ``> EPS``, as everywhere); one linear assignment per frame maximises the summed IoU, its pairs are scipy's.
``kind`` stays MISS / FP -- the five counts stay the evaluator's -- and each side records ``cross_partner`` (index
within the frame, -1), ``cross_class`` (the partner's class index, -1) and ``cross_iou`` (0.0).  Pairs of one class
are left out on purpose: a MISS and an FP of the same class at IoU >= 0.5 cannot both survive that class's assignment
(matching them would have raised its sum), so there is none to find.

``confusion`` int64 [9, 9] per sequence, labels ``CLASSES + ("none",)``: ``[g, t]`` counts the cross-class pairs of
ground-truth class g under tracker class t, ``[c, c]`` is CLR_TP of class c, column 8 the MISS rows and row 8 the FP
rows without a cross partner.  Row g sums to the ground-truth detections of class g, column t to the kept tracker
detections of class t.

The definition is stated twice.  ``bdd_events_host`` is numpy and scipy.  With a CUDA ``device`` the class split, the
similarity and the preprocessing are ``evaluation_bdd100k.device_front_bdd``'s, the calls ``device_tables_bdd`` stands on
(here the split carries row numbers in place of ids, which gives the source row of every split row), ONE launch of
``clipops_clear_events_f64`` walks the S * 8 problems, and ``clipops_bdd_cross_class_f64`` (memotr_amd/csrc/clip_tracks.h)
pairs every frame, one wavefront each; the confusion matrix is an integer ``bincount``.  Integer results and IoUs agree
with the host statement exactly.

Out of scope: BDD100K association analysis, a colour of its own for confused boxes, the class-combined keys.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import diagnose as D
from . import evaluation as E
from . import evaluation_bdd100k as B
from .diagnose import COUNTS, FP, GT_KIND_NAMES, IGNORED, MATCH, MISS, SWITCH, TP, TR_KIND_NAMES  # noqa: F401
from .evaluation_bdd100k import CLASSES, N_CLASSES

NONE = N_CLASSES                                    # row / column 8 of a confusion matrix
LABELS = CLASSES + ("none",)
CROSS_MAX_DIM = 2048                                # CLIPOPS_EVENTS_MAX_DIM: candidates of one side of a frame
CSV_HEADER = "frame,side,id,class,x0,y0,x1,y1,kind,partner_id,iou,frag,cross_id,cross_class,cross_iou"
CLASS_ID_TO_NAME = {v: k for k, v in B.CLASS_NAME_TO_CLASS_ID.items()}
_CLASS_INDEX = np.full(max(B.CLASS_IDS) + 1, -1, np.int32)
_CLASS_INDEX[list(B.CLASS_IDS)] = np.arange(N_CLASSES)
ROW_KEYS = ("gt_kind", "gt_frag", "gt_partner", "gt_iou", "gt_cross_partner", "gt_cross_class", "gt_cross_iou",
            "tr_kind", "tr_partner", "tr_cross_partner", "tr_cross_class", "tr_cross_iou")


def class_index(class_ids):
    """TrackEval's class ids -> class index 0 .. 7 in ``CLASSES``' order, -1 for any other id.  numpy in, numpy out;
    a torch tensor in, a tensor on its device out."""
    if isinstance(class_ids, np.ndarray):
        c = class_ids.astype(np.int64)
        known = (c >= 0) & (c < len(_CLASS_INDEX))
        return np.where(known, _CLASS_INDEX[np.where(known, c, 0)], -1).astype(np.int32)
    import torch
    c = class_ids.long()
    table = torch.from_numpy(_CLASS_INDEX).to(c.device)
    known = (c >= 0) & (c < len(_CLASS_INDEX))
    return torch.where(known, table[c.clamp(0, len(_CLASS_INDEX) - 1)], -1).int()


def _class_name(class_id: int) -> str:
    return CLASS_ID_TO_NAME.get(int(class_id), str(int(class_id)))


def _class_arg(cls) -> int:
    if cls not in CLASSES:
        raise ValueError(f"class {cls!r} is none of {', '.join(CLASSES)}")
    return CLASSES.index(cls)


# ------------------------------------------------------------------------------------ the events of one sequence
@dataclass
class BDDSequenceEvents:
    """The rows of one sequence as ``PackedBDD`` holds them (offsets per frame, boxes x0, y0, x1, y1, TrackEval's class
    ids) and the event of every row, as host arrays."""
    name: str
    gt_off: np.ndarray              # int32 [F + 1]
    tr_off: np.ndarray              # int32 [F + 1]
    gt_ids: np.ndarray              # int32 [NG]
    gt_boxes: np.ndarray            # float64 [NG, 4]
    gt_classes: np.ndarray          # int32 [NG]
    gt_kind: np.ndarray             # int32 [NG]
    gt_frag: np.ndarray             # int32 [NG]: 1 where a track is picked up again (per class the sum is Frag)
    gt_partner: np.ndarray          # int32 [NG]: index within the frame's tracker rows, -1
    gt_iou: np.ndarray              # float64 [NG]: the pair's similarity, 0
    gt_cross_partner: np.ndarray    # int32 [NG]: index within the frame's tracker rows, -1
    gt_cross_class: np.ndarray      # int32 [NG]: the cross partner's class index, -1
    gt_cross_iou: np.ndarray        # float64 [NG]
    tr_ids: np.ndarray              # int32 [NT]
    tr_boxes: np.ndarray            # float64 [NT, 4]
    tr_classes: np.ndarray          # int32 [NT]
    tr_kind: np.ndarray             # int32 [NT]
    tr_partner: np.ndarray          # int32 [NT]: index within the frame's ground-truth rows, -1
    tr_cross_partner: np.ndarray    # int32 [NT]
    tr_cross_class: np.ndarray      # int32 [NT]
    tr_cross_iou: np.ndarray        # float64 [NT]
    class_counts: np.ndarray        # int32 [8, 5]: CLR_TP, CLR_FN, CLR_FP, IDSW, Frag per class
    confusion_matrix: np.ndarray    # int64 [9, 9]

    ARRAYS = ("gt_off", "tr_off", "gt_ids", "gt_boxes", "gt_classes") + ROW_KEYS[:7] + (
        "tr_ids", "tr_boxes", "tr_classes") + ROW_KEYS[7:] + ("class_counts", "confusion_matrix")

    @property
    def n_frames(self) -> int:
        return len(self.gt_off) - 1

    def counts(self) -> Dict[str, Dict[str, int]]:
        """``{class: {"CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "Frag"}}``: the evaluator's fields of this sequence."""
        return {cls: {k: int(v) for k, v in zip(COUNTS, self.class_counts[c])} for c, cls in enumerate(CLASSES)}

    def confusion(self) -> Tuple[np.ndarray, Tuple[str, ...]]:
        """The 9 x 9 matrix (ground truth down, tracker across) and its labels, ``CLASSES + ("none",)``."""
        return self.confusion_matrix, LABELS

    def confusions(self, n: int = 10) -> List[Tuple[str, str, int]]:
        """The ``n`` largest class confusions as (gt_class, tracker_class, count), largest first, ties by class order."""
        return _largest_confusions(self.confusion_matrix, n)

    def ignored(self) -> List[Tuple[int, int, str]]:
        """(frame, tracker_id, class) of every tracker row the metric never saw, in row order."""
        frame = np.repeat(np.arange(self.n_frames), np.diff(self.tr_off))
        return [(int(frame[j]), int(self.tr_ids[j]), _class_name(self.tr_classes[j]))
                for j in np.flatnonzero(self.tr_kind == IGNORED)]

    def frame_errors(self, cls: Optional[str] = None) -> np.ndarray:
        """int64 [F, 3]: misses, false positives and switches of every frame, of one class or of all."""
        g = np.ones(len(self.gt_ids), bool) if cls is None else class_index(self.gt_classes) == _class_arg(cls)
        t = np.ones(len(self.tr_ids), bool) if cls is None else class_index(self.tr_classes) == _class_arg(cls)
        per_frame = lambda flag, off: np.diff(np.concatenate(([0], np.cumsum(flag)))[off])          # noqa: E731
        return np.stack([per_frame(g & (self.gt_kind == MISS), self.gt_off),
                         per_frame(t & (self.tr_kind == FP), self.tr_off),
                         per_frame(g & (self.gt_kind == SWITCH), self.gt_off)], 1).astype(np.int64)

    def worst_frames(self, n: int = 10, cls: Optional[str] = None) -> List[Tuple[int, int, int, int]]:
        """The ``n`` frames with the most errors: (frame, FN, FP, IDSW), by FN + FP + IDSW, ties by frame."""
        e = self.frame_errors(cls)
        order = np.argsort(-e.sum(1), kind="stable")[:max(int(n), 0)]
        return [(int(f), int(e[f, 0]), int(e[f, 1]), int(e[f, 2])) for f in order]

    def switches(self, cls: Optional[str] = None) -> List[Tuple[int, int, int, int]]:
        """(frame, gt_id, tracker_id_before, tracker_id_now) of every SWITCH row of class ``cls`` (default: of every
        class), in row order.  An id is followed within its class, as the metric follows it."""
        want = None if cls is None else _class_arg(cls)
        ci = class_index(self.gt_classes)
        last, out = {}, []
        for f in range(self.n_frames):
            t0 = int(self.tr_off[f])
            for i in range(int(self.gt_off[f]), int(self.gt_off[f + 1])):
                if self.gt_partner[i] < 0 or (want is not None and ci[i] != want):
                    continue
                key, tid = (int(ci[i]), int(self.gt_ids[i])), int(self.tr_ids[t0 + self.gt_partner[i]])
                if self.gt_kind[i] == SWITCH:
                    out.append((f, key[1], last[key], tid))
                last[key] = tid
        return out

    def as_sequence_events(self, cls: Optional[str] = None) -> D.SequenceEvents:
        """The rows of class ``cls`` (default: all rows) as a ``diagnose.SequenceEvents``, boxes as x, y, w, h:
        what ``write_error_frames``, ``error_table_host`` and ``error_table_device`` draw.  (Those name frames from 1.)"""
        g = np.ones(len(self.gt_ids), bool) if cls is None else class_index(self.gt_classes) == _class_arg(cls)
        t = np.ones(len(self.tr_ids), bool) if cls is None else class_index(self.tr_classes) == _class_arg(cls)
        before_g, before_t = np.concatenate(([0], np.cumsum(g))), np.concatenate(([0], np.cumsum(t)))
        g_frame = np.repeat(np.arange(self.n_frames), np.diff(self.gt_off))
        t_frame = np.repeat(np.arange(self.n_frames), np.diff(self.tr_off))

        def partner(mine, mine_frame, other_off, before_other):
            # a partner is of the row's own class: it stays, at its rank among the frame's selected rows
            first = other_off[mine_frame].astype(np.int64)
            there = before_other[first + np.maximum(mine, 0)] - before_other[first]
            return np.where(mine >= 0, there, -1).astype(np.int32)

        xywh = lambda b: np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).reshape(-1, 4)     # noqa: E731
        name = self.name if cls is None else f"{self.name}/{cls}"
        return D.SequenceEvents(
            name, before_g[self.gt_off].astype(np.int32), before_t[self.tr_off].astype(np.int32), self.gt_ids[g],
            xywh(self.gt_boxes[g]), self.gt_kind[g], self.gt_frag[g],
            partner(self.gt_partner, g_frame, self.tr_off, before_t)[g], self.gt_iou[g], self.tr_ids[t],
            xywh(self.tr_boxes[t]), self.tr_kind[t], partner(self.tr_partner, t_frame, self.gt_off, before_g)[t])

    def write_csv(self, path: str) -> None:
        """One line per input row, ground truth before tracker rows within a frame (``CSV_HEADER``): the frame from 0,
        the class by name (a class id outside BDD100K's categories as the number), floats as Python prints them (they
        read back to the same bits); partner_id and cross_id -1, cross_class ``none`` and the IoUs 0 without a partner."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        lines = [CSV_HEADER]
        sides = {"gt": (self.gt_off, self.gt_ids, self.gt_boxes, self.gt_classes, self.gt_kind, self.gt_partner,
                        self.gt_cross_partner, self.gt_cross_class, self.gt_cross_iou, GT_KIND_NAMES),
                 "tr": (self.tr_off, self.tr_ids, self.tr_boxes, self.tr_classes, self.tr_kind, self.tr_partner,
                        self.tr_cross_partner, self.tr_cross_class, self.tr_cross_iou, TR_KIND_NAMES)}
        for f in range(self.n_frames):
            for side, other in (("gt", "tr"), ("tr", "gt")):
                off, ids, boxes, classes, kind, partner, cross, cross_class, cross_iou, names = sides[side]
                o0, other_ids = int(sides[other][0][f]), sides[other][1]
                g0 = int(self.gt_off[f])
                for i in range(int(off[f]), int(off[f + 1])):
                    p, x = int(partner[i]), int(cross[i])
                    iou = 0.0 if p < 0 else float(self.gt_iou[i if side == "gt" else g0 + p])
                    box = ",".join(repr(float(v)) for v in boxes[i])
                    lines.append(f"{f},{side},{int(ids[i])},{_class_name(classes[i])},{box},{names[int(kind[i])]},"
                                 f"{int(other_ids[o0 + p]) if p >= 0 else -1},{iou!r},"
                                 f"{int(self.gt_frag[i]) if side == 'gt' else 0},"
                                 f"{int(other_ids[o0 + x]) if x >= 0 else -1},{LABELS[int(cross_class[i])]},"
                                 f"{float(cross_iou[i])!r}")
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    @classmethod
    def read_csv(cls, path: str, name: Optional[str] = None, n_frames: Optional[int] = None) -> "BDDSequenceEvents":
        """What ``write_csv`` wrote.  ``n_frames``: the sequence's length where its last frames hold no row."""
        kinds = {"gt": {v: k for k, v in GT_KIND_NAMES.items()}, "tr": {v: k for k, v in TR_KIND_NAMES.items()}}
        rows = {"gt": [], "tr": []}
        with open(path) as fh:
            if fh.readline().strip() != CSV_HEADER:
                raise ValueError(f"{path}: not a BDD100K events file")
            for line in fh:
                c = line.strip().split(",")
                if len(c) == 15:
                    rows[c[1]].append(c)
        F = max([int(n_frames or 0)] + [int(c[0]) + 1 for side in rows.values() for c in side])
        a = {}
        for s in rows:
            a[s + "_off"] = np.concatenate(([0], np.cumsum(np.bincount([int(c[0]) for c in rows[s]], minlength=F)))
                                           ).astype(np.int32)
            a[s + "_ids"] = np.array([int(c[2]) for c in rows[s]], np.int32)
            a[s + "_classes"] = np.array([B.CLASS_NAME_TO_CLASS_ID[c[3]] if c[3] in B.CLASS_NAME_TO_CLASS_ID
                                          else int(c[3]) for c in rows[s]], np.int32)
            a[s + "_boxes"] = np.array([[float(v) for v in c[4:8]] for c in rows[s]], np.float64).reshape(-1, 4)
            a[s + "_kind"] = np.array([kinds[s][c[8]] for c in rows[s]], np.int32)
            a[s + "_cross_class"] = np.array([LABELS.index(c[13]) if c[13] != "none" else -1 for c in rows[s]], np.int32)
            a[s + "_cross_iou"] = np.array([float(c[14]) for c in rows[s]], np.float64)
        a["gt_iou"] = np.array([float(c[10]) for c in rows["gt"]], np.float64)
        a["gt_frag"] = np.array([int(c[11]) for c in rows["gt"]], np.int32)
        index = {s: class_index(a[s + "_classes"]) for s in rows}
        for s, o in (("gt", "tr"), ("tr", "gt")):
            a[s + "_partner"] = np.full(len(rows[s]), -1, np.int32)
            a[s + "_cross_partner"] = np.full(len(rows[s]), -1, np.int32)
            for r, c in enumerate(rows[s]):
                # an id names one row per frame and class: the partner has the row's class, the cross partner cross_class
                for key, column, want in (("_partner", 9, index[s][r]), ("_cross_partner", 12, a[s + "_cross_class"][r])):
                    if int(c[column]) >= 0:
                        o0, o1 = a[o + "_off"][int(c[0])], a[o + "_off"][int(c[0]) + 1]
                        hit = (a[o + "_ids"][o0:o1] == int(c[column])) & (index[o][o0:o1] == want)
                        a[s + key][r] = int(np.flatnonzero(hit)[0])
        a["class_counts"], a["confusion_matrix"] = _tables_of_rows(a)
        return cls(name or os.path.splitext(os.path.basename(path))[0], *[a[k] for k in cls.ARRAYS])


def _largest_confusions(matrix: np.ndarray, n: int) -> List[Tuple[str, str, int]]:
    pairs = [(int(matrix[g, t]), g, t) for g in range(N_CLASSES) for t in range(N_CLASSES) if g != t and matrix[g, t] > 0]
    pairs.sort(key=lambda x: (-x[0], x[1], x[2]))
    return [(CLASSES[g], CLASSES[t], v) for v, g, t in pairs[:max(int(n), 0)]]


def _tables_of_rows(a: dict):
    """(int32 [8, 5] counts, int64 [9, 9] confusion) of one sequence from the events of its rows."""
    import torch
    gc, tc = class_index(a["gt_classes"]), class_index(a["tr_classes"])
    per_class = lambda flag, c: np.bincount(c[flag & (c >= 0)], minlength=N_CLASSES)[:N_CLASSES]      # noqa: E731
    matched = (a["gt_kind"] == MATCH) | (a["gt_kind"] == SWITCH)
    counts = np.stack([per_class(matched, gc), per_class(a["gt_kind"] == MISS, gc), per_class(a["tr_kind"] == FP, tc),
                       per_class(a["gt_kind"] == SWITCH, gc), per_class(a["gt_frag"] != 0, gc)], 1).astype(np.int32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).long()                                 # noqa: E731
    zeros = lambda x: torch.zeros(len(x), dtype=torch.int64)                                       # noqa: E731
    conf = _confusion(1, zeros(gc), t(gc), t(a["gt_kind"]), t(a["gt_cross_class"]), zeros(tc), t(tc), t(a["tr_kind"]),
                      t(a["tr_cross_partner"]))
    return counts, conf[0].numpy()


# --------------------------------------------------------------------------------- the definition, on the host
def _rows_from_split(gt_off, tr_off, split: dict, rows: dict) -> dict:
    """The events of the problem-major rows (``diagnose._to_input_rows`` over a class split) scattered to the packed
    input rows through ``gt_src`` / ``tr_src``; a partner becomes an index within the packed frame.  Rows of no split
    frame stay IGNORED.  Torch tensors on one device (the host's, for the host statement); a few index operations."""
    import torch
    dev = rows["gt_kind"].device
    i64 = lambda x: torch.as_tensor(x, device=dev).long()                                       # noqa: E731
    gt_off, tr_off, s_gt_off, s_tr_off = i64(gt_off), i64(tr_off), i64(split["gt_off"]), i64(split["tr_off"])
    gt_src, tr_src, frame_src = i64(split["gt_src"]), i64(split["tr_src"]), i64(split["frame_src"])
    new = lambda n, fill, dt=torch.int32: torch.full((n,), fill, dtype=dt, device=dev)          # noqa: E731
    NG, NT = int(gt_off[-1]), int(tr_off[-1])
    out = {"gt_kind": new(NG, IGNORED), "gt_frag": new(NG, 0), "gt_partner": new(NG, -1),
           "gt_iou": new(NG, 0.0, torch.float64), "tr_kind": new(NT, IGNORED), "tr_partner": new(NT, -1)}
    for k, src in (("gt_kind", gt_src), ("gt_frag", gt_src), ("gt_iou", gt_src), ("tr_kind", tr_src)):
        out[k][src] = rows[k]
    split_frames = torch.arange(len(frame_src), device=dev)
    for mine, mine_src, mine_off, other_src, other_off, s_other_off in (
            ("gt", gt_src, s_gt_off, tr_src, tr_off, s_tr_off), ("tr", tr_src, s_tr_off, gt_src, gt_off, s_gt_off)):
        partner = rows[mine + "_partner"].long()
        q = torch.repeat_interleave(split_frames, mine_off[1:] - mine_off[:-1])     # the split frame of a split row
        r = (partner >= 0).nonzero().reshape(-1)
        there = other_src[s_other_off[q[r]] + partner[r]]                           # the partner as a packed row
        out[mine + "_partner"][mine_src[r]] = (there - other_off[frame_src[q[r]]]).int()
    return out


def _confusion(n_seqs: int, gt_seq, gt_cls, gt_kind, gt_cross_class, tr_seq, tr_cls, tr_kind, tr_cross_partner):
    """int64 [S, 9, 9] from integer rows (torch int64 tensors on one device): one ``bincount``, no float, one order."""
    import torch
    seen = gt_kind != IGNORED
    matched = (gt_kind == MATCH) | (gt_kind == SWITCH)
    column = torch.where(matched, gt_cls, torch.where(gt_cross_class >= 0, gt_cross_class, NONE))
    lone = (tr_kind == FP) & (tr_cross_partner < 0)
    cell = torch.cat([(gt_seq * 81 + gt_cls * 9 + column)[seen], (tr_seq * 81 + NONE * 9 + tr_cls)[lone]])
    return torch.bincount(cell, minlength=n_seqs * 81).reshape(n_seqs, 9, 9)


def _row_sequences(seq_off, off):
    """The sequence of every row behind per-frame offsets ``off`` (numpy)."""
    frames = np.repeat(np.arange(len(seq_off) - 1), np.diff(seq_off))
    return np.repeat(frames, np.diff(off)).astype(np.int64)


def _cross_host(p: B.PackedBDD, gt_kind: np.ndarray, tr_kind: np.ndarray) -> dict:
    """The cross-class pairs of every frame: the statement ``clipops_bdd_cross_class_f64`` is held to."""
    gc, tc = class_index(p.gt_classes), class_index(p.tr_classes)
    out = {"gt_cross_partner": np.full(len(gc), -1, np.int32), "gt_cross_class": np.full(len(gc), -1, np.int32),
           "gt_cross_iou": np.zeros(len(gc)), "tr_cross_partner": np.full(len(tc), -1, np.int32),
           "tr_cross_class": np.full(len(tc), -1, np.int32), "tr_cross_iou": np.zeros(len(tc))}
    for f in range(len(p.gt_off) - 1):
        g0, g1, t0, t1 = p.gt_off[f], p.gt_off[f + 1], p.tr_off[f], p.tr_off[f + 1]
        g = np.flatnonzero((gt_kind[g0:g1] == MISS) & (gc[g0:g1] >= 0))
        t = np.flatnonzero((tr_kind[t0:t1] == FP) & (tc[t0:t1] >= 0))
        if len(g) == 0 or len(t) == 0:
            continue
        iou = B.box_iou_x0y0x1y1(p.gt_boxes[g0 + g], p.tr_boxes[t0 + t])
        score = np.where(iou < E.THRESHOLD - E.EPS, 0.0, iou)
        score[gc[g0 + g][:, None] == tc[t0 + t][None, :]] = 0.0
        rows, cols = E._assign(-score)
        hit = score[rows, cols] > E.EPS
        rows, cols = rows[hit], cols[hit]
        out["gt_cross_partner"][g0 + g[rows]], out["tr_cross_partner"][t0 + t[cols]] = t[cols], g[rows]
        out["gt_cross_class"][g0 + g[rows]], out["tr_cross_class"][t0 + t[cols]] = tc[t0 + t[cols]], gc[g0 + g[rows]]
        out["gt_cross_iou"][g0 + g[rows]] = out["tr_cross_iou"][t0 + t[cols]] = score[rows, cols]
    return out


def bdd_events_host(packed: B.PackedBDD) -> dict:
    """The events of every input row of ``packed`` (see the module's text) as numpy arrays over all sequences: the
    arrays of ``ROW_KEYS``, ``counts`` int32 [S, 8, 5] (CLR_TP, CLR_FN, CLR_FP, IDSW, Frag) and ``confusion`` int64
    [S, 9, 9]."""
    import torch
    p = packed.numpy()
    _, sim, d = B._preprocess_host(p)
    split = B.class_split_host(p)
    walk = D._walk_host(d, sim)
    rows = D._to_input_rows(B._as_sequences(p.names, split), d, walk,
                            torch.from_numpy(np.ascontiguousarray(sim, np.float64)))
    out = {k: v.numpy() for k, v in _rows_from_split(p.gt_off, p.tr_off, split, rows).items()}
    out.update(_cross_host(p, out["gt_kind"], out["tr_kind"]))
    S = len(p.names)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).long()                                 # noqa: E731
    out["counts"] = walk["counts"].reshape(S, N_CLASSES, 5)
    out["confusion"] = _confusion(S, t(_row_sequences(p.seq_off, p.gt_off)), t(class_index(p.gt_classes)),
                                  t(out["gt_kind"]), t(out["gt_cross_class"]), t(_row_sequences(p.seq_off, p.tr_off)),
                                  t(class_index(p.tr_classes)), t(out["tr_kind"]), t(out["tr_cross_partner"])).numpy()
    return out


# ------------------------------------------------------------------------------------------------ the device path
def launch_cross_class(gt_boxes, tr_boxes, gt_classes, tr_classes, gt_off, tr_off, gt_kind, tr_kind, max_gt: int,
                       max_tr: int, gt_partner, gt_class, gt_iou, tr_partner, tr_class, tr_iou, status) -> None:
    """``clipops_bdd_cross_class_f64`` on the current stream: contiguous CUDA tensors with the dtypes of
    include/clip_ops_hip.h; the seven outputs are written whole, nothing waits."""
    E._launch("clipops_bdd_cross_class_f64", gt_off.device,
              [gt_boxes, tr_boxes, gt_classes, tr_classes, gt_off, tr_off, gt_kind, tr_kind, int(gt_off.numel()) - 1,
               int(max_gt), int(max_tr), gt_partner, gt_class, gt_iou, tr_partner, tr_class, tr_iou, status])


def _device_rows(packed: B.PackedBDD, timings: dict = None) -> dict:
    """``bdd_events_host``'s arrays by the kernels, as torch tensors on ``packed``'s device, on the current stream:
    ``evaluation_bdd100k.device_front_bdd`` with the class split carrying row numbers, ONE launch of
    ``clipops_clear_events_f64`` over the S * 8 problems (``diagnose._walk_device``), the scatter to the input rows,
    ``clipops_bdd_cross_class_f64`` over the input frames and the confusion matrix from integers.  ``timings``: a
    dictionary that receives a pair of HIP events around each of the two launches of this module
    (tools/bench_bdd_events.py)."""
    import torch
    with E._on_stream(packed.gt_boxes.device):
        fr = B.device_front_bdd(packed, scatter_rows=True)
        tens, new, up, timed = fr.tens, fr.new, fr.up, E._timed(timings)
        seq_off, in_gt_off, in_tr_off = fr.split["seq_off"], tens["gt_off"].cpu().numpy(), tens["tr_off"].cpu().numpy()
        S, F, NG, NT = len(seq_off) - 1, len(in_gt_off) - 1, tens["gt_ids"].numel(), tens["tr_ids"].numel()
        # one walk over the S * 8 problems
        walk, counts = D._walk_device(fr, "(sequence, class)", timed)
        split = {"gt_off": fr.host.gt_off, "tr_off": fr.host.tr_off, "gt_src": fr.split["gt_src"],
                 "tr_src": fr.split["tr_src"], "frame_src": fr.split["frame_src"]}
        rows = _rows_from_split(in_gt_off, in_tr_off, split, D._to_input_rows(fr.host, fr.d, walk, fr.sim))
        # the cross-class pairs of every input frame, and the confusion matrix from integers
        cross = {"gt_cross_partner": new(NG, torch.int32), "gt_cross_class": new(NG, torch.int32),
                 "gt_cross_iou": new(NG, torch.float64), "tr_cross_partner": new(NT, torch.int32),
                 "tr_cross_class": new(NT, torch.int32), "tr_cross_iou": new(NT, torch.float64)}
        if F:
            status = new(F, torch.int32)
            timed("clipops_bdd_cross_class_f64", launch_cross_class, tens["gt_boxes"], tens["tr_boxes"],
                  tens["gt_classes"], tens["tr_classes"], tens["gt_off"], tens["tr_off"], rows["gt_kind"],
                  rows["tr_kind"], min(E._frame_max(in_gt_off), CROSS_MAX_DIM),
                  min(E._frame_max(in_tr_off), CROSS_MAX_DIM), *cross.values(), status)
            over = (status[:F] == -2).nonzero()
            if over.numel():
                f = int(over[0])
                s = int(np.searchsorted(seq_off, f, side="right")) - 1
                raise ValueError(f"sequence {packed.names[s]}, frame {f - int(seq_off[s])}: more than {CROSS_MAX_DIM} "
                                 "cross-class candidates on a side exceed the device limit (analyse it on the host)")
            E._raise_on_status(status[:F], "cross-class match", "frame")
        rows.update({k: v[:NG if k.startswith("gt") else NT] for k, v in cross.items()})
        rows["counts"] = counts.reshape(S, N_CLASSES, 5)
        rows["confusion"] = _confusion(S, up(_row_sequences(seq_off, in_gt_off)), class_index(tens["gt_classes"]).long(),
                                       rows["gt_kind"].long(), rows["gt_cross_class"].long(),
                                       up(_row_sequences(seq_off, in_tr_off)), class_index(tens["tr_classes"]).long(),
                                       rows["tr_kind"].long(), rows["tr_cross_partner"].long())
        return rows


# ---------------------------------------------------------------------------------------------------- entry points
def _split(p: B.PackedBDD, rows: dict) -> Dict[str, BDDSequenceEvents]:
    """Per sequence, from host arrays."""
    out = {}
    for s, name in enumerate(p.names):
        f0, f1 = int(p.seq_off[s]), int(p.seq_off[s + 1])
        g0, g1, t0, t1 = int(p.gt_off[f0]), int(p.gt_off[f1]), int(p.tr_off[f0]), int(p.tr_off[f1])
        a = {"gt_off": (p.gt_off[f0:f1 + 1] - g0).astype(np.int32), "tr_off": (p.tr_off[f0:f1 + 1] - t0).astype(np.int32),
             "class_counts": rows["counts"][s], "confusion_matrix": rows["confusion"][s]}
        for side, (r0, r1) in (("gt", (g0, g1)), ("tr", (t0, t1))):
            for k in ("ids", "boxes", "classes"):
                a[f"{side}_{k}"] = getattr(p, f"{side}_{k}")[r0:r1]
            a.update({k: rows[k][r0:r1] for k in ROW_KEYS if k.startswith(side)})
        out[name] = BDDSequenceEvents(name, *[a[k] for k in BDDSequenceEvents.ARRAYS])
    return out


def bdd_events(packed: B.PackedBDD, device=None) -> Dict[str, BDDSequenceEvents]:
    """``{name: BDDSequenceEvents}``.  ``device``: a CUDA device for the kernels, on the current stream (a missing
    library raises); "cpu" or None (the default) for the host statement, to which device tensors are copied."""
    if device is not None and str(device).startswith("cuda"):
        rows = _device_rows(packed if packed.is_device() else packed.to(device))
        rows = {k: v.cpu().numpy() for k, v in rows.items()}                       # (the one host copy; synchronises)
    else:
        rows = bdd_events_host(packed)
    return _split(packed.numpy(), rows)


def bdd_events_from_files(gt_dir: str, tracker_dir: str, device=None) -> Dict[str, BDDSequenceEvents]:
    """The events of result files in ``evaluation_bdd100k.evaluate_bdd_files``' layout, with its arguments."""
    return B.load_bdd_files(gt_dir, tracker_dir, device).events()


# ------------------------------------------------------------------------------------------------ the command line
def summed_confusion(events: Dict[str, BDDSequenceEvents]) -> np.ndarray:
    return sum((ev.confusion_matrix for ev in events.values()), np.zeros((9, 9), np.int64))


def confusion_csv(matrix: np.ndarray) -> str:
    """Ground truth down, tracker across, ``LABELS`` on both edges."""
    lines = ["gt\\tracker," + ",".join(LABELS)]
    lines += [LABELS[g] + "," + ",".join(str(int(v)) for v in matrix[g]) for g in range(9)]
    return "\n".join(lines) + "\n"


def summary_text(events: Dict[str, BDDSequenceEvents], worst: int = 10) -> str:
    """Per sequence and class the five counts; the ten largest confusions over all sequences; the number of ignored
    boxes; per sequence the ``worst`` frames with the most errors."""
    lines = []
    for name, ev in events.items():
        lines += [f"{name} {cls} " + " ".join(f"{k}={v}" for k, v in c.items()) for cls, c in ev.counts().items()]
    lines.append("confusions (ground truth -> tracker)")
    lines += [f"  {g} -> {t}: {n}" for g, t, n in _largest_confusions(summed_confusion(events), 10)]
    lines.append(f"ignored tracker boxes: {sum(int((ev.tr_kind == IGNORED).sum()) for ev in events.values())}")
    for name, ev in events.items():
        lines += [f"{name} frame {f}: FN={fn} FP={fp} IDSW={sw}" for f, fn, fp, sw in ev.worst_frames(worst)]
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    import argparse
    import glob
    ap = argparse.ArgumentParser(prog="python -m memotr_amd.diagnose_bdd100k", description=__doc__.split("\n\n")[0])
    ap.add_argument("--gt-dir", required=True)
    ap.add_argument("--tracker-dir", required=True)
    ap.add_argument("--out", required=True, help="receives <seq>.csv, confusion.csv, summary.txt and <seq>/frames/*.jpg")
    ap.add_argument("--frames-root", help="<frames-root>/<seq>/*.jpg in frame order: also write the annotated frames")
    ap.add_argument("--only-errors", action="store_true", help="only frames with a miss, a false positive or a switch")
    ap.add_argument("--device", default=None, help="a CUDA device for the kernels; default: the host statements")
    ap.add_argument("--worst", type=int, default=10, help="frames per sequence in summary.txt")
    args = ap.parse_args(argv)
    events = bdd_events_from_files(args.gt_dir, args.tracker_dir, args.device)
    os.makedirs(args.out, exist_ok=True)
    for name, ev in events.items():
        ev.write_csv(os.path.join(args.out, name + ".csv"))
        line = f"{name} " + " ".join(f"{k}={int(v)}" for k, v in zip(COUNTS, ev.class_counts.sum(0)))
        if args.frames_root:
            frames = sorted(glob.glob(os.path.join(glob.escape(os.path.join(args.frames_root, name)), "*.jpg")))
            written = D.write_error_frames(ev.as_sequence_events(), frames, os.path.join(args.out, name, "frames"),
                                           only_errors=args.only_errors, device=args.device)
            line += f" frames={len(written)}"
        print(line)
    with open(os.path.join(args.out, "confusion.csv"), "w") as f:
        f.write(confusion_csv(summed_confusion(events)))
    with open(os.path.join(args.out, "summary.txt"), "w") as f:
        f.write(summary_text(events, args.worst))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
