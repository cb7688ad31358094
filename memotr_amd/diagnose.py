"""Error analysis: where a tracker loses its CLEAR points.  ``evaluation.py`` returns counts (``CLR_FN = 4127``,
``IDSW = 311``); this module returns the decisions behind them, per input row, writes them as a CSV per sequence and
draws them into the frames: misses, false positives and identity switches boxed in their colours.

    events = events_from_files(gt_root, tracker_dir, seqmap, benchmark="MOT17", device="cuda")     # evaluate_files' arguments
    ev = events["dancetrack0004"]
    ev.counts()              # {"CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "Frag"}: evaluate_files(...)["dancetrack0004"]'s
    ev.switches()            # [(frame, gt_id, tracker_id_before, tracker_id_now), ...]
    ev.worst_frames(10)      # frames by FN + FP + IDSW, ties by frame
    ev.write_csv("events/dancetrack0004.csv")
    write_error_frames(ev, frame_paths, "errors/dancetrack0004", only_errors=True, quality=85, font_scale=2)

    python -m memotr_amd.diagnose --gt-root G --tracker-dir T --seqmap M --out DIR [--frames-root R --only-errors]

Frames are numbered from 1 wherever this module names one (``switches``, ``worst_frames``, the CSV, the file names of
``write_error_frames``): the first column of gt.txt, and the name of the image under ``img1``.

The definition is stated twice, like the evaluation's.  ``clear_events_host`` walks every sequence as
``evaluation._clear_host`` does, after ``evaluation._preprocess_host``, and keeps what that walk decides per row; it is
numpy and scipy.  With a CUDA ``device`` the similarity, the preprocessing match and the compaction are
``evaluation.device_front``'s, the calls ``evaluation.device_tables`` stands on, and ``clipops_clear_events_f64``
(memotr_amd/csrc/clip_tracks.h) walks the sequences, one wavefront each; integer results and similarities agree exactly.  The draw table is
``error_table_host`` -- ``render.track_table``'s rows with the colour of the event -- or ``clipops_error_table_f64``,
word for word the same.

Kinds.  A ground-truth row is IGNORED (removed by the preprocessing: not a pedestrian, or zero-marked), MATCH, SWITCH
(matched, and counted in IDSW at this row) or MISS.  A tracker row is IGNORED (matched to a distractor by the
preprocessing), TP (= MATCH), SWITCH (a TP whose partner is a SWITCH) or FP.

Scope: ``benchmark="MOT17"`` (DanceTrack, SportsMOT, MOT17) and ``"MOT15"`` (no preprocessing), as ``evaluation.py``.
BDD100K's events are diagnose_bdd100k.py's: eight problems per sequence, ignore regions and class confusions.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import evaluation as E

IGNORED, MATCH, SWITCH, MISS, FP = 0, 1, 2, 3, 4        # CLIPOPS_KIND_* of include/clip_ops_hip.h
TP = MATCH
EVENT_SWITCH, EVENT_FRAG = 1, 2                         # CLIPOPS_EVENT_*: the bits of the kernel's gt_flags
GT_KIND_NAMES = {IGNORED: "IGNORED", MATCH: "MATCH", SWITCH: "SWITCH", MISS: "MISS"}
TR_KIND_NAMES = {IGNORED: "IGNORED", TP: "TP", SWITCH: "SWITCH", FP: "FP"}
COLOURS = {TP: (0, 200, 0), FP: (255, 0, 0), MISS: (255, 200, 0), SWITCH: (255, 0, 255)}
COUNTS = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "Frag")
CSV_HEADER = "frame,side,id,x,y,w,h,kind,partner_id,iou,frag"
PADDING_ROW = np.array([0, 0, -1, -1] + [0] * 12, dtype=np.int32)     # draws nothing: x2 < x1


# ------------------------------------------------------------------------------------ the events of one sequence
@dataclass
class SequenceEvents:
    """The rows of one sequence as the files give them (``PackedSequences``' order; offsets per frame) and the event
    of every row, as host arrays."""
    name: str
    gt_off: np.ndarray          # int32 [F + 1]
    tr_off: np.ndarray          # int32 [F + 1]
    gt_ids: np.ndarray          # int32 [NG]
    gt_boxes: np.ndarray        # float64 [NG, 4] xywh
    gt_kind: np.ndarray         # int32 [NG]
    gt_frag: np.ndarray         # int32 [NG]: 1 where a track is picked up again (the sum is Frag)
    gt_partner: np.ndarray      # int32 [NG]: index within the frame's tracker rows, -1
    gt_iou: np.ndarray          # float64 [NG]: the pair's similarity, 0
    tr_ids: np.ndarray          # int32 [NT]
    tr_boxes: np.ndarray        # float64 [NT, 4] xywh
    tr_kind: np.ndarray         # int32 [NT]
    tr_partner: np.ndarray      # int32 [NT]: index within the frame's ground-truth rows, -1

    ARRAYS = ("gt_off", "tr_off", "gt_ids", "gt_boxes", "gt_kind", "gt_frag", "gt_partner", "gt_iou", "tr_ids",
              "tr_boxes", "tr_kind", "tr_partner")

    @property
    def n_frames(self) -> int:
        return len(self.gt_off) - 1

    def counts(self) -> Dict[str, int]:
        matched = (self.gt_kind == MATCH) | (self.gt_kind == SWITCH)
        return {"CLR_TP": int(matched.sum()), "CLR_FN": int((self.gt_kind == MISS).sum()),
                "CLR_FP": int((self.tr_kind == FP).sum()), "IDSW": int((self.gt_kind == SWITCH).sum()),
                "Frag": int(self.gt_frag.sum())}

    def frame_errors(self) -> np.ndarray:
        """int64 [F, 3]: misses, false positives and switches of every frame."""
        per_frame = lambda flag, off: np.concatenate(([0], np.cumsum(flag)))[off]              # noqa: E731
        fn, fp = np.diff(per_frame(self.gt_kind == MISS, self.gt_off)), np.diff(per_frame(self.tr_kind == FP, self.tr_off))
        return np.stack([fn, fp, np.diff(per_frame(self.gt_kind == SWITCH, self.gt_off))], 1).astype(np.int64)

    def worst_frames(self, n: int = 10) -> List[Tuple[int, int, int, int]]:
        """The ``n`` frames with the most errors: (frame, FN, FP, IDSW), by FN + FP + IDSW, ties by frame."""
        e = self.frame_errors()
        order = np.argsort(-e.sum(1), kind="stable")[:max(int(n), 0)]
        return [(int(f) + 1, int(e[f, 0]), int(e[f, 1]), int(e[f, 2])) for f in order]

    def switches(self) -> List[Tuple[int, int, int, int]]:
        """(frame, gt_id, tracker_id_before, tracker_id_now) of every SWITCH row, in row order."""
        last, out = {}, []
        for f in range(self.n_frames):
            g0, t0 = int(self.gt_off[f]), int(self.tr_off[f])
            for i in range(g0, int(self.gt_off[f + 1])):
                if self.gt_partner[i] < 0:
                    continue
                gid, tid = int(self.gt_ids[i]), int(self.tr_ids[t0 + self.gt_partner[i]])
                if self.gt_kind[i] == SWITCH:
                    out.append((f + 1, gid, last[gid], tid))
                last[gid] = tid
        return out

    def max_drawn_rows(self) -> int:
        """The most rows a frame's error table holds."""
        drawn = lambda flag, off: np.diff(np.concatenate(([0], np.cumsum(flag)))[off])          # noqa: E731
        n = drawn(self.gt_kind == MISS, self.gt_off) + drawn(self.tr_kind != IGNORED, self.tr_off)
        return int(n.max()) if len(n) else 0

    def write_csv(self, path: str) -> None:
        """One line per input row, ground truth before tracker rows within a frame:
        ``frame(1-based),side(gt|tr),id,x,y,w,h,kind,partner_id,iou,frag``; floats as Python prints them (they read
        back to the same bits), partner_id -1 and iou 0 without a partner."""
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        lines = [CSV_HEADER]
        for f in range(self.n_frames):
            g0, g1, t0, t1 = (int(v) for v in (self.gt_off[f], self.gt_off[f + 1], self.tr_off[f], self.tr_off[f + 1]))
            for i in range(g0, g1):
                p = int(self.gt_partner[i])
                box = ",".join(repr(float(v)) for v in self.gt_boxes[i])
                lines.append(f"{f + 1},gt,{int(self.gt_ids[i])},{box},{GT_KIND_NAMES[int(self.gt_kind[i])]},"
                             f"{int(self.tr_ids[t0 + p]) if p >= 0 else -1},{float(self.gt_iou[i])!r},"
                             f"{int(self.gt_frag[i])}")
            for j in range(t0, t1):
                p = int(self.tr_partner[j])
                box = ",".join(repr(float(v)) for v in self.tr_boxes[j])
                lines.append(f"{f + 1},tr,{int(self.tr_ids[j])},{box},{TR_KIND_NAMES[int(self.tr_kind[j])]},"
                             f"{int(self.gt_ids[g0 + p]) if p >= 0 else -1},"
                             f"{float(self.gt_iou[g0 + p]) if p >= 0 else 0.0!r},0")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")

    @classmethod
    def read_csv(cls, path: str, name: Optional[str] = None, n_frames: Optional[int] = None) -> "SequenceEvents":
        """What ``write_csv`` wrote.  ``n_frames``: the sequence's length where its last frames hold no row."""
        gt_kinds, tr_kinds = ({v: k for k, v in names.items()} for names in (GT_KIND_NAMES, TR_KIND_NAMES))
        rows = {"gt": [], "tr": []}
        with open(path) as f:
            if f.readline().strip() != CSV_HEADER:
                raise ValueError(f"{path}: not an events file")
            for line in f:
                c = line.strip().split(",")
                if len(c) == 11:
                    rows[c[1]].append(c)
        F = max([int(n_frames or 0)] + [int(c[0]) for side in rows.values() for c in side])
        off = {s: np.concatenate(([0], np.cumsum(np.bincount([int(c[0]) - 1 for c in rows[s]], minlength=F))))
               .astype(np.int32) for s in rows}
        col = lambda s, k, dt: np.array([c[k] for c in rows[s]], dtype=np.float64).astype(dt).reshape(-1)      # noqa: E731
        ids = {s: col(s, 2, np.int32) for s in rows}
        boxes = {s: np.array([[float(v) for v in c[3:7]] for c in rows[s]], np.float64).reshape(-1, 4) for s in rows}
        partner = {}
        for s, o in (("gt", "tr"), ("tr", "gt")):
            partner[s] = np.full(len(rows[s]), -1, np.int32)
            for r, c in enumerate(rows[s]):
                if int(c[8]) >= 0:
                    f = int(c[0]) - 1
                    partner[s][r] = int(np.flatnonzero(ids[o][off[o][f]:off[o][f + 1]] == int(c[8]))[0])
        return cls(name or os.path.splitext(os.path.basename(path))[0], off["gt"], off["tr"], ids["gt"], boxes["gt"],
                   np.array([gt_kinds[c[7]] for c in rows["gt"]], np.int32), col("gt", 10, np.int32), partner["gt"],
                   np.array([float(c[9]) for c in rows["gt"]], np.float64), ids["tr"], boxes["tr"],
                   np.array([tr_kinds[c[7]] for c in rows["tr"]], np.int32), partner["tr"])


# --------------------------------------------------------------------------------- the definition, on the host
def _walk_host(d: dict, sim: np.ndarray) -> dict:
    """``evaluation._clear_host``'s walk over the preprocessed data ``d`` (``evaluation._compact``), keeping per row what
    that function counts: the statement ``clipops_clear_events_f64`` is held to.  ``gt_partner`` / ``tr_partner``: the
    partner's index within its frame, -1; ``gt_flags``: EVENT_SWITCH | EVENT_FRAG; ``counts`` int32 [S, 5]."""
    S = len(d["seq_off"]) - 1
    gt_partner, tr_partner = np.full(len(d["gt_ids"]), -1, np.int32), np.full(len(d["tr_ids"]), -1, np.int32)
    gt_flags, counts = np.zeros(len(d["gt_ids"]), np.int32), np.zeros((S, 5), np.int32)
    for s in range(S):
        if d["n_gt_dets"][s] == 0 or d["n_tr_dets"][s] == 0:
            # host_tables skips the sequence; _sequence_result: everything missed, or everything false
            counts[s, 1], counts[s, 2] = d["n_gt_dets"][s], d["n_tr_dets"][s]
            continue
        G = int(d["n_gt_ids"][s])
        last, last_step = np.full(G, -1), np.full(G, -1)
        tp = fn = fp = idsw = frag = 0
        for f in range(d["seq_off"][s], d["seq_off"][s + 1]):
            g0, t0 = d["gt_off"][f], d["tr_off"][f]
            gi, ti = d["gt_ids"][g0:d["gt_off"][f + 1]], d["tr_ids"][t0:d["tr_off"][f + 1]]
            sm = sim[d["sim_off"][f]:d["sim_off"][f + 1]].reshape(len(gi), len(ti))
            if len(gi) == 0:
                fp += len(ti)
                continue
            if len(ti) == 0:
                fn += len(gi)
                continue
            score = 1000 * (ti[None, :] == last_step[gi[:, None]]) + sm
            score[sm < E.THRESHOLD - E.EPS] = 0
            rows, cols = E._assign(-score)
            hit = score[rows, cols] > 0 + E.EPS
            rows, cols = rows[hit], cols[hit]
            mg, mt = gi[rows], ti[cols]
            switch = (last[mg] >= 0) & (last[mg] != mt)
            again = (last_step[mg] < 0) & (last[mg] >= 0)          # was_free, and the id had been matched before
            gt_partner[g0 + rows], tr_partner[t0 + cols] = cols, rows
            gt_flags[g0 + rows] = EVENT_SWITCH * switch + EVENT_FRAG * again
            last[mg] = mt
            last_step[:] = -1
            last_step[mg] = mt
            idsw, frag = idsw + int(switch.sum()), frag + int(again.sum())
            tp, fn, fp = tp + len(mg), fn + len(gi) - len(mg), fp + len(ti) - len(mg)
        counts[s] = (tp, fn, fp, idsw, frag)
    return {"gt_partner": gt_partner, "gt_flags": gt_flags, "tr_partner": tr_partner, "counts": counts}


def _to_input_rows(p: E.PackedSequences, d: dict, walk: dict, sim) -> dict:
    """The compact arrays of a walk scattered back to the input rows through the keep indices.  ``p``, ``d`` and
    ``walk`` hold torch tensors on one device (the host's, for the host statement); a few index operations."""
    import torch
    dev = sim.device
    i64 = lambda x: torch.as_tensor(x, device=dev).long()                                       # noqa: E731
    gt_off, tr_off, c_gt_off, c_tr_off = i64(p.gt_off), i64(p.tr_off), i64(d["gt_off"]), i64(d["tr_off"])
    keep_gt, keep_tr, sim_off = i64(d["keep_gt"]), i64(d["keep_tr"]), i64(d["sim_off"])
    F = len(gt_off) - 1
    frames = torch.arange(F, device=dev)
    gt_frame = torch.repeat_interleave(frames, c_gt_off[1:] - c_gt_off[:-1])        # the frame of a compact row
    tr_frame = torch.repeat_interleave(frames, c_tr_off[1:] - c_tr_off[:-1])
    gp, gf, tp = i64(walk["gt_partner"]), i64(walk["gt_flags"]), i64(walk["tr_partner"])
    NG, NT = int(gt_off[-1]), int(tr_off[-1])
    new = lambda n, fill, dt=torch.int32: torch.full((n,), fill, dtype=dt, device=dev)          # noqa: E731
    out = {"gt_kind": new(NG, IGNORED), "gt_frag": new(NG, 0), "gt_partner": new(NG, -1),
           "gt_iou": new(NG, 0.0, torch.float64), "tr_kind": new(NT, IGNORED), "tr_partner": new(NT, -1)}
    # ground truth: kind and frag of every kept row; partner and similarity of the matched ones
    hit = gp >= 0
    kind = torch.where(hit, torch.where((gf & EVENT_SWITCH) != 0, SWITCH, MATCH), MISS)
    out["gt_kind"][keep_gt] = kind.int()
    out["gt_frag"][keep_gt] = ((gf & EVENT_FRAG) != 0).int()
    rows, fr = hit.nonzero().reshape(-1), gt_frame[hit]
    partner_row = keep_tr[c_tr_off[fr] + gp[rows]]                                  # the partner as an input row
    out["gt_partner"][keep_gt[rows]] = (partner_row - tr_off[fr]).int()
    width = c_tr_off[fr + 1] - c_tr_off[fr]
    out["gt_iou"][keep_gt[rows]] = sim[sim_off[fr] + (rows - c_gt_off[fr]) * width + gp[rows]]
    # tracker rows: TP, SWITCH where the partner is one, FP
    hit = tp >= 0
    rows, fr = hit.nonzero().reshape(-1), tr_frame[hit]
    partner_c = c_gt_off[fr] + tp[rows]
    kind = torch.full_like(tp, FP)
    kind[rows] = torch.where((gf[partner_c] & EVENT_SWITCH) != 0, SWITCH, TP)
    out["tr_kind"][keep_tr] = kind.int()
    out["tr_partner"][keep_tr[rows]] = (keep_gt[partner_c] - gt_off[fr]).int()
    return out


def _split(p: E.PackedSequences, rows: dict) -> Dict[str, SequenceEvents]:
    """Per sequence, from host arrays."""
    out = {}
    for s, name in enumerate(p.names):
        f0, f1 = int(p.seq_off[s]), int(p.seq_off[s + 1])
        g0, g1, t0, t1 = int(p.gt_off[f0]), int(p.gt_off[f1]), int(p.tr_off[f0]), int(p.tr_off[f1])
        out[name] = SequenceEvents(
            name, (p.gt_off[f0:f1 + 1] - g0).astype(np.int32), (p.tr_off[f0:f1 + 1] - t0).astype(np.int32),
            p.gt_ids[g0:g1], p.gt_boxes[g0:g1], rows["gt_kind"][g0:g1], rows["gt_frag"][g0:g1],
            rows["gt_partner"][g0:g1], rows["gt_iou"][g0:g1], p.tr_ids[t0:t1], p.tr_boxes[t0:t1],
            rows["tr_kind"][t0:t1], rows["tr_partner"][t0:t1])
    return out


def clear_events_host(packed: E.PackedSequences, benchmark: str = "MOT17") -> dict:
    """The events of every input row of ``packed`` (see the module's text), as numpy arrays over all sequences:
    ``gt_kind``, ``gt_frag``, ``gt_partner``, ``gt_iou``, ``tr_kind``, ``tr_partner``, and ``counts`` int32 [S, 5]
    (CLR_TP, CLR_FN, CLR_FP, IDSW, Frag).  MOT17 rules, or MOT15 without preprocessing; not BDD100K
    (diagnose_bdd100k.py)."""
    import torch
    _check_benchmark(benchmark)
    p = packed.numpy()
    _, sim, d = E._preprocess_host(p, benchmark)
    walk = _walk_host(d, sim)
    rows = _to_input_rows(p, d, walk, torch.from_numpy(np.ascontiguousarray(sim, np.float64)))
    out = {k: v.numpy() for k, v in rows.items()}
    out["counts"] = walk["counts"]
    return out


def _check_benchmark(benchmark: str) -> None:
    if benchmark not in ("MOT17", "MOT15"):
        raise ValueError(f"benchmark {benchmark!r} is not supported (MOT17 rules, or MOT15 for no preprocessing match; "
                         "BDD100K's events are memotr_amd.diagnose_bdd100k's)")


# ------------------------------------------------------------------------------------------------ the device path
def launch_clear_events(sim, sim_off, gt_off, tr_off, gt_ids, tr_ids, seq_off, n_gt_ids, max_gt: int, max_tr: int,
                        max_gt_ids: int, gt_partner, gt_flags, tr_partner, counts, status) -> None:
    """``clipops_clear_events_f64`` on the current stream: contiguous CUDA tensors with the dtypes of
    include/clip_ops_hip.h; the five outputs are written whole, nothing waits."""
    E._launch("clipops_clear_events_f64", seq_off.device,
              [sim, sim_off, gt_off, tr_off, gt_ids, tr_ids, seq_off, int(seq_off.numel()) - 1, n_gt_ids, int(max_gt),
               int(max_tr), int(max_gt_ids), gt_partner, gt_flags, tr_partner, counts, status])


def launch_error_table(gt_boxes, tr_boxes, gt_off, tr_off, gt_ids, tr_ids, gt_kind, tr_kind, max_rows: int, width: int,
                       height: int, bgr: bool, font_scale: int, table) -> None:
    """``clipops_error_table_f64`` on the current stream, into ``table`` int32 (F, max_rows, 16)."""
    E._launch("clipops_error_table_f64", table.device,
              [gt_boxes, tr_boxes, gt_off, tr_off, gt_ids, tr_ids, gt_kind, tr_kind, int(gt_off.numel()) - 1,
               int(max_rows), int(width), int(height), int(bool(bgr)), int(font_scale), table])


def _walk_device(fr: E.DeviceFront, sequence: str = "sequence", run=None):
    """``_walk_host`` over a front's sequences by one launch of ``clipops_clear_events_f64`` through the per-call hook
    ``run``: (the walk's arrays, ``counts`` int32 [S, 5]).  ``sequence``: what an error calls one."""
    import torch
    S, n_gt, n_tr = fr.S, len(fr.d["gt_ids"]), len(fr.d["tr_ids"])
    walk = {"gt_partner": fr.new(n_gt, torch.int32), "gt_flags": fr.new(n_gt, torch.int32),
            "tr_partner": fr.new(n_tr, torch.int32)}
    counts, status = torch.empty((max(S, 1), 5), dtype=torch.int32, device=fr.dev), fr.new(S, torch.int32)
    if S:
        (run or fr.run)("clipops_clear_events_f64", launch_clear_events, fr.sim, fr.sim_off, fr.gt_off, fr.tr_off,
                        fr.gt_ids, fr.tr_ids, fr.seq_off, fr.n_gt_ids, fr.max_gt, fr.max_tr, fr.max_gt_ids,
                        walk["gt_partner"], walk["gt_flags"], walk["tr_partner"], counts, status)
        E._raise_on_status(status[:S], "CLEAR events", sequence)
    return {"gt_partner": walk["gt_partner"][:n_gt], "gt_flags": walk["gt_flags"][:n_gt],
            "tr_partner": walk["tr_partner"][:n_tr]}, counts[:S]


def _device_rows(packed: E.PackedSequences, benchmark: str) -> dict:
    """``clear_events_host``'s arrays by the kernels, as torch tensors on ``packed``'s device: ``evaluation.device_front``
    (no launch here solves an identity assignment, so none is checked), then one launch of
    ``clipops_clear_events_f64``."""
    with E._on_stream(packed.gt_boxes.device):
        fr = E.device_front(packed, benchmark)
        walk, counts = _walk_device(fr)
        rows = _to_input_rows(fr.host, fr.d, walk, fr.sim)
        rows["counts"] = counts
        return rows


def clear_events(packed: E.PackedSequences, benchmark: str = "MOT17", device=None) -> Dict[str, SequenceEvents]:
    """``{name: SequenceEvents}``.  ``device``: a CUDA device for the kernels (a missing library raises); "cpu" or None
    (the default) for the host statement, to which device tensors are copied."""
    _check_benchmark(benchmark)
    if device is not None and str(device).startswith("cuda"):
        rows = _device_rows(packed if packed.is_device() else packed.to(device), benchmark)
        rows = {k: v.cpu().numpy() for k, v in rows.items()}                       # (the one host copy; synchronises)
    else:
        rows = clear_events_host(packed, benchmark)
    return _split(packed.numpy(), rows)


def events_from_files(gt_root: str, tracker_dir: str, seqmap: str, benchmark: str = "MOT17",
                      device=None) -> Dict[str, SequenceEvents]:
    """The events of result files in ``evaluation.evaluate_files``' layout, with its arguments."""
    return E.load_files(gt_root, tracker_dir, seqmap, benchmark, device).events()


# ------------------------------------------------------------------------------------------------ the error table
def _table_rows(ev: SequenceEvents, f: int):
    """(ids, xyxy float32 boxes, kinds) of frame ``f``'s table: misses, then the tracker rows that are not ignored."""
    g = np.arange(ev.gt_off[f], ev.gt_off[f + 1])
    t = np.arange(ev.tr_off[f], ev.tr_off[f + 1])
    g, t = g[ev.gt_kind[g] == MISS], t[ev.tr_kind[t] != IGNORED]
    xywh = np.concatenate([ev.gt_boxes[g], ev.tr_boxes[t]]).reshape(-1, 4)
    with np.errstate(over="ignore", invalid="ignore"):
        xyxy = np.stack([xywh[:, 0], xywh[:, 1], xywh[:, 0] + xywh[:, 2], xywh[:, 1] + xywh[:, 3]], 1).astype(np.float32)
    return np.concatenate([ev.gt_ids[g], ev.tr_ids[t]]), xyxy, np.concatenate([ev.gt_kind[g], ev.tr_kind[t]])


def error_table_host(ev: SequenceEvents, width: int, height: int, *, bgr: bool = False, font_scale: int = 1,
                     max_rows: Optional[int] = None) -> np.ndarray:
    """The draw tables of all frames, int32 (F, max_rows, 16): per frame ``render.track_table``'s rows for the MISS
    rows (labelled with the ground-truth id) and then the TP, SWITCH and FP rows (the tracker id), each box
    ``(x, y, x + w, y + h)`` formed in float64 and rounded once to float32, with the colour of the kind in word 4 and
    the text colour that follows from it in word 9; rows past ``max_rows`` (default: the fullest frame) are left out,
    the rest are rows that draw nothing."""
    from .render import ROW_WORDS, track_table
    n = ev.max_drawn_rows() if max_rows is None else int(max_rows)
    table = np.tile(PADDING_ROW, (ev.n_frames, n, 1)).reshape(ev.n_frames, n, ROW_WORDS)
    for f in range(ev.n_frames):
        ids, xyxy, kinds = _table_rows(ev, f)
        rows = track_table(ids, xyxy, width, height, bgr=bgr, font_scale=font_scale)
        for i, kind in enumerate(kinds):
            r, g, b = COLOURS[int(kind)]
            rows[i, 4] = (b | g << 8 | r << 16) if bgr else (r | g << 8 | b << 16)
            rows[i, 9] = 0 if (77 * r + 150 * g + 29 * b) >> 8 >= 128 else 0xFFFFFF
        table[f, :min(n, len(rows))] = rows[:n]
    return table


def error_table_device(ev: SequenceEvents, width: int, height: int, device, *, bgr: bool = False, font_scale: int = 1,
                       max_rows: Optional[int] = None):
    """``error_table_host`` by ``clipops_error_table_f64``: one upload of the sequence's rows, one launch on the current
    stream, a torch int32 (F, max_rows, 16) tensor on ``device``."""
    import torch
    if not 1 <= int(font_scale) <= 64:
        raise ValueError(f"font_scale {font_scale!r} is not an integer in 1 .. 64")
    n = ev.max_drawn_rows() if max_rows is None else int(max_rows)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)                 # noqa: E731
    table = torch.empty((ev.n_frames, n, 16), dtype=torch.int32, device=device)
    launch_error_table(up(ev.gt_boxes, np.float64), up(ev.tr_boxes, np.float64), up(ev.gt_off, np.int32),
                       up(ev.tr_off, np.int32), up(ev.gt_ids, np.int32), up(ev.tr_ids, np.int32),
                       up(ev.gt_kind, np.int32), up(ev.tr_kind, np.int32), n, width, height, bgr, font_scale, table)
    return table


def write_error_frames(ev: SequenceEvents, frame_paths: Sequence[str], out: str, *, only_errors: bool = False,
                       quality: int = 85, thickness: int = 2, font_scale: int = 1, device=None, chunk: int = 16,
                       threads: int = 4) -> List[str]:
    """The frames of a sequence with its events drawn in: ``frame_paths[f]`` is the JPEG of frame ``f + 1``, the files
    are ``<out>/<frame, 8 digits>.jpg`` (RGB, 4:2:0); returns their paths.  ``only_errors``: only frames with at least
    one MISS, FP or SWITCH.  With a CUDA ``device`` the frames go through in chunks: ``decode_jpegs`` onto the device,
    ``render.draw_resident_table`` with the frame's slice of the device table, ``encode_jpegs``.  With ``device=None``
    they go through ``draw_table_host`` and ``encode_jpeg``.  Either way a file is byte for byte
    ``encode_jpeg(draw_table_host(decoded frame, error_table_host(...)[f]))``."""
    import torch
    from .data.jpeg import decode_jpeg, decode_jpegs, parse_jpeg
    from .data.jpeg_write import encode_jpeg, encode_jpegs
    from .render import _check_options, draw_resident_table, draw_table_host
    _check_options(thickness, font_scale, 0)
    if len(frame_paths) != ev.n_frames:
        raise ValueError(f"sequence {ev.name}: {len(frame_paths)} frame paths for {ev.n_frames} frames")
    errors = ev.frame_errors().sum(1)
    todo = [f for f in range(ev.n_frames) if not only_errors or errors[f] > 0]
    os.makedirs(out, exist_ok=True)
    if not todo:
        return []
    with open(frame_paths[todo[0]], "rb") as fh:
        info = parse_jpeg(fh.read())
    H, W = info.height, info.width
    on_device = device is not None and str(device).startswith("cuda")
    paths = []

    def write(f, data):
        paths.append(os.path.join(out, f"{f + 1:08d}.jpg"))
        with open(paths[-1], "wb") as fh:
            fh.write(data)

    def check_size(frame, f):
        if tuple(frame.shape) != (H, W, 3):
            raise ValueError(f"sequence {ev.name}: frame {f + 1} is not {W} x {H} like the first one drawn")

    if not on_device:
        table = error_table_host(ev, W, H, font_scale=font_scale)
        for f in todo:
            frame = decode_jpeg(frame_paths[f], "cpu").numpy()
            check_size(frame, f)
            draw_table_host(frame, table[f], thickness, font_scale, 0)
            write(f, encode_jpeg(torch.from_numpy(frame), quality))
        return paths
    device = torch.device(device)
    with torch.cuda.device(device):
        table = error_table_device(ev, W, H, device, font_scale=font_scale)
        for c0 in range(0, len(todo), max(int(chunk), 1)):
            part = todo[c0:c0 + max(int(chunk), 1)]
            frames = decode_jpegs([frame_paths[f] for f in part], device, threads=threads)
            drawn = torch.empty((len(part), H, W, 3), dtype=torch.uint8, device=device)
            for k, f in enumerate(part):
                check_size(frames[k], f)
                draw_resident_table(frames[k], table[f], drawn[k], thickness, font_scale, 0)
            for f, data in zip(part, encode_jpegs(drawn, threads=threads, quality=quality)):
                write(f, data)
    return paths


# ------------------------------------------------------------------------------------------------ the command line
def summary_text(events: Dict[str, SequenceEvents], worst: int = 10) -> str:
    """Per sequence the five counts and the ``worst`` frames with the most errors."""
    lines = []
    for name, ev in events.items():
        lines.append(name + " " + " ".join(f"{k}={v}" for k, v in ev.counts().items()))
        lines += [f"  frame {f}: FN={fn} FP={fp} IDSW={sw}" for f, fn, fp, sw in ev.worst_frames(worst)]
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    import argparse
    import glob
    ap = argparse.ArgumentParser(prog="python -m memotr_amd.diagnose", description=__doc__.split("\n\n")[0])
    ap.add_argument("--gt-root", required=True)
    ap.add_argument("--tracker-dir", required=True)
    ap.add_argument("--seqmap", required=True)
    ap.add_argument("--benchmark", default="MOT17", choices=("MOT17", "MOT15"))
    ap.add_argument("--out", required=True, help="receives <seq>.csv, summary.txt and <seq>/frames/*.jpg")
    ap.add_argument("--frames-root", help="<frames-root>/<seq>/img1/*.jpg: also write the annotated frames")
    ap.add_argument("--only-errors", action="store_true", help="only frames with a miss, a false positive or a switch")
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--font-scale", type=int, default=1)
    ap.add_argument("--device", default=None, help="a CUDA device for the kernels; default: the host statements")
    args = ap.parse_args(argv)
    events = events_from_files(args.gt_root, args.tracker_dir, args.seqmap, args.benchmark, args.device)
    os.makedirs(args.out, exist_ok=True)
    for name, ev in events.items():
        ev.write_csv(os.path.join(args.out, name + ".csv"))
        line = name + " " + " ".join(f"{k}={v}" for k, v in ev.counts().items())
        if args.frames_root:
            frames = sorted(glob.glob(os.path.join(glob.escape(os.path.join(args.frames_root, name, "img1")), "*.jpg")))
            written = write_error_frames(ev, frames, os.path.join(args.out, name, "frames"),
                                         only_errors=args.only_errors, quality=args.quality,
                                         font_scale=args.font_scale, device=args.device)
            line += f" frames={len(written)}"
        print(line)
    with open(os.path.join(args.out, "summary.txt"), "w") as f:
        f.write(summary_text(events))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
