"""Association analysis: where a tracker loses its HOTA and IDF1.  ``evaluation.py`` returns ``AssA 49.2, IDF1 52.0``;
this module returns the matches behind them -- HOTA's per frame, at all 19 thresholds, and the Identity metric's map of
whole trajectories -- reduces them per identity, and draws the identity timeline: one row per ground-truth identity,
one column per frame, coloured by the tracker id matched there.

    assoc = association_from_files(gt_root, tracker_dir, seqmap, benchmark="MOT17", device="cuda")   # evaluate_files' arguments
    a = assoc["dancetrack0004"]
    a.totals()                   # HOTA_TP[19], the AssA / AssRe / AssPr numerators, IDTP, IDFN, IDFP: evaluate_files' sums
    a.ass_a(), a.id_f1()         # per ground-truth identity
    a.worst_identities(10)       # [(gt_id, AssA, length, n_partners), ...]
    a.fragments(gt_id)           # [(first_frame, last_frame, tracker_id), ...]
    a.write_rows_csv(...), a.write_identities_csv(...)
    write_timeline(a, "dancetrack0004_timeline.jpg", device="cuda")

    python -m memotr_amd.association --gt-root G --tracker-dir T --seqmap M --out DIR [--alpha 0.5] [--worst 10]

Frames are numbered from 1 wherever this module names one, as in ``diagnose``.

The definition is stated twice, like the evaluation's.  ``association_host`` repeats ``evaluation._hota_host``'s second
loop and ``evaluation._identity_host``'s assignment after ``evaluation._preprocess_host`` and keeps the pairs; it is
numpy and scipy.  With a CUDA ``device`` the similarity, the preprocessing match and the compaction are
``evaluation.device_front``'s and ``trackeval_accumulate`` is ``evaluation.device_accumulate``'s, the calls
``evaluation.device_tables`` stands on, and four kernels of memotr_amd/csrc/clip_tracks.h do the rest: ``clipops_hota_events_f64`` (one wavefront per frame),
``clipops_identity_pairs_i32`` (one per sequence), ``clipops_assoc_reduce_f64`` (one per identity) and
``clipops_timeline_u8`` (one workgroup per frame).  Integer results and similarities agree exactly, the per-identity
float sums to float64 summation order.

A pair's ``level`` is the number of thresholds ``a`` with ``similarity >= ALPHAS[a] - eps``: the pair is a true positive
at threshold ``a`` exactly when ``a < level``, so one record per row carries the matches at all 19 thresholds.

Scope: ``benchmark="MOT17"`` and ``"MOT15"``, as ``diagnose``.  BDD100K is out of scope.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import evaluation as E

N_ALPHA = len(E.ALPHAS)                                 # CLIPOPS_ASSOC_ALPHAS of include/clip_ops_hip.h
DEFAULT_ALPHA_INDEX = 9                                 # alpha = 0.5
ABSENT, UNMATCHED = (0, 0, 0), (96, 96, 96)             # timeline cells without a row / without a match
MAX_IMAGE_SIDE = 65535                                  # the JPEG writer's limit
ROWS_HEADER = "frame,side,id,x,y,w,h,kept,partner_id,iou,level"
IDENTITIES_HEADER = "side,id,length,tp50,AssA,AssRe_or_AssPr,n_partners,top_partner,top_count,id_partner,idtp,IDF1"
ROW_KEYS = ("kept", "partner_id", "iou", "level")
ID_KEYS = ("count", "tp", "num", "top", "id_partner", "idtp")


def _check_benchmark(benchmark: str) -> None:
    if benchmark not in ("MOT17", "MOT15"):
        raise ValueError(f"benchmark {benchmark!r} is not supported (MOT17 rules, or MOT15 for no preprocessing match; "
                         "BDD100K's association analysis is out of scope)")


def _check_alpha_index(alpha_index: int) -> int:
    if not 0 <= int(alpha_index) < N_ALPHA:
        raise ValueError(f"alpha_index {alpha_index!r} is not in 0 .. {N_ALPHA - 1}")
    return int(alpha_index)


# ------------------------------------------------------------------------------- the association of one sequence
@dataclass
class SequenceAssociation:
    """The rows of one sequence as the files give them (``PackedSequences``' order; offsets per frame) with the HOTA
    match of every row, and the tables of every identity that survives the preprocessing (ascending id), as host
    arrays.  ``*_num[:, 0]`` is the AssA numerator, ``[:, 1]`` AssRe's (ground truth) or AssPr's (tracker)."""
    name: str
    alpha_index: int
    gt_off: np.ndarray          # int32 [F + 1]
    tr_off: np.ndarray          # int32 [F + 1]
    gt_ids: np.ndarray          # int32 [NG]
    gt_boxes: np.ndarray        # float64 [NG, 4] xywh
    gt_kept: np.ndarray         # bool [NG]: the row survives the preprocessing
    gt_partner_id: np.ndarray   # int32 [NG]: the matched tracker row's id, -1
    gt_iou: np.ndarray          # float64 [NG]: the pair's similarity, 0
    gt_level: np.ndarray        # int32 [NG]: 0 .. 19
    tr_ids: np.ndarray
    tr_boxes: np.ndarray
    tr_kept: np.ndarray
    tr_partner_id: np.ndarray   # the matched ground-truth row's id, -1
    tr_iou: np.ndarray
    tr_level: np.ndarray
    gt_identities: np.ndarray   # int32 [G]: the ids of the tables' rows
    gt_count: np.ndarray        # int32 [G]: kept rows of the identity (its length)
    gt_tp: np.ndarray           # int32 [G, 19]
    gt_num: np.ndarray          # float64 [G, 2, 19]
    gt_n_partners: np.ndarray   # int32 [G]: tracker ids matched at alpha_index
    gt_top_partner: np.ndarray  # int32 [G]: the one matched most often there (ties: the lowest id), -1
    gt_top_count: np.ndarray    # int32 [G]
    gt_id_partner: np.ndarray   # int32 [G]: the tracker id the Identity metric credits, -1
    gt_idtp: np.ndarray         # int32 [G]
    tr_identities: np.ndarray
    tr_count: np.ndarray
    tr_tp: np.ndarray
    tr_num: np.ndarray
    tr_n_partners: np.ndarray
    tr_top_partner: np.ndarray
    tr_top_count: np.ndarray
    tr_id_partner: np.ndarray
    tr_idtp: np.ndarray

    ROW_ARRAYS = ("gt_off", "tr_off", "gt_ids", "gt_boxes", "gt_kept", "gt_partner_id", "gt_iou", "gt_level", "tr_ids",
                  "tr_boxes", "tr_kept", "tr_partner_id", "tr_iou", "tr_level")
    INT_TABLES = ("gt_identities", "gt_count", "gt_tp", "gt_n_partners", "gt_top_partner", "gt_top_count",
                  "gt_id_partner", "gt_idtp", "tr_identities", "tr_count", "tr_tp", "tr_n_partners", "tr_top_partner",
                  "tr_top_count", "tr_id_partner", "tr_idtp")
    FLOAT_TABLES = ("gt_num", "tr_num")

    @property
    def n_frames(self) -> int:
        return len(self.gt_off) - 1

    def _ratio(self, side: str, which: int) -> np.ndarray:
        tp, num = getattr(self, side + "_tp"), getattr(self, side + "_num")
        return (num[:, which] / np.maximum(1, tp)).mean(1) if len(tp) else np.zeros(0)

    def ass_a(self, side: str = "gt") -> np.ndarray:
        """float64 per identity: the mean over the thresholds of ``ass_num / max(1, tp)``."""
        return self._ratio(side, 0)

    def ass_re(self) -> np.ndarray:
        return self._ratio("gt", 1)

    def ass_pr(self) -> np.ndarray:
        return self._ratio("tr", 1)

    def id_f1(self, side: str = "gt") -> np.ndarray:
        """float64 per identity: ``2 idtp / (own length + the credited partner's length)``."""
        other = "tr" if side == "gt" else "gt"
        mine, partner = getattr(self, side + "_count"), getattr(self, side + "_id_partner")
        theirs = np.zeros(len(mine), np.int64)
        hit = partner >= 0
        theirs[hit] = getattr(self, other + "_count")[np.searchsorted(getattr(self, other + "_identities"), partner[hit])]
        return 2.0 * getattr(self, side + "_idtp") / np.maximum(1, mine + theirs)

    def totals(self) -> dict:
        """The sums ``evaluation`` forms its fields from, out of the per-identity tables: ``HOTA_TP`` int64 [19]; the
        ``AssA`` / ``AssRe`` / ``AssPr`` numerators float64 [19] (``hota_sums[:3]``); ``IDTP``, ``IDFN``, ``IDFP``."""
        idtp = int(self.gt_idtp.sum())
        return {"HOTA_TP": self.gt_tp.sum(0).astype(np.int64), "AssA": self.gt_num[:, 0].sum(0),
                "AssRe": self.gt_num[:, 1].sum(0), "AssPr": self.tr_num[:, 1].sum(0), "IDTP": idtp,
                "IDFN": int(self.gt_count.sum()) - idtp, "IDFP": int(self.tr_count.sum()) - idtp}

    def worst_identities(self, n: int = 10) -> List[Tuple[int, float, int, int]]:
        """(gt_id, AssA, length, n_partners) of ``n`` ground-truth identities: those matched at ``alpha_index`` by AssA,
        lowest first (ties by id), then the never-matched ones, longest first."""
        score, matched = self.ass_a(), self.gt_tp[:, self.alpha_index] > 0
        order = [i for i in np.argsort(score, kind="stable") if matched[i]]
        order += [i for i in np.argsort(-self.gt_count, kind="stable") if not matched[i]]
        return [(int(self.gt_identities[i]), float(score[i]), int(self.gt_count[i]), int(self.gt_n_partners[i]))
                for i in order[:max(int(n), 0)]]

    def fragments(self, gt_id: int) -> List[Tuple[int, int, int]]:
        """(first_frame, last_frame, tracker_id) of every run of consecutive frames in which ``gt_id`` is a true
        positive at ``alpha_index`` with the same tracker id; a frame without a match, or without the id, ends a run."""
        frame = np.repeat(np.arange(1, self.n_frames + 1), np.diff(self.gt_off))
        rows = np.flatnonzero((self.gt_ids == gt_id) & self.gt_kept & (self.gt_level > self.alpha_index))
        out: List[Tuple[int, int, int]] = []
        for r in rows:
            f, t = int(frame[r]), int(self.gt_partner_id[r])
            if out and out[-1][2] == t and out[-1][1] == f - 1:
                out[-1] = (out[-1][0], f, t)
            else:
                out.append((f, f, t))
        return out

    def write_rows_csv(self, path: str) -> None:
        """One line per input row, ground truth before tracker rows within a frame (``ROWS_HEADER``); floats as Python
        prints them, partner_id -1, iou 0 and level 0 without a partner."""
        lines = [ROWS_HEADER]
        for f in range(self.n_frames):
            for side in ("gt", "tr"):
                off, get = getattr(self, side + "_off"), lambda k: getattr(self, side + "_" + k)  # noqa: E731,B023
                for i in range(int(off[f]), int(off[f + 1])):
                    box = ",".join(repr(float(v)) for v in get("boxes")[i])
                    lines.append(f"{f + 1},{side},{int(get('ids')[i])},{box},{int(get('kept')[i])},"
                                 f"{int(get('partner_id')[i])},{float(get('iou')[i])!r},{int(get('level')[i])}")
        _write_text(path, lines)

    def write_identities_csv(self, path: str) -> None:
        """One line per identity, ground truth before tracker ids (``IDENTITIES_HEADER``; ``tp50``: the true positives
        at ``alpha_index``, 0.5 by default)."""
        lines = [IDENTITIES_HEADER]
        for side, second in (("gt", self.ass_re()), ("tr", self.ass_pr())):
            get = lambda k: getattr(self, side + "_" + k)                                        # noqa: E731,B023
            ass_a, id_f1 = self.ass_a(side), self.id_f1(side)
            for i, ident in enumerate(get("identities")):
                lines.append(f"{side},{int(ident)},{int(get('count')[i])},{int(get('tp')[i, self.alpha_index])},"
                             f"{float(ass_a[i])!r},{float(second[i])!r},{int(get('n_partners')[i])},"
                             f"{int(get('top_partner')[i])},{int(get('top_count')[i])},{int(get('id_partner')[i])},"
                             f"{int(get('idtp')[i])},{float(id_f1[i])!r}")
        _write_text(path, lines)


def _write_text(path: str, lines: List[str]) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


# --------------------------------------------------------------------------------- the definition, on the host
def _hota_events_host(d: dict, sim: np.ndarray) -> dict:
    """``evaluation._hota_host`` and ``evaluation._identity_host`` over the preprocessed data ``d``
    (``evaluation._compact``) with the pairs kept: the statement the kernels are held to.  Per compact row
    ``gt_partner`` / ``tr_partner`` (the partner's index within its frame, -1) and ``gt_level`` / ``tr_level``; per
    relabelled id, all sequences one behind the other (``gid_off`` / ``tid_off``), ``gt_count``, ``gt_id_partner`` (a
    relabelled tracker id, -1), ``gt_idtp`` and the tracker side's mirror; ``matches`` int32, per sequence [19, G, K]
    behind ``19 * cell_off``.  A sequence with an empty side is not walked, as ``host_tables`` skips it."""
    S = len(d["seq_off"]) - 1
    n_gid, n_tid = int(d["gid_off"][-1]), int(d["tid_off"][-1])
    out = {"gt_partner": np.full(len(d["gt_ids"]), -1, np.int32), "gt_level": np.zeros(len(d["gt_ids"]), np.int32),
           "tr_partner": np.full(len(d["tr_ids"]), -1, np.int32), "tr_level": np.zeros(len(d["tr_ids"]), np.int32),
           "gt_count": np.zeros(n_gid, np.int32), "tr_count": np.zeros(n_tid, np.int32),
           "gt_id_partner": np.full(n_gid, -1, np.int32), "gt_idtp": np.zeros(n_gid, np.int32),
           "tr_id_partner": np.full(n_tid, -1, np.int32), "tr_idtp": np.zeros(n_tid, np.int32),
           "matches": np.zeros(N_ALPHA * int(d["cell_off"][-1]), np.int32)}
    for s in range(S):
        G, K = int(d["n_gt_ids"][s]), int(d["n_tr_ids"][s])
        a0, a1, b0, b1 = (int(d[k][d["seq_off"][s + e]]) for k in ("gt_off", "tr_off") for e in (0, 1))
        gc, tc = np.bincount(d["gt_ids"][a0:a1], minlength=G), np.bincount(d["tr_ids"][b0:b1], minlength=K)
        out["gt_count"][d["gid_off"][s]:d["gid_off"][s + 1]] = gc
        out["tr_count"][d["tid_off"][s]:d["tid_off"][s + 1]] = tc
        if d["n_gt_dets"][s] == 0 or d["n_tr_dets"][s] == 0:
            continue
        frames = list(E._frames_of(d, sim, s))
        potential, both = np.zeros((G, K)), np.zeros((G, K), np.int64)
        for gi, ti, sm in frames:       # how much of each other two ids see, before any matching (_hota_host)
            denom = sm.sum(0)[None, :] + sm.sum(1)[:, None] - sm
            share = np.zeros_like(sm)
            np.divide(sm, denom, out=share, where=denom > 0 + E.EPS)
            potential[gi[:, None], ti[None, :]] += share
            r, c = np.nonzero(sm >= E.THRESHOLD)
            both[gi[r], ti[c]] += 1
        alignment = potential / (gc[:, None].astype(np.float64) + tc[None, :] - potential)
        matches = out["matches"][N_ALPHA * d["cell_off"][s]:N_ALPHA * d["cell_off"][s + 1]].reshape(N_ALPHA, G, K)
        for f, (gi, ti, sm) in zip(range(d["seq_off"][s], d["seq_off"][s + 1]), frames):
            if len(gi) == 0 or len(ti) == 0:
                continue
            rows, cols = E._assign(-(alignment[gi[:, None], ti[None, :]] * sm))
            level = (sm[rows, cols][:, None] >= E.ALPHAS[None, :] - E.EPS).sum(1)
            hit = level > 0
            rows, cols, level = rows[hit], cols[hit], level[hit]
            g0, t0 = d["gt_off"][f], d["tr_off"][f]
            out["gt_partner"][g0 + rows], out["gt_level"][g0 + rows] = cols, level
            out["tr_partner"][t0 + cols], out["tr_level"][t0 + cols] = rows, level
            for a in range(N_ALPHA):
                matches[a, gi[rows[level > a]], ti[cols[level > a]]] += 1
        # the Identity metric's map of whole trajectories (_identity_host)
        fn, fp = np.zeros((G + K, G + K)), np.zeros((G + K, G + K))
        fn[:G, K:], fp[G:, :K] = 1e10, 1e10
        fn[:G, :K] = gc[:, None] - both
        fn[np.arange(G), K + np.arange(G)] = gc
        fp[:G, :K] = tc[None, :] - both
        fp[G + np.arange(K), np.arange(K)] = tc
        rows, cols = E._assign(fn + fp)
        pair = (rows < G) & (cols < K)
        g, k = rows[pair], cols[pair]
        out["gt_id_partner"][d["gid_off"][s] + g], out["gt_idtp"][d["gid_off"][s] + g] = k, both[g, k]
        out["tr_id_partner"][d["tid_off"][s] + k], out["tr_idtp"][d["tid_off"][s] + k] = g, both[g, k]
    return out


def _reduce_host(d: dict, ev: dict, alpha_index: int) -> dict:
    """The per-identity tables from ``matches``, ``gt_count`` and ``tr_count``: ``gt_tp`` int32 [sum G, 19], ``gt_num``
    float64 [sum G, 2, 19], ``gt_top`` int32 [sum G, 3] (n_partners, top_partner as a relabelled id, top_count), and the
    tracker side's.  Every product and quotient as written: two roundings."""
    n_gid, n_tid = int(d["gid_off"][-1]), int(d["tid_off"][-1])
    out = {"gt_tp": np.zeros((n_gid, N_ALPHA), np.int32), "gt_num": np.zeros((n_gid, 2, N_ALPHA)),
           "gt_top": np.tile(np.array([0, -1, 0], np.int32), (n_gid, 1)),
           "tr_tp": np.zeros((n_tid, N_ALPHA), np.int32), "tr_num": np.zeros((n_tid, 2, N_ALPHA)),
           "tr_top": np.tile(np.array([0, -1, 0], np.int32), (n_tid, 1))}
    for s in range(len(d["seq_off"]) - 1):
        G, K = int(d["n_gt_ids"][s]), int(d["n_tr_ids"][s])
        if G == 0 or K == 0:
            continue
        gs, ts = slice(d["gid_off"][s], d["gid_off"][s + 1]), slice(d["tid_off"][s], d["tid_off"][s + 1])
        mi = ev["matches"][N_ALPHA * d["cell_off"][s]:N_ALPHA * d["cell_off"][s + 1]].reshape(N_ALPHA, G, K)
        m = mi.astype(np.float64)
        gc, tc = ev["gt_count"][gs][None, :, None].astype(np.float64), ev["tr_count"][ts][None, None, :].astype(np.float64)
        ass = m * (m / np.maximum(1, gc + tc - m))
        re, pr = m * (m / np.maximum(1, gc)), m * (m / np.maximum(1, tc))
        out["gt_tp"][gs], out["tr_tp"][ts] = mi.sum(2).T, mi.sum(1).T
        out["gt_num"][gs] = np.stack([ass.sum(2).T, re.sum(2).T], 1)
        out["tr_num"][ts] = np.stack([ass.sum(1).T, pr.sum(1).T], 1)
        for key, sl, m0 in (("gt_top", gs, mi[alpha_index]), ("tr_top", ts, mi[alpha_index].T)):
            top = m0.argmax(1)                          # (the first of equal maxima: the lowest id)
            count = m0[np.arange(len(m0)), top]
            out[key][sl] = np.stack([(m0 > 0).sum(1), np.where(count > 0, top, -1), count], 1)
    return out


def _to_input_rows(gt_ids, tr_ids, gt_off, tr_off, d: dict, ev: dict, sim) -> dict:
    """The compact events scattered back to the input rows through the keep indices (``diagnose._to_input_rows``' way):
    a dropped row has kept False, partner -1, level 0; a partner is named by its id as the files give it; iou is the
    pair's similarity entry.  Everything is a torch tensor on ``sim``'s device; a few index operations."""
    import torch
    dev = sim.device
    i64 = lambda x: torch.as_tensor(x, device=dev).long()                                       # noqa: E731
    gt_ids, tr_ids, gt_off, tr_off = i64(gt_ids), i64(tr_ids), i64(gt_off), i64(tr_off)
    c_gt_off, c_tr_off, sim_off = i64(d["gt_off"]), i64(d["tr_off"]), i64(d["sim_off"])
    keep_gt, keep_tr = i64(d["keep_gt"]), i64(d["keep_tr"])
    frames = torch.arange(len(gt_off) - 1, device=dev)
    gt_frame = torch.repeat_interleave(frames, c_gt_off[1:] - c_gt_off[:-1])        # the frame of a compact row
    tr_frame = torch.repeat_interleave(frames, c_tr_off[1:] - c_tr_off[:-1])
    gp, gl, tp, tl = (i64(ev[k]) for k in ("gt_partner", "gt_level", "tr_partner", "tr_level"))
    NG, NT = len(gt_ids), len(tr_ids)
    new = lambda n, fill, dt: torch.full((n,), fill, dtype=dt, device=dev)                      # noqa: E731
    out = {}
    for side, n, keep in (("gt", NG, keep_gt), ("tr", NT, keep_tr)):
        out[side + "_kept"] = new(n, False, torch.bool)
        out[side + "_kept"][keep] = True
        out[side + "_partner_id"], out[side + "_level"] = new(n, -1, torch.int32), new(n, 0, torch.int32)
        out[side + "_iou"] = new(n, 0.0, torch.float64)
    rows = (gp >= 0).nonzero().reshape(-1)
    fr = gt_frame[rows]
    width = c_tr_off[fr + 1] - c_tr_off[fr]
    out["gt_partner_id"][keep_gt[rows]] = tr_ids[keep_tr[c_tr_off[fr] + gp[rows]]].int()
    out["gt_iou"][keep_gt[rows]] = sim[sim_off[fr] + (rows - c_gt_off[fr]) * width + gp[rows]]
    out["gt_level"][keep_gt[rows]] = gl[rows].int()
    rows = (tp >= 0).nonzero().reshape(-1)
    fr = tr_frame[rows]
    width = c_tr_off[fr + 1] - c_tr_off[fr]
    out["tr_partner_id"][keep_tr[rows]] = gt_ids[keep_gt[c_gt_off[fr] + tp[rows]]].int()
    out["tr_iou"][keep_tr[rows]] = sim[sim_off[fr] + tp[rows] * width + (rows - c_tr_off[fr])]
    out["tr_level"][keep_tr[rows]] = tl[rows].int()
    return out


def association_host(packed: E.PackedSequences, benchmark: str = "MOT17",
                     alpha_index: int = DEFAULT_ALPHA_INDEX) -> dict:
    """The association of every input row and every identity of ``packed`` as numpy arrays over all sequences: per row
    ``gt_kept``, ``gt_partner_id``, ``gt_iou``, ``gt_level`` and the tracker side's; per identity (all sequences one
    behind the other, ``gid_off`` / ``tid_off``) ``gt_count``, ``gt_tp``, ``gt_num``, ``gt_top``, ``gt_id_partner``,
    ``gt_idtp`` with relabelled partner ids, and the tracker side's; ``matches`` and the compact events
    (``c::gt_partner`` ...).  MOT17 rules, or MOT15 without preprocessing; not BDD100K."""
    import torch
    _check_benchmark(benchmark)
    alpha_index = _check_alpha_index(alpha_index)
    p = packed.numpy()
    _, sim, d = E._preprocess_host(p, benchmark)
    ev = _hota_events_host(d, sim)
    rows = _to_input_rows(p.gt_ids, p.tr_ids, p.gt_off, p.tr_off, d, ev,
                          torch.from_numpy(np.ascontiguousarray(sim, np.float64)))
    out = {k: v.numpy() for k, v in rows.items()}
    out.update(_reduce_host(d, ev, alpha_index))
    out.update({k: ev[k] for k in ("gt_count", "tr_count", "gt_id_partner", "gt_idtp", "tr_id_partner", "tr_idtp",
                                   "matches")})
    out.update({"c::" + k: ev[k] for k in ("gt_partner", "gt_level", "tr_partner", "tr_level")})
    out.update(_identity_tables(p, d))
    return out


def _identity_tables(p: E.PackedSequences, d: dict) -> dict:
    """``gid_off`` / ``tid_off`` and, per relabelled id, the id as the files give it (the relabelling is the rank among
    the sequence's distinct kept ids)."""
    names = {"gt": [], "tr": []}
    for s in range(len(p.seq_off) - 1):
        for side, ids, keep in (("gt", p.gt_ids, d["keep_gt"]), ("tr", p.tr_ids, d["keep_tr"])):
            off = d[side + "_off"]
            names[side].append(np.unique(ids[keep[off[p.seq_off[s]]:off[p.seq_off[s + 1]]]]))
    cat = lambda parts: np.concatenate(parts + [np.zeros(0, np.int32)]).astype(np.int32)         # noqa: E731
    return {"gid_off": d["gid_off"], "tid_off": d["tid_off"], "gt_identities": cat(names["gt"]),
            "tr_identities": cat(names["tr"])}


def _split(p: E.PackedSequences, t: dict, alpha_index: int) -> Dict[str, SequenceAssociation]:
    """Per sequence, from host arrays; relabelled partner ids become the ids the files give."""
    out = {}
    for s, name in enumerate(p.names):
        f0, f1 = int(p.seq_off[s]), int(p.seq_off[s + 1])
        g0, g1, t0, t1 = int(p.gt_off[f0]), int(p.gt_off[f1]), int(p.tr_off[f0]), int(p.tr_off[f1])
        gs, ts = slice(int(t["gid_off"][s]), int(t["gid_off"][s + 1])), slice(int(t["tid_off"][s]), int(t["tid_off"][s + 1]))
        gt_names, tr_names = t["gt_identities"][gs], t["tr_identities"][ts]

        def named(partner, names):
            safe = np.concatenate([names, np.full(1, -1, np.int32)])            # (index -1: no partner)
            return safe[partner].astype(np.int32)

        out[name] = SequenceAssociation(
            name, alpha_index, (p.gt_off[f0:f1 + 1] - g0).astype(np.int32), (p.tr_off[f0:f1 + 1] - t0).astype(np.int32),
            p.gt_ids[g0:g1], p.gt_boxes[g0:g1], t["gt_kept"][g0:g1], t["gt_partner_id"][g0:g1], t["gt_iou"][g0:g1],
            t["gt_level"][g0:g1], p.tr_ids[t0:t1], p.tr_boxes[t0:t1], t["tr_kept"][t0:t1], t["tr_partner_id"][t0:t1],
            t["tr_iou"][t0:t1], t["tr_level"][t0:t1],
            gt_names, t["gt_count"][gs], t["gt_tp"][gs], t["gt_num"][gs], t["gt_top"][gs, 0],
            named(t["gt_top"][gs, 1], tr_names), t["gt_top"][gs, 2], named(t["gt_id_partner"][gs], tr_names),
            t["gt_idtp"][gs],
            tr_names, t["tr_count"][ts], t["tr_tp"][ts], t["tr_num"][ts], t["tr_top"][ts, 0],
            named(t["tr_top"][ts, 1], gt_names), t["tr_top"][ts, 2], named(t["tr_id_partner"][ts], gt_names),
            t["tr_idtp"][ts])
    return out


# ------------------------------------------------------------------------------------------------ the device path
def launch_hota_events(sim, sim_off, gt_off, tr_off, gt_ids, tr_ids, frame_seq, n_tr_ids, cell_off, alignment,
                       max_gt: int, max_tr: int, gt_partner, gt_level, tr_partner, tr_level, matches, status,
                       spare=None) -> None:
    """``clipops_hota_events_f64`` on the current stream: contiguous CUDA tensors with the dtypes of
    include/clip_ops_hip.h; the five outputs are written whole, ``matches`` (zeroed by the caller, or None) is
    incremented; nothing waits."""
    alphas = np.ascontiguousarray(E.ALPHAS, np.float64)
    E._launch("clipops_hota_events_f64", sim.device,
              [sim, sim_off, gt_off, tr_off, gt_ids, tr_ids, frame_seq, int(gt_off.numel()) - 1, n_tr_ids, cell_off,
               alignment, alphas.ctypes.data, int(max_gt), int(max_tr), gt_partner, gt_level, tr_partner, tr_level,
               matches, status], spare)


def launch_identity_pairs(n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off, gt_count, tr_count, id_matches, max_ids: int,
                          gt_id_partner, gt_idtp, tr_id_partner, tr_idtp, status, spare=None) -> None:
    """``clipops_identity_pairs_i32`` on the current stream; the five outputs are written whole."""
    E._launch("clipops_identity_pairs_i32", n_gt_ids.device,
              [int(n_gt_ids.numel()), n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off, gt_count, tr_count, id_matches,
               int(max_ids), gt_id_partner, gt_idtp, tr_id_partner, tr_idtp, status], spare)


def launch_assoc_reduce(n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off, gt_count, tr_count, matches, max_side_ids: int,
                        alpha_index: int, gt_tp, gt_num, gt_top, tr_tp, tr_num, tr_top, spare=None) -> None:
    """``clipops_assoc_reduce_f64`` on the current stream; the six outputs are written whole."""
    E._launch("clipops_assoc_reduce_f64", n_gt_ids.device,
              [int(n_gt_ids.numel()), n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off, gt_count, tr_count, matches,
               int(max_side_ids), int(alpha_index), gt_tp, gt_num, gt_top, tr_tp, tr_num, tr_top], spare)


def launch_timeline(gt_off, gt_ids, partner_id, level, n_ids: int, alpha_index: int, cell_w: int, cell_h: int, bgr: bool,
                    image, spare=None) -> None:
    """``clipops_timeline_u8`` on the current stream, into ``image`` uint8 (n_ids * cell_h, F * cell_w, 3)."""
    E._launch("clipops_timeline_u8", image.device,
              [gt_off, gt_ids, partner_id, level, int(n_ids), int(gt_off.numel()) - 1, int(alpha_index), int(cell_w),
               int(cell_h), int(bool(bgr)), image], spare)


def device_association_tables(packed: E.PackedSequences, benchmark: str = "MOT17",
                              alpha_index: int = DEFAULT_ALPHA_INDEX, timings: dict = None) -> dict:
    """``association_host``'s arrays by the kernels, as torch tensors on ``packed``'s device:
    ``evaluation.device_front`` and ``evaluation.device_accumulate``, then the four launches of this module's kernels,
    and the scatter to the input rows in index operations.  The front waits for the device (the compaction and the
    relabelling are the host's); behind it nothing waits: the status words of the launches are returned as
    ``frame_status`` / ``id_status`` for ``raise_on_status`` once they are on the host.  ``timings``: a dict that
    receives, per launch of this module's kernels, a list of (start, end) event pairs (tools/bench_assoc.py)."""
    import torch
    with E._on_stream(packed.gt_boxes.device):
        fr = E.device_front(packed, benchmark, on_host="analyse")
        acc = E.device_accumulate(fr)
        S, F, dev, new, timed = fr.S, fr.F, fr.dev, fr.new, E._timed(timings)
        n_gt, n_tr, n_gid, n_tid, cells = len(fr.d["gt_ids"]), len(fr.d["tr_ids"]), fr.n_gid, fr.n_tid, fr.cells
        ev = {"gt_partner": new(n_gt, torch.int32), "gt_level": new(n_gt, torch.int32),
              "tr_partner": new(n_tr, torch.int32), "tr_level": new(n_tr, torch.int32)}
        matches = new(N_ALPHA * cells, torch.int32, 0)
        frame_status, id_status = new(F, torch.int32), new(S, torch.int32)
        ids = {"gt_id_partner": new(n_gid, torch.int32), "gt_idtp": new(n_gid, torch.int32),
               "tr_id_partner": new(n_tid, torch.int32), "tr_idtp": new(n_tid, torch.int32)}
        tables = {"gt_tp": torch.empty((max(n_gid, 1), N_ALPHA), dtype=torch.int32, device=dev),
                  "gt_num": torch.empty((max(n_gid, 1), 2, N_ALPHA), dtype=torch.float64, device=dev),
                  "gt_top": torch.empty((max(n_gid, 1), 3), dtype=torch.int32, device=dev),
                  "tr_tp": torch.empty((max(n_tid, 1), N_ALPHA), dtype=torch.int32, device=dev),
                  "tr_num": torch.empty((max(n_tid, 1), 2, N_ALPHA), dtype=torch.float64, device=dev),
                  "tr_top": torch.empty((max(n_tid, 1), 3), dtype=torch.int32, device=dev)}
        if F:
            timed("clipops_hota_events_f64", launch_hota_events, fr.sim, fr.sim_off, fr.gt_off, fr.tr_off, fr.gt_ids,
                  fr.tr_ids, fr.frame_seq, fr.n_tr_ids, fr.cell_off, acc["alignment"], fr.max_gt, fr.max_tr,
                  ev["gt_partner"], ev["gt_level"], ev["tr_partner"], ev["tr_level"], matches, frame_status, fr.spare)
        if S:
            timed("clipops_identity_pairs_i32", launch_identity_pairs, fr.n_gt_ids, fr.n_tr_ids, fr.cell_off,
                  fr.gid_off, fr.tid_off, acc["gt_count"], acc["tr_count"], acc["id_matches"], fr.max_ids,
                  ids["gt_id_partner"], ids["gt_idtp"], ids["tr_id_partner"], ids["tr_idtp"], id_status, fr.spare)
            timed("clipops_assoc_reduce_f64", launch_assoc_reduce, fr.n_gt_ids, fr.n_tr_ids, fr.cell_off, fr.gid_off,
                  fr.tid_off, acc["gt_count"], acc["tr_count"], matches, fr.max_side, alpha_index, tables["gt_tp"],
                  tables["gt_num"], tables["gt_top"], tables["tr_tp"], tables["tr_num"], tables["tr_top"], fr.spare)
        ev = {"gt_partner": ev["gt_partner"][:n_gt], "gt_level": ev["gt_level"][:n_gt],
              "tr_partner": ev["tr_partner"][:n_tr], "tr_level": ev["tr_level"][:n_tr]}
        out = _to_input_rows(fr.tens["gt_ids"], fr.tens["tr_ids"], fr.host.gt_off, fr.host.tr_off, fr.d, ev, fr.sim)
        out.update({"gt_count": acc["gt_count"][:n_gid], "tr_count": acc["tr_count"][:n_tid],
                    "matches": matches[:N_ALPHA * cells]})
        out.update({k: v[:n_gid if k.startswith("gt") else n_tid] for k, v in list(ids.items()) + list(tables.items())})
        out.update({"c::" + k: v for k, v in ev.items()})
        out["frame_status"], out["id_status"] = frame_status[:F], id_status[:S]
        out["host"] = _identity_tables(fr.host, fr.d)
        return out


def raise_on_status(frame_status, id_status) -> None:
    """The status words of ``device_association_tables`` (host arrays or tensors): raises for a frame or a sequence
    whose assignment was infeasible or larger than its launch was sized for."""
    for status, what, unit in ((frame_status, "HOTA events", "frame"), (id_status, "Identity pairs", "sequence")):
        bad = np.flatnonzero(np.asarray(status.cpu() if hasattr(status, "cpu") else status))
        if len(bad):
            code = int(status[int(bad[0])])
            why = "exceeds the size the launch was made for" if code == -2 else "has no feasible assignment"
            raise RuntimeError(f"{what}: {unit} {int(bad[0])} {why} (status {code})")


def _one_copy(tensors: dict) -> dict:
    """Device tensors as host arrays through one buffer: every tensor's bytes behind one another (8-byte aligned) in
    one uint8 tensor, one copy of it to the host, views of the copy."""
    import torch
    parts, layout, at = [], {}, 0
    for k, v in tensors.items():
        flat = v.contiguous().view(-1).view(torch.uint8)
        pad = -flat.numel() % 8
        parts += [flat, flat.new_zeros(pad)]
        layout[k] = (at, flat.numel(), v)
        at += flat.numel() + pad
    host = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, np.uint8)        # (the one host copy; synchronises)
    np_dtype = lambda t: torch.empty(0, dtype=t.dtype).numpy().dtype                             # noqa: E731
    return {k: host[a:a + n].view(np_dtype(v)).reshape(tuple(v.shape)) for k, (a, n, v) in layout.items()}


def association(packed: E.PackedSequences, benchmark: str = "MOT17", device=None,
                alpha_index: int = DEFAULT_ALPHA_INDEX) -> Dict[str, SequenceAssociation]:
    """``{name: SequenceAssociation}``.  ``device``: a CUDA device for the kernels (a missing library raises); "cpu" or
    None (the default) for the host statement, to which device tensors are copied."""
    _check_benchmark(benchmark)
    alpha_index = _check_alpha_index(alpha_index)
    if device is not None and str(device).startswith("cuda"):
        t = device_association_tables(packed if packed.is_device() else packed.to(device), benchmark, alpha_index)
        host = t.pop("host")
        t.pop("matches")
        t = _one_copy(t)
        raise_on_status(t.pop("frame_status"), t.pop("id_status"))
        t.update(host)
    else:
        t = association_host(packed, benchmark, alpha_index)
    return _split(packed.numpy(), t, alpha_index)


def association_from_files(gt_root: str, tracker_dir: str, seqmap: str, benchmark: str = "MOT17",
                           device=None, alpha_index: int = DEFAULT_ALPHA_INDEX) -> Dict[str, SequenceAssociation]:
    """The association of result files in ``evaluation.evaluate_files``' layout, with its arguments."""
    return E.load_files(gt_root, tracker_dir, seqmap, benchmark, device).association(alpha_index)


# --------------------------------------------------------------------------------------------------- the timeline
def _timeline_rows(assoc: SequenceAssociation):
    """The kept ground-truth rows of a sequence as the timeline takes them: offsets per frame, the identity's row in
    the picture, the partner's id, the level."""
    count = np.concatenate(([0], np.cumsum(assoc.gt_kept)))[assoc.gt_off].astype(np.int32)
    kept = assoc.gt_kept
    row = np.searchsorted(assoc.gt_identities, assoc.gt_ids[kept]).astype(np.int32)
    return count, row, assoc.gt_partner_id[kept].astype(np.int32), assoc.gt_level[kept].astype(np.int32)


def _timeline_size(assoc: SequenceAssociation, alpha_index, cell_w: int, cell_h: int):
    alpha_index = _check_alpha_index(assoc.alpha_index if alpha_index is None else alpha_index)
    if int(cell_w) < 1 or int(cell_h) < 1:
        raise ValueError(f"cell_w {cell_w!r} and cell_h {cell_h!r} must be at least 1")
    G, F = len(assoc.gt_identities), assoc.n_frames
    if G * int(cell_h) > MAX_IMAGE_SIDE or F * int(cell_w) > MAX_IMAGE_SIDE:
        raise ValueError(f"sequence {assoc.name}: a timeline of {F * int(cell_w)} x {G * int(cell_h)} pixels exceeds "
                         f"{MAX_IMAGE_SIDE} on a side (use smaller cells)")
    return alpha_index, G, F


def timeline_host(assoc: SequenceAssociation, alpha_index: Optional[int] = DEFAULT_ALPHA_INDEX, cell_w: int = 2,
                  cell_h: int = 6, bgr: bool = False) -> np.ndarray:
    """The identity timeline, uint8 (G * cell_h, F * cell_w, 3): one row of cells per surviving ground-truth identity
    in ascending id, one column per frame.  A cell is black where the identity has no kept row, (96, 96, 96) where its
    row is no true positive at ``alpha_index``, else ``render.PALETTE[partner tracker id % 64]`` (channels swapped for
    ``bgr``)."""
    from .render import PALETTE
    alpha_index, G, F = _timeline_size(assoc, alpha_index, cell_w, cell_h)
    off, row, partner, level = _timeline_rows(assoc)
    cells = np.zeros((G, F, 3), np.uint8)
    frame = np.repeat(np.arange(F), np.diff(off))
    for f, g, p, lv in zip(frame, row, partner, level):
        c = PALETTE[int(p) % 64] if lv > alpha_index and p >= 0 else UNMATCHED
        cells[g, f] = c[::-1] if bgr and c is not UNMATCHED else c
    return np.repeat(np.repeat(cells, int(cell_h), 0), int(cell_w), 1)


def timeline(assoc: SequenceAssociation, alpha_index: Optional[int] = DEFAULT_ALPHA_INDEX, cell_w: int = 2,
             cell_h: int = 6, bgr: bool = False, device=None):
    """``timeline_host``; with a CUDA ``device`` by ``clipops_timeline_u8`` (one upload of the sequence's rows, one
    launch on the current stream), a torch uint8 tensor on that device."""
    import torch
    if device is None or not str(device).startswith("cuda"):
        return torch.from_numpy(timeline_host(assoc, alpha_index, cell_w, cell_h, bgr))
    alpha_index, G, F = _timeline_size(assoc, alpha_index, cell_w, cell_h)
    image = torch.empty((G * int(cell_h), F * int(cell_w), 3), dtype=torch.uint8, device=device)
    off, row, partner, level = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in _timeline_rows(assoc))
    if G and F:
        launch_timeline(off, row, partner, level, G, alpha_index, cell_w, cell_h, bgr, image)
    return image


def write_timeline(assoc: SequenceAssociation, path: str, quality: int = 90, device=None,
                   alpha_index: Optional[int] = DEFAULT_ALPHA_INDEX, cell_w: int = 2, cell_h: int = 6) -> str:
    """The timeline as a baseline JPEG without chroma subsampling (its cells are a few pixels wide)."""
    from .data.jpeg_write import encode_jpeg
    image = timeline(assoc, alpha_index, cell_w, cell_h, False, device)
    if image.numel() == 0:
        raise ValueError(f"sequence {assoc.name}: no identity or no frame to draw")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(encode_jpeg(image, quality, subsampling="4:4:4"))
    return path


# ------------------------------------------------------------------------------------------------ the command line
def summary_text(assoc: Dict[str, SequenceAssociation], worst: int = 10) -> str:
    """Per sequence the totals and the ``worst`` identities with their fragments."""
    lines = []
    for name, a in assoc.items():
        t, i = a.totals(), a.alpha_index
        ass = [float(np.mean(t[k] / np.maximum(1, t["HOTA_TP"]))) for k in ("AssA", "AssRe", "AssPr")]
        lines.append(f"{name} HOTA_TP@{E.ALPHAS[i]:.2f}={int(t['HOTA_TP'][i])} AssA={ass[0]:.5f} AssRe={ass[1]:.5f} "
                     f"AssPr={ass[2]:.5f} IDTP={t['IDTP']} IDFN={t['IDFN']} IDFP={t['IDFP']}")
        for gt_id, score, length, n_partners in a.worst_identities(worst):
            runs = " ".join(f"{f0}-{f1}:{k}" for f0, f1, k in a.fragments(gt_id))
            lines.append(f"  gt {gt_id}: AssA={score:.5f} length={length} partners={n_partners} [{runs}]")
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m memotr_amd.association", description=__doc__.split("\n\n")[0])
    ap.add_argument("--gt-root", required=True)
    ap.add_argument("--tracker-dir", required=True)
    ap.add_argument("--seqmap", required=True)
    ap.add_argument("--benchmark", default="MOT17", choices=("MOT17", "MOT15"))
    ap.add_argument("--out", required=True, help="receives <seq>_rows.csv, <seq>_identities.csv, <seq>_timeline.jpg "
                                                 "and summary.txt")
    ap.add_argument("--device", default=None, help="a CUDA device for the kernels; default: the host statements")
    ap.add_argument("--alpha", type=float, default=0.5, help="the threshold of the timeline and the partner counts")
    ap.add_argument("--worst", type=int, default=10)
    args = ap.parse_args(argv)
    alpha_index = int(np.argmin(np.abs(E.ALPHAS - args.alpha)))
    if abs(E.ALPHAS[alpha_index] - args.alpha) > 1e-6:
        ap.error(f"--alpha {args.alpha} is not one of HOTA's thresholds 0.05, 0.10 .. 0.95")
    device = None if args.device in (None, "cpu") else args.device
    assoc = association_from_files(args.gt_root, args.tracker_dir, args.seqmap, args.benchmark, device, alpha_index)
    os.makedirs(args.out, exist_ok=True)
    for name, a in assoc.items():
        a.write_rows_csv(os.path.join(args.out, name + "_rows.csv"))
        a.write_identities_csv(os.path.join(args.out, name + "_identities.csv"))
        if len(a.gt_identities) and a.n_frames:
            write_timeline(a, os.path.join(args.out, name + "_timeline.jpg"), device=device, alpha_index=alpha_index)
    text = summary_text(assoc, args.worst)
    with open(os.path.join(args.out, "summary.txt"), "w") as f:
        f.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
