"""Shared by the post-process tests (memotr_amd/postprocess.py, ``ResultLog.filled`` / ``BankResultLog.filled``): result
rows with holes, an independent per-track loop in float64, logs built from rows, and a scripted stand-in model whose
tracks go unreported for a few frames."""
import numpy as np
import torch

from memotr_amd.results import BANK_ROW_I, ROW_F, BankResultLog, ResultLog, Rows


def rows_from_mask(present, seed=0, labels=None):
    """``Rows`` sorted by (frame, id) with a row wherever ``present[id, frame]``: pixel-scale boxes of -200 .. 2200,
    unit-scale scores, labels 0 .. 7 (constant along a track unless ``labels`` (n_ids, n_frames) is given)."""
    present = np.asarray(present, bool)
    n_ids, n_frames = present.shape
    rs = np.random.RandomState(seed)
    boxes = rs.uniform(-200, 2200, (n_ids, n_frames, 4)).astype(np.float32)
    scores = rs.uniform(0, 1, (n_ids, n_frames)).astype(np.float32)
    if labels is None:
        labels = np.repeat(rs.randint(0, 8, (n_ids, 1)), n_frames, axis=1)
    frames, ids = np.nonzero(present.T)                     # frame-major: sorted by (frame, id)
    return Rows(frames.astype(np.int64), ids.astype(np.int64), np.asarray(labels)[ids, frames].astype(np.int64),
                np.ascontiguousarray(boxes[ids, frames]), scores[ids, frames].copy())


def random_mask(n_ids, n_frames, drop, seed):
    return np.random.RandomState(seed).uniform(0, 1, (n_ids, n_frames)) >= drop


def runs_mask(n_ids, n_frames, fraction, longest, seed):
    """Every row present, then about ``fraction`` of them removed in runs of 1 .. ``longest`` frames."""
    rs = np.random.RandomState(seed)
    mask = np.ones((n_ids, n_frames), bool)
    while mask.mean() > 1 - fraction:
        i, f, n = rs.randint(n_ids), rs.randint(n_frames), 1 + rs.randint(longest)
        mask[i, f:f + n] = False
    return mask


def empty_rows():
    return Rows(np.zeros((0,), np.int64), np.zeros((0,), np.int64), np.zeros((0,), np.int64),
                np.zeros((0, 4), np.float32), np.zeros((0,), np.float32))


def values_of(rows):
    return np.concatenate((rows.boxes_xyxy, rows.scores[:, None]), axis=1)


def loop_fill(rows, max_gap, min_length=0):
    """The definition again, as a plain loop over tracks in Python floats (float64): a list of
    ``(frame, id, label, values, ends)`` sorted by (frame, id); ``values`` are the five numbers, exact for an input row
    (``ends`` None) and ``a + (b - a) * k / (m + 1)`` for a new one (``ends`` = the (a, b) pairs)."""
    tracks = {}
    vals = values_of(rows)
    for i in range(len(rows.frames)):
        tracks.setdefault(int(rows.ids[i]), []).append((int(rows.frames[i]), int(rows.labels[i]),
                                                        [float(v) for v in vals[i]]))
    out = []
    for tid, track in tracks.items():
        if len(track) < min_length:
            continue
        track.sort(key=lambda r: r[0])
        for n, (f0, label, a) in enumerate(track):
            out.append((f0, tid, label, a, None))
            if n + 1 == len(track):
                break
            f1, _, b = track[n + 1]
            m = f1 - f0 - 1
            if 1 <= m <= max_gap:
                for k in range(1, m + 1):
                    out.append((f0 + k, tid, label, [x + (y - x) * k / (m + 1) for x, y in zip(a, b)],
                                list(zip(a, b))))
    out.sort(key=lambda r: (r[0], r[1]))
    return out


def assert_same_rows(got, want):
    """Bit for bit (int32 views of the floats), equal counts and order; a NaN only has to be a NaN."""
    assert got.frames.tolist() == want.frames.tolist()
    assert got.ids.tolist() == want.ids.tolist()
    assert got.labels.tolist() == want.labels.tolist()
    g, w = values_of(got), values_of(want)
    assert g.dtype == np.float32 and w.dtype == np.float32 and g.shape == w.shape
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan)
    assert np.array_equal(g.view(np.int32)[~nan], w.view(np.int32)[~nan])


def hole_threshold(sequences):
    """A result threshold that leaves a one-frame hole in some track of ``sequences`` (a list of ``Rows`` reported at a
    lower threshold): halfway between a score that is a strict minimum in time and the lower of its two neighbours, the
    widest such step there is.  (The result threshold only filters the report: the tracks live as before.)"""
    best = (0.0, None)
    for rows in sequences:
        for tid in np.unique(rows.ids):
            pick = np.flatnonzero(rows.ids == tid)
            f, s = rows.frames[pick], rows.scores[pick].astype(np.float64)
            for i in range(1, len(pick) - 1):
                if f[i - 1] + 1 == f[i] == f[i + 1] - 1 and s[i] < min(s[i - 1], s[i + 1]):
                    best = max(best, (min(s[i - 1], s[i + 1]) - s[i], 0.5 * (min(s[i - 1], s[i + 1]) + s[i])))
    assert best[1] is not None, "no track's score dips for a frame: choose other frames"
    return best[1]


def log_from_rows(rows, device, spare=0):
    """A ``ResultLog`` on ``device`` that holds ``rows`` in the given order (``spare``: unused rows behind them that the
    log counts as offered)."""
    m = len(rows.frames)
    log = ResultLog(device, capacity=m + spare)
    if m:
        log.rows_i[:m] = torch.from_numpy(np.stack((rows.frames, rows.ids, rows.labels), axis=1)).to(device)
        log.rows_f[:m] = torch.from_numpy(values_of(rows)).to(device)
    log.counters[0] = m
    log._bound = m + spare
    return log


def bank_log_from_rows(sequences, device, seed=0):
    """A ``BankResultLog`` holding ``{sequence: Rows}``, the frames of the sequences interleaved step by step and the
    rows of a step in a shuffled order (a bank writes slot order, not id order)."""
    parts_i, parts_f = [np.zeros((0, BANK_ROW_I), np.int64)], [np.zeros((0, ROW_F), np.float32)]
    for seq, rows in sequences.items():
        parts_i.append(np.stack((np.full_like(rows.frames, seq), rows.frames, rows.ids, rows.labels), axis=1))
        parts_f.append(values_of(rows))
    rows_i, rows_f = np.concatenate(parts_i), np.concatenate(parts_f)
    order = np.lexsort((np.random.RandomState(seed).permutation(len(rows_i)), rows_i[:, 1]))     # by frame, then mixed
    rows_i, rows_f = rows_i[order], rows_f[order]
    m = len(rows_i)
    log = BankResultLog(device, capacity=max(1, m))
    log.rows_i[:m], log.rows_f[:m] = torch.from_numpy(rows_i).to(device), torch.from_numpy(rows_f).to(device)
    log.counters[0] = m
    log._bound = m
    return log


# ---------------------------------------------------------------------------------------------- a scripted model
HIDDEN, N_DET = 256, 3                          # (256: the width RuntimeTracker gives a new track's unset fields)
REPORTED, MISSED, GONE = 3.0, -0.5, -9.0        # logits: sigmoid = 0.95 / 0.38 / 0.0001
SCRIPT_THRESHOLDS = dict(DET_SCORE_THRESH=0.9, TRACK_SCORE_THRESH=0.2, RESULT_SCORE_THRESH=0.5, MISS_TOLERANCE=5,
                         USE_MOTION=False)
# frames at which track i scores below RESULT_SCORE_THRESH (and above TRACK_SCORE_THRESH: it lives on)
SCRIPT_MISSED = {0: (2, 3), 1: (1,), 2: ()}
SCRIPT_SPURIOUS_FRAME = 2                       # detect query 0 fires once more here; that track is never seen again


class ScriptedModel(torch.nn.Module):
    """Stands in for the network in a ``SequenceTracker``: frame 0 gives birth to ``N_DET`` tracks that drift linearly;
    track i is ``MISSED`` at the frames ``SCRIPT_MISSED[i]`` and reported otherwise; at ``SCRIPT_SPURIOUS_FRAME`` one
    more track is born that scores ``GONE`` from then on.  The frame counter restarts whenever the tracker comes with
    no track (a new sequence)."""

    def __init__(self, device="cpu"):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=device))
        self.hidden_dim, self.num_classes = HIDDEN, 1
        self.frame_idx = 0

    def forward(self, frame=None, tracks=None, encoded=None, stage=None):
        if stage == "encode":
            return {}
        dev, t = self.anchor.device, tracks[0]
        if len(t) == 0:
            self.frame_idx = 0
        f = self.frame_idx
        self.frame_idx += 1
        ids = t.ids.tolist()
        rows = N_DET + len(ids)
        logits = torch.full((1, rows, 1), GONE)
        boxes = torch.full((1, rows, 4), 0.25)
        for k in range(N_DET):
            boxes[0, k] = torch.tensor([0.2 + 0.2 * k + 0.01 * f, 0.3 + 0.02 * f, 0.2, 0.3])
        if f == 0:
            logits[0, :N_DET] = REPORTED
        elif f == SCRIPT_SPURIOUS_FRAME:
            logits[0, 0] = REPORTED
            boxes[0, 0] = torch.tensor([0.8, 0.8, 0.1, 0.1])
        for row, tid in enumerate(ids, start=N_DET):
            if tid in SCRIPT_MISSED:
                logits[0, row] = MISSED if f in SCRIPT_MISSED[tid] else REPORTED
                boxes[0, row] = torch.tensor([0.2 + 0.2 * tid + 0.01 * f + 0.003 * (f % 3), 0.3 + 0.02 * f, 0.2, 0.3])
        return {"pred_logits": logits.to(dev), "pred_bboxes": boxes.to(dev), "last_ref_pts": boxes.clone().to(dev),
                "outputs": torch.zeros((1, rows, HIDDEN), device=dev),
                "det_query_embed": torch.zeros((N_DET, HIDDEN), device=dev),
                "aux_outputs": [{"queries": torch.zeros((1, rows, HIDDEN), device=dev)}]}

    def postprocess_single_frame(self, previous_tracks, new_tracks, unmatched_dets):
        from memotr_amd.structures.track_instances import TrackInstances
        active = TrackInstances.cat_tracked_instances(previous_tracks[0], new_tracks[0])
        return [active[active.ids >= 0]]
