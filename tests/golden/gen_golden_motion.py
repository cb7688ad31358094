"""Golden generator for the motion post-process (USE_MOTION).  Run from the repo root, with the reference checked out:

    python tests/golden/gen_golden_motion.py

The reference's own frame loop (``Submitter.run``, submit_engine.py:58-120) runs on the CPU with its own
``RuntimeTracker(use_motion=True)`` and ``Motion``, around a scripted stand-in model: ``forward`` hands out pre-drawn
logits / boxes / reference points and records the track state it is handed (``ids``, ``ref_pts``, ``disappear_time``,
``last_appear_boxes`` -- what the motion code produced for the previous frame), ``postprocess_single_frame`` is
``cat_tracked_instances`` followed by ``ids >= 0`` (the query updater without its embedding update).  The LOGITS ARE
SCRIPTED per track id, so that the scenario holds each case the motion code distinguishes; the generator asserts
them.  Hidden size 256 (the reference's newborn ``TrackInstances`` defaults to it).

Only data is written (tests/golden/motion_*.npz): the scripted per-frame model outputs that are not zeros, the
recorded per-frame state and the MOT result lines.  No reference source is copied.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from gen_golden_model import install_stubs, save_npz  # noqa: E402

HI, LO, AT = 3.0, -3.0, 0.0       # a track's own logit: seen, missed, and sigmoid(0) = 0.5 = the threshold exactly
THRESH = 0.5
HIDDEN = 256
ORI_H, ORI_W = 480, 640

# One scenario: per frame, the detect slots that fire (a newborn per firing slot, ids in slot order) and, per live
# track id, the logit of the track's own class (default HI).  Frame count = len(det).
SCENARIOS = {
    # K = 1, L = 5, min_length = 3, miss_tolerance = 4
    #   id 0: seen f1-f2 (count 3 = min_length), missed f3 and f4 (disappear_time 1, then 2: extrapolated twice),
    #         back at f5 (history cleared), seen f6-f7 (rebuilt to 3), missed f8 (extrapolated again)
    #   id 1: seen f1-f7 (trimmed to 5 from f5 on), missed f8 (count = max_length), back at f9 exactly AT the threshold
    #   id 2: missed from f1 (count 1 < min_length: ref_pts unchanged), retired at f4 (disappear_time 4)
    #   id 3: exactly AT the threshold at f1 (seen: the comparison is strict)
    #   id 4: born at f5, seen f6, missed f7 (count 2 < min_length)
    "a": dict(K=1, D=5, L=5, min_length=3, miss_tolerance=4, motion_lambda=0.5,
              det=[[0, 1, 2, 3], [], [], [], [], [4], [], [], [], [], []],
              track={0: {3: LO, 4: LO, 8: LO}, 1: {8: LO, 9: AT}, 2: {1: LO, 2: LO, 3: LO, 4: LO},
                     3: {1: AT}, 4: {7: LO}}),
    # K = 8, L = 2, min_length = 2: every seen pair of frames qualifies, every push past the second trims
    "b": dict(K=8, D=4, L=2, min_length=2, miss_tolerance=4, motion_lambda=0.25,
              det=[[1, 3], [0], [], [], [], [], [2], [], [], []],
              track={0: {2: LO, 3: LO, 6: LO}, 1: {1: LO, 2: LO, 3: LO, 4: LO}, 2: {3: AT, 4: LO, 5: LO, 6: LO},
                     3: {8: LO}}),
}


def install_motion_stubs():
    install_stubs()
    log = types.ModuleType("log")
    logger = types.ModuleType("log.logger")
    logger.Logger = type("Logger", (), {})
    data = types.ModuleType("data")
    seq = types.ModuleType("data.seq_dataset")
    seq.SeqDataset = type("SeqDataset", (), {})
    log.logger, data.seq_dataset = logger, seq
    for name, mod in (("log", log), ("log.logger", logger), ("data", data), ("data.seq_dataset", seq)):
        sys.modules[name] = mod


class ScriptedModel(torch.nn.Module):
    def __init__(self, sc, seed):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.hidden_dim, self.num_classes = HIDDEN, sc["K"]
        self.sc, self.g = sc, torch.Generator().manual_seed(seed)
        self.frame_idx = 0
        self.tracker = None           # the reference RuntimeTracker: its motions' lengths are recorded as `count`
        self.frames, self.records = [], []

    def forward(self, frame, tracks):
        sc, f, t = self.sc, self.frame_idx, tracks[0]
        D, K, n = sc["D"], sc["K"], len(t)
        ids = t.ids.tolist()
        self.records.append(dict(
            ids=t.ids.clone(), ref_pts=t.ref_pts.clone(), disappear_time=t.disappear_time.clone(),
            last_appear_boxes=t.last_appear_boxes.clone().reshape(-1, 4),
            count=torch.as_tensor([len(self.tracker.motions[i]) for i in ids], dtype=torch.long)))
        logits = torch.full((1, D + n, K), -6.0)
        for slot in sc["det"][f]:
            cls = (slot * 3 + f) % K
            logits[0, slot, cls] = HI
        for row, tid in enumerate(ids):
            logits[0, D + row, t.labels[row]] = sc["track"].get(tid, {}).get(f, HI)
        # boxes: centres in (0.2, 0.8), sizes in (0.08, 0.3) -- inside the frame, area well above the 100 px filter
        r = torch.rand((1, D + n, 4), generator=self.g)
        boxes = torch.cat((0.2 + 0.6 * r[..., :2], 0.08 + 0.22 * r[..., 2:]), dim=-1)
        last_ref_pts = torch.randn((1, D + n, 4), generator=self.g)
        self.frames.append(dict(logits=logits.clone(), boxes=boxes.clone(), last_ref_pts=last_ref_pts.clone()))
        self.frame_idx += 1
        return {"pred_logits": logits, "pred_bboxes": boxes, "last_ref_pts": last_ref_pts,
                "outputs": torch.zeros((1, D + n, HIDDEN)), "det_query_embed": torch.zeros((D, HIDDEN)),
                "aux_outputs": [{"queries": torch.zeros((1, D + n, HIDDEN))}]}

    def postprocess_single_frame(self, previous_tracks, new_tracks, unmatched_dets):
        from structures.track_instances import TrackInstances
        active = TrackInstances.cat_tracked_instances(previous_tracks[0], new_tracks[0])
        return [active[active.ids >= 0]]


def run_scenario(name, sc, seed):
    from models.runtime_tracker import RuntimeTracker
    from submit_engine import Submitter
    n_frames = len(sc["det"])
    model = ScriptedModel(sc, seed).eval()
    sub = Submitter.__new__(Submitter)
    sub.dataset_name, sub.seq_name, sub.model = "DanceTrack", "seq", model
    sub.tracker = RuntimeTracker(det_score_thresh=THRESH, track_score_thresh=THRESH,
                                 miss_tolerance=sc["miss_tolerance"], use_motion=True,
                                 motion_min_length=sc["min_length"], motion_max_length=sc["L"], use_dab=True)
    model.tracker = sub.tracker
    sub.result_score_thresh, sub.motion_lambda = THRESH, sc["motion_lambda"]
    sub.device, sub.use_dab, sub.use_motion, sub.visualize = torch.device("cpu"), True, True, False
    image, ori = torch.zeros((1, 3, 32, 32)), torch.zeros((1, ORI_H, ORI_W, 3))
    sub.dataloader = [((image, ori), ["frame.jpg"])] * n_frames
    with tempfile.TemporaryDirectory() as tmp:
        sub.outputs_dir, sub.predict_dir = tmp, tmp
        sub.run()
        with open(os.path.join(tmp, "seq.txt")) as fh:
            mot_lines = fh.read()

    rec, L, m = model.records, sc["L"], sc["min_length"]
    # ---- the seven cases, from what the reference recorded (record f + 1 is the state frame f left behind)
    changed = []                      # (frame, id, disappear_time, count, pushes) of every row the motion code moved
    pushes = {}                       # id -> boxes pushed since the history was last empty
    seen = dict(small=False, cleared=False, rebuilt=False, retired=False, at_thresh=False)
    for f in range(n_frames - 1):
        before, after = rec[f], rec[f + 1]
        prev = {int(i): k for k, i in enumerate(before["ids"])}
        if set(prev) - set(after["ids"].tolist()):
            seen["retired"] = True
        own = {tid: sc["track"].get(tid, {}).get(f, HI) for tid in prev}
        for k, tid in enumerate(after["ids"].tolist()):
            dt, cnt = int(after["disappear_time"][k]), int(after["count"][k])
            if tid not in prev:
                pushes[tid] = 1
                continue
            if dt == 0:
                pushes[tid] = 1 if int(before["disappear_time"][prev[tid]]) > 0 else pushes[tid] + 1
            assert cnt == min(pushes[tid], L), (name, f, tid, cnt, pushes[tid])
            if own[tid] == AT:
                assert dt == 0, "a score exactly at the threshold counts as seen"
                seen["at_thresh"] = True
            moved = not torch.equal(after["ref_pts"][k], before["ref_pts"][prev[tid]])
            assert moved == (dt > 0 and cnt >= m), (name, f, tid, dt, cnt)
            if moved:
                changed.append((f, tid, dt, cnt, pushes[tid]))
            if dt > 0 and cnt < m:
                seen["small"] = True
            if dt == 0 and int(before["disappear_time"][prev[tid]]) > 0:
                assert cnt == 1
                seen["cleared"] = True
    assert any(cnt == m for _, _, _, cnt, _ in changed), "extrapolated with count == min_length"
    assert any(cnt == L and pushed > L for _, _, _, cnt, pushed in changed), "extrapolated with a trimmed full history"
    assert any((f + 1, tid, 2) in {c[:3] for c in changed} for f, tid, dt, _, _ in changed if dt == 1), \
        "extrapolated over two consecutive missed frames"
    cleared_ids = set()
    for f in range(n_frames - 1):
        prev = {int(i): k for k, i in enumerate(rec[f]["ids"])}
        for k, tid in enumerate(rec[f + 1]["ids"].tolist()):
            if tid in prev and int(rec[f + 1]["disappear_time"][k]) == 0 and int(rec[f]["disappear_time"][prev[tid]]) > 0:
                cleared_ids.add((tid, f))
    seen["rebuilt"] = any(tid == c and f > cf for f, tid, _, _, _ in changed for c, cf in cleared_ids)
    assert all(seen.values()), (name, seen)

    arrays = {"meta": np.asarray([sc["K"], sc["D"], sc["L"], sc["min_length"], sc["miss_tolerance"], n_frames,
                                  ORI_H, ORI_W], dtype=np.int64),
              "thresh_lambda": np.asarray([THRESH, sc["motion_lambda"]], dtype=np.float64),
              "mot_lines": np.frombuffer(mot_lines.encode(), dtype=np.uint8).copy()}
    for f in range(n_frames):
        for k, v in model.frames[f].items():
            arrays[f"f{f}_{k}"] = v.numpy()
        for k, v in rec[f].items():
            arrays[f"f{f}_in_{k}"] = v.numpy()
    save_npz(os.path.join(OUT, f"motion_{name}.npz"), **arrays)
    print(f"motion_{name}: {n_frames} frames, {len(changed)} extrapolated rows, "
          f"{mot_lines.count(chr(10))} result lines, cases {seen}")


def main():
    install_motion_stubs()
    torch.manual_seed(0)
    for seed, (name, sc) in enumerate(sorted(SCENARIOS.items())):
        with torch.no_grad():
            run_scenario(name, sc, 100 + seed)


if __name__ == "__main__":
    main()
