"""Shared by the motion tests: the golden scenarios (tests/golden/motion_*.npz, written by
tests/golden/gen_golden_motion.py from the reference's own frame loop) and the stand-in model that replays them."""
import torch

from conftest import load_golden

HIDDEN = 256
SCENARIOS = ("motion_a", "motion_b")
_CACHE = {}


def scenario(name):
    """The fixture as torch tensors (loaded once, never modified) plus its scalars."""
    if name not in _CACHE:
        z = load_golden(name)
        K, D, L, min_length, miss_tolerance, n_frames, ori_h, ori_w = (int(v) for v in z["meta"])
        thresh, lam = (float(v) for v in z["thresh_lambda"])
        frames = [{k: torch.from_numpy(z[f"f{f}_{k}"]) for k in
                   ("logits", "boxes", "last_ref_pts", "in_ids", "in_ref_pts", "in_disappear_time",
                    "in_last_appear_boxes", "in_count")} for f in range(n_frames)]
        _CACHE[name] = dict(K=K, D=D, L=L, min_length=min_length, miss_tolerance=miss_tolerance, n_frames=n_frames,
                            ori_h=ori_h, ori_w=ori_w, thresh=thresh, motion_lambda=lam, frames=frames,
                            mot_lines=bytes(z["mot_lines"]).decode())
    return _CACHE[name]


class ReplayModel(torch.nn.Module):
    """The generator's stand-in model: ``forward`` hands out the scripted outputs of the next frame (everything the
    fixture does not store is zeros) and records the track state it is handed; ``postprocess_single_frame`` is the
    query updater without its embedding update.  Takes both call forms: the reference's ``(frame, tracks)`` and
    ``SequenceTracker``'s encode / decode halves."""

    def __init__(self, sc, device="cpu"):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=device))
        self.hidden_dim, self.num_classes = HIDDEN, sc["K"]
        self.sc, self.frame_idx, self.records = sc, 0, []

    def forward(self, frame=None, tracks=None, encoded=None, stage=None):
        if stage == "encode":
            return {}
        sc, dev, t = self.sc, self.anchor.device, tracks[0]
        fr = sc["frames"][self.frame_idx]
        self.frame_idx += 1
        self.records.append({k: getattr(t, k) for k in ("ids", "ref_pts", "disappear_time", "last_appear_boxes")})
        rows = fr["logits"].shape[1]
        assert rows == sc["D"] + len(t), "the run has left the scripted scenario"
        return {"pred_logits": fr["logits"].to(dev), "pred_bboxes": fr["boxes"].to(dev),
                "last_ref_pts": fr["last_ref_pts"].to(dev), "outputs": torch.zeros((1, rows, HIDDEN), device=dev),
                "det_query_embed": torch.zeros((sc["D"], HIDDEN), device=dev),
                "aux_outputs": [{"queries": torch.zeros((1, rows, HIDDEN), device=dev)}]}

    def postprocess_single_frame(self, previous_tracks, new_tracks, unmatched_dets):
        from memotr_amd.structures.track_instances import TrackInstances
        active = TrackInstances.cat_tracked_instances(previous_tracks[0], new_tracks[0])
        return [active[active.ids >= 0]]


def run_sequence_tracker(sc, device="cpu", **overrides):
    """The scenario through ``SequenceTracker(use_motion=True)``: (tracker, model with its records, MOT text)."""
    from memotr_amd.inference import SequenceTracker
    model = ReplayModel(sc, device)
    kw = dict(dataset_name="DanceTrack", det_score_thresh=sc["thresh"], track_score_thresh=sc["thresh"],
              result_score_thresh=sc["thresh"], miss_tolerance=sc["miss_tolerance"], use_dab=True, use_motion=True,
              motion_lambda=sc["motion_lambda"], motion_min_length=sc["min_length"], motion_max_length=sc["L"])
    kw.update(overrides)
    tracker = SequenceTracker(model, **kw)
    image = torch.zeros((3, 32, 32))
    text = ""
    for f in range(sc["n_frames"]):
        result = tracker.step(image, sc["ori_h"], sc["ori_w"])
        text += "".join(tracker.mot_lines(f, result))
    return tracker, model, text
