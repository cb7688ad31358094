"""CPU: the motion post-process (USE_MOTION) against the reference's own frame loop.

tests/golden/motion_*.npz hold two scripted scenarios run through the reference's ``Submitter.run`` with its
``RuntimeTracker(use_motion=True)`` (tests/golden/gen_golden_motion.py).  On CPU tensors ``MotionState`` runs its host
statement (memotr_amd/models/motion.py), which has to reproduce them bit for bit: every frame's ``ids``,
``disappear_time``, ``last_appear_boxes`` and the ``ref_pts`` the model is handed, and the MOT result lines.
"""
import pytest
import torch

from motion_helpers import SCENARIOS, ReplayModel, run_sequence_tracker, scenario

FIELDS = ("ids", "disappear_time", "last_appear_boxes", "ref_pts")


def assert_records_equal(sc, records):
    assert len(records) == sc["n_frames"]
    for f, (got, fr) in enumerate(zip(records, sc["frames"])):
        for k in FIELDS:
            want = fr["in_" + k]
            have = got[k].cpu().reshape(want.shape)
            assert have.dtype == want.dtype and torch.equal(have, want), (f, k, have, want)


@pytest.mark.parametrize("name", SCENARIOS)
def test_sequence_tracker_reproduces_the_reference(name):
    sc = scenario(name)
    tracker, model, text = run_sequence_tracker(sc)
    assert_records_equal(sc, model.records)
    assert text == sc["mot_lines"]
    tracker.tracker.motions.check()
    assert sum(bool((fr["in_disappear_time"] > 0).any()) for fr in sc["frames"]) >= 3      # (the scenario has misses)


@pytest.mark.parametrize("name", SCENARIOS)
def test_runtime_tracker_and_motion_state_reproduce_the_reference(name):
    """The same loop written out: RuntimeTracker.update, the stand-in updater, MotionState.extrapolate -- and the
    table's counts against the lengths of the reference's per-track histories."""
    from memotr_amd.models.runtime_tracker import RuntimeTracker
    from memotr_amd.structures.track_instances import TrackInstances
    sc = scenario(name)
    model = ReplayModel(sc)
    rt = RuntimeTracker(det_score_thresh=sc["thresh"], track_score_thresh=sc["thresh"],
                        miss_tolerance=sc["miss_tolerance"], use_motion=True, motion_min_length=sc["min_length"],
                        motion_max_length=sc["L"], use_dab=True)
    assert rt.use_motion and rt.motions is None
    tracks = [TrackInstances(hidden_dim=256, num_classes=sc["K"], use_dab=True)]
    for f in range(sc["n_frames"]):
        if f:
            counts = rt.motions.count[tracks[0].ids].long()
            assert torch.equal(counts, sc["frames"][f]["in_count"]), f
        res = model(tracks=tracks)
        previous, new = rt.update(model_outputs=res, tracks=tracks)
        tracks = model.postprocess_single_frame(previous, new, None)
        t = tracks[0]
        before = t.ref_pts
        kept = before.clone()
        t.ref_pts = rt.motions.extrapolate(t.ids, t.disappear_time, t.last_appear_boxes, t.ref_pts,
                                           sc["motion_lambda"])
        assert t.ref_pts is not before and torch.equal(before, kept)            # out of place
    assert_records_equal(sc, model.records)
    assert rt.max_obj_id == sum(int((fr["logits"][0, :sc["D"]].max(-1).values > 0).sum()) for fr in sc["frames"])


def test_growth_from_a_small_table_changes_nothing():
    sc = scenario("motion_a")
    from memotr_amd.models import motion
    made = []

    class Small(motion.MotionState):
        def __init__(self, max_length, min_length, device, capacity=4):
            super().__init__(max_length, min_length, device, capacity=4)
            made.append(self)

    orig, motion.MotionState = motion.MotionState, Small
    try:
        tracker, model, text = run_sequence_tracker(sc)
    finally:
        motion.MotionState = orig
    state = tracker.tracker.motions
    assert isinstance(state, Small) and state.capacity == 8 and tracker.tracker.max_obj_id == 5
    assert_records_equal(sc, model.records)
    assert text == sc["mot_lines"]
    big, _, _ = run_sequence_tracker(sc)
    ref = big.tracker.motions
    assert ref.capacity == 1024
    assert torch.equal(state.count[:5], ref.count[:5]) and torch.equal(state.boxes[:5], ref.boxes[:5])
    assert state.boxes.shape == (8, sc["L"], 4) and state.count.dtype == torch.int32


def test_from_config_honours_the_four_keys():
    from memotr_amd.configs import dancetrack_config
    from memotr_amd.inference import SequenceTracker
    cfg = dancetrack_config()
    assert (cfg["USE_MOTION"], cfg["MOTION_MIN_LENGTH"], cfg["MOTION_MAX_LENGTH"], cfg["MOTION_LAMBDA"]) == \
        (False, 3, 5, 0.5)
    sc = scenario("motion_a")
    off = SequenceTracker.from_config(ReplayModel(sc), cfg)
    assert off.use_motion is False and off.tracker.use_motion is False and off.tracker.motions is None
    on = SequenceTracker.from_config(ReplayModel(sc), dancetrack_config(USE_MOTION=True, MOTION_MIN_LENGTH=2,
                                                                          MOTION_MAX_LENGTH=7, MOTION_LAMBDA=0.25))
    assert on.use_motion is True and on.motion_lambda == 0.25
    assert (on.tracker.use_motion, on.tracker.motion_min_length, on.tracker.motion_max_length) == (True, 2, 7)
    bare = {k: v for k, v in cfg.items() if not k.startswith("MOTION_") and k != "USE_MOTION"}
    d = SequenceTracker.from_config(ReplayModel(sc), bare)
    assert (d.use_motion, d.motion_lambda, d.tracker.motion_min_length, d.tracker.motion_max_length) == \
        (False, 0.5, 3, 5)


def test_argument_errors():
    from memotr_amd.models.motion import MotionState
    from memotr_amd.models.runtime_tracker import RuntimeTracker
    with pytest.raises(ValueError, match="min_length"):
        MotionState(5, 1, "cpu")                    # the reference divides by count - 1
    with pytest.raises(ValueError, match="min_length"):
        MotionState(3, 4, "cpu")
    with pytest.raises(ValueError, match="max_length"):
        MotionState(17, 3, "cpu")
    MotionState(16, 16, "cpu"), MotionState(2, 2, "cpu")
    with pytest.raises(ValueError, match="min_length"):
        RuntimeTracker(use_motion=True, motion_min_length=1)
    RuntimeTracker(use_motion=False, motion_min_length=1)        # not looked at when the switch is off
    s = MotionState(5, 3, "cpu", capacity=4)
    with pytest.raises(TypeError, match="float32"):
        s.register(0, torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(TypeError, match="int64"):
        s.extrapolate(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.long), torch.zeros(2, 4),
                      torch.zeros(2, 4), 0.5)


def test_rows_outside_the_table_are_skipped_and_reported():
    from memotr_amd.models.motion import MotionState
    s = MotionState(5, 3, "cpu", capacity=4)
    s.register(0, torch.full((3, 4), 0.25))
    table = (s.boxes.clone(), s.count.clone())
    ids = torch.tensor([-1, 9, 1])
    scores = torch.tensor([[0.9], [0.1], [0.9]])
    boxes, lab = torch.full((3, 4), 0.5), torch.full((3, 4), 0.125)
    new_ids, dt, new_lab = s.observe(scores, torch.zeros(3, dtype=torch.long), boxes, ids, torch.tensor([2, 3, 0]), lab,
                                     0.5, 4)
    assert new_ids.tolist() == [-1, 9, 1] and dt.tolist() == [0, 4, 0]      # (id 9 is past its tolerance: kept)
    assert torch.equal(new_lab, torch.tensor([[0.125] * 4, [0.125] * 4, [0.5] * 4]))
    assert s.count.tolist() == [1, 2, 1, 0] and torch.equal(s.boxes[0], table[0][0])
    with pytest.raises(RuntimeError, match="negative track id.*past the table"):
        s.check()


def test_motion_off_never_builds_a_state():
    sc = scenario("motion_a")
    tracker, model, _ = run_sequence_tracker(sc, use_motion=False)
    assert tracker.tracker.motions is None and tracker.use_motion is False
    for rec in model.records:
        assert rec["last_appear_boxes"].shape[0] == 0           # nothing writes the field on today's path
    # the same decisions either way: motion only moves ref_pts
    for rec, fr in zip(model.records, sc["frames"]):
        assert torch.equal(rec["ids"], fr["in_ids"]) and torch.equal(rec["disappear_time"], fr["in_disappear_time"])
