"""GPU: the command-line entry's chain on the device (memotr_amd/main.py).  One epoch on the small DanceTrack tree with
captured graphs required, then ``submit`` and ``evaluate`` on the directory the run left, no file written by hand; and
the component values that the run log takes from the device against ``get_mean_by_n_gts(with_log=True)`` on the same
clips.

The model is ``test_frames_gpu.build_memotr_cuda`` (stand-in backbone, 256 channels, 2 + 2 layers); frames are 48 x 80
JPEG files, trained at 96 x 160 and tracked at 96 x 160; clips have 2 frames, the epoch 10 clips."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

import clip_loader_helpers as H
import dataset_trees as T
from test_frames_gpu import build_memotr_cuda
from test_main_cpu import base_config

from memotr_amd import main as M
from memotr_amd.configs import load_yaml

pytestmark = pytest.mark.gpu

OPTIONS = dict(raw_size=(96, 160), area_thresh=0)
PLAN = dataclasses.replace(H.PLAIN, final=(96, 160))


def new_model(seed):
    import memotr_amd.modules.ms_deform_attn as mod
    torch.manual_seed(seed)
    model = build_memotr_cuda()
    with torch.no_grad():               # the zero-initialised sampling heads would make every query look at one point
        for m in model.modules():
            if isinstance(m, mod.MSDeformAttn):
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)
    return model


@pytest.fixture(scope="module")
def run(tmp_path_factory, hip_lib, clip_lib):
    """The training run, once: {"root", "out", "config", "model", "events", "logged", "wanted"}.  ``logged`` is every
    (name, value) the run log's window received, in order; ``wanted`` the ``with_log=True`` dict of each clip, taken
    inside the step, i.e. on the same device values."""
    from memotr_amd import build, runlog
    from memotr_amd.models.criterion import ClipCriterion
    for name in ("frame", "jpeg", "jpeg_enc", "augment", "static_clip", "opt", "track_eval"):
        build.build(name)
    tmp = tmp_path_factory.mktemp("main_gpu")
    root = T.write_trees(str(tmp / "data"), only=("DanceTrack",))
    with open(os.path.join(root, "DanceTrack", "train_seqmap.txt"), "w") as f:
        f.write("name\n" + "".join(seq + "\n" for seq in sorted(T.DANCE_SEQS)))
    out = str(tmp / "run")
    config = base_config(DATA_ROOT=root, OUTPUTS_DIR=out, SEED=11, DEVICE="cuda", HIDDEN_DIM=256, FFN_DIM=256)
    model = new_model(4)
    events, logged, wanted = [], [], []
    update, reduce = runlog.MetricWindow.update, ClipCriterion.get_mean_by_n_gts

    def spy_update(self, name, value):
        logged.append((name, value))
        update(self, name, value)

    def spy_reduce(self, with_log=True):
        loss, log = reduce(self, with_log=True)         # reads the components: the values are the ones the step uses
        wanted.append(log)
        return loss, log

    tf32 = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    rng = torch.get_rng_state()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
        mp.setenv("PYTHONHASHSEED", "0")
        mp.setattr(runlog.MetricWindow, "update", spy_update)
        mp.setattr(ClipCriterion, "get_mean_by_n_gts", spy_reduce)
        trained, _, _, states = M.run(config, model=model, dataset=H.dance_dataset(root, plans=[PLAN]), log_every=4,
                                      on_log=events.append)
    torch.cuda.synchronize()
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = tf32
    torch.set_rng_state(rng)
    assert trained is model and states == {"start_epoch": 1, "global_iters": 10}
    return dict(root=root, out=out, config=config, model=model, events=events, logged=logged, wanted=wanted)


def test_the_run_leaves_config_log_scalars_and_a_checkpoint(run):
    out = run["out"]
    assert load_yaml(os.path.join(out, "train", "config.yaml")) == run["config"]
    with open(os.path.join(out, "train", "log.txt")) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("[Epoch 0] lr=[{'lr_backbone': 2e-05}")
    assert [line.split("]")[0] for line in lines[1:-1]] == [f"[Epoch=0, Iter={i}/10" for i in (0, 4, 8)]
    assert lines[-1].startswith("[Epoch: 0, Total Time: 0min] loss = ")
    for line in lines[1:]:
        assert all(f"frame{i}_{k} = " in line for i in (0, 1) for k in ("box_l1_loss", "box_giou_loss",
                                                                        "label_focal_loss"))
    with open(os.path.join(out, "train", "scalars.jsonl")) as f:
        scalars = [json.loads(line) for line in f]
    assert all(math.isfinite(s["value"]) for s in scalars) and len(scalars) == 1 + 4 * 7
    ckpt = torch.load(os.path.join(out, "checkpoint_0.pth"), map_location="cpu")
    assert ckpt["states"] == {"start_epoch": 1, "global_iters": 10}
    assert all(torch.isfinite(v).all() for v in ckpt["model"].values() if v.is_floating_point())


def test_the_logged_components_are_the_with_log_values_of_the_same_clips(run):
    """Both sides divide the SAME float32 device value by the same integer count: ``log_components`` on the device in
    float32, ``get_mean_by_n_gts(with_log=True)`` on the host in float64.  The float64 quotient rounded to float32 is
    within half a float32 ulp of the exact quotient and the device's quotient within one (a correctly rounded division
    gives the same number; a reciprocal-based one may differ in the last bit): the bound is one float32 ulp."""
    logged, wanted = run["logged"], run["wanted"]
    assert len(wanted) == 10
    names = [f"frame{i}_{k}" for i in (0, 1) for k in ("box_l1_loss", "box_giou_loss", "label_focal_loss")]
    per_clip = ["total_loss"] + names + ["time per iter"]
    assert [n for n, _ in logged] == per_clip * 10
    for clip, want in enumerate(wanted):
        assert list(want) == names
        got = dict(logged[clip * len(per_clip):(clip + 1) * len(per_clip)])
        for name in names:
            value, count = want[name]
            assert count == 1 and value > 0
            ulp = float(np.spacing(np.float32(value)))
            print(f"clip {clip} {name}: logged {got[name]!r} with_log {value!r} diff/ulp {(got[name] - value) / ulp:+.3f}")
            assert abs(got[name] - value) <= ulp, (clip, name)
    # the total loss is the very tensor the step returned: what on_log averaged
    totals = [v for n, v in logged if n == "total_loss"]
    assert run["events"][0]["loss"] == totals[0]
    assert run["events"][-1]["loss"] == pytest.approx(sum(totals) / 10, rel=1e-12)


def test_submit_and_evaluate_run_on_what_the_training_left(run, monkeypatch):
    from memotr_amd import submit as S
    from memotr_amd.inference import SequenceTracker
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    monkeypatch.setenv("PYTHONHASHSEED", "0")
    root, out, config = run["root"], run["out"], run["config"]
    model = new_model(5).eval()
    model.load_state_dict(torch.load(os.path.join(out, "checkpoint_0.pth"), map_location="cpu")["model"])
    files = M.run(dict(config, MODE="submit", SUBMIT_DIR=out, SUBMIT_MODEL="checkpoint_0.pth",
                       SUBMIT_DATA_SPLIT="train"), model=model, tracker_options=OPTIONS)
    assert [os.path.basename(f) for f in files] == [seq + ".txt" for seq in sorted(T.DANCE_SEQS)]
    for seq, path in zip(sorted(T.DANCE_SEQS), files):
        frames = S.sequence_frames("DanceTrack", os.path.join(root, "DanceTrack", "train", seq))
        t = SequenceTracker(model, dataset_name="DanceTrack", det_score_thresh=0.0, track_score_thresh=0.0,
                            result_score_thresh=0.0, miss_tolerance=5, use_dab=True, **OPTIONS)
        want = [line for idx, result in t.track_jpeg(frames) for line in t.mot_lines(idx, result)]
        with open(path) as f:
            assert f.read() == "".join(want) and len(want) >= 20 * T.DANCE_SEQS[seq]
    metrics = M.run(dict(config, MODE="eval", EVAL_DIR=out, EVAL_MODE="specific", EVAL_MODEL="checkpoint_0.pth",
                         EVAL_DATA_SPLIT="train"), model=new_model(6).eval(), tracker_options=OPTIONS)
    with open(os.path.join(out, "train", "metrics.jsonl")) as f:
        (line,) = [json.loads(x) for x in f]
    assert line["checkpoint"] == "checkpoint_0.pth" and line["metrics"] == metrics
    assert all(math.isfinite(metrics[k]) for k in ("HOTA", "MOTA", "IDF1"))
