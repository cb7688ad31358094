"""GPU: ``submit`` on the device (memotr_amd/submit.py) writes, for every sequence of the small DanceTrack tree, the
lines of a hand loop of ``track_jpeg`` + ``mot_lines`` with a fresh tracker -- device JPEG decode, inference graphs,
the result-row kernel and the one read per sequence together."""
import os

import pytest
import torch

import dataset_trees as T
from test_frames_gpu import build_memotr_cuda

from memotr_amd import submit as S
from memotr_amd.inference import SequenceTracker

pytestmark = pytest.mark.gpu

OPTIONS = dict(raw_size=(96, 160), area_thresh=0)


def test_submit_on_the_device_writes_the_lines_of_the_frame_loop(hip_lib, clip_lib, tmp_path, monkeypatch):
    import memotr_amd.modules.ms_deform_attn as mod
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    root = T.write_trees(str(tmp_path / "data"), only=("DanceTrack",))
    torch.manual_seed(4)
    model = build_memotr_cuda().eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, mod.MSDeformAttn):
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)
    config = dict(SUBMIT_DIR=str(tmp_path / "out"), SUBMIT_MODEL=None, SUBMIT_DATA_SPLIT="train", DATA_ROOT=root,
                  DET_SCORE_THRESH=0.0, TRACK_SCORE_THRESH=0.0, RESULT_SCORE_THRESH=0.0, MISS_TOLERANCE=5)
    files = S.submit(config, model=model, train_config=dict(DATASET="DanceTrack", USE_DAB=True), tracker_options=OPTIONS)
    assert [os.path.basename(f) for f in files] == [seq + ".txt" for seq in sorted(T.DANCE_SEQS)]
    for seq, path in zip(sorted(T.DANCE_SEQS), files):
        frames = S.sequence_frames("DanceTrack", os.path.join(root, "DanceTrack", "train", seq))
        t = SequenceTracker(model, dataset_name="DanceTrack", det_score_thresh=0.0, track_score_thresh=0.0,
                            result_score_thresh=0.0, miss_tolerance=5, use_dab=True, **OPTIONS)
        want = [line for idx, result in t.track_jpeg(frames) for line in t.mot_lines(idx, result)]
        with open(path) as f:
            assert f.read() == "".join(want) and len(want) >= 20 * T.DANCE_SEQS[seq]
