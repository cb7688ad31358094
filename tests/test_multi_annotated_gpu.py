"""GPU: annotated output without a host result, on the device: the checks of tests/test_multi_annotated_cpu.py with the
draw-table kernel, the overlay kernel and the batched JPEG device stage in place of the host statements -- the files are
still the host statements' bytes -- and the added work of a step (the table launch and ``add_step``) under
``torch.cuda.set_sync_debug_mode("error")``."""
import pytest
import torch

import multi_annotated_cases as A
import multi_track_cases as M

from memotr_amd import render as R
from memotr_amd.functions import clip_ops
from memotr_amd.inference import SequenceTracker
from memotr_amd.inference_multi import _Step
from memotr_amd.results import BankResultLog, ResultLog

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(request):
    for lib in ("hip_lib", "clip_lib"):
        request.getfixturevalue(lib)
    return M.scenario_model(256).cuda()


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
def test_the_logged_loop_writes_the_host_statements_files_of_the_logged_rows(model, subsampling):
    A.check_logged(model, "cuda", subsampling)


def test_the_generator_writes_the_files_of_the_results_it_yields(model):
    A.check_generator(model, "cuda")


def test_one_sequence_logged_writes_the_files_of_track_annotated(model, tmp_path):
    A.check_single(model, "cuda", tmp_path)


def test_submit_writes_one_annotated_file_per_frame_and_the_same_results(model, tmp_path):
    thresholds = dict(DET_SCORE_THRESH=0.7, TRACK_SCORE_THRESH=0.45, RESULT_SCORE_THRESH=0.6, MISS_TOLERANCE=2,
                      USE_MOTION=False)
    A.check_submit(model, tmp_path, thresholds, dict(raw_size=M.RAW_SIZE, area_thresh=10))


def test_the_table_and_add_step_read_nothing_from_the_device(model):
    """After a warm-up run (graphs captured, the writer's buffers made), steps 3-6 of the lockstep loop with the table
    launch and ``add_step`` behind them run with torch's synchronisation check set to raise; so do the table launch and
    ``add_step`` of the one-sequence loop (its tracker's own bookkeeping reads the device: that is ``track_logged``'s)."""
    seqs = M.sequences()
    pair = [seqs[1], seqs[2]]
    sink, log = A.Files(), BankResultLog("cuda", capacity=4096)
    tracker = A.tracker_for(model)
    writer = R.MultiAnnotatedWriter(sink, quality=A.QUALITY, **A.DRAW)
    tracker.track_many_annotated_logged(pair, writer, log)                # warm-up
    tracker.begin(2)
    seq_frame = torch.tensor([[0, 0], [1, 0]]).cuda()
    ori_wh = torch.tensor([[M.FRAME_W, M.FRAME_H]] * 2, dtype=torch.float32).cuda()
    for i in range(3):
        step = _Step([pair[0][i], pair[1][i]])
        enc = tracker._encoded(step, False)                      # steps 1-2
        tracker._done_step = step
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            tracker._track(enc, None, False)                     # steps 3-5
            log.append(tracker.bank, seq_frame, ori_wh, tracker.result_score_thresh, tracker.area_thresh)       # step 6
            tracker._annotate(writer, [(7, i), (8, i)], ori_wh, False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # one sequence: the table from the tracks and the step behind it
    single = SequenceTracker(model, **M.OPTIONS)
    frames = [f.cuda() for f in seqs[1]]
    assert single.track_annotated_logged(frames[:2], writer, ResultLog("cuda"), sequence=9) == 2
    t = single.tracks[0]
    assert len(t) > 0
    one_wh = ori_wh[:1].contiguous()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        table = clip_ops.draw_table(t.boxes[None], t.scores[None], t.ids[None], one_wh, single.result_score_thresh,
                                    single.area_thresh, font_scale=writer.font_scale)
        writer.add_step([(9, 2)], [frames[2]], table)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    writer.close()
    # the warm-up's 4 + 3 files, three steps of two streams, two frames of the one sequence and the one step behind them
    assert len(sink.files) == (4 + 3) + 6 + 2 + 1 and {(7, 2), (8, 0), (9, 2)} <= set(sink.files)
    assert int(tracker.bank.counters[:, 0].min()) > 0
