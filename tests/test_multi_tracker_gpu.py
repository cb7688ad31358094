"""GPU: ``MultiSequenceTracker`` (memotr_amd/inference_multi.py) on the device with the 256-wide small model (the head
size of the hand-written attention kernels): the scenario of tests/test_multi_tracker_cpu.py -- three sequences of 2, 4
and 3 frames on two streams -- against three ``SequenceTracker`` runs, with the inference graphs on and off; a bank that
grows in the middle of a sequence; a stream refilled by a second sequence; ``track_many_logged`` + ``BankResultLog``
against ``track_many``; and one lockstep step under ``torch.cuda.set_sync_debug_mode("error")``."""
import pytest
import torch

import multi_track_cases as M

from memotr_amd.inference_multi import MultiSequenceTracker, _Step
from memotr_amd.results import BankResultLog

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenario(request):
    """The model on the device, the sequences and the three one-sequence runs (computed once, read by every test)."""
    for lib in ("hip_lib", "clip_lib"):
        request.getfixturevalue(lib)
    model, seqs = M.scenario_model(256).cuda(), M.sequences()
    want, margin = M.single_runs(model, seqs)
    return model, seqs, want, margin


def tracker_for(model, n_streams=2, cap=32, **options):
    return MultiSequenceTracker(model, n_streams=n_streams, cap=cap, **dict(M.OPTIONS, **options))


def test_the_scenario_decides_nothing_near_a_threshold(scenario):
    _, _, want, margin = scenario
    print("smallest decision margin of the one-sequence runs:", margin)
    assert margin > M.MARGIN, f"a decision score lies {margin} from its threshold: choose another seed"
    assert M.scenario_is_eventful(want)


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("n_streams", [2, 1])
def test_lockstep_streams_track_what_one_tracker_per_sequence_tracks(scenario, monkeypatch, n_streams, graphs):
    """Two streams: the second sequence outlives the first, whose stream is refilled by the third.  One stream: every
    sequence refills the stream of the one before it -- ids start again from 0 and nothing is carried over, or the rows
    would not be those of a fresh tracker."""
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "1" if graphs else "0")
    model, seqs, want, margin = scenario
    assert margin > M.MARGIN
    enc, dec = model.infer_graphs().encode, model.transformer.decoder.infer_graphs().decode
    replays = enc.replays, dec.replays
    tracker = tracker_for(model, n_streams)
    got = M.multi_runs(tracker, seqs)
    M.assert_equivalent(want, got)
    assert tracker.frame_counts == list(M.LENGTHS) and tracker.bank.n_streams == 1
    # with the graphs on, every step's encode half and decoder loop were replays (no quiet eager path)
    steps = {2: 5, 1: sum(M.LENGTHS)}[n_streams]
    assert not enc.failed and not dec.failed
    assert (enc.replays - replays[0], dec.replays - replays[1]) == ((steps, steps) if graphs else (0, 0))


def test_a_bank_grown_in_the_middle_of_a_sequence_loses_nothing(scenario):
    model, seqs, want, margin = scenario
    assert margin > M.MARGIN and max(len(r.ids) for seq in want for r in seq) > 16
    tracker = tracker_for(model, cap=16)
    M.assert_equivalent(want, M.multi_runs(tracker, seqs))
    assert tracker.bank.cap > 16
    tracker.bank.check()


def test_logged_tracking_gives_the_lines_of_track_many(scenario):
    model, seqs, _, _ = scenario
    tracker = tracker_for(model)
    got = M.multi_runs(tracker, seqs)
    log = BankResultLog("cuda", capacity=8)                  # (grows on the way)
    assert tracker_for(model).track_many_logged(seqs, log) == list(M.LENGTHS)
    for s, results in enumerate(got):
        lines = [line for idx, r in enumerate(results) for line in tracker.mot_lines(idx, r)]
        assert log.mot_lines(s) == lines and lines


def test_jpeg_sources_are_decoded_a_step_ahead_to_the_same_tracks(scenario):
    from memotr_amd.data import encode_jpeg
    from memotr_amd.inference import SequenceTracker
    model = scenario[0]
    # (frames of their own: the codec moves the scenario's scores, and these keep clear of the thresholds)
    streams = [[bytes(encode_jpeg(f, quality=90, subsampling="4:2:0")) for f in frames]
               for frames in M.sequences((2, 3), first=5)]
    want, margin = [], float("inf")
    for src in streams:
        t = SequenceTracker(model, **M.OPTIONS)
        d = M.Decisions(t, model.query_updater.update_threshold)
        want.append([r for _, r in t.track_jpeg(src)])
        margin = min(margin, d.margin())
    assert margin > M.MARGIN
    M.assert_equivalent(want, M.multi_runs(tracker_for(model), streams))


def test_steps_3_to_6_do_not_synchronise(scenario):
    """After a warm-up run (graphs captured, tables uploaded), decode, bank update, query update, the count copy and the
    result rows of one step run with torch's synchronisation check set to raise."""
    model, seqs, _, _ = scenario
    pair = [seqs[1], seqs[2]]
    log = BankResultLog("cuda", capacity=4096)
    tracker = tracker_for(model)
    tracker.track_many_logged(pair, log)                     # warm-up
    tracker.begin(2)
    seq_frame = torch.tensor([[0, 0], [1, 0]]).cuda()
    ori_wh = torch.tensor([[M.FRAME_W, M.FRAME_H]] * 2, dtype=torch.float32).cuda()
    for i in range(3):
        step = _Step([pair[0][i], pair[1][i]])
        enc = tracker._encoded(step, False)                  # steps 1-2
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            tracker._track(enc, None, False)                 # steps 3-5
            log.append(tracker.bank, seq_frame, ori_wh, tracker.result_score_thresh, tracker.area_thresh)       # step 6
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert int(tracker.bank.counters[:, 0].min()) > 0
    # ... and the mode does raise on this build: a read-back is refused
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            tracker.bank.counters.tolist()
    finally:
        torch.cuda.set_sync_debug_mode("default")
