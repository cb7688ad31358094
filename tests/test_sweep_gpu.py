"""GPU: ``SweepTracker`` (memotr_amd/inference_sweep.py) on the device with the 256-wide small model: every sequence of
the scenario under the four settings of tests/sweep_cases.py in one pass against a fresh ``SequenceTracker`` per setting,
with the inference graphs on and off; one setting against ``MultiSequenceTracker(n_streams=1)``, bit for bit (the same
kernels at B = 1); a bank that grows in the middle of a sequence; ``track_logged`` + ``BankResultLog`` against ``track``;
and one step under ``torch.cuda.set_sync_debug_mode("error")``."""
import pytest
import torch

import multi_track_cases as M
import sweep_cases as C

from memotr_amd.inference_multi import MultiSequenceTracker, _Step
from memotr_amd.inference_sweep import SweepTracker
from memotr_amd.results import BankResultLog

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenario(request):
    """The model on the device, the sequences and every setting's one-sequence runs (computed once, read by every test)."""
    for lib in ("hip_lib", "clip_lib"):
        request.getfixturevalue(lib)
    model, seqs = M.scenario_model(256).cuda(), M.sequences()
    want, margin = C.single_runs(model, seqs)
    return model, seqs, want, margin


def tracker_for(model, settings=C.SETTINGS, cap=32, **options):
    return SweepTracker(model, settings, cap=cap, **dict(C.OPTIONS, **options))


def test_the_scenario_decides_nothing_near_a_threshold(scenario):
    _, _, want, margin = scenario
    print("smallest decision margin of the one-sequence runs:", margin)
    assert margin > M.MARGIN, f"a decision score lies {margin} from its threshold: choose other settings"
    assert all(M.scenario_is_eventful(runs) for runs in want)
    assert C.some_frame_differs(want)


@pytest.mark.parametrize("graphs", [True, False])
def test_every_stream_tracks_what_a_tracker_with_its_setting_tracks(scenario, monkeypatch, graphs):
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "1" if graphs else "0")
    model, seqs, want, margin = scenario
    assert margin > M.MARGIN
    enc, dec = model.infer_graphs().encode, model.transformer.decoder.infer_graphs().decode
    replays = enc.replays, dec.replays
    got = C.sweep_runs(tracker_for(model), seqs)
    for k in range(len(C.SETTINGS)):
        M.assert_equivalent(want[k], got[k])
    assert C.some_frame_differs(got)                         # not every stream under setting 0
    # with the graphs on, every frame's encode half (B = 1) and every step's decoder loop (B = S) were replays
    steps = sum(M.LENGTHS)
    assert not enc.failed and not dec.failed
    assert (enc.replays - replays[0], dec.replays - replays[1]) == ((steps, steps) if graphs else (0, 0))


def test_one_setting_is_the_one_stream_bank_bit_for_bit(scenario):
    model, seqs, _, _ = scenario
    got = C.sweep_runs(tracker_for(model, C.SETTINGS[:1]), seqs)[0]
    multi = MultiSequenceTracker(model, n_streams=1, cap=32, **dict(C.OPTIONS, **C.SETTINGS[0]))
    for frames, runs in zip(seqs, got):
        want = M.multi_runs(multi, [frames])[0]
        assert len(want) == len(runs)
        for a, b in zip(want, runs):
            assert len(a.ids) > 0
            assert torch.equal(a.ids, b.ids) and torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores)
            assert torch.equal(a.labels, b.labels)


def test_a_bank_grown_in_the_middle_of_a_sequence_loses_nothing(scenario):
    """Settings A, F and E, as tests/test_multi_tracker_gpu.py grows its bank under A.  (D, with births from 0.6 on, fills
    sixteen slots before the live counts -- looked at one step late -- can grow the bank: that is the overflow
    ``check`` reports at the end of a sequence, tests/test_sweep_cpu.py, not growth.)"""
    model, seqs, want, margin = scenario
    assert margin > M.MARGIN
    picked = [0, 2, 3]
    busiest = max(range(len(seqs)), key=lambda s: max(len(r.ids) for k in picked for r in want[k][s]))
    assert max(len(r.ids) for k in picked for r in want[k][busiest]) > 16
    tracker = tracker_for(model, [C.SETTINGS[k] for k in picked], cap=16)
    got = C.sweep_runs(tracker, [seqs[busiest]])
    for i, k in enumerate(picked):
        M.assert_equivalent([want[k][busiest]], got[i])
    assert tracker.bank.cap > 16


def test_logged_tracking_gives_the_lines_of_track(scenario):
    model, seqs, _, _ = scenario
    tracker = tracker_for(model)
    log = BankResultLog("cuda", capacity=8)                  # (grows on the way)
    for frames in seqs[1:]:
        got = C.sweep_runs(tracker, [frames])
        log.reset()
        assert tracker_for(model).track_logged(frames, log) == len(frames)
        for k in range(len(C.SETTINGS)):
            lines = [line for idx, r in enumerate(got[k][0]) for line in tracker.mot_lines(idx, r)]
            assert log.mot_lines(k) == lines and lines


def test_steps_3_to_6_do_not_synchronise(scenario):
    """After a warm-up run (graphs captured, the mask broadcast), the broadcast of the encode result, decode, bank update,
    query update, the count copy and the result rows of one step run with torch's synchronisation check set to raise."""
    model, seqs, _, _ = scenario
    frames, S = seqs[1], len(C.SETTINGS)
    log = BankResultLog("cuda", capacity=4096)
    tracker = tracker_for(model)
    tracker.track_logged(frames, log)                        # warm-up
    tracker.begin(S)
    ori_wh = torch.tensor([[M.FRAME_W, M.FRAME_H]] * S, dtype=torch.float32).cuda()
    for i in range(3):
        seq_frame = torch.tensor([[k, i] for k in range(S)]).cuda()
        enc = tracker._encoded(_Step([frames[i]]), False)    # steps 1-2: one frame
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            tracker._track(enc, None, False)                 # steps 2b-5
            log.append_streams(tracker.bank, seq_frame, ori_wh, tracker.thresholds)       # step 6
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert int(tracker.bank.counters[:, 0].min()) > 0
