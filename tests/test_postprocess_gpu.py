"""GPU: ``ResultLog.filled`` / ``BankResultLog.filled`` (clipops_fill_gaps_f32, memotr_amd/csrc/clip_fill_gaps.h) against
the host statement (memotr_amd/postprocess.py ``fill_gaps``), bit for bit: table sizes at the wavefront and chunk edges
of the scans and ranks, holes across those edges, bank tables, the capacity rule with guard words, the status bits, and
tracking runs and ``submit`` with the pass on."""
import os

import numpy as np
import pytest
import torch

import dataset_trees as T
import multi_track_cases as M
import postprocess_cases as C

from memotr_amd import submit as S
from memotr_amd.postprocess import fill_gaps
from memotr_amd.results import BankResultLog, ResultLog, Rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def libraries(request):
    request.getfixturevalue("hip_lib"), request.getfixturevalue("clip_lib")


def check(rows, max_gap, min_length=0, n_frames=None, n_ids=None, shuffle=None):
    """The device pass on ``rows`` (stored in a shuffled order when asked) against the host statement."""
    stored = rows
    if shuffle is not None:
        perm = np.random.RandomState(shuffle).permutation(len(rows.frames))
        stored = Rows(*(a[perm] for a in rows))
    got = C.log_from_rows(stored, "cuda", spare=3).filled(max_gap, min_length, n_frames=n_frames, n_ids=n_ids)
    assert isinstance(got, ResultLog) and got.device.type == "cuda"
    want = fill_gaps(rows, max_gap, min_length)
    C.assert_same_rows(got.read(), want)
    return want


def three_track_mask(n_frames, seed):
    """id 0 in every frame, id 1 with about 40 % of its rows missing, id 2 in every seventh frame."""
    mask = np.zeros((3, n_frames), bool)
    mask[0] = True
    mask[1] = C.random_mask(1, n_frames, 0.4, seed)[0]
    mask[2, ::7] = True
    return mask


@pytest.mark.parametrize("n_frames", [1, 2, 63, 64, 65, 1023, 1025])
def test_frame_axis_sizes(n_frames):
    rows = C.rows_from_mask(three_track_mask(n_frames, n_frames), n_frames)
    for max_gap, min_length in ((5, 0), (6, 2), (0, 0)):
        check(rows, max_gap, min_length, n_frames=n_frames, n_ids=3, shuffle=1)
    check(rows, 6, 0)                                       # the sizes found by the log's own small read


@pytest.mark.parametrize("n_ids", [1, 64, 65, 1030])
def test_id_axis_sizes(n_ids):
    rows = C.rows_from_mask(C.random_mask(n_ids, 70, 0.3, n_ids), n_ids)
    want = check(rows, 3, 20, n_frames=70, n_ids=n_ids, shuffle=2)
    assert len(want.frames) != len(rows.frames)
    check(rows, 3, 0)


def test_holes_across_the_wavefront_and_chunk_edges():
    n_frames = 1100
    mask = np.ones((4, n_frames), bool)
    mask[0, 62:66] = False                                  # straddles 63 / 64
    mask[1, 1020:1028] = False                              # straddles 1023 / 1024
    mask[2, 1:n_frames - 1] = False                         # only the first and the last frame
    mask[3, 64:1024] = False                                # a hole of exactly the inner chunk
    rows = C.rows_from_mask(mask, 9)
    for max_gap in (3, 4, 8, 960, n_frames):
        want = check(rows, max_gap, 0, n_frames=n_frames, n_ids=4)
    assert len(want.frames) == 4 * n_frames                 # max_gap = n_frames closes everything
    check(rows, 7, 3, n_frames=n_frames, n_ids=4)           # the two-row track goes, and fills nothing


def test_full_sparse_and_nan_tables():
    full = C.rows_from_mask(np.ones((5, 130), bool), 3)
    assert len(check(full, 10, 2, n_frames=130, n_ids=5).frames) == 5 * 130
    mask = np.zeros((90, 70), bool)                         # only ids 0 and n_ids - 1
    mask[0, ::4], mask[89, 1::5] = True, True
    check(C.rows_from_mask(mask, 4), 4, 0, n_frames=70, n_ids=90)
    check(C.empty_rows(), 4, 2)
    check(C.empty_rows(), 4, 2, n_frames=10, n_ids=10)
    mask = np.zeros((2, 12), bool)
    mask[:, [0, 3, 7, 11]] = True
    rows = C.rows_from_mask(mask, 5)
    rows.scores[2], rows.boxes_xyxy[5, 1] = np.nan, np.inf
    want = check(rows, 3, 0, n_frames=12, n_ids=2)
    assert np.isnan(want.scores).sum() > 1
    # a table much larger than what it holds, ids and frames far from 0
    rows = Rows(np.asarray([5000, 5003, 5004], np.int64), np.asarray([900, 900, 17], np.int64), np.zeros(3, np.int64),
                rows.boxes_xyxy[:3], rows.scores[4:7])
    check(rows, 2, 0, n_frames=6000, n_ids=1000)
    check(rows, 2, 0)


def test_random_deletion_on_200_frames_of_40_ids():
    rows = C.rows_from_mask(C.random_mask(40, 200, 0.3, 7), 7)
    want = check(rows, 5, 4, n_frames=200, n_ids=40, shuffle=3)
    assert len(want.frames) > len(rows.frames)
    again = C.log_from_rows(want, "cuda").filled(5, 4, n_frames=200, n_ids=40)       # idempotent on the device too
    C.assert_same_rows(again.read(), want)
    a, b = (C.log_from_rows(rows, "cuda").filled(5, 4) for _ in range(2))              # the same bits every time
    assert torch.equal(a.rows_f[:len(want.frames)].view(torch.int32), b.rows_f[:len(want.frames)].view(torch.int32))
    assert torch.equal(a.rows_i[:len(want.frames)], b.rows_i[:len(want.frames)])


def test_bank_tables():
    sequences = {0: C.rows_from_mask(C.random_mask(70, 40, 0.35, 0), 0),
                 1: C.rows_from_mask(three_track_mask(1030, 1), 1),
                 3: C.rows_from_mask(C.random_mask(5, 66, 0.5, 2), 2)}               # sequence 2 has no row
    log = C.bank_log_from_rows(sequences, "cuda")
    for kwargs in (dict(n_frames=1030, n_ids=70, n_sequences=4), dict(), dict(n_sequences=5, n_ids=64 + 7)):
        got = log.filled(4, 3, **kwargs)
        assert isinstance(got, BankResultLog) and got.dataset_name == log.dataset_name
        assert sorted(got.read()) == [0, 1, 3]
        for seq, rows in sequences.items():
            C.assert_same_rows(got.read()[seq], fill_gaps(rows, 4, 3))
            C.assert_same_rows(got.sequence(seq).read(), fill_gaps(rows, 4, 3))
        assert len(got.sequence(2)) == 0
        # the table itself is in (sequence, frame, id) order
        stored = int(got.counters[0])
        rows_i = got.rows_i[:stored].cpu().numpy()
        assert np.array_equal(np.lexsort((rows_i[:, 2], rows_i[:, 1], rows_i[:, 0])), np.arange(stored))
    assert C.bank_log_from_rows({}, "cuda").filled(3).read() == {}
    with pytest.raises(RuntimeError, match="sequence out of range"):
        log.filled(4, 3, n_sequences=3).read()


def test_a_table_that_is_too_small_drops_rows_and_writes_nothing_behind_it():
    from memotr_amd import _clip_lib as L
    rows = C.rows_from_mask(C.random_mask(6, 50, 0.4, 11), 11)
    want = fill_gaps(rows, 5)
    total, capacity, guard = len(want.frames), 100, 8
    assert total > capacity + 10
    log = C.log_from_rows(rows, "cuda")
    out_f = torch.full(((capacity + guard) * 5,), -7.25, device="cuda")
    out_i = torch.full(((capacity + guard) * 3,), -77, dtype=torch.int64, device="cuda")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    workspace = torch.empty(L.lib.clipops_fill_gaps_workspace(1, 6, 50), dtype=torch.int32, device="cuda")
    for start in (0, 40):                                   # the second call appends behind 40 rows: 60 find room
        counters.copy_(torch.tensor([start, 0], dtype=torch.int32))
        L.check(L.lib.clipops_fill_gaps_f32(
            log.rows_f.data_ptr(), log.rows_i.data_ptr(), log.counters.data_ptr(), log._bound, 3, 1, 6, 50, 5, 0,
            workspace.data_ptr(), out_f.data_ptr(), out_i.data_ptr(), counters.data_ptr(), status.data_ptr(), capacity,
            torch.cuda.current_stream().cuda_stream), "clipops_fill_gaps_f32")
        assert counters.tolist() == [capacity, total - (capacity - start)] and status.tolist() == [0]
        assert bool((out_f[capacity * 5:] == -7.25).all()) and bool((out_i[capacity * 3:] == -77).all())
        n = capacity - start
        got_f = out_f[start * 5:capacity * 5].reshape(n, 5).cpu().numpy()
        got_i = out_i[start * 3:capacity * 3].reshape(n, 3).cpu().numpy()
        assert np.array_equal(got_f.view(np.int32), C.values_of(want)[:n].view(np.int32))
        assert got_i[:, 0].tolist() == want.frames[:n].tolist() and got_i[:, 1].tolist() == want.ids[:n].tolist()
    # the log's own read names the dropped rows
    small = log.filled(5)
    small.counters[1] = 3
    with pytest.raises(RuntimeError, match="found no room"):
        small.read()


def test_each_status_bit_raises_in_read():
    rows = C.rows_from_mask(C.random_mask(4, 20, 0.3, 13), 13)
    twice = Rows(*(np.concatenate((a, a[5:6])) for a in rows))
    with pytest.raises(RuntimeError, match=r"duplicate \(frame, id\)"):
        C.log_from_rows(twice, "cuda").filled(3, n_frames=20, n_ids=4).read()
    log = C.log_from_rows(rows, "cuda")
    with pytest.raises(RuntimeError, match="id out of range"):
        log.filled(3, n_frames=20, n_ids=3).read()
    with pytest.raises(RuntimeError, match="frame out of range"):
        log.filled(3, n_frames=19, n_ids=4).read()
    negative = Rows(rows.frames, np.where(rows.ids == 2, -1, rows.ids), rows.labels, rows.boxes_xyxy, rows.scores)
    with pytest.raises(RuntimeError, match="id out of range"):
        C.log_from_rows(negative, "cuda").filled(3).read()
    with pytest.raises(RuntimeError, match="id out of range.*frame out of range"):
        log.filled(3, n_frames=0, n_ids=0).read()
    with pytest.raises(ValueError):
        log.filled(-1)
    with pytest.raises(ValueError, match="cells"):
        log.filled(3, n_frames=1 << 20, n_ids=1 << 12)
    C.assert_same_rows(log.filled(3, n_frames=20, n_ids=4).read(), fill_gaps(rows, 3))


def test_filled_with_known_sizes_does_not_synchronise():
    rows = C.rows_from_mask(C.random_mask(8, 100, 0.3, 17), 17)
    log = C.log_from_rows(rows, "cuda")
    log.filled(4, 2, n_frames=100, n_ids=8)                  # warm-up: the allocator has the blocks
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = log.filled(4, 2, n_frames=100, n_ids=8)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    C.assert_same_rows(got.read(), fill_gaps(rows, 4, 2))


# ---------------------------------------------------------------------------------------------- tracking runs
@pytest.fixture(scope="module")
def scenario_model():
    return M.scenario_model(256).cuda()


def test_track_logged_then_filled_is_the_host_statement_of_the_log(scenario_model):
    """The 256-wide small model of tests/multi_track_cases.py on nine frames; the result threshold is then put where
    some track's score dips for a frame, so that the log has a hole to fill."""
    from memotr_amd.inference import SequenceTracker
    frames = M.sequences((6, 9, 7))[1]
    options = dict(M.OPTIONS, result_score_thresh=0.45, miss_tolerance=4)
    log = ResultLog("cuda")
    assert SequenceTracker(scenario_model, **options).track_logged(frames, log) == 9
    options["result_score_thresh"] = C.hole_threshold([log.read()])
    log.reset()
    t = SequenceTracker(scenario_model, **options)
    assert t.track_logged(frames, log) == 9
    raw = log.read()
    print("rows as tracked:", len(raw.frames), "filled:", len(fill_gaps(raw, 5).frames))
    assert len(fill_gaps(raw, 5).frames) > len(raw.frames) > 0
    for max_gap, min_length in ((5, 0), (1, 3), (0, 0)):
        want = fill_gaps(raw, max_gap, min_length)
        got = log.filled(max_gap, min_length, n_frames=9, n_ids=t.tracker.max_obj_id)
        C.assert_same_rows(got.read(), want)
        assert got.mot_lines("DanceTrack") == C.log_from_rows(want, "cpu").mot_lines("DanceTrack")
        C.assert_same_rows(log.filled(max_gap, min_length).read(), want)
    C.assert_same_rows(log.read(), raw)                     # the log itself is as it was


def test_track_many_logged_then_filled(scenario_model):
    from memotr_amd.inference_multi import MultiSequenceTracker
    seqs = M.sequences((6, 9, 7))
    options = dict(M.OPTIONS, result_score_thresh=0.45, miss_tolerance=4)
    log = BankResultLog("cuda")
    counts = MultiSequenceTracker(scenario_model, n_streams=2, cap=32, **options).track_many_logged(seqs, log)
    assert counts == [6, 9, 7]
    options["result_score_thresh"] = C.hole_threshold(list(log.read().values()))
    log.reset()
    MultiSequenceTracker(scenario_model, n_streams=2, cap=32, **options).track_many_logged(seqs, log)
    raw = log.read()
    assert sorted(raw) == [0, 1, 2]
    assert sum(len(fill_gaps(r, 3).frames) for r in raw.values()) > sum(len(r.frames) for r in raw.values())
    for kwargs in (dict(n_frames=9, n_sequences=3), dict()):
        got = log.filled(3, 2, **kwargs)
        for seq in range(3):
            want = fill_gaps(raw[seq], 3, 2)
            print("sequence", seq, "rows as tracked:", len(raw[seq].frames), "filled:", len(want.frames))
            C.assert_same_rows(got.sequence(seq).read(), want)
            assert got.mot_lines(seq) == C.log_from_rows(want, "cpu").mot_lines("DanceTrack")


@pytest.mark.parametrize("streams", [1, 2])
def test_submit_writes_the_host_statement_of_its_own_rows(scenario_model, tmp_path, monkeypatch, streams):
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.inference_multi import MultiSequenceTracker
    monkeypatch.delenv("MEMOTR_POSTPROCESS", raising=False)
    root = T.write_trees(str(tmp_path / "data"), only=("DanceTrack",))
    thresholds = dict(DET_SCORE_THRESH=0.8, TRACK_SCORE_THRESH=0.45, RESULT_SCORE_THRESH=0.62, MISS_TOLERANCE=4,
                      USE_MOTION=False)
    options = dict(dataset_name="DanceTrack", use_dab=True, det_score_thresh=0.8, track_score_thresh=0.45,
                   result_score_thresh=0.62, miss_tolerance=4, raw_size=M.RAW_SIZE, area_thresh=10)
    names = sorted(T.DANCE_SEQS)
    paths = [S.sequence_frames("DanceTrack", os.path.join(root, "DanceTrack", "train", seq)) for seq in names]
    if streams == 1:
        raw = []
        for p in paths:
            log = ResultLog("cuda")
            SequenceTracker(scenario_model, **options).track_logged(p, log)
            raw.append(log.read())
    else:
        log = BankResultLog("cuda")
        MultiSequenceTracker(scenario_model, n_streams=2, **options).track_many_logged(paths, log)
        raw = [log.sequence(i).read() for i in range(len(paths))]
    pp = dict(max_gap=3, min_length=2)
    want = ["".join(C.log_from_rows(fill_gaps(r, **pp), "cpu").mot_lines("DanceTrack")) for r in raw]
    plain = ["".join(C.log_from_rows(r, "cpu").mot_lines("DanceTrack")) for r in raw]

    def run(out, **kwargs):
        config = dict(thresholds, SUBMIT_DIR=str(tmp_path / out), SUBMIT_MODEL=None, SUBMIT_DATA_SPLIT="train",
                      DATA_ROOT=root)
        files = S.submit(config, model=scenario_model, train_config=dict(DATASET="DanceTrack", USE_DAB=True),
                         tracker_options=dict(raw_size=M.RAW_SIZE, area_thresh=10), streams=streams, **kwargs)
        texts = []
        for path in files:
            with open(path) as f:
                texts.append(f.read())
        return texts

    assert run("on", postprocess=pp) == want
    assert run("off") == plain
    print("streams", streams, "lines as tracked:", [t.count("\n") for t in plain], "filled:", [t.count("\n") for t in want])
