"""CPU: the result log (memotr_amd/results.py) on CPU tensors is the host statement the result-row kernel is held to.
It gives, string for string, what ``SequenceTracker._report`` + ``mot_lines`` give; scores and areas exactly at their
float32 thresholds and NaN rows are dropped; the clip library's binding matches its header at ABI 12 and the new entry
point reports argument errors without a device.  ``TIE_ROWS`` is shared with tests/test_result_log_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header

from memotr_amd.results import ResultLog, host_rows

NAN = float("nan")
# (cx, cy, w, h), scores, kept? -- against result_score_thresh 0.5 or 0.7 (see the test), area_thresh 100, 100 x 200 px
F32 = lambda x: float(np.float32(x))                                                # noqa: E731
TIE_ROWS = [
    ((0.5, 0.5, 0.2, 0.3), (0.9, 0.1), True),                  # 40 x 30 px, well inside
    ((0.5, 0.5, 0.2, 0.3), (F32(0.5), 0.2), False),            # the score is float32(0.5): not above 0.5
    ((0.5, 0.5, 0.2, 0.3), (0.1, F32(0.7)), None),             # float32(0.7): above 0.5, not above 0.7
    ((0.5, 0.5, 0.05, 0.1), (0.9, 0.9), False),                # 10 x 10 px: area 100 is not above 100
    ((0.5, 0.5, 0.055, 0.1), (0.9, 0.9), True),                # 11 x 10 px
    ((0.5, 0.5, 0.2, 0.3), (NAN, 0.9), False),                 # a NaN score wins the max and fails the comparison
    ((0.5, 0.5, 0.2, 0.3), (0.9, NAN), False),
    ((0.5, 0.5, NAN, 0.3), (0.9, 0.9), False),                 # a NaN box: NaN area
    ((0.5, 0.5, 0.2, NAN), (0.9, 0.9), False),
    ((0.25, 0.75, 0.5, 0.5), (F32(0.7), float(np.nextafter(np.float32(0.7), np.float32(1)))), True),   # one ulp above
]


def tie_tensors(device="cpu"):
    boxes = torch.tensor([r[0] for r in TIE_ROWS], dtype=torch.float32, device=device)
    scores = torch.tensor([r[1] for r in TIE_ROWS], dtype=torch.float32, device=device)
    ids = torch.arange(100, 100 + len(TIE_ROWS), device=device)
    return boxes, scores, ids, torch.zeros_like(ids)


def tie_expected(score_thresh):
    return [100 + i for i, r in enumerate(TIE_ROWS) if (r[2] if r[2] is not None else score_thresh < 0.7)]


def random_tracks(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    boxes = torch.rand(n, 4, generator=g) * torch.tensor([0.8, 0.8, 0.3, 0.3]) + torch.tensor([0.1, 0.1, 0.0, 0.0])
    return boxes, torch.rand(n, K, generator=g), torch.randperm(1000, generator=g)[:n], \
        torch.randint(0, 8, (n,), generator=g)


class _Tracks:
    """What ``_report`` reads of a TrackInstances."""

    def __init__(self, boxes, scores, ids, labels):
        self.boxes, self.scores, self.ids, self.labels = boxes, scores, ids, labels
        self.hidden_dim, self.num_classes = 8, scores.shape[-1]

    def __len__(self):
        return len(self.ids)


def reporter(score_thresh, area_thresh, dataset="DanceTrack"):
    from memotr_amd.inference import SequenceTracker
    t = SequenceTracker.__new__(SequenceTracker)              # _report and mot_lines read these three only
    t.result_score_thresh, t.area_thresh, t.use_dab, t.dataset_name = score_thresh, area_thresh, True, dataset
    return t


@pytest.mark.parametrize("K", [1, 8])
def test_the_host_statement_gives_the_lines_of_report_and_mot_lines(K):
    tracker, log = reporter(0.5, 100), ResultLog("cpu", capacity=16)
    want, kept, total = [], 0, 0
    for frame, (n, size) in enumerate([(40, (1080, 1920)), (0, (1080, 1920)), (75, (480, 641)), (3, (97, 131))]):
        boxes, scores, ids, labels = random_tracks(n, K, seed=10 * K + frame)
        result = tracker._report(_Tracks(boxes, scores, ids, labels), *size)
        want += tracker.mot_lines(frame, result)
        log.append(boxes, scores, ids, labels, frame, size[0], size[1], 0.5, 100)
        kept, total = kept + len(result), total + n
    assert 0 < kept < total
    rows = log.read()
    assert len(rows.frames) == kept and rows.boxes_xyxy.dtype == np.float32 and rows.ids.dtype == np.int64
    assert log.mot_lines("DanceTrack") == want
    assert int(log.counters[0]) == kept and int(log.counters[1]) == 0 and log.capacity >= kept
    log.reset()
    assert len(log) == 0 and log.mot_lines("DanceTrack") == []
    with pytest.raises(ValueError, match="not supported"):
        log.mot_lines("BDD100K")


def test_one_dimensional_scores_are_one_class():
    boxes, scores, ids, labels = random_tracks(20, 1, seed=3)
    a, b = ResultLog("cpu"), ResultLog("cpu")
    a.append(boxes, scores, ids, labels, 0, 100, 200, 0.5, 10)
    b.append(boxes, scores[:, 0], ids, labels, 0, 100, 200, 0.5, 10)
    assert a.mot_lines("MOT17") == b.mot_lines("MOT17") and len(a) > 0


@pytest.mark.parametrize("score_thresh", [0.5, 0.7])
def test_ties_and_nan_are_dropped(score_thresh):
    boxes, scores, ids, labels = tie_tensors()
    assert float(boxes[3, 2] * 200 * boxes[3, 3] * 100) == 100.0             # exactly at the area threshold
    log = ResultLog("cpu")
    log.append(boxes, scores, ids, labels, 0, 100, 200, score_thresh, 100)
    assert log.read().ids.tolist() == tie_expected(score_thresh)
    # ... and that is what _report keeps
    result = reporter(score_thresh, 100)._report(_Tracks(boxes, scores, ids, labels), 100, 200)
    assert result.ids.tolist() == tie_expected(score_thresh)
    assert torch.equal(result.boxes, torch.from_numpy(log.read().boxes_xyxy))


def test_bdd_frames_and_evaluator_rows_are_what_the_frame_loop_gives():
    from memotr_amd.evaluation import TrackingEvaluator
    from memotr_amd.inference import SequenceTracker
    tracker, log = reporter(0.5, 100, "BDD100K"), ResultLog("cpu")
    paths = [f"/data/BDD100K/images/track/val/b1c81faa-3df17267/b1c81faa-3df17267-{t:07d}.jpg" for t in range(1, 5)]
    want, ev_a, ev_b = [], TrackingEvaluator(), TrackingEvaluator()
    for frame, n in enumerate([12, 0, 9, 5]):
        boxes, scores, ids, labels = random_tracks(n, 8, seed=50 + frame)
        if frame == 3:
            scores = scores * 0.4                                                # a frame with tracks and no row
        result = tracker._report(_Tracks(boxes, scores, ids, labels), 720, 1280)
        want.append(SequenceTracker.bdd_frame_result(frame, result, paths[frame]))
        ev_a.add_frame("s", frame, result)
        log.append(boxes, scores, ids, labels, frame, 720, 1280, 0.5, 100)
    got = log.bdd_frames(paths)
    assert got == want and got[1]["labels"] == [] and got[3]["labels"] == [] and got[0]["labels"]
    assert got[2]["videoName"] == "b1c81faa-3df17267" and got[2]["frameIndex"] == 2
    log.add_to(ev_b, "s", n_frames=4)
    a, b = ev_a.sequences()["s"], ev_b.sequences()["s"]
    assert len(a["tracker_ids"]) == len(b["tracker_ids"]) == 4
    for k in ("tracker_ids", "tracker_boxes"):
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[k], b[k])), k


def test_the_log_grows_and_read_raises_on_dropped_rows():
    log = ResultLog("cpu", capacity=8)
    for frame in range(5):
        boxes, scores, ids, labels = random_tracks(100, 1, seed=frame)
        log.append(boxes, scores, ids, labels, frame, 1000, 1000, -1.0, -1.0)
    assert len(log) == 500 and log.capacity >= 500 and log.read().frames.tolist() == sorted(log.read().frames.tolist())
    log.counters[1] = 2
    log._rows = None
    with pytest.raises(RuntimeError, match="2 rows found no room"):
        log.read()


@pytest.mark.parametrize("kind", ["one sequence", "bank"])
def test_both_logs_share_the_tables_growth_and_the_two_read_errors(kind):
    from memotr_amd.results import BANK_ROW_I, ROW_I, BankResultLog
    log, width = (ResultLog("cpu", capacity=4), ROW_I) if kind == "one sequence" else \
        (BankResultLog("cpu", capacity=4), BANK_ROW_I)
    rows_i = torch.arange(3 * width).reshape(3, width)
    rows_i[:, 0] = 0                                            # (frame 0, or sequence 0 of the bank log)
    rows_f = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    log.rows_i[:3], log.rows_f[:3], log.counters[0], log._bound = rows_i, rows_f, 3, 3
    log._make_room(6)                                           # 3 in use + 6 offered > 4: max(2 * 4, 9)
    assert log.capacity == 9 and tuple(log.rows_i.shape) == (9, width) and tuple(log.rows_f.shape) == (9, 5)
    assert torch.equal(log.rows_i[:3], rows_i) and torch.equal(log.rows_f[:3], rows_f)
    got = log.read() if kind == "one sequence" else log.read()[0]
    assert got.ids.tolist() == rows_i[:, width - 2].tolist() and got.scores.tolist() == rows_f[:, 4].tolist()
    log.counters[0], log._rows = 5, None
    with pytest.raises(RuntimeError, match=r"result log: 5 rows stored, 3 offered \(counters written from elsewhere\?\)"):
        log.read()
    log.counters[0], log.counters[1] = 3, 2
    with pytest.raises(RuntimeError, match="result log: 2 rows found no room in a table of 9"):
        log.read()
    log.reset()
    assert log.counters.tolist() == [0, 0] and log.capacity == 9
    assert len(log) == 0 if kind == "one sequence" else log.read() == {}


def test_host_rows_keeps_input_order_and_float32():
    boxes, scores, ids, labels = random_tracks(30, 8, seed=9)
    rows_f, rows_i = host_rows(boxes.double(), scores.double(), ids, labels, 7, 1080, 1920, 0.5, 100)
    assert rows_f.dtype == torch.float32 and rows_i.dtype == torch.int64 and (rows_i[:, 0] == 7).all()
    keep = (scores.max(-1).values > 0.5) & (boxes[:, 2] * 1920 * boxes[:, 3] * 1080 > 100)
    assert rows_i[:, 1].tolist() == ids[keep].tolist() and rows_i[:, 2].tolist() == labels[keep].tolist()
    assert torch.equal(rows_f[:, 4], scores.max(-1).values[keep])
    empty_f, empty_i = host_rows(boxes[:0], scores[:0], ids[:0], labels[:0], 0, 10, 10, 0.5, 100)
    assert tuple(empty_f.shape) == (0, 5) and tuple(empty_i.shape) == (0, 3)


# ---------------------------------------------------------------------------------------------- the library
def test_the_binding_matches_the_header_at_abi_12(clip_lib):
    declared = assert_binding_matches_header(clip_lib, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert "clipops_result_rows_f32" in declared and clip_lib.ABI_VERSION == 12
    assert clip_lib.lib.clipops_abi_version() == 12


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib, d = clip_lib.lib, ctypes.c_void_p(64)

    def call(boxes=d, scores=d, ids=d, labels=d, n=4, K=1, rows_f=d, rows_i=d, counters=d, capacity=16):
        return lib.clipops_result_rows_f32(boxes, scores, ids, labels, n, K, 0, 100.0, 100.0, 0.5, 100.0, rows_f, rows_i,
                                           counters, capacity, None)

    assert call(n=-1) == 1 and b"negative" in lib.clipops_last_error()
    assert call(capacity=-1) == 1 and b"negative" in lib.clipops_last_error()
    assert call(K=0) == 1 and b"K < 1" in lib.clipops_last_error()
    for name in ("boxes", "scores", "ids", "labels", "rows_f", "rows_i", "counters"):
        assert call(**{name: None}) == 1 and b"null" in lib.clipops_last_error(), name
    # no rows: a successful no-op that launches nothing, whatever the pointers, and clears the error text
    assert call(n=0, boxes=None, rows_f=None, counters=None) == 0 and lib.clipops_last_error() == b""
    with pytest.raises(RuntimeError, match="null pointer"):
        clip_lib.check(call(ids=None), "clipops_result_rows_f32")
