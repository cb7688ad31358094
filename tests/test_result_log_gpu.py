"""GPU: the result-row kernel (clipops_result_rows_f32, memotr_amd/csrc/clip_tracks.h) against the host statement
(memotr_amd/results.py:host_rows through a CPU ``ResultLog``), bit for bit: every keep pattern at the lane, wavefront
and chunk edges, input order, appending, the capacity rule with guard words behind the tables, growth, ties and NaN;
and ``SequenceTracker.track_logged`` + ``ResultLog.mot_lines`` against ``track`` / ``track_jpeg`` + ``mot_lines``, byte
for byte."""
import numpy as np
import pytest
import torch

from dataset_trees import frame_pixels
from test_frames_gpu import build_memotr_cuda
from test_result_log_cpu import tie_expected, tie_tensors

from memotr_amd.results import ResultLog

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 600)
PATTERNS = ("all", "none", "alternating", "first", "last", "63_64", "255_256", "random30")
ORI_H, ORI_W, SCORE_T, AREA_T = 1080, 1920, 0.5, 100


def keep_mask(pattern, n):
    keep = torch.zeros(n, dtype=torch.bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "alternating":
        keep[::2] = True
    elif pattern == "first":
        keep[:1] = True
    elif pattern == "last":
        keep[-1:] = True
    elif pattern == "63_64":
        keep[63:65] = True
    elif pattern == "255_256":
        keep[255:257] = True
    elif pattern == "random30":
        keep = torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.3
    return keep


def tracks_for(keep, K, seed):
    """Rows that pass both filters where ``keep`` is set; the others fail the score filter (even rows) or the area
    filter (odd rows).  ids are a fixed permutation of arange(n)."""
    n = len(keep)
    g = torch.Generator().manual_seed(seed)
    boxes = torch.rand(n, 4, generator=g) * torch.tensor([0.6, 0.6, 0.2, 0.2]) + torch.tensor([0.2, 0.2, 0.05, 0.05])
    scores = torch.rand(n, K, generator=g) * 0.4                      # all below the threshold ...
    top = torch.randint(0, K, (n,), generator=g)
    scores[torch.arange(n), top] = 0.6 + 0.4 * torch.rand(n, generator=g)         # ... but one column per row
    rows = torch.arange(n)
    by_score, by_area = ~keep & (rows % 2 == 0), ~keep & (rows % 2 == 1)
    scores[by_score] *= 0.5
    boxes[by_area, 2:] = 0.004                                        # 7.7 x 4.3 px
    return boxes, scores, torch.randperm(n, generator=g), torch.randint(0, 8, (n,), generator=g)


def both_logs(calls, capacity=4096):
    """The same appends on a CPU log (the host statement) and on a device log."""
    host, dev = ResultLog("cpu", capacity), ResultLog("cuda", capacity)
    for frame, (boxes, scores, ids, labels) in calls:
        host.append(boxes, scores, ids, labels, frame, ORI_H, ORI_W, SCORE_T, AREA_T)
        dev.append(boxes.cuda(), scores.cuda(), ids.cuda(), labels.cuda(), frame, ORI_H, ORI_W, SCORE_T, AREA_T)
    return host, dev


def assert_same_tables(host, dev):
    counters = dev.counters.cpu()
    assert counters.tolist() == host.counters.tolist() and counters[1] == 0
    m = int(counters[0])
    assert torch.equal(dev.rows_f[:m].cpu().view(torch.int32), host.rows_f[:m].view(torch.int32))
    assert torch.equal(dev.rows_i[:m].cpu(), host.rows_i[:m])
    return m


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_kernel_equals_the_host_statement_at_every_size_and_keep_pattern(clip_lib, pattern, K):
    for n in SIZES:
        keep = keep_mask(pattern, n)
        boxes, scores, ids, labels = tracks_for(keep, K, seed=1000 * K + n)
        host, dev = both_logs([(3, (boxes, scores, ids, labels))])
        m = assert_same_tables(host, dev)
        assert m == int(keep.sum()), (n, m)
        # input order: the stored ids are the kept ones of the shuffled arange, in the order they came in
        assert dev.rows_i[:m, 1].cpu().tolist() == ids[keep].tolist() and (dev.rows_i[:m, 0] == 3).all()
        assert dev.read().ids.tolist() == ids[keep].tolist()


def test_appending_continues_behind_the_rows_already_there(clip_lib):
    calls = []
    for frame, n in enumerate([300, 0, 70]):
        calls.append((frame, tracks_for(keep_mask("random30", n), 8, seed=frame)))
    host, dev = both_logs(calls)
    m = assert_same_tables(host, dev)
    frames = dev.read().frames.tolist()
    assert m == len(frames) and set(frames) == {0, 2} and frames == sorted(frames)
    assert dev.mot_lines("DanceTrack") == host.mot_lines("DanceTrack")
    dev.reset()
    assert dev.counters.cpu().tolist() == [0, 0] and len(dev) == 0


def test_rows_past_the_capacity_are_counted_and_nothing_is_written_behind_the_tables(clip_lib):
    n, K, guard = 300, 8, 64
    keep = keep_mask("alternating", n)
    kept = int(keep.sum())
    boxes, scores, ids, labels = tracks_for(keep, K, seed=5)
    host = ResultLog("cpu")
    host.append(boxes, scores, ids, labels, 9, ORI_H, ORI_W, SCORE_T, AREA_T)
    b, s, i, lab = boxes.cuda(), scores.cuda(), ids.cuda(), labels.cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for capacity, want in ((kept, [kept, 0]), (kept - 1, [kept - 1, 1])):
        rows_f = torch.full((capacity * 5 + guard,), -7.5, device="cuda")
        rows_i = torch.full((capacity * 3 + guard,), -77, dtype=torch.int64, device="cuda")
        counters = torch.zeros(2 + guard, dtype=torch.int32, device="cuda")
        counters[2:] = -777
        clip_lib.check(clip_lib.lib.clipops_result_rows_f32(
            b.data_ptr(), s.data_ptr(), i.data_ptr(), lab.data_ptr(), n, K, 9, float(ORI_W), float(ORI_H), SCORE_T,
            float(AREA_T), rows_f.data_ptr(), rows_i.data_ptr(), counters.data_ptr(), capacity, stream),
            "clipops_result_rows_f32")
        assert counters[:2].cpu().tolist() == want
        m = want[0]                                                   # the first rows are the ones stored
        assert torch.equal(rows_f[:capacity * 5].cpu().view(m, 5).view(torch.int32), host.rows_f[:m].view(torch.int32))
        assert torch.equal(rows_i[:capacity * 3].cpu().view(m, 3), host.rows_i[:m])
        assert (rows_f[capacity * 5:] == -7.5).all() and (rows_i[capacity * 3:] == -77).all()
        assert (counters[2:] == -777).all()
    # a table that is full already: everything is counted as dropped, the stored count stays
    counters = torch.tensor([4, 1], dtype=torch.int32, device="cuda")
    rows_f = torch.full((4 * 5 + guard,), -7.5, device="cuda")
    rows_i = torch.full((4 * 3 + guard,), -77, dtype=torch.int64, device="cuda")
    clip_lib.check(clip_lib.lib.clipops_result_rows_f32(
        b.data_ptr(), s.data_ptr(), i.data_ptr(), lab.data_ptr(), n, K, 9, float(ORI_W), float(ORI_H), SCORE_T,
        float(AREA_T), rows_f.data_ptr(), rows_i.data_ptr(), counters.data_ptr(), 4, stream), "clipops_result_rows_f32")
    assert counters.cpu().tolist() == [4, 1 + kept]
    assert (rows_f == -7.5).all() and (rows_i == -77).all()


def test_a_small_log_grows_without_dropping_a_row(clip_lib):
    calls = [(frame, tracks_for(keep_mask("all", 100), 1, seed=20 + frame)) for frame in range(5)]
    host, dev = both_logs(calls, capacity=8)
    assert assert_same_tables(host, dev) == 500 and dev.capacity >= 500
    rows = dev.read()
    assert len(rows.frames) == 500 and int(dev.counters[1]) == 0
    assert rows.frames.tolist() == [f for f in range(5) for _ in range(100)]
    assert np.array_equal(rows.boxes_xyxy, host.read().boxes_xyxy) and np.array_equal(rows.scores, host.read().scores)


@pytest.mark.parametrize("score_thresh", [0.5, 0.7])
def test_ties_and_nan_are_dropped_on_the_device(clip_lib, score_thresh):
    boxes, scores, ids, labels = tie_tensors()
    host, dev = ResultLog("cpu"), ResultLog("cuda")
    host.append(boxes, scores, ids, labels, 0, 100, 200, score_thresh, 100)
    dev.append(boxes.cuda(), scores.cuda(), ids.cuda(), labels.cuda(), 0, 100, 200, score_thresh, 100)
    assert_same_tables(host, dev)
    assert dev.read().ids.tolist() == tie_expected(score_thresh)


def test_track_logged_gives_the_lines_of_track_and_track_jpeg(hip_lib, clip_lib, monkeypatch):
    """The d32 model and thresholds of test_inference_graphs_match_the_eager_tracker (births: the three best
    detections of the first frame; track threshold 0) on eight 48 x 80 frames."""
    from memotr_amd.data import encode_jpeg
    from memotr_amd.data.frames import preprocess_frames, target_size
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models.utils import logits_to_scores
    import memotr_amd.modules.ms_deform_attn as mod
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    frames = [torch.from_numpy(frame_pixels(i)) for i in range(8)]
    streams = [encode_jpeg(f, quality=90, subsampling="4:2:0") for f in frames]
    raw_size = (96, 160)
    torch.manual_seed(4)
    model = build_memotr_cuda().eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, mod.MSDeformAttn):
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)

    def tracker(result_score_thresh):
        t = SequenceTracker(model, det_score_thresh=0.5, track_score_thresh=0.0, miss_tolerance=5, use_dab=True,
                            result_score_thresh=result_score_thresh, area_thresh=0, raw_size=raw_size)
        with torch.no_grad():   # random-init scores sit near 0.01: give birth to the three best detections of frame 0
            frame = preprocess_frames(frames[0].cuda(), size=target_size(48, 80, *raw_size))
            res = model(frame=frame, tracks=t.tracks)
            best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
        t.tracker.det_score_thresh = float(best.topk(3).values[-1]) - 1e-6
        return t

    def lines_of(results, t):
        return [line for idx, result in results for line in t.mot_lines(idx, result)]

    t = tracker(0.0)
    results = list(t.track(frames))
    every = lines_of(results, t)
    top = torch.cat([r.scores.max(-1).values for _, r in results])
    assert len(every) == len(top) >= 6
    thresh = float(top.median())

    t = tracker(thresh)
    want = lines_of(t.track(frames), t)
    assert 0 < len(want) < len(every)

    log = ResultLog("cuda", capacity=4)                       # (grows on the way)
    assert tracker(thresh).track_logged(frames, log) == 8
    assert log.mot_lines("DanceTrack") == want

    t = tracker(thresh)
    want_jpeg = lines_of(t.track_jpeg(streams), t)
    assert want_jpeg
    log.reset()
    assert tracker(thresh).track_logged(streams, log) == 8
    assert log.mot_lines("DanceTrack") == want_jpeg
    assert tracker(thresh).track_logged([], log) == 0
