"""GPU: the evaluation kernels (memotr_amd/csrc/track_eval.hip) against what TrackEval produced for the fixtures
(same bars as tests/test_track_eval_cpu.py: similarities, ids and integer fields exact, float fields within 1e-9) and
against the host statement on sequences that are not in the fixtures; the same bits on every run, for every grouping
of the sequences into calls and on any stream; and the evaluator fed by SequenceTracker."""
import numpy as np
import pytest
import torch

from model_helpers import TinyBackbone, small_config
from track_eval_helpers import FLOAT_BAR, SETS, check_results, check_tables, golden

from memotr_amd import evaluation as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def track_eval_lib():
    from memotr_amd.build import build_track_eval_lib
    build_track_eval_lib()
    from memotr_amd import _track_eval_lib
    return _track_eval_lib


@pytest.fixture(scope="module")
def frame_lib():
    from memotr_amd.build import build_frame_lib
    build_frame_lib()
    from memotr_amd import _frame_lib
    return _frame_lib


def host_of(tables):
    return {k: v.cpu().numpy() for k, v in tables.items()}


@pytest.fixture(scope="module")
def random_set():
    """Three sequences of different lengths and densities that are not in the fixtures, and their host tables.  Like
    the fixtures they must not depend on the order HOTA's alignment sums are formed in: checked here the same way, on
    the host statement with the frames reversed."""
    S = E.synthetic_sequence
    seqs = {"a": S(101, 70, 14, n_distractors=3, zero_marked=0.05), "b": S(102, 9, 30, n_false=4, switch=0.1),
            "c": S(103, 131, 6, miss=0.3, gap=0.1)}
    packed = E.pack_sequences(seqs)
    tables = E.host_tables(packed)
    backwards = E.host_tables(E.pack_sequences({n: {k: v[::-1] for k, v in s.items()} for n, s in seqs.items()}))
    assert np.array_equal(tables["hota_tp"], backwards["hota_tp"])
    return packed, tables


@pytest.mark.parametrize("name", sorted(SETS))
def test_kernels_equal_trackeval_on_the_fixtures(track_eval_lib, name):
    g, packed = golden(name)
    dev = packed.to("cuda")
    check_tables(host_of(E.device_tables(dev, SETS[name])), g)
    res = E.evaluate_packed(dev, SETS[name], device="cuda")
    assert list(res) == packed.names + ["COMBINED_SEQ"]
    print("largest float difference", check_results(res, g, packed.names))


def test_kernels_equal_the_host_statement_on_a_random_set(track_eval_lib, random_set):
    packed, want = random_set
    got = host_of(E.device_tables(packed.to("cuda")))
    live = (want["n_gt_dets"] > 0) & (want["n_tr_dets"] > 0)
    assert live.all()
    for k in ("raw_similarity", "similarity", "gt_off", "tr_off", "gt_ids", "tr_ids", "n_gt_ids", "n_tr_ids",
              "n_gt_dets", "n_tr_dets", "hota_tp", "clear_ints", "identity"):
        assert np.array_equal(got[k], want[k]), k
    a, b = E.evaluate_packed(packed.to("cuda"), device="cuda"), E.evaluate_packed(packed, device="cpu")
    worst = 0.0
    for name in a:
        for k in a[name]:
            diff = float(np.max(np.abs(np.asarray(a[name][k], np.float64) - np.asarray(b[name][k], np.float64))))
            worst = max(worst, diff)
            assert diff <= (0 if k in E.INT_FIELDS + E.HOTA_INT_ARRAYS else FLOAT_BAR), (name, k, diff)
    print("largest float difference", worst)


def test_two_runs_give_the_same_bits(track_eval_lib, random_set):
    dev = random_set[0].to("cuda")
    a, b = E.device_tables(dev), E.device_tables(dev)
    assert sorted(a) == sorted(b) and "matches" in a and "alignment" in a
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_one_call_equals_a_call_per_sequence(track_eval_lib, random_set):
    packed = random_set[0]
    together = E.evaluate_packed(packed.to("cuda"), device="cuda")
    for i, name in enumerate(packed.names):
        alone = E.evaluate_packed(packed.select(i).to("cuda"), device="cuda")[name]
        for k in alone:
            assert np.array_equal(alone[k], together[name][k]), (name, k)


def test_a_call_on_another_stream(track_eval_lib, random_set):
    dev = random_set[0].to("cuda")
    want = E.device_tables(dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    got = E.device_tables(dev, stream=stream)
    stream.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k]), k
        got[k].record_stream(stream)


def test_problems_beyond_the_cap_are_errors(track_eval_lib):
    def crowd(n_gt, n_tr):
        grid = lambda n: np.stack([np.arange(n) * 30.0, np.zeros(n), np.full(n, 20.0), np.full(n, 20.0)], 1)  # noqa: E731
        return E.pack_sequences({"s": {"gt_ids": [np.arange(n_gt)], "gt_boxes": [grid(n_gt)],
                                       "tracker_ids": [np.arange(n_tr)], "tracker_boxes": [grid(n_tr)]}}).to("cuda")
    with pytest.raises(ValueError, match="2200 ground-truth plus tracker ids"):
        E.evaluate_packed(crowd(1100, 1100), device="cuda")
    with pytest.raises(RuntimeError, match="exceeds TRACKEVAL_MAX_DIM = 2048"):
        E.evaluate_packed(crowd(2049, 3), device="cuda")
    res = E.evaluate_packed(crowd(700, 740), device="cuda")["s"]               # under the cap, beyond 64 KiB of LDS: evaluated
    assert res["IDTP"] == res["CLR_TP"] == 700 and res["IDFP"] == 40 and res["HOTA_TP"][-1] == 700


def build_memotr_cuda(hidden=256, ffn=256):
    from memotr_amd.models.backbone import BackboneWithPE
    from memotr_amd.models.deformable_transformer import build as build_tr
    from memotr_amd.models.memotr import MeMOTR
    from memotr_amd.models.position_embedding import build as build_pe
    from memotr_amd.models.query_updater import build as build_qu
    cfg = small_config()
    cfg.update(HIDDEN_DIM=hidden, FFN_DIM=ffn, NUM_ENC_LAYERS=2, NUM_DEC_LAYERS=2)
    model = MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=1, n_det_queries=cfg["NUM_DET_QUERIES"],
                   n_feature_levels=4, hidden_dim=hidden, ffn_dim=ffn, dropout=0.0, use_dab=True)
    return model.cuda()


def test_evaluator_fed_by_sequence_tracker(track_eval_lib, frame_lib, hip_lib, clip_lib, monkeypatch):
    """Two frames of online tracking, the tracker's own output as ground truth: everything is found under its id."""
    from memotr_amd.inference import SequenceTracker
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "0")
    torch.manual_seed(4)
    tracker = SequenceTracker(build_memotr_cuda().eval(), det_score_thresh=0.0, track_score_thresh=0.0,
                              result_score_thresh=0.0, miss_tolerance=5, use_dab=True, area_thresh=0,
                              raw_size=(192, 320))
    g = torch.Generator().manual_seed(40)
    frames = [torch.randint(0, 256, (150, 200, 3), dtype=torch.uint8, generator=g) for _ in range(2)]
    ev = E.TrackingEvaluator(device="cuda")
    n = 0
    for frame_idx, result in tracker.track(frames, bgr=True):
        tracker.tracker.det_score_thresh = 2.0                  # births on the first frame only
        ev.add_frame("clip", frame_idx, result)
        boxes = [[x1, y1, x2 - x1, y2 - y1] for x1, y1, x2, y2 in result.boxes.tolist()]
        ev.add_ground_truth("clip", frame_idx + 1, result.ids.tolist(), boxes)
        n += len(result)
    res = ev.evaluate()
    assert list(res) == ["clip", "COMBINED_SEQ"] and n >= 4
    c = res["COMBINED_SEQ"]
    assert c["CLR_TP"] == c["IDTP"] == c["GT_Dets"] == c["Dets"] == n and c["CLR_Frames"] == 2
    assert c["MOTA"] == 1.0 and c["IDF1"] == 1.0 and c["HOTA(0)"] == 1.0 and c["IDSW"] == 0
