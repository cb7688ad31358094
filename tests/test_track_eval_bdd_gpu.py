"""GPU: the BDD100K evaluation on the device (memotr_amd/csrc/track_eval_bdd.hip in front of the metric kernels of
track_eval.hip) against what TrackEval produced for the fixture (same bars as tests/test_track_eval_bdd_cpu.py:
similarities, ids and integer fields exact, float fields within 1e-9) and against the host statement on a multi-class
set that is not in the fixture; the same bits on every run, for every grouping of the sequences into calls and on any
stream; mostly-empty classes at S * 8 scale; the identity cap; and the evaluator fed by SequenceTracker."""
import numpy as np
import pytest
import torch

from model_helpers import TinyBackbone, small_config
from track_eval_bdd_helpers import check_results, check_tables, golden, same_results
from track_eval_helpers import FLOAT_BAR

from memotr_amd import evaluation_bdd100k as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bdd_lib():
    from memotr_amd.build import build_track_eval_bdd_lib, build_track_eval_lib
    build_track_eval_lib()
    build_track_eval_bdd_lib()
    from memotr_amd import _track_eval_bdd_lib
    return _track_eval_bdd_lib


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
    """Three multi-class sequences of different lengths and densities that are not in the fixture, and their host
    tables.  Like the fixture they must not depend on the order HOTA's alignment sums are formed in: checked here the
    same way, on the host statement with the frames reversed."""
    S = B.synthetic_bdd_sequence
    seqs = {"a": S(101, 40, 30, n_false=3, n_regions=3), "b": S(102, 9, 40, n_false=6, switch=0.1, n_classes=3),
            "c": S(103, 67, 12, miss=0.3, gap=0.1, n_regions=1)}
    packed = B.pack_bdd(seqs)
    tables = B.host_tables_bdd(packed)
    backwards = B.host_tables_bdd(B.pack_bdd({n: {k: v[::-1] for k, v in s.items()} for n, s in seqs.items()}))
    assert np.array_equal(tables["hota_tp"], backwards["hota_tp"])
    return packed, tables


def test_kernels_equal_trackeval_on_the_fixture(bdd_lib):
    g, packed = golden()
    dev = packed.to("cuda")
    check_tables(host_of(B.device_tables_bdd(dev)), g)
    res = B.evaluate_packed_bdd(dev, device="cuda")
    print("largest float difference", check_results(res, g, packed.names))


def test_class_split_is_stable_and_complete(bdd_lib):
    _, packed = golden()
    want, got = B.class_split_host(packed), host_of(B.device_tables_bdd(packed.to("cuda")))
    for k in ("gt_off", "tr_off", "gt_ids", "tr_ids", "gt_boxes", "tr_boxes"):
        assert np.array_equal(got["split_" + k], want[k]), k


def test_kernels_equal_the_host_statement_on_a_random_set(bdd_lib, random_set):
    packed, want = random_set
    got = host_of(B.device_tables_bdd(packed.to("cuda")))
    live = (want["n_gt_dets"] > 0) & (want["n_tr_dets"] > 0)
    assert live.sum() >= 16 and not live.all()                   # sequence b has 3 classes only
    assert len(want["tr_ids"]) < int(np.isin(packed.tr_classes, B.CLASS_IDS).sum())      # regions removed detections
    for k in ("raw_similarity", "similarity") + B.TABLE_KEYS:
        assert np.array_equal(got[k], want[k]), k
    for k in ("hota_tp", "clear_ints", "identity"):              # (an empty side: fixed by the counts, not by these)
        assert np.array_equal(got[k][live], want[k][live]), k
    a, b = B.evaluate_packed_bdd(packed.to("cuda"), device="cuda"), B.evaluate_packed_bdd(packed, device="cpu")
    print("largest float difference", same_results(a, b, FLOAT_BAR))


def test_two_runs_give_the_same_bits(bdd_lib, random_set):
    dev = random_set[0].to("cuda")
    a, b = B.device_tables_bdd(dev), B.device_tables_bdd(dev)
    assert sorted(a) == sorted(b) and "matches" in a and "alignment" in a and "tr_remove" in a
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_one_call_equals_a_call_per_sequence(bdd_lib, random_set):
    packed = random_set[0]
    together = B.evaluate_packed_bdd(packed.to("cuda"), device="cuda")
    for i, name in enumerate(packed.names):
        alone = B.evaluate_packed_bdd(packed.select(i).to("cuda"), device="cuda")[name]
        for cls in alone:
            for k in alone[cls]:
                assert np.array_equal(alone[cls][k], together[name][cls][k]), (name, cls, k)


def test_a_call_on_another_stream(bdd_lib, random_set):
    dev = random_set[0].to("cuda")
    want = B.device_tables_bdd(dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    got = B.device_tables_bdd(dev, stream=stream)
    stream.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k]), k
        got[k].record_stream(stream)


def test_seven_of_eight_classes_empty_in_every_sequence(bdd_lib):
    """Most (sequence, class) pairs of real data are empty: 12 sequences of one class each are 96 problems of which
    84 have nothing on either side.  They evaluate, and carry the fixed values into the class average."""
    seqs = {f"s{i}": B.synthetic_bdd_sequence(200 + i, 5 + i, 4, n_classes=1, n_regions=1) for i in range(12)}
    packed = B.pack_bdd(seqs)
    assert set(packed.gt_classes.tolist()) == set(packed.tr_classes.tolist()) == {1}
    got, want = B.evaluate_packed_bdd(packed.to("cuda"), device="cuda"), B.evaluate_packed_bdd(packed, device="cpu")
    same_results(got, want, FLOAT_BAR)
    comb = got["COMBINED_SEQ"]
    for cls in B.CLASSES[1:]:
        c = comb[cls]
        assert c["Dets"] == c["GT_Dets"] == c["CLR_TP"] == c["CLR_FN"] == c["CLR_FP"] == c["IDTP"] == 0, cls
        assert (c["LocA"] == 1).all() and (c["HOTA"] == 0).all() and c["MOTA"] == 0 and c["CLR_Frames"] == 0, cls
        assert all(got[n][cls]["MLR"] == 1.0 and got[n][cls]["LocA(0)"] == 1.0 for n in seqs), cls
    ped, av = comb["pedestrian"], comb["cls_comb_cls_av"]
    assert ped["CLR_TP"] > 0 and av["CLR_TP"] == ped["CLR_TP"]
    assert av["MOTA"] == np.mean([ped["MOTA"]] + [0.0] * 7) and av["LocA(0)"] == np.mean([ped["LocA(0)"]] + [1.0] * 7)
    assert comb["cls_comb_det_av"]["MOTA"] == ped["MOTA"] and comb["BIKE"]["Dets"] == 0


def test_ids_beyond_the_cap_in_one_class_are_an_error_naming_it(bdd_lib):
    n = 1100
    grid = np.stack([np.arange(n) * 30.0, np.zeros(n), np.arange(n) * 30.0 + 20, np.full(n, 20.0)], 1)
    one = lambda cls: {"gt_ids": [np.arange(n)], "gt_boxes": [grid], "gt_classes": [np.full(n, cls)],      # noqa: E731
                       "tracker_ids": [np.arange(n)], "tracker_boxes": [grid], "tracker_classes": [np.full(n, cls)]}
    small = {"gt_ids": [np.arange(3)], "gt_boxes": [grid[:3]], "gt_classes": [np.full(3, 4)],
             "tracker_ids": [np.arange(3)], "tracker_boxes": [grid[:3]], "tracker_classes": [np.full(3, 4)]}
    packed = B.pack_bdd({"fine": small, "crowded": one(6)}).to("cuda")
    with pytest.raises(ValueError, match="sequence crowded, class truck: 2200 ground-truth plus tracker ids"):
        B.evaluate_packed_bdd(packed, device="cuda")
    # the same detections spread over two classes stay under the cap and are evaluated
    both = one(6)
    both["gt_classes"] = both["tracker_classes"] = [np.where(np.arange(n) % 2, 6, 5)]
    res = B.evaluate_packed_bdd(B.pack_bdd({"crowded": both}).to("cuda"), device="cuda")["COMBINED_SEQ"]
    assert res["truck"]["IDTP"] == res["bus"]["IDTP"] == n // 2 and res["VEHICLE"]["CLR_TP"] == n


def build_memotr_cuda(hidden=256, ffn=256):
    from memotr_amd.models.backbone import BackboneWithPE
    from memotr_amd.models.deformable_transformer import build as build_tr
    from memotr_amd.models.memotr import MeMOTR
    from memotr_amd.models.position_embedding import build as build_pe
    from memotr_amd.models.query_updater import build as build_qu
    cfg = small_config()
    cfg.update(HIDDEN_DIM=hidden, FFN_DIM=ffn, NUM_ENC_LAYERS=2, NUM_DEC_LAYERS=2)
    model = MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=8, n_det_queries=cfg["NUM_DET_QUERIES"],
                   n_feature_levels=4, hidden_dim=hidden, ffn_dim=ffn, dropout=0.0, use_dab=True)
    return model.cuda()


def test_evaluator_fed_by_sequence_tracker(bdd_lib, frame_lib, hip_lib, clip_lib, monkeypatch):
    """Two frames of online tracking with 8 classes, the tracker's own output as ground truth: everything is found
    under its id, in its class."""
    from memotr_amd.inference import SequenceTracker
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "0")
    torch.manual_seed(4)
    tracker = SequenceTracker(build_memotr_cuda().eval(), dataset_name="BDD100K", det_score_thresh=0.0,
                              track_score_thresh=0.0, result_score_thresh=0.0, miss_tolerance=5, use_dab=True,
                              area_thresh=0, raw_size=(192, 320))
    g = torch.Generator().manual_seed(40)
    frames = [torch.randint(0, 256, (150, 200, 3), dtype=torch.uint8, generator=g) for _ in range(2)]
    ev = B.BDD100KEvaluator(device="cuda")
    n = 0
    for frame_idx, result in tracker.track(frames, bgr=True):
        tracker.tracker.det_score_thresh = 2.0                  # births on the first frame only
        ev.add_frame("clip", frame_idx, result)
        ev.add_ground_truth("clip", frame_idx, result.ids.tolist(), result.boxes.tolist(),
                            [B.LABEL_TO_CATEGORY[k] for k in result.labels.tolist()])
        n += len(result)
    res = ev.evaluate()
    assert list(res) == ["clip", "COMBINED_SEQ"] and n >= 4
    c = res["COMBINED_SEQ"]["cls_comb_det_av"]
    assert c["CLR_TP"] == c["IDTP"] == c["GT_Dets"] == c["Dets"] == n
    assert c["MOTA"] == 1.0 and c["IDF1"] == 1.0 and c["HOTA(0)"] == 1.0 and c["IDSW"] == 0
    assert sum(res["COMBINED_SEQ"][cls]["Dets"] for cls in B.CLASSES) == n
