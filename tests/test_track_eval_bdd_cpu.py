"""CPU: the host statement of the BDD100K evaluation (memotr_amd/evaluation_bdd100k.py) against what TrackEval's
BDD100K code produced (tests/golden/trackeval_bdd100k.npz, tests/golden/gen_golden_track_eval_bdd.py): similarities
bit for bit, preprocessed ids and every integer field exactly, float fields within 1e-9, the class-combined keys
included; the summary lines, the label map, the evaluator fed from ``bdd_frame_result`` records through files, the
errors, and the C ABI of libtrack_eval_bdd_hip.so without a device."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header
from track_eval_bdd_helpers import check_results, check_tables, golden

from memotr_amd import evaluation as E
from memotr_amd import evaluation_bdd100k as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bdd_lib():
    from memotr_amd.build import build_track_eval_bdd_lib
    build_track_eval_bdd_lib()
    from memotr_amd import _track_eval_bdd_lib
    return _track_eval_bdd_lib


@pytest.fixture(scope="module")
def host_result():
    g, packed = golden()
    return B.evaluate_packed_bdd(packed, device="cpu")


def test_host_statement_equals_trackeval(host_result):
    g, packed = golden()
    check_tables(B.host_tables_bdd(packed), g)
    print("largest float difference", check_results(host_result, g, packed.names))


def test_fixture_covers_the_edges():
    g, p = golden()
    assert p.names == ["edges", "wide_65x7", "tall_70x9", "regions_70", "walk37", "walk41", "one_frame", "no_tracker",
                       "no_gt"]
    split = B.class_split_host(p)
    n_gt, n_tr, n_ig = np.diff(split["gt_off"]), np.diff(split["tr_off"]), np.diff(p.ig_off)
    assert ((n_tr == 65) & (n_gt == 7)).any() and ((n_gt == 70) & (n_tr == 9)).any() and (n_ig == 70).any()
    assert ((n_gt == 0) & (n_tr > 0)).any() and ((n_tr == 0) & (n_gt > 0)).any() and (n_ig == 0).any()
    assert (g["raw_similarity"] == 0.5).any() and (g["raw_similarity"] == 1.0).any()
    assert len(g["pre::tr_ids"]) < int(np.isin(p.tr_classes, B.CLASS_IDS).sum())        # regions removed detections
    assert len(g["pre::gt_ids"]) == int(np.isin(p.gt_classes, B.CLASS_IDS).sum())       # nothing leaves the ground truth
    assert set(p.gt_classes.tolist()) | set(p.tr_classes.tolist()) == set(B.CLASS_IDS)  # all 8 classes, no other id
    dets = g["pre::n_gt_dets"].reshape(-1, 8), g["pre::n_tr_dets"].reshape(-1, 8)
    e = p.names.index("edges")
    bus, moto, train = (B.CLASSES.index(c) for c in ("bus", "motorcycle", "train"))
    assert dets[0][e, bus] > 0 and dets[1][e, bus] == 0 and dets[0][e, moto] == 0 and dets[1][e, moto] > 0
    assert dets[0][e, train] == 0 and dets[1][e, train] == 0
    assert (dets[1][p.names.index("no_tracker")] == 0).all() and (dets[0][p.names.index("no_gt")] == 0).all()
    # the edges the hand-made frames are there for: intersection over area exactly 0.5 (kept), 1 (removed),
    # a matched detection inside a region and a detection without area (both kept)
    f = slice(p.seq_off[e], p.seq_off[e + 1])
    ioa = [B.box_ioa_x0y0x1y1(p.tr_boxes[p.tr_off[q]:p.tr_off[q + 1]], p.ig_boxes[p.ig_off[q]:p.ig_off[q + 1]])
           for q in range(f.start, f.stop)]
    values = np.concatenate([x.reshape(-1) for x in ioa])
    assert (values == 0.5).any() and (values == 1.0).any() and ((values > 0.5) & (values < 1)).any()
    # a tracker id under two classes
    by_id = {}
    for i, c in zip(p.tr_ids.tolist(), p.tr_classes.tolist()):
        by_id.setdefault(i, set()).add(c)
    assert any(len(v) > 1 for v in by_id.values())


def test_edge_frames_keep_and_remove_what_the_rules_say():
    g, p = golden()
    e = p.names.index("edges")
    t = B.host_tables_bdd(p.select(e))
    T = int(p.seq_off[e + 1] - p.seq_off[e])
    kept = np.diff(t["tr_off"]).reshape(8, T)                   # detections left per (class, frame)
    ped, rider, car = (B.CLASSES.index(c) for c in ("pedestrian", "rider", "car"))
    assert kept[car, 0] == 0                                    # inside a Crowd row, unmatched: removed
    assert kept[car, 1] == 1                                    # 0.5 of it inside a trailer: kept; 0.55: removed
    assert kept[car, 2] == 2                                    # matched inside a region; no area: kept
    assert kept[ped, 5] == 0 and kept[rider, 5] == 1            # no ground truth: the regions still apply
    assert kept[ped, 0] == 2 and kept[ped, 6] == 2


def test_iou_and_ioa_follow_the_corner_form():
    a = np.array([[0.0, 0, 10, 10], [0.1, 0.2, 0.1 + 1e-9, 0.7], [5, 5, 5, 9], [1e8 + 0.1, 3, 1e8 + 7.3, 11.7]])
    b = np.array([[0.0, 0, 10, 5], [0.1, 0.2, 0.30000000000000004, 0.7], [1e8, 0, 1e8 + 5, 9]])
    iou, ioa = B.box_iou_x0y0x1y1(a, b), B.box_ioa_x0y0x1y1(a, b)
    assert iou[0, 0] == 0.5 and ioa[0, 0] == 0.5 and (iou[2] == 0).all() and (ioa[2] == 0).all()
    assert B.box_ioa_x0y0x1y1(b, a)[0, 0] == 1.0                # over the FIRST argument's area
    # the operation order, entry by entry: areas from the corners as they are, union = area + area - intersection
    rng = np.random.RandomState(0)
    c = rng.uniform(0, 100, (40, 2))
    c = np.concatenate([c, c + rng.uniform(5, 60, (40, 2))], 1)
    got_iou, got_ioa = B.box_iou_x0y0x1y1(c[:25], c[25:]), B.box_ioa_x0y0x1y1(c[:25], c[25:])
    for i, p in enumerate(c[:25]):
        for j, q in enumerate(c[25:]):
            inter = max(min(p[2], q[2]) - max(p[0], q[0]), 0) * max(min(p[3], q[3]) - max(p[1], q[1]), 0)
            area_p, area_q = (p[2] - p[0]) * (p[3] - p[1]), (q[2] - q[0]) * (q[3] - q[1])
            assert got_iou[i, j] == inter / (area_p + area_q - inter) and got_ioa[i, j] == inter / area_p
    assert (got_iou > 0).any()
    assert iou.shape == (4, 3) and B.box_iou_x0y0x1y1(a[:0], b).shape == (0, 3) and B.box_ioa_x0y0x1y1(a, b[:0]).shape == (4, 0)


def test_summary_has_the_names_order_and_values_of_the_summary_files(host_result):
    g, _ = golden()
    s = B.bdd_summary(host_result)
    assert list(s) == list(B.CLASSES + B.COMBINED_KEYS)
    assert [str(k) for k in g["summary_keys"]] == ["cls_comb_cls_av", "cls_comb_det_av", "car", "HUMAN"]
    for key, names, values in zip(g["summary_keys"], g["summary_names"], g["summary_values"]):
        mine = s[str(key)]
        assert list(mine) == [str(n) for n in names] == list(E.SUMMARY_FIELDS)
        for k, v in zip(mine, values):
            assert mine[k] == float(v), (key, k, mine[k], v)
            assert isinstance(mine[k], int) == (k in E.INT_FIELDS)


def test_class_combinations():
    _, packed = golden()
    comb = B.evaluate_packed_bdd(packed.select(packed.names.index("edges")))["COMBINED_SEQ"]
    per_class = [comb[c] for c in B.CLASSES]
    av, det = comb["cls_comb_cls_av"], comb["cls_comb_det_av"]
    train = comb["train"]                                       # absent everywhere: the fixed values, averaged in
    assert train["Dets"] == train["GT_Dets"] == 0 and (train["LocA"] == 1).all() and train["HOTA(0)"] == 0
    assert comb["bus"]["CLR_FN"] == comb["bus"]["GT_Dets"] > 0 and comb["motorcycle"]["CLR_FP"] > 0
    assert np.allclose(av["LocA"], np.mean([c["LocA"] for c in per_class], axis=0), rtol=0, atol=1e-15)
    assert av["MOTA"] == np.mean([c["MOTA"] for c in per_class]) and av["MOTP_sum"] == np.mean([c["MOTP_sum"] for c in per_class])
    for k in ("CLR_TP", "IDSW", "IDTP", "Dets", "GT_IDs", "CLR_Frames"):
        assert av[k] == det[k] == sum(c[k] for c in per_class), k
    assert det["MOTP_sum"] == sum(c["MOTP_sum"] for c in per_class)
    human = comb["HUMAN"]
    assert human["CLR_TP"] == comb["pedestrian"]["CLR_TP"] + comb["rider"]["CLR_TP"]
    assert comb["VEHICLE"]["Dets"] == sum(comb[c]["Dets"] for c in ("car", "truck", "bus", "train"))
    assert "all" not in comb


def test_label_index_to_category_to_class_id():
    from memotr_amd.inference import BDD_CLS2LABEL
    assert B.CLASSES == ("pedestrian", "rider", "car", "bus", "truck", "train", "motorcycle", "bicycle")
    assert B.CLASS_IDS == (1, 2, 4, 5, 6, 7, 10, 11)
    assert B.LABEL_TO_CATEGORY == tuple(BDD_CLS2LABEL[k + 1] for k in range(8))
    assert B.LABEL_TO_CATEGORY == ("pedestrian", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")
    assert B.LABEL_TO_CLASS_ID == (1, 2, 4, 6, 5, 7, 10, 11)    # truck / bus: the model's order is not TrackEval's
    assert sorted(B.LABEL_TO_CLASS_ID) == sorted(B.CLASS_IDS)
    assert [B.CLASS_NAME_TO_CLASS_ID[c] for c in B.DISTRACTOR_CATEGORIES] == [3, 8, 9]
    assert sorted(c for m in B.SUPER_CATEGORIES.values() for c in m) == sorted(B.CLASSES)


class Result:
    """What SequenceTracker reports: ids, label indices and xyxy boxes (float32, as ``_report`` makes them)."""

    def __init__(self, ids, labels, boxes):
        self.ids, self.labels = torch.as_tensor(ids), torch.as_tensor(labels)
        self.boxes = torch.as_tensor(boxes, dtype=torch.float32)


def tracked(seed, n_frames=6):
    rng = np.random.RandomState(seed)
    out = []
    for t in range(n_frames):
        n = rng.randint(0, 6)
        xy = rng.uniform(0, 500, (n, 2)).astype(np.float32)
        out.append(Result(rng.permutation(9)[:n], rng.randint(0, 8, n),
                          np.concatenate([xy, xy + rng.uniform(20, 90, (n, 2)).astype(np.float32)], 1)))
    return out


def write_files(tmp_path, by_seq, key):
    """Tracker files from ``bdd_frame_result`` records (its ``frameIndex`` renamed where ``key`` is ``index``), frames
    in reverse order; ground truth: the same boxes moved a little under other ids, a trailer and a Crowd row added."""
    from memotr_amd.inference import SequenceTracker
    gt_dir, tracker_dir = tmp_path / "gt", tmp_path / "tracker"
    gt_dir.mkdir()
    tracker_dir.mkdir()
    for seq, results in by_seq.items():
        records, truth = [], []
        for t, r in enumerate(results):
            rec = SequenceTracker.bdd_frame_result(t, r, f"videos/{seq}/{seq}-{t + 1:07d}.jpg")
            assert rec["frameIndex"] == t and all(isinstance(a["id"], str) for a in rec["labels"])
            labels = [{"id": int(a["id"]) + 100, "category": a["category"],
                       "box2d": dict(a["box2d"], x1=a["box2d"]["x1"] + 1.5), "attributes": {"Crowd": False}}
                      for a in rec["labels"]]
            labels.append({"id": 900, "category": "trailer", "box2d": {"x1": 600.0, "y1": 0.0, "x2": 700.0, "y2": 90.0}})
            labels.append({"id": 901, "category": "car", "box2d": {"x1": 700.0, "y1": 0.0, "x2": 800.0, "y2": 90.0},
                           "attributes": {"Crowd": True}})
            truth.append({"name": rec["name"], key: t, "labels": labels})
            rec["labels"].append({"id": "77", "category": "car",       # a false positive inside the Crowd row: removed
                                  "box2d": {"x1": 710.0, "y1": 5.0, "x2": 790.0, "y2": 80.0}})
            rec[key] = rec.pop("frameIndex")
            records.append(rec)
        (tracker_dir / f"{seq}.json").write_text(json.dumps(records[::-1]))
        (gt_dir / f"{seq}.json").write_text(json.dumps(truth))
    return str(gt_dir), str(tracker_dir)


@pytest.mark.parametrize("key", ["frameIndex", "index"])
def test_evaluate_bdd_files_equals_the_evaluator_fed_in_memory(tmp_path, key):
    by_seq = {"seq_a": tracked(5, 7), "seq_b": tracked(6, 4)}
    gt_dir, tracker_dir = write_files(tmp_path, by_seq, key)
    res = B.evaluate_bdd_files(gt_dir, tracker_dir)
    assert list(res) == ["seq_a", "seq_b", "COMBINED_SEQ"]
    ev = B.BDD100KEvaluator()
    for seq, results in by_seq.items():
        for t, r in enumerate(results):
            ev.add_frame(seq, t, Result(r.ids.tolist() + [77], r.labels.tolist() + [2],
                                        r.boxes.tolist() + [[710.0, 5.0, 790.0, 80.0]]))
            boxes = [[x1 + 1.5, y1, x2, y2] for x1, y1, x2, y2 in r.boxes.tolist()]
            ev.add_ground_truth(seq, t, [i + 100 for i in r.ids.tolist()] + [900, 901],
                                boxes + [[600.0, 0, 700, 90], [700.0, 0, 800, 90]],
                                [B.LABEL_TO_CATEGORY[k] for k in r.labels.tolist()] + ["trailer", "car"],
                                [False] * len(r.ids) + [False, True])
    want = ev.evaluate()
    for name in res:
        for cls in res[name]:
            for k in res[name][cls]:
                assert np.array_equal(res[name][cls][k], want[name][cls][k]), (name, cls, k)
    c = res["COMBINED_SEQ"]["cls_comb_det_av"]
    n = sum(len(r.ids) for rs in by_seq.values() for r in rs)
    assert c["CLR_TP"] == c["GT_Dets"] == c["Dets"] == n > 0    # id 77 is gone
    assert 0 < c["CLR_Frames"] <= 11 * 8                        # (CLEAR counts no frames for a pair with an empty side)
    assert c["IDSW"] == 0 and c["MOTA"] == 1.0 and 0.5 < c["MOTP"] < 1.0
    assert res["COMBINED_SEQ"]["car"]["Dets"] == sum(int((r.labels == 2).sum()) for rs in by_seq.values() for r in rs)


def test_evaluator_rejects_what_trackeval_rejects(tmp_path):
    box = [[0.0, 0, 1, 1], [2.0, 2, 3, 3]]
    ev = B.BDD100KEvaluator()
    ev.add_ground_truth("s", 0, [4, 4], box, ["car", "car"])
    with pytest.raises(ValueError, match="more than once in class car"):
        ev.evaluate()
    ev = B.BDD100KEvaluator()                                   # the same id under two classes of one frame is fine
    ev.add_ground_truth("s", 0, [4, 5], box, ["car", "bus"])
    ev.add_tracker_rows("s", 0, [4, 4], box, ["car", "truck"])
    assert ev.evaluate()["s"]["car"]["CLR_TP"] == 1
    ev.add_tracker_rows("s", 1, [4, 4], box, [4, 4])
    with pytest.raises(ValueError, match="tracker id occurs more than once"):
        ev.evaluate()
    with pytest.raises(ValueError, match="unknown category 'tram'"):
        B.BDD100KEvaluator().add_ground_truth("s", 0, [1], box[:1], ["tram"])
    with pytest.raises(ValueError, match="unknown class id"):
        B.BDD100KEvaluator().add_tracker_rows("s", 0, [1], box[:1], [12])
    ev = B.BDD100KEvaluator()
    ev.add_ground_truth("s", 0, [2 ** 31], box[:1], ["car"])
    with pytest.raises(ValueError, match="outside"):
        ev.evaluate()
    ev = B.BDD100KEvaluator()
    ev.add_ground_truth("s", 3, [4], box[:1], ["car"])
    ev.set_length("s", 2)
    with pytest.raises(ValueError, match="outside 0 .. 1"):
        ev.evaluate()
    # files: unequal frame counts
    gt_dir, tracker_dir = tmp_path / "gt", tmp_path / "tr"
    gt_dir.mkdir()
    tracker_dir.mkdir()
    (gt_dir / "v.json").write_text(json.dumps([{"index": 0, "labels": []}, {"index": 1, "labels": []}]))
    (tracker_dir / "v.json").write_text(json.dumps([{"index": 0, "labels": []}]))
    with pytest.raises(ValueError, match="do not match"):
        B.evaluate_bdd_files(str(gt_dir), str(tracker_dir))


def test_the_default_device_is_the_host_statement():
    _, packed = golden()
    one = packed.select(packed.names.index("one_frame"))
    a, b = B.evaluate_packed_bdd(one), B.evaluate_packed_bdd(one, device="cpu")
    assert all(np.array_equal(a["one_frame"][c][k], b["one_frame"][c][k]) for c in B.CLASSES for k in a["one_frame"][c])


# ------------------------------------------------------------------------------------------------------- the C ABI
def header():
    return open(os.path.join(ROOT, "include", "track_eval_bdd_hip.h")).read()


def test_library_exports_every_declared_symbol(bdd_lib):
    syms = assert_binding_matches_header(bdd_lib, "track_eval_bdd_hip.h", "bddeval", "BDDEVAL_ABI_VERSION")
    assert len(syms) == 6
    assert int(re.search(r"#define BDDEVAL_N_CLASSES (\d+)", header()).group(1)) == bdd_lib.N_CLASSES == len(B.CLASSES)
    assert "#define BDDEVAL_MAX_DIM TRACKEVAL_MAX_DIM" in header()
    from memotr_amd import _track_eval_lib
    assert bdd_lib.MAX_DIM == _track_eval_lib.MAX_DIM


def test_argument_errors_are_reported_without_a_device(bdd_lib):
    lib = bdd_lib.lib
    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch
    err = lib.bddeval_last_error
    calls = {
        "bddeval_class_count": lambda n=3, a=p: lib.bddeval_class_count(a, p, p, p, p, p, n, p, p, None),
        "bddeval_class_split": lambda n=3, a=p: lib.bddeval_class_split(a, p, p, p, p, p, p, p, p, p, n, p, p, p, p, p, p,
                                                                       None),
        "bddeval_similarity": lambda n=3, a=p: lib.bddeval_similarity(a, p, p, p, p, n, p, None),
        "bddeval_preproc": lambda n=3, a=p, g=5, k=5: lib.bddeval_preproc(a, p, p, p, p, p, p, p, n, g, k, p, p, None),
    }
    for name, call in calls.items():
        assert call(a=None) == 1 and b"null pointer" in err() and name.encode() in err(), name
        assert call(n=-1) == 1 and b"negative" in err() and name.encode() in err(), name
        assert call(n=0) == 0 and err() == b"", name             # an empty call launches nothing and clears the text
    assert calls["bddeval_class_count"](n=2 ** 31 // 8 + 1) == 2 and b"exceed" in err()
    assert calls["bddeval_preproc"](g=2049) == 2 and b"exceeds BDDEVAL_MAX_DIM = 2048" in err() and b"2049" in err()
    assert calls["bddeval_preproc"](k=2049) == 2 and b"BDDEVAL_MAX_DIM" in err()
    assert calls["bddeval_preproc"](g=-1) == 1 and b"negative" in err()
    with pytest.raises(RuntimeError, match="null pointer"):
        bdd_lib.check(calls["bddeval_similarity"](a=None), "bddeval_similarity")
