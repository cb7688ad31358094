"""CPU: the host statement of the BDD100K error analysis (memotr_amd/diagnose_bdd100k.py): the per-class counts
against the evaluator and against what TrackEval's BDD100K code recorded (tests/golden/trackeval_bdd100k.npz), the
cross-class pairs against a brute force over all partial maps, the scripted frames of tests/bdd_events_cases.py, the
confusion matrix's sums, the files and the command line, and the C ABI of the new entry point without a device."""
import ctypes
import os

import numpy as np
import pytest

import bdd_events_cases as C
from cabi_helpers import assert_binding_matches_header
from track_eval_bdd_helpers import golden

from memotr_amd import diagnose as D
from memotr_amd import diagnose_bdd100k as DB
from memotr_amd import evaluation_bdd100k as B


@pytest.fixture(scope="module")
def scripted():
    return DB.bdd_events(C.scripted_pack())


def check_sums(ev):
    """Row g of the confusion matrix sums to the ground-truth detections of class g, column t to the kept tracker
    detections of class t; the diagonal is CLR_TP; [8, 8] is 0."""
    m, labels = ev.confusion()
    assert m.shape == (9, 9) and m.dtype == np.int64 and labels == B.CLASSES + ("none",)
    gc, tc = DB.class_index(ev.gt_classes), DB.class_index(ev.tr_classes)
    assert np.array_equal(m[:8].sum(1), np.bincount(gc[gc >= 0], minlength=8))
    assert np.array_equal(m[:, :8].sum(0), np.bincount(tc[ev.tr_kind != DB.IGNORED], minlength=8))
    assert np.array_equal(np.diag(m)[:8], ev.class_counts[:, 0]) and m[8, 8] == 0
    assert m.sum() - np.trace(m) - m[:8, 8].sum() - m[8, :8].sum() == int((ev.gt_cross_partner >= 0).sum())


def check_counts(events, fields):
    for name, ev in events.items():
        assert ev.class_counts.shape == (8, 5) and ev.class_counts.dtype == np.int32
        for cls, counts in ev.counts().items():
            assert counts == {k: int(fields[name][cls][k]) for k in DB.COUNTS}, (name, cls)
        check_sums(ev)


# ---------------------------------------------------------------------------------------------- the per-class walk
def test_counts_are_the_evaluators():
    plain = B.pack_bdd({f"s{seed}": B.synthetic_bdd_sequence(seed, 40 + seed, 12, n_regions=2 + seed % 2)
                        for seed in (1, 2, 5)})
    events = DB.bdd_events(plain)
    check_counts(events, B.evaluate_packed_bdd(plain))
    assert sum(len(ev.ignored()) for ev in events.values()) > 0
    assert sum(int(ev.class_counts[:, 3].sum()) for ev in events.values()) > 0          # switches, and picked-up tracks
    assert sum(int(ev.class_counts[:, 4].sum()) for ev in events.values()) > 0
    pack, events = C.random_pack()
    check_counts(events, B.evaluate_packed_bdd(pack))
    assert sum(len(ev.confusions(100)) for ev in events.values()) > 0


def test_counts_are_trackevals():
    """The five counts of every (sequence, class) of the fixture recorded from TrackEval's BDD100K code."""
    g, packed = golden()
    events = DB.bdd_events(packed)
    rows = [str(r) for r in g["res_rows"]]
    for name, ev in events.items():
        for c, cls in enumerate(B.CLASSES):
            row = rows.index(f"{name}/{cls}")
            assert ev.class_counts[c].tolist() == [int(g["res::" + k][row]) for k in DB.COUNTS], (name, cls)
        check_sums(ev)
    assert sum(int(ev.class_counts[:, 3].sum()) for ev in events.values()) > 0


def test_rows_agree_with_their_counts_and_partners_point_back():
    for ev in list(C.random_pack()[1].values()) + list(DB.bdd_events(golden()[1]).values()):
        counts, conf = DB._tables_of_rows({k: getattr(ev, k) for k in ev.ARRAYS})
        assert np.array_equal(counts, ev.class_counts) and np.array_equal(conf, ev.confusion_matrix)
        gc, tc = DB.class_index(ev.gt_classes), DB.class_index(ev.tr_classes)
        for f in range(ev.n_frames):
            g0, t0 = int(ev.gt_off[f]), int(ev.tr_off[f])
            for i in range(g0, int(ev.gt_off[f + 1])):
                for partner, back, same_class in ((ev.gt_partner, ev.tr_partner, True),
                                                  (ev.gt_cross_partner, ev.tr_cross_partner, False)):
                    if partner[i] >= 0:
                        j = t0 + int(partner[i])
                        assert j < ev.tr_off[f + 1] and back[j] == i - g0 and (gc[i] == tc[j]) == same_class
                assert (ev.gt_partner[i] >= 0) == (ev.gt_kind[i] in (DB.MATCH, DB.SWITCH))
                assert ev.gt_cross_partner[i] < 0 or ev.gt_kind[i] == DB.MISS
        assert np.array_equal(ev.tr_partner >= 0, np.isin(ev.tr_kind, (DB.MATCH, DB.SWITCH)))
        assert ((ev.tr_cross_partner < 0) | (ev.tr_kind == DB.FP)).all()
        assert np.array_equal(ev.gt_kind == DB.IGNORED, gc < 0)


# ---------------------------------------------------------------------------------------------- the cross-class pass
def test_cross_class_pairs_reach_the_brute_force_optimum():
    _, events = C.random_pack()
    unique = several = 0
    for ev in events.values():
        for f in range(ev.n_frames):
            best, optima = C.brute_force(ev, f)
            pairs = C.cross_pairs(ev, f)
            values = [C.admissible(ev, i, j) for i, j in pairs]
            assert all(v is not None for v in values), (ev.name, f)
            assert abs(sum(values) - best) <= 1e-9, (ev.name, f)
            if len(optima) == 1:
                assert pairs == optima[0], (ev.name, f)
                unique += len(pairs) > 0
            else:
                several += 1
            for i, j in pairs:                      # both sides record the pair, its classes and its IoU
                t0, g0 = int(ev.tr_off[f]), int(ev.gt_off[f])
                assert ev.tr_cross_partner[j] == i - g0
                assert ev.gt_cross_class[i] == DB.class_index(ev.tr_classes[j:j + 1])[0]
                assert ev.tr_cross_class[j] == DB.class_index(ev.gt_classes[i:i + 1])[0]
                assert ev.gt_cross_iou[i] == ev.tr_cross_iou[j] == B.box_iou_x0y0x1y1(ev.gt_boxes[i], ev.tr_boxes[j])[0, 0]
    assert unique > 10


def test_no_pair_of_one_class_is_left_to_find():
    """A MISS and an FP of one class at IoU >= 0.5 cannot both survive that class's assignment."""
    for ev in list(C.random_pack()[1].values()) + list(DB.bdd_events(golden()[1]).values()):
        gc, tc = DB.class_index(ev.gt_classes), DB.class_index(ev.tr_classes)
        for f in range(ev.n_frames):
            g, t = C.candidates(ev, f)
            iou = B.box_iou_x0y0x1y1(ev.gt_boxes[g], ev.tr_boxes[t])
            assert not ((iou >= 0.5 - 1e-12) & (gc[g][:, None] == tc[t][None, :])).any(), (ev.name, f)


# -------------------------------------------------------------------------------------------------- scripted frames
def kinds(ev):
    return ev.gt_kind.tolist(), ev.tr_kind.tolist()


def test_a_car_labelled_truck(scripted):
    ev = scripted["car_as_truck"]
    assert kinds(ev) == ([DB.MISS], [DB.FP])
    assert ev.confusion_matrix[C.CAR, C.TRUCK] == 1 and ev.confusion_matrix.sum() == 1
    assert ev.gt_cross_partner.tolist() == [0] and ev.tr_cross_partner.tolist() == [0]
    assert ev.gt_cross_class.tolist() == [C.TRUCK] and ev.tr_cross_class.tolist() == [C.CAR]
    assert ev.gt_cross_iou.tolist() == ev.tr_cross_iou.tolist() == [0.9]
    assert ev.counts()["car"]["CLR_FN"] == 1 and ev.counts()["truck"]["CLR_FP"] == 1
    assert ev.confusions() == [("car", "truck", 1)] and ev.gt_iou.tolist() == [0.0]


def test_the_threshold_is_half(scripted):
    below, above = scripted["below_half"], scripted["above_half"]
    assert kinds(below) == kinds(above) == ([DB.MISS], [DB.FP])
    assert below.gt_cross_partner.tolist() == [-1] and below.gt_cross_class.tolist() == [-1]
    assert below.gt_cross_iou.tolist() == below.tr_cross_iou.tolist() == [0.0]
    assert below.confusion_matrix[C.CAR, 8] == 1 and below.confusion_matrix[8, C.TRUCK] == 1
    assert above.gt_cross_partner.tolist() == [0] and above.confusion_matrix[C.CAR, C.TRUCK] == 1
    assert 0.5 < above.gt_cross_iou[0] < 0.502


def test_the_larger_iou_wins_and_a_tie_is_scipys(scripted):
    ev = scripted["larger_wins"]
    assert ev.gt_cross_partner.tolist() == [-1, 0] and ev.tr_cross_partner.tolist() == [1]
    assert ev.gt_cross_iou.tolist() == [0.0, 0.875] and ev.tr_cross_class.tolist() == [C.BUS]
    assert ev.confusion_matrix[C.BUS, C.TRUCK] == 1 and ev.confusion_matrix[C.CAR, 8] == 1
    tie = scripted["tie"]
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(-np.full((2, 2), 0.8))
    want = np.full(2, -1)
    want[rows] = cols
    assert tie.gt_cross_partner.tolist() == want.tolist() and sorted(tie.tr_cross_partner.tolist()) == [0, 1]
    assert tie.gt_cross_iou.tolist() == [0.8, 0.8]


def test_ignore_regions_and_other_categories(scripted):
    inside, outside = scripted["inside_region"], scripted["outside_region"]
    assert kinds(inside) == ([DB.MISS], [DB.IGNORED]) and kinds(outside) == ([DB.MISS], [DB.FP])
    assert inside.ignored() == [(0, 7, "truck")] and outside.ignored() == []
    assert inside.counts()["truck"]["CLR_FP"] == 0 and outside.counts()["truck"]["CLR_FP"] == 1
    assert inside.confusion_matrix[8].sum() == 0 and outside.confusion_matrix[8, C.TRUCK] == 1
    over = scripted["region_over_candidate"]                    # IoU 0.9 with a car, but the metric never saw it
    assert kinds(over) == ([DB.MISS], [DB.IGNORED]) and over.gt_cross_partner.tolist() == [-1]
    assert over.tr_cross_partner.tolist() == [-1] and over.confusion_matrix[C.CAR, 8] == 1
    other = scripted["other_category"]
    assert kinds(other) == ([DB.MISS], [DB.IGNORED, DB.FP]) and other.ignored() == [(0, 7, "other vehicle")]
    assert other.gt_cross_partner.tolist() == [-1] and other.tr_cross_partner.tolist() == [-1, -1]
    for ev in (inside, outside, over, other):
        check_sums(ev)


def test_empty_sides(scripted):
    ev = scripted["empty_sides"]
    assert ev.n_frames == 3 and kinds(ev) == ([DB.MISS], [DB.FP])
    assert ev.gt_cross_partner.tolist() == [-1] and ev.tr_cross_partner.tolist() == [-1]       # not in one frame
    assert ev.worst_frames(3) == [(0, 0, 1, 0), (1, 1, 0, 0), (2, 0, 0, 0)]
    none, lone = scripted["no_tracker"], scripted["no_gt"]
    assert kinds(none) == ([DB.MISS, DB.MISS], []) and none.counts()["car"]["CLR_FN"] == 2
    assert kinds(lone) == ([], [DB.FP]) and lone.counts()["truck"]["CLR_FP"] == 1
    for e in (ev, none, lone):
        check_sums(e)


def test_two_classes_swapped_in_one_frame(scripted):
    ev = scripted["swap"]
    assert kinds(ev) == ([DB.MISS, DB.MISS], [DB.FP, DB.FP])
    assert ev.gt_cross_partner.tolist() == [0, 1] and ev.tr_cross_partner.tolist() == [0, 1]
    assert ev.confusion_matrix[C.CAR, C.TRUCK] == 1 and ev.confusion_matrix[C.TRUCK, C.CAR] == 1
    assert ev.confusions() == [("car", "truck", 1), ("truck", "car", 1)]        # a tie: by class order
    assert ev.gt_cross_iou.tolist() == [0.9, 0.8]


def test_every_kind_in_one_sequence(scripted):
    ev = scripted["every_kind"]
    assert ev.gt_kind.tolist() == [DB.MATCH, DB.MATCH, DB.MISS, DB.MATCH, DB.MISS, DB.MISS, DB.SWITCH, DB.MATCH]
    assert ev.tr_kind.tolist() == [DB.TP, DB.TP, DB.FP, DB.TP, DB.FP, DB.IGNORED, DB.SWITCH, DB.TP]
    assert ev.switches() == ev.switches("car") == [(3, 1, 7, 8)] and ev.switches("pedestrian") == []
    assert ev.ignored() == [(2, 5, "rider")] and ev.confusions() == [("car", "bus", 2)]
    assert ev.worst_frames(2) == [(2, 2, 1, 0), (1, 1, 1, 0)]
    assert ev.worst_frames(1, "pedestrian") == [(2, 1, 0, 0)] and ev.worst_frames(1, "car") == [(1, 1, 0, 0)]
    with pytest.raises(ValueError, match="none of"):
        ev.switches("lorry")
    check_sums(ev)


# ------------------------------------------------------------------------------------------------------ the files
def test_the_csv_round_trip_is_exact(tmp_path, scripted):
    for ev in list(C.random_pack()[1].values()) + list(scripted.values()):
        path = str(tmp_path / "events" / (ev.name + ".csv"))
        ev.write_csv(path)
        with open(path) as f:
            assert f.readline().strip() == DB.CSV_HEADER
        C.same_events({ev.name: DB.BDDSequenceEvents.read_csv(path, n_frames=ev.n_frames)}, {ev.name: ev})
    with open(str(tmp_path / "events" / "car_as_truck.csv")) as f:
        assert f.read().splitlines()[1:] == [
            "0,gt,1,car,0.0,0.0,100.0,100.0,MISS,-1,0.0,0,7,truck,0.9",
            "0,tr,7,truck,0.0,0.0,100.0,90.0,FP,-1,0.0,0,1,car,0.9"]
    with pytest.raises(ValueError, match="not a BDD100K events file"):
        (tmp_path / "x.csv").write_text(D.CSV_HEADER + "\n")
        DB.BDDSequenceEvents.read_csv(str(tmp_path / "x.csv"))


def test_sequence_events_draw_unchanged(scripted):
    ev = scripted["every_kind"]
    everything, cars = ev.as_sequence_events(), ev.as_sequence_events("car")
    assert everything.n_frames == cars.n_frames == 4
    assert np.array_equal(everything.gt_kind, ev.gt_kind) and np.array_equal(everything.tr_partner, ev.tr_partner)
    assert np.array_equal(everything.gt_boxes[0], [0.0, 0.0, 100.0, 100.0]) and everything.tr_boxes[0, 3] == 90.0
    total = {k: sum(c[k] for c in ev.counts().values()) for k in DB.COUNTS}
    assert everything.counts() == total and cars.counts() == ev.counts()["car"]
    assert cars.gt_ids.tolist() == [1, 1, 1, 1] and cars.tr_ids.tolist() == [7, 8]
    assert cars.gt_partner.tolist() == [0, -1, -1, 0] and cars.tr_partner.tolist() == [0, 0]
    assert cars.switches() == [(4, 1, 7, 8)]                    # (diagnose.py names frames from 1)
    table = D.error_table_host(everything, 1200, 1200)
    assert table.shape == (4, 3, 16)
    colour = lambda kind: D.COLOURS[kind][0] | D.COLOURS[kind][1] << 8 | D.COLOURS[kind][2] << 16       # noqa: E731
    # frame 2: the two misses, then the false positive; the ignored rider is not drawn
    assert table[2, :, 4].tolist() == [colour(D.MISS), colour(D.MISS), colour(D.FP)]
    assert table[3, :2, 4].tolist() == [colour(D.SWITCH), colour(D.TP)] and table[3, 2, 2] == -1
    pack, events = C.random_pack()
    for name, e in events.items():
        for cls in B.CLASSES:
            assert e.as_sequence_events(cls).counts() == e.counts()[cls], (name, cls)


def test_the_command_line(tmp_path, capsys):
    pack, events = C.random_pack()
    gt_dir, tracker_dir = C.write_tree(str(tmp_path / "tree"), pack)
    got = DB.bdd_events_from_files(gt_dir, tracker_dir)                 # (in the order of the file names)
    assert list(got) == sorted(events)
    C.same_events({name: got[name] for name in events}, events)
    out = str(tmp_path / "report")
    assert DB.main(["--gt-dir", gt_dir, "--tracker-dir", tracker_dir, "--out", out, "--worst", "2"]) == 0
    assert sorted(os.listdir(out)) == sorted([n + ".csv" for n in pack.names] + ["confusion.csv", "summary.txt"])
    text = open(os.path.join(out, "summary.txt")).read().splitlines()
    for name, ev in events.items():
        for cls, counts in ev.counts().items():
            assert f"{name} {cls} " + " ".join(f"{k}={v}" for k, v in counts.items()) in text
        assert sum(line.startswith(f"{name} frame ") for line in text) == 2
        C.same_events({name: DB.BDDSequenceEvents.read_csv(os.path.join(out, name + ".csv"), n_frames=ev.n_frames)},
                      {name: ev})
    total = DB.summed_confusion(events)
    assert f"ignored tracker boxes: {sum(len(ev.ignored()) for ev in events.values())}" in text
    g, t, n = DB._largest_confusions(total, 1)[0]
    assert text[text.index("confusions (ground truth -> tracker)") + 1] == f"  {g} -> {t}: {n}"
    rows = open(os.path.join(out, "confusion.csv")).read().splitlines()
    assert rows[0] == "gt\\tracker," + ",".join(DB.LABELS) and len(rows) == 10
    assert [[int(v) for v in r.split(",")[1:]] for r in rows[1:]] == total.tolist()
    assert len(capsys.readouterr().out.splitlines()) == len(pack.names)


def test_the_evaluator_hands_out_events_and_the_old_modules_still_refuse():
    ev = B.BDD100KEvaluator()
    ev.add_ground_truth("v", 0, [1, 2], [C.GT_BOX, [500.0, 500.0, 560.0, 560.0]], ["car", "other person"])
    ev.add_tracker_rows("v", 0, [7, 8], [C.overlapping(0.9), [505.0, 505.0, 555.0, 555.0]], ["truck", "pedestrian"])
    got = ev.events()["v"]
    assert got.gt_kind.tolist() == [DB.MISS] and got.tr_kind.tolist() == [DB.FP, DB.IGNORED]        # (0-based frames)
    assert got.ignored() == [(0, 8, "pedestrian")] and got.confusions() == [("car", "truck", 1)]
    with pytest.raises(ValueError, match="BDD100K"):
        D._check_benchmark("BDD100K")


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_is_declared_and_the_abi_stays_12(clip_lib):
    declared = assert_binding_matches_header(clip_lib, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert "clipops_bdd_cross_class_f64" in declared
    assert clip_lib.ABI_VERSION == 12 and clip_lib.lib.clipops_abi_version() == 12
    assert DB.CROSS_MAX_DIM == 2048


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib, p = clip_lib.lib, ctypes.c_void_p(64)
    inputs = ("gt_boxes", "tr_boxes", "gt_classes", "tr_classes", "gt_off", "tr_off", "gt_kind", "tr_kind")
    outputs = ("gt_partner", "gt_class", "gt_iou", "tr_partner", "tr_class", "tr_iou", "status")

    def cross(n_frames=2, max_gt=8, max_tr=8, **ptrs):
        a = {k: ptrs.get(k, p) for k in inputs + outputs}
        return lib.clipops_bdd_cross_class_f64(*[a[k] for k in inputs], n_frames, max_gt, max_tr,
                                               *[a[k] for k in outputs], None)

    for kwargs in (dict(n_frames=-1), dict(max_gt=-1), dict(max_tr=-1)):
        assert cross(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
    for kwargs in (dict(max_gt=2049), dict(max_tr=2049)):
        assert cross(**kwargs) == 2 and b"CLIPOPS_EVENTS_MAX_DIM" in lib.clipops_last_error(), kwargs
    for name in inputs + outputs:
        assert cross(**{name: None}) == 1 and b"null" in lib.clipops_last_error(), name
    assert cross(n_frames=0, **{k: None for k in inputs + outputs}) == 0 and lib.clipops_last_error() == b""
