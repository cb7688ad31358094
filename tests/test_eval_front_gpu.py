"""GPU: the device fronts the five device paths share (``evaluation.device_front``,
``evaluation_bdd100k.device_front_bdd``).  Each consumer makes the library calls, in the order and number, it made when
it carried a front of its own (the literals below were read off that code and recorded from it on an MI355X); what
``device_tables`` and ``device_association_tables`` expose of the preprocessed data agrees to the bit; and every
consumer equals its host statement on the shapes the copies had drifted on: no sequence, no frame, nothing kept on one
side, no preprocessing match, and for BDD100K no row of an evaluated class."""
import numpy as np
import pytest
import torch

import association_cases as AC
from track_eval_bdd_helpers import golden as bdd_golden

from memotr_amd import association as A
from memotr_amd import diagnose as D
from memotr_amd import diagnose_bdd100k as DB
from memotr_amd import evaluation as E
from memotr_amd import evaluation_bdd100k as B

pytestmark = pytest.mark.gpu

METRIC_CALLS = [("trackeval_accumulate", 1), ("trackeval_hota_match", 1), ("trackeval_hota_reduce", 1),
                ("trackeval_clear", 1), ("trackeval_identity", 1)]
TABLE_CALLS = {"MOT17": [("trackeval_similarity", 2), ("trackeval_preproc_match", 1)] + METRIC_CALLS,
               "MOT15": [("trackeval_similarity", 2)] + METRIC_CALLS}
BDD_TABLE_CALLS = [("bddeval_class_count", 1), ("bddeval_class_split", 1), ("bddeval_similarity", 2),
                   ("bddeval_preproc", 1)] + METRIC_CALLS
# the launches of their own modules, which is all tools/bench_assoc.py and tools/bench_bdd_events.py read
ASSOCIATION_CALLS = [("clipops_hota_events_f64", 1), ("clipops_identity_pairs_i32", 1), ("clipops_assoc_reduce_f64", 1)]
BDD_EVENT_CALLS = [("clipops_clear_events_f64", 1), ("clipops_bdd_cross_class_f64", 1)]


@pytest.fixture(scope="module")
def libs(clip_lib):
    from memotr_amd.build import build_track_eval_bdd_lib, build_track_eval_lib
    build_track_eval_lib(), build_track_eval_bdd_lib()
    return clip_lib


def calls(timings):
    """(name, number of calls) in the order of each name's first call; every entry a pair of events."""
    assert all(isinstance(a, torch.cuda.Event) and isinstance(b, torch.cuda.Event) for v in timings.values() for a, b in v)
    return [(name, len(pairs)) for name, pairs in timings.items()]


def host_of(tables):
    return {k: v.cpu().numpy() for k, v in tables.items()}


# ------------------------------------------------------------------------------------------- the launch sequences
@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_the_mot_consumers_make_the_calls_they_made_alone(libs, prefix):
    benchmark, packed = AC.SETS[prefix], AC.golden(prefix)[1].to("cuda")
    t_tables, t_assoc = {}, {}
    tables = E.device_tables(packed, benchmark, timings=t_tables)
    assoc = A.device_association_tables(packed, benchmark, timings=t_assoc)
    rows = D._device_rows(packed, benchmark)
    assert calls(t_tables) == TABLE_CALLS[benchmark]
    assert calls(t_assoc) == ASSOCIATION_CALLS
    # the three stand on one front: what they expose of the preprocessed data is the same bytes
    assert torch.equal(assoc["matches"], tables["matches"]) and int(tables["matches"].sum()) > 0
    gt_off, tr_off, sim = (tables[k].cpu().numpy() for k in ("gt_off", "tr_off", "similarity"))
    sim_off = E._sim_offsets(gt_off, tr_off)
    assert len(sim) == sim_off[-1]
    host = assoc["host"]
    assert np.array_equal(host["gid_off"], np.concatenate(([0], np.cumsum(tables["n_gt_ids"].cpu().numpy()))))
    assert np.array_equal(host["tid_off"], np.concatenate(([0], np.cumsum(tables["n_tr_ids"].cpu().numpy()))))
    seq_off = packed.seq_off.cpu().numpy()
    for side, off, n_ids in (("gt", gt_off, host["gid_off"]), ("tr", tr_off, host["tid_off"])):
        ids, count = tables[side + "_ids"].cpu().numpy(), assoc[side + "_count"].cpu().numpy()
        assert len(assoc["c::" + side + "_partner"]) == len(ids) == off[-1]
        for s in range(len(seq_off) - 1):               # the relabelled ids behind the compact offsets, counted
            mine = ids[off[seq_off[s]]:off[seq_off[s + 1]]]
            assert np.array_equal(np.bincount(mine, minlength=n_ids[s + 1] - n_ids[s]), count[n_ids[s]:n_ids[s + 1]])
    partner = assoc["c::gt_partner"].cpu().numpy()      # a matched row's iou is its entry of the similarity
    frame = np.repeat(np.arange(len(gt_off) - 1), np.diff(gt_off))
    hit = np.flatnonzero(partner >= 0)
    entry = sim_off[frame[hit]] + (hit - gt_off[frame[hit]]) * np.diff(tr_off)[frame[hit]] + partner[hit]
    iou = assoc["gt_iou"].cpu().numpy()
    assert len(hit) > 0 and np.array_equal(sim[entry], iou[assoc["gt_level"].cpu().numpy() > 0])     # (rows keep their order)
    assert torch.equal(rows["counts"][:, :4].long(), tables["clear_ints"][:, :4])       # CLR_TP, CLR_FN, CLR_FP, IDSW
    live = (tables["n_gt_dets"] > 0) & (tables["n_tr_dets"] > 0)
    assert torch.equal(rows["counts"][live, 4].long(), tables["clear_ints"][live, 7])    # Frag


def test_the_bdd_consumers_make_the_calls_they_made_alone(libs):
    packed = bdd_golden()[1].to("cuda")
    t_tables, t_rows = {}, {}
    tables = B.device_tables_bdd(packed, timings=t_tables)
    rows = DB._device_rows(packed, timings=t_rows)
    assert calls(t_tables) == BDD_TABLE_CALLS
    assert calls(t_rows) == BDD_EVENT_CALLS
    counts = rows["counts"].reshape(-1, 5).long()
    assert torch.equal(counts[:, :4], tables["clear_ints"][:, :4]) and int(counts[:, 0].sum()) > 0
    live = (tables["n_gt_dets"] > 0) & (tables["n_tr_dets"] > 0)
    assert torch.equal(counts[live, 4], tables["clear_ints"][live, 7])


# --------------------------------------------------------------------------------------------- degenerate shapes
BOXES = [[0.0, 0.0, 10.0, 10.0], [100.0, 0.0, 10.0, 10.0], [200.0, 0.0, 10.0, 10.0]]
ids = lambda *v: np.array(v, np.int64)                                                      # noqa: E731
boxes = lambda *v: np.array([BOXES[i] for i in v], np.float64).reshape(-1, 4)                # noqa: E731


def three_frames(gt_class):
    """Two ground-truth ids of one class over three frames, three tracker ids on and beside them."""
    gt, tr = [(1, 2), (1, 2), (2,)], [(7, 8, 9), (7,), (8, 7)]
    where = {1: 0, 2: 1, 7: 0, 8: 1, 9: 2}
    return {"s": {"gt_ids": [ids(*f) for f in gt], "gt_boxes": [boxes(*[where[i] for i in f]) for f in gt],
                  "gt_classes": [np.full(len(f), gt_class) for f in gt],
                  "tracker_ids": [ids(*f) for f in tr], "tracker_boxes": [boxes(*[where[i] for i in f]) for f in tr]}}


MOT_CASES = {
    "no_sequence": ({}, "MOT17"),
    "no_frame": ({"s": {k: [] for k in ("gt_ids", "gt_boxes", "tracker_ids", "tracker_boxes")}}, "MOT17"),
    "no_pedestrian": (three_frames(8), "MOT17"),        # all ground truth is a distractor: nothing kept on its side
    "mot15": (three_frames(8), "MOT15"),                # no preprocessing match, no class filter
}
# a per-sequence float sum of these cases has at most 6 non-negative terms (2 x 3 id pairs, 5 matched rows), none above
# 3 (three frames): two summation orders of them are at most (n - 1) * 2**-52 * sum apart
SUM_BAR = 5 * 2.0 ** -52 * 18


@pytest.mark.parametrize("case", sorted(MOT_CASES))
def test_the_mot_consumers_equal_their_host_statements_on_degenerate_packs(libs, case):
    sequences, benchmark = MOT_CASES[case]
    packed = E.pack_sequences(sequences)
    dev = packed.to("cuda")
    # evaluation
    want, got = E.host_tables(packed, benchmark), host_of(E.device_tables(dev, benchmark))
    live = (want["n_gt_dets"] > 0) & (want["n_tr_dets"] > 0)        # (the host statement does not walk the others)
    assert list(live) == {"no_sequence": [], "no_frame": [False], "no_pedestrian": [False], "mot15": [True]}[case]
    for k in ("raw_similarity", "similarity", "gt_off", "tr_off", "gt_ids", "tr_ids", "n_gt_ids", "n_tr_ids",
              "n_gt_dets", "n_tr_dets"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in ("hota_tp", "clear_ints", "identity", "hota_sums", "motp_sum"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        bar = SUM_BAR if k in ("hota_sums", "motp_sum") else 0
        assert np.all(np.abs(got[k][live] - want[k][live]) <= bar), k
    if not packed.names:
        for device in ("cpu", "cuda"):
            with pytest.raises(ValueError, match="no sequence to evaluate"):
                E.evaluate_packed(packed, benchmark, device=device)
    else:
        a, b = E.evaluate_packed(dev, benchmark, device="cuda"), E.evaluate_packed(packed, benchmark)
        assert list(a) == list(b) == ["s", "COMBINED_SEQ"]
        for name in a:
            for k in a[name]:
                diff = np.max(np.abs(np.asarray(a[name][k], np.float64) - np.asarray(b[name][k], np.float64)))
                assert diff <= (0 if k in E.INT_FIELDS + E.HOTA_INT_ARRAYS else SUM_BAR), (name, k, diff)
    # CLEAR events
    want, got = D.clear_events_host(packed, benchmark), host_of(D._device_rows(dev, benchmark))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    # association
    want, got = A.association_host(packed, benchmark), A.device_association_tables(dev, benchmark)
    got = dict(host_of({k: v for k, v in got.items() if k != "host"}), **got["host"])
    assert set(got) >= set(want)
    assert len(got["frame_status"]) == len(packed.gt_off) - 1 and len(got["id_status"]) == len(packed.names)
    A.raise_on_status(got["frame_status"], got["id_status"])
    for k in AC.int_keys(want) + ["gt_iou", "tr_iou"]:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in AC.NUM_KEYS:
        assert got[k].shape == want[k].shape and np.all(np.abs(got[k] - want[k]) <= SUM_BAR), k
    if packed.names:
        a, b = A.association(dev, benchmark, device="cuda")["s"], A.association(packed, benchmark)["s"]
        assert a.totals()["IDTP"] == b.totals()["IDTP"] == (4 if case == "mot15" else 0)


def bdd_outside():
    """One frame whose only rows are of classes outside the eight (3: other person, 9: other vehicle)."""
    return {"s": {"gt_ids": [ids(1)], "gt_boxes": [boxes(0)], "gt_classes": [ids(3)], "tracker_ids": [ids(5)],
                  "tracker_boxes": [boxes(0)], "tracker_classes": [ids(9)]}}


@pytest.mark.parametrize("case", ["no_sequence", "outside"])
def test_the_bdd_consumers_equal_their_host_statements_on_degenerate_packs(libs, case):
    packed = B.pack_bdd({} if case == "no_sequence" else bdd_outside())
    dev = packed.to("cuda")
    want, got = B.host_tables_bdd(packed), host_of(B.device_tables_bdd(dev))
    assert set(got) >= set(want) and len(want["hota_tp"]) == len(packed.names) * B.N_CLASSES
    assert not want["n_gt_dets"].any() and not want["n_tr_dets"].any()      # (no pair is walked: the rest is shapes)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    for k in ("raw_similarity", "similarity") + B.TABLE_KEYS:
        assert np.array_equal(got[k], want[k]), k
    if packed.names:
        B_a, B_b = B.evaluate_packed_bdd(dev, device="cuda"), B.evaluate_packed_bdd(packed)
        assert list(B_a) == list(B_b)
        for name in B_a:
            for cls in B_a[name]:
                for k, v in B_a[name][cls].items():
                    assert np.array_equal(np.asarray(v, np.float64), np.asarray(B_b[name][cls][k], np.float64)), (cls, k)
    else:
        for device in ("cpu", "cuda"):
            with pytest.raises(ValueError, match="no sequence to evaluate"):
                B.evaluate_packed_bdd(packed, device=device)
    want, got = DB.bdd_events_host(packed), host_of(DB._device_rows(dev))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    if packed.names:
        assert list(got["gt_kind"]) == list(got["tr_kind"]) == [DB.IGNORED]
